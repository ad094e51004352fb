// CTC prefix beam search on the head's logits alone (avsr_ctc_prefix_search, include/avsr_hip.h; the rule is INTEGRATION.md section 8).
// The search itself -- the frame, its phases 1-5, the LDS layout, the outputs -- is csrc/ctc_prefix_search.h's cp_search, shared with the
// language-model forms (csrc/ctc_prefix_lm.hip, csrc/ctc_prefix_ngram.hip).  This file is its instantiation without a model, the plain
// kernel's limits and its entry points.
#include "ctc_prefix_search.h"

namespace avsr {

// dynamic LDS: cp_lds_words(V, W, L_max) words
__global__ __launch_bounds__(256) void ctc_prefix_kernel(const avsr_ctc_prefix_args A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cp_smem[];
  cp_no_model none;
  cp_search(A, cp_terms{}, none, cp_smem);
}

// AVSR_OK, or why the shape cannot run (the LDS bound holds at the three maxima: 137 KiB)
static int ctc_prefix_limits(int V, int W, int LM) { return cp_limits(V, W, LM, AVSR_CTC_PREFIX_MAX_W); }

}  // namespace avsr

extern "C" int avsr_ctc_prefix_search_supported(int32_t V, int32_t beam_width, int32_t L_max) {
  return avsr::ctc_prefix_limits(V, beam_width, L_max) == AVSR_OK ? 1 : 0;
}

extern "C" int avsr_ctc_prefix_search(const avsr_ctc_prefix_args* a, void* stream) {
  using namespace avsr;
  int rc = cp_check_args(a);
  if (!rc) rc = ctc_prefix_limits(a->V, a->beam_width, a->L_max);
  if (rc) return rc;
  return cp_launch<ctc_prefix_kernel>(sizeof(uint32_t) * cp_lds_words(a->V, a->beam_width, a->L_max), stream, *a);
}

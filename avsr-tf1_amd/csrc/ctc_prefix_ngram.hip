// CTC prefix beam search with a back-off n-gram fused into the frame loop (avsr_ctc_prefix_search_ngram, include/avsr_hip.h; the rule is
// INTEGRATION.md section 8): the search of csrc/ctc_prefix_search.h (cp_search: ONE launch per batch, one 256-thread workgroup per
// utterance, the beam in LDS, fp32, no atomics, two launches bit-identical) with lam(. | g) read from a device-resident back-off
// automaton.  This file is the model's side only: the walk, the Step object the search calls, the limits and the launch.
//
// State placement.  Per label sequence the model holds ONE int32: the node of the longest suffix of (GO, g) that is a context of the
// model.  It lives in LDS behind the search's own words, [2 W rows], addressed by the same per-slot row index as the lam rows (a stay
// inherits its parent's row, an extension takes a row no old slot references, so no step reads a node that the same step writes).
// No workspace, no global-memory state: the only global traffic of a step is the read-only tables.
//
// Phase 6 for the M <= 16 kept extensions of a frame (skipped by the search's workgroup-uniform branch when M = 0):
//   a. thread m < M:  node[new_m] = next[arc], arc = the arc the walk for (node[parent_m], tok_m) ends on        (prologue: node[0] = start)
//   b. M * V independent walks over the 256 threads: lam[new_m][c] = walk(node[new_m], c)
// The walk itself (ngram_node / ngram_find / ngram_walk: the bounded, clamped chain of dependent L2 reads) is csrc/ngram_walk.h, shared with
// beam search's n-gram step (csrc/beam_ngram.hip).
#include "ctc_prefix_search.h"
#include "ngram_walk.h"

namespace avsr {

// the n-gram as cp_search's Step: one node id per pool row in LDS
struct cpn_step {
  const ngram_view G;
  const int V, start;
  int* sNode;                                                              // [2 W]
  static size_t extra(int W) { return 2 * (size_t)W; }
  __device__ __forceinline__ void init(int, int, uint32_t* words) { sNode = reinterpret_cast<int*>(words); }
  __device__ __forceinline__ void prologue(int) {}
  __device__ __forceinline__ void step(int M, const int* sTok, const int* sPar, const int* sNew, float* sLam, bool first) {
    const int tid = threadIdx.x;
    if (tid < M) {
      int node = ngram_node(G, start);
      if (!first) {
        int arc;
        ngram_walk(G, ngram_node(G, sNode[sPar[tid]]), sTok[tid], arc);
        node = ngram_node(G, G.next[arc]);
      }
      sNode[sNew[tid]] = node;
    }
    lds_barrier();
    for (int e = tid; e < M * V; e += 256) {
      const int m = e / V, c = e - m * V, nw = sNew[m];
      int arc;
      sLam[nw * V + c] = ngram_walk(G, sNode[nw], c, arc);
    }
    lds_barrier();
  }
};

// dynamic LDS: cp_lds_words(V, W, L_max, true, 2 W) words
__global__ __launch_bounds__(256) void ctc_prefix_ngram_kernel(const avsr_ctc_prefix_args A, const avsr_ctc_prefix_ngram G) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cpn_smem[];
  cpn_step step{ngram_view_of(G), G.V, G.start, nullptr};
  const cp_terms terms{G.weight, G.bonus, G.go_id, G.eos_id, G.s_lm, G.lm_steps, G.lm_logp};
  cp_search(A, terms, step, cpn_smem);
}

// AVSR_OK, or why the shape cannot run (decided on the host, nothing dereferenced)
static int ctc_prefix_ngram_limits(int V, int W, int LM, int n_nodes, int n_arcs) {
  const bool bad = n_nodes < 1 || n_arcs < V;
  const bool big = n_nodes > AVSR_CTC_PREFIX_NGRAM_MAX_NODES || n_arcs > AVSR_CTC_PREFIX_NGRAM_MAX_ARCS;
  return cp_limits(V, W, LM, AVSR_CTC_PREFIX_LM_MAX_W, true, cpn_step::extra(W), bad, big);        // (LDS at the three maxima: 70 KiB)
}

}  // namespace avsr

extern "C" int avsr_ctc_prefix_ngram_supported(int32_t V, int32_t beam_width, int32_t L_max, int32_t n_nodes, int32_t n_arcs) {
  return avsr::ctc_prefix_ngram_limits(V, beam_width, L_max, n_nodes, n_arcs) == AVSR_OK ? 1 : 0;
}

extern "C" int avsr_ctc_prefix_search_ngram(const avsr_ctc_prefix_args* a, const avsr_ctc_prefix_ngram* ng, void* stream) {
  using namespace avsr;
  if (!ng) return AVSR_ERR_ARG;
  int rc = cp_check_args(a);
  if (!rc) rc = cp_check_terms(a->V, ng->V, ng->go_id, ng->eos_id, ng->weight, ng->bonus);
  if (!rc) rc = ctc_prefix_ngram_limits(a->V, a->beam_width, a->L_max, ng->n_nodes, ng->n_arcs);
  if (rc) return rc;
  if (ng->start < 0 || ng->start >= ng->n_nodes) return AVSR_ERR_ARG;
  if (!ng->bow || !ng->backoff || !ng->arc_begin || !ng->sym || !ng->logp || !ng->next || !ng->s_lm || !ng->lm_steps) return AVSR_ERR_ARG;
  const size_t lds = sizeof(uint32_t) * cp_lds_words(a->V, a->beam_width, a->L_max, true, cpn_step::extra(a->beam_width));
  return cp_launch<ctc_prefix_ngram_kernel>(lds, stream, *a, *ng);
}

// Shallow fusion of a WORD-level back-off n-gram into beam search through a lexicon trie (avsr_beam_word_ngram, include/avsr_hip.h; the
// rule is INTEGRATION.md section 8, the table under ctc_word_ngram_lm): one launch per decode step over the R = B * K hypothesis rows,
// queued where the LSTM's and the unit n-gram's steps are queued (attn_rnn.hip, K0), writing the [R][V] term lm_logp[r][c] =
// lam(c | labels of row r) that the selection (or the CTC step's pre-combination) reads.  The model's side -- trie search, transition,
// close / hc / eos, the per-class value -- is csrc/word_ngram_walk.h, the one copy the CTC prefix search's word step uses.
//
// State.  Per row THREE int32 in a ping-pong state[2][3][R]: h (the automaton node of the closed words), p (the trie node of the open
// word; 0 = root, -1 = OOV) and hc (the node a space would leave; h at the root), so that a space reads its parent's cached value and
// EOS needs one walk from it.  The selection permutes rows and another workgroup may own the parent's row, so step s reads half s & 1
// at parent_rows[r] and writes half (s + 1) & 1 at r.  Step 0 puts every row at (start, root, start) and reads neither tok nor the
// stale half.
//
// Mapping.  As in beam_ngram.hip nothing here is bound by arithmetic or bandwidth, only by chains of dependent L2 reads, so the launch
// is spread wide instead of deep: BWN_ROWS = 4 rows per 256-thread workgroup (160 workgroups at R = 640).  Threads 0 .. 3 do the
// group's transitions, one each -- at most one trie search or one walk -- and then close, hc and eos of the new state (at most two
// dependent walks); they leave p, close and eos in LDS and (h, p, hc) in the other half.  After one barrier the threads take the values
// e = tid, tid + 256, ... of the group's [rows][V]: a letter costs one binary search among the children of p; space, EOS and the
// non-units come from the row's scalars.  A row whose tok is EOS transitions like any other; its values are not read.
// Plain loads, vector stores, no atomics: two launches on the same inputs are bit-identical.  Every node id, word id, trie node, arc
// range, tok and parent_rows value read from memory is clamped into its table or range before it is used as an index -- a stale h or
// hc into [0, n_nodes) (else 0), a stale p into [-1, n_trie_nodes) (else the root) -- so stale or foreign inputs address nothing outside
// the buffers.  All loops are bounded.
#include <math.h>
#include "beam.h"
#include "word_ngram_walk.h"
#include "prof.h"

namespace avsr {

constexpr int BWN_ROWS = 4;

__global__ __launch_bounds__(256) void beam_word_ngram_step_kernel(const word_model M, int R, const int32_t* tok,
                                                                    const int32_t* parent_rows, const int32_t* st_in, int32_t* st_out,
                                                                    float* lm_logp, int first) {
  __shared__ int sP[BWN_ROWS];
  __shared__ float sClose[BWN_ROWS], sEos[BWN_ROWS];
  const int tid = threadIdx.x, r0 = blockIdx.x * BWN_ROWS, V = M.V;
  const int nr = min(BWN_ROWS, R - r0);
  if (tid < nr) {
    const int r = r0 + tid;
    int h = ngram_node(M.G, M.start), p = 0;
    if (!first) {
      int par = parent_rows[r], t = tok[r];
      par = (unsigned)par < (unsigned)R ? par : 0;
      t = (unsigned)t < (unsigned)V ? t : 0;
      h = ngram_node(M.G, st_in[par]);
      p = st_in[R + par];
      p = (p >= WN_OOV && p < M.T.n_nodes) ? p : 0;
      M.advance(h, p, ngram_node(M.G, st_in[2 * R + par]), t);
    }
    float cl, eos;
    int hc;
    M.scalars(h, p, cl, hc, eos);
    st_out[r] = h; st_out[R + r] = p; st_out[2 * R + r] = hc;
    sP[tid] = p; sClose[tid] = cl; sEos[tid] = eos;
  }
  __syncthreads();
  for (int e = tid; e < nr * V; e += 256) {
    const int m = e / V, c = e - m * V;
    lm_logp[(long)(r0 + m) * V + c] = M.value(sP[m], c, sClose[m], sEos[m]);
  }
}

// AVSR_OK, or why the step cannot run (decided on the host, nothing dereferenced)
int beam_word_ngram_check(const avsr_beam_word_ngram* g) {
  if (!g || g->n_nodes < 1 || g->Vw < 2 || g->n_arcs < g->Vw || g->n_trie_nodes < 1 || g->n_trie_arcs < 1 || g->V < 2 || g->n_rows < 1)
    return AVSR_ERR_ARG;
  if (g->start < 0 || g->start >= g->n_nodes || g->eos_w < 0 || g->eos_w >= g->Vw || g->unk_id < -1 || g->unk_id >= g->Vw)
    return AVSR_ERR_ARG;
  if (g->go_id < 0 || g->go_id >= g->V || g->eos_id < 0 || g->eos_id >= g->V || g->space_id < 0 || g->space_id >= g->V ||
      g->space_id == g->go_id || g->space_id == g->eos_id || g->go_id == g->eos_id)
    return AVSR_ERR_ARG;
  if (!(g->oov <= 0.f) || g->oov == -INFINITY) return AVSR_ERR_ARG;
  if (!(g->lm_weight >= 0.f) || isinf(g->lm_weight)) return AVSR_ERR_ARG;
  if (g->n_nodes > AVSR_CTC_PREFIX_NGRAM_MAX_NODES || g->n_arcs > AVSR_CTC_PREFIX_NGRAM_MAX_ARCS ||
      g->n_trie_nodes > AVSR_CTC_PREFIX_NGRAM_MAX_NODES || g->n_trie_arcs > AVSR_CTC_PREFIX_NGRAM_MAX_ARCS)
    return AVSR_ERR_UNSUPPORTED;
  if ((long)g->n_rows * g->V >= (1L << 31) || (long)g->n_rows * 6 >= (1L << 31)) return AVSR_ERR_UNSUPPORTED;
  if (!g->bow || !g->backoff || !g->arc_begin || !g->sym || !g->logp || !g->next || !g->t_begin || !g->t_sym || !g->t_next || !g->t_word ||
      !g->state || !g->lm_logp)
    return AVSR_ERR_ARG;
  return AVSR_OK;
}

int beam_word_ngram_step_launch(const avsr_beam_word_ngram& g, const int32_t* tok, const int32_t* parent_rows, int step, hipStream_t s) {
  const int R = g.n_rows;
  ProfScope ps(PROF_STEP_LINEAR, s);                // the term of a step, booked where the LSTM's output layer is
  hipLaunchKernelGGL(beam_word_ngram_step_kernel, dim3((R + BWN_ROWS - 1) / BWN_ROWS), dim3(256), 0, s, word_model_of(g), R, tok,
                     parent_rows, g.state + (long)(step & 1) * 3 * R, g.state + (long)((step + 1) & 1) * 3 * R, g.lm_logp,
                     step == 0 ? 1 : 0);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

}  // namespace avsr

extern "C" int avsr_beam_word_ngram_supported(const avsr_beam_word_ngram* wn) { return avsr::beam_word_ngram_check(wn) == AVSR_OK ? 1 : 0; }

extern "C" int avsr_beam_word_ngram_step(const avsr_beam_word_ngram* wn, const int32_t* tok, const int32_t* parent_rows, int32_t n_rows,
                                         int32_t step, void* stream) {
  if (!wn || !tok || !parent_rows || n_rows <= 0 || step < 0) return AVSR_ERR_ARG;
  const int rc = avsr::beam_word_ngram_check(wn);
  if (rc) return rc;
  if (n_rows != wn->n_rows) return AVSR_ERR_ARG;
  return avsr::beam_word_ngram_step_launch(*wn, tok, parent_rows, step, (hipStream_t)stream);
}

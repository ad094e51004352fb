// Shallow fusion of a back-off n-gram into beam search (avsr_beam_ngram, include/avsr_hip.h; the rule is INTEGRATION.md section 8): one
// launch per decode step over the R = B * K hypothesis rows, queued where the LSTM's step is queued (attn_rnn.hip, K0), writing the
// [R][V] term lm_logp[r][c] = lam(c | GO, labels of row r) that the selection (or the CTC step's pre-combination) reads.
//
// State.  Per row ONE int32: the node of the longest suffix of (GO, labels) that is a context of the model, in a ping-pong node[2][R].
// The selection permutes rows and another workgroup may own the parent's row, so step s reads node[s & 1][parent_rows[r]] and writes
// node[(s + 1) & 1][r] -- the two halves of avsr_beam_lm's state.  Step 0 starts every row at `start` (tok is GO then) and reads neither
// tok nor the stale half.
//
// Mapping.  The R * V values are independent walks (csrc/ngram_walk.h: chains of dependent L2 reads, a few hundred bytes of tables each),
// and a row's transition is one more walk that all V of them wait for.  Nothing here is bound by arithmetic or bandwidth, only by the
// length of that chain, so the launch is spread wide instead of deep: BN_ROWS = 4 rows per 256-thread workgroup (160 workgroups at
// R = 640, under one per CU; at V = 31 every walk of a row group has a thread of its own, wider vocabularies loop).  Threads 0 .. 3
// walk the group's transitions, one each, and leave the nodes in LDS and in the other half; after one barrier the threads take the
// values e = tid, tid + 256, ... of the group's [rows][V].  A row whose tok is EOS transitions like any other; its values are not read.
// Plain loads, vector stores, no atomics: two launches on the same inputs are bit-identical.  Every node id, arc range, tok and
// parent_rows value is clamped into its table, so stale or foreign inputs address nothing outside the buffers.
#include <math.h>
#include "beam.h"
#include "ngram_walk.h"
#include "prof.h"

namespace avsr {

constexpr int BN_ROWS = 4;

__global__ __launch_bounds__(256) void beam_ngram_step_kernel(const ngram_view G, int V, int start, int R, const int32_t* tok,
                                                               const int32_t* parent_rows, const int32_t* node_in, int32_t* node_out,
                                                               float* lm_logp, int first) {
  __shared__ int sNode[BN_ROWS];
  const int tid = threadIdx.x, r0 = blockIdx.x * BN_ROWS;
  const int nr = min(BN_ROWS, R - r0);
  if (tid < nr) {
    const int r = r0 + tid;
    int node = ngram_node(G, start);
    if (!first) {
      const int p = parent_rows[r], t = tok[r];
      int arc;
      ngram_walk(G, ngram_node(G, node_in[(unsigned)p < (unsigned)R ? p : 0]), (unsigned)t < (unsigned)V ? t : 0, arc);
      node = ngram_node(G, G.next[arc]);
    }
    sNode[tid] = node;
    node_out[r] = node;
  }
  __syncthreads();
  for (int e = tid; e < nr * V; e += 256) {
    const int m = e / V, c = e - m * V;
    int arc;
    lm_logp[(long)(r0 + m) * V + c] = ngram_walk(G, sNode[m], c, arc);
  }
}

// AVSR_OK, or why the step cannot run (decided on the host, nothing dereferenced)
int beam_ngram_check(const avsr_beam_ngram* g) {
  if (!g || g->n_nodes < 1 || g->V < 2 || g->n_arcs < g->V || g->n_rows < 1) return AVSR_ERR_ARG;
  if (g->start < 0 || g->start >= g->n_nodes) return AVSR_ERR_ARG;
  if (!(g->lm_weight >= 0.f) || isinf(g->lm_weight)) return AVSR_ERR_ARG;
  if (g->n_nodes > AVSR_CTC_PREFIX_NGRAM_MAX_NODES || g->n_arcs > AVSR_CTC_PREFIX_NGRAM_MAX_ARCS) return AVSR_ERR_UNSUPPORTED;
  if ((long)g->n_rows * g->V >= (1L << 31)) return AVSR_ERR_UNSUPPORTED;
  if (!g->bow || !g->backoff || !g->arc_begin || !g->sym || !g->logp || !g->next || !g->node || !g->lm_logp) return AVSR_ERR_ARG;
  return AVSR_OK;
}

int beam_ngram_step_launch(const avsr_beam_ngram& g, const int32_t* tok, const int32_t* parent_rows, int step, hipStream_t s) {
  const int R = g.n_rows;
  ProfScope ps(PROF_STEP_LINEAR, s);                // the term of a step, booked where the LSTM's output layer is
  hipLaunchKernelGGL(beam_ngram_step_kernel, dim3((R + BN_ROWS - 1) / BN_ROWS), dim3(256), 0, s, ngram_view_of(g), g.V, g.start, R, tok,
                     parent_rows, g.node + (long)(step & 1) * R, g.node + (long)((step + 1) & 1) * R, g.lm_logp, step == 0 ? 1 : 0);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

}  // namespace avsr

extern "C" int avsr_beam_ngram_supported(const avsr_beam_ngram* ng) { return avsr::beam_ngram_check(ng) == AVSR_OK ? 1 : 0; }

extern "C" int avsr_beam_ngram_step(const avsr_beam_ngram* ng, const int32_t* tok, const int32_t* parent_rows, int32_t n_rows, int32_t step,
                                    void* stream) {
  if (!ng || !tok || !parent_rows || n_rows <= 0 || step < 0) return AVSR_ERR_ARG;
  const int rc = avsr::beam_ngram_check(ng);
  if (rc) return rc;
  if (n_rows != ng->n_rows) return AVSR_ERR_ARG;
  return avsr::beam_ngram_step_launch(*ng, tok, parent_rows, step, (hipStream_t)stream);
}

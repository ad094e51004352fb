// CTC prefix beam search with a language model fused into the frame loop (avsr_ctc_prefix_search_lm, include/avsr_hip.h; the rule is
// INTEGRATION.md section 8): ctc_prefix_search.h's search -- ONE launch per batch, one 256-thread workgroup per utterance, the beam in LDS,
// fp32, no atomics, two launches bit-identical -- whose extensions also carry  w * lam(c | g) + beta,  lam = log_softmax of avsr.LM's
// evaluate graph after GO, g.  The LM's LSTM step runs INSIDE the workgroup's frame loop, and only on the frames that keep an extension.
//
// State placement.  Per label sequence the LM holds (c, h) per layer and the row lam(. | g) [V]:
//   (c, h)  in the caller's workspace, [B][2 W rows][layers][H] each (global memory, L2-resident: far too big for LDS at H = 256);
//   lam     in LDS, [2 W rows][V].
// Both are addressed through a per-slot ROW INDEX into the pool of 2 W rows: a stay inherits its parent's row (an old slot stays at most
// once), an extension takes a row that no OLD slot references -- at most W old plus W new rows are in use, so 2 W always suffice, the
// selection order may permute the stays freely, nothing is ever copied, and no step reads a row that the same step writes.
//
// The search itself -- phases 1-5 of a frame, the pool rows, the epilogue -- is csrc/ctc_prefix_search.h's cp_search, shared with the
// plain and the n-gram form (csrc/ctc_prefix.hip, csrc/ctc_prefix_ngram.hip); this file holds the LSTM step it calls, the limits and the
// entry points.  Phase 5 lists the kept extensions (M <= W <= 16: ONE 16-row tile).  Phase 6, skipped by a workgroup-uniform branch when
// M = 0:
//   per layer   z = W_j . [emb[c] | h_prev(parent row)]  as v_mfma_f32_16x16x4_f32 with the WEIGHTS as the A operand (16 gate columns of
//               the unit-interleaved layout = 4 whole units) and the slots as the B operand: lane (i16, g) ends with the four gates of
//               unit 4 tile + g for slot i16 in its accumulator, so bias, gates, clip and the (c, h) update finish in registers.  The four
//               waves split the H / 4 tiles, two per round (they share the B operand); operands are read from L2 / L1 with the 16-byte pairing
//               of beam_lm_out_kernel (cpl_dot below).
//   then        Dense(V) on the top h the same way into the slot's lam row, and a log-softmax per row by 16 lanes.
// Barriers: lds_barrier() orders LDS only.  The hand-over of h between layers and of the new state to later frames goes through global
// memory, so those barriers are __syncthreads() (vmcnt(0) + barrier: stores drained before, loads issued after; the waves of a workgroup
// share one L1, which a workgroup-scope fence keeps coherent).
// Prologue: one step from a zeroed row on GO for slot 0.  Epilogue: final = p + w * lam(EOS | g), the <= W entries re-sorted by final
// (descending, ties to the earlier slot), s_lm, lm_steps, and the optional lam rows of the final entries.
#include "ctc_prefix_search.h"

namespace avsr {

__device__ __forceinline__ const float* cpl_pick(const float* const p[AVSR_MAX_LM_LAYERS], int j) {
  return j == 0 ? p[0] : (j == 1 ? p[1] : (j == 2 ? p[2] : p[3]));       // (no dynamic index into the kernel's arguments)
}

// acc[t] += W_t . [x0 | x1] for NT 16-row weight tiles that share the B operand: weight row i16 of tile t starts at w[t] and holds
// K0 + K1 contiguous columns, the first K0 meet x0 and the rest x1 (lane (i16, g): inputs 16 ch + 4 g .. + 3 of chunk ch, of weight row
// i16 and of slot i16 -- the pairing of beam_lm_out_kernel; K0 % 4 == 0, so a 16-byte piece lies in one segment).  The chunks run through
// a ring of CPL_U register buffers: a buffer is refilled as soon as its products are issued, so CPL_U - 1 chunks of loads are always in
// flight under the MFMAs (one wave per SIMD is all the occupancy this kernel has).  Nothing in the loop branches (the wait-count pass
// waits for everything at a join between a load and its use): a piece past K0 + K1 reads offset 0 and is zeroed where it is used, never
// where it is loaded.  Measured (tools/ctc_prefix_lm_cost.py, 16 to 512 units): the step's time grows with the weight BYTES at about
// 10 bytes per clock and CU whatever the depth of this ring.  The likely cause (no counters were read): adjacent lanes hold adjacent
// weight ROWS, so a wave's 16-byte loads touch 16 cache lines and are not coalesced.  Not built: staging the tiles through LDS (or a 4 x 4 transpose inside lane quads) so
// that four adjacent lanes read 64 contiguous bytes.  Slots >= M read slot 0's row: a column of the
// product depends on its own slot alone, and theirs is not stored.
#define CPL_U 8
template <int NT>
__device__ __forceinline__ void cpl_dot(const float* const (&w)[NT], int K0, const float* x0, int K1, const float* x1, int g,
                                        f32x4 (&acc)[NT]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int Kt = K0 + K1, n = (Kt + 15) >> 4;
  const float* x1s = x1 - K0;                                              // (only ever dereferenced at offsets >= K0)
  f32x4 a[NT][CPL_U], xv[CPL_U];
  auto load = [&](int ch, int u) {                                         // (u is a constant after unrolling)
    const int k = 16 * ch + 4 * g, ko = k < Kt ? k : 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) a[t][u] = ld4(w[t] + ko);
    xv[u] = ld4((ko < K0 ? x0 : x1s) + ko);
  };
#pragma unroll
  for (int u = 0; u < CPL_U; ++u) load(u, u);
  __builtin_amdgcn_sched_barrier(0);
  for (int base = 0; base < n; base += CPL_U) {
#pragma unroll
    for (int u = 0; u < CPL_U; ++u) {
      const int ch = base + u;
      const f32x4 xx = 16 * ch + 4 * g < Kt ? xv[u] : zero;
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][u][e], xx[e], acc[t], 0, 0, 0);
      load(ch + CPL_U, u);
      __builtin_amdgcn_sched_barrier(0);                                   // keep the refill here: the scheduler would sink it to its use
    }
  }
}

// One LM step for the M <= 16 listed slots: token sTok[m], previous state in pool row sPar[m], new state and lam into pool row sNew[m].
// Called by the whole workgroup; ends with the lam rows visible to every thread.
__device__ __forceinline__ void cpl_lm_step(const avsr_ctc_prefix_lm& L, float* wsC, float* wsH, int M, const int* sTok, const int* sPar,
                                            const int* sNew, float* sLam) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int H = L.H, E = L.E, V = L.V, nl = L.n_layers;
  const bool act = i16 < M;
  const int tok = act ? sTok[i16] : 0, par = act ? sPar[i16] : 0, nw = act ? sNew[i16] : 0;
  const long rs = (long)nl * H;                                            // floats per pool row
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < nl; ++j) {
    const int Kin = j == 0 ? E : H, K = Kin + H;
    const float* xin = j == 0 ? L.embedding + (long)tok * E : wsH + nw * rs + (long)(j - 1) * H;
    const float* hp = wsH + par * rs + (long)j * H;
    const float* wj = cpl_pick(L.wt, j);
    const float* bj = cpl_pick(L.bias, j);
    // C layout: row 4 g + r = gate r of unit 4 c + g, column i16 = the slot -- the cell finishes in this lane's registers
    auto cell = [&](int c, f32x4 acc) {
      const int u = 4 * c + g;
      const f32x4 z = acc + ld4(bj + 4 * u);
      const float cprev = wsC[par * rs + (long)j * H + u];
      const float gi = p_sigmoid(z[0]), gj = p_tanh(z[1]), gf = p_sigmoid(z[2] + 1.0f), go = p_sigmoid(z[3]);
      float cn = gf * cprev + gi * gj;
      cn = fminf(1.0f, fmaxf(-1.0f, cn));                                  // cell_clip = 1.0
      wsC[nw * rs + (long)j * H + u] = cn;
      wsH[nw * rs + (long)j * H + u] = go * p_tanh(cn);
    };
    for (int c = wave; 4 * c < H; c += 8) {                                // two tiles of 4 units per round: they share the x operand
      const int c1 = c + 4;
      const bool two = 4 * c1 < H;
      const float* w0 = wj + (long)(16 * c + i16) * K;                     // (4 H rows: 16 c + i16 < 4 H for every tile)
      const float* const wa[2] = {w0, two ? wj + (long)(16 * c1 + i16) * K : w0};
      f32x4 acc[2] = {zero, zero};
      cpl_dot<2>(wa, Kin, xin, H, hp, g, acc);
      if (act) {
        cell(c, acc[0]);
        if (two) cell(c1, acc[1]);
      }
    }
    __syncthreads();                                                      // h of this layer: stores drained, then read by every wave
  }
  {
    const float* ht = wsH + nw * rs + (long)(nl - 1) * H;
    for (int c = wave; 16 * c < V; c += 4) {
      const int v = 16 * c + i16;
      const float* const wr[1] = {L.wout_t + (long)(v < V ? v : 0) * H};    // (a row past V: computed on row 0, not stored)
      f32x4 acc[1] = {zero};
      cpl_dot<1>(wr, H, ht, 0, ht, g, acc);
      if (act) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int vv = 16 * c + 4 * g + r;
          if (vv < V) sLam[nw * V + vv] = acc[0][r] + L.bout[vv];
        }
      }
    }
  }
  lds_barrier();
  {
    const int rl = tid >> 4, q = tid & 15;                                // 16 lanes (one DPP row) per listed slot
    if (rl < M) {
      float* row = sLam + sNew[rl] * V;
      float mx = -INFINITY;
      for (int v = q; v < V; v += 16) mx = fmaxf(mx, row[v]);
      mx = row16_max(mx);
      float sum = 0.f;
      for (int v = q; v < V; v += 16) sum += expf(row[v] - mx);
      sum = row16_sum(sum);
      const float lse = mx + logf(sum);
      for (int v = q; v < V; v += 16) row[v] -= lse;
    }
  }
  lds_barrier();
}

// the LSTM as cp_search's Step: (c, h) of the 2 W pool rows in the caller's workspace, no LDS of its own
struct cpl_lstm_step {
  const avsr_ctc_prefix_lm& L;
  float* wsC;
  float* wsH;
  static size_t extra(int) { return 0; }
  __device__ __forceinline__ void init(int b, int W, uint32_t*) {
    const long pool = (long)2 * W * L.n_layers * L.H;                 // floats of one utterance's c (or h) pool
    wsC = reinterpret_cast<float*>(L.ws) + (long)b * 2 * pool;
    wsH = wsC + pool;
  }
  __device__ __forceinline__ void prologue(int tid) {                  // pool row 1: the zero state
    for (int e = tid; e < L.n_layers * L.H; e += 256) { wsC[(long)L.n_layers * L.H + e] = 0.f; wsH[(long)L.n_layers * L.H + e] = 0.f; }
  }
  __device__ __forceinline__ void step(int M, const int* sTok, const int* sPar, const int* sNew, float* sLam, bool) {
    cpl_lm_step(L, wsC, wsH, M, sTok, sPar, sNew, sLam);
  }
};

// dynamic LDS: cp_lds_words(V, W, L_max, true) words
__global__ __launch_bounds__(256) void ctc_prefix_lm_kernel(const avsr_ctc_prefix_args A, const avsr_ctc_prefix_lm L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cpl_smem[];
  cpl_lstm_step step{L, nullptr, nullptr};
  const cp_terms terms{L.weight, L.bonus, L.go_id, L.eos_id, L.s_lm, L.lm_steps, L.lm_logp};
  cp_search(A, terms, step, cpl_smem);
}

// AVSR_OK, or why the shape cannot run (decided on the host, nothing dereferenced)
static int ctc_prefix_lm_limits(int V, int W, int LM, int nl, int H, int E, int one_hot) {
  const bool bad = nl < 1 || H < 1 || E < 1 || (one_hot && E < V);
  const long lim = 1L << 31, kmax = (E > H ? E : H) + H;             // 32-bit element offsets inside a weight matrix and a pool
  const bool big = nl > AVSR_MAX_LM_LAYERS || H % 4 || E % 4 || (long)V * E >= lim || 4L * H * kmax >= lim || (long)V * H >= lim ||
                   4L * W * nl * H >= lim;
  return cp_limits(V, W, LM, AVSR_CTC_PREFIX_LM_MAX_W, true, cpl_lstm_step::extra(W), bad, big);   // (LDS at the three maxima: 70 KiB)
}

}  // namespace avsr

extern "C" int avsr_ctc_prefix_lm_supported(int32_t V, int32_t beam_width, int32_t L_max, int32_t n_layers, int32_t H, int32_t E,
                                            int32_t one_hot) {
  return avsr::ctc_prefix_lm_limits(V, beam_width, L_max, n_layers, H, E, one_hot) == AVSR_OK ? 1 : 0;
}

extern "C" int64_t avsr_ctc_prefix_lm_ws_bytes(int32_t B, int32_t beam_width, int32_t n_layers, int32_t H) {
  if (B < 1 || beam_width < 1 || n_layers < 1 || H < 1) return 0;
  return (int64_t)sizeof(float) * B * 2 * 2 * beam_width * n_layers * H;       // (c, h) x 2 W rows x layers x H
}

extern "C" int avsr_ctc_prefix_search_lm(const avsr_ctc_prefix_args* a, const avsr_ctc_prefix_lm* lm, void* stream) {
  using namespace avsr;
  if (!lm) return AVSR_ERR_ARG;
  int rc = cp_check_args(a);
  if (!rc) rc = cp_check_terms(a->V, lm->V, lm->go_id, lm->eos_id, lm->weight, lm->bonus);
  if (!rc) rc = ctc_prefix_lm_limits(a->V, a->beam_width, a->L_max, lm->n_layers, lm->H, lm->E, lm->one_hot);
  if (rc) return rc;
  if (!lm->embedding || !lm->wout_t || !lm->bout || !lm->ws || !lm->s_lm || !lm->lm_steps) return AVSR_ERR_ARG;
  for (int j = 0; j < lm->n_layers; ++j)
    if (!lm->wt[j] || !lm->bias[j]) return AVSR_ERR_ARG;
  if (lm->ws_bytes < avsr_ctc_prefix_lm_ws_bytes(a->B, a->beam_width, lm->n_layers, lm->H)) return AVSR_ERR_ARG;
  const size_t lds = sizeof(uint32_t) * cp_lds_words(a->V, a->beam_width, a->L_max, true, cpl_lstm_step::extra(a->beam_width));
  return cp_launch<ctc_prefix_lm_kernel>(lds, stream, *a, *lm);
}

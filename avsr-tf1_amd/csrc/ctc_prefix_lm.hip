// CTC prefix beam search with a language model fused into the frame loop (avsr_ctc_prefix_search_lm, include/avsr_hip.h; the rule is
// INTEGRATION.md section 8): ctc_prefix.hip's search -- ONE launch per batch, one 256-thread workgroup per utterance, the beam in LDS,
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
// Frame t: phases 1-5 are ctc_prefix.hip's, with the term taken from the parent slot's lam row in the candidate phase, in the merged
// partner's extension inside `stay` and in phase 5's recomputation.  Phase 5 also hands out the rows (one thread, <= 2 W bit operations)
// and lists the kept extensions (M <= W <= 16: ONE 16-row tile).  Phase 6, skipped by a workgroup-uniform branch when M = 0:
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
#include "wave.h"
#include "avsr_hip.h"
#include "prof.h"

namespace avsr {

#define CPL_LDS_MAX_BYTES (160 * 1024)

// ctc_prefix.hip's words, then lam [2 W][V], row index and s_lm [2][W] each, final [W], order [W], three lists of 16
static inline size_t cpl_lds_words(int V, int W, int LM) {
  const size_t C = (size_t)V + 1, LW = ((size_t)LM + 3) / 4;
  return 2 * (size_t)W * LW + 17 * (size_t)W + 20 + 2 * C + (size_t)W * C + 2 * (size_t)W * V + 6 * (size_t)W + 48;
}

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

// dynamic LDS: cpl_lds_words(V, W, L_max) words
__global__ __launch_bounds__(256) void ctc_prefix_lm_kernel(const avsr_ctc_prefix_args A, const avsr_ctc_prefix_lm L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cpl_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int T = A.T, V = A.V, C = V + 1, W = A.beam_width, LM = A.L_max, LW = (LM + 3) >> 2;
  uint32_t* sLab = cpl_smem;                                        // [2][W][LW]
  float* sPb = reinterpret_cast<float*>(sLab + 2 * W * LW);         // [2][W] each, half h at [h * W]
  float* sPnb = sPb + 2 * W;
  float* sP = sPnb + 2 * W;
  int* sLen = reinterpret_cast<int*>(sP + 2 * W);
  int* sLast = sLen + 2 * W;
  uint32_t* sHash = reinterpret_cast<uint32_t*>(sLast + 2 * W);     // of the label sequence
  uint32_t* sHpar = sHash + 2 * W;                                  // of the sequence without its last symbol
  int* sM = reinterpret_cast<int*>(sHpar + 2 * W);                  // merge partner, -1: none
  int* sSel = sM + 2 * W;                                           // [W]
  int* sCnt = sSel + W;                                             // [0], [1]: entries of the halves; [2]: entries selected; [3]: extensions kept
  float* sRed = reinterpret_cast<float*>(sCnt + 4);                 // [2][4][2] per-wave (max, sum) of a staged row
  float* sZ = sRed + 16;                                            // [2][C]
  float* sCand = sZ + 2 * C;                                        // [W * C]
  float* sLam = sCand + W * C;                                      // [2 W][V]: lam(. | g) per pool row
  int* sRow = reinterpret_cast<int*>(sLam + 2 * W * V);             // [2][W]: pool row of a slot
  float* sSlm = reinterpret_cast<float*>(sRow + 2 * W);             // [2][W]: sum of the lam terms of the slot's labels
  float* sFin = sSlm + 2 * W;                                       // [W]
  int* sOrd = reinterpret_cast<int*>(sFin + W);                     // [W]: slot at output position r
  int* sTok = sOrd + W;                                             // [16] each: the kept extensions of a frame
  int* sPar = sTok + 16;
  int* sNew = sPar + 16;

  int Tb = A.in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const float* zb = A.z + (long)b * T * A.ld;
  const bool own0 = tid < C, own1 = tid + 256 < C;                  // columns tid and tid + 256 (C <= 257)
  const float lw = L.weight, beta = L.bonus;
  const long pool = (long)2 * W * L.n_layers * L.H;                 // floats of one utterance's c (or h) pool
  float* wsC = reinterpret_cast<float*>(L.ws) + (long)b * 2 * pool;
  float* wsH = wsC + pool;
  int steps = 0;

  // row -> sZ[buf], its per-wave (max, sum) -> sRed[buf]
  auto stage = [&](int buf, float z0, float z1) {
    float mx = own0 ? z0 : -INFINITY;
    if (own1) mx = fmaxf(mx, z1);
    mx = wave64_max(mx);                                           // (called by whole waves only)
    float s = own0 ? expf(z0 - mx) : 0.f;
    if (own1) s += expf(z1 - mx);
    s = wave64_sum(s);
    if (own0) sZ[buf * C + tid] = z0;
    if (own1) sZ[buf * C + tid + 256] = z1;
    if (lane == 0) { sRed[buf * 8 + wave * 2] = mx; sRed[buf * 8 + wave * 2 + 1] = s; }
  };

  if (tid == 0) {
    sPb[0] = 0.f; sPnb[0] = -INFINITY; sP[0] = 0.f; sLen[0] = 0; sLast[0] = -1; sHash[0] = 0u; sHpar[0] = 0u; sM[0] = -1;
    sCnt[0] = 1;
    sRow[0] = 0; sSlm[0] = 0.f;
    sTok[0] = L.go_id; sPar[0] = 1; sNew[0] = 0; sCnt[3] = 1;       // the empty prefix: one step on GO from the zero state (pool row 1)
  }
  for (int e = tid; e < L.n_layers * L.H; e += 256) { wsC[(long)L.n_layers * L.H + e] = 0.f; wsH[(long)L.n_layers * L.H + e] = 0.f; }
  if (Tb > 0) stage(0, own0 ? zb[tid] : 0.f, own1 ? zb[tid + 256] : 0.f);
  __syncthreads();                                                  // the zeroed row is read from global memory

  // t = -1 is the prologue: phase 6 alone, on the list written above (one call site of the step keeps the loop's registers low)
  for (int t = -1; t < Tb; ++t) {
    if (t >= 0) {
    const int cur = t & 1, nxt = cur ^ 1, n = sCnt[cur];
    const bool more = t + 1 < Tb;
    float zn0 = 0.f, zn1 = 0.f;
    if (more) {                                                     // next row: in flight under the frame's search phases
      const float* zr = zb + (long)(t + 1) * A.ld;
      if (own0) zn0 = zr[tid];
      if (own1) zn1 = zr[tid + 256];
    }
    const float* pb = sPb + cur * W;
    const float* pnb = sPnb + cur * W;
    const float* pp = sP + cur * W;
    const int* len = sLen + cur * W;
    const int* last = sLast + cur * W;
    const uint32_t* hash = sHash + cur * W;
    const uint32_t* hpar = sHpar + cur * W;
    int* mrg = sM + cur * W;
    const uint32_t* lab = sLab + cur * W * LW;
    const int* row = sRow + cur * W;
    const float* zc = sZ + cur * C;
    float lse;
    {
      const float* rd = sRed + cur * 8;
      const float M = fmaxf(fmaxf(rd[0], rd[2]), fmaxf(rd[4], rd[6]));
      float S = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) if (rd[2 * w] != -INFINITY) S += rd[2 * w + 1] * expf(rd[2 * w] - M);
      lse = M + logf(S);
    }
    const float yV = zc[V] - lse;

    // ---- 1. merge partners: labels(j) == labels(k) without its last symbol ----
    for (int q = tid; q < n * n; q += 256) {
      const int k = q / n, j = q - k * n, lj = len[j];
      if (lj + 1 != len[k] || hash[j] != hpar[k]) continue;
      const uint32_t* rk = lab + k * LW;
      const uint32_t* rj = lab + j * LW;
      uint32_t diff = 0u;
#pragma unroll 4
      for (int w = 0; 4 * w < lj; ++w) {
        const int nb = lj - 4 * w;
        diff |= (rk[w] ^ rj[w]) & (nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u));
      }
      if (!diff) mrg[k] = j;
    }
    lds_barrier();

    // the language model's term of extending slot k by c
    auto term = [&](int k, int c) { return lw * sLam[row[k] * V + c] + beta; };
    // p_b and p_nb of the stay of slot k, its partner's extension merged in
    auto stay = [&](int k, float& sb, float& snb) {
      const int lk = last[k], j = mrg[k];
      sb = pp[k] + yV;
      snb = -INFINITY;
      if (lk >= 0) {
        const float yl = zc[lk] - lse;
        snb = pnb[k] + yl;
        if (j >= 0) snb = lse2(snb, (last[j] == lk ? pb[j] : pp[j]) + yl + term(j, lk));
      }
    };
    auto extend = [&](int k, int c) { return len[k] < LM ? (c == last[k] ? pb[k] : pp[k]) + (zc[c] - lse) + term(k, c) : -INFINITY; };

    // ---- 2. candidates ----
    for (int idx = tid; idx < n * C; idx += 256) {
      const int k = idx / C, c = idx - k * C;
      float v;
      if (c == V) { float sb, snb; stay(k, sb, snb); v = lse2(sb, snb); }
      else v = extend(k, c);
      sCand[idx] = v;
    }
    lds_barrier();
    // ---- 3. an extension that was merged into a stay is no candidate of its own ----
    if (tid < n && mrg[tid] >= 0) sCand[mrg[tid] * C + last[tid]] = -INFINITY;
    lds_barrier();

    // ---- 4. selection, wave 0 ----
    if (wave == 0) {
      const int NC = n * C;
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int i = lane; i < NC; i += 64) { const float v = sCand[i]; if (v > bv) { bv = v; bi = i; } }
      int ns = 0;
      for (int r = 0; r < W; ++r) {
        const float v = wave64_max(bv);                             // (all 64 lanes are active here: the loop's exits are uniform)
        if (v == -INFINITY) break;
        const int i = wave64_min_i(bv == v ? bi : 0x7fffffff);        // the lowest index among the lanes that hold the maximum
        if (lane == 0) sSel[r] = i;
        ns = r + 1;
        if (bi == i) {
          sCand[i] = -INFINITY;
          bv = -INFINITY; bi = 0x7fffffff;
          for (int u = lane; u < NC; u += 64) { const float x = sCand[u]; if (x > bv) { bv = x; bi = u; } }
        }
      }
      if (lane == 0) sCnt[2] = ns;
    }
    lds_barrier();

    // ---- 5. the new beam, its pool rows, the trace, the next row ----
    const int ns = sCnt[2];
    if (tid < W) {
      const int r = tid;
      int k = -1, c = -1;
      float nb_ = -INFINITY, nnb_ = -INFINITY;
      if (r < ns) {
        const int idx = sSel[r];
        k = idx / C; c = idx - k * C;
        int nl, nlast;
        uint32_t nh, nhp;
        float slm = sSlm[cur * W + k];
        if (c == V) { stay(k, nb_, nnb_); nl = len[k]; nlast = last[k]; nh = hash[k]; nhp = hpar[k]; }
        else {
          nnb_ = extend(k, c); nl = len[k] + 1; nlast = c; nh = hash[k] * 0x9E3779B1u + (uint32_t)(c + 1); nhp = hash[k];
          slm += sLam[row[k] * V + c];
        }
        const int o = nxt * W + r;
        sPb[o] = nb_; sPnb[o] = nnb_; sP[o] = lse2(nb_, nnb_); sLen[o] = nl; sLast[o] = nlast; sHash[o] = nh; sHpar[o] = nhp;
        sM[o] = -1; sSlm[o] = slm;
      }
      if (A.trace_parent) {
        const long q = ((long)b * T + t) * W + r;
        A.trace_parent[q] = k; A.trace_sym[q] = c; A.trace_pb[q] = nb_; A.trace_pnb[q] = nnb_;
      }
    }
    if (tid == 64) {                                                // a stay inherits its row; an extension takes one no OLD slot references
      uint32_t used = 0u;
      for (int k = 0; k < n; ++k) used |= 1u << row[k];
      int M = 0;
      for (int r = 0; r < ns; ++r) {
        const int idx = sSel[r], k = idx / C, c = idx - k * C;
        if (c == V) sRow[nxt * W + r] = row[k];
        else {
          const int f = __ffs((int)~used) - 1;                      // <= W old + < W new bits are set of 2 W <= 32: one is free
          used |= 1u << f;
          sRow[nxt * W + r] = f; sTok[M] = c; sPar[M] = row[k]; sNew[M] = f;
          ++M;
        }
      }
      sCnt[3] = M;
    }
    {
      uint32_t* nlab = sLab + nxt * W * LW;
      for (int e = tid; e < ns * LW; e += 256) {
        const int r = e / LW, w = e - r * LW, idx = sSel[r], k = idx / C, c = idx - k * C, lo = len[k];
        const uint32_t src = lab[k * LW + w];
        if (c == V) { if (4 * w < lo) nlab[e] = src; }
        else if (w < (lo >> 2)) nlab[e] = src;
        else if (w == (lo >> 2)) { const int sh = 8 * (lo & 3); nlab[e] = (src & ((1u << sh) - 1u)) | ((uint32_t)c << sh); }
      }
    }
    if (tid == 0) sCnt[nxt] = ns;
    if (more) stage(nxt, zn0, zn1);
    lds_barrier();
    }

    // ---- 6. the language model's step for the kept extensions (workgroup-uniform branch) ----
    const int M = sCnt[3];
    if (M > 0) {
      cpl_lm_step(L, wsC, wsH, M, sTok, sPar, sNew, sLam);
      steps += t >= 0 ? 1 : 0;
    }
  }

  // ---- the final beam: final = p + w lam(EOS | g), re-sorted ----
  const int fh = Tb & 1, n = sCnt[fh];
  if (tid < n) sFin[tid] = sP[fh * W + tid] + lw * sLam[sRow[fh * W + tid] * V + L.eos_id];
  lds_barrier();
  if (tid < n) {
    const float f = sFin[tid];
    int rank = 0;
    for (int r = 0; r < n; ++r) rank += (sFin[r] > f || (sFin[r] == f && r < tid)) ? 1 : 0;
    sOrd[rank] = tid;
  }
  lds_barrier();
  const uint32_t* lab = sLab + fh * W * LW;
  int32_t* ids = A.ids + (long)b * W * LM;
  for (int e = tid; e < W * LM; e += 256) {
    const int r = e / LM, l = e - r * LM;
    int v = -1;
    if (r < n) {
      const int s = sOrd[r];
      if (l < sLen[fh * W + s]) v = (int)((lab[s * LW + (l >> 2)] >> (8 * (l & 3))) & 0xffu);
    }
    ids[e] = v;
  }
  if (tid < W) {
    const int s = tid < n ? sOrd[tid] : 0;
    A.lens[(long)b * W + tid] = tid < n ? sLen[fh * W + s] : 0;
    A.score[(long)b * W + tid] = tid < n ? sFin[s] : -INFINITY;
    L.s_lm[(long)b * W + tid] = tid < n ? sSlm[fh * W + s] + sLam[sRow[fh * W + s] * V + L.eos_id] : 0.f;
  }
  if (L.lm_logp) {
    float* out = L.lm_logp + (long)b * W * V;
    for (int e = tid; e < W * V; e += 256) {
      const int r = e / V, v = e - r * V;
      out[e] = r < n ? sLam[sRow[fh * W + sOrd[r]] * V + v] : 0.f;
    }
  }
  if (tid == 0) L.lm_steps[b] = steps;
}

// AVSR_OK, or why the shape cannot run (decided on the host, nothing dereferenced)
static int ctc_prefix_lm_limits(int V, int W, int LM, int nl, int H, int E, int one_hot) {
  if (V < 1 || W < 1 || LM < 1 || nl < 1 || H < 1 || E < 1) return AVSR_ERR_ARG;
  if (one_hot && E < V) return AVSR_ERR_ARG;
  if (V > AVSR_CTC_PREFIX_MAX_V || W > AVSR_CTC_PREFIX_LM_MAX_W || LM > AVSR_CTC_PREFIX_MAX_L) return AVSR_ERR_UNSUPPORTED;
  if (nl > AVSR_MAX_LM_LAYERS || H % 4 || E % 4) return AVSR_ERR_UNSUPPORTED;
  const long lim = 1L << 31, kmax = (E > H ? E : H) + H;             // 32-bit element offsets inside a weight matrix and a pool
  if ((long)V * E >= lim || 4L * H * kmax >= lim || (long)V * H >= lim || 4L * W * nl * H >= lim) return AVSR_ERR_UNSUPPORTED;
  if (sizeof(uint32_t) * cpl_lds_words(V, W, LM) > CPL_LDS_MAX_BYTES) return AVSR_ERR_UNSUPPORTED;   // (holds at the three maxima: 70 KiB)
  return AVSR_OK;
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
  if (!a || !lm || !a->z || !a->in_len || !a->ids || !a->lens || !a->score) return AVSR_ERR_ARG;
  if (a->B <= 0 || a->T <= 0 || a->ld < (int64_t)a->V + 1) return AVSR_ERR_ARG;
  const int ntr = (a->trace_parent != 0) + (a->trace_sym != 0) + (a->trace_pb != 0) + (a->trace_pnb != 0);
  if (ntr != 0 && ntr != 4) return AVSR_ERR_ARG;
  if (lm->V != a->V || lm->go_id < 0 || lm->go_id >= a->V || lm->eos_id < 0 || lm->eos_id >= a->V) return AVSR_ERR_ARG;
  if (!(lm->weight >= 0.f) || lm->weight == INFINITY || !(lm->bonus == lm->bonus) || lm->bonus == INFINITY || lm->bonus == -INFINITY)
    return AVSR_ERR_ARG;
  const int rc = ctc_prefix_lm_limits(a->V, a->beam_width, a->L_max, lm->n_layers, lm->H, lm->E, lm->one_hot);
  if (rc) return rc;
  if (!lm->embedding || !lm->wout_t || !lm->bout || !lm->ws || !lm->s_lm || !lm->lm_steps) return AVSR_ERR_ARG;
  for (int j = 0; j < lm->n_layers; ++j)
    if (!lm->wt[j] || !lm->bias[j]) return AVSR_ERR_ARG;
  if (lm->ws_bytes < avsr_ctc_prefix_lm_ws_bytes(a->B, a->beam_width, lm->n_layers, lm->H)) return AVSR_ERR_ARG;
  const size_t lds = sizeof(uint32_t) * cpl_lds_words(a->V, a->beam_width, a->L_max);
  static bool attr_set = false;
  if (lds > 64 * 1024 && !attr_set) {
    if (hipFuncSetAttribute((const void*)ctc_prefix_lm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CPL_LDS_MAX_BYTES) != hipSuccess)
      return AVSR_ERR_HIP;
    attr_set = true;
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(PROF_STEP_LINEAR, s);
  hipLaunchKernelGGL(ctc_prefix_lm_kernel, dim3(a->B), dim3(256), lds, s, *a, *lm);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// The CTC prefix beam search with a language-model term, written ONCE over the model that supplies
// lam(. | g): phases 1-5 of a frame, the hand-out of pool rows, the list of kept extensions, the final re-sort and the outputs.  The two
// kernels that instantiate it differ only in phase 6, the model's step for the kept extensions:
//   csrc/ctc_prefix_lm.hip      an avsr.LM LSTM; per-row state (c, h) in a global workspace
//   csrc/ctc_prefix_ngram.hip   a back-off n-gram automaton; per-row state one node id in LDS (the `extra` words below)
// What the search needs of a model is a `Step` object:
//   extra(W)                                  (host, static) LDS words of per-row state behind the search's own
//   init(b, W, extra_words)                   called by every thread before anything else
//   prologue(tid)                             global-memory writes that the first step reads (a __syncthreads() follows)
//   step(M, sTok, sPar, sNew, sLam, first)    called by the WHOLE workgroup under a workgroup-uniform branch: for m < M <= 16 the label
//                                             sequence in pool row sNew[m] is the one in row sPar[m] extended by sTok[m]; set its state and
//                                             the row sLam[sNew[m] * V .. + V) = lam(. | g), and end with the rows visible to every thread.
//                                             first: the empty prefix (sTok[0] = GO, sPar[0] a row in its initial state, sNew[0] = 0).
// and of its descriptor the fields of cpl_terms.  Everything is force-inlined: an instantiation is one kernel with one call site of the
// step, as the LSTM kernel was before the search moved here.
#pragma once
#include "wave.h"
#include "avsr_hip.h"

namespace avsr {

#define CPL_LDS_MAX_BYTES (160 * 1024)

// ctc_prefix.hip's words, then lam [2 W][V], row index and s_lm [2][W] each, final [W], order [W], three lists of 16
static inline size_t cpl_lds_words(int V, int W, int LM) {
  const size_t C = (size_t)V + 1, LW = ((size_t)LM + 3) / 4;
  return 2 * (size_t)W * LW + 17 * (size_t)W + 20 + 2 * C + (size_t)W * C + 2 * (size_t)W * V + 6 * (size_t)W + 48;
}

// what the search itself reads of a model's descriptor
struct cpl_terms {
  float weight, bonus;
  int go_id, eos_id;
  float* s_lm;
  int32_t* lm_steps;
  float* lm_logp;
};

// smem: cpl_lds_words(V, W, L_max) + Step::extra(W) words of dynamic LDS
template <class Step>
__device__ __forceinline__ void cpl_search(const avsr_ctc_prefix_args& A, const cpl_terms& L, Step& mdl, uint32_t* cpl_smem) {
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
  mdl.init(b, W, reinterpret_cast<uint32_t*>(sNew + 16));

  int Tb = A.in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const float* zb = A.z + (long)b * T * A.ld;
  const bool own0 = tid < C, own1 = tid + 256 < C;                  // columns tid and tid + 256 (C <= 257)
  const float lw = L.weight, beta = L.bonus;
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
    sTok[0] = L.go_id; sPar[0] = 1; sNew[0] = 0; sCnt[3] = 1;       // the empty prefix: one step on GO from the initial state (pool row 1)
  }
  mdl.prologue(tid);
  if (Tb > 0) stage(0, own0 ? zb[tid] : 0.f, own1 ? zb[tid + 256] : 0.f);
  __syncthreads();                                                  // what the prologue wrote is read from global memory

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
      mdl.step(M, sTok, sPar, sNew, sLam, t < 0);
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

}  // namespace avsr

// The CTC prefix beam search, written ONCE: the frame-synchronous search on the head's logits that sums over
// alignments, with no decoder step, optionally with a language-model term fused into the frame loop.  fp32, gfx950, no atomics: two
// launches on the same inputs are bit-identical.  Four kernels instantiate cp_search:
//   csrc/ctc_prefix.hip         no model (cp_no_model): the plain search, beam widths up to 64
//   csrc/ctc_prefix_lm.hip      an avsr.LM LSTM; per-row state (c, h) in a global workspace
//   csrc/ctc_prefix_ngram.hip   a back-off n-gram automaton; per-row state one node id in LDS (the `extra` words below)
//   csrc/ctc_prefix_word_ngram.hip   a word-level n-gram behind a lexicon trie; per-row state five words in LDS
// The no-model case is a compile-time policy: that kernel holds no term, no pool rows, no phase 6 and no re-sort.
//
// ONE launch per batch, one 256-thread workgroup per utterance, the whole frame loop inside: the dependent chain is T_b frames long and
// nothing of a frame leaves the chip.  In LDS: the beam's label rows (one byte per label -- V <= 256 -- packed four to a word, ping-pong),
// per slot (p_b, p_nb, p, length, last symbol, two hashes, merge partner) as a ping-pong too, two rows of logits, the candidate scores
// [n (V + 1)] and the selection.  Row t + 1 of z is loaded into registers at the top of frame t and staged at its end, so T is not
// bounded by on-chip memory and the load's latency lies under the frame's work.
//
// Frame t (n = entries in the beam, C = V + 1; five LDS-only barriers):
//   1. merge partners.  Two candidates of a frame name the same label sequence only as the stay of slot k and the extension of slot j by
//      last(k), where labels(j) = labels(k) without its last symbol; k has at most one such j.  All n^2 pairs are tried by LABEL
//      COMPARISON: the lengths and two rolling hashes (of the sequence, of the sequence without its last symbol) only decide which pairs
//      are compared word by word -- unequal hashes prove unequal labels, equal hashes prove nothing and are not trusted.  A prefix that
//      left the beam and was re-created while its extension stayed is found like any other: nothing is remembered across frames.
//   2. candidates.  idx = k C + c: c < V the extension (-inf at length L_max), c = V the stay with its partner's extension merged in.
//   3. the merged extensions are struck (-inf).
//   4. selection inside wave 0: lane l owns the candidates idx = l (mod 64) and keeps its best; each of up to W rounds is a wave
//      maximum of p, then a wave minimum of idx over the lanes that hold it (DPP row rotations, no LDS), after which the winning lane
//      strikes its candidate and rescans its own.  Stops at p = -inf, so the beam may hold fewer than W.  The beam's slot order is the selection order: it is sorted.
//   5. the new beam into the other half: states recomputed from the old half (a few flops), label rows copied word-wise, the appended
//      symbol composed into its word; the trace rows; row t + 1 staged with its per-wave (max, sum) for the log-softmax.
// The barrier is wave.h's lds_barrier: s_waitcnt lgkmcnt(0) + s_barrier, so the prefetch and the trace stores are not waited for at every phase.
//
// With a model, an extension of slot k by c also carries  w * lam(c | labels(k)) + beta  -- in the candidate phase, in the merged
// partner's extension inside `stay` and in phase 5's recomputation.  lam rows live in LDS, [2 W rows][V], addressed through a per-slot
// ROW INDEX into a pool of 2 W rows: a stay inherits its parent's row, an extension takes a row that no OLD slot references (phase 5,
// one thread, <= 2 W <= 32 bit operations), so nothing is ever copied and no step reads a row that the same step writes.  Phase 5 also
// lists the M <= W <= 16 kept extensions; phase 6, the model's step for them, is skipped by a workgroup-uniform branch when M = 0.  The
// empty prefix's row comes from one such step before frame 0.  After the last frame: final = p + w * lam(EOS | g), the entries re-sorted
// by final (descending, ties to the earlier slot), s_lm, lm_steps, and the optional lam rows of the final entries.
// What the search needs of a model is a `Step` object:
//   extra(W)                                  (host, static) LDS words of per-row state behind the search's own
//   init(b, W, extra_words)                   called by every thread before anything else
//   prologue(tid)                             global-memory writes that the first step reads (a __syncthreads() follows)
//   step(M, sTok, sPar, sNew, sLam, first)    called by the WHOLE workgroup under a workgroup-uniform branch: for m < M <= 16 the label
//                                             sequence in pool row sNew[m] is the one in row sPar[m] extended by sTok[m]; set its state and
//                                             the row sLam[sNew[m] * V .. + V) = lam(. | g), and end with the rows visible to every thread.
//                                             first: the empty prefix (sTok[0] = GO, sPar[0] a row in its initial state, sNew[0] = 0).
// and of its descriptor the fields of cp_terms.  Everything is force-inlined: an instantiation is one kernel with one call site of the
// step.  The host part at the end holds the argument checks and the launch that the three entry points share.
#pragma once
#include <type_traits>
#include "wave.h"
#include "avsr_hip.h"
#include "prof.h"

namespace avsr {

#define CP_LDS_MAX_BYTES (160 * 1024)

// the search's words; with a model then lam [2 W][V], row index and s_lm [2][W] each, final [W], order [W], three lists of 16, and the
// model's own `extra`
static inline size_t cp_lds_words(int V, int W, int LM, bool model = false, size_t extra = 0) {
  const size_t C = (size_t)V + 1, LW = ((size_t)LM + 3) / 4;
  const size_t plain = 2 * (size_t)W * LW + 17 * (size_t)W + 20 + 2 * C + (size_t)W * C;
  return model ? plain + 2 * (size_t)W * V + 6 * (size_t)W + 48 + extra : plain;
}

// what the search itself reads of a model's descriptor
struct cp_terms {
  float weight, bonus;
  int go_id, eos_id;
  float* s_lm;
  int32_t* lm_steps;
  float* lm_logp;
};

// the Step of the plain search: nothing of it is ever called
struct cp_no_model {
  static size_t extra(int) { return 0; }
};

// smem: cp_lds_words(V, W, L_max, model, Step::extra(W)) words of dynamic LDS
template <class Step>
__device__ __forceinline__ void cp_search(const avsr_ctc_prefix_args& A, const cp_terms& L, Step& mdl, uint32_t* smem) {
  constexpr bool kModel = !std::is_same<Step, cp_no_model>::value;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int T = A.T, V = A.V, C = V + 1, W = A.beam_width, LM = A.L_max, LW = (LM + 3) >> 2;
  uint32_t* sLab = smem;                                            // [2][W][LW]
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
  // with a model only (cp_lds_words: without one the words end here)
  float* sLam = sCand + W * C;                                      // [2 W][V]: lam(. | g) per pool row
  int* sRow = reinterpret_cast<int*>(sLam + 2 * W * V);             // [2][W]: pool row of a slot
  float* sSlm = reinterpret_cast<float*>(sRow + 2 * W);             // [2][W]: sum of the lam terms of the slot's labels
  float* sFin = sSlm + 2 * W;                                       // [W]
  int* sOrd = reinterpret_cast<int*>(sFin + W);                     // [W]: slot at output position r
  int* sTok = sOrd + W;                                             // [16] each: the kept extensions of a frame
  int* sPar = sTok + 16;
  int* sNew = sPar + 16;
  if constexpr (kModel) mdl.init(b, W, reinterpret_cast<uint32_t*>(sNew + 16));

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
    if constexpr (kModel) {
      sRow[0] = 0; sSlm[0] = 0.f;
      sTok[0] = L.go_id; sPar[0] = 1; sNew[0] = 0; sCnt[3] = 1;     // the empty prefix: one step on GO from the initial state (pool row 1)
    }
  }
  if constexpr (kModel) mdl.prologue(tid);
  if (Tb > 0) stage(0, own0 ? zb[tid] : 0.f, own1 ? zb[tid + 256] : 0.f);
  if constexpr (kModel) __syncthreads();                            // what the prologue wrote is read from global memory
  else lds_barrier();

  // with a model, t = -1 is the prologue: phase 6 alone, on the list written above (one call site of the step keeps the loop's registers low)
  for (int t = kModel ? -1 : 0; t < Tb; ++t) {
    if (!kModel || t >= 0) {
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
    const int* row = sRow + cur * W;                                // (with a model)
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

    // x, the CTC part of extending slot k by c, with the language model's term of that extension
    auto with_term = [&](float x, int k, int c) {
      if constexpr (kModel) return x + (lw * sLam[row[k] * V + c] + beta);
      else return x;
    };
    // p_b and p_nb of the stay of slot k, its partner's extension merged in
    auto stay = [&](int k, float& sb, float& snb) {
      const int lk = last[k], j = mrg[k];
      sb = pp[k] + yV;
      snb = -INFINITY;
      if (lk >= 0) {
        const float yl = zc[lk] - lse;
        snb = pnb[k] + yl;
        if (j >= 0) snb = lse2(snb, with_term((last[j] == lk ? pb[j] : pp[j]) + yl, j, lk));
      }
    };
    auto extend = [&](int k, int c) { return len[k] < LM ? with_term((c == last[k] ? pb[k] : pp[k]) + (zc[c] - lse), k, c) : -INFINITY; };

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
        float slm = 0.f;
        if constexpr (kModel) slm = sSlm[cur * W + k];
        if (c == V) { stay(k, nb_, nnb_); nl = len[k]; nlast = last[k]; nh = hash[k]; nhp = hpar[k]; }
        else {
          nnb_ = extend(k, c); nl = len[k] + 1; nlast = c; nh = hash[k] * 0x9E3779B1u + (uint32_t)(c + 1); nhp = hash[k];
          if constexpr (kModel) slm += sLam[row[k] * V + c];
        }
        const int o = nxt * W + r;
        sPb[o] = nb_; sPnb[o] = nnb_; sP[o] = lse2(nb_, nnb_); sLen[o] = nl; sLast[o] = nlast; sHash[o] = nh; sHpar[o] = nhp;
        sM[o] = -1;
        if constexpr (kModel) sSlm[o] = slm;
      }
      if (A.trace_parent) {
        const long q = ((long)b * T + t) * W + r;
        A.trace_parent[q] = k; A.trace_sym[q] = c; A.trace_pb[q] = nb_; A.trace_pnb[q] = nnb_;
      }
    }
    if constexpr (kModel) {
      if (tid == 64) {                                              // a stay inherits its row; an extension takes one no OLD slot references
        uint32_t used = 0u;
        for (int k = 0; k < n; ++k) used |= 1u << row[k];
        int M = 0;
        for (int r = 0; r < ns; ++r) {
          const int idx = sSel[r], k = idx / C, c = idx - k * C;
          if (c == V) sRow[nxt * W + r] = row[k];
          else {
            const int f = __ffs((int)~used) - 1;                    // <= W old + < W new bits are set of 2 W <= 32: one is free
            used |= 1u << f;
            sRow[nxt * W + r] = f; sTok[M] = c; sPar[M] = row[k]; sNew[M] = f;
            ++M;
          }
        }
        sCnt[3] = M;
      }
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
    if constexpr (kModel) {
      const int M = sCnt[3];
      if (M > 0) {
        mdl.step(M, sTok, sPar, sNew, sLam, t < 0);
        steps += t >= 0 ? 1 : 0;
      }
    }
  }

  // ---- the final beam (sorted: the slot order is the selection order); with a model: final = p + w lam(EOS | g), re-sorted ----
  const int fh = Tb & 1, n = sCnt[fh];
  if constexpr (kModel) {
    if (tid < n) sFin[tid] = sP[fh * W + tid] + lw * sLam[sRow[fh * W + tid] * V + L.eos_id];
    lds_barrier();
    if (tid < n) {
      const float f = sFin[tid];
      int rank = 0;
      for (int r = 0; r < n; ++r) rank += (sFin[r] > f || (sFin[r] == f && r < tid)) ? 1 : 0;
      sOrd[rank] = tid;
    }
    lds_barrier();
  }
  auto slot_at = [&](int r) {                                       // (r < n)
    if constexpr (kModel) return sOrd[r];
    else return r;
  };
  const uint32_t* lab = sLab + fh * W * LW;
  int32_t* ids = A.ids + (long)b * W * LM;
  for (int e = tid; e < W * LM; e += 256) {
    const int r = e / LM, l = e - r * LM;
    int v = -1;
    if (r < n) {
      const int s = slot_at(r);
      if (l < sLen[fh * W + s]) v = (int)((lab[s * LW + (l >> 2)] >> (8 * (l & 3))) & 0xffu);
    }
    ids[e] = v;
  }
  if (tid < W) {
    const int s = tid < n ? slot_at(tid) : 0;
    A.lens[(long)b * W + tid] = tid < n ? sLen[fh * W + s] : 0;
    if constexpr (kModel) {
      A.score[(long)b * W + tid] = tid < n ? sFin[s] : -INFINITY;
      L.s_lm[(long)b * W + tid] = tid < n ? sSlm[fh * W + s] + sLam[sRow[fh * W + s] * V + L.eos_id] : 0.f;
    } else {
      A.score[(long)b * W + tid] = tid < n ? sP[fh * W + s] : -INFINITY;
    }
  }
  if constexpr (kModel) {
    if (L.lm_logp) {
      float* out = L.lm_logp + (long)b * W * V;
      for (int e = tid; e < W * V; e += 256) {
        const int r = e / V, v = e - r * V;
        out[e] = r < n ? sLam[sRow[fh * W + sOrd[r]] * V + v] : 0.f;
      }
    }
    if (tid == 0) L.lm_steps[b] = steps;
  }
}

// ---- host: what the three entry points check and how they launch ----

// the search's own arguments: AVSR_OK or AVSR_ERR_ARG
static inline int cp_check_args(const avsr_ctc_prefix_args* a) {
  if (!a || !a->z || !a->in_len || !a->ids || !a->lens || !a->score) return AVSR_ERR_ARG;
  if (a->B <= 0 || a->T <= 0 || a->ld < (int64_t)a->V + 1) return AVSR_ERR_ARG;
  const int ntr = (a->trace_parent != 0) + (a->trace_sym != 0) + (a->trace_pb != 0) + (a->trace_pnb != 0);
  if (ntr != 0 && ntr != 4) return AVSR_ERR_ARG;
  return AVSR_OK;
}

// a model's term against the search's V: AVSR_OK or AVSR_ERR_ARG
static inline int cp_check_terms(int V, int mV, int go_id, int eos_id, float weight, float bonus) {
  if (mV != V || go_id < 0 || go_id >= V || eos_id < 0 || eos_id >= V) return AVSR_ERR_ARG;
  if (!(weight >= 0.f) || weight == INFINITY || !(bonus == bonus) || bonus == INFINITY || bonus == -INFINITY) return AVSR_ERR_ARG;
  return AVSR_OK;
}

// AVSR_OK, or why the shape cannot run: the search's part of a kernel's limits, against that kernel's widest beam and LDS words.
// model_bad / model_big: the model's own shape is no shape at all / is one the kernel does not cover.
static inline int cp_limits(int V, int W, int LM, int max_W, bool model = false, size_t extra = 0, bool model_bad = false,
                            bool model_big = false) {
  if (V < 1 || W < 1 || LM < 1 || model_bad) return AVSR_ERR_ARG;
  if (V > AVSR_CTC_PREFIX_MAX_V || W > max_W || LM > AVSR_CTC_PREFIX_MAX_L || model_big) return AVSR_ERR_UNSUPPORTED;
  if (sizeof(uint32_t) * cp_lds_words(V, W, LM, model, extra) > CP_LDS_MAX_BYTES) return AVSR_ERR_UNSUPPORTED;
  return AVSR_OK;
}

// one workgroup per utterance with lds bytes of dynamic LDS (above 64 KiB the kernel is told so, once)
template <auto Kernel, class... Desc>
static inline int cp_launch(size_t lds, void* stream, const avsr_ctc_prefix_args& a, const Desc&... desc) {
  static bool attr_set = false;                                     // (per kernel)
  if (lds > 64 * 1024 && !attr_set) {
    if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CP_LDS_MAX_BYTES) != hipSuccess)
      return AVSR_ERR_HIP;
    attr_set = true;
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(PROF_STEP_LINEAR, s);
  hipLaunchKernelGGL(Kernel, dim3(a.B), dim3(256), lds, s, a, desc...);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

}  // namespace avsr

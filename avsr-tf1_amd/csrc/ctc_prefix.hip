// CTC prefix beam search on the head's logits alone (avsr_ctc_prefix_search, include/avsr_hip.h; the rule is INTEGRATION.md section 8):
// the frame-synchronous search that sums over alignments, with no decoder step.  fp32, gfx950, no atomics: two launches on the same
// inputs are bit-identical.
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
#include "wave.h"
#include "avsr_hip.h"
#include "prof.h"

namespace avsr {

#define CP_LDS_MAX_BYTES (160 * 1024)

static inline size_t cp_lds_words(int V, int W, int LM) {
  const size_t C = (size_t)V + 1, LW = ((size_t)LM + 3) / 4;
  return 2 * (size_t)W * LW + 17 * (size_t)W + 20 + 2 * C + (size_t)W * C;
}

// dynamic LDS: cp_lds_words(V, W, L_max) words
__global__ __launch_bounds__(256) void ctc_prefix_kernel(const avsr_ctc_prefix_args A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cp_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int T = A.T, V = A.V, C = V + 1, W = A.beam_width, LM = A.L_max, LW = (LM + 3) >> 2;
  uint32_t* sLab = cp_smem;                                         // [2][W][LW]
  float* sPb = reinterpret_cast<float*>(sLab + 2 * W * LW);         // [2][W] each, half h at [h * W]
  float* sPnb = sPb + 2 * W;
  float* sP = sPnb + 2 * W;
  int* sLen = reinterpret_cast<int*>(sP + 2 * W);
  int* sLast = sLen + 2 * W;
  uint32_t* sHash = reinterpret_cast<uint32_t*>(sLast + 2 * W);     // of the label sequence
  uint32_t* sHpar = sHash + 2 * W;                                  // of the sequence without its last symbol
  int* sM = reinterpret_cast<int*>(sHpar + 2 * W);                  // merge partner, -1: none
  int* sSel = sM + 2 * W;                                           // [W]
  int* sCnt = sSel + W;                                             // [0], [1]: entries of the halves; [2]: entries selected
  float* sRed = reinterpret_cast<float*>(sCnt + 4);                 // [2][4][2] per-wave (max, sum) of a staged row
  float* sZ = sRed + 16;                                            // [2][C]
  float* sCand = sZ + 2 * C;                                        // [W * C]

  int Tb = A.in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const float* zb = A.z + (long)b * T * A.ld;
  const bool own0 = tid < C, own1 = tid + 256 < C;                  // columns tid and tid + 256 (C <= 257)

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
  }
  if (Tb > 0) stage(0, own0 ? zb[tid] : 0.f, own1 ? zb[tid + 256] : 0.f);
  lds_barrier();

  for (int t = 0; t < Tb; ++t) {
    const int cur = t & 1, nxt = cur ^ 1, n = sCnt[cur];
    const bool more = t + 1 < Tb;
    float zn0 = 0.f, zn1 = 0.f;
    if (more) {                                                     // next row: in flight under the whole frame
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

    // p_b and p_nb of the stay of slot k, its partner's extension merged in
    auto stay = [&](int k, float& sb, float& snb) {
      const int lk = last[k], j = mrg[k];
      sb = pp[k] + yV;
      snb = -INFINITY;
      if (lk >= 0) {
        const float yl = zc[lk] - lse;
        snb = pnb[k] + yl;
        if (j >= 0) snb = lse2(snb, (last[j] == lk ? pb[j] : pp[j]) + yl);
      }
    };
    auto extend = [&](int k, int c) { return len[k] < LM ? (c == last[k] ? pb[k] : pp[k]) + (zc[c] - lse) : -INFINITY; };

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

    // ---- 5. the new beam, the trace, the next row ----
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
        if (c == V) { stay(k, nb_, nnb_); nl = len[k]; nlast = last[k]; nh = hash[k]; nhp = hpar[k]; }
        else { nnb_ = extend(k, c); nl = len[k] + 1; nlast = c; nh = hash[k] * 0x9E3779B1u + (uint32_t)(c + 1); nhp = hash[k]; }
        const int o = nxt * W + r;
        sPb[o] = nb_; sPnb[o] = nnb_; sP[o] = lse2(nb_, nnb_); sLen[o] = nl; sLast[o] = nlast; sHash[o] = nh; sHpar[o] = nhp;
        sM[o] = -1;
      }
      if (A.trace_parent) {
        const long q = ((long)b * T + t) * W + r;
        A.trace_parent[q] = k; A.trace_sym[q] = c; A.trace_pb[q] = nb_; A.trace_pnb[q] = nnb_;
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

  // ---- the final beam (sorted: the slot order is the selection order) ----
  const int fh = Tb & 1, n = sCnt[fh];
  const uint32_t* lab = sLab + fh * W * LW;
  int32_t* ids = A.ids + (long)b * W * LM;
  for (int e = tid; e < W * LM; e += 256) {
    const int r = e / LM, l = e - r * LM;
    int v = -1;
    if (r < n && l < sLen[fh * W + r]) v = (int)((lab[r * LW + (l >> 2)] >> (8 * (l & 3))) & 0xffu);
    ids[e] = v;
  }
  if (tid < W) {
    A.lens[(long)b * W + tid] = tid < n ? sLen[fh * W + tid] : 0;
    A.score[(long)b * W + tid] = tid < n ? sP[fh * W + tid] : -INFINITY;
  }
}

// AVSR_OK, or why the shape cannot run
static int ctc_prefix_limits(int V, int W, int LM) {
  if (V < 1 || W < 1 || LM < 1) return AVSR_ERR_ARG;
  if (V > AVSR_CTC_PREFIX_MAX_V || W > AVSR_CTC_PREFIX_MAX_W || LM > AVSR_CTC_PREFIX_MAX_L) return AVSR_ERR_UNSUPPORTED;
  if (sizeof(uint32_t) * cp_lds_words(V, W, LM) > CP_LDS_MAX_BYTES) return AVSR_ERR_UNSUPPORTED;   // (holds at the three maxima: 137 KiB)
  return AVSR_OK;
}

}  // namespace avsr

extern "C" int avsr_ctc_prefix_search_supported(int32_t V, int32_t beam_width, int32_t L_max) {
  return avsr::ctc_prefix_limits(V, beam_width, L_max) == AVSR_OK ? 1 : 0;
}

extern "C" int avsr_ctc_prefix_search(const avsr_ctc_prefix_args* a, void* stream) {
  using namespace avsr;
  if (!a || !a->z || !a->in_len || !a->ids || !a->lens || !a->score) return AVSR_ERR_ARG;
  if (a->B <= 0 || a->T <= 0 || a->ld < (int64_t)a->V + 1) return AVSR_ERR_ARG;
  const int ntr = (a->trace_parent != 0) + (a->trace_sym != 0) + (a->trace_pb != 0) + (a->trace_pnb != 0);
  if (ntr != 0 && ntr != 4) return AVSR_ERR_ARG;
  const int rc = ctc_prefix_limits(a->V, a->beam_width, a->L_max);
  if (rc) return rc;
  const size_t lds = sizeof(uint32_t) * cp_lds_words(a->V, a->beam_width, a->L_max);
  static bool attr_set = false;
  if (lds > 64 * 1024 && !attr_set) {
    if (hipFuncSetAttribute((const void*)ctc_prefix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CP_LDS_MAX_BYTES) != hipSuccess)
      return AVSR_ERR_HIP;
    attr_set = true;
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(PROF_STEP_LINEAR, s);
  hipLaunchKernelGGL(ctc_prefix_kernel, dim3(a->B), dim3(256), lds, s, *a);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// CTC auxiliary loss on an encoder's outputs (use_ctc): per-utterance negative log-likelihood of the label row without its EOS and
// its gradient with respect to the head's logits, in ONE launch (fp32, gfx950).  Not in the reference: the definition is
// tf.nn.ctc_loss's / torch's -- the blank is the LAST class (C - 1), an utterance with no valid alignment contributes 0 and a zero
// gradient (zero_infinity).
//
// Work split: one workgroup per utterance (the utterances are independent: nothing persistent, no inter-workgroup traffic).  Thread i
// owns the blank state 2i and the label state 2i + 1 of the 2U + 1 states, so a transition needs one value of a neighbouring thread
// (label i - 1 going forward, blank / label i + 1 going backward), exchanged through LDS with ONE barrier per time step.
//
// Phases (T_b = frames of the utterance, U its labels):
//   1. log-softmax of rows t < T_b over the real C classes (16 lanes per row), written into dz: every later phase reads the row it
//      needs from there, and the backward sweep overwrites row t with the gradient once nothing reads it any more.
//   2. alpha, t = 0 .. T_b - 1, in the log domain; after every step the states are shifted by their maximum m_t, so what is stored
//      (workspace: alpha^_t [T, 2L], m_t [T]) stays within fp32's accurate range whatever T is; log p(target) = sum_t m_t (fp64
//      accumulator, one add per step) + log(exp alpha^_{T-1}(last blank) + exp alpha^_{T-1}(last label)).
//   3. beta backwards, carried as beta^_t = log beta_t - (log p - sum_{u <= t} m_u): the shift is the alpha sweep's, so the sweep
//      needs no maximum of its own and exp(alpha^_t(s) + beta^_t(s) - logp_t(l_s)) sums to 1 over s up to the rounding accumulated
//      along the two sweeps (1e-4 at T = 500); dividing by the step's own sum -- the occupancy as a softmax over the states -- takes
//      that common factor out again (beta_t here includes the emission of step t).
//      dz[t, k] = weight / denom * (softmax_t[k] - sum of the occupancies of class k) is formed in the same sweep: beta never goes
//      to memory.
// No floating-point atomics: the label states are grouped by class once per utterance (index list in LDS, ascending state order) and
// thread k sums the states of class k in that order; the blank states (every even state) are summed by a wave reduction plus a
// fixed-order sum over the waves.  Two launches on the same inputs are bit-identical.
// Rows t >= T_b, and every row of an utterance without a valid alignment, are stored as zeros by every launch.
#include "wave.h"
#include "avsr_hip.h"

namespace avsr {

#define S_(x) ((hipStream_t)(x))

// (expf(a - m) + expf(b - m): rounds differently from wave.h's lse2 (1 + expf(-|a - b|)), so the loss keeps its own)
__device__ __forceinline__ float ctc_lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m));
}
__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// rows [r0, r1) x columns [0, C) of utterance b's block of dz = 0
__device__ __forceinline__ void ctc_zero_rows(float* dzb, long ld, int C, int r0, int r1) {
  const int n = (r1 - r0) * C;
  for (int idx = threadIdx.x; idx < n; idx += blockDim.x) {
    const int r = idx / C, c = idx - r * C;
    dzb[(long)(r0 + r) * ld + c] = 0.f;
  }
}

// blockDim.x = NT: a multiple of 64, >= max(L, C), <= 1024.  Dynamic LDS: ctc_lds_bytes(NT, L, C).
__global__ __launch_bounds__(1024) void ctc_loss_kernel(const avsr_ctc_args A) {
  extern __shared__ __attribute__((aligned(16))) float ctc_smem[];
  const int NT = blockDim.x, i = threadIdx.x, lane = i & 63, wv = i >> 6, nw = NT >> 6;
  const int b = blockIdx.x, T = A.T, L = A.L, C = A.C, blank = C - 1;
  const long ld = A.ld;
  const int XS = NT + 2;                  // exchange rows: thread i's value at [i + 1], -inf sentinels at [0] and [NT + 1]
  float* exE = ctc_smem;                  // [2][XS]  blank states (beta sweep)
  float* exO = exE + 2 * XS;              // [2][XS]  label states
  float* gam = exO + 2 * XS;              // [2][NT]  occupancies of the label states
  float* red = gam + 2 * NT;              // [2][16]  per-wave maxima (alpha) / blank occupancy sums (beta)
  float* red2 = red + 32;                 // [2][16]  per-wave sums of all occupancies (beta)
  float* fin = red2 + 32;                 // [4]
  int* lab = reinterpret_cast<int*>(fin + 4);   // [L]
  int* cidx = lab + L;                    // [L]      label positions grouped by class
  int* cstart = cidx + L;                 // [C + 1]

  int Tb = A.in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  int ll = A.labels_len[b];
  ll = ll > L ? L : ll;
  const int U = ll > 1 ? ll - 1 : 0;      // the label row without its trailing EOS
  float* const dzb = A.dz + (long)b * T * ld;
  const float* const zb = A.z + (long)b * T * ld;
  const float* const lp = dzb;            // phase 1 leaves the log-probabilities here
  float* const wsb = A.ws + (long)b * T * (2 * L + 1);
  float* const wsm = wsb + (long)T * 2 * L;

  for (int j = i; j < L; j += NT) lab[j] = A.labels[(long)b * L + j];
  if (i < 2) { exE[i * XS] = exO[i * XS] = -INFINITY; exE[i * XS + NT + 1] = exO[i * XS + NT + 1] = -INFINITY; }
  __syncthreads();
  const bool hasE = i <= U, hasO = i < U;
  const int li = hasO ? lab[i] : 0;
  const bool badi = hasO && (li < 0 || li >= blank);
  const bool repi = hasO && i > 0 && li == lab[i - 1];               // label i repeats label i - 1: no skip over the blank between
  const bool repn = (i + 1 < U) && lab[i + 1] == li;
  {   // feasibility, decided here: T_b >= U + (adjacent equal pairs), T_b >= 1, every label a real class
    int* ired = reinterpret_cast<int*>(red);
    const int nrep = __popcll(__ballot(repi)), nbad = __popcll(__ballot(badi));
    if (lane == 0) { ired[wv] = nrep; ired[16 + wv] = nbad; }
    __syncthreads();
    int reps = 0, bad = 0;
    for (int w = 0; w < nw; ++w) { reps += ired[w]; bad += ired[16 + w]; }
    __syncthreads();                       // (red is reused below)
    if (Tb < 1 || bad || Tb < U + reps) {
      ctc_zero_rows(dzb, ld, C, 0, T);
      if (i == 0) { A.nll[b] = 0.f; A.status[b] = 0; A.utt_loss[b] = 0.f; }
      return;
    }
  }
  ctc_zero_rows(dzb, ld, C, Tb, T);

  // ---- phase 1: log-softmax rows ----------------------------------------------------------------------------------------------
  {
    const int g = i >> 4, j = i & 15, ng = NT >> 4;
    for (int t0 = 0; t0 < Tb; t0 += ng) {
      const int t = t0 + g;
      const bool on = t < Tb;
      const float* zr = zb + (long)(on ? t : 0) * ld;
      float mx = -INFINITY;
      for (int c = j; c < C; c += 16) mx = fmaxf(mx, zr[c]);
      mx = group16_max(mx);
      float s = 0.f;
      for (int c = j; c < C; c += 16) s += expf(zr[c] - mx);
      s = group16_sum(s);
      const float lz = mx + logf(s);
      if (on) for (int c = j; c < C; c += 16) dzb[(long)t * ld + c] = zr[c] - lz;
    }
  }
  // ---- label positions grouped by class (ascending position inside a class) ----------------------------------------------------
  if (i < blank) {
    int n = 0;
    for (int j = 0; j < U; ++j) n += (lab[j] == i);
    cstart[i + 1] = n;
  }
  __syncthreads();                         // (also: phase 1's rows are visible to the whole workgroup)
  if (i == 0) {
    cstart[0] = 0;
    for (int k = 0; k < blank; ++k) cstart[k + 1] += cstart[k];
  }
  __syncthreads();
  if (i < blank) {
    int p = cstart[i];
    for (int j = 0; j < U; ++j) if (lab[j] == i) cidx[p++] = j;
  }

  // ---- phase 2: alpha ----------------------------------------------------------------------------------------------------------
  float e, o;                              // alpha^ of states 2i / 2i + 1
  double msum = 0.0;
  {
    float lpB = lp[blank], lpL = lp[li];
    e = i == 0 ? lpB : -INFINITY;
    o = (i == 0 && hasO) ? lpL : -INFINITY;
    for (int t = 0; t < Tb; ++t) {
      const bool more = t + 1 < Tb;
      if (more) { lpB = lp[(long)(t + 1) * ld + blank]; lpL = lp[(long)(t + 1) * ld + li]; }     // next row: off the chain
      const int buf = t & 1;
      const float mx = wave64_max(fmaxf(e, o));
      exO[buf * XS + i + 1] = o;
      if (lane == 0) red[buf * 16 + wv] = mx;
      lds_barrier();
      float m = red[buf * 16];
      for (int w = 1; w < nw; ++w) m = fmaxf(m, red[buf * 16 + w]);
      if (m == -INFINITY) m = 0.f;
      e -= m; o -= m;
      const float se = e, so = o;
      msum += (double)m;
      if (more) {
        const float om1 = exO[buf * XS + i] - m;                       // label i - 1
        const float ne = hasE ? lpB + ctc_lse2(e, om1) : -INFINITY;
        const float no = hasO ? lpL + ctc_lse3(o, e, repi ? -INFINITY : om1) : -INFINITY;
        e = ne; o = no;
      }
      // (stored last: the wait for the next row's log-probabilities above then has only the previous step's stores ahead of it)
      if (hasE) wsb[(long)t * 2 * L + i] = se;
      if (hasO) wsb[(long)t * 2 * L + L + i] = so;
      if (i == 0) wsm[t] = m;
    }
  }
  // (the loop leaves e, o = alpha^_{T_b - 1}: its last pass computes no successor)
  if (i == U) { fin[0] = e; if (U == 0) fin[1] = -INFINITY; }
  if (U > 0 && i == U - 1) fin[1] = o;
  __syncthreads();
  const float lf = ctc_lse2(fin[0], fin[1]);
  if (!(lf > -INFINITY && lf < INFINITY)) {            // (not reachable with finite logits: the alignment exists)
    ctc_zero_rows(dzb, ld, C, 0, Tb);
    if (i == 0) { A.nll[b] = 0.f; A.status[b] = 0; A.utt_loss[b] = 0.f; }
    return;
  }
  const float inv = 1.f / (A.denom[0] + 1e-12f);       // the sequence loss's normaliser, as avsr_seq_loss_fun applies it
  const float scale = A.weight * inv;
  if (i == 0) {
    const float nll = -(float)(msum + (double)lf);
    A.nll[b] = nll; A.status[b] = 1; A.utt_loss[b] = scale * nll;
  }

  // ---- phase 3: beta, occupancies, dz ------------------------------------------------------------------------------------------
  {
    int t = Tb - 1;
    const int iw = i < L ? i : L - 1, ik = i < C ? i : C - 1;         // (every thread loads, from a valid address: no branches around the prefetch)
    float lpB = lp[(long)t * ld + blank], lpL = lp[(long)t * ld + li];
    float aE = wsb[(long)t * 2 * L + iw], aO = wsb[(long)t * 2 * L + L + iw];
    float lpk = lp[(long)t * ld + ik];
    float mn = 0.f;                                     // m_{t+1}
    float bE = -INFINITY, bO = -INFINITY;               // beta^_{t+1} of states 2i / 2i + 1
    for (; t >= 0; --t) {
      float nlpB = 0.f, nlpL = 0.f, naE = -INFINITY, naO = -INFINITY, nlpk = 0.f, nmn = 0.f;
      if (t > 0) {                                      // row t - 1: off the chain
        nlpB = lp[(long)(t - 1) * ld + blank]; nlpL = lp[(long)(t - 1) * ld + li];
        naE = wsb[(long)(t - 1) * 2 * L + iw];
        naO = wsb[(long)(t - 1) * 2 * L + L + iw];
        nlpk = lp[(long)(t - 1) * ld + ik];
        nmn = wsm[t];
      }
      float nbE, nbO;
      if (t == Tb - 1) {
        nbE = i == U ? lpB - lf : -INFINITY;
        nbO = (U > 0 && i == U - 1) ? lpL - lf : -INFINITY;
      } else {
        const int pb = (t + 1) & 1;
        const float e1 = exE[pb * XS + i + 2], o1 = exO[pb * XS + i + 2];      // blank / label i + 1
        nbE = hasE ? lpB + ctc_lse2(bE, bO) - mn : -INFINITY;
        nbO = hasO ? lpL + ctc_lse3(bO, e1, repn ? -INFINITY : o1) - mn : -INFINITY;
      }
      bE = nbE; bO = nbO;
      const float gE = hasE ? expf(aE + bE - lpB) : 0.f;
      const float gO = hasO ? expf(aO + bO - lpL) : 0.f;
      const int buf = t & 1;
      exE[buf * XS + i + 1] = bE;
      exO[buf * XS + i + 1] = bO;
      gam[buf * NT + i] = gO;
      const float sB = wave64_sum(gE), sA = wave64_sum(gE + gO);
      if (lane == 0) { red[buf * 16 + wv] = sB; red2[buf * 16 + wv] = sA; }
      lds_barrier();
      if (i < C) {
        float G = 0.f, tot = 0.f;
        for (int w = 0; w < nw; ++w) tot += red2[buf * 16 + w];
        if (i == blank) {
          for (int w = 0; w < nw; ++w) G += red[buf * 16 + w];
        } else {
          const int j1 = cstart[i + 1];
          for (int j = cstart[i]; j < j1; ++j) G += gam[buf * NT + cidx[j]];
        }
        dzb[(long)t * ld + i] = scale * (expf(lpk) - (tot > 0.f ? G / tot : 0.f));
      }
      lpB = nlpB; lpL = nlpL; aE = naE; aO = naO; lpk = nlpk; mn = nmn;
    }
  }
}

// per-frame argmax over the C classes, lowest index on ties; frames t >= T_b: -1
__global__ void ctc_best_path_kernel(const float* z, long ld, const int32_t* in_len, int B, int T, int C, int32_t* ids) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (long)B * T) return;
  const int b = (int)(r / T), t = (int)(r - (long)b * T);
  int Tb = in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  if (t >= Tb) { ids[r] = -1; return; }
  const float* zr = z + r * ld;
  float best = zr[0];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = zr[c];
    if (v > best) { best = v; arg = c; }
  }
  ids[r] = arg;
}

static inline int ctc_threads(int L, int C) {
  int n = L > C ? L : C;
  n = (n + 63) / 64 * 64;
  return n < 256 ? 256 : n;
}
static inline size_t ctc_lds_bytes(int NT, int L, int C) {
  return sizeof(float) * (size_t)(4 * (NT + 2) + 2 * NT + 64 + 4) + sizeof(int) * (size_t)(2 * L + C + 1);
}

}  // namespace avsr

using namespace avsr;

extern "C" int64_t avsr_ctc_ws_floats(int32_t B, int32_t T, int32_t L) {
  if (B <= 0 || T <= 0 || L <= 0) return 0;
  return (int64_t)B * T * (2 * (int64_t)L + 1);
}

extern "C" int avsr_ctc_loss(const avsr_ctc_args* a, void* stream) {
  if (!a || !a->z || !a->labels || !a->labels_len || !a->in_len || !a->denom || !a->nll || !a->status || !a->utt_loss || !a->dz || !a->ws)
    return AVSR_ERR_ARG;
  if (a->B <= 0 || a->T <= 0 || a->L <= 0 || a->C < 2 || a->ld < a->C || a->z == a->dz) return AVSR_ERR_ARG;
  if (a->ws_floats < avsr_ctc_ws_floats(a->B, a->T, a->L)) return AVSR_ERR_ARG;
  const int NT = ctc_threads(a->L, a->C);
  if (NT > 1024) return AVSR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(ctc_loss_kernel, dim3(a->B), dim3(NT), ctc_lds_bytes(NT, a->L, a->C), S_(stream), *a);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_ctc_best_path(const float* z, int64_t ld, const int32_t* in_len, int32_t B, int32_t T, int32_t C, int32_t* ids,
                                  void* stream) {
  if (!z || !in_len || !ids || B <= 0 || T <= 0 || C < 1 || ld < C) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(ctc_best_path_kernel, dim3((unsigned)(((long)B * T + 255) / 256)), dim3(256), 0, S_(stream), z, (long)ld, in_len, B,
                     T, C, ids);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

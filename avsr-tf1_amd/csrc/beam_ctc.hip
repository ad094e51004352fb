// Joint CTC / attention scoring inside beam search (avsr_beam_ctc, include/avsr_hip.h): the CTC prefix score of every hypothesis row,
// queued ahead of every selection of avsr_attn_rnn_fwd_ctc.  fp32, gfx950, no atomics: two launches on the same inputs are bit-identical.
//
// Once per decode (beam_ctc_begin_kernel, one workgroup per utterance): y = log_softmax of the head's rows t < T_b over the V + 1 real
// classes (one wave per row), and the empty prefix's state into half 0 of the ping-pong: r_n = -inf, r_b[t] = sum_{u <= t} y[u][blank]
// (the blank column is kept in LDS while the rows are normalised; one thread adds it up in frame order), psi = 0, last = -1.
//
// Per step (beam_ctc_step_kernel, one 256-thread workgroup per hypothesis row r, R = n_utt * beam_width of them):
//   1. state update.  Row r continues row p = parent_rows[r] of half step & 1 with symbol c = tok[r] and writes half (step + 1) & 1.
//      All threads stage phi[t] (r_b of the parent where c == last(parent), else r_n (+) r_b), y[t][c] and y[t][blank] in LDS.  The
//      two recursions are first-order and affine in the probability domain, so each is run as a scan: the 64 lanes of wave 0 walk
//      ceil(T_b / 64) frames each, their chunk maps are combined in 6 shuffle rounds and all threads close the frames in parallel --
//      2 x (8 + 6) dependent log-add steps at T_b = 500 instead of 500 (one thread walking the chain measured 219 us per step of the
//      search).  The row's psi(g.c) is the block-wide log-sum-exp of phi[t - 1] + y[t][c], recomputed here
//      instead of being kept for all K V candidates.  Step 0 (tok = GO: the empty prefix), rows that took EOS and finished rows copy the parent's state through.
//   2. scoring.  psi(g.v) for all V symbols needs no recursion: it is the log-sum-exp over t of phi_v[t - 1] + y[t][v] with phi_v one
//      of two vectors of the row's own new state (v == last: r_b, else r_n (+) r_b), both staged in LDS.  The 256 threads are
//      TG = 256 / CP frame groups x CP columns (CP = V rounded up to a power of two): a thread owns one symbol and every TG-th frame,
//      reads of a frame's y row are contiguous, and it keeps an online (max, sum) pair -- one expf per element, a rescale only when the
//      maximum moves, four frames' loads in flight.  The TG pairs of a symbol meet in LDS and are merged in group order.  psi(g.EOS) = r_n[T_b-1] (+) r_b[T_b-1].
//      term[r][v] = psi(g.v) - psi(g), 0 for every v where psi(g) = -inf, T_b = 0 or the row is finished; never NaN.
//   The selection gets ONE pre-combined buffer extra[r][v] = weight * term + lm_weight * lm_logp (the second part when a language model
//   is fused) and runs as beam_step_kernel<.., LM = true> with weight 1: its instantiations are the ones that run without CTC.
#include "wave.h"
#include "avsr_hip.h"
#include "prof.h"
#include "beam.h"

namespace avsr {

// Inclusive scan, over the 64 lanes of a wave, of the affine maps N -> (N + A) (+) B of the lanes' frame chunks (earlier chunk first);
// returns what enters the lane's chunk when -inf enters the first: the B of the lanes before it composed.
__device__ __forceinline__ float bc_scan_maps(float A, float B, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float Ap = __shfl_up(A, o, 64), Bp = __shfl_up(B, o, 64);
    if (lane >= o) { B = lse2(Bp + A, B); A = Ap + A; }
  }
  const float in = __shfl_up(B, 1, 64);
  return lane == 0 ? -INFINITY : in;
}

// dynamic LDS: T floats
__global__ __launch_bounds__(256) void beam_ctc_begin_kernel(const avsr_beam_ctc A) {
  extern __shared__ __attribute__((aligned(16))) float cum[];      // [T] blank column, then its prefix sum
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = A.T, V = A.V, C = V + 1, K = A.beam_width;
  int Tb = A.in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const float* zb = A.z + (long)b * T * A.ld;
  float* yb = A.y + (long)b * T * C;
  for (int t = wave; t < Tb; t += 4) {
    const float* zr = zb + (long)t * A.ld;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, zr[c]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(zr[c] - mx);
    sum = wave_sum(sum);
    const float lse = mx + logf(sum);
    for (int c = lane; c < C; c += 64) yb[(long)t * C + c] = zr[c] - lse;
    if (lane == 0) cum[t] = zr[V] - lse;
  }
  __syncthreads();
  if (tid == 0) {
    float acc = 0.f;
    for (int t = 0; t < Tb; ++t) { acc += cum[t]; cum[t] = acc; }
  }
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    const long r = (long)b * K + k;
    float2* st = reinterpret_cast<float2*>(A.state) + r * T;           // half 0
    for (int t = tid; t < Tb; t += 256) st[t] = make_float2(-INFINITY, cum[t]);
  }
  if (tid < K) { A.psi[(long)b * K + tid] = 0.f; A.last[(long)b * K + tid] = -1; }
}

// dynamic LDS: 5 T + 520 floats.  CP: V rounded up to a power of two (16 .. 256).
__global__ __launch_bounds__(256) void beam_ctc_step_kernel(const avsr_beam_ctc A, const int32_t* tok, const int32_t* parent_rows,
                                                            const int32_t* fin, int step, int CP) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int T = A.T, V = A.V, C = V + 1, K = A.beam_width, eos = A.eos_id;
  const int R = A.n_utt * K, r = blockIdx.x, b = r / K, tid = threadIdx.x;
  float* sPhi = sm;                  // parent's phi for symbol c; after the update: r'_n (+) r'_b
  float* sYc = sPhi + T;
  float* sYb = sYc + T;
  float* sRn = sYb + T;
  float* sRb = sRn + T;
  float* mM = sRb + T;               // [256] online maxima, [TG][CP]
  float* mS = mM + 256;              // [256] online sums
  float* red = mS + 256;             // [8]
  int Tb = A.in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const int pin = step & 1, pout = (step + 1) & 1;
  int c = tok[r], p = parent_rows[r];
  c = c < 0 ? 0 : (c >= V ? V - 1 : c);                    // what the selection writes lies inside; nothing outside is ever addressed
  p = p < 0 ? 0 : (p >= R ? R - 1 : p);
  const bool dead = fin[r] != 0 || (step > 0 && c == eos);
  const bool copy = dead || step == 0;
  const float2* sin = reinterpret_cast<const float2*>(A.state) + ((long)pin * R + p) * T;
  float2* sout = reinterpret_cast<float2*>(A.state) + ((long)pout * R + r) * T;
  const float* yb = A.y + (long)b * T * C;
  const float ppsi = A.psi[(long)pin * R + p];
  const int plast = A.last[(long)pin * R + p];
  float psi;
  int last;
  if (copy) {
    for (int t = tid; t < Tb; t += 256) { const float2 v = sin[t]; sRn[t] = v.x; sRb[t] = v.y; }
    psi = ppsi; last = plast;
    __syncthreads();
  } else {
    const bool empty = plast < 0, same = c == plast;
    for (int t = tid; t < Tb; t += 256) {
      const float2 v = sin[t];
      sPhi[t] = same ? v.y : lse2(v.x, v.y);
      sYc[t] = yb[(long)t * C + c];
      sYb[t] = yb[(long)t * C + V];
    }
    __syncthreads();
    // r'_n[t] = (r'_n[t-1] (+) phi[t-1]) + y[t][c] is affine in r'_n[t-1] (in the probability domain), so the T_b dependent steps become
    // CH = ceil(T_b / 64) of them: lane l of wave 0 walks frames [l CH, (l + 1) CH) from -inf, keeping per frame the map of its chunk so
    // far -- N -> (N + A[t]) (+) B[t] -- then the lanes' whole-chunk maps are scanned (6 rounds) and every frame is closed in parallel
    // with what enters its chunk.  Only sums of log-probabilities and (+) are formed: nothing cancels.
    const int CH = (Tb + 63) >> 6;
    if (tid < 64) {
      float Am = 0.f, Bv = -INFINITY;
      const int t0 = tid * CH, t1 = min(Tb, t0 + CH);
      for (int t = t0; t < t1; ++t) {
        if (t == 0) { Am = -INFINITY; Bv = empty ? sYc[0] : -INFINITY; }
        else { const float yc = sYc[t]; Bv = lse2(Bv, sPhi[t - 1]) + yc; Am += yc; }
        sRn[t] = Am; sRb[t] = Bv;
      }
      mM[tid] = bc_scan_maps(Am, Bv, tid);
    }
    // psi(g.c): block-wide max-shifted log-sum-exp of x[0] = r'_n[0], x[t] = phi[t - 1] + y[t][c]
    float mx = -INFINITY;
    for (int t = tid; t < Tb; t += 256) mx = fmaxf(mx, t == 0 ? (empty ? sYc[0] : -INFINITY) : sPhi[t - 1] + sYc[t]);
    mx = block_max_256(mx, red);
    float sum = 0.f;
    if (mx != -INFINITY)
      for (int t = tid; t < Tb; t += 256) sum += expf((t == 0 ? (empty ? sYc[0] : -INFINITY) : sPhi[t - 1] + sYc[t]) - mx);
    sum = block_sum_256(sum, red + 4);
    psi = mx == -INFINITY ? -INFINITY : mx + logf(sum);
    last = c;
    __syncthreads();                                                   // wave 0's maps are in LDS; sPhi and sYc are free
    for (int t = tid; t < Tb; t += 256) sRn[t] = lse2(sRb[t], mM[t / CH] + sRn[t]);
    __syncthreads();
    // r'_b[t] = (r'_n[t-1] (+) r'_b[t-1]) + y[t][blank], r'_b[0] = -inf: the same, on the finished r'_n (A goes to sYc, B to sRb)
    if (tid < 64) {
      float Am = 0.f, Bv = -INFINITY;
      const int t0 = tid * CH, t1 = min(Tb, t0 + CH);
      for (int t = t0; t < t1; ++t) {
        if (t == 0) { Am = -INFINITY; Bv = -INFINITY; }
        else { const float ybl = sYb[t]; Bv = lse2(Bv, sRn[t - 1]) + ybl; Am += ybl; }
        sYc[t] = Am; sRb[t] = Bv;
      }
      mS[tid] = bc_scan_maps(Am, Bv, tid);
    }
    __syncthreads();
    for (int t = tid; t < Tb; t += 256) sRb[t] = lse2(sRb[t], mS[t / CH] + sYc[t]);
    __syncthreads();
  }
  for (int t = tid; t < Tb; t += 256) {
    const float rn = sRn[t], rb = sRb[t];
    sout[t] = make_float2(rn, rb);
    sPhi[t] = lse2(rn, rb);
  }
  if (tid == 0) { A.psi[(long)pout * R + r] = psi; A.last[(long)pout * R + r] = last; }
  float* term = A.term + (long)r * V;
  float* extra = A.extra + (long)r * V;
  if (dead || Tb == 0 || psi == -INFINITY) {                           // (uniform over the workgroup)
    const bool lm = A.lm_logp && !dead;
    for (int v = tid; v < V; v += 256) {
      term[v] = 0.f;
      extra[v] = lm ? A.lm_weight * A.lm_logp[(long)r * V + v] : 0.f;
    }
    return;
  }
  __syncthreads();
  // ---- scoring: thread (tg, col) owns symbol col and the frames 1 + tg, 1 + tg + TG, ... ----
  const int col = tid & (CP - 1), tg = tid / CP, TG = 256 / CP;
  float m = -INFINITY, s = 0.f;
  if (col < V) {
    const float* ph = col == last ? sRb : sPhi;
    if (tg == 0 && last < 0) { m = yb[col]; s = 1.f; }                 // r'_n[0] of the empty prefix's extensions
    for (int t = 1 + tg; t < Tb; t += 4 * TG) {                          // four frames' loads in flight, then their updates in frame order
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int tu = t + u * TG;
        x[u] = tu < Tb ? ph[tu - 1] + yb[(long)tu * C + col] : -INFINITY;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (x[u] > m) { s = s * expf(m - x[u]) + 1.f; m = x[u]; }
        else if (x[u] != -INFINITY) s += expf(x[u] - m);
      }
    }
  }
  mM[tid] = m; mS[tid] = s;
  __syncthreads();
  if (tid < V) {
    float M = -INFINITY;
    for (int g = 0; g < TG; ++g) M = fmaxf(M, mM[g * CP + tid]);
    float pv;
    if (tid == eos) pv = sPhi[Tb - 1];
    else if (M == -INFINITY) pv = -INFINITY;
    else {
      float S = 0.f;
      for (int g = 0; g < TG; ++g) { const float mg = mM[g * CP + tid]; if (mg != -INFINITY) S += mS[g * CP + tid] * expf(mg - M); }
      pv = M + logf(S);
    }
    const float tv = pv - psi;
    term[tid] = tv;
    extra[tid] = A.weight * tv + (A.lm_logp ? A.lm_weight * A.lm_logp[(long)r * V + tid] : 0.f);
  }
}

// extra = weight * term (+ lm_weight * lm_logp): the pre-combined buffer of avsr_beam_search_step_ctc
__global__ void beam_ctc_combine_kernel(const float* term, float weight, const float* lm_logp, float lm_weight, float* extra, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    extra[i] = weight * term[i] + (lm_logp ? lm_weight * lm_logp[i] : 0.f);
}

// AVSR_OK, or why the step cannot run (decided on the host, nothing dereferenced)
int beam_ctc_check(const avsr_beam_ctc* c) {
  if (!c || c->n_utt <= 0 || c->beam_width <= 0 || c->T <= 0 || c->V <= 1 || c->eos_id < 0 || c->eos_id >= c->V) return AVSR_ERR_ARG;
  if (!(c->weight >= 0.f) || !(c->weight <= 3.0e38f) || c->ld < c->V + 1) return AVSR_ERR_ARG;
  if (!c->z || !c->in_len || !c->y || !c->state || !c->psi || !c->last || !c->term || !c->extra) return AVSR_ERR_ARG;
  if (c->T > AVSR_BEAM_CTC_MAX_T || c->V > AVSR_BEAM_CTC_MAX_V || c->beam_width > 64) return AVSR_ERR_UNSUPPORTED;
  if ((long)c->n_utt * c->beam_width * c->T >= (1L << 28) || (long)c->n_utt * c->T * c->ld >= (1L << 30)) return AVSR_ERR_UNSUPPORTED;
  return AVSR_OK;
}

int beam_ctc_begin_launch(const avsr_beam_ctc& c, hipStream_t s) {
  ProfScope ps(PROF_STEP_LINEAR, s);
  hipLaunchKernelGGL(beam_ctc_begin_kernel, dim3(c.n_utt), dim3(256), sizeof(float) * c.T, s, c);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

int beam_ctc_step_launch(const avsr_beam_ctc& c, const int32_t* tok, const int32_t* parent_rows, const int32_t* fin, int step, hipStream_t s) {
  ProfScope ps(PROF_STEP_LINEAR, s);
  int CP = 16;
  while (CP < c.V) CP <<= 1;
  hipLaunchKernelGGL(beam_ctc_step_kernel, dim3(c.n_utt * c.beam_width), dim3(256), sizeof(float) * (5 * (size_t)c.T + 520), s, c, tok,
                     parent_rows, fin, step, CP);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

int beam_ctc_combine_launch(const float* term, float weight, const float* lm_logp, float lm_weight, float* extra, long n, hipStream_t s) {
  hipLaunchKernelGGL(beam_ctc_combine_kernel, dim3(blocks_for(n)), dim3(256), 0, s, term, weight, lm_logp, lm_weight, extra, n);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

}  // namespace avsr

extern "C" int avsr_beam_ctc_supported(const avsr_beam_ctc* ctc) { return avsr::beam_ctc_check(ctc) == AVSR_OK ? 1 : 0; }

extern "C" int avsr_beam_ctc_begin(const avsr_beam_ctc* ctc, void* stream) {
  const int rc = avsr::beam_ctc_check(ctc);
  if (rc) return rc;
  return avsr::beam_ctc_begin_launch(*ctc, (hipStream_t)stream);
}

extern "C" int avsr_beam_ctc_step(const avsr_beam_ctc* ctc, const int32_t* tok, const int32_t* parent_rows, const int32_t* fin, int32_t step,
                                  void* stream) {
  if (!ctc || !tok || !parent_rows || !fin || step < 0) return AVSR_ERR_ARG;
  const int rc = avsr::beam_ctc_check(ctc);
  if (rc) return rc;
  return avsr::beam_ctc_step_launch(*ctc, tok, parent_rows, fin, step, (hipStream_t)stream);
}

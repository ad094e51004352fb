// Beam search: the selection step and the final gather_tree.  ONE launch site for the step (beam_step_launch): the decoder's scheduler
// (attn_rnn.hip, mode 3) and the avsr_beam_search_step* entries fill a BeamStep (beam.h) and go through it: the tests run what the model runs.
#include "beam.h"

namespace avsr {

// One BeamSearchDecoder step for one utterance (one 256-thread workgroup per utterance): see avsr_hip.h mode 3 and
// oracle.beam_search_decode.  Everything the step reads comes in with ONE round of loads; the per-beam log-sum-exp is a wave reduction,
// its logf / the 2 K length penalties (powf) run one per lane side by side; every thread keeps its (at most two) candidates
// -- score as a sortable 32-bit key, accumulated log-probability -- in REGISTERS, and the top K are K rounds of
// {wave arg-max of a 64-bit (score key, ~index) word, four wave winners through LDS}: larger score first, LOWER index on ties
// (= tf.nn.top_k's order; -inf scores stay selectable, in index order).
// History, measured at c4 (B * K = 640 rows, V = 31; profiles/r04_beam_gemm_dissect.txt): round 2 one thread selecting serially 165 us;
// round 3 one wave, candidates in LDS, parents' flags loaded inside every round 22 us; rank by counting (every candidate against
// every other, broadcast LDS reads) 28 us -- 310 x 310 comparisons are more instructions than ten reductions.
// NCT > 0: the output layer runs here too (seq2seq.py:339 the decoder's Dense(vocab) under BeamSearchDecoder): the utterance's K rows of
// the attention output [K x O] times Wout^T [O x V] as NCT 16-column tiles of v_mfma_f32_16x16x4_f32, wave w taking the O / 4 inputs
// [w O / 4, (w + 1) O / 4), the four partial tiles summed through LDS -- one launch and one read-back of the logits less per step
// (the separate projection was a 7 us launch of 640 x 31 outputs).  Needs K <= 16, V <= 16 NCT, O % 256 == 0.  NCT == 0: logits given.
// LM: shallow fusion (avsr_beam_lm): an unfinished beam's step log-probability gets + lm_weight * lm_logp[row][v], lm_logp = the
// language model's log_softmax [B * K][V] (beam_lm.hip).  Weight 0 takes the branch without the term, so the search is bit for bit the
// one without a model; LM == false compiles the term out (lm_logp / lm_weight unused): the instruction stream of the search as it was.
template <int NCT, bool LM>
__global__ __launch_bounds__(256) void beam_step_kernel(float* logits, long logits_sb, int V, int K, int l, int eos, float w,
                                 const float* logp_in, const int32_t* fin_in, const int32_t* len_in,
                                 float* logp_out, int32_t* fin_out, int32_t* len_out, int32_t* tok, int32_t* parent_rows,
                                 int32_t* step_ids, int32_t* parent_ids, int32_t* n_unfinished,
                                 const float* xa, long xsb, int O, const float* wout_t, const float* bout,
                                 const float* lm_logp, float lm_weight) {
  extern __shared__ __attribute__((aligned(16))) float sm[];   // logits [K*V] | lse [K] | max [K] | sum [K] | penalties [K][2] | fin [K] | len [K] | logp [K] | alive | winners [2][4] x 64 bit
  const int n = K * V;
  float* lg_s = sm;
  float* lse_s = lg_s + n;
  float* mx_s = lse_s + K;
  float* sum_s = mx_s + K;
  float* pen = sum_s + K;
  int* fin_s = reinterpret_cast<int*>(pen + 2 * K);
  int* len_s = fin_s + K;
  float* logp_s = reinterpret_cast<float*>(len_s + K);
  int* alive_s = reinterpret_cast<int*>(logp_s + K);
  unsigned long long* win = reinterpret_cast<unsigned long long*>(sm + ((n + 8 * K + 1 + 1) & ~1));      // 8-byte aligned
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float FMIN = -3.4028234663852886e38f;
  // Steps queued past the end of the search (the host reads the "all finished" counter a chunk late): dynamic_decode has stopped, so
  // the step hands its input state through unchanged.  Without this a beam that finished at the last real step would be re-scored with
  // len + 1 and the beams re-ordered -- harmless for gather_tree (it reads step_ids / parent_ids [:T] and the maximum length) but not for
  // a caller reading the per-beam state afterwards.  n_unfinished[-1] is the previous step's count, complete when this launch starts.
  if (l > 0 && n_unfinished[-1] == 0) {
    if (tid < K) {
      const int r = b * K + tid;
      logp_out[r] = logp_in[r]; fin_out[r] = fin_in[r]; len_out[r] = len_in[r];
      tok[r] = eos; parent_rows[r] = r; step_ids[r] = eos; parent_ids[r] = tid;
    }
    return;
  }
  if (tid < K) { fin_s[tid] = fin_in[b * K + tid]; len_s[tid] = len_in[b * K + tid]; logp_s[tid] = logp_in[b * K + tid]; }
  if (tid == 0) alive_s[0] = 0;
  if constexpr (NCT > 0) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    float* part = reinterpret_cast<float*>(win + 8);               // [4 waves][16 rows][16 NCT columns]
    const int i16 = lane & 15, g = lane >> 4, kw = O >> 2;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float* xr = xa + (long)(b * K + (i16 < K ? i16 : 0)) * xsb + wave * kw + 4 * g;
    const float* wr[NCT];
    f32x4 acc[NCT];
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      const int v = c * 16 + i16;
      wr[c] = wout_t + (long)(v < V ? v : 0) * O + wave * kw + 4 * g;
      acc[c] = zero;
    }
    const bool arow = i16 < K;
#pragma unroll 1
    for (int kk = 0; kk < kw; kk += 64) {                         // lane (i16, g) holds inputs kk + 16 u + 4 g .. + 3 of row / column i16
      f32x4 a[4], bv[4][NCT];                                     // (all loads of four 16-input groups in flight, then their products)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = *reinterpret_cast<const f32x4*>(xr + kk + 16 * u);
#pragma unroll
        for (int c = 0; c < NCT; ++c) bv[u][c] = *reinterpret_cast<const f32x4*>(wr[c] + kk + 16 * u);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!arow) a[u] = zero;
#pragma unroll
        for (int c = 0; c < NCT; ++c) if (c * 16 + i16 >= V) bv[u][c] = zero;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < NCT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], bv[u][c][e], acc[c], 0, 0, 0);
      }
    }
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(wave * 16 + 4 * g + r) * (16 * NCT) + c * 16 + i16] = acc[c][r];
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const int k = i / V, v = i - k * V, o = k * (16 * NCT) + v;
      const float sv = ((part[o] + part[256 * NCT + o]) + (part[512 * NCT + o] + part[768 * NCT + o])) + bout[v];
      lg_s[i] = sv;
      logits[(long)(b * K + k) * logits_sb + v] = sv;
    }
  } else {
    for (int i = tid; i < n; i += 256) {
      const int k = i / V, v = i - k * V;
      lg_s[i] = logits[(long)(b * K + k) * logits_sb + v];
    }
  }
  __syncthreads();
  for (int k = wave; k < K; k += 4) {                 // max and exp-sum of beam k: wave reductions over its V logits
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, lg_s[k * V + v]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += expf(lg_s[k * V + v] - mx);
    sum = wave_sum(sum);
    if (lane == 0) { mx_s[k] = mx; sum_s[k] = sum; }
  }
  __syncthreads();
  // one logf / powf per lane: K log-sum-exps on wave 0, the 2 K length penalties ((5 + len) / 6) ^ w of the two possible lengths of a
  // beam's continuations on waves 1-3 (the same powf values as one call per candidate)
  if (tid < K) lse_s[tid] = mx_s[tid] + logf(sum_s[tid]);
  for (int j = tid - 64; j >= 0 && j < 2 * K; j += 192) pen[j] = powf((5.0f + (float)(len_s[j >> 1] + (j & 1))) / 6.0f, w);
  __syncthreads();
  // ---- this thread's candidates i = tid + 256 c: key (0 = none / taken) and accumulated log-probability, in registers ----
  constexpr int NC = 4;                               // K * V <= 1024
  unsigned key[NC];
  float tot[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int i = tid + 256 * c;
    key[c] = 0u; tot[c] = 0.f;
    if (i < n) {
      const int k = i / V, v = i - k * V;
      const bool fin = fin_s[k] != 0;
      float sl = fin ? (v == eos ? 0.f : FMIN) : lg_s[i] - lse_s[k];
      if constexpr (LM) {
        if (!fin && lm_weight != 0.f) sl += lm_weight * lm_logp[(long)(b * K + k) * V + v];
      }
      const float t = logp_s[k] + sl;
      const float sc = t / pen[2 * k + ((fin || v == eos) ? 0 : 1)];
      const unsigned u = __builtin_bit_cast(unsigned, sc);
      key[c] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);        // monotone in the score; -inf -> 0x007fffff (> 0 = none)
      tot[c] = t;
    }
  }
  int alive = 0;
  for (int j = 0; j < K; ++j) {
    // this thread's best remaining candidate as one 64-bit word: (score key, ~index) -- larger is better, lower index wins ties
    unsigned long long best = 0ull;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const unsigned long long cand = key[c] ? (((unsigned long long)key[c] << 32) | (unsigned)(0xffffffffu - (unsigned)(tid + 256 * c))) : 0ull;
      best = cand > best ? cand : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned hi = (unsigned)__shfl_xor((int)(best >> 32), o, 64), lo = (unsigned)__shfl_xor((int)(unsigned)best, o, 64);
      const unsigned long long other = ((unsigned long long)hi << 32) | lo;
      best = other > best ? other : best;
    }
    unsigned long long* slot = win + (j & 1) * 4;
    if (lane == 0) slot[wave] = best;
    __syncthreads();
    unsigned long long g = slot[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) g = slot[q] > g ? slot[q] : g;
    const int idx = (int)(0xffffffffu - (unsigned)g);
    if ((idx & 255) == tid) {                           // the owner writes hypothesis j and retires the candidate
      const int c = idx >> 8;
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < NC; ++q) if (q == c) { t = tot[q]; key[q] = 0u; }
      const int word = idx % V, parent = idx / V, r = b * K + j, pr = b * K + parent;
      const bool pf = fin_s[parent] != 0;
      const int f = (pf || word == eos) ? 1 : 0;
      logp_out[r] = t;
      fin_out[r] = f;
      len_out[r] = len_s[parent] + (pf ? 0 : 1);
      tok[r] = word;
      parent_rows[r] = pr;
      step_ids[r] = word;
      parent_ids[r] = parent;
      if (!f) ++alive;
    }
  }
  if (alive) atomicAdd(alive_s, alive);
  __syncthreads();
  if (tid == 0 && alive_s[0]) atomicAdd(n_unfinished, alive_s[0]);
}

__global__ void beam_gather_tree_kernel(const int32_t* step_ids, const int32_t* parent_ids, const int32_t* beam_len, int32_t* out,
                                        int nutt, int K, int T, int eos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nutt * K) return;
  const int b = i / K, k = i % K, R = nutt * K;
  int ml = 0;
  for (int j = 0; j < K; ++j) ml = max(ml, beam_len[b * K + j]);
  ml = min(ml, T);
  int32_t* o = out + (long)b * T * K + k;              // out[b][t][k]
  for (int t = 0; t < T; ++t) o[(long)t * K] = eos;
  if (ml <= 0) return;
  int parent = parent_ids[(long)(ml - 1) * R + b * K + k];
  o[(long)(ml - 1) * K] = step_ids[(long)(ml - 1) * R + b * K + k];
  for (int level = ml - 2; level >= 0; --level) {
    o[(long)level * K] = step_ids[(long)level * R + b * K + parent];
    parent = parent_ids[(long)level * R + b * K + parent];
  }
  bool seen = false;
  for (int t = 0; t < ml; ++t) {
    if (seen) o[(long)t * K] = eos;
    else if (o[(long)t * K] == eos) seen = true;
  }
}

template <int NCT, bool LM>
static void beam_step_go(const BeamStep& s, hipStream_t st) {
  hipLaunchKernelGGL((beam_step_kernel<NCT, LM>), dim3(s.n_utt), dim3(256), (s.K * s.V + 8 * s.K + 24 + 1024 * NCT) * sizeof(float), st,
                     s.logits, s.logits_sb, s.V, s.K, s.step, s.eos, s.length_penalty, s.logp_in, s.fin_in, s.len_in, s.logp_out, s.fin_out,
                     s.len_out, s.tok, s.parent_rows, s.step_ids + (long)s.step * s.n_utt * s.K, s.parent_ids + (long)s.step * s.n_utt * s.K, s.n_unfinished + s.step,
                     s.x, s.x_sb, s.O, s.wout_t, s.bout, s.extra, s.extra_weight);
}

int beam_step_launch(const BeamStep& s, bool allow_inside, hipStream_t st) {
  if (!beam_step_fits(s.K, s.V)) return AVSR_ERR_UNSUPPORTED;
  int nct = 0;
  if (allow_inside && s.x) {
    if (!s.wout_t || !s.bout || s.O <= 0) return AVSR_ERR_ARG;
    if (!(nct = beam_step_nct(s))) return AVSR_ERR_UNSUPPORTED;
  }
  if (s.extra) { if (nct == 2) beam_step_go<2, true>(s, st); else if (nct == 4) beam_step_go<4, true>(s, st); else beam_step_go<0, true>(s, st); }
  else { if (nct == 2) beam_step_go<2, false>(s, st); else if (nct == 4) beam_step_go<4, false>(s, st); else beam_step_go<0, false>(s, st); }
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

}  // namespace avsr

extern "C" int avsr_beam_gather_tree(const int32_t* step_ids, const int32_t* parent_ids, const int32_t* beam_len, int32_t* out,
                                     int32_t n_utt, int32_t beam_width, int32_t T, int32_t eos_id, void* stream) {
  using namespace avsr;
  if (!step_ids || !parent_ids || !beam_len || !out || n_utt <= 0 || beam_width <= 0 || T <= 0) return AVSR_ERR_ARG;
  const int n = n_utt * beam_width;
  hipLaunchKernelGGL(beam_gather_tree_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, step_ids, parent_ids, beam_len, out,
                     n_utt, beam_width, T, eos_id);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// The launch avsr_attn_rnn_fwd (mode 3) issues, on its own: logits given, or the output layer inside the step (x != NULL).
extern "C" int avsr_beam_search_step_lm(float* logits, int32_t n_utt, int32_t beam_width, int32_t V, int32_t step, int32_t eos_id,
                                        float length_penalty_weight, const float* logp_in, const int32_t* fin_in, const int32_t* len_in,
                                        float* logp_out, int32_t* fin_out, int32_t* len_out, int32_t* tok, int32_t* parent_rows,
                                        int32_t* step_ids, int32_t* parent_ids, int32_t* n_unfinished, const float* x, int64_t x_stride,
                                        int32_t O, const float* wout_t, const float* bout, const float* lm_logp, float lm_weight,
                                        void* stream) {
  if (!logits || !logp_in || !fin_in || !len_in || !logp_out || !fin_out || !len_out || !tok || !parent_rows || !step_ids || !parent_ids ||
      !n_unfinished || n_utt <= 0 || beam_width <= 0 || V <= 0 || step < 0 || eos_id < 0 || eos_id >= V)
    return AVSR_ERR_ARG;
  const avsr::BeamStep s{logits, (long)V, n_utt, beam_width, V, step, eos_id, length_penalty_weight, logp_in, fin_in, len_in, logp_out, fin_out,
                         len_out, tok, parent_rows, step_ids, parent_ids, n_unfinished, x, (long)x_stride, O, wout_t, bout, lm_logp, lm_weight};
  return avsr::beam_step_launch(s, true, (hipStream_t)stream);
}

extern "C" int avsr_beam_search_step_ctc(float* logits, int32_t n_utt, int32_t beam_width, int32_t V, int32_t step, int32_t eos_id,
                                         float length_penalty_weight, const float* logp_in, const int32_t* fin_in, const int32_t* len_in,
                                         float* logp_out, int32_t* fin_out, int32_t* len_out, int32_t* tok, int32_t* parent_rows,
                                         int32_t* step_ids, int32_t* parent_ids, int32_t* n_unfinished, const float* x, int64_t x_stride,
                                         int32_t O, const float* wout_t, const float* bout, const float* lm_logp, float lm_weight,
                                         const float* ctc_term, float ctc_weight, float* extra, void* stream) {
  if (ctc_term && ctc_weight != 0.f) {
    if (!extra || !(ctc_weight > 0.f) || n_utt <= 0 || beam_width <= 0 || V <= 0) return AVSR_ERR_ARG;
    const int rc = avsr::beam_ctc_combine_launch(ctc_term, ctc_weight, lm_weight != 0.f ? lm_logp : nullptr, lm_weight, extra,
                                                 (long)n_utt * beam_width * V, (hipStream_t)stream);
    if (rc) return rc;
    lm_logp = extra;
    lm_weight = 1.f;
  }
  return avsr_beam_search_step_lm(logits, n_utt, beam_width, V, step, eos_id, length_penalty_weight, logp_in, fin_in, len_in, logp_out, fin_out,
                                  len_out, tok, parent_rows, step_ids, parent_ids, n_unfinished, x, x_stride, O, wout_t, bout, lm_logp, lm_weight,
                                  stream);
}

extern "C" int avsr_beam_search_step(float* logits, int32_t n_utt, int32_t beam_width, int32_t V, int32_t step, int32_t eos_id,
                                     float length_penalty_weight, const float* logp_in, const int32_t* fin_in, const int32_t* len_in,
                                     float* logp_out, int32_t* fin_out, int32_t* len_out, int32_t* tok, int32_t* parent_rows,
                                     int32_t* step_ids, int32_t* parent_ids, int32_t* n_unfinished, const float* x, int64_t x_stride,
                                     int32_t O, const float* wout_t, const float* bout, void* stream) {
  return avsr_beam_search_step_lm(logits, n_utt, beam_width, V, step, eos_id, length_penalty_weight, logp_in, fin_in, len_in, logp_out, fin_out,
                                  len_out, tok, parent_rows, step_ids, parent_ids, n_unfinished, x, x_stride, O, wout_t, bout, nullptr, 0.f, stream);
}

// Attention rescoring of the CTC n-best (decoding_algorithm='attention_rescoring'; the rule is INTEGRATION.md section 8): the two small
// kernels behind the teacher-forced decoder passes.  fp32, gfx950, no atomics, every reduction in a fixed order: two launches on the
// same inputs are bit-identical.
//
// avsr_seq_logprob: out[b * out_stride] = sum_{t < min(labels_len[b], L)} log_softmax(logits[b][t])[labels[b][t]].  Forward only (nothing
//   like avsr_seq_loss_fun's B * L * V d logits is written, no normaliser).  One 256-thread workgroup per utterance; wave w takes the rows
//   t = w, w + 4, ...: a row (V <= 1024) is read ONCE into registers, 64 * NCH wide, its maximum and the sum of exp(x - max) are wave
//   reductions (wave.h: DPP rows, the four row results in a fixed order), the label's logit is one more (uniform) load.  A wave adds its
//   rows in ascending t, the four wave sums are combined as (0 + 1) + (2 + 3): the geometry is part of the definition, not a tuning knob.
//   Bandwidth bound: B * L * V floats read once (c2: 64 x 152 x 41 = 1.6 MB), B floats written.
// avsr_rescore_select: per utterance final[k] = s_att[k] (+ weight * s_ctc[k]) over the first n[b] slots and their stable sort, largest
//   first, ties to the lower k: ONE wave per utterance, lane k ranks its own entry against the others (K <= 64 uniform lane reads).
//   The product and the sum are rounded separately (no fused multiply-add), so final is the fp32 expression as written.
#include "wave.h"
#include "avsr_hip.h"

namespace avsr {

template <int NCH>
__global__ __launch_bounds__(256) void seq_logprob_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ labels_len, int L, int V, float* __restrict__ out,
                                                          long out_stride) {
  __shared__ float part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  int n = labels_len[b];
  n = n < 0 ? 0 : (n > L ? L : n);
  float acc = 0.f;
  for (int t = wave; t < n; t += 4) {                                  // (wave-uniform trip count: no divergence around the reductions)
    const float* row = logits + ((long)b * L + t) * V;
    float x[NCH];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int v = c * 64 + lane;
      x[c] = v < V ? row[v] : -INFINITY;
      m = fmaxf(m, x[c]);
    }
    m = wave64_max(m);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) s += expf(x[c] - m);                   // exp(-inf) = 0 for the lanes past V; the maximum contributes 1
    s = wave64_sum(s);
    const int lab = labels[(long)b * L + t];
    // a label outside 0 .. V-1 is never dereferenced: it contributes -inf
    const float lp = (lab >= 0 && lab < V) ? (row[lab] - m) - logf(s) : -INFINITY;
    acc += lp;
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (tid == 0) out[(long)b * out_stride] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(64) void rescore_select_kernel(const float* __restrict__ s_att, const float* __restrict__ s_ctc,
                                                            const int32_t* __restrict__ n, int K, float weight,
                                                            int32_t* __restrict__ order, float* __restrict__ final_out) {
  const int k = threadIdx.x, b = blockIdx.x;
  int nb = n[b];
  nb = nb < 0 ? 0 : (nb > K ? K : nb);
  const bool valid = k < nb;
  float f = -INFINITY;
  if (valid) {
#pragma clang fp contract(off)                                         // (hipcc contracts a * b + c by default, also through __fmul_rn)
    f = s_att[(long)b * K + k];
    if (weight != 0.f) {
      const float prod = weight * s_ctc[(long)b * K + k];
      f = f + prod;
    }
  }
  const float key = f == f ? f : -INFINITY;                            // (a NaN would rank nowhere: the order stays a permutation)
  int rank = 0;
  for (int j = 0; j < nb; ++j) {                                       // nb is wave-uniform, j a uniform lane index
    const float o = rdlane_f(key, j);
    rank += (o > key || (o == key && j < k)) ? 1 : 0;
  }
  if (k < K) {
    const int slot = valid ? rank : k;                                 // ranks fill 0 .. nb-1, the empty slots stay where they are
    order[(long)b * K + slot] = valid ? k : -1;
    final_out[(long)b * K + slot] = f;
  }
}

}  // namespace avsr

extern "C" int avsr_seq_logprob(const float* logits, const int32_t* labels, const int32_t* labels_len, int32_t B, int32_t L, int32_t V,
                                float* out, int64_t out_stride, void* stream) {
  using namespace avsr;
  if (!logits || !labels || !labels_len || !out || B <= 0 || L <= 0 || V < 2 || out_stride < 1) return AVSR_ERR_ARG;
  if (V > 1024) return AVSR_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (V <= 64) hipLaunchKernelGGL(seq_logprob_kernel<1>, dim3(B), dim3(256), 0, s, logits, labels, labels_len, L, V, out, (long)out_stride);
  else if (V <= 256) hipLaunchKernelGGL(seq_logprob_kernel<4>, dim3(B), dim3(256), 0, s, logits, labels, labels_len, L, V, out, (long)out_stride);
  else hipLaunchKernelGGL(seq_logprob_kernel<16>, dim3(B), dim3(256), 0, s, logits, labels, labels_len, L, V, out, (long)out_stride);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_rescore_select(const float* s_att, const float* s_ctc, const int32_t* n, int32_t B, int32_t K, float weight,
                                   int32_t* order, float* final_out, void* stream) {
  using namespace avsr;
  if (!s_att || !s_ctc || !n || !order || !final_out || B <= 0 || K < 1 || K > 64) return AVSR_ERR_ARG;
  if (!(weight >= 0.f) || weight > 3.0e38f) return AVSR_ERR_ARG;      // negative, NaN, inf
  hipLaunchKernelGGL(rescore_select_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, s_att, s_ctc, n, K, weight, order, final_out);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

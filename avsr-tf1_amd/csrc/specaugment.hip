// SpecAugment on an encoder's input (spec_augment; not in the reference; the rule is INTEGRATION.md section 8): frequency bands and time
// spans of x [B, T, F_in] replaced by zero or by the utterance's own column mean, drawn anew from the step's device-side key.
//   y [B, T, F] contiguous, F >= F_in: EVERY element is written -- unmasked elements bit for bit, padding columns and rows beyond len as
//   zeros; x is never modified (it is the captured graph's input).
// Launches, all on the caller's stream, no host read, no memset / memcpy, no atomics (two runs give identical bits):
//   'mean' fill  sa_partial_kernel   grid (row chunks, B): column sums of the chunk's valid rows -> part [B][chunks][F_in]   (reads x once)
//                sa_mean_kernel      one thread per (b, column): the chunks' sums added in chunk order in fp64, / n, rounded once
//                sa_apply_kernel     grid (row chunks, B): the draw, then copy / fill                          (reads x again, writes y)
//   'zero' fill  sa_apply_kernel alone                                                                    (reads x once, writes y once)
// A bandwidth kernel: the grid runs over utterances x row chunks (>= 1024 workgroups where the rows allow, not one per utterance), a
// thread owns four adjacent columns (their band flags and fill values are computed once) and keeps four rows' 16-byte loads in flight.
// 16-byte access where F_in, ld and the base address allow it (loads) and where F does (stores); otherwise element by element.
// The draw (all uint32): the 2 x 8 (start, end) pairs of an utterance are computed by 16 threads of every workgroup into LDS.
#include "common.h"
#include "avsr_hip.h"

namespace avsr {

#define SA_MAX_MASKS AVSR_SPEC_AUGMENT_MAX_MASKS

struct SaArgs {
  const float* x; const int32_t* len; const int32_t* seed; float* y; float* part; float* mean;
  long ld;
  int B, T, F_in, F, rc, nchunk;
  int n_freq, freq_width, P, n_time, time_width;
  uint32_t ratio_q16, s_freq, s_time;
  int mean_fill;
};

__device__ __forceinline__ int sa_len(const SaArgs& A, int b) {
  const int n = A.len[b];
  return n < 0 ? 0 : (n > A.T ? A.T : n);
}

// lo / hi [16]: time masks in slots 0..7 (rows lo <= t < hi), bands in slots 8..15 (bins lo <= c % P < hi); unused slots are empty
__device__ __forceinline__ void sa_draw(const SaArgs& A, int b, int n, int* lo, int* hi) {
  const int k = threadIdx.x;
  if (k < 2 * SA_MAX_MASKS) {
    const bool time = k < SA_MAX_MASKS;
    const int m = time ? k : k - SA_MAX_MASKS;
    int a = 0, w = 0;
    if (m < (time ? A.n_time : A.n_freq)) {
      const uint32_t seed = (uint32_t)A.seed[0], stream = time ? A.s_time : A.s_freq;
      const uint32_t span = time ? (uint32_t)n : (uint32_t)A.P;
      const uint32_t lim = time ? ((uint32_t)n * A.ratio_q16) >> 16 : span;          // n <= 65535, ratio_q16 <= 65536: no overflow
      const uint32_t width = (uint32_t)(time ? A.time_width : A.freq_width);
      const uint32_t cap = width < lim ? width : lim;                                // <= span
      const uint32_t idx = ((uint32_t)b * 64u + (uint32_t)m) * 2u;
      const uint32_t ww = hash_u32(seed, stream, idx) % (cap + 1u);
      a = (int)(hash_u32(seed, stream, idx + 1u) % (span - ww + 1u));
      w = (int)ww;
    }
    lo[k] = a; hi[k] = a + w;
  }
  __syncthreads();
}

template <bool VEC>
__device__ __forceinline__ f32x4 sa_load(const float* p, int c0, int width) {
  if (VEC) return c0 < width ? ld4(p) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = c0 + j < width ? p[j] : 0.f;
  return v;
}
template <bool VEC>
__device__ __forceinline__ void sa_store(float* p, int c0, int width, f32x4 v) {
  if (VEC) { if (c0 < width) st4(p, v); return; }
#pragma unroll
  for (int j = 0; j < 4; ++j) if (c0 + j < width) p[j] = v[j];
}

// thread -> (column quad q, row group g of G): Q quads; Q < 256: G = 256 / Q groups share the block, else every thread walks quads
struct SaMap { int q, qstep, g, G; };
__device__ __forceinline__ SaMap sa_map(int Q) {
  SaMap M;
  if (Q < 256) { M.G = 256 / Q; M.g = (int)threadIdx.x / Q; M.q = (int)threadIdx.x - M.g * Q; M.qstep = Q; }
  else { M.G = 1; M.g = 0; M.q = (int)threadIdx.x; M.qstep = 256; }
  return M;
}

template <bool VI>
__global__ __launch_bounds__(256) void sa_partial_kernel(const SaArgs A) {
  __shared__ f32x4 red[256];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int n = sa_len(A, b);
  const int r0 = chunk * A.rc, r1 = min(n, r0 + A.rc);
  const int Q = (A.F_in + 3) >> 2;
  const SaMap M = sa_map(Q);
  const float* xb = A.x + (long)b * A.T * A.ld;
  float* out = A.part + ((long)b * A.nchunk + chunk) * A.F_in;
  for (int q0 = 0; q0 < Q; q0 += M.qstep) {               // (G > 1: one pass)
    const int q = q0 + M.q, c0 = q * 4;
    const bool on = M.g < M.G && q < Q;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (on)
      for (int r = r0 + M.g; r < r1; r += 4 * M.G) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int rr = r + u * M.G;
          v[u] = rr < r1 ? sa_load<VI>(xb + (long)rr * A.ld + c0, c0, A.F_in) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += v[u];
      }
    if (M.G > 1) {                                        // the row groups' sums, added in group order
      red[threadIdx.x] = acc;
      __syncthreads();
      if (on && M.g == 0) {
        for (int gg = 1; gg < M.G; ++gg) acc += red[gg * Q + q];
        sa_store<VI>(out + c0, c0, A.F_in, acc);
      }
    } else if (on) {
      sa_store<VI>(out + c0, c0, A.F_in, acc);
    }
  }
}

__global__ __launch_bounds__(256) void sa_mean_kernel(const SaArgs A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)A.B * A.F_in) return;
  const int b = (int)(i / A.F_in), c = (int)(i - (long)b * A.F_in);
  const int n = sa_len(A, b);
  const float* p = A.part + (long)b * A.nchunk * A.F_in + c;
  double s = 0.0;
  for (int k = 0; k < A.nchunk; ++k) s += (double)p[(long)k * A.F_in];
  A.mean[i] = n > 0 ? (float)(s / (double)n) : 0.f;
}

template <bool VI, bool VO>
__global__ __launch_bounds__(256) void sa_apply_kernel(const SaArgs A) {
  __shared__ int lo[2 * SA_MAX_MASKS], hi[2 * SA_MAX_MASKS];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int n = sa_len(A, b);
  sa_draw(A, b, n, lo, hi);
  const int r0 = chunk * A.rc, r1 = min(A.T, r0 + A.rc);
  const int Q = (A.F + 3) >> 2;
  const SaMap M = sa_map(Q);
  if (M.g >= M.G) return;
  const float* xb = A.x + (long)b * A.T * A.ld;
  float* yb = A.y + (long)b * A.T * A.F;
  const float* mb = A.mean + (long)b * A.F_in;
  for (int q = M.q; q < Q; q += M.qstep) {
    const int c0 = q * 4;
    bool band[4];
    f32x4 fill;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      band[j] = false;
      fill[j] = (A.mean_fill && c < A.F_in) ? mb[c] : 0.f;
      if (A.n_freq > 0 && c < A.F_in) {
        const int cm = c % A.P;
        for (int k = 0; k < A.n_freq; ++k) band[j] = band[j] || (cm >= lo[SA_MAX_MASKS + k] && cm < hi[SA_MAX_MASKS + k]);
      }
    }
    for (int r = r0 + M.g; r < r1; r += 4 * M.G) {
      f32x4 v[4];
      bool span[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + u * M.G;
        span[u] = false;
        for (int k = 0; k < A.n_time; ++k) span[u] = span[u] || (rr >= lo[k] && rr < hi[k]);      // (spans lie inside [0, n))
        v[u] = (rr < n && !span[u]) ? sa_load<VI>(xb + (long)rr * A.ld + c0, c0, A.F_in) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + u * M.G;
        if (rr >= r1) continue;
        f32x4 o = v[u];
        if (rr < n) {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (span[u] || band[j]) o[j] = fill[j];
        }
        sa_store<VO>(yb + (long)rr * A.F + c0, c0, A.F, o);
      }
    }
  }
}

// rows per chunk / chunks of a [B, T] batch: >= 1024 workgroups where the rows allow, chunks of >= 4 rows, <= 128 partial rows per utterance
static void sa_chunks(int B, int T, int& rc, int& nchunk) {
  int want = (1024 + B - 1) / B;
  if (want > 128) want = 128;
  rc = (T + want - 1) / want;
  if (rc < 4) rc = 4;
  nchunk = (T + rc - 1) / rc;
}

}  // namespace avsr

using namespace avsr;

extern "C" int avsr_spec_augment_supported(int32_t B, int32_t T, int32_t F, int32_t freq_masks, int32_t time_masks) {
  if (B < 1 || T < 1 || F < 1 || freq_masks < 0 || time_masks < 0) return 0;
  if (T > AVSR_SPEC_AUGMENT_MAX_T || B > 65535) return 0;
  if (freq_masks > SA_MAX_MASKS || time_masks > SA_MAX_MASKS) return 0;
  return (int64_t)B * T * F < ((int64_t)1 << 31) ? 1 : 0;
}

extern "C" int64_t avsr_spec_augment_ws_floats(int32_t B, int32_t T, int32_t F_in) {
  if (B < 1 || T < 1 || F_in < 1) return 0;
  int rc, nchunk;
  sa_chunks(B, T, rc, nchunk);
  return (int64_t)B * nchunk * F_in + (int64_t)B * F_in;
}

extern "C" int avsr_spec_augment(const avsr_spec_augment_args* a, void* stream) {
  if (!a || !a->x || !a->len || !a->seed || !a->y || a->y == a->x) return AVSR_ERR_ARG;
  if (a->F_in < 1 || a->F < a->F_in || a->ld < a->F_in) return AVSR_ERR_ARG;
  if (a->freq_width < 0 || a->time_width < 0 || a->ratio_q16 < 0 || a->ratio_q16 > 65536) return AVSR_ERR_ARG;
  if (a->freq_masks > 0 && a->freq_bins < 1) return AVSR_ERR_ARG;
  if ((a->mean_fill != 0 && a->mean_fill != 1) || (a->video != 0 && a->video != 1)) return AVSR_ERR_ARG;
  if (a->video && a->freq_masks != 0) return AVSR_ERR_ARG;                    // the video stream takes time masks only
  if (!avsr_spec_augment_supported(a->B, a->T, a->F, a->freq_masks, a->time_masks)) return AVSR_ERR_UNSUPPORTED;
  SaArgs A;
  A.x = a->x; A.len = a->len; A.seed = a->seed; A.y = a->y; A.part = nullptr; A.mean = nullptr;
  A.ld = (long)a->ld; A.B = a->B; A.T = a->T; A.F_in = a->F_in; A.F = a->F;
  sa_chunks(a->B, a->T, A.rc, A.nchunk);
  A.n_freq = a->freq_masks; A.freq_width = a->freq_width; A.P = a->freq_masks > 0 ? a->freq_bins : 1;
  A.n_time = a->time_masks; A.time_width = a->time_width; A.ratio_q16 = (uint32_t)a->ratio_q16;
  A.s_freq = RNG_STREAM_SPEC_AUDIO_FREQ; A.s_time = a->video ? RNG_STREAM_SPEC_VIDEO_TIME : RNG_STREAM_SPEC_AUDIO_TIME;
  A.mean_fill = a->mean_fill;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(A.nchunk, A.B);
  const bool vi = (A.F_in & 3) == 0 && (A.ld & 3) == 0 && ((uintptr_t)A.x & 15) == 0;
  const bool vo = (A.F & 3) == 0 && ((uintptr_t)A.y & 15) == 0;
  if (A.mean_fill) {
    if (!a->ws || a->ws_floats < avsr_spec_augment_ws_floats(a->B, a->T, a->F_in) || ((uintptr_t)a->ws & 15)) return AVSR_ERR_ARG;
    A.part = a->ws; A.mean = a->ws + (long)A.B * A.nchunk * A.F_in;
    if (vi) hipLaunchKernelGGL(sa_partial_kernel<true>, grid, dim3(256), 0, s, A);
    else hipLaunchKernelGGL(sa_partial_kernel<false>, grid, dim3(256), 0, s, A);
    AVSR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sa_mean_kernel, dim3((unsigned)(((long)A.B * A.F_in + 255) / 256)), dim3(256), 0, s, A);
    AVSR_CHECK_LAUNCH();
  } else {
    A.mean = a->y;                                                              // never read (mean_fill == 0)
  }
  if (vi && vo) hipLaunchKernelGGL((sa_apply_kernel<true, true>), grid, dim3(256), 0, s, A);
  else if (vi) hipLaunchKernelGGL((sa_apply_kernel<true, false>), grid, dim3(256), 0, s, A);
  else if (vo) hipLaunchKernelGGL((sa_apply_kernel<false, true>), grid, dim3(256), 0, s, A);
  else hipLaunchKernelGGL((sa_apply_kernel<false, false>), grid, dim3(256), 0, s, A);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// Lip-crop augmentation in the train step (video_augment; not in the reference, which only lists the intent at the top of its
// resnet_cnn(); the rule is INTEGRATION.md section 8): per utterance -- never per frame -- a horizontal flip, a shift of up to S pixels
// per axis with edge replication, a contrast factor about the utterance's own channel means and a brightness offset, drawn anew from the
// step's device-side key.
//   x [B, T, H, W, C] contiguous -> y of the same shape: EVERY element is written, frames t >= n_b = clamp(len[b], 0, T) as zeros; x is
//   never modified (it is the captured graph's input).
// Launches, all on the caller's stream, no host read, no memset / memcpy, no atomics (two runs give identical bits):
//   contrast > 0   va_partial_kernel  grid (frame chunks, B): channel sums of the chunk's valid frames -> part [B][chunks][C]  (reads x once)
//                  va_mean_kernel     one thread per (b, channel): the chunks' sums added in chunk order in fp64, / (n H W), rounded once
//                  va_apply_kernel    grid (frame chunks, B): the draws, then gather / apply                    (reads x again, writes y)
//   otherwise      va_apply_kernel alone                                                                   (reads x once, writes y once)
// A bandwidth kernel, output-stationary: the grid runs over utterances x frame chunks (>= 1024 workgroups where the frames allow), a thread
// owns four adjacent output floats of a frame, works out their four source offsets ONCE (they are the same in every frame of the
// utterance) and keeps four frames' loads in flight.  The sources are gathered element by element (a flipped pixel reverses groups of
// C floats, a shift moves rows by dx * C floats: neither keeps 16-byte alignment for C = 3); the stores are 16 bytes where H * W * C
// and the base address allow.  The five draws of an utterance (all uint32) are computed by five threads of every workgroup into LDS.
#include <float.h>
#include "common.h"
#include "avsr_hip.h"

// every fp32 operation of the rule is rounded on its own.  HIP's __fmul_rn / __fadd_rn are plain operators that the compiler contracts
// into a fused multiply-add all the same (their header is read under the default contraction mode), so the operators are written out
// below this pragma instead: va_mul / va_add / va_sub are never fused with a neighbour
#pragma clang fp contract(off)

namespace avsr {

#define VA_MAX_C AVSR_VIDEO_AUGMENT_MAX_C
#define VA_FRAMES 4                                        // frames in flight per thread

struct VaArgs {
  const float* x; const int32_t* len; const int32_t* seed; float* y; float* part; float* mean;
  int B, T, H, W, C, F, fc, nchunk;                        // F = H * W * C floats per frame; fc frames per chunk
  int S;
  uint32_t flip_q24;
  float contrast, brightness;
  int mode;                                                // 0 geometry only, 1 brightness only (y = v + d), 2 contrast (and brightness)
};

__device__ __forceinline__ float va_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float va_add(float a, float b) { return a + b; }
__device__ __forceinline__ float va_sub(float a, float b) { return a - b; }

__device__ __forceinline__ int va_len(const VaArgs& A, int b) {
  const int n = A.len[b];
  return n < 0 ? 0 : (n > A.T ? A.T : n);
}

// 2u - 1 of a 24-bit u in [0, 1): exact in fp32
__device__ __forceinline__ float va_pm1(uint32_t h) {
  const float u = (float)(h >> 8) * (1.0f / 16777216.0f);
  return va_add(va_mul(2.0f, u), -1.0f);
}

// channel sums of a chunk's valid frames.  Thread k < Sq owns the quads k, k + Sq, ... of every frame, Sq = 256 - 256 % C: 4 * Sq is a
// multiple of C, so lane j of a thread's quads is one channel throughout.  The 4 * Sq lane sums of a workgroup are then added per
// channel in a fixed order (three strided LDS passes): in all, fc * H * W terms per fp32 partial.
template <bool VI>
__global__ __launch_bounds__(256) void va_partial_kernel(const VaArgs A) {
  __shared__ float red[1024], red2[256];
  const int b = blockIdx.y, chunk = blockIdx.x, C = A.C;
  const int n = va_len(A, b);
  const int r0 = chunk * A.fc, r1 = min(n, r0 + A.fc);
  const int Q = (A.F + 3) >> 2, Sq = 256 - 256 % C;
  const float* xb = A.x + (long)b * A.T * A.F;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if ((int)threadIdx.x < Sq)
    for (int q = threadIdx.x; q < Q; q += Sq) {
      const int e0 = q * 4;
      for (int r = r0; r < r1; r += VA_FRAMES) {
        f32x4 v[VA_FRAMES];
#pragma unroll
        for (int u = 0; u < VA_FRAMES; ++u) {
          v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (r + u < r1) {
            const float* p = xb + (long)(r + u) * A.F + e0;
            if (VI) v[u] = ld4(p);
            else {
#pragma unroll
              for (int j = 0; j < 4; ++j) if (e0 + j < A.F) v[u][j] = p[j];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < VA_FRAMES; ++u) acc += v[u];
      }
    }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[threadIdx.x * 4 + j] = acc[j];         // lane e = 4 k + j holds channel e % C (threads >= Sq: unused)
  __syncthreads();
  const int N0 = 4 * Sq / C, G1 = 256 / C, G2 = G1 < 8 ? G1 : 8;          // per channel: N0 lane sums -> G1 -> G2 -> 1
  const int c = (int)threadIdx.x % C, g = (int)threadIdx.x / C;
  if (g < G1) {
    float s = 0.f;
    for (int i = g; i < N0; i += G1) s += red[c + C * i];
    red2[c + C * g] = s;
  }
  __syncthreads();
  if (g < G2) {
    float s = 0.f;
    for (int i = g; i < G1; i += G2) s += red2[c + C * i];
    red[c + C * g] = s;
  }
  __syncthreads();
  if (g == 0) {
    float s = 0.f;
    for (int i = 0; i < G2; ++i) s += red[c + C * i];
    A.part[((long)b * A.nchunk + chunk) * C + c] = s;
  }
}

__global__ __launch_bounds__(256) void va_mean_kernel(const VaArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.B * A.C) return;
  const int b = i / A.C, c = i - b * A.C;
  const int n = va_len(A, b);
  const float* p = A.part + (long)b * A.nchunk * A.C + c;
  double s = 0.0;
  for (int k = 0; k < A.nchunk; ++k) s += (double)p[(long)k * A.C];
  A.mean[i] = n > 0 ? (float)(s / ((double)n * (double)A.H * (double)A.W)) : 0.f;
}

template <bool VO>
__global__ __launch_bounds__(256) void va_apply_kernel(const VaArgs A) {
  __shared__ int geo[3];                                   // flip, dx, dy
  __shared__ float pho[2];                                 // cf, d
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int n = va_len(A, b);
  if (threadIdx.x < 5) {
    const uint32_t seed = (uint32_t)A.seed[0], k = threadIdx.x, ub = (uint32_t)b;
    if (k == 0) geo[0] = (hash_u32(seed, RNG_STREAM_VIDEO_AUG_GEOMETRY, 4u * ub) >> 8) < A.flip_q24 ? 1 : 0;
    else if (k < 3) geo[k] = (int)(hash_u32(seed, RNG_STREAM_VIDEO_AUG_GEOMETRY, 4u * ub + k) % (2u * (uint32_t)A.S + 1u)) - A.S;
    else pho[k - 3] = va_pm1(hash_u32(seed, RNG_STREAM_VIDEO_AUG_PHOTOMETRIC, 2u * ub + (k - 3u)));
  }
  __syncthreads();
  const int flip = geo[0], dx = geo[1], dy = geo[2];
  const float cf = va_add(1.0f, va_mul(A.contrast, pho[0])), d = va_mul(A.brightness, pho[1]);
  const int r0 = chunk * A.fc, r1 = min(A.T, r0 + A.fc);
  const int Q = (A.F + 3) >> 2, C = A.C, W = A.W, H = A.H;
  const float* xb = A.x + (long)b * A.T * A.F;
  float* yb = A.y + (long)b * A.T * A.F;
  for (int q = threadIdx.x; q < Q; q += 256) {
    const int e0 = q * 4;
    int off[4];
    float m[4], md[4];
    int pix = e0 / C, c = e0 - pix * C;
    int i = pix / W, j = pix - i * W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ii = min(max(i - dy, 0), H - 1);           // (past the frame's end, e0 + k >= F: clamped all the same, never stored)
      const int jj = min(max(j - dx, 0), W - 1);
      off[k] = (ii * W + (flip ? W - 1 - jj : jj)) * C + c;
      m[k] = A.mode == 2 ? A.mean[b * C + c] : 0.f;
      md[k] = va_add(m[k], d);
      if (++c == C) { c = 0; if (++j == W) { j = 0; ++i; } }
    }
    for (int r = r0; r < r1; r += VA_FRAMES) {
      f32x4 v[VA_FRAMES];
#pragma unroll
      for (int u = 0; u < VA_FRAMES; ++u) {
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r + u < n) {                                   // (n <= T; frames >= n are written as zeros)
          const float* p = xb + (long)(r + u) * A.F;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[u][k] = p[off[k]];
        }
      }
#pragma unroll
      for (int u = 0; u < VA_FRAMES; ++u) {
        const int rr = r + u;
        if (rr >= r1) continue;
        f32x4 o = v[u];
        if (rr < n && A.mode != 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            o[k] = A.mode == 2 ? va_add(va_mul(cf, va_sub(o[k], m[k])), md[k]) : va_add(o[k], d);
        }
        float* py = yb + (long)rr * A.F + e0;
        if (VO) st4(py, o);
        else {
#pragma unroll
          for (int k = 0; k < 4; ++k) if (e0 + k < A.F) py[k] = o[k];
        }
      }
    }
  }
}

// frames per chunk / chunks of a [B, T] batch: >= 1024 workgroups where the frames allow, chunks of a multiple of VA_FRAMES frames
static void va_chunks(int B, int T, int& fc, int& nchunk) {
  int want = (1024 + B - 1) / B;
  if (want > 128) want = 128;
  fc = (T + want - 1) / want / VA_FRAMES * VA_FRAMES;
  if (fc < VA_FRAMES) fc = VA_FRAMES;
  nchunk = (T + fc - 1) / fc;
}

}  // namespace avsr

using namespace avsr;

extern "C" int avsr_video_augment_supported(int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t max_shift) {
  if (B < 1 || T < 1 || H < 1 || W < 1 || C < 1 || max_shift < 0) return 0;
  if (T > AVSR_VIDEO_AUGMENT_MAX_T || B > 65535 || C > VA_MAX_C) return 0;
  if (max_shift >= (H < W ? H : W)) return 0;
  const int64_t lim = (int64_t)1 << 31;
  int64_t F = (int64_t)H * W;                               // (< 2^62)
  if (F >= lim) return 0;
  F *= C;
  if (F >= lim) return 0;
  return (int64_t)B * T * F < lim ? 1 : 0;                  // (B * T < 2^32, F < 2^31: no overflow)
}

extern "C" int64_t avsr_video_augment_ws_floats(int32_t B, int32_t T, int32_t H, int32_t W, int32_t C) {
  if (B < 1 || T < 1 || H < 1 || W < 1 || C < 1) return 0;
  int fc, nchunk;
  va_chunks(B, T, fc, nchunk);
  return (int64_t)B * nchunk * C + (int64_t)B * C;
}

extern "C" int avsr_video_augment(const avsr_video_augment_args* a, void* stream) {
  if (!a || !a->x || !a->len || !a->seed || !a->y || a->y == a->x) return AVSR_ERR_ARG;
  if (a->flip_q24 < 0 || a->flip_q24 > (1 << 24)) return AVSR_ERR_ARG;
  if (!(a->contrast >= 0.f && a->contrast < 1.f) || !(a->brightness >= 0.f && a->brightness <= FLT_MAX)) return AVSR_ERR_ARG;
  if (!avsr_video_augment_supported(a->B, a->T, a->H, a->W, a->C, a->max_shift)) return AVSR_ERR_UNSUPPORTED;
  VaArgs A;
  A.x = a->x; A.len = a->len; A.seed = a->seed; A.y = a->y; A.part = nullptr; A.mean = a->y;      // (mean: never read unless mode 2)
  A.B = a->B; A.T = a->T; A.H = a->H; A.W = a->W; A.C = a->C; A.F = a->H * a->W * a->C;
  va_chunks(a->B, a->T, A.fc, A.nchunk);
  A.S = a->max_shift; A.flip_q24 = (uint32_t)a->flip_q24; A.contrast = a->contrast; A.brightness = a->brightness;
  A.mode = a->contrast > 0.f ? 2 : (a->brightness > 0.f ? 1 : 0);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(A.nchunk, A.B);
  if (A.mode == 2) {
    if (!a->ws || a->ws_floats < avsr_video_augment_ws_floats(a->B, a->T, a->H, a->W, a->C) || ((uintptr_t)a->ws & 15)) return AVSR_ERR_ARG;
    A.part = a->ws; A.mean = a->ws + (long)A.B * A.nchunk * A.C;
    if ((A.F & 3) == 0 && ((uintptr_t)A.x & 15) == 0) hipLaunchKernelGGL(va_partial_kernel<true>, grid, dim3(256), 0, s, A);
    else hipLaunchKernelGGL(va_partial_kernel<false>, grid, dim3(256), 0, s, A);
    AVSR_CHECK_LAUNCH();
    hipLaunchKernelGGL(va_mean_kernel, dim3((unsigned)((A.B * A.C + 255) / 256)), dim3(256), 0, s, A);
    AVSR_CHECK_LAUNCH();
  }
  if ((A.F & 3) == 0 && ((uintptr_t)A.y & 15) == 0) hipLaunchKernelGGL(va_apply_kernel<true>, grid, dim3(256), 0, s, A);
  else hipLaunchKernelGGL(va_apply_kernel<false>, grid, dim3(256), 0, s, A);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

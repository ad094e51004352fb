// Lip-crop CNN front-end pieces (video.resnet_cnn, avsr/video.py:143-195): NHWC im2col / col2im around the fp32 MFMA GEMM for the shapes
// the frame-resident kernels do not cover, ReLU / SELU and residual-add helpers, instance norm.  (Batch norm: batchnorm.hip.)
//
// Convolutions are lowered to GEMMs: col[(n,ho,wo)][(i,j,c)] = x[n, ho*s - pad_t + i, wo*s - pad_l + j, c] (zero outside)
// times the TF kernel [kh, kw, cin, cout] read as a [kh*kw*cin, cout] matrix (HWIO is already that matrix, row-major).
// The data gradient is the transposed GEMM followed by the gather-form col2im below (no atomics, deterministic).
#include "common.h"
#include "avsr_hip.h"

namespace avsr {

__global__ void im2col_kernel(const float* x, float* col, int N, int H, int W, int C, int kh, int kw, int s, int pt, int pl,
                              int Ho, int Wo) {
  const long K = (long)kh * kw * C;
  const long total = (long)N * Ho * Wo * K;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    long r = idx / C;
    const int j = (int)(r % kw); r /= kw;
    const int i = (int)(r % kh); r /= kh;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho);
    const int n = (int)(r / Ho);
    const int h = ho * s - pt + i, w = wo * s - pl + j;
    col[idx] = (h >= 0 && h < H && w >= 0 && w < W) ? x[(((long)n * H + h) * W + w) * C + c] : 0.f;
  }
}

// dx[n,h,w,c] = sum over kernel taps (i,j) of dcol[(n,ho,wo)][(i,j,c)] with ho*s - pt + i == h, wo*s - pl + j == w
__global__ void col2im_kernel(const float* dcol, float* dx, int N, int H, int W, int C, int kh, int kw, int s, int pt, int pl,
                              int Ho, int Wo, float beta) {
  const long K = (long)kh * kw * C;
  const long total = (long)N * H * W * C;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    long r = idx / C;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H);
    const int n = (int)(r / H);
    float acc = 0.f;
    for (int i = 0; i < kh; ++i) {
      const int hn = h + pt - i;
      if (hn < 0 || hn % s) continue;
      const int ho = hn / s;
      if (ho >= Ho) continue;
      for (int j = 0; j < kw; ++j) {
        const int wn = w + pl - j;
        if (wn < 0 || wn % s) continue;
        const int wo = wn / s;
        if (wo >= Wo) continue;
        acc += dcol[(((long)n * Ho + ho) * Wo + wo) * K + ((long)i * kw + j) * C + c];
      }
    }
    dx[idx] = beta != 0.f ? acc + beta * dx[idx] : acc;
  }
}

__global__ void relu_kernel(const float* x, float* y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = fmaxf(x[i], 0.f);
}
// dx = dy * [y > 0]
__global__ void relu_bwd_kernel(const float* y, const float* dy, float* dx, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}
// tf.nn.selu: scale * (x > 0 ? x : alpha * (exp(x) - 1))   (input Dense layers, encoder.py:148-171)
#define SELU_SCALE 1.0507009873554805f
#define SELU_ALPHA 1.6732632423543772f
__global__ void selu_kernel(const float* z, float* y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float x = z[i];
    y[i] = SELU_SCALE * (x > 0.f ? x : SELU_ALPHA * (expf(x) - 1.0f));
  }
}
// dz = dy * selu'(z)
__global__ void selu_bwd_kernel(const float* z, const float* dy, float* dz, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float x = z[i];
    dz[i] = dy[i] * SELU_SCALE * (x > 0.f ? 1.0f : SELU_ALPHA * expf(x));
  }
}
// out = a + b
__global__ void add_kernel(const float* a, const float* b, float* out, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = a[i] + b[i];
}

static inline int blocks_for_n(long n) {
  long b = (n + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

}  // namespace avsr

using namespace avsr;
#define S_(x) ((hipStream_t)(x))

extern "C" int avsr_im2col(const float* x, float* col, int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw,
                           int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, void* stream) {
  if (!x || !col || N <= 0 || H <= 0 || W <= 0 || C <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || Ho <= 0 || Wo <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(im2col_kernel, dim3(blocks_for_n((long)N * Ho * Wo * kh * kw * C)), dim3(256), 0, S_(stream), x, col, N, H, W, C, kh,
                     kw, stride, pad_t, pad_l, Ho, Wo);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_col2im(const float* dcol, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw,
                           int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, float beta, void* stream) {
  if (!dcol || !dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || Ho <= 0 || Wo <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(col2im_kernel, dim3(blocks_for_n((long)N * H * W * C)), dim3(256), 0, S_(stream), dcol, dx, N, H, W, C, kh, kw,
                     stride, pad_t, pad_l, Ho, Wo, beta);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_relu(const float* x, float* y, int64_t n, void* stream) {
  if (!x || !y || n <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(relu_kernel, dim3(blocks_for_n(n)), dim3(256), 0, S_(stream), x, y, (long)n);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}
extern "C" int avsr_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream) {
  if (!y || !dy || !dx || n <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks_for_n(n)), dim3(256), 0, S_(stream), y, dy, dx, (long)n);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}
extern "C" int avsr_add(const float* a, const float* b, float* out, int64_t n, void* stream) {
  if (!a || !b || !out || n <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(add_kernel, dim3(blocks_for_n(n)), dim3(256), 0, S_(stream), a, b, out, (long)n);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_selu(const float* z, float* y, int64_t n, void* stream) {
  if (!z || !y || n <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(selu_kernel, dim3(blocks_for_n(n)), dim3(256), 0, S_(stream), z, y, (long)n);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}
extern "C" int avsr_selu_bwd(const float* z, const float* dy, float* dz, int64_t n, void* stream) {
  if (!z || !dy || !dz || n <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(selu_bwd_kernel, dim3(blocks_for_n(n)), dim3(256), 0, S_(stream), z, dy, dz, (long)n);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}


// ---------------------------------------------------------------------------------------------
// tf.contrib.layers.instance_norm on [B, T, F] encoder inputs (avsr/encoder.py:51-55): statistics over the time axis per
// (utterance, feature) -- zero padding included -- epsilon 1e-6, learned gamma / beta per feature.
// One workgroup per (utterance, 64 features): 256 threads = 64 features x 4 time lanes.
namespace avsr {

__global__ __launch_bounds__(256) void instnorm_fwd_kernel(const float* x, float* y, const float* gamma, const float* beta, float* mean_o,
                                                           float* invstd_o, int T, int F, float eps) {
  __shared__ float red[4][64];
  const int b = blockIdx.x, f = blockIdx.y * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const bool ok = f < F;
  const float* xb = x + (long)b * T * F + f;
  float s = 0.f;
  if (ok) for (int t = g; t < T; t += 4) s += xb[(long)t * F];
  red[g][threadIdx.x & 63] = s;
  __syncthreads();
  const float mean = (red[0][threadIdx.x & 63] + red[1][threadIdx.x & 63] + red[2][threadIdx.x & 63] + red[3][threadIdx.x & 63]) / (float)T;
  __syncthreads();
  float q = 0.f;
  if (ok) for (int t = g; t < T; t += 4) { const float d = xb[(long)t * F] - mean; q += d * d; }
  red[g][threadIdx.x & 63] = q;
  __syncthreads();
  const float var = (red[0][threadIdx.x & 63] + red[1][threadIdx.x & 63] + red[2][threadIdx.x & 63] + red[3][threadIdx.x & 63]) / (float)T;
  const float istd = rsqrtf(var + eps);
  if (!ok) return;
  if (g == 0) { mean_o[(long)b * F + f] = mean; invstd_o[(long)b * F + f] = istd; }
  const float ga = gamma[f] * istd, be = beta[f];
  float* yb = y + (long)b * T * F + f;
  for (int t = g; t < T; t += 4) yb[(long)t * F] = (xb[(long)t * F] - mean) * ga + be;
}

// dx may alias dy.  dgamma_part / dbeta_part [B][F]: per-utterance sums (the caller column-sums them over B).
__global__ __launch_bounds__(256) void instnorm_bwd_kernel(const float* x, const float* dy, const float* gamma, const float* mean_i,
                                                           const float* invstd_i, float* dx, float* dgamma_part, float* dbeta_part,
                                                           int T, int F) {
  __shared__ float red[2][4][64];
  const int b = blockIdx.x, fl = threadIdx.x & 63, f = blockIdx.y * 64 + fl, g = threadIdx.x >> 6;
  const bool ok = f < F;
  const long base = (long)b * T * F + f;
  const float mean = ok ? mean_i[(long)b * F + f] : 0.f, istd = ok ? invstd_i[(long)b * F + f] : 0.f;
  float s1 = 0.f, s2 = 0.f;
  if (ok)
    for (int t = g; t < T; t += 4) {
      const float d = dy[base + (long)t * F];
      s1 += d;
      s2 += d * (x[base + (long)t * F] - mean) * istd;
    }
  red[0][g][fl] = s1; red[1][g][fl] = s2;
  __syncthreads();
  s1 = red[0][0][fl] + red[0][1][fl] + red[0][2][fl] + red[0][3][fl];
  s2 = red[1][0][fl] + red[1][1][fl] + red[1][2][fl] + red[1][3][fl];
  if (!ok) return;
  if (g == 0) { dgamma_part[(long)b * F + f] = s2; dbeta_part[(long)b * F + f] = s1; }
  const float k = gamma[f] * istd, m1 = s1 / (float)T, m2 = s2 / (float)T;
  for (int t = g; t < T; t += 4) {
    const float xh = (x[base + (long)t * F] - mean) * istd;
    dx[base + (long)t * F] = k * (dy[base + (long)t * F] - m1 - xh * m2);
  }
}

}  // namespace avsr

extern "C" int avsr_instnorm_fwd(const float* x, float* y, int32_t B, int32_t T, int32_t F, const float* gamma, const float* beta,
                                 float* mean_out, float* invstd_out, float eps, void* stream) {
  if (!x || !y || !gamma || !beta || !mean_out || !invstd_out || B <= 0 || T <= 0 || F <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(avsr::instnorm_fwd_kernel, dim3(B, (F + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, y, gamma, beta, mean_out,
                     invstd_out, T, F, eps);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_instnorm_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* invstd, float* dx,
                                 float* dgamma_part, float* dbeta_part, int32_t B, int32_t T, int32_t F, void* stream) {
  if (!x || !dy || !gamma || !mean || !invstd || !dx || !dgamma_part || !dbeta_part || B <= 0 || T <= 0 || F <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(avsr::instnorm_bwd_kernel, dim3(B, (F + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, dy, gamma, mean, invstd, dx,
                     dgamma_part, dbeta_part, T, F);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

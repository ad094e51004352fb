// Batch normalisation: every kernel and entry point of it, forward and backward.  y = (x - mean) * invstd * gamma + beta over the last
// axis of a [rows][F] map, statistics over ALL rows (tf.layers.batch_normalization, avsr/encoder.py:44-50, avsr/video.py:4-14).
//
// Three families, in the order of this file:
//
// 1. Row-walking forms (avsr_batchnorm_*).  The kernels read the map itself: per-block partial sums, the mean, per-block centred
//    squares, the variance, then the apply pass; the backward walks the map twice (sums, then dx).  Used where no convolution has
//    produced the statistics on its way: the batch norm of the encoder input features (model_encoder.py), and in the 2-D lip CNN
//    (cnn.py) the layers whose convolutions fall back to the direct or im2col kernels, every layer in evaluation when its output map
//    must be written, and avsr_batchnorm_apply where a reader needs the normalised map itself.  The avsr_batchnorm_sync_* entry points are the same kernels cut at the
//    points where a data-parallel trainer all-reduces (sum | centred squares, or both moments at once in fp64).
//    avsr_dp_sync_unpack, which turns that all-reduced buffer into float operands, stays in elementwise.hip: it also unpacks the loss
//    normalisers and reads nothing of this file.
// 2. Partial-row forms (avsr_bn_*, avsr_conv3d_bn_finalize).  A convolution epilogue (conv_mfma.hip, conv3d.hip) or
//    avsr_bn_bwd_stage1 has already left per-workgroup partial rows [nparts][2*C]; a finalise kernel merges them in fp64 and emits
//    per-channel vectors (mean / invstd / loader scale, shift forward; d gamma, d beta and the coefficients k1, k2, k3 of
//    dx = k1*dz + k2*x + k3 backward), and the consumer -- the next convolution's loader, or avsr_bn_bwd_apply -- applies them.  Used by
//    the fused layers of the 2-D lip CNN (cnn.py) and by every layer of the 3-D one (cnn3d.py).
// 3. fp64 forms (avsr_bn_partials_f64, avsr_bn_*_f64).  Family 2 cut around an all-reduce: the merge alone writes fp64 sums, the host
//    all-reduces them with the row count behind, and the tails run on the GLOBAL sums (DataParallelTrainer(sync_cnn_bn=True)).
//
// Which variance the moving average takes (`bessel`), stated once: TF 1.13 runs the fused batch-norm kernel only on rank-4 inputs, and
// that kernel feeds the Bessel-corrected variance var * n / (n - 1) to the moving variance.  So the 2-D lip CNN's [N,H,W,C] maps take
// bessel = 1; the rank-3 encoder input [B,T,F] and the rank-5 maps [B,T,H,W,C] of the 3-D lip CNN go through tf.nn.moments and take the
// biased variance, bessel = 0.  The normalisation itself always uses the biased variance.
//
// Every reduction here runs in a fixed order (two stages, no float atomics): results are deterministic.
#include "reduce.h"
#include "avsr_hip.h"

using namespace avsr;
#define S_(x) ((hipStream_t)(x))

// ===== 1. row-walking forms over [rows][F] ===================================================================================================
namespace {

// batch norm over rows (tf.layers.batch_normalization axis=-1, encoder.py:44-50): statistics over ALL
// B*T rows including zero padding.  Stage 1: partial sums.  Stage 2: partial centred squares.  Stage 3:
// normalise (+ moving-average update and saved mean / inv-std by block 0).
// Thread layout of the row-walking BN kernels: G = 256 / F row sub-groups of F columns (F < 256), so narrow feature
// vectors (80 audio / 128 video) still use the whole block; the sub-groups are combined in LDS, one partial row per block.
__global__ void bn_partial_sum_kernel(const float* x, float* part, int rows, int F, int rows_per_blk) {
  __shared__ float red[256];
  const int G = F < 256 ? 256 / F : 1;
  const int r0 = blockIdx.x * rows_per_blk, r1 = min(rows, r0 + rows_per_blk);
  for (int base = 0; base < (G > 1 ? 1 : F); base += blockDim.x) {      // G > 1: a single pass (G*F <= 256)
    const int idx = base + threadIdx.x;
    const int f = G > 1 ? idx % F : idx, g = G > 1 ? idx / F : 0;
    float s0 = 0.f, s1 = 0.f;
    if (G > 1 ? idx < G * F : idx < F) {
      int r = r0 + g;
      for (; r + G < r1; r += 2 * G) { s0 += x[(long)r * F + f]; s1 += x[(long)(r + G) * F + f]; }
      if (r < r1) s0 += x[(long)r * F + f];
    }
    if (G > 1) block_group_reduce(s0 + s1, idx, F, G, red, part + (long)blockIdx.x * F);
    else if (idx < F) part[(long)blockIdx.x * F + idx] = s0 + s1;
  }
}

// mean[f] = sum of partials / rows   (one launch, one block per 32 columns; npart = nblk: a block emits ONE partial row whatever G is)
// total != nullptr: the divisor is the (all-reduced) row count total[0] instead of `rows` (sync batch-norm).
__global__ __launch_bounds__(1024) void bn_mean_kernel(const float* part, int npart, float* mean, int rows, int F,
                                                       const float* total = nullptr) {
  if (total) rows = (int)total[0];
  __shared__ double red[32][33];
  const int fl = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int f = blockIdx.x * 32 + fl;
  double s = 0.0;
  if (f < F)
    for (int i = g; i < npart; i += 32) s += (double)part[(long)i * F + f];
  red[g][fl] = s;
  __syncthreads();
  if (g == 0 && f < F) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < 32; ++j) t += red[j][fl];
    mean[f] = (float)(t / rows);
  }
}

__global__ void bn_partial_sq_kernel(const float* x, const float* mean_v, float* part, int rows, int F, int rows_per_blk) {
  __shared__ float red[256];
  const int G = F < 256 ? 256 / F : 1;
  const int r0 = blockIdx.x * rows_per_blk, r1 = min(rows, r0 + rows_per_blk);
  for (int base = 0; base < (G > 1 ? 1 : F); base += blockDim.x) {
    const int idx = base + threadIdx.x;
    const int f = G > 1 ? idx % F : idx, g = G > 1 ? idx / F : 0;
    float s0 = 0.f, s1 = 0.f;
    if (G > 1 ? idx < G * F : idx < F) {
      const float mean = mean_v[f];
      int r = r0 + g;
      for (; r + G < r1; r += 2 * G) {
        const float d0 = x[(long)r * F + f] - mean, d1 = x[(long)(r + G) * F + f] - mean;
        s0 += d0 * d0; s1 += d1 * d1;
      }
      if (r < r1) { const float d0 = x[(long)r * F + f] - mean; s0 += d0 * d0; }
    }
    if (G > 1) block_group_reduce(s0 + s1, idx, F, G, red, part + (long)blockIdx.x * F);
    else if (idx < F) part[(long)blockIdx.x * F + idx] = s0 + s1;
  }
}

// var from the centred-square partials, inverse std, moving-average update (one launch, one block per 32 columns)
__global__ __launch_bounds__(1024) void bn_var_kernel(const float* part, int npart, const float* mean_v, float* invstd_v, float* mov_mean,
                                                      float* mov_var, int rows, int F, float eps, float momentum,
                                                      int bessel, const float* total = nullptr) {
  if (total) rows = (int)total[0];
  __shared__ double red[32][33];
  const int fl = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int f = blockIdx.x * 32 + fl;
  double s = 0.0;
  if (f < F)
    for (int i = g; i < npart; i += 32) s += (double)part[(long)i * F + f];
  red[g][fl] = s;
  __syncthreads();
  if (g == 0 && f < F) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < 32; ++j) t += red[j][fl];
    const float var = (float)(t / rows), mean = mean_v[f];
    invstd_v[f] = rsqrtf(var + eps);
    if (mov_mean) {
      // bessel: which variance the moving average takes (file header)
      const float unbiased = bessel ? var * ((float)rows / (float)max(1, rows - 1)) : var;
      mov_mean[f] = momentum * mov_mean[f] + (1.f - momentum) * mean;
      mov_var[f] = momentum * mov_var[f] + (1.f - momentum) * unbiased;
    }
  }
}

// y = (x - mean) * invstd * gamma + beta, flat over rows * F (F % 4 == 0: one float4 per thread-iteration)
__global__ void bn_apply_kernel(const float* x, const float* mean_v, const float* invstd_v, const float* mov_mean, const float* mov_var,
                                const float* gamma, const float* beta, float* y, long n4, int F, int training, float eps, int relu) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)((i * 4) % F);
    const f32x4 xv = ld4(x + i * 4);
    f32x4 yv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float mean = training ? mean_v[f + e] : mov_mean[f + e];
      const float istd = training ? invstd_v[f + e] : rsqrtf(mov_var[f + e] + eps);
      yv[e] = (xv[e] - mean) * (gamma[f + e] * istd) + beta[f + e];
      if (relu) yv[e] = fmaxf(yv[e], 0.f);
    }
    st4(y + i * 4, yv);
  }
}

// xhat[r][f] = (x - mean) * invstd  (for d gamma = sum dy * xhat)
__global__ void bn_xhat_kernel(const float* x, const float* mean, const float* invstd, float* xhat, long n, int F) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    xhat[i] = (x[i] - mean[f]) * invstd[f];
  }
}

// partial rows of the row-walking passes: 64 rows per block, at most 2048 blocks (the merge stays one short launch), fewer when the
// scratch cannot hold one row [width] per block.  Returns the block count (0: the scratch holds none), *rpb_out = rows per block.
int bn_blocks(int rows, int width, int64_t scratch_floats, int* rpb_out) {
  const int maxblk = 2048;
  int rpb = rows > 64 * maxblk ? (rows + maxblk - 1) / maxblk : 64;
  int nblk = (rows + rpb - 1) / rpb;
  if ((long)nblk * width > scratch_floats) {
    nblk = scratch_floats < width ? 0 : (int)(scratch_floats / width);
    if (nblk < 1) return 0;
    rpb = (rows + nblk - 1) / nblk;
    nblk = (rows + rpb - 1) / rpb;
  }
  *rpb_out = rpb;
  return nblk;
}

// grid of the flat float4 passes: one float4 per thread-iteration, at most `cap` blocks of 256
int bn_flat_grid(long n4, int cap) {
  long b = (n4 + 255) / 256;
  return (int)(b > cap ? cap : b);
}

// The launch geometry of every entry point of this file whose grid depends on its arguments (avsr_batchnorm_plan reports it, the entry
// points launch by it: the two cannot drift apart).  Pointers are the callers' business; the argument checks on rows, F and the scratch
// are here.  Returns p->err.
int bn_plan(int op, int64_t rows, int F, int64_t scratch_floats, int flags, avsr_bn_plan* p) {
  *p = avsr_bn_plan{0, 0, 0, 0, 0, 0, AVSR_ERR_ARG, 0};
  const bool stage = op == AVSR_BN_PLAN_BWD_STAGE1 || op == AVSR_BN_PLAN_BWD_APPLY;
  if (op < AVSR_BN_PLAN_FWD || op > AVSR_BN_PLAN_BWD_APPLY || rows <= 0 || F <= 0 || (!stage && rows > 0x7fffffffL)) return p->err;
  p->G = F < 256 ? 256 / F : 1;
  switch (op) {
    case AVSR_BN_PLAN_FWD:                               // scratch: partials [blocks][F] | mean [F] | invstd [F]
    case AVSR_BN_PLAN_SYNC_SUM:                          // scratch: partials [blocks][F]
    case AVSR_BN_PLAN_SYNC_SQSUM: {
      if (F % 4) return p->err;
      p->blocks = bn_blocks((int)rows, F, op == AVSR_BN_PLAN_FWD ? scratch_floats - 2 * F : scratch_floats, &p->rows_per_block);
      if (!p->blocks) return p->err;
      if (op == AVSR_BN_PLAN_FWD) p->apply_grid = bn_flat_grid(rows * F / 4, 4096);
      break;
    }
    case AVSR_BN_PLAN_BWD: {                             // scratch: partials [blocks][2F] | sums [2F]
      const long n = rows * F;
      p->blocks = bn_blocks((int)rows, 2 * F, scratch_floats - 2 * F, &p->rows_per_block);
      if (!p->blocks) return p->err;
      p->vec = F >= 4 && 1024 % F == 0 && (flags & AVSR_BN_PLAN_ALIGNED) && rows >= 4096;
      if (p->vec) {                                      // the float4 kernels stride the flat map: no rows per block
        int vb = bn_flat_grid(n / 4, 1024);
        if ((long)vb * 2 * F + 2 * F > scratch_floats) vb = (int)((scratch_floats - 2 * F) / (2L * F));
        if (vb < 1) return p->err;
        p->blocks = vb;
        p->rows_per_block = 0;
      }
      p->direct = (flags & AVSR_BN_PLAN_DIRECT) != 0;
      if (flags & AVSR_BN_PLAN_DX) p->apply_grid = p->vec ? bn_flat_grid(n / 4, 4096) : blocks_for(n, 256, 8192);
      break;
    }
    case AVSR_BN_PLAN_SYNC_MOMENTS: {                    // scratch: fp64 partials [blocks][2F]
      int nblk = (int)((rows + 63) / 64);
      if (nblk > 1024) nblk = 1024;
      while (nblk > 1 && (long)nblk * 2 * F * 2 > scratch_floats) nblk /= 2;
      if ((long)nblk * 2 * F * 2 > scratch_floats) return p->err;
      p->rows_per_block = (int)((rows + nblk - 1) / nblk);
      p->blocks = (int)((rows + p->rows_per_block - 1) / p->rows_per_block);
      p->G = 1;
      break;
    }
    case AVSR_BN_PLAN_BWD_STAGE1: {                      // G: the row lanes RL of a block
      if (F % 4 || F > 1024) return p->err;
      const int RL = 256 / (F / 4);
      long per = (rows + 511) / 512;
      if (per < 8L * RL) per = 8L * RL;                  // at least eight passes of a block's row lanes
      if (per > 0x7fffffffL) return p->err;
      p->G = RL;
      p->rows_per_block = (int)per;
      p->blocks = (int)((rows + per - 1) / per);
      break;
    }
    default: {                                           // AVSR_BN_PLAN_BWD_APPLY
      if (F % 4) return p->err;
      const long n4 = rows * (F / 4);
      long blocks = (n4 + 256 * 8 - 1) / (256 * 8);
      if (blocks > 2048) blocks = 2048;
      p->G = 0;
      p->apply_grid = (int)blocks;
      break;
    }
  }
  return p->err = AVSR_OK;
}

}  // namespace

extern "C" int avsr_batchnorm_plan(int32_t op, int64_t rows, int32_t F, int64_t scratch_floats, int32_t flags, avsr_bn_plan* out) {
  if (!out) return AVSR_ERR_ARG;
  const int rc = bn_plan(op, rows, F, scratch_floats, flags, out);
  if (rc) *out = avsr_bn_plan{0, 0, 0, 0, 0, 0, rc, 0};   // a refused call launches nothing
  return rc;
}

extern "C" int avsr_batchnorm_fwd_ex(const float* x, float* y, int32_t rows, int32_t F, const float* gamma, const float* beta,
                                     float* moving_mean, float* moving_var, float* save_mean, float* save_invstd, int32_t training,
                                     float eps, float momentum, int32_t relu, int32_t bessel, float* scratch, int64_t scratch_floats, void* stream) {
  if (!x || !y || !gamma || !beta || rows <= 0 || F <= 0 || !scratch || (!moving_mean != !moving_var)) return AVSR_ERR_ARG;
  avsr_bn_plan pl;
  if (bn_plan(AVSR_BN_PLAN_FWD, rows, F, scratch_floats, 0, &pl)) return pl.err;      // 2*F floats of the scratch hold mean | invstd
  const int nblk = pl.blocks, rpb = pl.rows_per_block;
  // scratch: partials [nblk][F] | mean [F] | invstd [F]  (mean / invstd go to save_mean / save_invstd when given)
  float* part = scratch;
  float* mean_v = save_mean ? save_mean : scratch + (long)nblk * F;
  float* invstd_v = save_invstd ? save_invstd : scratch + (long)nblk * F + F;
  if (training) {
    hipLaunchKernelGGL(bn_partial_sum_kernel, dim3(nblk), dim3(256), 0, S_(stream), x, part, rows, F, rpb);
    AVSR_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_mean_kernel, dim3((F + 31) / 32), dim3(1024), 0, S_(stream), part, nblk, mean_v, rows, F);
    AVSR_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_partial_sq_kernel, dim3(nblk), dim3(256), 0, S_(stream), x, mean_v, part, rows, F, rpb);
    AVSR_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_var_kernel, dim3((F + 31) / 32), dim3(1024), 0, S_(stream), part, nblk, mean_v, invstd_v, moving_mean,
                       moving_var, rows, F, eps, momentum, bessel);
    AVSR_CHECK_LAUNCH();
  } else if (!moving_mean || !moving_var) {
    return AVSR_ERR_ARG;
  }
  const long n4 = (long)rows * F / 4;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(pl.apply_grid), dim3(256), 0, S_(stream), x, mean_v, invstd_v, moving_mean, moving_var, gamma, beta, y,
                     n4, F, training, eps, relu);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_batchnorm_fwd(const float* x, float* y, int32_t rows, int32_t F, const float* gamma,
                                  const float* beta, float* moving_mean, float* moving_var, float* save_mean,
                                  float* save_invstd, int32_t training, float* scratch, int64_t scratch_floats,
                                  void* stream) {
  return avsr_batchnorm_fwd_ex(x, y, rows, F, gamma, beta, moving_mean, moving_var, save_mean, save_invstd, training, 1e-3f, 0.99f, 0,
                               0 /* rank-3 input: non-fused path, biased moving variance */, scratch, scratch_floats, stream);
}

extern "C" int avsr_batchnorm_apply(const float* x, float* y, int32_t rows, int32_t F, const float* gamma, const float* beta, const float* mean,
                                    const float* invstd, int32_t relu, void* stream) {
  if (!x || !y || !gamma || !beta || !mean || !invstd || rows <= 0 || F <= 0 || F % 4) return AVSR_ERR_ARG;
  const long n4 = (long)rows * F / 4;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(bn_flat_grid(n4, 4096)), dim3(256), 0, S_(stream), x, mean, invstd, nullptr, nullptr, gamma, beta, y, n4, F, 1, 0.f, relu);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_batchnorm_xhat(const float* x, const float* mean, const float* invstd, float* xhat, int32_t rows,
                                   int32_t F, void* stream) {
  if (!x || !mean || !invstd || !xhat) return AVSR_ERR_ARG;
  const long n = (long)rows * F;
  hipLaunchKernelGGL(bn_xhat_kernel, dim3(blocks_for(n)), dim3(256), 0, S_(stream), x, mean, invstd, xhat, n, F);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

namespace {

// ---- batch-norm backward (training statistics), optionally through a following ReLU -------------------------------
// dy' = dy * [bn(x) > 0] (relu) ;  d beta = sum dy' ;  d gamma = sum dy' * xhat ;
// dx = gamma * invstd * (dy' - (sum dy' + xhat * sum dy' xhat) / rows)
__global__ void bn_bwd_partial_kernel(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean,
                                      const float* invstd, float* part, int rows, int F, int rows_per_blk, int relu) {
  __shared__ float red[512];
  const int G = F < 256 ? 256 / F : 1;
  const int r0 = blockIdx.x * rows_per_blk, r1 = min(rows, r0 + rows_per_blk);
  float* prow = part + (long)blockIdx.x * 2 * F;
  for (int base = 0; base < (G > 1 ? 1 : F); base += blockDim.x) {      // G > 1: a single pass (G*F <= 256)
    const int idx = base + threadIdx.x;
    const bool on = G > 1 ? idx < G * F : idx < F;
    const int f = G > 1 ? idx % F : idx, g = G > 1 ? idx / F : 0;
    float s1 = 0.f, s2 = 0.f;
    if (on) {
      const float m = mean[f], is = invstd[f], ga = gamma[f], be = beta[f];
      for (int r = r0 + g; r < r1; r += G) {
        const float xh = (x[(long)r * F + f] - m) * is;
        float d = dy[(long)r * F + f];
        if (relu && !(xh * ga + be > 0.f)) d = 0.f;
        s1 += d;
        s2 += d * xh;
      }
    }
    if (G > 1) {                                     // sub-groups combined through LDS in group order: one partial row per block
      if (on) { red[idx] = s1; red[256 + idx] = s2; }
      __syncthreads();
      if (idx < F) {
        float t1 = 0.f, t2 = 0.f;
        for (int gg = 0; gg < G; ++gg) { t1 += red[gg * F + idx]; t2 += red[256 + gg * F + idx]; }
        prow[idx] = t1; prow[F + idx] = t2;
      }
    } else if (on) { prow[f] = s1; prow[F + f] = s2; }
  }
}

__global__ void bn_bwd_apply_kernel(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean,
                                    const float* invstd, const float* sum1, const float* sum2, float* dx, long n, int rows, int F, int relu,
                                    float dx_beta) {
  const float inv_rows = 1.0f / (float)rows;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const float is = invstd[f], ga = gamma[f];
    const float xh = (x[i] - mean[f]) * is;
    float d = dy[i];
    if (relu && !(xh * ga + beta[f] > 0.f)) d = 0.f;
    const float v = ga * is * (d - (sum1[f] + xh * sum2[f]) * inv_rows);
    dx[i] = dx_beta != 0.f ? v + dx_beta * dx[i] : v;
  }
}

// 16-byte versions for F | 1024 (every channel count of the lip CNN): a thread owns FOUR fixed channels -- the grid stride (1024 floats
// per block) is a multiple of F -- so the per-channel constants are loaded once and there is no per-element modulo.
// (The scalar kernels above spent a 64-bit modulo and six table loads per element: 4 TB/s on 600 MB maps.)
__global__ __launch_bounds__(256) void bn_bwd_partial4_kernel(const float* x, const float* dy, const float* gamma, const float* beta,
                                                               const float* mean, const float* invstd, float* part, long n4, int F, int relu) {
  __shared__ f32x4 red[2][256];
  const int f = (int)((threadIdx.x * 4) % F);
  const f32x4 m = ld4(mean + f), is = ld4(invstd + f), ga = ld4(gamma + f), be = ld4(beta + f);
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 xv = ld4(x + i * 4), dv = ld4(dy + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (xv[e] - m[e]) * is[e];
      float d = dv[e];
      if (relu && !(xh * ga[e] + be[e] > 0.f)) d = 0.f;
      s1[e] += d;
      s2[e] += d * xh;
    }
  }
  red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2;
  __syncthreads();
  const int tpf = F >> 2;                               // threads per channel period
  if ((int)threadIdx.x < tpf) {                         // threads t, t + tpf, t + 2 tpf, ... own the same four channels
    f32x4 t1 = {0.f, 0.f, 0.f, 0.f}, t2 = t1;
    for (int k = threadIdx.x; k < 256; k += tpf) { t1 += red[0][k]; t2 += red[1][k]; }
    st4(part + (long)blockIdx.x * 2 * F + 4 * threadIdx.x, t1);
    st4(part + (long)blockIdx.x * 2 * F + F + 4 * threadIdx.x, t2);
  }
}

__global__ __launch_bounds__(256) void bn_bwd_apply4_kernel(const float* x, const float* dy, const float* gamma, const float* beta,
                                                             const float* mean, const float* invstd, const float* sum1, const float* sum2, float* dx,
                                                             long n4, int rows, int F, int relu, float dx_beta) {
  const int f = (int)((threadIdx.x * 4) % F);
  const float inv_rows = 1.0f / (float)rows;
  const f32x4 m = ld4(mean + f), is = ld4(invstd + f), ga = ld4(gamma + f), be = ld4(beta + f);
  f32x4 c1 = ld4(sum1 + f), c2 = ld4(sum2 + f);
#pragma unroll
  for (int e = 0; e < 4; ++e) { c1[e] *= inv_rows; c2[e] *= inv_rows; }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 xv = ld4(x + i * 4), dv = ld4(dy + i * 4);
    f32x4 o;
    if (dx_beta != 0.f) o = ld4(dx + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (xv[e] - m[e]) * is[e];
      float d = dv[e];
      if (relu && !(xh * ga[e] + be[e] > 0.f)) d = 0.f;
      const float v = ga[e] * is[e] * (d - (c1[e] + xh * c2[e]));
      o[e] = dx_beta != 0.f ? v + dx_beta * o[e] : v;
    }
    st4(dx + i * 4, o);
  }
}

}  // namespace

extern "C" int avsr_batchnorm_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean,
                                  const float* invstd, float* dx, float* dgamma, float* dbeta, int32_t rows, int32_t F, int32_t relu,
                                  float dx_beta, float* scratch, int64_t scratch_floats, void* stream) {
  if (!x || !dy || !gamma || !beta || !mean || !invstd || !scratch || rows <= 0 || F <= 0) return AVSR_ERR_ARG;
  float* part = scratch;
  const long n = (long)rows * F;
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  // what the plan takes from the pointers: every operand on 16 bytes (the float4 kernels), both sums wanted on 16 bytes (written
  // where the caller wants them), a dx to write
  const bool aligned = al16(x) && al16(dy) && (!dx || al16(dx)) && al16(gamma) && al16(beta) && al16(mean) && al16(invstd) && al16(scratch);
  const bool direct = dbeta && dgamma && al16(dbeta) && al16(dgamma);
  avsr_bn_plan pl;
  if (bn_plan(AVSR_BN_PLAN_BWD, rows, F, scratch_floats, (aligned ? AVSR_BN_PLAN_ALIGNED : 0) | (direct ? AVSR_BN_PLAN_DIRECT : 0) | (dx ? AVSR_BN_PLAN_DX : 0), &pl))
    return pl.err;
  const int nblk = pl.blocks, rpb = pl.rows_per_block;
  const bool vec = pl.vec != 0;
  float* sums = scratch + (long)nblk * 2 * F;          // [2F]: sum dy' | sum dy' xhat
  if (vec) hipLaunchKernelGGL(bn_bwd_partial4_kernel, dim3(nblk), dim3(256), 0, S_(stream), x, dy, gamma, beta, mean, invstd, part, n / 4, F, relu);
  else hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(nblk), dim3(256), 0, S_(stream), x, dy, gamma, beta, mean, invstd, part, rows, F, rpb, relu);
  AVSR_CHECK_LAUNCH();
  // the reduced sums ARE d beta | d gamma: one reduction launch writes them where the caller wants them and the apply pass reads
  // them from there (16-byte aligned destinations for the vector kernel; else through the scratch + two copies)
  float* const s1 = direct ? dbeta : sums;
  float* const s2 = direct ? dgamma : sums + F;
  { const int rc = avsr_colsum_final_launch_split(part, 2L * F, nblk, s1, s2, F, 2 * F, 1.0f, 0.0f, stream); if (rc) return rc; }
  if (dx) {
    if (vec) {
      hipLaunchKernelGGL(bn_bwd_apply4_kernel, dim3(pl.apply_grid), dim3(256), 0, S_(stream), x, dy, gamma, beta, mean, invstd, s1, s2, dx, n / 4, rows, F, relu,
                         dx_beta);
    } else {
      hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(pl.apply_grid), dim3(256), 0, S_(stream), x, dy, gamma, beta, mean, invstd, s1, s2, dx, n, rows,
                         F, relu, dx_beta);
    }
    AVSR_CHECK_LAUNCH();
  }
  if (!direct) {
    if (dbeta && avsr::dev_copy(dbeta, sums, sizeof(float) * F, S_(stream)) != hipSuccess) return AVSR_ERR_HIP;
    if (dgamma && avsr::dev_copy(dgamma, sums + F, sizeof(float) * F, S_(stream)) != hipSuccess) return AVSR_ERR_HIP;
  }
  return AVSR_OK;
}

// ---- sync batch-norm over data-parallel ranks: the three local phases around the two host-side all-reduces ----
extern "C" int avsr_batchnorm_sync_sum(const float* x, int32_t rows, int32_t F, float* sum_out, float* scratch,
                                       int64_t scratch_floats, void* stream) {
  if (!x || !sum_out || !scratch || rows <= 0 || F <= 0 || F % 4) return AVSR_ERR_ARG;
  avsr_bn_plan pl;
  if (bn_plan(AVSR_BN_PLAN_SYNC_SUM, rows, F, scratch_floats, 0, &pl)) return pl.err;
  const int nblk = pl.blocks, rpb = pl.rows_per_block;
  hipLaunchKernelGGL(bn_partial_sum_kernel, dim3(nblk), dim3(256), 0, S_(stream), x, scratch, rows, F, rpb);
  AVSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_mean_kernel, dim3((F + 31) / 32), dim3(1024), 0, S_(stream), scratch, nblk, sum_out, 1, F, nullptr);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_batchnorm_sync_sqsum(const float* x, int32_t rows, int32_t F, const float* sum_global,
                                         const float* total_rows, float* mean_out, float* sq_out, float* scratch,
                                         int64_t scratch_floats, void* stream) {
  if (!x || !sum_global || !total_rows || !mean_out || !sq_out || !scratch || rows <= 0 || F <= 0 || F % 4) return AVSR_ERR_ARG;
  avsr_bn_plan pl;
  if (bn_plan(AVSR_BN_PLAN_SYNC_SQSUM, rows, F, scratch_floats, 0, &pl)) return pl.err;
  const int nblk = pl.blocks, rpb = pl.rows_per_block;
  hipLaunchKernelGGL(bn_mean_kernel, dim3((F + 31) / 32), dim3(1024), 0, S_(stream), sum_global, 1, mean_out, 1, F, total_rows);
  AVSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_partial_sq_kernel, dim3(nblk), dim3(256), 0, S_(stream), x, mean_out, scratch, rows, F, rpb);
  AVSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_mean_kernel, dim3((F + 31) / 32), dim3(1024), 0, S_(stream), scratch, nblk, sq_out, 1, F, nullptr);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_batchnorm_sync_apply(const float* x, float* y, int32_t rows, int32_t F, const float* gamma,
                                         const float* beta, float* moving_mean, float* moving_var, const float* mean,
                                         const float* sq_global, const float* total_rows, float* invstd_out, float eps,
                                         float momentum, int32_t relu, void* stream) {
  if (!x || !y || !gamma || !beta || !mean || !sq_global || !total_rows || !invstd_out || rows <= 0 || F <= 0 || F % 4 ||
      (!moving_mean != !moving_var))
    return AVSR_ERR_ARG;
  hipLaunchKernelGGL(bn_var_kernel, dim3((F + 31) / 32), dim3(1024), 0, S_(stream), sq_global, 1, mean, invstd_out, moving_mean,
                     moving_var, 1, F, eps, momentum, 0, total_rows);
  AVSR_CHECK_LAUNCH();
  const long n4 = (long)rows * F / 4;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(bn_flat_grid(n4, 4096)), dim3(256), 0, S_(stream), x, mean, invstd_out, moving_mean, moving_var, gamma, beta, y,
                     n4, F, 1, eps, relu);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// ---- ONE small collective per data-parallel step (SURVEY 8(e) collectives (2) + (3) fused) ----
// avsr_batchnorm_sync_moments: per-feature sum x | sum x^2 of this rank's rows in DOUBLE precision into out64 [2F] (the global
// variance is then E[x^2] - mean^2 evaluated in fp64: exact to ~1e-13 relative for feature-scale inputs, so the second,
// mean-dependent reduction -- and its all-reduce -- is not needed).
namespace {
__global__ __launch_bounds__(256) void bn_moments_partial_kernel(const float* __restrict__ x, double* __restrict__ part, int rows, int F, int rpb) {
  const int r0 = blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
  for (int f = threadIdx.x; f < F; f += 256) {
    double s = 0.0, s2 = 0.0;
    for (int r = r0; r < r1; ++r) { const double v = (double)x[(long)r * F + f]; s += v; s2 += v * v; }
    part[(long)blockIdx.x * 2 * F + f] = s;
    part[(long)blockIdx.x * 2 * F + F + f] = s2;
  }
}
__global__ __launch_bounds__(256) void bn_moments_final_kernel(const double* __restrict__ part, int nblk, int F2, double* __restrict__ out) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F2) return;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) s += part[(long)i * F2 + f];
  out[f] = s;
}
}  // namespace
extern "C" int avsr_batchnorm_sync_moments(const float* x, int32_t rows, int32_t F, double* out64, float* scratch, int64_t scratch_floats,
                                           void* stream) {
  if (!x || !out64 || !scratch || rows <= 0 || F <= 0 || ((uintptr_t)scratch & 7)) return AVSR_ERR_ARG;
  avsr_bn_plan pl;
  if (bn_plan(AVSR_BN_PLAN_SYNC_MOMENTS, rows, F, scratch_floats, 0, &pl)) return pl.err;
  const int nblk = pl.blocks, rpb = pl.rows_per_block;
  double* part = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(bn_moments_partial_kernel, dim3(nblk), dim3(256), 0, S_(stream), x, part, rows, F, rpb);
  AVSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_moments_final_kernel, dim3((2 * F + 255) / 256), dim3(256), 0, S_(stream), part, nblk, 2 * F, out64);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// ===== 2. partial-row forms fed by the convolution epilogues ================================================================================
namespace {

// ---- the three steps the finalise kernels of families 2 and 3 are made of, one copy each ----
// fp64 merge of partial rows part [nparts][2*C] (first | second sum per channel) by a workgroup of 1024 threads over 16 channels: 16
// lanes read 16 consecutive channels of a partial row (64 B segments), 64 row groups stride the rows, then the first 16 threads add the
// 64 groups in order.  (1024 threads: 512 partial rows are eight loads per thread -- a latency chain, not a bandwidth one.)
// True for the thread that holds the sums of channel blockIdx.x * 16 + (threadIdx.x & 15); every other thread is done.
__device__ __forceinline__ bool merge_partials(const float* part, int nparts, int C, double* s_out, double* s2_out) {
  __shared__ double red[2][64][17];
  const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
  double s = 0.0, s2 = 0.0;
  if (c < C)
    for (int p = rg; p < nparts; p += 64) { s += (double)part[(long)p * 2 * C + c]; s2 += (double)part[(long)p * 2 * C + C + c]; }
  red[0][rg][cl] = s; red[1][rg][cl] = s2;
  __syncthreads();
  if (threadIdx.x >= 16 || c >= C) return false;
  s = 0.0; s2 = 0.0;
  for (int r = 0; r < 64; ++r) { s += red[0][r][cl]; s2 += red[1][r][cl]; }
  *s_out = s; *s2_out = s2;
  return true;
}

// forward tail of channel c from its sum s, sum of squares s2 and row count: mean, clamped biased variance, inverse std; the loader
// affine (scale != NULL); the moving averages (mov_mean != NULL), whose variance is Bessel-corrected or biased (file header)
template <bool BESSEL>
__device__ __forceinline__ void finalize_channel(int c, double s, double s2, double count, float eps, float momentum, float* mean,
                                                 float* invstd, float* mov_mean, float* mov_var, const float* gamma, const float* beta,
                                                 float* scale, float* shift) {
  const double m = s / count;
  double var = s2 / count - m * m;
  if (var < 0.0) var = 0.0;
  const float is = rsqrtf((float)var + eps);
  mean[c] = (float)m;
  invstd[c] = is;
  if (scale) {                                          // y = x * scale + shift  ==  (x - mean) * invstd * gamma + beta
    const float sc = gamma[c] * is;
    scale[c] = sc;
    shift[c] = beta[c] - (float)m * sc;
  }
  if (mov_mean) {
    const float v = BESSEL ? (float)(var * (count / (count > 1.0 ? count - 1.0 : 1.0))) : (float)var;
    mov_mean[c] = momentum * mov_mean[c] + (1.f - momentum) * (float)m;
    mov_var[c] = momentum * mov_var[c] + (1.f - momentum) * v;
  }
}

// backward tail of channel c from (sum dz | sum dz*x): d beta (+)= sum dz and d gamma (+)= invstd * (sum dz*x - mean * sum dz) take
// this rank's sums (sl, sxl) -- a gradient all-reduce adds the ranks' shares -- and the coefficients of dx = k1*dz + k2*x + k3,
//   k[0..C) = gamma*invstd, k[C..2C) = -gamma*invstd^2 * b, k[2C..3C) = -gamma*invstd*a + gamma*invstd^2 * b * mean
// with a = sum dz / count, b = invstd * (sum dz*x - mean * sum dz) / count, take the sums (s, sx) and the row count of the whole batch,
// so that dx = gamma*invstd * (dz - a - xhat*b).  On one rank the two pairs of sums are the same.
__device__ __forceinline__ void bwd_finalize_channel(int c, int C, double sl, double sxl, double s, double sx, double count,
                                                     const float* mean, const float* invstd, const float* gamma, float* dgamma,
                                                     float* dbeta, float grad_beta, float* k) {
  const double m = mean[c], is = invstd[c], g = gamma[c];
  const double sxh_l = is * (sxl - m * sl);              // sum dz * xhat, this rank
  if (dbeta) dbeta[c] = (grad_beta != 0.f ? grad_beta * dbeta[c] : 0.f) + (float)sl;
  if (dgamma) dgamma[c] = (grad_beta != 0.f ? grad_beta * dgamma[c] : 0.f) + (float)sxh_l;
  const double sxh = is * (sx - m * s);
  const double a = s / count, b = sxh / count;
  k[c] = (float)(g * is);
  k[C + c] = (float)(-g * is * is * b);
  k[2 * C + c] = (float)(-g * is * a + g * is * is * b * m);
}

// finalise batch-norm statistics from the per-workgroup partial sums the convolution epilogue wrote: part [nparts][2*C] (sum | sum of
// squares), count = rows per channel
template <bool BESSEL>
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* part, int nparts, int C, double count, float eps, float momentum,
                                                          float* mean, float* invstd, float* mov_mean, float* mov_var, const float* gamma,
                                                          const float* beta, float* scale, float* shift) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);
  double s, s2;
  if (!merge_partials(part, nparts, C, &s, &s2)) return;
  finalize_channel<BESSEL>(c, s, s2, count, eps, momentum, mean, invstd, mov_mean, mov_var, gamma, beta, scale, shift);
}

// evaluation graph (training=False, video.py:8-12): scale / shift of the loader-applied batch norm from the MOVING statistics
__global__ void bn_eval_affine_kernel(const float* gamma, const float* beta, const float* mov_mean, const float* mov_var, float eps, float* scale,
                                      float* shift, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = gamma[c] * rsqrtf(mov_var[c] + eps);
  scale[c] = sc;
  shift[c] = beta[c] - mov_mean[c] * sc;
}

// Batch-norm backward, stage 1 on its own (the form avsr_conv_bwd_data_bn fuses into a single-launch data gradient's epilogue), for a
// batch norm whose output gradient was assembled by several launches (the per-class 3x3/2 data gradient of a wide layer):
//   dz = dy * [relu(scale*x + shift) > 0]   (or [y > 0] when the batch-norm output map was written),  part [nparts][2C] = (sum dz | sum dz*x)
// dz may alias dy.  C % 4 == 0, C <= 1024; *nparts <= 512 blocks, each over a contiguous run of rows.
__global__ __launch_bounds__(256) void bn_bwd_stage1_kernel(const float* dy, const float* __restrict__ x, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const float* __restrict__ y, float* dz, long rows,
                                                            int C, long rows_per_block, float* __restrict__ part) {
  __shared__ float red[256][9];
  const int C4 = C / 4, RL = 256 / C4, q = threadIdx.x % C4, rl = threadIdx.x / C4;
  const long r0 = blockIdx.x * rows_per_block, r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, sx = s;
  f32x4 sc = s, sh = s;
  if (scale && rl < RL) { sc = ld4(scale + 4 * q); sh = ld4(shift + 4 * q); }
  if (rl < RL)
    for (long r = r0 + rl; r < r1; r += RL) {
      const long o = r * C + 4 * q;
      const f32x4 g = ld4(dy + o), xv = ld4(x + o);
      f32x4 v;
      if (scale) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(xv[e], sc[e], sh[e]) > 0.f ? g[e] : 0.f;
      } else {
        const f32x4 yv = ld4(y + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = yv[e] > 0.f ? g[e] : 0.f;
      }
      st4(dz + o, v);
      s += v; sx += v * xv;
    }
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[threadIdx.x][e] = s[e]; red[threadIdx.x][4 + e] = sx[e]; }
  __syncthreads();
  if (threadIdx.x >= C4) return;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < RL; ++r)
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += red[r * C4 + q][e];
  float* p = part + (long)blockIdx.x * 2 * C;
#pragma unroll
  for (int e = 0; e < 4; ++e) { p[4 * q + e] = a[e]; p[C + 4 * q + e] = a[4 + e]; }
}

// Batch-norm backward, stage 2 (after avsr_conv_bwd_data_bn or avsr_bn_bwd_stage1 wrote dz and the partial sums [nparts][2*C] =
// (sum dz | sum dz*x)): d gamma, d beta and the coefficients k [3C] that avsr_bn_bwd_apply reads
__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float* part, int nparts, int C, double count, const float* mean,
                                                              const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                                                              float grad_beta, float* k) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);
  double s, s2;
  if (!merge_partials(part, nparts, C, &s, &s2)) return;
  bwd_finalize_channel(c, C, s, s2, s, s2, count, mean, invstd, gamma, dgamma, dbeta, grad_beta, k);
}

// dx = beta*dx + k1[c]*dz + k2[c]*x + k3[c] over [rows][C] maps, C % 4 == 0 (16-byte accesses, one channel quad per lane)
__global__ __launch_bounds__(256) void bn_bwd_coef_apply_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                                const float* __restrict__ k, float* __restrict__ dx, long n4, int C4, int C, float beta) {
  const long stride = (long)gridDim.x * 256;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n4; idx += stride) {
    const int c = (int)(idx % C4) * 4;
    const f32x4 k1 = ld4(k + c), k2 = ld4(k + C + c), k3 = ld4(k + 2 * C + c);
    const f32x4 a = ld4(dz + idx * 4), b = ld4(x + idx * 4);
    f32x4 v = k1 * a + k2 * b + k3;
    if (beta != 0.f) v += beta * ld4(dx + idx * 4);
    st4(dx + idx * 4, v);
  }
}

}  // namespace

extern "C" int avsr_bn_finalize(const float* part, int32_t nparts, int32_t C, int64_t count, float eps, float momentum, float* mean,
                                float* invstd, float* mov_mean, float* mov_var, const float* gamma, const float* beta, float* scale,
                                float* shift, void* stream) {
  if (!part || nparts <= 0 || C <= 0 || count <= 0 || !mean || !invstd || (scale && (!gamma || !beta || !shift)) || (!mov_mean != !mov_var))
    return AVSR_ERR_ARG;
  hipLaunchKernelGGL(bn_finalize_kernel<true>, dim3((C + 15) / 16), dim3(1024), 0, S_(stream), part, nparts, C, (double)count, eps, momentum, mean,
                     invstd, mov_mean, mov_var, gamma, beta, scale, shift);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// the same over the rank-5 maps of the 3-D lip CNN (statistics from the avsr_conv3d_fwd epilogue): biased moving variance
extern "C" int avsr_conv3d_bn_finalize(const float* part, int32_t nparts, int32_t C, int64_t count, float eps, float momentum, float* mean,
                                       float* invstd, float* mov_mean, float* mov_var, const float* gamma, const float* beta, float* scale,
                                       float* shift, void* stream) {
  if (!part || nparts <= 0 || C <= 0 || count <= 0 || !mean || !invstd || (scale && (!gamma || !beta || !shift)) || (!mov_mean != !mov_var))
    return AVSR_ERR_ARG;
  hipLaunchKernelGGL(bn_finalize_kernel<false>, dim3((C + 15) / 16), dim3(1024), 0, S_(stream), part, nparts, C, (double)count, eps, momentum, mean,
                     invstd, mov_mean, mov_var, gamma, beta, scale, shift);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_bn_eval_affine(const float* gamma, const float* beta, const float* mov_mean, const float* mov_var, float eps, float* scale,
                                   float* shift, int32_t C, void* stream) {
  if (!gamma || !beta || !mov_mean || !mov_var || !scale || !shift || C <= 0) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(bn_eval_affine_kernel, dim3((C + 63) / 64), dim3(64), 0, S_(stream), gamma, beta, mov_mean, mov_var, eps, scale, shift, C);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_bn_bwd_stage1(const float* dy, const float* x, const float* scale, const float* shift, const float* y, float* dz, int64_t rows,
                                  int32_t C, float* part, int32_t* nparts, void* stream) {
  if (!dy || !x || !dz || !part || !nparts || rows <= 0 || C <= 0 || C % 4 || C > 1024 || (!scale && !y) || (scale && !shift)) return AVSR_ERR_ARG;
  avsr_bn_plan pl;
  if (bn_plan(AVSR_BN_PLAN_BWD_STAGE1, rows, C, 0, 0, &pl)) return pl.err;
  const int blocks = pl.blocks;
  const long per = pl.rows_per_block;
  *nparts = blocks;
  hipLaunchKernelGGL(bn_bwd_stage1_kernel, dim3(blocks), dim3(256), 0, S_(stream), dy, x, scale, shift, y, dz, (long)rows, C, per, part);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_bn_bwd_finalize(const float* part, int32_t nparts, int32_t C, int64_t count, const float* mean, const float* invstd,
                                    const float* gamma, float* dgamma, float* dbeta, float grad_beta, float* k, void* stream) {
  if (!part || nparts <= 0 || C <= 0 || count <= 0 || !mean || !invstd || !gamma || !k) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 15) / 16), dim3(1024), 0, S_(stream), part, nparts, C, (double)count, mean, invstd, gamma,
                     dgamma, dbeta, grad_beta, k);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

extern "C" int avsr_bn_bwd_apply(const float* dz, const float* x, const float* k, float* dx, int64_t rows, int32_t C, float beta, void* stream) {
  if (!dz || !x || !k || !dx || rows <= 0 || C <= 0 || C % 4) return AVSR_ERR_ARG;
  avsr_bn_plan pl;
  if (bn_plan(AVSR_BN_PLAN_BWD_APPLY, rows, C, 0, 0, &pl)) return pl.err;
  const long n4 = rows * (C / 4);
  hipLaunchKernelGGL(bn_bwd_coef_apply_kernel, dim3(pl.apply_grid), dim3(256), 0, S_(stream), dz, x, k, dx, n4, C / 4, C, beta);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// ===== 3. fp64 forms around the data-parallel all-reduce ====================================================================================
// batch-norm statistics across data-parallel ranks (opt-in: DataParallelTrainer(sync_cnn_bn=True)).  The partial sums a convolution
// epilogue wrote are merged into fp64 per-channel sums, the host all-reduces that small buffer (with the rank's row count behind it),
// and the finalisation reads the GLOBAL sums: mean / variance / moving averages / loader affine of the whole batch on every rank
// (video.py:4-14 over the global batch).  The merge and the tails are those of family 2.
namespace {
__global__ __launch_bounds__(1024) void bn_partials_f64_kernel(const float* part, int nparts, int C, double* out) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);
  double s, s2;
  if (!merge_partials(part, nparts, C, &s, &s2)) return;
  out[c] = s; out[C + c] = s2;
}
// sums [2C + 1]: sum | sum of squares | rows per channel (all ranks)
__global__ void bn_finalize_f64_kernel(const double* sums, int C, float eps, float momentum, float* mean, float* invstd, float* mov_mean,
                                       float* mov_var, const float* gamma, const float* beta, float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  finalize_channel<true>(c, sums[c], sums[C + c], sums[2 * C], eps, momentum, mean, invstd, mov_mean, mov_var, gamma, beta, scale, shift);
}
// local [2C]: this rank's (sum dz | sum dz*x); global [2C + 1]: the all-reduced sums and the global row count
__global__ void bn_bwd_finalize_f64_kernel(const double* local, const double* global, int C, const float* mean, const float* invstd,
                                           const float* gamma, float* dgamma, float* dbeta, float grad_beta, float* k) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  bwd_finalize_channel(c, C, local[c], local[C + c], global[c], global[C + c], global[2 * C], mean, invstd, gamma, dgamma, dbeta, grad_beta, k);
}
}  // namespace
extern "C" int avsr_bn_partials_f64(const float* part, int32_t nparts, int32_t C, double* out64, void* stream) {
  if (!part || nparts <= 0 || C <= 0 || !out64) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(bn_partials_f64_kernel, dim3((C + 15) / 16), dim3(1024), 0, S_(stream), part, nparts, C, out64);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}
extern "C" int avsr_bn_finalize_f64(const double* sums, int32_t C, float eps, float momentum, float* mean, float* invstd, float* mov_mean,
                                    float* mov_var, const float* gamma, const float* beta, float* scale, float* shift, void* stream) {
  if (!sums || C <= 0 || !mean || !invstd || (scale && (!gamma || !beta || !shift)) || (!mov_mean != !mov_var)) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(bn_finalize_f64_kernel, dim3((C + 63) / 64), dim3(64), 0, S_(stream), sums, C, eps, momentum, mean, invstd, mov_mean, mov_var,
                     gamma, beta, scale, shift);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}
extern "C" int avsr_bn_bwd_finalize_f64(const double* local, const double* global, int32_t C, const float* mean, const float* invstd,
                                        const float* gamma, float* dgamma, float* dbeta, float grad_beta, float* k, void* stream) {
  if (!local || !global || C <= 0 || !mean || !invstd || !gamma || !k) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(bn_bwd_finalize_f64_kernel, dim3((C + 63) / 64), dim3(64), 0, S_(stream), local, global, C, mean, invstd, gamma, dgamma, dbeta,
                     grad_beta, k);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

// Column reductions: out[f] = alpha * sum_r a[r][f] * (b ? b[r][f] : 1) + beta * out[f], deterministic (no float atomics).
// Two passes, one kernel each, both driven by a table of up to 32 independent jobs whose blocks find their job by block index:
//   partial pass  blocks of rows -> one fp32 partial row each                         (colsum_partial_kernel)
//   final pass    the partial rows of a column, summed in fp64, rounded once to fp32   (colsum_final_kernel)
// Who runs what:
//   avsr_colsum                          one job through both passes (32 rows per block, <= 2048 blocks)
//   avsr_colsum_multi                    the train step's bias gradients: all jobs of a half-pass in two launches
//   avsr_colsum_final_launch[_split]     the final pass alone over partial rows another kernel wrote (split-K / direct weight-gradient
//                                        slabs, batch-norm statistics, the embedding gradient)
//   slab_reduce                          the same for the slabs of conv_wgrad.hip (either kind of job): launched at once, or recorded
//                                        between avsr_slab_defer_begin and _end and run as one launch at the end
#include "reduce.h"
#include "avsr_hip.h"

namespace avsr {

#define RED_JOBS 32
// a, b: two-level row addressing (same convention as avsr_gemm); rpb rows per block; part: [blocks][F]
struct PartJob { const float* a; const float* b; float* part; long lda, ldoa, ldb, ldob; int Ta, Tb, rows, F, rpb; };
struct PartLaunch { int n; int blk0[RED_JOBS]; PartJob job[RED_JOBS]; };
// part: nblk rows `ld` floats apart.  kind 0: columns [0, split) -> out, [split, F) -> out2.  kind 1: the pixel-pair slab of an 8-channel
// weight gradient (conv_wgrad.hip): 9*Ci*8 kernel entries -> out, then 8 bias entries -> out2, each the sum of two slab columns.
struct FinalJob { const float* part; long ld; int nblk, F; float* out; float* out2; int split, kind, Ci; float alpha, beta; };
struct FinalLaunch { int n; int blk0[RED_JOBS]; FinalJob job[RED_JOBS]; };

// the job whose block range [blk0[j], blk0[j + 1]) holds this block
__device__ __forceinline__ int job_of_block(const int* blk0, int n) {
  int j = 0;
#pragma unroll 1
  for (int k = 1; k < n; ++k) if ((int)blockIdx.x >= blk0[k]) j = k;
  return __builtin_amdgcn_readfirstlane(j);
}

// rows [r0, r1) of a job -> one partial row (256 threads; red: 256 floats)
__device__ __forceinline__ void partial_of_rows(const PartJob& J, int r0, int r1, float* red, float* row) {
  const float* a = J.a; const float* b = J.b;
  const int F = J.F, G = F < 256 ? 256 / F : 1;
  if (G > 1) {
    const int idx = threadIdx.x, f = idx % F, g = idx / F;
    float s = 0.f;
    if (idx < G * F)
      for (int r = r0 + g; r < r1; r += G) {
        const float x = a[rowoff(r, J.lda, J.Ta, J.ldoa) + f];
        s += b ? x * b[rowoff(r, J.ldb, J.Tb, J.ldob) + f] : x;
      }
    block_group_reduce(s, idx, F, G, red, row);
    return;
  }
  // wide records (the [B*T, 4H] gate gradients: 131 MB each): 16-byte loads, eight rows in flight per thread -- a bandwidth stream,
  // not a latency chain (two 4-byte loads in flight per thread ran at 2.4 TB/s)
  const bool vec = (F & 3) == 0 && ((uintptr_t)a & 15) == 0 && (J.lda & 3) == 0 && (J.ldoa & 3) == 0 &&
                   (!b || (((uintptr_t)b & 15) == 0 && (J.ldb & 3) == 0 && (J.ldob & 3) == 0));
  if (vec) {
    for (int f = threadIdx.x * 4; f < F; f += 4 * blockDim.x) {
      f32x4 acc[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int r = r0; r < r1; r += 8) {
        f32x4 x[8], y[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const bool in = r + u < r1;
          x[u] = in ? ld4(a + rowoff(r + u, J.lda, J.Ta, J.ldoa) + f) : f32x4{0.f, 0.f, 0.f, 0.f};
          if (b) y[u] = in ? ld4(b + rowoff(r + u, J.ldb, J.Tb, J.ldob) + f) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += b ? x[u] * y[u] : x[u];
      }
      st4(row + f, ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])));
    }
    return;
  }
  for (int f = threadIdx.x; f < F; f += blockDim.x) {
    float s0 = 0.f, s1 = 0.f;
    int r = r0;
    for (; r + 1 < r1; r += 2) {                        // two independent chains: two loads in flight per thread
      const float x0 = a[rowoff(r, J.lda, J.Ta, J.ldoa) + f], x1 = a[rowoff(r + 1, J.lda, J.Ta, J.ldoa) + f];
      s0 += b ? x0 * b[rowoff(r, J.ldb, J.Tb, J.ldob) + f] : x0;
      s1 += b ? x1 * b[rowoff(r + 1, J.ldb, J.Tb, J.ldob) + f] : x1;
    }
    if (r < r1) { const float x0 = a[rowoff(r, J.lda, J.Ta, J.ldoa) + f]; s0 += b ? x0 * b[rowoff(r, J.ldb, J.Tb, J.ldob) + f] : x0; }
    row[f] = s0 + s1;
  }
}

// Row group g of 32 walks partial rows g, g + 32, ... of column o0 (TWO: plus column o1 of the same row), four rows' loads in flight.
// The two forms add the four rows up in the order each has always had (a tree / one after the other), so neither changes a bit.
template <bool TWO>
__device__ __forceinline__ double walk_partials(const float* part, long ld, int nblk, int g, long o0, long o1) {
  double s = 0.0;
  int i = g;
  for (; i + 96 < nblk; i += 128) {
    float x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { x[u] = part[(long)(i + 32 * u) * ld + o0]; if (TWO) y[u] = part[(long)(i + 32 * u) * ld + o1]; }
    if (TWO) {
#pragma unroll
      for (int u = 0; u < 4; ++u) s += (double)x[u] + (double)y[u];
    } else {
      s += ((double)x[0] + (double)x[1]) + ((double)x[2] + (double)x[3]);
    }
  }
  for (; i < nblk; i += 32) s += TWO ? (double)part[(long)i * ld + o0] + (double)part[(long)i * ld + o1] : (double)part[(long)i * ld + o0];
  return s;
}

// the 32 row groups' sums of 32 columns -> fp64 total per column (LDS, group order), one rounding to fp32, *o = alpha * total + beta * *o
__device__ __forceinline__ void tree_write(double s, double (*red)[33], int g, int fl, float* o, float alpha, float beta) {
  red[g][fl] = s;
  __syncthreads();
  if (g == 0 && o) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 32; ++k) t += red[k][fl];
    const float v = alpha * (float)t;
    *o = beta != 0.f ? v + beta * *o : v;
  }
}

__global__ __launch_bounds__(256) void colsum_partial_kernel(const PartLaunch L) {
  __shared__ float red[256];
  const int j = job_of_block(L.blk0, L.n);
  const PartJob& J = L.job[j];
  const int blk = (int)blockIdx.x - L.blk0[j];
  partial_of_rows(J, blk * J.rpb, min(J.rows, (blk + 1) * J.rpb), red, J.part + (long)blk * J.F);
}

// one block per 32 outputs of a job: 32 row groups x 32 columns of threads
__global__ __launch_bounds__(1024) void colsum_final_kernel(const FinalLaunch L) {
  __shared__ double red[32][33];
  const int j = job_of_block(L.blk0, L.n);
  const FinalJob& J = L.job[j];
  const int fl = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int f = ((int)blockIdx.x - L.blk0[j]) * 32 + fl;
  long o0 = -1, o1 = -1;                                // slab column(s) behind output f
  float* o = nullptr;                                   // its destination
  if (J.kind == 0) {
    if (f < J.F) { o0 = f; o = f < J.split ? J.out + f : J.out2 + (f - J.split); }
  } else {
    const int Ci = J.Ci, nw = 9 * Ci * 8;
    if (f < nw) {
      const int co = f & 7, ci = (f >> 3) % Ci, t = (f >> 3) / Ci, ti = t / 3, tj = t - ti * 3;
      o0 = ((ti * 4 + tj) * Ci + ci) * 16 + co;
      o1 = ((ti * 4 + tj + 1) * Ci + ci) * 16 + 8 + co;
      o = J.out + f;
    } else if (f < nw + 8 && J.out2) { o0 = 12 * Ci * 16 + (f - nw); o1 = o0 + 8; o = J.out2 + (f - nw); }
  }
  double s = 0.0;
  if (o) s = J.kind == 0 ? walk_partials<false>(J.part, J.ld, J.nblk, g, o0, o1) : walk_partials<true>(J.part, J.ld, J.nblk, g, o0, o1);
  tree_write(s, red, g, fl, o, J.alpha, J.beta);
}

static int final_launch(FinalLaunch& L, hipStream_t s) {
  int blocks = 0;
  for (int j = 0; j < L.n; ++j) { L.blk0[j] = blocks; blocks += ((L.job[j].kind ? 9 * L.job[j].Ci * 8 + 8 : L.job[j].F) + 31) / 32; }
  hipLaunchKernelGGL(colsum_final_kernel, dim3(blocks), dim3(1024), 0, s, L);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}
static int final_launch_one(const FinalJob& J, void* stream) {
  FinalLaunch L;
  L.n = 1; L.job[0] = J;
  return final_launch(L, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Deferred slab reductions.  Every weight-gradient launch of the lip CNN leaves per-workgroup partial slabs that a tiny kernel then sums
// (5 us of launch latency for ~1 MB, twelve times per step, each in line behind its convolution).  Nothing reads a weight gradient
// before the optimiser, so between avsr_slab_defer_begin() and avsr_slab_defer_end() those reductions are only RECORDED (the caller
// gives every convolution its own scratch region) and run as ONE launch at the end.
static thread_local bool g_slab_defer = false;
static thread_local FinalLaunch g_slab_jobs;
static int slab_flush(hipStream_t s) {
  if (!g_slab_jobs.n) return AVSR_OK;
  const int rc = final_launch(g_slab_jobs, s);
  g_slab_jobs.n = 0;
  return rc;
}
bool slab_deferring() { return g_slab_defer; }
int slab_reduce(const float* part, long ld, int nblk, int F, float* out, float* out2, int split, int kind, int Ci, float alpha, float beta,
                hipStream_t s) {
  const FinalJob J{part, ld, nblk, F, out, out2, split, kind, Ci, alpha, beta};
  if (!g_slab_defer) return final_launch_one(J, s);
  if (g_slab_jobs.n == RED_JOBS) { const int rc = slab_flush(s); if (rc != AVSR_OK) return rc; }
  g_slab_jobs.job[g_slab_jobs.n++] = J;
  return AVSR_OK;
}

}  // namespace avsr

using namespace avsr;

extern "C" int avsr_slab_defer_begin(void) {
  g_slab_jobs.n = 0;                                    // (a collection left open by an aborted pass is dropped)
  g_slab_defer = true;
  return AVSR_OK;
}
extern "C" int avsr_slab_defer_end(void* stream) {
  g_slab_defer = false;
  return slab_flush((hipStream_t)stream);
}

int avsr_colsum_final_launch(const float* part, int nblk, float* out, int F, float alpha, float beta, void* stream) {
  return final_launch_one(FinalJob{part, (long)F, nblk, F, out, nullptr, 0x7fffffff, 0, 0, alpha, beta}, stream);
}
int avsr_colsum_final_launch_split(const float* part, long ld, int nblk, float* out, float* out2, int split, int F, float alpha, float beta,
                                   void* stream) {
  return final_launch_one(FinalJob{part, ld, nblk, F, out, out2, split, 0, 0, alpha, beta}, stream);
}

extern "C" int avsr_colsum(const avsr_mat* a, const avsr_mat* b, int32_t rows, int32_t F, float alpha, float beta,
                           float* out, float* scratch, int64_t scratch_floats, void* stream) {
  if (!a || !a->ptr || !out || !scratch || rows <= 0 || F <= 0) return AVSR_ERR_ARG;
  const int maxblk = 2048;                                     // at most 2048 partial rows: the final pass stays one short launch
  int rpb = rows > 32 * maxblk ? (rows + maxblk - 1) / maxblk : 32;
  int nblk = (rows + rpb - 1) / rpb;
  if ((long)nblk * F > scratch_floats) {
    nblk = (int)(scratch_floats / F);
    if (nblk < 1) return AVSR_ERR_ARG;
    rpb = (rows + nblk - 1) / nblk;
    nblk = (rows + rpb - 1) / rpb;
  }
  PartLaunch P;
  P.n = 1; P.blk0[0] = 0;
  P.job[0] = PartJob{a->ptr, b ? b->ptr : nullptr, scratch, (long)a->ld, (long)a->ldo, b ? (long)b->ld : 0, b ? (long)b->ldo : 0,
                     a->T, b ? b->T : 0, rows, F, rpb};
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, P);
  AVSR_CHECK_LAUNCH();
  return avsr_colsum_final_launch(scratch, nblk, out, F, alpha, beta, stream);
}

// Many column sums in TWO launches (bias gradients of a train step: one per cell / layer, each a pass over a [B*T, F] record
// followed by a tiny reduction -- 12 + 33 launches of ~5-20 us before; seq2seq.py:222 tf.gradients of the `bias` variables).
extern "C" int avsr_colsum_multi(const avsr_colsum_job* jobs, int32_t n, float* scratch, int64_t scratch_floats, void* stream) {
  if (n <= 0) return AVSR_OK;
  if (!jobs || !scratch) return AVSR_ERR_ARG;
  for (int j0 = 0; j0 < n; j0 += RED_JOBS) {             // more than 32 jobs: consecutive launch pairs
    PartLaunch P;
    FinalLaunch L;
    P.n = L.n = n - j0 < RED_JOBS ? n - j0 : RED_JOBS;
    long used = 0;
    int blocks = 0;
    for (int k = 0; k < P.n; ++k) {
      const avsr_colsum_job& Q = jobs[j0 + k];
      if (!Q.a.ptr || !Q.out || Q.rows <= 0 || Q.F <= 0) return AVSR_ERR_ARG;
      // <= 256 partial rows per job (the big records are [32000, 1024]: 125 rows per block), >= 32 rows per block
      int rpb = (Q.rows + 255) / 256;
      if (rpb < 32) rpb = 32;
      const int nblk = (Q.rows + rpb - 1) / rpb;
      P.job[k] = PartJob{Q.a.ptr, Q.b.ptr, scratch + used, (long)Q.a.ld, (long)Q.a.ldo, (long)Q.b.ld, (long)Q.b.ldo, Q.a.T, Q.b.T, Q.rows, Q.F, rpb};
      L.job[k] = FinalJob{scratch + used, (long)Q.F, nblk, Q.F, Q.out, nullptr, 0x7fffffff, 0, 0, Q.alpha, Q.beta};
      used += (long)nblk * Q.F;
      P.blk0[k] = blocks; blocks += nblk;
    }
    if (used > scratch_floats) return AVSR_ERR_ARG;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P);
    AVSR_CHECK_LAUNCH();
    const int rc = final_launch(L, (hipStream_t)stream);
    if (rc != AVSR_OK) return rc;
  }
  return AVSR_OK;
}

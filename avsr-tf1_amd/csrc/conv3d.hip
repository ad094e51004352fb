// Spatio-temporal convolutions of the 3dconv_cnn lip front-end (avsr/video.py:34-46 conv3d_wrapper, :92-105 residual_block_3d,
// :198-222 conv3d_cnn): tf.layers.conv3d over NDHWC maps [B, T, H, W, C], no bias, TF SAME padding per axis, temporal stride 1.
//
// All three products run as implicit GEMMs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate):
//   forward      y[pos][co]          = sum_{tap, ci} src(pos, tap)[ci] * w[tap][ci][co]
//   data grad    dx[pos][ci]         = sum_{tap, co} dy(pos, tap)[co] * w[tap][ci][co]      (gather form: every dx pixel written once)
//   weight grad  dw[tap][ci][co]     = sum_{pos} x(pos, tap)[ci] * dy[pos][co]              (split over positions, deterministic reduction)
// The forward and the data gradient share one kernel (c3_gather_kernel): a workgroup of four waves owns 128 destination positions by up
// to 64 destination channels; the kernel taps of the current stage sit in LDS as the B operand, the A operand is gathered from global
// memory (float4 per lane along the channels; neighbouring taps and frames hit the L1 / L2 copies of the same lines).
// Loader transform (forward and weight gradient): the source is max(x*scale[c] + shift[c], 0) -- the consumer-side batch_norm_relu
// of video.py:4-14, so the normalised map is never written -- or, with relu = 0, the plain affine x*scale + shift (layer 0's
// `inputs * 2 - 1`).  Zero padding is inserted AFTER the transform, as in the graph.  Forward epilogue: optional residual add (itself
// optionally a lazily normalised map) and per-workgroup batch-norm partial sums of what it wrote.
#include "common.h"
#include "prof.h"
#include "avsr_hip.h"

using namespace avsr;

#ifndef S_
#define S_(x) ((hipStream_t)(x))
#endif
#define C3_STAGE_FLOATS 16384     // LDS floats of staged kernel taps per workgroup (64 KiB: two workgroups per CU in 160 KiB)
#define C3_MAX_PARTS 512          // statistic partial rows (one per workgroup of the forward launch)

namespace {

struct C3Args {
  const float* src; const float* w; float* dst;
  const float* res; const float* res_sc; const float* res_sh;
  const float* sc; const float* sh; float* stats;
  int B, T, SH, SW, Cs, DH, DW, Cd;
  int kt, kh, kw, S, pf, pt, pl;
  int CsL;                 // K rows per tap: Cs, or 4 for Cs < 4 (masked)
  int relu;                // loader transform: 1 = max(x*sc + sh, 0), 0 = x*sc + sh (sc == NULL: none)
  float beta;              // data gradient: dx = beta*dx + ...
  int M;                   // destination positions B*T*DH*DW
  int ntile;               // tiles of 128 positions
  int tps;                 // taps per LDS stage
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// TR = false: forward (src = x, dst = y, K rows (tap, ci)); TR = true: data gradient (src = dy, dst = dx, K rows (tap, co)).
template <int NT, bool TR>
__global__ __launch_bounds__(256, 2) void c3_gather_kernel(const C3Args A) {
  constexpr int P = NT * 16 + 4;                       // LDS pitch of a K row (the four lane groups land 16 banks apart)
  __shared__ float wl[C3_STAGE_FLOATS];
  __shared__ int tab[C3_STAGE_FLOATS / (4 * 20)];      // per 4-row group of the stage: tap (a, b, c) and first channel
  __shared__ float lsc[128], lsh[128];
  __shared__ float red[4][2][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const int cg = blockIdx.y * 64;
  const int taps = A.kt * A.kh * A.kw;
  const int nstage = (taps + A.tps - 1) / A.tps;
  if (A.sc) for (int i = tid; i < A.Cs && i < 128; i += 256) { lsc[i] = A.sc[i]; lsh[i] = A.sh[i]; }

  auto stage = [&](int tap0) {
    const int nt = min(A.tps, taps - tap0), rows = nt * A.CsL, rows16 = (rows + 15) & ~15;
    for (int i = tid; i < rows16 * P; i += 256) {
      const int r = i / P, n = i - r * P, col = cg + n;
      float v = 0.f;
      if (r < rows && n < NT * 16 && col < A.Cd) {
        const int tap = tap0 + r / A.CsL, ks = r % A.CsL;
        if (ks < A.Cs) v = TR ? A.w[((long)tap * A.Cd + col) * A.Cs + ks] : A.w[((long)tap * A.Cs + ks) * A.Cd + col];
      }
      wl[i] = v;
    }
    for (int q = tid; q < rows16 / 4; q += 256) {
      const int r = q * 4, tap = tap0 + min(r, rows - 1) / A.CsL, ks = r % A.CsL;
      const int a = tap / (A.kh * A.kw), b = (tap / A.kw) % A.kh, c = tap % A.kw;
      tab[q] = r < rows ? (a | (b << 4) | (c << 8) | (ks << 12)) : -1;
    }
  };
  if (nstage == 1) stage(0);
  __syncthreads();

  float s1[NT], s2[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) { s1[j] = 0.f; s2[j] = 0.f; }

  for (int tile = blockIdx.x; tile < A.ntile; tile += gridDim.x) {
    // this lane's A-operand row of each of the wave's two m tiles
    int pb[2], pt_[2], py[2], px[2];
    bool pv[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int p = tile * 128 + wv * 32 + mt * 16 + l16;
      pv[mt] = p < A.M;
      const int q = pv[mt] ? p : 0;
      px[mt] = q % A.DW;
      const int r = q / A.DW;
      py[mt] = r % A.DH;
      const int f = r / A.DH;
      pt_[mt] = f % A.T;
      pb[mt] = f / A.T;
    }
    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int st = 0; st < nstage; ++st) {
      const int tap0 = st * A.tps;
      if (nstage > 1) { __syncthreads(); stage(tap0); __syncthreads(); }
      const int rows = min(A.tps, taps - tap0) * A.CsL;
      for (int k0 = 0; k0 < rows; k0 += 16) {
        const int t4 = tab[(k0 >> 2) + g];
        float av[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
          for (int e = 0; e < 4; ++e) av[mt][e] = 0.f;
          if (t4 < 0 || !pv[mt]) continue;
          const int a = t4 & 15, b = (t4 >> 4) & 15, c = (t4 >> 8) & 15, ks = t4 >> 12;
          int ts, hs, ws;
          bool ok;
          if (!TR) {
            ts = pt_[mt] + a - A.pf; hs = py[mt] * A.S + b - A.pt; ws = px[mt] * A.S + c - A.pl;
            ok = ts >= 0 && ts < A.T && hs >= 0 && hs < A.SH && ws >= 0 && ws < A.SW;
          } else {
            ts = pt_[mt] + A.pf - a;
            const int hh = py[mt] + A.pt - b, ww = px[mt] + A.pl - c, sm = A.S - 1, sh = A.S >> 1;
            ok = ts >= 0 && ts < A.T && hh >= 0 && ww >= 0 && !(hh & sm) && !(ww & sm);
            hs = hh >> sh; ws = ww >> sh;
            ok = ok && hs < A.SH && ws < A.SW;
          }
          if (!ok) continue;
          const float* sp = A.src + ((((long)pb[mt] * A.T + ts) * A.SH + hs) * A.SW + ws) * A.Cs + ks;
          if (A.Cs >= 4) {
            const f32x4 v = ld4(sp);
            av[mt][0] = v[0]; av[mt][1] = v[1]; av[mt][2] = v[2]; av[mt][3] = v[3];
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < A.Cs) av[mt][e] = sp[e];
          }
          if (!TR && A.sc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (ks + e < A.Cs) {
                const float u = fmaf(av[mt][e], lsc[ks + e], lsh[ks + e]);
                av[mt][e] = A.relu ? fmaxf(u, 0.f) : u;
              }
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float* wr = wl + (k0 + 4 * g + e) * P + l16;
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const float bv = wr[j * 16];
            acc[0][j] = mfma4(av[0][e], bv, acc[0][j]);
            acc[1][j] = mfma4(av[1][e], bv, acc[1][j]);
          }
        }
      }
    }
    // epilogue: D row (lane >> 4)*4 + i of each m tile, column lane & 15 of each n tile
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tile * 128 + wv * 32 + mt * 16 + g * 4 + i;
        if (p >= A.M) continue;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int n = cg + j * 16 + l16;
          if (n >= A.Cd) continue;
          const long o = (long)p * A.Cd + n;
          float v = acc[mt][j][i];
          if (TR) {
            if (A.beta != 0.f) v += A.beta * A.dst[o];
          } else if (A.res) {
            float r = A.res[o];
            if (A.res_sc) r = fmaxf(fmaf(r, A.res_sc[n], A.res_sh[n]), 0.f);
            v += r;
          }
          A.dst[o] = v;
          s1[j] += v;
          s2[j] += v * v;
        }
      }
    }
  }
  if (TR || !A.stats) return;
  // per-workgroup statistics: lane groups, then waves in a fixed order (deterministic)
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    float a = s1[j], b = s2[j];
    a += __shfl_xor(a, 16); a += __shfl_xor(a, 32);
    b += __shfl_xor(b, 16); b += __shfl_xor(b, 32);
    if (lane < 16) { red[wv][0][j * 16 + lane] = a; red[wv][1][j * 16 + lane] = b; }
  }
  __syncthreads();
  if (tid < NT * 16) {
    const int n = cg + tid;
    if (n < A.Cd) {
      const float a = (red[0][0][tid] + red[1][0][tid]) + (red[2][0][tid] + red[3][0][tid]);
      const float b = (red[0][1][tid] + red[1][1][tid]) + (red[2][1][tid] + red[3][1][tid]);
      A.stats[(long)blockIdx.x * 2 * A.Cd + n] = a;
      A.stats[(long)blockIdx.x * 2 * A.Cd + A.Cd + n] = b;
    }
  }
}

struct C3WArgs {
  const float* x; const float* dy; float* part;
  const float* sc; const float* sh; int relu;
  int B, T, H, W, Ci, Ho, Wo, Co;
  int kt, kh, kw, S, pf, pt, pl;
  int M;                   // K rows of the kernel: taps * Ci
  long P;                  // output positions B*T*Ho*Wo
  long chunk;              // positions per split (multiple of 4)
};

// Weight gradient: a workgroup owns 256 rows (tap, ci) of dw (4 waves x 4 m tiles) by up to 64 columns co and one split of the
// positions; A = x gathered at (position, tap) [row][k = position], B = dy [k = position][co].  Partial slab [split][M][Co].
template <int NT>
__global__ __launch_bounds__(256, 2) void c3_wgrad_kernel(const C3WArgs A) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const int cg = blockIdx.z * 64;
  const long p0 = (long)blockIdx.y * A.chunk;
  const long p1 = min(p0 + A.chunk, A.P);
  if (p0 >= p1) return;
  int ra[4], rb[4], rc[4], rci[4];
  bool rv[4];
  float rsc[4], rsh[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int r = (blockIdx.x * 16 + wv * 4 + mt) * 16 + l16;
    rv[mt] = r < A.M;
    const int rr = rv[mt] ? r : 0, tap = rr / A.Ci;
    rci[mt] = rr - tap * A.Ci;
    ra[mt] = tap / (A.kh * A.kw); rb[mt] = (tap / A.kw) % A.kh; rc[mt] = tap % A.kw;
    rsc[mt] = A.sc ? A.sc[rci[mt]] : 1.f;
    rsh[mt] = A.sc ? A.sh[rci[mt]] : 0.f;
  }
  if ((blockIdx.x * 16 + wv * 4) * 16 >= A.M) return;     // a whole wave past the last row (no barriers in this kernel)
  // this lane's position p = p0 + g (+4 per step), decoded once and advanced with carries
  long p = p0 + g;
  int px, py, pt, pb;
  {
    const long q = p < A.P ? p : 0;
    px = (int)(q % A.Wo);
    const long r = q / A.Wo;
    py = (int)(r % A.Ho);
    const long f = r / A.Ho;
    pt = (int)(f % A.T);
    pb = (int)(f / A.T);
  }
  f32x4 acc[4][NT];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long pbase = p0; pbase < p1; pbase += 4) {
    const bool ok = p < p1;
    float bv[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = cg + j * 16 + l16;
      bv[j] = (ok && n < A.Co) ? A.dy[p * A.Co + n] : 0.f;
    }
    float av[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      av[mt] = 0.f;
      const int ts = pt + ra[mt] - A.pf, hs = py * A.S + rb[mt] - A.pt, ws = px * A.S + rc[mt] - A.pl;
      if (ok && rv[mt] && ts >= 0 && ts < A.T && hs >= 0 && hs < A.H && ws >= 0 && ws < A.W) {
        float v = A.x[((((long)pb * A.T + ts) * A.H + hs) * A.W + ws) * A.Ci + rci[mt]];
        if (A.sc) { v = fmaf(v, rsc[mt], rsh[mt]); if (A.relu) v = fmaxf(v, 0.f); }
        av[mt] = v;
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[mt][j] = mfma4(av[mt], bv[j], acc[mt][j]);
    p += 4;
    px += 4;
    while (px >= A.Wo) {
      px -= A.Wo;
      if (++py >= A.Ho) { py = 0; if (++pt >= A.T) { pt = 0; ++pb; } }
    }
  }
  float* part = A.part + (long)blockIdx.y * A.M * A.Co;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (blockIdx.x * 16 + wv * 4 + mt) * 16 + g * 4 + i;
      if (r >= A.M) continue;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = cg + j * 16 + l16;
        if (n < A.Co) part[(long)r * A.Co + n] = acc[mt][j][i];
      }
    }
  }
}

__global__ void c3_slab_sum_kernel(const float* part, int nsplit, long n, float* out, float beta) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < nsplit; ++k) s += part[(long)k * n + i];
  out[i] = beta != 0.f ? beta * out[i] + s : s;
}

bool desc_ok(const avsr_conv3d_desc* c) {
  if (!c || c->B <= 0 || c->T <= 0 || c->H <= 0 || c->W <= 0 || c->Ci <= 0 || c->Co <= 0) return false;
  if (c->kt < 1 || c->kt > 3 || c->kh < 1 || c->kh > 3 || c->kw < 1 || c->kw > 3) return false;
  if (c->stride != 1 && c->stride != 2) return false;
  if (c->Ci > 128 || (c->Ci >= 4 && c->Ci % 4) || c->Co % 4 || c->Co > 128) return false;
  if (c->pad_f < 0 || c->pad_f >= c->kt || c->pad_t < 0 || c->pad_t >= c->kh || c->pad_l < 0 || c->pad_l >= c->kw) return false;
  if (c->Ho <= 0 || c->Wo <= 0 || (c->Ho - 1) * c->stride - c->pad_t >= c->H || (c->Wo - 1) * c->stride - c->pad_l >= c->W) return false;
  if (c->scale && !c->shift) return false;
  return true;
}

int nt_of(int cols) { return cols >= 64 ? 4 : (cols + 15) / 16; }

int launch_gather(const C3Args& a0, int cols, bool tr, hipStream_t s) {
  C3Args a = a0;
  const int NT = nt_of(cols);
  const int P = NT * 16 + 4, taps = a.kt * a.kh * a.kw;
  int tps = (C3_STAGE_FLOATS / P) / a.CsL;             // whole taps of K rows per stage (rows rounded to 16 below)
  while (tps > 0 && ((tps * a.CsL + 15) & ~15) * P > C3_STAGE_FLOATS) --tps;
  if (tps < 1) return AVSR_ERR_UNSUPPORTED;
  a.tps = tps < taps ? tps : taps;
  a.ntile = (a.M + 127) / 128;
  const int gx = a.ntile < C3_MAX_PARTS ? a.ntile : C3_MAX_PARTS;
  dim3 grid(gx, (cols + 63) / 64);
#define C3_G(n) do { if (tr) hipLaunchKernelGGL((c3_gather_kernel<n, true>), grid, dim3(256), 0, s, a); \
                     else hipLaunchKernelGGL((c3_gather_kernel<n, false>), grid, dim3(256), 0, s, a); } while (0)
  switch (NT) { case 1: C3_G(1); break; case 2: C3_G(2); break; case 3: C3_G(3); break; default: C3_G(4); break; }
#undef C3_G
  return hipGetLastError() == hipSuccess ? gx : AVSR_ERR_HIP;
}

long wgrad_splits(const avsr_conv3d_desc* c, long* chunk) {
  const int M = c->kt * c->kh * c->kw * c->Ci;
  const long P = (long)c->B * c->T * c->Ho * c->Wo;
  const long wgs = (long)((M + 255) / 256) * ((c->Co + 63) / 64);
  long sp = 1024 / wgs;
  if (sp < 1) sp = 1;
  if (sp > 512) sp = 512;
  long ch = (P + sp - 1) / sp;
  if (ch < 256) ch = 256;
  ch = (ch + 3) & ~3L;
  sp = (P + ch - 1) / ch;
  if (chunk) *chunk = ch;
  return sp;
}

}  // namespace

extern "C" int avsr_conv3d_supported(const avsr_conv3d_desc* c) { return desc_ok(c) ? 1 : 0; }

extern "C" int64_t avsr_conv3d_wgrad_scratch_floats(const avsr_conv3d_desc* c) {
  if (!desc_ok(c)) return -1;
  return (int64_t)wgrad_splits(c, nullptr) * c->kt * c->kh * c->kw * c->Ci * c->Co;
}

static C3Args base_args(const avsr_conv3d_desc* c) {
  C3Args a{};
  a.B = c->B; a.T = c->T; a.kt = c->kt; a.kh = c->kh; a.kw = c->kw; a.S = c->stride;
  a.pf = c->pad_f; a.pt = c->pad_t; a.pl = c->pad_l;
  return a;
}

extern "C" int avsr_conv3d_fwd(const avsr_conv3d_desc* c, const float* x, const float* w, const float* res, const float* res_scale,
                               const float* res_shift, float* y, float* stats, int32_t* nparts, void* stream) {
  if (!desc_ok(c)) return c ? AVSR_ERR_UNSUPPORTED : AVSR_ERR_ARG;
  if (!x || !w || !y || (stats && !nparts) || (res_scale && (!res || !res_shift))) return AVSR_ERR_ARG;
  C3Args a = base_args(c);
  a.src = x; a.w = w; a.dst = y; a.res = res; a.res_sc = res_scale; a.res_sh = res_shift; a.sc = c->scale; a.sh = c->shift;
  a.stats = stats; a.relu = c->relu;
  a.SH = c->H; a.SW = c->W; a.Cs = c->Ci; a.DH = c->Ho; a.DW = c->Wo; a.Cd = c->Co;
  a.CsL = c->Ci < 4 ? 4 : c->Ci;
  a.M = c->B * c->T * c->Ho * c->Wo;
  const double flops = 2.0 * a.M * c->Co * c->kt * c->kh * c->kw * c->Ci;
  ProfScope ps(PROF_CONV_FWD, S_(stream), flops);
  const int n = launch_gather(a, c->Co, false, S_(stream));
  if (n < 0) return n;
  if (nparts) *nparts = stats ? n : 0;
  return AVSR_OK;
}

extern "C" int avsr_conv3d_bwd_data(const avsr_conv3d_desc* c, const float* dy, const float* w, float* dx, float beta, void* stream) {
  if (!desc_ok(c)) return c ? AVSR_ERR_UNSUPPORTED : AVSR_ERR_ARG;
  if (!dy || !w || !dx) return AVSR_ERR_ARG;
  C3Args a = base_args(c);
  a.src = dy; a.w = w; a.dst = dx; a.beta = beta;
  a.SH = c->Ho; a.SW = c->Wo; a.Cs = c->Co; a.DH = c->H; a.DW = c->W; a.Cd = c->Ci;
  a.CsL = c->Co;
  a.M = c->B * c->T * c->H * c->W;
  const double flops = 2.0 * c->B * c->T * c->Ho * c->Wo * c->Co * c->kt * c->kh * c->kw * c->Ci;
  ProfScope ps(PROF_CONV_BWD_DATA, S_(stream), flops);
  const int n = launch_gather(a, c->Ci, true, S_(stream));
  return n < 0 ? n : AVSR_OK;
}

extern "C" int avsr_conv3d_bwd_weight(const avsr_conv3d_desc* c, const float* x, const float* dy, float* dw, float beta, float* scratch,
                                      int64_t scratch_floats, void* stream) {
  if (!desc_ok(c)) return c ? AVSR_ERR_UNSUPPORTED : AVSR_ERR_ARG;
  if (!x || !dy || !dw || !scratch) return AVSR_ERR_ARG;
  long chunk = 0;
  const long sp = wgrad_splits(c, &chunk);
  const int M = c->kt * c->kh * c->kw * c->Ci;
  if (scratch_floats < sp * M * c->Co) return AVSR_ERR_ARG;
  C3WArgs a{};
  a.x = x; a.dy = dy; a.part = scratch; a.sc = c->scale; a.sh = c->shift; a.relu = c->relu;
  a.B = c->B; a.T = c->T; a.H = c->H; a.W = c->W; a.Ci = c->Ci; a.Ho = c->Ho; a.Wo = c->Wo; a.Co = c->Co;
  a.kt = c->kt; a.kh = c->kh; a.kw = c->kw; a.S = c->stride; a.pf = c->pad_f; a.pt = c->pad_t; a.pl = c->pad_l;
  a.M = M; a.P = (long)c->B * c->T * c->Ho * c->Wo; a.chunk = chunk;
  const double flops = 2.0 * a.P * M * c->Co;
  ProfScope ps(PROF_CONV_BWD_WEIGHT, S_(stream), flops);
  dim3 grid((M + 255) / 256, (unsigned)sp, (c->Co + 63) / 64);
  switch (nt_of(c->Co)) {
    case 1: hipLaunchKernelGGL(c3_wgrad_kernel<1>, grid, dim3(256), 0, S_(stream), a); break;
    case 2: hipLaunchKernelGGL(c3_wgrad_kernel<2>, grid, dim3(256), 0, S_(stream), a); break;
    case 3: hipLaunchKernelGGL(c3_wgrad_kernel<3>, grid, dim3(256), 0, S_(stream), a); break;
    default: hipLaunchKernelGGL(c3_wgrad_kernel<4>, grid, dim3(256), 0, S_(stream), a); break;
  }
  if (hipGetLastError() != hipSuccess) return AVSR_ERR_HIP;
  const long n = (long)M * c->Co;
  hipLaunchKernelGGL(c3_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S_(stream), scratch, (int)sp, n, dw, beta);
  return hipGetLastError() == hipSuccess ? AVSR_OK : AVSR_ERR_HIP;
}

// Waveform audio front-end: padded waveforms [B, N] -> stacked log-mel features [B, T_out, F] in ONE launch (fp32, gfx950).
//
// The pipeline is the dataset writer's (avsr/audio.py compute_stfts / compute_log_mel_spectrograms, avsr/dataset_writer.py
// _stack_features): frame t = x[step*t : step*t + frame_length] * periodic Hann, zero-padded to 512 -> real FFT -> magnitude -> mel
// triangles -> log(. + 1e-6) -> rows of `window` frames taken every `stride` frames.  The [B, frames, 257] spectrum never leaves the CU.
//
// Work split: a workgroup of 4 waves owns LM_FC = 16 consecutive frames of one utterance, one wave per frame at a time.  The 512-point
// real FFT is a 256-point complex FFT of z[k] = x[2k] + i x[2k+1] followed by the split step.  The complex FFT is a radix-4 Stockham
// autosort (4 passes, 4 points per lane): pass 0 reads the samples from global memory, the other three exchange through the wave's own
// LDS slice (re / im planes, index i stored at i + i/32: the pass-0 stores, 4 dwords apart, then fall on 32 distinct banks and the
// pass-1 stores are two-way at worst; every load is unit-stride).  The mel reduction is a gather per filter over its contiguous bin
// range (each bin feeds at most two filters: <= 514 weights in all), so the summation order is fixed.  Every frame's log-mel vector is
// staged in LDS and stored to each output row that holds it (frame f is slot j of row r when f = stride*r + j); rows at and beyond an
// utterance's length and the columns beyond num_mel_bins*window are stored as zeros, so every output element is written exactly once.
#include "common.h"
#include "avsr_hip.h"

namespace avsr {

constexpr int LM_FC = 16;          // frames per workgroup
constexpr int LM_FPW = LM_FC / 4;  // frames per wave
constexpr int LM_FFT = 512;
constexpr int LM_NC = LM_FFT / 2;  // complex points
constexpr int LM_BINS = LM_NC + 1;
constexpr int LM_MAXM = 128;
constexpr int LM_MAXWIN = 16;

__device__ __forceinline__ int lm_slot(int i) { return i + (i >> 5); }

__device__ __forceinline__ void lm_fft4(float* re, float* im) {
  const float a0r = re[0] + re[2], a0i = im[0] + im[2], a1r = re[0] - re[2], a1i = im[0] - im[2];
  const float a2r = re[1] + re[3], a2i = im[1] + im[3];
  const float a3r = im[1] - im[3], a3i = re[3] - re[1];                 // (v1 - v3) * (-i)
  re[0] = a0r + a2r; im[0] = a0i + a2i;
  re[1] = a1r + a3r; im[1] = a1i + a3i;
  re[2] = a0r - a2r; im[2] = a0i - a2i;
  re[3] = a1r - a3r; im[3] = a1i - a3i;
}

__device__ __forceinline__ void lm_frame_lengths(const avsr_logmel_args& A, int b, int& n, int& frames, int& rows) {
  n = A.wav_len[b];
  n = n < 0 ? 0 : (n > A.N ? A.N : n);
  frames = n >= A.frame_length ? 1 + (n - A.frame_length) / A.frame_step : 0;
  rows = frames >= A.window ? (frames - A.window) / A.stride + 1 : 0;
  if (rows > A.T_out) rows = A.T_out;
}

__global__ __launch_bounds__(256) void logmel_kernel(const avsr_logmel_args A) {
  __shared__ float s_re[4][LM_NC + 8], s_im[4][LM_NC + 8];
  __shared__ float s_mag[4][LM_BINS + 3];
  __shared__ float s_lm[LM_FC][LM_MAXM];
  const int b = blockIdx.y, f0 = blockIdx.x * LM_FC;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int M = A.num_mel_bins;
  int n, frames_b, rows_b;
  lm_frame_lengths(A, b, n, frames_b, rows_b);
  if (blockIdx.x == 0 && threadIdx.x == 0 && A.out_len) A.out_len[b] = rows_b;

  if (f0 < frames_b) {                                   // (block-uniform: a chunk of padding frames goes straight to the stores)
    const float2* tw = reinterpret_cast<const float2*>(A.twiddle);   // exp(-2 pi i k / 512), k < 512
    float win[8];
    float2 w1[3], w2[3], w3[3], wsplit[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i0 = 2 * (lane + 64 * r);
      win[2 * r] = i0 < A.frame_length ? A.hann[i0] : 0.f;
      win[2 * r + 1] = i0 + 1 < A.frame_length ? A.hann[i0 + 1] : 0.f;
      wsplit[r] = tw[lane + 64 * r];
    }
#pragma unroll
    for (int r = 1; r < 4; ++r) {                        // pass with Ns points per sub-transform: exp(-2 pi i r (lane % Ns) / (4 Ns))
      w1[r - 1] = tw[r * (lane & 3) * 32];
      w2[r - 1] = tw[r * (lane & 15) * 8];
      w3[r - 1] = tw[r * (lane & 63) * 2];
    }
    int mlo[2], mcnt[2], mptr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = lane + 64 * h;
      mlo[h] = mcnt[h] = mptr[h] = 0;
      if (m < M) {
        int lo = A.mel_lo[m], cnt = A.mel_cnt[m], p = A.mel_ptr[m];
        lo = lo < 0 ? 0 : (lo > LM_BINS ? LM_BINS : lo);
        p = p < 0 ? 0 : (p > A.mel_nnz ? A.mel_nnz : p);
        cnt = cnt < 0 ? 0 : cnt;
        if (cnt > LM_BINS - lo) cnt = LM_BINS - lo;
        if (cnt > A.mel_nnz - p) cnt = A.mel_nnz - p;
        mlo[h] = lo; mcnt[h] = cnt; mptr[h] = p;
      }
    }
    const float* x = A.wav + (long)b * A.N;
    float* sre = s_re[wv];
    float* sim = s_im[wv];
    float* smag = s_mag[wv];
#pragma unroll 1
    for (int i = 0; i < LM_FPW; ++i) {
      const int fl = wv * LM_FPW + i, f = f0 + fl;
      float re[4], im[4];
      if (f < frames_b) {                                // samples step*f .. step*f + frame_length - 1 < n <= N
        const float* xf = x + (long)f * A.frame_step;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i0 = 2 * (lane + 64 * r);
          re[r] = i0 < A.frame_length ? xf[i0] * win[2 * r] : 0.f;
          im[r] = i0 + 1 < A.frame_length ? xf[i0 + 1] * win[2 * r + 1] : 0.f;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) re[r] = im[r] = 0.f;
      }
      // pass 0 (Ns = 1): no twiddles; lane j stores to 4j + r
      lm_fft4(re, im);
#pragma unroll
      for (int r = 0; r < 4; ++r) { const int s = lm_slot(4 * lane + r); sre[s] = re[r]; sim[s] = im[r]; }
#pragma unroll
      for (int pass = 1; pass < 4; ++pass) {
        const int Ns = 1 << (2 * pass);
        const float2* w = pass == 1 ? w1 : (pass == 2 ? w2 : w3);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int s = lm_slot(lane + 64 * r); re[r] = sre[s]; im[r] = sim[s]; }
#pragma unroll
        for (int r = 1; r < 4; ++r) {
          const float tr = re[r] * w[r - 1].x - im[r] * w[r - 1].y;
          im[r] = re[r] * w[r - 1].y + im[r] * w[r - 1].x;
          re[r] = tr;
        }
        lm_fft4(re, im);
        __syncthreads();
        const int j0 = (lane / Ns) * Ns * 4 + (lane % Ns);
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int s = lm_slot(j0 + r * Ns); sre[s] = re[r]; sim[s] = im[r]; }
      }
      __syncthreads();
      // split step: X[k] = E + W512^k O, E = (Z[k] + conj Z[256-k]) / 2, O = (Z[k] - conj Z[256-k]) / (2i); |X[k]| for k <= 256
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = lane + 64 * r, s = lm_slot(k), sc = lm_slot((LM_NC - k) & (LM_NC - 1));
        const float zr = sre[s], zi = sim[s], cr = sre[sc], ci = -sim[sc];
        const float er = 0.5f * (zr + cr), ei = 0.5f * (zi + ci);
        const float orr = 0.5f * (zi - ci), oi = -0.5f * (zr - cr);
        const float xr = er + wsplit[r].x * orr - wsplit[r].y * oi;
        const float xi = ei + wsplit[r].x * oi + wsplit[r].y * orr;
        smag[k] = sqrtf(xr * xr + xi * xi);
        if (k == 0) smag[LM_NC] = fabsf(zr - zi);       // X[256] = Re Z[0] - Im Z[0]
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int m = lane + 64 * h;
        if (m < M) {
          float acc = 0.f;
          const float* wts = A.mel_w + mptr[h];
          const float* mg = smag + mlo[h];
          for (int c = 0; c < mcnt[h]; ++c) acc = fmaf(wts[c], mg[c], acc);
          s_lm[fl][m] = logf(acc + 1e-6f);
        }
      }
    }
  }
  __syncthreads();
  // stores: frame f is slot j of row r when f = stride*r + j
  const int MW = M * A.window;
  float* out = A.out + (long)b * A.T_out * A.F;
  for (int idx = threadIdx.x; idx < LM_FC * M; idx += 256) {
    const int fl = idx / M, m = idx - fl * M, f = f0 + fl;
    const float v = s_lm[fl][m];
    for (int j = 0; j < A.window; ++j) {
      const int d = f - j;
      if (d < 0 || d % A.stride) continue;
      const int r = d / A.stride;
      if (r < A.T_out) out[(long)r * A.F + j * M + m] = r < rows_b ? v : 0.f;
    }
  }
  const int padw = A.F - MW;                             // zero columns up to the consumer's row width
  for (int idx = threadIdx.x; idx < LM_FC * padw; idx += 256) {
    const int fl = idx / padw, c = idx - fl * padw, f = f0 + fl;
    if (f % A.stride) continue;
    const int r = f / A.stride;
    if (r < A.T_out) out[(long)r * A.F + MW + c] = 0.f;
  }
}

}  // namespace avsr

extern "C" int avsr_logmel_supported(int32_t frame_length, int32_t fft_length, int32_t num_mel_bins, int32_t window, int32_t stride) {
  using namespace avsr;
  return fft_length == LM_FFT && frame_length >= 1 && frame_length <= fft_length && num_mel_bins >= 1 && num_mel_bins <= LM_MAXM &&
         window >= 1 && window <= LM_MAXWIN && stride >= 1 && stride <= window;
}

extern "C" int avsr_logmel_fwd(const avsr_logmel_args* a, void* stream) {
  using namespace avsr;
  if (!a || !a->wav || !a->wav_len || !a->hann || !a->twiddle || !a->mel_lo || !a->mel_cnt || !a->mel_ptr || !a->mel_w || !a->out)
    return AVSR_ERR_ARG;
  if (a->B <= 0 || a->B > 65535 || a->N <= 0 || a->T_out <= 0 || a->frame_step <= 0 || a->mel_nnz <= 0) return AVSR_ERR_ARG;
  if (!avsr_logmel_supported(a->frame_length, a->fft_length, a->num_mel_bins, a->window, a->stride)) return AVSR_ERR_UNSUPPORTED;
  if (a->F < a->num_mel_bins * a->window) return AVSR_ERR_ARG;
  const long frames_pad = (long)(a->T_out - 1) * a->stride + a->window;      // every output row's frames
  const long gx = (frames_pad + LM_FC - 1) / LM_FC;
  if (gx > 0x7fffffffL) return AVSR_ERR_ARG;
  hipLaunchKernelGGL(logmel_kernel, dim3((unsigned)gx, (unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

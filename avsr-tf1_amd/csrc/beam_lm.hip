// Shallow-fusion language model inside beam search (avsr_beam_lm, include/avsr_hip.h): one step of avsr.LM's evaluate graph over the
// R = B * K hypothesis rows, queued ahead of every selection of avsr_attn_rnn_fwd_lm.
//
// The model is the decoder block with no attention memory, so its cell step IS the product the decoder's own beam step runs
// (beam_gemm.hip): layer 0   z = [emb[tok[r]] | h_0[parent[r]]] . W_0 + b_0 -> i, j, f, o -> c_0, h_0 of row r
//                  layer j   z = [h_{j-1}[r]  | h_j[parent[r]]] . W_j + b_j                 (own row below, parent's row behind)
// one launch of beam_gemm_kernel<LSTM> per layer -- 64 x 64 output tiles, operand rows gathered while they are staged, the previous
// state read out of the OTHER half of the [2][layers][R][H] ping-pong, so no row is overwritten while another row still needs it.
// A layer is parallel over its 4 H gate columns (1 x 256 at 640 rows: 160 workgroups); folding the layers of a 16-row tile into one
// workgroup would make each of the 40 tiles stream every weight by itself.
// beam_lm_out_kernel then closes the step: Dense(V) on the top layer's h as 16 x 16 MFMA tiles and log_softmax per row -> lm_logp.
#include "avsr_hip.h"
#include "prof.h"
#include "beam.h"
#include "beam_gemm.h"

namespace avsr {

// lm_logp[r, :] = log_softmax(h[r, :] . Wout + bout).  One 256-thread workgroup per 16 rows: wave w takes the 16-column tiles w, w + 4, ...
// of v_mfma_f32_16x16x4_f32 over the whole H (lane (i16, g) holds inputs kk + 4 g .. + 3 of row / column i16: one 16-byte load per
// operand and four products per 16 inputs, the pairing beam_step_kernel uses); the tile's logits meet in LDS [16][V], then 16 lanes
// per row reduce max and exp-sum.  Rows >= R: zero operands, nothing written.
__global__ __launch_bounds__(256) void beam_lm_out_kernel(const float* h, int R, int H, const float* wout_t, const float* bout, int V,
                                                          float* lm_logp) {
  extern __shared__ __attribute__((aligned(16))) float lg[];      // [16][V]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int row = blockIdx.x * 16 + i16;
  const bool arow = row < R;
  const float* xr = h + (long)(arow ? row : 0) * H;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int nct = (V + 15) >> 4;
  for (int c = wave; c < nct; c += 4) {
    const int v = c * 16 + i16;
    const bool bcol = v < V;
    const float* wr = wout_t + (long)(bcol ? v : 0) * H;
    f32x4 acc = zero;
    for (int kk = 0; kk < H; kk += 16) {
      const int k = kk + 4 * g;
      const bool kin = k < H;                                     // H % 4 == 0: a 16-byte piece is inside or outside as a whole
      f32x4 a = ld4(xr + (kin ? k : 0)), b = ld4(wr + (kin ? k : 0));
      if (!(arow && kin)) a = zero;
      if (!(bcol && kin)) b = zero;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
    }
    if (bcol) {
      const float bv = bout[v];
#pragma unroll
      for (int r = 0; r < 4; ++r) lg[(4 * g + r) * V + v] = acc[r] + bv;   // C layout: row 4 g + r, column i16
    }
  }
  __syncthreads();
  const int rl = tid >> 4, j = tid & 15, orow = blockIdx.x * 16 + rl;
  float mx = -INFINITY;
  for (int v = j; v < V; v += 16) mx = fmaxf(mx, lg[rl * V + v]);
  mx = group16_max(mx);
  float sum = 0.f;
  for (int v = j; v < V; v += 16) sum += expf(lg[rl * V + v] - mx);
  sum = group16_sum(sum);
  const float lse = mx + logf(sum);
  if (orow < R)
    for (int v = j; v < V; v += 16) lm_logp[(long)orow * V + v] = lg[rl * V + v] - lse;
}

// AVSR_OK, or why the step cannot run (decided on the host, nothing dereferenced)
int beam_lm_check(const avsr_beam_lm* m) {
  if (!m || m->n_layers < 1 || m->H <= 0 || m->E <= 0 || m->V <= 0 || m->n_rows <= 0) return AVSR_ERR_ARG;
  if (m->n_layers > AVSR_MAX_LM_LAYERS || m->H % 4 || m->E % 4 || m->V > 1024) return AVSR_ERR_UNSUPPORTED;
  if (!m->embedding || !m->wout_t || !m->bout || !m->state_c || !m->state_h || !m->lm_logp) return AVSR_ERR_ARG;
  for (int j = 0; j < m->n_layers; ++j)
    if (!m->wt[j] || !m->bias[j]) return AVSR_ERR_ARG;
  if (m->one_hot && m->E < m->V) return AVSR_ERR_ARG;
  // beam_gemm_kernel addresses its operands with 32-bit byte offsets
  const long H = m->H, E = m->E, kmax = (E > H ? E : H) + H, lim = 1L << 31;
  if ((long)m->V * E * 4 >= lim || (long)m->n_rows * H * 4 >= lim || 4 * H * kmax * 4 >= lim || (long)m->n_rows * m->V * 4 >= lim)
    return AVSR_ERR_UNSUPPORTED;
  return AVSR_OK;
}

int beam_lm_step_launch(const avsr_beam_lm& m, const int32_t* tok, const int32_t* parent_rows, int step, hipStream_t s) {
  const int R = m.n_rows, H = m.H, E = m.E, nl = m.n_layers;
  const long half = (long)nl * R * H, lay = (long)R * H;
  const int pin = step & 1, pout = (step + 1) & 1;
  if (step == 0) {                                  // MultiRNNCell.zero_state: the half step 0 reads
    DevBatch db(s);
    db.zero(m.state_c, sizeof(float) * half);
    db.zero(m.state_h, sizeof(float) * half);
    if (db.flush() != hipSuccess) return AVSR_ERR_HIP;
  }
  static thread_local BGLaunch G;
  for (int j = 0; j < nl; ++j) {
    ProfScope ps(PROF_STEP_LSTM_FWD, s);            // a cell step, booked like the decoder's
    G = BGLaunch{};
    BGProb& P = G.p[0];
    BGSrc& x = P.src[P.nsrc++];
    if (j == 0) { x.a = m.embedding; x.sb = E; x.gather = tok; x.K = E; }
    else { x.a = m.state_h + pout * half + (j - 1) * lay; x.sb = H; x.gather = nullptr; x.K = H; }     // this step's output of the layer below
    BGSrc& hp = P.src[P.nsrc++];
    hp.a = m.state_h + pin * half + j * lay; hp.sb = H; hp.gather = parent_rows; hp.K = H;
    P.R = R; P.N = 4 * H; P.wt = m.wt[j]; P.ldw = (j == 0 ? E : H) + H;
    P.ntx = (P.N + BG_T - 1) / BG_T; P.tile0 = 0;
    P.bias = m.bias[j]; P.c_in = m.state_c + pin * half + j * lay; P.parent = parent_rows;
    P.c_out = m.state_c + pout * half + j * lay; P.h_out = m.state_h + pout * half + j * lay;
    G.nprob = 1; G.ntiles = P.ntx * ((R + BG_T - 1) / BG_T);
    const int rc = beam_gemm_launch(G, true, s);
    if (rc) return rc;
  }
  ProfScope ps(PROF_STEP_LINEAR, s);                // output layer + log_softmax: a dense step
  hipLaunchKernelGGL(beam_lm_out_kernel, dim3((R + 15) / 16), dim3(256), sizeof(float) * 16 * m.V, s,
                     m.state_h + pout * half + (nl - 1) * lay, R, H, m.wout_t, m.bout, m.V, m.lm_logp);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}

}  // namespace avsr

extern "C" int avsr_beam_lm_supported(const avsr_beam_lm* lm) { return avsr::beam_lm_check(lm) == AVSR_OK ? 1 : 0; }

extern "C" int avsr_beam_lm_step(const avsr_beam_lm* lm, const int32_t* tok, const int32_t* parent_rows, int32_t n_rows, int32_t step,
                                 void* stream) {
  if (!lm || !tok || !parent_rows || n_rows <= 0 || step < 0) return AVSR_ERR_ARG;
  const int rc = avsr::beam_lm_check(lm);
  if (rc) return rc;
  if (n_rows != lm->n_rows) return AVSR_ERR_ARG;
  return avsr::beam_lm_step_launch(*lm, tok, parent_rows, step, (hipStream_t)stream);
}

// Host-side scheduler for the attention-wrapped LSTM sequence (decoder train / greedy, AV-Align
// top encoder layer) -- see avsr_hip.h for the contract and the reference call sites.
//
// Forward chain per step:  [LSTM step] -> [Bahdanau query layer]* -> [attention partials] ->
//                          [attention layer (merges partials)] -> ([logits] -> [sample])^greedy
// Backward chain per step: [d attention] -> [d context] -> [attention backward] -> [partial sums]
//                          -> [LSTM backward]
// Every box is one launch covering all mechanisms; weight/keys gradients are deferred to post-loop
// GEMMs over all L steps (done by the caller with avsr_gemm).
#include "step.h"
#include "attn.h"
#include "beam.h"          // the selection step, the LM / CTC steps ahead of it
#include "beam_gemm.h"     // the tiled cell / attention-layer steps of mode 3
#include "dec_persist.h"   // the fused launches tried first
#include "cell_state.h"    // the layout of `state` / `dstate`

extern "C" int avsr_step_launch_raw(const void* launch, void* stream);                  // step.hip
extern "C" int avsr_attn_launch_raw(const void* launch, int backward, void* stream);    // attention.hip

namespace avsr {

struct SlabJob {
  float* dst; long dst_sb;
  const float* add; long add_sb;
  const float* src[AVSR_MAX_MECH]; int nslab[AVSR_MAX_MECH];
  int nsrc, W;
};
struct SlabLaunch { int njob, B; SlabJob job[AVSR_MAX_MECH + 1]; };

// dst[b, k] = add[b, k] + sum_sets sum_c src[c][b][k]
__global__ void slab_sum_kernel(const SlabLaunch L) {
  const SlabJob& J = L.job[blockIdx.y];
  const long total = (long)L.B * J.W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / J.W), k = (int)(i % J.W);
    float s = J.add ? J.add[(long)b * J.add_sb + k] : 0.f;
    for (int j = 0; j < J.nsrc; ++j)
      for (int c = 0; c < J.nslab[j]; ++c) s += J.src[j][((long)c * L.B + b) * J.W + k];
    J.dst[(long)b * J.dst_sb + k] = s;
  }
}

// GreedyEmbeddingHelper.sample/next_inputs + dynamic_decode finished bookkeeping (one block).
__global__ void greedy_sample_kernel(const float* logits, long logits_sb, int V, int32_t* ids, long ids_sb, int32_t* tok,
                                     int32_t* steplen, int32_t* n_unfinished, int B, int l, int eos) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int local = 0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    int id = 0;
    if (l < steplen[b]) {
      const float* lg = logits + (long)b * logits_sb;
      float best = lg[0];
      for (int v = 1; v < V; ++v)
        if (lg[v] > best) { best = lg[v]; id = v; }   // first maximum (tf.argmax)
      tok[b] = id;
      if (id == eos) steplen[b] = l + 1; else local += 1;
    }
    ids[(long)b * ids_sb] = id;
  }
  atomicAdd(&cnt, local);
  __syncthreads();
  if (threadIdx.x == 0) n_unfinished[0] = cnt;
}

// ScheduledEmbeddingTrainingHelper.sample/next_inputs (contrib/seq2seq/python/ops/helper.py): per utterance draw
// select ~ Bernoulli(p); where selected feed the embedding of a categorical sample of this step's logits, else the
// ground-truth token.  One block per utterance; the draw is an fp32 inverse CDF in index order (oracle: categorical_f32).
__global__ void sched_sample_kernel(const float* logits, long logits_sb, int V, const int32_t* labels, int32_t* fed, float* xs,
                                    const float* emb, int B, int L, int E, int l, const int32_t* seed, float prob,
                                    float keep_in, uint32_t r_in, int in_W) {
  __shared__ int tok_s;
  extern __shared__ float lg_s[];          // this utterance's logits: fetched by all lanes together with the seed and the
  const int b = blockIdx.x;                // label, so the serial inverse-CDF below runs out of LDS (one memory round trip)
  if (l + 1 >= L) return;
  const uint32_t sd0 = (uint32_t)seed[0];
  const int label = labels[(long)b * L + l];
  {
    const float* lg = logits + (long)b * logits_sb;
    for (int v = threadIdx.x; v < V; v += blockDim.x) lg_s[v] = lg[v];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t sd = sd0;
    const uint32_t idx = (uint32_t)(b * L + l);
    int tok = label;
    if (prob > 0.f && uniform01(sd, 1000u, idx) < prob) {
      const float* lg = lg_s;
      float mx = lg[0];
      for (int v = 1; v < V; ++v) mx = fmaxf(mx, lg[v]);
      float tot = 0.f;
      for (int v = 0; v < V; ++v) tot += expf(lg[v] - mx);
      const float target = uniform01(sd, 1001u, idx) * tot;
      float run = 0.f;
      tok = V - 1;
      for (int v = 0; v < V; ++v) {
        run += expf(lg[v] - mx);
        if (run > target) { tok = v; break; }
      }
    }
    fed[(long)b * L + l + 1] = tok;
    tok_s = tok;
  }
  __syncthreads();
  const int tok = tok_s;
  const bool on = keep_in < 1.0f;
  const uint32_t sd = sd0;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float v = emb[(long)tok * E + e];
    if (on) v = uniform01(sd, r_in, (uint32_t)(((long)b * L + l + 1) * in_W + e)) < keep_in ? v / keep_in : 0.f;
    xs[((long)b * L + l + 1) * E + e] = v;
  }
}


// Output layer + ScheduledEmbeddingTrainingHelper step fused into ONE launch of the decoder's sequential chain (it replaces a
// dense step launch + sched_sample_kernel): block = utterance b.
//   logits[b, :] = x[b, :] . Wout + bout   (zero past the utterance's step length, as dynamic_decode's impute_finished)
//   then the draw of sched_sample_kernel above and the (input-dropped) embedding of the token fed to step l+1.
// Thread (vc = tid & 31, ks = tid >> 5): column v0 + vc, K slice ks of 8 (16-byte loads, Wout^T rows are K-contiguous).
__global__ __launch_bounds__(256) void logits_sample_kernel(const float* x, long x_sb, int O, const float* wout_t, const float* bout,
                                                            float* logits, long logits_sb, int V, const int32_t* steplen,
                                                            const int32_t* labels, int32_t* fed, float* xs, const float* emb, int B, int L,
                                                            int E, int l, const int32_t* seed, float prob, float keep_in, uint32_t r_in,
                                                            int in_W) {
  extern __shared__ float lg_s[];          // [V] logits of this utterance
  __shared__ float part[8][33];
  __shared__ int tok_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int vc = tid & 31, ks = tid >> 5;
  const uint32_t sd0 = seed ? (uint32_t)seed[0] : 0u;
  const int label = (l + 1 < L) ? labels[(long)b * L + l] : 0;
  const bool valid = !(steplen && l >= steplen[b]);
  const float* xr = x + (long)b * x_sb;
  const int kper = ((O + 31) / 32) * 4;    // K slice length, multiple of 4
  const int k0 = ks * kper, k1 = min(O, k0 + kper);
  for (int v0 = 0; v0 < V; v0 += 32) {
    const int v = v0 + vc;
    float a = 0.f;
    if (v < V) {
      const float* wr = wout_t + (long)v * O;
      for (int k = k0; k < k1; k += 4) {
        const f32x4 xv = ld4(xr + k), wv = ld4(wr + k);
        a += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
      }
    }
    part[ks][vc] = a;
    __syncthreads();
    if (ks == 0 && v < V) {
      float z = ((part[0][vc] + part[1][vc]) + (part[2][vc] + part[3][vc])) + ((part[4][vc] + part[5][vc]) + (part[6][vc] + part[7][vc]));
      z = valid ? z + (bout ? bout[v] : 0.f) : 0.f;
      lg_s[v] = z;
      logits[(long)b * logits_sb + v] = z;
    }
    __syncthreads();
  }
  if (l + 1 >= L) return;
  if (tid == 0) {
    const uint32_t idx = (uint32_t)(b * L + l);
    int tok = label;
    if (prob > 0.f && uniform01(sd0, 1000u, idx) < prob) {
      float mx = lg_s[0];
      for (int v = 1; v < V; ++v) mx = fmaxf(mx, lg_s[v]);
      float tot = 0.f;
      for (int v = 0; v < V; ++v) tot += expf(lg_s[v] - mx);
      const float target = uniform01(sd0, 1001u, idx) * tot;
      float run = 0.f;
      tok = V - 1;
      for (int v = 0; v < V; ++v) {
        run += expf(lg_s[v] - mx);
        if (run > target) { tok = v; break; }
      }
    }
    fed[(long)b * L + l + 1] = tok;
    tok_s = tok;
  }
  __syncthreads();
  const int tok = tok_s;
  const bool on = keep_in < 1.0f;
  for (int e = tid; e < E; e += blockDim.x) {
    float v = emb[(long)tok * E + e];
    if (on) v = uniform01(sd0, r_in, (uint32_t)(((long)b * L + l + 1) * in_W + e)) < keep_in ? v / keep_in : 0.f;
    xs[((long)b * L + l + 1) * E + e] = v;
  }
}

// output record of decoder layer j (0 = the attention-fed cell): [B][L+1][H], slot l+1 = step l
static inline float* layer_out(const avsr_attn_rnn& d, int j) { return j == 0 ? (d.n_extra > 0 ? d.out0 : d.cell_out) : d.extra[j - 1].out; }
// One decoder layer as the cell-step builders read it: j = 0 the attention-fed cell (its fields sit in avsr_attn_rnn itself), j > 0
// extra[j - 1] (MultiRNNCell above it: same buffer conventions).  kw = row length of wt / wt2, roff = where their recurrent columns
// (the recurrent rows of w / w2) begin: E + A + H and E + A for layer 0, 2H and H above.
struct DecLayer {
  const float *wt, *wt2, *w, *w2, *bias, *bias2;
  float *gates, *cs, *out, *rh_seq, *hs_seq, *xin_seq, *state, *dstate, *dgates, *dgates2;
  uint32_t cell_id;
  int kw, roff;
};
static inline DecLayer dec_layer(const avsr_attn_rnn& d, int j) {
  const int H = d.H, EA = d.E + d.n_mech * H;
  if (j == 0) return {d.wt, d.wt2, d.w, d.w2, d.bias, d.bias2, d.gates, d.cs, layer_out(d, 0), d.rh_seq, d.hs_seq, nullptr, d.state, d.dstate,
                      d.dgates, d.dgates2, (uint32_t)d.cell_id, EA + H, EA};
  const avsr_dec_layer& X = d.extra[j - 1];
  return {X.wt, X.wt2, X.w, X.w2, X.bias, X.bias2, X.gates, X.cs, X.out, X.rh_seq, X.hs_seq, X.xin_seq, X.state, X.dstate,
          X.dgates, X.dgates2, (uint32_t)X.cell_id, 2 * H, H};
}
static inline int nchunk(const avsr_attn_mech& m) { return (m.T + m.chunk - 1) / m.chunk; }
static inline bool is_bahdanau(const avsr_attn_mech& m) { return m.type >= ATT_BAHDANAU; }

static int validate(const avsr_attn_rnn* d) {
  if (!d || d->B <= 0 || d->L <= 0 || d->H <= 0 || d->H % 4 || d->E % 4 || d->n_mech < 0 || d->n_mech > AVSR_MAX_MECH)
    return AVSR_ERR_ARG;
  if (!d->wt || !d->gates || !d->cs || !d->cell_out || !d->state || !d->steplen) return AVSR_ERR_ARG;
  if (d->n_mech > 0 && !d->att) return AVSR_ERR_ARG;
  if (d->n_extra < 0 || d->n_extra > AVSR_MAX_DEC_EXTRA) return AVSR_ERR_ARG;
  if (d->n_extra > 0) {
    if (!d->out0 || d->extra[d->n_extra - 1].out != d->cell_out) return AVSR_ERR_ARG;
    for (int j = 0; j < d->n_extra; ++j) {
      const avsr_dec_layer& X = d->extra[j];
      if (!X.wt || !X.gates || !X.cs || !X.out || !X.state) return AVSR_ERR_ARG;
      if (d->cell == 1 && (!X.wt2 || !X.rh_seq)) return AVSR_ERR_ARG;  // GRU layers: candidate kernel and the r*h record
    }
  }
  for (int m = 0; m < d->n_mech; ++m) {
    const avsr_attn_mech& M = d->mech[m];
    if (M.T <= 0 || M.D % 4 || M.chunk <= 0 || M.chunk > ATTN_MAX_CHUNK || nchunk(M) > STEP_MAX_SLAB) return AVSR_ERR_ARG;
    if (M.D > 1024 || d->H > 1024) return AVSR_ERR_UNSUPPORTED;
    if (!M.keys || !M.values || !M.watt_t || !M.scores || !M.ctx || !M.pstat || !M.pctx) return AVSR_ERR_ARG;
    if (M.type < 0 || M.type > ATT_NORMED_BAHDANAU) return AVSR_ERR_UNSUPPORTED;
    if (M.type == ATT_SCALED_LUONG && !M.g) return AVSR_ERR_ARG;
    if (is_bahdanau(M) && (!M.v || !M.wq_t || !M.pq)) return AVSR_ERR_ARG;
  }
  return AVSR_OK;
}

// What avsr_attn_rnn_fwd checks of its arguments after validate(), before any launch.
static int fwd_check(const avsr_attn_rnn& d) {
  const int B = d.B, A = d.n_mech * d.H;
  if (d.mode == 1 && (!d.embedding || !d.wout_t || !d.logits || !d.ids || !d.tok || !d.n_unfinished)) return AVSR_ERR_ARG;
  if (d.mode == 2 && (!d.embedding || !d.wout_t || !d.logits || !d.xs || !d.labels || !d.fed || !d.seed)) return AVSR_ERR_ARG;
  if (d.mode == 3 && (!d.embedding || !d.wout_t || !d.logits || !d.tok || !d.n_unfinished || d.beam_width <= 0 || B % d.beam_width ||
                      !d.beam_logp || !d.beam_fin || !d.beam_len || !d.step_ids || !d.parent_ids || !d.parent_rows)) return AVSR_ERR_ARG;
  if (d.mode == 3 && (!beam_step_fits(d.beam_width, d.V) || d.beam_width > 64)) return AVSR_ERR_UNSUPPORTED;
  if (d.cell == 1 && (!d.wt2 || !d.rh_seq)) return AVSR_ERR_ARG;
  const bool drop = d.seed && d.mode != 1 && (d.keep_in < 1.f || d.keep_state < 1.f || d.keep_out < 1.f);
  if (drop && (!d.hs_seq || (A > 0 && !d.attd))) return AVSR_ERR_ARG;
  if (drop)
    for (int j = 0; j < d.n_extra; ++j)
      if (!d.extra[j].hs_seq || !d.extra[j].xin_seq) return AVSR_ERR_ARG;
  return AVSR_OK;
}

// What avsr_attn_rnn_bwd checks of its arguments after validate(), before any launch; counts the mechanisms of either family.
static int bwd_check(const avsr_attn_rnn& d, int* n_bah_out, int* n_luong_out) {
  if (!d.w || !d.dgates || !d.dstate) return AVSR_ERR_ARG;
  if (d.n_mech > 0 && !d.datt) return AVSR_ERR_ARG;
  int n_bah = 0, n_luong = 0;
  for (int m = 0; m < d.n_mech; ++m) {
    const avsr_attn_mech& M = d.mech[m];
    if (!M.watt || !M.dscores || !M.dctx || !M.pdq) return AVSR_ERR_ARG;
    if (is_bahdanau(M)) { if (!M.wq || !M.dpq) return AVSR_ERR_ARG; ++n_bah; } else ++n_luong;
  }
  if (1 + d.n_mech + n_bah > STEP_MAX_SRC) return AVSR_ERR_UNSUPPORTED;
  if (d.cell == 1 && (!d.w2 || !d.dgates2)) return AVSR_ERR_ARG;
  if (((n_luong > 0) || d.dcell_ext) && !d.dq) return AVSR_ERR_ARG;
  if (d.n_extra > 0 && (d.dh_final || d.dc_final)) return AVSR_ERR_UNSUPPORTED;     // final-state gradients: single-cell blocks only
  for (int j = 0; j < d.n_extra; ++j)
    if (!d.extra[j].w || !d.extra[j].dgates || !d.extra[j].dstate) return AVSR_ERR_ARG;
  for (int j = 0; d.cell == 1 && j < d.n_extra; ++j)
    if (!d.extra[j].w2 || !d.extra[j].dgates2) return AVSR_ERR_ARG;           // GRU layers: candidate kernel and its gradient record
  *n_bah_out = n_bah; *n_luong_out = n_luong;
  return AVSR_OK;
}

// Which blocks avsr_attn_rnn_bwd offers to the fused BPTT launch first (Luong blocks, and one-memory Bahdanau blocks).
static inline bool bwd_tries_fused(const avsr_attn_rnn& d) { return d.n_mech > 0 && d.cell != 1 && d.n_extra == 0; }

static void fill_attn_launch(const avsr_attn_rnn& d, int l, AttnLaunch& AL) {
  const int B = d.B, H = d.H, L = d.L;
  AL = AttnLaunch{};
  AL.nmech = d.n_mech; AL.B = B;
  int off = 0;
  for (int m = 0; m < d.n_mech; ++m) {
    const avsr_attn_mech& M = d.mech[m];
    AttnMechDev& X = AL.m[m];
    const int nc = nchunk(M);
    AL.blk_off[m] = off;
    off += B * nc;
    X.keys = M.keys; X.values = M.values; X.values_sb = M.values_sb; X.values_st = M.values_st; X.len = M.len;
    if (is_bahdanau(M)) { X.query = M.pq + (long)l * H; X.query_sb = (long)L * H; }
    else { X.query = d.cell_out + (long)(l + 1) * H; X.query_sb = (long)(L + 1) * H; }
    X.g = M.g; X.v = M.v; X.bq = M.bq;
    X.scores = M.scores + (long)l * M.T; X.scores_sb = (long)L * M.T;
    X.pm = M.pstat + (long)(2 * l) * nc * B; X.pl = M.pstat + (long)(2 * l + 1) * nc * B;
    X.pctx = M.pctx;
    X.T = M.T; X.D = M.D; X.H = H; X.type = M.type; X.nchunk = nc; X.chunk = M.chunk;
    X.mem_div = (d.mode == 3 && d.mem_shared && d.beam_width > 1) ? d.beam_width : 1;
    if (M.dctx) { X.dctx = M.dctx + (long)l * M.D; X.dctx_sb = (long)L * M.D; }
    X.ctx = M.ctx + (long)l * M.D; X.ctx_sb = (long)L * M.D;
    if (M.dscores) { X.dscores = M.dscores + (long)l * M.T; X.dscores_sb = (long)L * M.T; }
    X.pdq = M.pdq;
  }
  AL.blk_off[d.n_mech] = off;
}

}  // namespace avsr

// lm != NULL (mode 3 only, checked by the caller): the language-model step runs ahead of every step's selection.
// ng != NULL (likewise; never together with lm): the back-off n-gram's step takes that place (beam_ngram.hip).
// wn != NULL (likewise; never together with lm or ng): the word-level n-gram's step behind a lexicon trie (beam_word_ngram.hip).
// ctc != NULL (mode 3, weight > 0): the CTC prefix-score step runs after it, and the selection reads ctc->extra -- the two terms
// combined by that step -- as its one additive term with weight 1 (beam_ctc.hip).
static int attn_rnn_fwd_impl(const avsr_attn_rnn* dp, const avsr_beam_lm* lm, const avsr_beam_ngram* ng,
                             const avsr_beam_word_ngram* wn, const avsr_beam_ctc* ctc, int32_t l_begin, int32_t l_end, void* stream) {
  using namespace avsr;
  int rc = validate(dp);
  if (rc) return rc;
  if ((lm != nullptr) + (ng != nullptr) + (wn != nullptr) > 1) return AVSR_ERR_ARG;   // one language model per search
  // the fused model's [R][V] term and its weight, whichever model it is: what the selection reads when no CTC step pre-combines it
  const float* const fused_logp = lm ? lm->lm_logp : ng ? ng->lm_logp : wn ? wn->lm_logp : nullptr;
  const float fused_weight = lm ? lm->lm_weight : ng ? ng->lm_weight : wn ? wn->lm_weight : 0.f;
  const avsr_attn_rnn& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  const int B = d.B, H = d.H, L = d.L, E = d.E, A = d.n_mech * H;
  if (l_begin < 0 || l_end > L || l_begin > l_end) return AVSR_ERR_ARG;
  if ((rc = fwd_check(d))) return rc;
  const bool feed = (d.mode == 1 || d.mode == 3);      // inputs come from the embedding of the previous prediction
  const bool gru = d.cell == 1;
  const bool drop = d.seed && d.mode != 1 && (d.keep_in < 1.f || d.keep_state < 1.f || d.keep_out < 1.f);
  const uint32_t cid4 = (uint32_t)d.cell_id * 4;
  const size_t bh = sizeof(float) * B * H;

  if (l_begin == 0) {
    // initial state -> ping-pong parity 0, cell_out slot 0 = h0, attention slot 0 = 0: one launch (every operation reads the caller's
    // h0 / c0 or writes zeros: none reads another's result)
    avsr::DevBatch db(s);
    const size_t hrow = sizeof(float) * H, orow = sizeof(float) * (L + 1) * H;
    if (d.h0) { db.copy(st_h(d.state, B, H, 0), d.h0, bh); db.copy_2d(layer_out(d, 0), orow, d.h0, hrow, hrow, B); }
    else { db.zero(st_h(d.state, B, H, 0), bh); db.zero_2d(layer_out(d, 0), orow, hrow, B); }
    if (d.c0) db.copy(st_c(d.state, B, H, 0), d.c0, bh);
    else db.zero(st_c(d.state, B, H, 0), bh);
    for (int j = 0; j < d.n_extra; ++j) {            // layers above start from the zero state (decoder_unimodal.py:151-157)
      const avsr_dec_layer& X = d.extra[j];
      db.zero(X.state, 4 * bh);
      db.zero_2d(X.out, orow, hrow, B);
      if (drop && X.hs_seq) db.zero_2d(X.hs_seq, orow, hrow, B);
    }
    if (A > 0) db.zero_2d(d.att, sizeof(float) * (L + 1) * A, sizeof(float) * A, B);
    if (drop) {
      if (d.h0) db.copy_2d(d.hs_seq, orow, d.h0, hrow, hrow, B);
      else db.zero_2d(d.hs_seq, orow, hrow, B);
      if (A > 0) db.zero_2d(d.attd, sizeof(float) * (L + 1) * A, sizeof(float) * A, B);
    }
    if (db.flush() != hipSuccess) return AVSR_ERR_HIP;
  }

  static thread_local StepLaunch SL;
  static thread_local AttnLaunch AL;
  // the whole range as ONE persistent launch where the fused decode kernel covers the configuration (dec_persist.hip)
  int l_first = l_begin;
  {
    const int prc = avsr_dec_persist_fwd(dp, l_begin, l_end, stream);
    if (prc == AVSR_OK) l_first = l_end;
    else if (prc != AVSR_ERR_UNSUPPORTED) return prc;
  }
  // beam search: the per-step unfinished counters [L] of this call's range, zeroed once (not one fill per step)
  if (d.mode == 3 && l_first < l_end && avsr::dev_zero(d.n_unfinished + l_first, sizeof(int32_t) * (l_end - l_first), s) != hipSuccess)
    return AVSR_ERR_HIP;
  // beam search: the B * K-row cell and attention-layer steps as 64 x 64-tiled products with row-gathered operands (beam_gemm.hip)
  const bool beam_dense = d.mode == 3 && !gru && d.n_extra == 0 && !drop && beam_dense_on();
  for (int l = l_first; l < l_end; ++l) {
    // ---- K0: language-model step on the symbols and parents the previous selection left (independent of the decoder's chain) ----
    if (lm && (rc = beam_lm_step_launch(*lm, d.tok, d.parent_rows, l, s))) return rc;
    if (ng && (rc = beam_ngram_step_launch(*ng, d.tok, d.parent_rows, l, s))) return rc;
    if (wn && (rc = beam_word_ngram_step_launch(*wn, d.tok, d.parent_rows, l, s))) return rc;
    if (ctc && (rc = beam_ctc_step_launch(*ctc, d.tok, d.parent_rows, d.beam_fin + (long)(l & 1) * B, l, s))) return rc;
    // ---- K1: LSTM step -------------------------------------------------------------------
    bool cell_done = false;
    if (beam_dense) {
      const int brc = beam_cell_launch(d, l, s);
      if (brc == AVSR_OK) cell_done = true;
      else if (brc != AVSR_ERR_UNSUPPORTED) return brc;
    }
    // Layer 0 is fed the token (or the caller's xs) and the attention of the previous step; layer j > 0 (MultiRNNCell) consumes the
    // output layer j-1 emitted a moment ago.  Everything after the input sources is the same cell.  A GRU takes two launches.
    for (int j = 0; j <= d.n_extra; ++j)
     for (int phase = 0; phase < (gru ? 2 : 1) && !(j == 0 && cell_done); ++phase) {
      const DecLayer Y = dec_layer(d, j);
      const bool cand = gru && phase == 1;                   // the candidate launch, through r*h of the gate launch
      SL.ntask = 1;
      StepTask& tk = SL.task[0];
      tk = StepTask{};
      const float* wt = cand ? Y.wt2 : Y.wt;
      if (j > 0) {
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = (drop ? Y.xin_seq : layer_out(d, j - 1)) + (long)(l + 1) * H; x.sb = (long)(L + 1) * H; x.K = H; x.w = wt; x.ldw = Y.kw;
        x.kind = SRC_OWNROW;
      } else if (feed) {
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = d.embedding; x.sb = E; x.K = E; x.w = wt; x.ldw = Y.kw; x.kind = SRC_PLAIN;
        tk.gather = d.tok;
      } else if (d.mode == 2) {
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = d.xs + (long)l * E; x.sb = (long)L * E; x.K = E; x.w = wt; x.ldw = Y.kw; x.kind = SRC_PLAIN;
      }
      if (j == 0 && A > 0) {
        StepSrc& a = tk.src[tk.nsrc++];
        a.a = (drop ? d.attd : d.att) + (long)l * A; a.sb = (long)(L + 1) * A; a.K = A; a.w = wt + E; a.ldw = Y.kw; a.kind = SRC_PLAIN;
      }
      StepSrc& h = tk.src[tk.nsrc++];
      h.a = cand ? st_rh(Y.state, B, H) : st_h(Y.state, B, H, l & 1); h.sb = H; h.K = H; h.w = wt + Y.roff; h.ldw = Y.kw;
      // r*h was written by the gate phase of THIS step into this hypothesis' own row: under beam search only the previous state
      // (h, and the attention fed back) lives in the parent's row
      h.kind = cand ? SRC_OWNROW : SRC_PLAIN;
      if (d.mode == 3) tk.gather2 = d.parent_rows;
      tk.B = B; tk.t = l; tk.T = L; tk.reverse = 0; tk.len = d.steplen;
      tk.s2 = (j == 0 && d.mode == 0) ? 1 : 0;               // mode 0: the caller hoisted x . Wx into layer 0's `gates`
      tk.p4 = st_h(Y.state, B, H, l & 1);
      if (gru && !cand) {
        tk.N = 2 * H; tk.mode = EP_GRU_GATES; tk.bias = Y.bias;
        tk.p0 = Y.gates; tk.p1 = st_rh(Y.state, B, H); tk.p2 = Y.rh_seq;
      } else {
        if (gru) { tk.N = H; tk.mode = EP_GRU_CAND; tk.bias = Y.bias2; tk.p0 = Y.cs; tk.p1 = Y.gates; }
        else { tk.N = 4 * H; tk.mode = EP_LSTM_FWD; tk.bias = Y.bias; tk.p0 = Y.gates; tk.p1 = Y.cs;
               tk.p3 = st_c(Y.state, B, H, l & 1); tk.p5 = st_c(Y.state, B, H, (l + 1) & 1); }
        tk.p2 = Y.out + H; tk.s0 = (long)(L + 1) * H; tk.s1 = H;
        tk.p6 = st_h(Y.state, B, H, (l + 1) & 1);
        if (drop) {
          tk.seed = d.seed; tk.k_st = d.keep_state; tk.k_out = d.keep_out; tk.k_in = 1.0f;
          tk.r_st = Y.cell_id * 4 + 1; tk.r_out = Y.cell_id * 4 + 2;
          tk.p9 = Y.hs_seq + H; tk.s4 = (long)(L + 1) * H; tk.s5 = H;
          if (j < d.n_extra) {   // what the layer above consumes: this output under that layer's input mask
            tk.p11 = d.extra[j].xin_seq + H; tk.k_in = d.keep_in; tk.r_in = (uint32_t)d.extra[j].cell_id * 4; tk.in_W = H; tk.in_coff = 0;
          }
        }
      }
      if ((rc = avsr_step_launch_raw(&SL, stream))) return rc;
    }

    if (d.n_mech > 0) {
      // ---- Kq: Bahdanau processed query  pq = cell_out . Wq ---------------------------------
      SL.ntask = 0;
      for (int m = 0; m < d.n_mech; ++m) {
        const avsr_attn_mech& M = d.mech[m];
        if (!is_bahdanau(M)) continue;
        StepTask& tk = SL.task[SL.ntask++];
        tk = StepTask{};
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = d.cell_out + (long)(l + 1) * H; x.sb = (long)(L + 1) * H; x.K = H; x.w = M.wq_t; x.ldw = H; x.kind = SRC_PLAIN;
        tk.B = B; tk.N = H; tk.mode = EP_LINEAR; tk.t = l; tk.T = L;
        tk.p0 = M.pq + (long)l * H; tk.s0 = (long)L * H;
      }
      if (SL.ntask && (rc = avsr_step_launch_raw(&SL, stream))) return rc;

      // ---- K2: attention partials ---------------------------------------------------------
      fill_attn_launch(d, l, AL);
      if ((rc = avsr_attn_launch_raw(&AL, 0, stream))) return rc;

      // ---- K3: attention layer  att_m = [cell_out, ctx_m] . W_att,m --------------------------
      bool layer_done = false;
      if (beam_dense) {
        const int brc = beam_attention_layer_launch(d, l, s);
        if (brc == AVSR_OK) layer_done = true;
        else if (brc != AVSR_ERR_UNSUPPORTED) return brc;
      }
      SL.ntask = 0;
      for (int m = 0; m < d.n_mech && !layer_done; ++m) {
        const avsr_attn_mech& M = d.mech[m];
        const int nc = nchunk(M);
        StepTask& tk = SL.task[SL.ntask++];
        tk = StepTask{};
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = d.cell_out + (long)(l + 1) * H; x.sb = (long)(L + 1) * H; x.K = H; x.w = M.watt_t; x.ldw = H + M.D; x.kind = SRC_PLAIN;
        StepSrc& c = tk.src[tk.nsrc++];
        c.a = M.pctx; c.sb = M.D; c.K = M.D; c.w = M.watt_t + H; c.ldw = H + M.D; c.kind = SRC_SOFTMAX;
        tk.pm = M.pstat + (long)(2 * l) * nc * B; tk.pl = M.pstat + (long)(2 * l + 1) * nc * B;
        tk.nslab = nc; tk.slab_stride = (long)B * M.D;
        tk.ctx_save = M.ctx + (long)l * M.D; tk.ctx_sb = (long)L * M.D;
        tk.B = B; tk.N = H; tk.mode = EP_LINEAR; tk.t = l; tk.T = L; tk.len = d.steplen;
        tk.p0 = d.att + (long)(l + 1) * A + (long)m * H; tk.s0 = (long)(L + 1) * A;
        if (drop) {   // pre-dropped copy = the attention half of step l+1's cell input (mask index of time l+1)
          tk.seed = d.seed; tk.k_in = d.keep_in; tk.r_in = cid4; tk.in_W = E + A; tk.in_coff = (E + A) + E + m * H;
          tk.p9 = d.attd + (long)(l + 1) * A + (long)m * H; tk.s4 = (long)(L + 1) * A;
        }
      }
      if (!layer_done && (rc = avsr_step_launch_raw(&SL, stream))) return rc;
    }

    if (d.mode >= 1) {
      // ---- K4/K5: output layer + greedy / scheduled sample / beam step ------------------------
      const bool oa = d.output_attention && A > 0;
      const int O = oa ? A : H;
      const float* xa = oa ? d.att + (long)(l + 1) * A : d.cell_out + (long)(l + 1) * H;
      const long xsb = oa ? (long)(L + 1) * A : (long)(L + 1) * H;
      const bool fused_sample = d.mode == 2 && O % 4 == 0 && d.V <= 8192;
      if (fused_sample) {
        hipLaunchKernelGGL(logits_sample_kernel, dim3(B), dim3(256), sizeof(float) * d.V, s, xa, xsb, O, d.wout_t, d.bout,
                           d.logits + (long)l * d.V, (long)L * d.V, d.V, d.steplen, d.labels, d.fed, d.xs, d.embedding, B, L, E, l, d.seed,
                           d.sampling_prob, drop ? d.keep_in : 1.0f, cid4, E + A);
        AVSR_CHECK_LAUNCH();
        continue;
      }
      // beam search: the selection step (beam.h); on the dense path the output layer runs inside it where beam_step_nct allows
      BeamStep bs{};
      bool bs_inside = false;
      if (d.mode == 3) {
        const long pin = (long)(l & 1) * B, pout = (long)((l + 1) & 1) * B;       // halves of the ping-pong beam state
        bs = BeamStep{d.logits + (long)l * d.V, (long)L * d.V, B / d.beam_width, d.beam_width, d.V, l, d.eos_id, d.length_penalty,
                      d.beam_logp + pin, d.beam_fin + pin, d.beam_len + pin, d.beam_logp + pout, d.beam_fin + pout, d.beam_len + pout,
                      d.tok, d.parent_rows, d.step_ids, d.parent_ids, d.n_unfinished, xa, xsb, O, d.wout_t, d.bout,
                      ctc ? ctc->extra : fused_logp, ctc ? 1.f : fused_weight};
        bs_inside = beam_dense && beam_step_nct(bs) != 0;
      }
      if (!bs_inside) {
        SL.ntask = 1;
        StepTask& tk = SL.task[0];
        tk = StepTask{};
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = xa; x.sb = xsb;
        x.K = O; x.w = d.wout_t; x.ldw = O; x.kind = SRC_PLAIN;
        tk.B = B; tk.N = d.V; tk.mode = EP_LINEAR; tk.t = l; tk.T = L; tk.len = (d.mode == 3) ? nullptr : d.steplen; tk.bias = d.bout;
        tk.p0 = d.logits + (long)l * d.V; tk.s0 = (long)L * d.V;
        if ((rc = avsr_step_launch_raw(&SL, stream))) return rc;
      }
      if (d.mode == 1) {
        hipLaunchKernelGGL(greedy_sample_kernel, dim3(1), dim3(256), 0, s, d.logits + (long)l * d.V, (long)L * d.V, d.V,
                           d.ids + l, (long)L, d.tok, d.steplen, d.n_unfinished, B, l, d.eos_id);
      } else if (d.mode == 3) {
        if ((rc = beam_step_launch(bs, bs_inside, s))) return rc;
      } else {
        hipLaunchKernelGGL(sched_sample_kernel, dim3(B), dim3(128), sizeof(float) * d.V, s, d.logits + (long)l * d.V, (long)L * d.V, d.V, d.labels,
                           d.fed, d.xs, d.embedding, B, L, E, l, d.seed, d.sampling_prob, drop ? d.keep_in : 1.0f, cid4, E + A);
      }
      AVSR_CHECK_LAUNCH();
    }
  }
  if (l_end == L) {
    avsr::DevBatch db(s);
    if (d.h_final) db.copy(d.h_final, st_h(d.state, B, H, L & 1), bh);
    if (!gru && d.c_final) db.copy(d.c_final, st_c(d.state, B, H, L & 1), bh);
    if (db.flush() != hipSuccess) return AVSR_ERR_HIP;
  }
  return AVSR_OK;
}

extern "C" int avsr_attn_rnn_fwd(const avsr_attn_rnn* dp, int32_t l_begin, int32_t l_end, void* stream) {
  return attn_rnn_fwd_impl(dp, nullptr, nullptr, nullptr, nullptr, l_begin, l_end, stream);
}

extern "C" int avsr_attn_rnn_fwd_lm(const avsr_attn_rnn* dp, const avsr_beam_lm* lm, int32_t l_begin, int32_t l_end, void* stream) {
  if (!dp || !lm) return AVSR_ERR_ARG;
  if (dp->mode != 3) return AVSR_ERR_ARG;                      // fusion is defined on the beam
  const int rc = avsr::beam_lm_check(lm);
  if (rc) return rc;
  if (lm->V != dp->V || lm->n_rows != dp->B) return AVSR_ERR_ARG;
  return attn_rnn_fwd_impl(dp, lm, nullptr, nullptr, nullptr, l_begin, l_end, stream);
}

extern "C" int avsr_attn_rnn_fwd_ctc(const avsr_attn_rnn* dp, const avsr_beam_lm* lm, const avsr_beam_ctc* ctc, int32_t l_begin,
                                     int32_t l_end, void* stream) {
  if (!dp || !ctc) return AVSR_ERR_ARG;
  if (dp->mode != 3) return AVSR_ERR_ARG;                      // joint scoring is defined on the beam
  int rc = avsr::beam_ctc_check(ctc);
  if (rc) return rc;
  if (ctc->V != dp->V || (long)ctc->n_utt * ctc->beam_width != dp->B || ctc->beam_width != dp->beam_width || ctc->eos_id != dp->eos_id)
    return AVSR_ERR_ARG;
  if (lm) {
    if ((rc = avsr::beam_lm_check(lm))) return rc;
    if (lm->V != dp->V || lm->n_rows != dp->B || ctc->lm_logp != lm->lm_logp) return AVSR_ERR_ARG;
  } else if (ctc->lm_logp) {
    return AVSR_ERR_ARG;
  }
  return attn_rnn_fwd_impl(dp, lm, nullptr, nullptr, ctc->weight == 0.f ? nullptr : ctc, l_begin, l_end, stream);
}

extern "C" int avsr_attn_rnn_fwd_ngram(const avsr_attn_rnn* dp, const avsr_beam_ngram* ng, const avsr_beam_ctc* ctc, int32_t l_begin,
                                       int32_t l_end, void* stream) {
  if (!dp || !ng) return AVSR_ERR_ARG;
  if (dp->mode != 3) return AVSR_ERR_ARG;                      // fusion is defined on the beam
  int rc = avsr::beam_ngram_check(ng);
  if (rc) return rc;
  if (ng->V != dp->V || ng->n_rows != dp->B) return AVSR_ERR_ARG;
  if (ctc) {
    if ((rc = avsr::beam_ctc_check(ctc))) return rc;
    if (ctc->V != dp->V || (long)ctc->n_utt * ctc->beam_width != dp->B || ctc->beam_width != dp->beam_width || ctc->eos_id != dp->eos_id ||
        ctc->lm_logp != ng->lm_logp)
      return AVSR_ERR_ARG;
  }
  return attn_rnn_fwd_impl(dp, nullptr, ng, nullptr, ctc && ctc->weight != 0.f ? ctc : nullptr, l_begin, l_end, stream);
}

extern "C" int avsr_attn_rnn_fwd_word_ngram(const avsr_attn_rnn* dp, const avsr_beam_word_ngram* wn, const avsr_beam_ctc* ctc,
                                            int32_t l_begin, int32_t l_end, void* stream) {
  if (!dp || !wn) return AVSR_ERR_ARG;
  if (dp->mode != 3) return AVSR_ERR_ARG;                      // fusion is defined on the beam
  int rc = avsr::beam_word_ngram_check(wn);
  if (rc) return rc;
  if (wn->V != dp->V || wn->n_rows != dp->B) return AVSR_ERR_ARG;
  if (ctc) {
    if ((rc = avsr::beam_ctc_check(ctc))) return rc;
    if (ctc->V != dp->V || (long)ctc->n_utt * ctc->beam_width != dp->B || ctc->beam_width != dp->beam_width || ctc->eos_id != dp->eos_id ||
        ctc->lm_logp != wn->lm_logp)
      return AVSR_ERR_ARG;
  }
  return attn_rnn_fwd_impl(dp, nullptr, nullptr, wn, ctc && ctc->weight != 0.f ? ctc : nullptr, l_begin, l_end, stream);
}

extern "C" int avsr_attn_rnn_bwd(const avsr_attn_rnn* dp, void* stream) {
  using namespace avsr;
  int rc = validate(dp);
  if (rc) return rc;
  const avsr_attn_rnn& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  const int B = d.B, H = d.H, L = d.L, E = d.E, A = d.n_mech * H;
  int n_bah = 0, n_luong = 0;
  if ((rc = bwd_check(d, &n_bah, &n_luong))) return rc;
  const bool drop = d.seed && (d.keep_in < 1.f || d.keep_state < 1.f || d.keep_out < 1.f);
  const uint32_t cid4 = (uint32_t)d.cell_id * 4;
  const bool gru = d.cell == 1;
  const int G = gru ? 2 : 4;      // gate pre-activations per unit
  const bool use_dq = (n_luong > 0) || d.dcell_ext;
  const size_t bh = sizeof(float) * B * H;
  const int NX = d.n_extra;
  {
    avsr::DevBatch db(s);                            // the zeroed rolling state of every layer: one launch
    for (int j = 0; j < NX; ++j) db.zero(d.extra[j].dstate, 12 * bh);
    db.zero(d.dstate, 12 * bh);
    if (db.flush() != hipSuccess) return AVSR_ERR_HIP;
    // ... then the final-state gradients into their slots of it (a second launch: they overwrite part of what the first zeroes)
    if (!gru && d.dc_final) db.copy(ds_dc(d.dstate, B, H, L & 1), d.dc_final, bh);
    if (d.dh_final) db.copy(gru ? dg_carry(d.dstate, B, H, L & 1) : ds_dh(d.dstate, B, H, L & 1), d.dh_final, bh);
    if (db.flush() != hipSuccess) return AVSR_ERR_HIP;
  }

  static thread_local StepLaunch SL;
  static thread_local AttnLaunch AL;
  static thread_local SlabLaunch BL;
  // the whole loop as one persistent launch where the fused kernel covers the block (csrc/dec_persist_bwd.hip)
  bool fused = false;
  if (bwd_tries_fused(d)) {
    const int frc = avsr_dec_persist_bwd(dp, stream);
    if (frc == AVSR_OK) fused = true;
    else if (frc != AVSR_ERR_UNSUPPORTED) return frc;
  }
  for (int l = fused ? -1 : L - 1; l >= 0; --l) {
    if (A > 0) {
      // ---- KB3: d attention_l = datt_ext[l] + dG_{l+1} . Wx_att^T ----------------------------
      SL.ntask = 1;
      {
        StepTask& tk = SL.task[0];
        tk = StepTask{};
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = gru ? dg_dgg(d.dstate, B, H, (l + 1) & 1) : ds_dg(d.dstate, B, H, (l + 1) & 1); x.sb = G * H; x.K = G * H; x.w = d.w + (long)E * G * H; x.ldw = G * H; x.kind = SRC_PLAIN;
        if (gru) {
          StepSrc& x2 = tk.src[tk.nsrc++];
          x2.a = dg_dpc(d.dstate, B, H, (l + 1) & 1); x2.sb = H; x2.K = H; x2.w = d.w2 + (long)E * H; x2.ldw = H; x2.kind = SRC_PLAIN;
        }
        tk.B = B; tk.N = A; tk.mode = EP_LINEAR; tk.t = l; tk.T = L;
        if (d.datt_ext) { tk.p1 = const_cast<float*>(d.datt_ext) + (long)l * A; tk.s1 = (long)L * A; }
        tk.p0 = d.datt + (long)l * A; tk.s0 = (long)L * A;
        if (drop) {   // the product is the gradient of step l+1's DROPPED attention input
          tk.act = 8; tk.seed = d.seed; tk.k_in = d.keep_in; tk.r_in = cid4; tk.in_W = E + A; tk.in_coff = (E + A) + E;
        }
      }
      if ((rc = avsr_step_launch_raw(&SL, stream))) return rc;
      // ---- KB4: d ctx_m = d att_m . W_att,m[H:, :]^T ----------------------------------------
      SL.ntask = 0;
      for (int m = 0; m < d.n_mech; ++m) {
        const avsr_attn_mech& M = d.mech[m];
        StepTask& tk = SL.task[SL.ntask++];
        tk = StepTask{};
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = d.datt + (long)l * A + (long)m * H; x.sb = (long)L * A; x.K = H; x.w = M.watt + (long)H * H; x.ldw = H; x.kind = SRC_PLAIN;
        tk.B = B; tk.N = M.D; tk.mode = EP_LINEAR; tk.t = l; tk.T = L;
        tk.p0 = M.dctx + (long)l * M.D; tk.s0 = (long)L * M.D;
      }
      if ((rc = avsr_step_launch_raw(&SL, stream))) return rc;
      // ---- KB5: attention backward -----------------------------------------------------------
      fill_attn_launch(d, l, AL);
      if ((rc = avsr_attn_launch_raw(&AL, 1, stream))) return rc;
    }
    // ---- KB5b: reduce the per-chunk query gradients --------------------------------------------
    BL = SlabLaunch{};
    BL.B = B;
    // LSTM with only Luong mechanisms (<= 2): the cell-backward epilogue sums the partials itself (no launch here)
    const bool fold_dq = use_dq && !gru && n_bah == 0 && n_luong <= 2;
    if (use_dq && !fold_dq) {
      SlabJob& J = BL.job[BL.njob++];
      J.dst = d.dq + (long)l * H; J.dst_sb = (long)L * H; J.W = H;
      if (d.dcell_ext) { J.add = d.dcell_ext + (long)l * H; J.add_sb = (long)L * H; }
      for (int m = 0; m < d.n_mech; ++m)
        if (!is_bahdanau(d.mech[m])) { J.src[J.nsrc] = d.mech[m].pdq; J.nslab[J.nsrc] = nchunk(d.mech[m]); ++J.nsrc; }
    }
    for (int m = 0; m < d.n_mech; ++m) {
      const avsr_attn_mech& M = d.mech[m];
      if (!is_bahdanau(M)) continue;
      SlabJob& J = BL.job[BL.njob++];
      J.dst = M.dpq + (long)l * H; J.dst_sb = (long)L * H; J.W = H;
      J.src[0] = M.pdq; J.nslab[0] = nchunk(M); J.nsrc = 1;
    }
    if (BL.njob) {
      int gx = (B * H + 255) / 256;
      if (gx > 64) gx = 64;
      hipLaunchKernelGGL(slab_sum_kernel, dim3(gx, BL.njob), dim3(256), 0, s, BL);
      AVSR_CHECK_LAUNCH();
    }
    // ---- KB2: LSTM backward, top layer first.  The TOP layer's emitted output is what the attention mechanisms and the
    // attention layers consumed; every layer below receives d(output) from the layer above of the SAME step (through that
    // layer's input mask) next to its own recurrent path.
    for (int j = NX; j >= 0; --j) {
      SL.ntask = 1;
      StepTask& tk = SL.task[0];
      tk = StepTask{};
      const bool top = (j == NX);
      const DecLayer Y = dec_layer(d, j);
      float* const ds = Y.dstate;
      const int p = l & 1, q = (l + 1) & 1;
      StepSrc& a = tk.src[tk.nsrc++];          // the layer's own dG(l+1) through the recurrent rows of its kernel
      a.a = gru ? dg_dgg(ds, B, H, q) : ds_dg(ds, B, H, q); a.sb = G * H; a.K = G * H; a.w = Y.w + (long)Y.roff * G * H; a.ldw = G * H;
      a.kind = SRC_PLAIN;
      if (top) {
        for (int m = 0; m < d.n_mech; ++m) {
          const avsr_attn_mech& M = d.mech[m];
          StepSrc& x = tk.src[tk.nsrc++];
          x.a = d.datt + (long)l * A + (long)m * H; x.sb = (long)L * A; x.K = H; x.w = M.watt; x.ldw = H; x.kind = SRC_PLAIN;
          if (is_bahdanau(M)) {
            StepSrc& y = tk.src[tk.nsrc++];
            y.a = M.dpq + (long)l * H; y.sb = (long)L * H; y.K = H; y.w = M.wq; y.ldw = H; y.kind = SRC_PLAIN;
          }
        }
      } else {   // d(output of layer j) = dG_{j+1}(l) . Wx_{j+1}^T: the layer above ran a moment ago (a GRU: its gate and its candidate kernel)
        const DecLayer U = dec_layer(d, j + 1);
        StepSrc& x = tk.src[tk.nsrc++];
        x.a = gru ? dg_dgg(U.dstate, B, H, p) : ds_dg(U.dstate, B, H, p); x.sb = G * H; x.K = G * H; x.w = U.w; x.ldw = G * H; x.kind = SRC_PLAIN;
        if (gru) {
          StepSrc& x2 = tk.src[tk.nsrc++];
          x2.a = dg_dpc(U.dstate, B, H, p); x2.sb = H; x2.K = H; x2.w = U.w2; x2.ldw = H; x2.kind = SRC_PLAIN;
        }
      }
      tk.B = B; tk.N = H; tk.t = l; tk.T = L; tk.reverse = 0; tk.len = d.steplen;
      tk.p0 = Y.gates; tk.p1 = Y.cs;
      float* const hrec = drop ? Y.hs_seq : Y.out;           // slot l = h consumed by step l (GRU)
      if (gru) {
        tk.mode = EP_GRU_BWD_CAND;
        tk.p2 = hrec; tk.s2 = (long)(L + 1) * H; tk.s3 = H;
        tk.p4 = dg_carry(ds, B, H, q); tk.p5 = dg_dpc(ds, B, H, p); tk.p3 = Y.dgates2; tk.p6 = dg_tmp(ds, B, H, 0); tk.p7 = dg_tmp(ds, B, H, 1);
      } else {
        tk.mode = EP_LSTM_BWD;
        if (j == 0) tk.bias = d.c0;                  // c_init; the layers above start from 0: bias stays NULL
        tk.p2 = Y.dgates; tk.p3 = ds_dg(ds, B, H, p);
        tk.p4 = ds_dc(ds, B, H, q); tk.p5 = ds_dc(ds, B, H, p);
        tk.p6 = ds_dh(ds, B, H, q); tk.p7 = ds_dh(ds, B, H, p);
      }
      if (top) {
        if (fold_dq) {
          if (d.dcell_ext) { tk.p8 = const_cast<float*>(d.dcell_ext); tk.s0 = (long)L * H; tk.s1 = H; }
          int k = 0;
          for (int m = 0; m < d.n_mech; ++m) {
            if (is_bahdanau(d.mech[m])) continue;
            if (k == 0) { tk.pm = d.mech[m].pdq; tk.nslab = nchunk(d.mech[m]); }
            else { tk.pl = d.mech[m].pdq; tk.pad0 = nchunk(d.mech[m]); }
            ++k;
          }
        } else if (use_dq) { tk.p8 = d.dq; tk.s0 = (long)L * H; tk.s1 = H; }
      }
      if (drop) {
        tk.seed = d.seed; tk.k_st = d.keep_state; tk.k_out = d.keep_out; tk.k_in = 1.0f;
        tk.r_st = Y.cell_id * 4 + 1; tk.r_out = Y.cell_id * 4 + 2;
        if (!top) { tk.k_in = d.keep_in; tk.r_in = (uint32_t)d.extra[j].cell_id * 4; tk.in_W = H; tk.in_coff = 0; }
      }
      if ((rc = avsr_step_launch_raw(&SL, stream))) return rc;
      if (gru) {   // second phase of THIS layer: through r*h and the gate pre-activations (the layer below reads both results)
        SL.ntask = 1;
        StepTask& tg = SL.task[0];
        tg = StepTask{};
        StepSrc& ag = tg.src[tg.nsrc++];
        tg.B = B; tg.N = H; tg.mode = EP_GRU_BWD_GATES; tg.t = l; tg.T = L; tg.reverse = 0; tg.len = d.steplen;
        tg.s2 = (long)(L + 1) * H; tg.s3 = H;
        ag.a = dg_dpc(ds, B, H, p); ag.sb = H; ag.K = H; ag.w = Y.w2 + (long)Y.roff * H; ag.ldw = H; ag.kind = SRC_PLAIN;
        tg.p0 = Y.gates; tg.p2 = hrec;
        tg.p6 = dg_tmp(ds, B, H, 0); tg.p7 = dg_tmp(ds, B, H, 1); tg.p5 = dg_carry(ds, B, H, p); tg.p3 = Y.dgates; tg.p1 = dg_dgg(ds, B, H, p);
        if ((rc = avsr_step_launch_raw(&SL, stream))) return rc;
      }
    }
  }
  // gradient wrt the initial state
  if (d.dh0) {
    SL.ntask = 1;
    StepTask& tk = SL.task[0];
    tk = StepTask{};
    StepSrc& a = tk.src[tk.nsrc++];
    a.a = gru ? dg_dgg(d.dstate, B, H, 0) : ds_dg(d.dstate, B, H, 0); a.sb = G * H; a.K = G * H; a.w = d.w + (long)(E + A) * G * H; a.ldw = G * H; a.kind = SRC_PLAIN;
    tk.B = B; tk.N = H; tk.mode = EP_LINEAR; tk.t = 0; tk.T = L;
    tk.p1 = gru ? dg_carry(d.dstate, B, H, 0) : ds_dh(d.dstate, B, H, 0); tk.s1 = H;
    tk.p0 = d.dh0; tk.s0 = H;
    if ((rc = avsr_step_launch_raw(&SL, stream))) return rc;
  }
  if (!gru && d.dc0 && avsr::dev_copy(d.dc0, ds_dc(d.dstate, B, H, 0), bh, s) != hipSuccess) return AVSR_ERR_HIP;
  return AVSR_OK;
}

// The dry path of the two calls above: their argument checks, then the question they put to the fused launches first.
extern "C" int avsr_attn_rnn_plan(const avsr_attn_rnn* dp, int32_t bwd, avsr_attn_rnn_launch* out) {
  using namespace avsr;
  int rc = validate(dp);
  if (rc) return rc;
  if (!out || bwd < 0 || bwd > 1) return AVSR_ERR_ARG;
  const avsr_attn_rnn& d = *dp;
  int prc = AVSR_ERR_UNSUPPORTED;
  if (!bwd) {
    if ((rc = fwd_check(d))) return rc;
    prc = avsr_dec_persist_fwd_plan(dp, out);
  } else {
    int n_bah = 0, n_luong = 0;
    if ((rc = bwd_check(d, &n_bah, &n_luong))) return rc;
    if (bwd_tries_fused(d)) prc = avsr_dec_persist_bwd_plan(dp, out);
  }
  if (prc == AVSR_OK) return AVSR_OK;
  if (prc != AVSR_ERR_UNSUPPORTED) return prc;
  *out = avsr_attn_rnn_launch{};
  out->form = AVSR_ATTN_FORM_PER_STEP; out->variant = -1; out->launches = d.L;
  return AVSR_OK;
}

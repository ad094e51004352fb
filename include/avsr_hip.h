/* avsr_hip.h -- C ABI of libavsr_hip.so, the MI355X (gfx950) engine for the AVSR seq2seq hot path.
 *
 * The reference (georgesterpu/avsr-tf1) has no FFI / plugin interface: every op of the hot path is a
 * TensorFlow-1.13 graph node built from Python.  This header therefore draws the boundary at the
 * granularity of the TensorFlow sequence primitives the reference calls, one entry point per
 * primitive, cited below.  Host code (the avsr_tf1_amd package) stays Python and binds these with ctypes
 * (see INTEGRATION.md); PyTorch tensors are only the container for device memory.
 *
 * Conventions: plain pointers and sizes; all pointers are DEVICE pointers unless stated; fp32
 * row-major, batch-major [B, T, F]; lengths int32; `stream` is a hipStream_t passed as void*.
 * Every function returns 0 on success or a negative AVSR_ERR_* code; nothing throws or aborts, no
 * function allocates or synchronises (all are hipGraph-capturable).
 *
 * Internal weight layout ("engine layout", produced by avsr_tf1_amd/params.py from TF layout):
 *   LSTM kernel  W  [in+H][H][4]   = TF kernel [in+H][4H] with column (g*H + u) moved to (u*4 + g),
 *                                    gate order i, j, f, o kept (rnn_cell_impl.LSTMCell)
 *   LSTM kernel  Wt [H*4][in+H]    = transpose of W (forward operand)
 *   dense kernels: TF [in][out] ("w") and transposed [out][in] ("wt")
 */
#ifndef AVSR_HIP_H
#define AVSR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libavsr_hip.so is built with -fvisibility=hidden: exactly the functions declared in this header are exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define AVSR_OK 0
#define AVSR_ERR_ARG (-1)
#define AVSR_ERR_HIP (-2)
#define AVSR_ERR_UNSUPPORTED (-3)

#define AVSR_MAX_LAYERS 4
#define AVSR_MAX_MECH 4
#define AVSR_MAX_STACKS 4
#define AVSR_HAVE_ATTN 1
#define AVSR_MAX_TRANSPOSE 16
#define AVSR_MAX_SEGMENTS 32

int avsr_abi_version(void);
/* sizeof() of a struct of this header by name ("avsr_attn_rnn", ...), -1 if unknown: lets an FFI binding verify its
 * struct layouts against the library before the first launch (avsr_tf1_amd/_lib.py does). */
int64_t avsr_sizeof(const char* name);

/* ---------------------------------------------------------------------------------------------
 * Dense GEMM (fp32 MFMA).  Replaces tf.matmul / tf.layers.Dense over all B*T rows: hoisted
 * LSTMCell input projections (avsr/cells.py:14-18 via avsr/encoder.py:80,:110), attention
 * memory_layer (avsr/attention.py:26-72), output Dense (avsr/decoder_unimodal.py:112), and the
 * matching tf.gradients GEMMs (avsr/seq2seq.py:222).
 *   C = alpha * op(A) * op(B) + beta * C + bias
 * Row r of a stored matrix lives at ptr + (T ? (r / T) * ldo + (r % T) * ld : r * ld).
 * trans_a: A stored [K][M];  trans_b: B stored [N][K].
 * splitk > 1 needs workspace of batch*splitk*M*N floats (deterministic two-pass reduction). */
typedef struct avsr_mat {
  float* ptr;
  int64_t ld;
  int32_t T;
  int32_t pad_;
  int64_t ldo;
} avsr_mat;

typedef struct avsr_gemm_desc {
  avsr_mat A, B, C;
  const float* bias;
  int32_t M, N, K;
  int32_t trans_a, trans_b;
  float alpha, beta;
  int32_t batch;
  int64_t stride_a, stride_b, stride_c;
  const float* alpha_dev;       /* optional device scalar multiplied into alpha (learned attention scale g) */
  int32_t splitk;
  int32_t pad_;
  float* workspace;
  int64_t workspace_floats;
  /* optional: colsum[n] = colsum_beta * colsum[n] + sum_k op(B)[k][n], taken from the B tiles while they pass through the kernel (the bias
   * gradient of a layer whose weight gradient this GEMM is: seq2seq.py:222 -- the same d gates, one pass less over them).  trans_b == 0
   * and batch == 1 only; with split-K the workspace must hold splitk * N more floats. */
  float* colsum;
  float colsum_beta;
  int32_t pad2_;
} avsr_gemm_desc;

int avsr_gemm(const avsr_gemm_desc* d, void* stream);
/* n INDEPENDENT GEMMs (no output of one is an operand or the output of another; split-K workspaces disjoint) issued side by side:
 * entries of one operand-layout class share a launch (and one split-K reduction launch) -- the many few-workgroup matmuls of a train
 * step (state bridges decoder_bimodal.py:480-490, per-memory attention gradients, the row blocks of a cell kernel's gradient,
 * seq2seq.py:222) cost one dependent launch each when issued one by one.  Same per-entry semantics as avsr_gemm; n <= 64. */
int avsr_gemm_batch(const avsr_gemm_desc* descs, int32_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-layer masked RNN over a sequence.  Replaces tf.nn.dynamic_rnn(MultiRNNCell(LSTMCell...),
 * sequence_length=...) and each direction of tf.nn.bidirectional_dynamic_rnn
 * (avsr/encoder.py:80-88, :110-119; cells from avsr/cells.py:61-102).  Several independent stacks
 * (video/audio, forward/backward direction) advance in ONE launch per wavefront step.
 *
 * Semantics (tf rnn.py _rnn_step): for t >= len[b] the output row is zero and the state is copied
 * through; reverse=1 processes utterance b in the order len[b]-1 .. 0 (array_ops.reverse_sequence)
 * and stores results at their original time positions.
 *
 * Buffers per layer (caller-allocated):
 *   gates  [B][T][H][4]  forward: activated gates i,j,f,o.  If hoisted=1 it must hold x*Wx(+0 bias)
 *                        on entry (bias is added by the kernel).
 *   cs     [B][T][H]     cell states (post clip)
 *   out    [B][T+2][ld_out] (+out_col)  slot s = time s-1; caller keeps slot 0 and slots > len zero.
 *   state  scratch 4*B*H floats (h and c ping-pong; the layout of state / dstate: csrc/cell_state.h)
 *   dgates [B][T][H][4]  backward: d(pre-activation)
 *   dstate scratch (2*4 + 2 + 2)*B*H floats
 *   dout   gradient wrt out (same slot layout/stride as out), top layer only (others NULL)
 */
typedef struct avsr_rnn_layer {
  int32_t units, in_dim, hoisted, out_col;
  const float* wt;
  const float* w;
  const float* bias;
  float* gates;
  float* cs;
  float* out;
  int64_t ld_out;
  float* state;
  float* h_final;
  float* c_final;
  float* dgates;
  float* dstate;
  const float* dout;
  int64_t ld_dout;
  int32_t dout_col;
  int32_t residual;             /* ResidualWrapper around this layer's cell (cells.py:91-92; layers > 0, LSTM or GRU, units == in_dim):
                                 * emitted output = cell output + layer input.  Runs through the per-step launches; `state`
                                 * must hold 6*B*units and `dstate` 14*B*units floats, and hs_seq must be given (it then records
                                 * the recurrent h even without dropout: `out` holds h + input). */
  /* DropoutWrapper buffers (NULL when dropout is off): both [B][T+2][units], slot s = time s-1 */
  float* hs_seq;                /* state-dropped h (what the next time step consumed): dWh operand */
  float* xt_seq;                /* output as seen by the consumer above (output mask x its input mask): dWx operand */
  /* GRU (stack.cell == 1; rnn_cell_impl.GRUCell, avsr/cells.py:25-29).  wt/w/bias = gate kernel [in+H][2H] with unit-
   * interleaved columns (2*unit + {0:r,1:u}) and its transpose; wt2/w2/bias2 = candidate kernel [in+H][H].
   * `gates` holds [B][T][H][2] (hoisted x.Wg_x on entry), `cs` the candidate record [B][T][H] (hoisted x.Wc_x on entry),
   * rh_seq [B][T][H] = r*h (dWc operand); backward: dgates [B][T][H][2], dgates2 [B][T][H].
   * wt2 and rh_seq (forward), w2 and dgates2 (backward) are required of every GRU layer, here, in avsr_dec_layer and in
   * avsr_attn_rnn: a call without one returns AVSR_ERR_ARG and writes nothing.  bias2, like bias, may be NULL: a zero bias. */
  const float* wt2;
  const float* w2;
  const float* bias2;
  float* rh_seq;
  float* dgates2;
} avsr_rnn_layer;

typedef struct avsr_rnn_stack {
  int32_t B, T, reverse, n_layers;
  int32_t cell, pad_;             /* 0 = LSTM, 1 = GRU */
  const int32_t* len;
  const float* dh_final;          /* [B][H_top] gradient wrt the top layer's final h (may be NULL) */
  const float* dc_final;
  /* tf.contrib.rnn.DropoutWrapper(input/state/output keep prob, variational_recurrent=False) (avsr/cells.py:46-54).
   * Masks are stateless: bit = hash(*seed, stream, index) (csrc/common.h hash_u32), stream = cell_id*4 + {0 in,1 state,2 out},
   * cell_id = cell_id_base + layer, index = (b*T + t)*width + column.  seed == NULL disables dropout.  With dropout on,
   * `state` scratch must hold 6*B*H floats per layer.  consumer_*: input mask of whatever reads the TOP layer's output
   * through xt_seq (AV-Align attentive layer); consumer_width 0 = none. */
  const int32_t* seed;
  float keep_in, keep_state, keep_out, consumer_keep;
  int32_t cell_id_base, consumer_stream, consumer_width, pad2_;
  avsr_rnn_layer layer[AVSR_MAX_LAYERS];
} avsr_rnn_stack;

int avsr_rnn_fwd(const avsr_rnn_stack* stacks, int32_t n_stacks, void* stream);
int avsr_rnn_bwd(const avsr_rnn_stack* stacks, int32_t n_stacks, void* stream);

/* Opt-in persistent execution of avsr_rnn_fwd (LSTM stacks): ONE launch runs the whole layer/time wavefront,
 * weights and (c, h) state stay in registers, steps are ordered by device-side arrival counters instead of
 * launch boundaries.  `sync` = caller-owned int32 device scratch of `ints` words: word 0 is a sticky error flag
 * (a bounded wait expired; zero it before installing, read it back to check), the rest are counters
 * (264 header words, then per layer 256 progress words for the XCD-local kernels or ceil(B/16)*T arrival counters for the
 * agent-scope forward; a BPTT task whose output crosses an XCD pair adds groups*T more).  NULL disables.  What does not fit
 * silently uses the next form, in the end the per-step launches; same results either way.  A call goes per-step as a whole when
 * any stack is a GRU, has a ResidualWrapper'd layer, or the stacks differ in B.  Forward, per layer: units % 8 == 0, units <= 256,
 * in_dim % 4 == 0, in_dim <= 256 unless hoisted, layer 0 hoisted, `out` given, B*(T+2)*max(ld_out, 4*units) < 2^29, with dropout
 * hs_seq given (and the lower layer's xt_seq); at most 8 layers in a launch, and 96 workgroups per XCD (units/16 for a hoisted layer
 * of units % 16 == 0, else units/8) for the XCD-local kernels, 512 workgroups in all (ceil(B/16) * units/8 per layer) for the
 * agent-scope kernel.  Two stacks that pass all but the 96 together run side by side on XCD halves when each has <= 96 and B <= 64.
 * BPTT, per layer: units % 16 == 0, units <= 256, the layer above takes in_dim == units, B*T*units*4 < 2^29; at most 12 tasks in a
 * launch (K-split: one per layer and one helper per layer edge) and, after the cells are divided over the two XCDs of a pair, 64
 * workgroups (units/16 per task) per XCD for the K-split kernel, which also needs its float scratch, or 28 (units/16, units/32 for a
 * top layer of units % 32 == 0) for the unit-partitioned one.  avsr_rnn_plan answers which form a call would take. */
int avsr_rnn_set_persistent(int32_t* sync, int64_t ints);
/* Which persistent kernels may be used: bit 0 = agent-scope (any placement, 16-row tiles), bit 1 = XCD-local
 * (8-row groups bound to the XCD their workgroups actually run on; tried first) and the persistent BPTT,
 * bit 2 = K-split BPTT off (only the unit-partitioned persistent BPTT runs).  Default 3. */
int avsr_rnn_set_persistent_mode(int mode);
/* Float device scratch for the K-split persistent BPTT (bit 1 of the mode without bit 2): its partial-gradient slabs and one
 * [B,T,units] operand per encoder cell that has a layer above it.  NULL / too small: that form is skipped (the unit-partitioned
 * BPTT or the per-step launches run instead). */
int avsr_rnn_set_persistent_scratch(float* scratch, int64_t floats);
/* Read-only plan query: what avsr_rnn_fwd (bwd == 0) or avsr_rnn_bwd (bwd == 1) WOULD launch for these stacks if `mode` were the
 * avsr_rnn_set_persistent_mode bits, a sync scratch of `sync_ints` words (0 = none) and a K-split float scratch of `scratch_floats`
 * (0 = none) were installed.  Decided by the same host code on its dry path: the descriptors' pointers are only tested for NULL, never
 * dereferenced, nothing is launched and no HIP call is made (runs without a GPU); the installed scratch and mode are left as they
 * were.  Not to be called while another thread is inside avsr_rnn_fwd / avsr_rnn_bwd.  Writes up to `cap` records and returns their
 * number: 1 when all stacks share the launches (and for the per-step form), n_stacks when every stack gets launches of its own; or
 * AVSR_ERR_ARG, or AVSR_ERR_UNSUPPORTED where the call itself would return it (more than 8 layers in all for the per-step form).
 *   form            AVSR_RNN_FORM_*
 *   stacks          stacks covered by this record
 *   rows_per_group  batch rows of a group (forward: per XCD, 8 or 16; agent-scope: per 16-row tile; BPTT: 16 per XCD pair / XCD)
 *   rows_per_slice  batch rows of one launch (0 per-step)
 *   launches        kernel launches: ceil(B / rows_per_slice); per-step: wavefront steps x phases
 *   wg_per_xcd      workgroup slots per XCD (the larger half; agent-scope: workgroups of the launch; 0 per-step)
 *   crossing_edges  BPTT: layer edges that cross the XCD pair
 *   top_tiles       unit-partitioned BPTT: 16-unit tiles per workgroup of a top layer (2 if any top layer takes two) */
#define AVSR_RNN_FORM_PER_STEP 0          /* one launch per wavefront step (csrc/step.hip) */
#define AVSR_RNN_FORM_FWD_XCD8 1          /* rnn_persist_fwd_xcd_kernel<8> */
#define AVSR_RNN_FORM_FWD_XCD8_Q4 2       /* rnn_persist_fwd_xcd_kernel<8, true>: every layer 256 wide */
#define AVSR_RNN_FORM_FWD_XCD16 3         /* rnn_persist_fwd_xcd_kernel<16>: B > 64, 128-row slices */
#define AVSR_RNN_FORM_FWD_PARTS 4         /* rnn_persist_fwd_xcd_kernel<16>, two stacks on XCD halves */
#define AVSR_RNN_FORM_FWD_AGENT 5         /* rnn_persist_fwd_kernel (agent scope) */
#define AVSR_RNN_FORM_BWD_KSPLIT 6        /* rnn_persist_bwdk_kernel, a group per XCD pair, 64-row slices */
#define AVSR_RNN_FORM_BWD_KSPLIT_SOLO 7   /* rnn_persist_bwdk_kernel, a group per XCD, 128-row slices */
#define AVSR_RNN_FORM_BWD_UNIT 8          /* rnn_persist_bwd_kernel (unit-partitioned), 64-row slices */
typedef struct avsr_rnn_launch {
  int32_t form, stacks, rows_per_group, rows_per_slice;
  int32_t launches, wg_per_xcd, crossing_edges, top_tiles;
} avsr_rnn_launch;
int avsr_rnn_plan(const avsr_rnn_stack* stacks, int32_t n_stacks, int32_t bwd, int32_t mode, int64_t sync_ints, int64_t scratch_floats,
                  avsr_rnn_launch* out, int32_t cap);

/* ---------------------------------------------------------------------------------------------
 * Attention-wrapped LSTM over a sequence.  Replaces
 *   seq2seq.dynamic_decode(BasicDecoder(AttentionWrapper(LSTMCell, [mechanisms]), helper, Dense(V)))
 * for the unimodal and bimodal decoders (avsr/decoder_unimodal.py:299-352 train, :176-217 greedy;
 * avsr/decoder_bimodal.py:227-277, :279-326) and tf.nn.dynamic_rnn over the AttentionWrapper'd top
 * audio layer of AV-Align (avsr/encoder.py:265-290).
 *
 * Per step l (AttentionWrapper.call):  x' = [x_l, attention_{l-1}] -> LSTM -> cell_out;
 * for each mechanism m: alpha_m = softmax(score_m(cell_out)), ctx_m = alpha_m . values_m,
 * att_m = [cell_out, ctx_m] . W_att,m;  attention_l = concat_m att_m.
 * Steps with l >= steplen[b] are frozen (state copy-through, zero outputs).
 *
 * mode 0 (train / encoder): x_l . Wx is hoisted by the caller into `gates` (avsr_gemm).
 * mode 1 (greedy):          x_l = embedding[tok[b]]; after each step logits = out . Wout + bout,
 *                           ids[b,l] = argmax (0 once finished), steplen[b] is set when EOS is emitted
 *                           (GreedyEmbeddingHelper + impute_finished).  The caller initialises
 *                           steplen[b] = L and tok[b] = GO, and may run steps in slices [l0, l1).
 *
 * Buffers (A = n_mech * H):
 *   gates [B][L][H][4], cs [B][L][H], cell_out [B][L+1][H] (slot l+1 = step l; slot 0 = h0, written
 *   by the op), att [B][L+1][A] (slot l+1 = attention after step l; slot 0 zero, written by the op),
 *   state scratch 4*B*H (its layout, and dstate's: csrc/cell_state.h).
 *   per mechanism: scores [B][L][T] raw scores (Luong: un-scaled), ctx [B][L][D], pq [B][L][H]
 *   (Bahdanau), pstat [L][2][nchunk][B], pctx scratch [nchunk][B][D], with nchunk = ceil(T / chunk).
 * Backward adds: dgates [B][L][H][4], dstate scratch 12*B*H, datt [B][L][A], dq scratch [B][L][H]
 *   (required with a Luong mechanism or dcell_ext; a staging buffer of the per-step path, not an output: most forms never write it);
 *   per mechanism dscores [B][L][T], dctx [B][L][D], dpq [B][L][H] (Bahdanau), pdq scratch
 *   [nchunk][B][H].  Inputs datt_ext [B][L][A] / dcell_ext [B][L][H]: gradient of the loss wrt the
 *   emitted attention / cell output of every step (from the output layer, or from the consumer of the
 *   encoder memory); either may be NULL.  Outputs dh0, dc0 [B][H].
 */
typedef struct avsr_attn_mech {
  int32_t type;                 /* 0 luong, 1 scaled_luong, 2 bahdanau, 3 normed_bahdanau */
  int32_t T, D, chunk;
  const int32_t* len;           /* [B] memory lengths */
  const float* keys;            /* [B][T][H] */
  const float* values;          /* row (b,t) at values + b*values_sb + t*values_st */
  int64_t values_sb, values_st;
  const float* g;               /* scalar: scaled_luong */
  const float* v;               /* [H] Bahdanau (normed: g*v/|v|) */
  const float* bq;              /* [H] normed_bahdanau bias */
  const float* wq_t;            /* [H][H]   query_layer^T */
  const float* wq;              /* [H][H]   query_layer */
  const float* watt_t;          /* [H][H+D] attention_layer^T */
  const float* watt;            /* [H+D][H] attention_layer */
  float* scores;
  float* ctx;
  float* pq;
  float* pstat;
  float* pctx;
  float* dscores;
  float* dctx;
  float* dpq;
  float* pdq;
} avsr_attn_mech;

/* One extra decoder layer above the attention-fed cell: the wrapped cell is a MultiRNNCell (cells.py:96-100,
 * decoder_unimodal.py:101-108 with len(decoder_units_per_layer) > 1).  LSTM or GRU (the block's cell kind), width = H of the block.  Layer j consumes
 * the emitted output of layer j-1 of the same step; the TOP layer's output is what the attention mechanisms query and
 * what `cell_out` records, so the top layer's `out` must be the block's cell_out.  State starts at zero
 * (decoder_unimodal.py:151-157).  Buffers: wt [4H][2H] / w [2H][4H] (rows: input part, then recurrent part), bias [H][4],
 * gates [B][L][H][4], cs [B][L][H], out [B][L+1][H] (slot l+1 = step l, slot 0 = 0), state 4*B*H, dgates [B][L][H][4],
 * dstate 12*B*H (layout: csrc/cell_state.h); dropout only: hs_seq [B][L+1][H] state-dropped h, xin_seq [B][L+1][H] = the input as this layer consumed it
 * (slot l+1 = step l: lower layer's output mask x this layer's input mask).
 * GRU layers (round 6): wt [2H][2H] / w [2H][2H] = the gate kernel (columns unit-interleaved r, u), bias [H][2], gates [B][L][H][2],
 * cs = the candidate record [B][L][H], dgates [B][L][H][2]; plus the candidate kernel wt2 [H][2H] / w2 [2H][H] (rows: input part, then
 * the r*h part), bias2 [H], rh_seq [B][L][H] (r*h as the candidate consumed it) and dgates2 [B][L][H] (d candidate pre-activation). */
typedef struct avsr_dec_layer {
  const float* wt;
  const float* w;
  const float* bias;
  float* gates;
  float* cs;
  float* out;
  float* state;
  float* hs_seq;
  float* xin_seq;
  float* dgates;
  float* dstate;
  int32_t cell_id, pad_;
  const float* wt2;             /* GRU only (NULL for LSTM layers) */
  const float* w2;
  const float* bias2;
  float* rh_seq;
  float* dgates2;
} avsr_dec_layer;
#define AVSR_MAX_DEC_EXTRA 3

typedef struct avsr_attn_rnn {
  int32_t B, L, H, E, n_mech, output_attention, V, mode;
  int32_t go_id, eos_id;
  int32_t* steplen;             /* [B] valid steps (labels_len / audio len); greedy: updated in place */
  const float* wt;              /* [4H][E + A + H] */
  const float* w;               /* [E + A + H][4H] */
  const float* bias;            /* [H][4] */
  float* gates;
  float* cs;
  float* cell_out;
  float* att;
  const float* h0;
  const float* c0;
  float* state;
  float* h_final;
  float* c_final;
  avsr_attn_mech mech[AVSR_MAX_MECH];
  /* greedy */
  const float* embedding;       /* [V][E] */
  const float* wout_t;          /* [V][O], O = A if output_attention else H */
  const float* bout;            /* [V] */
  float* logits;                /* [B][L][V] (greedy: per-step logits, zero once finished) */
  int32_t* ids;                 /* [B][L] */
  int32_t* tok;                 /* [B] */
  int32_t* n_unfinished;        /* [1] device counter, recomputed after every greedy step */
  /* backward */
  float* dgates;
  float* dstate;
  float* datt;
  float* dq;
  const float* datt_ext;
  const float* dcell_ext;
  float* dh0;
  float* dc0;
  const float* dh_final;        /* [B][H] gradient wrt the final cell state (AV-Align: from the decoder init) */
  const float* dc_final;
  /* DropoutWrapper on the wrapped cell (train only; seed NULL = off), stream = cell_id*4 + kind, input width E + A */
  const int32_t* seed;
  float keep_in, keep_state, keep_out, sampling_prob;
  int32_t cell_id, pad3_;
  float* hs_seq;                /* [B][L+1][H] state-dropped h, slot 0 = h0 (dropout only) */
  float* attd;                  /* [B][L+1][A] input-dropped attention fed to the next step, slot 0 = 0 (dropout only) */
  /* mode 2 = train with scheduled sampling (ScheduledEmbeddingTrainingHelper, avsr/decoder_unimodal.py:304-309):
   * x_l = xs[b][l][:] (caller fills slot 0 = dropout(emb[GO])); after step l the op computes logits[b][l][:], draws
   * select ~ Bernoulli(sampling_prob) and a categorical sample with the stateless RNG (streams 1000 / 1001, index b*L+l)
   * and writes fed[b][l+1] = select ? sample : labels[b][l], xs[b][l+1][:] = dropout(emb[fed[b][l+1]]). */
  float* xs;                    /* [B][L][E] */
  const int32_t* labels;        /* [B][L] */
  int32_t* fed;                 /* [B][L] tokens actually fed (fed[b][0] = GO set by the caller) */
  /* GRU cell (cell == 1): same conventions as avsr_rnn_layer; gates [B][L][H][2], cs = candidate record [B][L][H] */
  int32_t cell, pad4_;
  const float* wt2;
  const float* w2;
  const float* bias2;
  float* rh_seq;
  float* dgates2;
  /* mode 3 = beam search (contrib.seq2seq.BeamSearchDecoder, avsr/decoder_unimodal.py:248-271, avsr/decoder_bimodal.py:358-381):
   * the B rows are beam_width consecutive hypotheses per utterance over tile_batch'ed memories.  After every step the op
   * scores log_softmax(logits) + beam log-prob with the length penalty ((5+len)/6)^w, keeps the top beam_width of the
   * beam_width*V continuations per utterance (ties -> lower index), and records step_ids / parent_ids [L][B].  The next
   * step reads its previous state through parent_rows (no state copies).  Caller initialises tok = GO, parent_rows = identity,
   * beam_logp[0] = {0, -inf, ...} per utterance, beam_fin = beam_len = 0, steplen = L.  In this mode n_unfinished is an
   * [L] array: entry l = number of unfinished beams after step l (dynamic_decode stops at the first 0).
   * mem_shared != 0: the attention memories are NOT tiled -- keys / values / len of every mechanism hold one entry per UTTERANCE
   * (B / beam_width rows) and hypothesis row b attends memory row b / beam_width: the beam_width hypotheses of an utterance read the
   * same bytes (L2 / Infinity-Cache hits) instead of beam_width copies streamed from HBM every step. */
  int32_t beam_width, mem_shared;
  float length_penalty;
  float pad6_;
  float* beam_logp;             /* [2][B] ping-pong */
  int32_t* beam_fin;            /* [2][B] */
  int32_t* beam_len;            /* [2][B] */
  int32_t* step_ids;            /* [L][B] */
  int32_t* parent_ids;          /* [L][B] */
  int32_t* parent_rows;         /* [B] */
  /* multi-layer decoder cell: n_extra layers above the attention-fed one (0 = the plain single cell).  out0 = output
   * record of the attention-fed layer [B][L+1][H] (slot 0 = h0), needed because cell_out then belongs to the top layer. */
  int32_t n_extra, prof_tag;    /* prof_tag: 1 = this block is the AV-Align attentive encoder layer (encoder.py:265-290): its fused launches are
                                 * timed as their own avsr_prof classes (13 / 14) instead of the decoder's (8 / 9); no effect on results */
  float* out0;
  avsr_dec_layer extra[AVSR_MAX_DEC_EXTRA];
  /* Scratch of the fused persistent decode kernel (csrc/dec_persist.hip; avsr/decoder_bimodal.py:241-275,
   * avsr/decoder_unimodal.py:320-350 as ONE launch per call): per-quarter softmax partials and split-K logits.
   * >= avsr_attn_rnn_fused_ws_floats(B, n_mech, Dmax) floats; NULL = always use one launch per step and phase. */
  float* fused_ws;
  int64_t fused_ws_floats;
} avsr_attn_rnn;
int64_t avsr_attn_rnn_fused_ws_floats(int32_t B, int32_t n_mech, int32_t Dmax);
/* 1 if the fused persistent decode kernels are built for this descriptor (the block is inside their plan), else 0. */
int avsr_attn_rnn_fused_eligible(const avsr_attn_rnn* d);
/* 1 if avsr_attn_rnn_fwd(d, ...) WILL run the fused forward kernel right now: eligible, forward fusion switched on
 * (avsr_attn_rnn_set_fused 1 or 2) and the persistent sync scratch registered and large enough.  Greedy decode
 * (avsr/decoder_unimodal.py:176-217) issues all maximum_iterations steps as one call only then; otherwise it keeps its
 * host check every few steps. */
int avsr_attn_rnn_fused_fwd_active(const avsr_attn_rnn* d);
/* avsr_attn_rnn_bwd runs the same block's BPTT loop as one launch of the fused persistent backward kernel (csrc/dec_persist_bwd.hip)
 * under the same conditions.  Process-wide switch: 0 per-step launches, 1 (default) fused forward and backward, 2 forward only,
 * 3 backward only; the path also needs avsr_rnn_set_persistent's sync scratch. */
int avsr_attn_rnn_set_fused(int32_t on);
/* Read-only plan query: what avsr_attn_rnn_fwd (bwd == 0, any step range) or avsr_attn_rnn_bwd (bwd == 1) WOULD launch for this descriptor
 * under the current avsr_attn_rnn_set_fused setting and the sync scratch registered with avsr_rnn_set_persistent.  Decided by the same
 * host code as the calls on its dry path: the descriptor's pointers are only tested for NULL, never dereferenced, nothing is launched and
 * no HIP call is made (runs without a GPU).  Returns AVSR_OK and one record, or the AVSR_ERR_ARG / AVSR_ERR_UNSUPPORTED the call's own
 * argument checks would return.
 *   form            AVSR_ATTN_FORM_*
 *   variant         fused: 0 one Luong memory (<= 128 frames per quarter), 1 two memories (<= 32, <= 128), 2 two memories (<= 128, <= 32),
 *                   3 the attentive layer in 16-row groups (one memory, <= 64 frames per half), 4 one (normed) Bahdanau memory; per-step: -1
 *   rows_per_group  batch rows of a group (8 or 16; 0 per-step)
 *   v64             1 = the 33..64-symbol template of the forward kernel (always 0 for the BPTT: it has no output layer)
 *   launches        fused: kernel launches = slices of 8 groups, ceil(B / (8 * rows_per_group)); per-step: cell launches = L
 *   quarter[m]      frames of memory m resident in one workgroup: ceil(T_m / (32 / rows_per_group)) (0 per-step and for m >= n_mech)
 *   lds_bytes       dynamic LDS of a launch (the BPTT kernel has its own figure; 0 per-step) */
#define AVSR_ATTN_FORM_PER_STEP 0         /* one launch per step and phase (csrc/attn_rnn.hip) */
#define AVSR_ATTN_FORM_FUSED 1            /* dec_persist_kernel / dec_persist_bwd_kernel, one launch per slice */
typedef struct avsr_attn_rnn_launch {
  int32_t form, variant, rows_per_group, v64;
  int32_t launches, pad_;
  int32_t quarter[AVSR_MAX_MECH];
  int64_t lds_bytes;
} avsr_attn_rnn_launch;
int avsr_attn_rnn_plan(const avsr_attn_rnn* d, int32_t bwd, avsr_attn_rnn_launch* out);
/* Beam search (mode 3): which kernels run the B * K-row steps.  1 (default) = all beam-shaped kernels: the per-step attention
 * as one workgroup per (utterance, chunk) serving all K hypotheses over the shared memories, scores and contexts on the matrix
 * pipe with the hypotheses as one MFMA row tile (attn_fwd_beam_mfma_kernel), and the LSTM cell / attention layers as 64 x 64-tiled products with row-gathered operands
 * (csrc/beam_gemm.hip); 2 = the scalar K-hypotheses attention kernel (attn_fwd_beam_kernel) only, dense steps through the small-tile step kernel;
 * 0 = the general kernels everywhere.  0 and 2 give bit-identical scores, statistics and contexts; 1 differs from them by the
 * summation order of the dense products (tests/test_gpu_beam.py checks all three against the oracle). */
int avsr_attn_rnn_set_beam_kernel(int32_t on);

int avsr_attn_rnn_fwd(const avsr_attn_rnn* d, int32_t l_begin, int32_t l_end, void* stream);
int avsr_attn_rnn_bwd(const avsr_attn_rnn* d, void* stream);
/* gather_tree over the recorded beam steps: out[b][t][k] for t < T (ids after the first EOS and past the longest beam = EOS) */
int avsr_beam_gather_tree(const int32_t* step_ids, const int32_t* parent_ids, const int32_t* beam_len, int32_t* out,
                          int32_t n_utt, int32_t beam_width, int32_t T, int32_t eos_id, void* stream);

/* One BeamSearchDecoder step on GIVEN logits [n_utt * beam_width][V] -- the selection avsr_attn_rnn_fwd (mode 3) runs after its output
 * layer, as an entry point of its own (contrib.seq2seq `_beam_search_step` as decoder_unimodal.py:248-271 / decoder_bimodal.py:358-381
 * reach it through BeamSearchDecoder): log_softmax, finished beams continue with EOS at log-probability 0, scores =
 * accumulated log-probability / ((5 + len) / 6)^w with an EOS continuation not counted in len, top beam_width of the beam_width * V
 * continuations per utterance (best first, ties -> lower index).  State in / out: logp, fin, len [n_utt * beam_width] (start:
 * logp = {0, -inf, ...} per utterance, fin = len = 0); tok / parent_rows [n_utt * beam_width] = the kept symbols and the global rows of their
 * parents; step_ids / parent_ids [L][n_utt * beam_width] and n_unfinished [L] (zeroed by the caller) are written at index `step`
 * (a step after one that left n_unfinished == 0 hands the state through unchanged).  beam_width * V <= 1024.
 * x != NULL: the decoder's output layer runs inside the step as it does in the default evaluation path (seq2seq.py:339 Dense(vocab)):
 * logits [row][v] = x[row * x_stride + .] (O inputs) . wout_t[v][.] + bout[v] are COMPUTED (and written to `logits`) before the selection;
 * needs beam_width <= 16, V <= 64, O % 256 == 0, 16-byte aligned x / wout_t, else AVSR_ERR_UNSUPPORTED.  x == NULL: `logits` is the input.
 * tests/test_gpu_beam.py replays TensorFlow's own trace of the reference's sample search (avsr/visualise/00025.html) through it. */
int avsr_beam_search_step(float* logits, int32_t n_utt, int32_t beam_width, int32_t V, int32_t step, int32_t eos_id,
                          float length_penalty_weight, const float* logp_in, const int32_t* fin_in, const int32_t* len_in,
                          float* logp_out, int32_t* fin_out, int32_t* len_out, int32_t* tok, int32_t* parent_rows,
                          int32_t* step_ids, int32_t* parent_ids, int32_t* n_unfinished, const float* x, int64_t x_stride,
                          int32_t O, const float* wout_t, const float* bout, void* stream);

/* Shallow fusion of a language model into beam search (csrc/beam_lm.hip).  The reference trains such a model (avsr/lm.py,
 * experiment_lrs2_lm.py) but never connects it to the recogniser; the scoring rule is this project's own:
 *   step_logp[k][v] = log_softmax(logits_am[k])[v] + lm_weight * log_softmax(logits_lm[k])[v]        (unfinished beam k)
 * and everything else of the step is avsr_beam_search_step unchanged (a finished beam continues with EOS at log-probability 0, no
 * language-model term; EOS gets its term like any other symbol).  lm_weight == 0 reproduces the search without a model bit for bit.
 * The model is avsr.LM's evaluate graph: embedding (or one-hot rows) of the previous symbol -> n_layers LSTM layers of width H from the
 * zero state (TF gate order i, j, f, o, forget bias 1, cell clip 1, the cell of avsr_rnn_layer) -> Dense(V) -> log_softmax.  Each
 * hypothesis row keeps (c, h) of every layer; after a selection row r continues from the state of row parent_rows[r], read out of the
 * other half of a ping-pong (step s reads half s & 1 and writes half (s + 1) & 1; step 0 zeroes half 0 first).
 * Buffers: embedding [V][E] (one_hot != 0: the unit rows, E >= V, that the engine keeps for embedding_size <= 0; the flag is
 * informational -- the kernels read the table either way, only the host check E >= V looks at it), wt[j] [4H][K_j] with
 * K_0 = E + H and K_j = 2H (rows: input part, then recurrent part; gate columns unit-interleaved as everywhere), bias[j] [H][4],
 * wout_t [V][H], bout [V], state_c / state_h [2][n_layers][n_rows][H], lm_logp [n_rows][V].  H % 4 == 0, E % 4 == 0, V <= 1024,
 * 1 <= n_layers <= AVSR_MAX_LM_LAYERS.  tok[r] must lie in [0, V) and parent_rows[r] in [0, n_rows): what avsr_beam_search_step writes. */
#define AVSR_MAX_LM_LAYERS 4
typedef struct avsr_beam_lm {
  int32_t n_layers, H, E, V;
  int32_t one_hot, n_rows;
  float lm_weight;
  int32_t pad_;
  const float* embedding;
  const float* wt[AVSR_MAX_LM_LAYERS];
  const float* bias[AVSR_MAX_LM_LAYERS];
  const float* wout_t;
  const float* bout;
  float* state_c;
  float* state_h;
  float* lm_logp;
} avsr_beam_lm;
/* 1 if avsr_beam_lm_step runs this descriptor, else 0 (decided on the host; nothing is dereferenced). */
int avsr_beam_lm_supported(const avsr_beam_lm* lm);
/* One language-model step over n_rows (== lm->n_rows) hypothesis rows: n_layers launches of the row-gathered MFMA cell product
 * (beam_gemm_kernel) and one of the output layer + log_softmax; rows past n_rows of a partial tile contribute and write nothing. */
int avsr_beam_lm_step(const avsr_beam_lm* lm, const int32_t* tok, const int32_t* parent_rows, int32_t n_rows, int32_t step, void* stream);
/* avsr_beam_search_step with the language-model term: lm_logp [n_utt * beam_width][V] (NULL = avsr_beam_search_step exactly). */
int avsr_beam_search_step_lm(float* logits, int32_t n_utt, int32_t beam_width, int32_t V, int32_t step, int32_t eos_id,
                             float length_penalty_weight, const float* logp_in, const int32_t* fin_in, const int32_t* len_in,
                             float* logp_out, int32_t* fin_out, int32_t* len_out, int32_t* tok, int32_t* parent_rows,
                             int32_t* step_ids, int32_t* parent_ids, int32_t* n_unfinished, const float* x, int64_t x_stride,
                             int32_t O, const float* wout_t, const float* bout, const float* lm_logp, float lm_weight, void* stream);
/* avsr_attn_rnn_fwd in mode 3 with avsr_beam_lm_step ahead of every selection (lm->n_rows == d->B, lm->V == d->V), under every
 * avsr_attn_rnn_set_beam_kernel setting.  A step queued after the search has ended advances the model harmlessly (tok = EOS,
 * parent_rows = identity) and its output is not read. */
int avsr_attn_rnn_fwd_lm(const avsr_attn_rnn* d, const avsr_beam_lm* lm, int32_t l_begin, int32_t l_end, void* stream);

/* Joint CTC / attention scoring inside beam search (csrc/beam_ctc.hip; the rule is this project's own):
 *   step_logp[k][v] = log_softmax(logits_am[k])[v] (+ lm_weight * log p_lm) + weight * (psi(g_k . v) - psi(g_k))      (unfinished beam k)
 * psi(g) = log-probability, under the CTC head, of all label sequences that start with the beam's label prefix g; psi(g . EOS) =
 * log p_ctc(g | x).  The term is 0 where psi(g_k) = -inf or the utterance has no frames, may be -inf, is never NaN; a finished beam
 * gets none.  The terms telescope: a beam that ends with EOS has accumulated weight * log p_ctc(its labels | x).
 * z: the head's logits [n_utt * T][ld] over V + 1 real classes, the blank is class V; in_len [n_utt], T_b = clamp(in_len, 0, T).
 * Buffers: y [n_utt][T][V + 1] (log_softmax of the rows t < T_b); state [2][R][T][2] (r_n, r_b per frame), psi [2][R], last [2][R]
 * with R = n_utt * beam_width: a ping-pong like avsr_beam_lm's -- avsr_beam_ctc_begin writes the empty prefix into half 0, step s reads
 * row parent_rows[r] of half s & 1 and writes row r of half (s + 1) & 1 (step 0: tok = GO, the empty prefix is copied through and
 * scored; a row with tok = EOS or fin != 0 copies its parent through and gets term 0).  term [R][V]; extra [R][V] = weight * term
 * (+ lm_weight * lm_logp where lm_logp != NULL: the buffer the selection reads as its one additive term, with weight 1).
 * 1 <= T <= AVSR_BEAM_CTC_MAX_T, 2 <= V <= AVSR_BEAM_CTC_MAX_V, beam_width <= 64, weight >= 0, ld >= V + 1. */
#define AVSR_BEAM_CTC_MAX_T 2048
#define AVSR_BEAM_CTC_MAX_V 256
typedef struct avsr_beam_ctc {
  int32_t n_utt, beam_width, T, V;
  int32_t eos_id;
  float weight;
  int64_t ld;
  const float* z;
  const int32_t* in_len;
  float* y;
  float* state;
  float* psi;
  int32_t* last;
  float* term;
  float* extra;
  const float* lm_logp;      /* NULL, or the fused language model's [R][V] (avsr_beam_lm.lm_logp) */
  float lm_weight;
  int32_t pad_;
} avsr_beam_ctc;
/* 1 if the entry points below run this descriptor, else 0 (decided on the host; nothing is dereferenced). */
int avsr_beam_ctc_supported(const avsr_beam_ctc* ctc);
/* Once per decode: y and the empty prefix's state (half 0).  One launch. */
int avsr_beam_ctc_begin(const avsr_beam_ctc* ctc, void* stream);
/* One step over the R rows: state update, then term and extra.  tok / parent_rows / fin [R] as avsr_beam_search_step leaves them
 * (values outside [0, V) / [0, R) are clamped: nothing outside the buffers is addressed).  One launch. */
int avsr_beam_ctc_step(const avsr_beam_ctc* ctc, const int32_t* tok, const int32_t* parent_rows, const int32_t* fin, int32_t step,
                       void* stream);
/* avsr_beam_search_step_lm with the CTC term next to the language model's: ctc_term [n_utt * beam_width][V] and a scratch buffer
 * extra of the same size, into which weight * ctc_term (+ lm_weight * lm_logp) is combined first.  ctc_term == NULL or
 * ctc_weight == 0: avsr_beam_search_step_lm exactly (extra is not touched). */
int avsr_beam_search_step_ctc(float* logits, int32_t n_utt, int32_t beam_width, int32_t V, int32_t step, int32_t eos_id,
                              float length_penalty_weight, const float* logp_in, const int32_t* fin_in, const int32_t* len_in,
                              float* logp_out, int32_t* fin_out, int32_t* len_out, int32_t* tok, int32_t* parent_rows,
                              int32_t* step_ids, int32_t* parent_ids, int32_t* n_unfinished, const float* x, int64_t x_stride,
                              int32_t O, const float* wout_t, const float* bout, const float* lm_logp, float lm_weight,
                              const float* ctc_term, float ctc_weight, float* extra, void* stream);
/* avsr_attn_rnn_fwd in mode 3 with avsr_beam_ctc_step -- after avsr_beam_lm_step when lm != NULL -- ahead of every selection, under
 * every avsr_attn_rnn_set_beam_kernel setting (ctc->n_utt * ctc->beam_width == d->B, ctc->V == d->V; with lm, ctc->lm_logp must be
 * lm->lm_logp).  The caller has run avsr_beam_ctc_begin.  ctc->weight == 0: avsr_attn_rnn_fwd / avsr_attn_rnn_fwd_lm exactly, no CTC
 * launch.  A step queued after the search has ended (tok = EOS, parent_rows = identity) copies state through and is not read. */
int avsr_attn_rnn_fwd_ctc(const avsr_attn_rnn* d, const avsr_beam_lm* lm, const avsr_beam_ctc* ctc, int32_t l_begin, int32_t l_end,
                          void* stream);

/* CTC prefix beam search on the head's logits alone (csrc/ctc_prefix.hip; the rule is this project's own):
 * frame-synchronous, sums over alignments, no decoder step.  z [B * T][ld] are the head's logits over V + 1 real classes, the blank
 * is class V; in_len [B], T_b = clamp(in_len, 0, T).  Frames t >= T_b and columns >= V + 1 of a wider row are never read.
 * Outputs, per utterance the final beam sorted by p = p_b (+) p_nb descending (ties: the lower candidate index):
 *   ids [B][beam_width][L_max] (-1 padded), lens [B][beam_width] (0 for an empty slot), score [B][beam_width] (p; -inf for an empty
 *   slot).  Without pruning p is log p_ctc(labels | x); T_b = 0 gives the empty sequence with score 0.  Nothing is ever NaN.
 * Trace (all four NULL in production, or all four given): the beam after every frame t < T_b as [B][T][beam_width] -- the slot of the
 * previous beam it continues, the symbol (V = stay; -1 / -1 for an empty slot), p_b and p_nb.  Rows t >= T_b are not written.
 * One launch, one workgroup per utterance, no atomics: bit-identical across launches.
 * Limits (all state of the search lives in LDS): 1 <= V <= 256, 1 <= beam_width <= 64, 1 <= L_max <= 512 -- at the three maxima the
 * workgroup holds 135 KiB of the CU's 160 KiB. */
#define AVSR_CTC_PREFIX_MAX_V 256
#define AVSR_CTC_PREFIX_MAX_W 64
#define AVSR_CTC_PREFIX_MAX_L 512
typedef struct avsr_ctc_prefix_args {
  int32_t B, T, V, beam_width, L_max;
  int32_t pad_;
  int64_t ld;
  const float* z;
  const int32_t* in_len;
  int32_t* ids;
  int32_t* lens;
  float* score;
  int32_t* trace_parent;
  int32_t* trace_sym;
  float* trace_pb;
  float* trace_pnb;
} avsr_ctc_prefix_args;
/* 1 if avsr_ctc_prefix_search runs this shape, else 0 (decided on the host; nothing is dereferenced). */
int avsr_ctc_prefix_search_supported(int32_t V, int32_t beam_width, int32_t L_max);
/* AVSR_ERR_ARG for a NULL / non-positive / inconsistent argument, AVSR_ERR_UNSUPPORTED outside the limits: both before any launch. */
int avsr_ctc_prefix_search(const avsr_ctc_prefix_args* a, void* stream);

/* The prefix search with a language model fused into the frame loop (csrc/ctc_prefix_lm.hip; the rule is INTEGRATION.md section 8):
 *   extend g by c < V:   next[g.c].p_nb (+)= (p_b if c == last(g) else p) + y[t][c] + (weight * lam(c | g) + bonus)
 *   after the last frame final[g] = p + weight * lam(EOS | g), and the beam is re-sorted by final (descending, ties to the earlier slot)
 * lam(. | g) = log_softmax of avsr.LM's evaluate graph (avsr_beam_lm's model and buffer layouts: embedding [V][E], wt[j] [4H][K_j],
 * bias[j] [H][4], wout_t [V][H], bout [V]) after GO, g_0 .. g_{n-1} from the zero state.  Stays, merging, candidate indices, selection
 * on p and ties are avsr_ctc_prefix_search's; weight == 0 and bonus == 0 give its ids, lens and score.  Every one of the V classes, GO
 * and EOS included, gets its term.  a->score holds final; the trace (a->trace_*) is the per-frame beam, before the final re-sort.
 *   s_lm [B][beam_width]        sum_i lam(g_i | g_0 .. g_{i-1}) + lam(EOS | g) of the entry at that output position (0 for an empty slot)
 *   lm_steps [B]                number of frames on which the model's step ran (the frames that kept an extension)
 *   lm_logp [B][beam_width][V]  NULL, or (debug) the row lam(. | g) of every output entry (0 for an empty slot)
 *   ws                          avsr_ctc_prefix_lm_ws_bytes(B, beam_width, n_layers, H) bytes, 16-byte aligned: (c, h) of 2 beam_width
 *                               label sequences per utterance; written before it is read, so it needs no initial value
 * One launch, one workgroup per utterance, no atomics: bit-identical across launches.  The model's step runs inside the frame loop.
 * Limits: avsr_ctc_prefix_search's on V and L_max, 1 <= beam_width <= AVSR_CTC_PREFIX_LM_MAX_W (the kept extensions of a frame are ONE
 * 16-row MFMA tile), V == lm->V, 0 <= go_id, eos_id < V, and a model avsr_beam_lm_supported accepts: 1 <= n_layers <= AVSR_MAX_LM_LAYERS,
 * H % 4 == 0, E % 4 == 0 (one_hot != 0: E >= V).  weight finite and >= 0, bonus finite. */
#define AVSR_CTC_PREFIX_LM_MAX_W 16
typedef struct avsr_ctc_prefix_lm {
  int32_t n_layers, H, E, V;
  int32_t one_hot, go_id, eos_id;
  float weight, bonus;
  int32_t pad_;
  const float* embedding;
  const float* wt[AVSR_MAX_LM_LAYERS];
  const float* bias[AVSR_MAX_LM_LAYERS];
  const float* wout_t;
  const float* bout;
  void* ws;
  int64_t ws_bytes;
  float* s_lm;
  int32_t* lm_steps;
  float* lm_logp;
} avsr_ctc_prefix_lm;
/* 1 if avsr_ctc_prefix_search_lm runs this shape, else 0 (decided on the host; nothing is dereferenced). */
int avsr_ctc_prefix_lm_supported(int32_t V, int32_t beam_width, int32_t L_max, int32_t n_layers, int32_t H, int32_t E, int32_t one_hot);
/* Bytes of avsr_ctc_prefix_lm.ws (0 for a non-positive argument). */
int64_t avsr_ctc_prefix_lm_ws_bytes(int32_t B, int32_t beam_width, int32_t n_layers, int32_t H);
/* AVSR_ERR_ARG for a NULL / non-positive / inconsistent argument, AVSR_ERR_UNSUPPORTED outside the limits: both before any launch. */
int avsr_ctc_prefix_search_lm(const avsr_ctc_prefix_args* a, const avsr_ctc_prefix_lm* lm, void* stream);

/* The same fused search with a back-off N-GRAM as the model (csrc/ctc_prefix_ngram.hip; the rule is INTEGRATION.md section 8): every
 * word above about extensions, final, s_lm, lm_steps, lm_logp, the trace and weight == 0 holds; only lam(. | g) differs.  The model is
 * a device-resident automaton (avsr-tf1_amd/ngram.py compile_tables writes it).  Node 0 is the root (the empty context); every other node
 * is a context of 1 .. N-1 symbols:
 *   bow [n_nodes]            back-off weight of the context (natural log; 0 at the root, which is never left)
 *   backoff [n_nodes]        node of the context without its first symbol (0 at the root)
 *   arc_begin [n_nodes + 1]  the node's arcs are [arc_begin[n], arc_begin[n + 1]), sorted by sym; the root's are the V arcs 0 .. V-1 with
 *                            sym[c] == c (a class the model lacks holds the floor -99 ln 10 and next = 0), so arc_begin[1] == V
 *   sym, logp, next [n_arcs] the class, lam(sym | context) where the n-gram is listed, and the node of the longest suffix of
 *                            context . sym that is a node
 * One value: acc = 0; while the node has no arc for c: acc += bow[node], node = backoff[node]; then lam = acc + logp[arc] -- fp32
 * additions in exactly this order, so a host restatement in fp32 gives the same bits.  The walk visits at most
 * AVSR_CTC_PREFIX_NGRAM_MAX_ORDER - 1 nodes before it looks at the root, whatever the tables hold, and every index it reads is clamped
 * into its table (the walk is csrc/ngram_walk.h, shared with avsr_beam_ngram below).  The label sequence () has node `start` (the node
 * of (GO), or 0); an extension by c moves its node along next.
 * No workspace: the state is one node id per pool row, in LDS.
 * Limits: avsr_ctc_prefix_search's on V and L_max, 1 <= beam_width <= AVSR_CTC_PREFIX_LM_MAX_W, 1 <= n_nodes <=
 * AVSR_CTC_PREFIX_NGRAM_MAX_NODES, V <= n_arcs <= AVSR_CTC_PREFIX_NGRAM_MAX_ARCS; V == a->V, 0 <= go_id, eos_id < V, 0 <= start <
 * n_nodes; weight finite and >= 0, bonus finite. */
#define AVSR_CTC_PREFIX_NGRAM_MAX_ORDER 16
#define AVSR_CTC_PREFIX_NGRAM_MAX_NODES (1 << 24)
#define AVSR_CTC_PREFIX_NGRAM_MAX_ARCS (1 << 26)
typedef struct avsr_ctc_prefix_ngram {
  int32_t n_nodes, n_arcs, V, start;
  int32_t go_id, eos_id;
  float weight, bonus;
  const float* bow;
  const int32_t* backoff;
  const int32_t* arc_begin;
  const int32_t* sym;
  const float* logp;
  const int32_t* next;
  float* s_lm;
  int32_t* lm_steps;
  float* lm_logp;
} avsr_ctc_prefix_ngram;
/* 1 if avsr_ctc_prefix_search_ngram runs this shape, else 0 (decided on the host; nothing is dereferenced). */
int avsr_ctc_prefix_ngram_supported(int32_t V, int32_t beam_width, int32_t L_max, int32_t n_nodes, int32_t n_arcs);
/* AVSR_ERR_ARG for a NULL / non-positive / inconsistent argument, AVSR_ERR_UNSUPPORTED outside the limits: both before any launch. */
int avsr_ctc_prefix_search_ngram(const avsr_ctc_prefix_args* a, const avsr_ctc_prefix_ngram* ng, void* stream);

/* The same fused search over CHARACTER units with a WORD-level back-off n-gram behind a lexicon trie (csrc/ctc_prefix_word_ngram.hip;
 * the rule, with its table of cases, is INTEGRATION.md section 8): every word above about extensions, final, s_lm, lm_steps, lm_logp,
 * the trace and weight == 0 holds; only lam(. | g) differs.  Units: space_id is the space, class 0 (MASK) and go_id are non-units,
 * eos_id is EOS, every other class below V is a letter.  Two read-only tables (avsr-tf1_amd/ngram.py compile_word_tables writes them):
 *   the word automaton   avsr_ctc_prefix_ngram's six tables over WORD ids 0 .. Vw-1 (the root holds Vw arcs), walked by the same
 *                        csrc/ngram_walk.h; start = the node of (<s>), eos_w = the id of </s>, unk_id = the id of <unk> or -1
 *   the lexicon trie     CSR over the vocabulary's spellings, node 0 the root: the children of node n are the arcs
 *                        [t_begin[n], t_begin[n + 1]), t_sym (unit ids) sorted per node, t_next the child; t_word[n] = the word that
 *                        ends at n, or -1
 * State of a label sequence, a function of the labels alone: (h, p) = (the automaton node of the words closed so far, the trie node of
 * the letters since the last space -- the root without any, the sink OOV once they have left every spelling).
 *   letter c:   0 if p has the child c or p is OOV, else oov (paid once, on leaving the lexicon)
 *   space:      0 at the root; walk(h, w) where p ends the word w; oov + U(h) at a proper prefix; U(h) at OOV --
 *               U(h) = walk(h, <unk>), or 0 with h -> node 0 when the model has no <unk>
 *   EOS:        (what the space costs) + walk(the node after that space, </s>)
 *   MASK, GO:   the floor -99 ln 10
 * fp32 additions in exactly this order, so the host restatement (ngram.py word_lam) gives the same bits.  Every node id, word id and
 * arc range read from a table is clamped into its table; all loops are bounded.
 * No workspace: the state and three cached scalars per pool row live in LDS.
 * Limits: avsr_ctc_prefix_search_ngram's, with AVSR_CTC_PREFIX_NGRAM_MAX_NODES / _MAX_ARCS applied to the trie as well (1 <=
 * n_trie_nodes, 1 <= n_trie_arcs); 2 <= Vw <= n_arcs, 0 <= eos_w < Vw, -1 <= unk_id < Vw; 0 <= space_id < V with space_id, go_id and
 * eos_id distinct; oov finite and <= 0. */
typedef struct avsr_ctc_prefix_word_ngram {
  int32_t n_nodes, n_arcs, Vw, start;
  int32_t eos_w, unk_id, n_trie_nodes, n_trie_arcs;
  int32_t V, space_id, go_id, eos_id;
  float weight, bonus, oov;
  int32_t pad_;
  const float* bow;
  const int32_t* backoff;
  const int32_t* arc_begin;
  const int32_t* sym;
  const float* logp;
  const int32_t* next;
  const int32_t* t_begin;
  const int32_t* t_sym;
  const int32_t* t_next;
  const int32_t* t_word;
  float* s_lm;
  int32_t* lm_steps;
  float* lm_logp;
} avsr_ctc_prefix_word_ngram;
/* 1 if avsr_ctc_prefix_search_word_ngram runs this shape, else 0 (decided on the host; nothing is dereferenced). */
int avsr_ctc_prefix_word_ngram_supported(int32_t V, int32_t beam_width, int32_t L_max, int32_t n_nodes, int32_t n_arcs, int32_t Vw,
                                         int32_t n_trie_nodes, int32_t n_trie_arcs);
/* AVSR_ERR_ARG for a NULL / non-positive / inconsistent argument, AVSR_ERR_UNSUPPORTED outside the limits: both before any launch. */
int avsr_ctc_prefix_search_word_ngram(const avsr_ctc_prefix_args* a, const avsr_ctc_prefix_word_ngram* wg, void* stream);

/* Shallow fusion of the same back-off N-GRAM into BEAM SEARCH (csrc/beam_ngram.hip; the rule is this project's own, INTEGRATION.md
 * section 8), the counterpart of avsr_beam_lm with the automaton above as the model:
 *   step_logp[k][v] = log_softmax(logits_am[k])[v] + lm_weight * lam(v | GO, g_k)  (+ the CTC term of avsr_beam_ctc)     (unfinished beam k)
 * lam is exactly the value of avsr_ctc_prefix_ngram: context = the last N-1 symbols of GO, g_k, back-off, the finite floor for a class
 * the model lacks -- so the term is always finite.  EOS gets its term like any other symbol; a finished beam continues with EOS at 0 and
 * no term; lm_weight == 0 reproduces the search without a model bit for bit.  No length bonus: beam search has its length penalty.
 * The six tables are avsr_ctc_prefix_ngram's (ngram.py compile_tables), read by the one walk both kernels share (csrc/ngram_walk.h): fp32
 * additions in its fixed order, at most AVSR_CTC_PREFIX_NGRAM_MAX_ORDER - 1 nodes before the root, every index clamped into its table.
 * State: one node id per hypothesis row in a ping-pong node [2][n_rows] like avsr_beam_lm's -- step s reads node[s & 1][parent_rows[r]]
 * and writes node[(s + 1) & 1][r]; step 0 puts every row at `start` and reads neither tok nor the other half.  A row whose tok is EOS
 * transitions like any other; its values are never read.  tok / parent_rows outside [0, V) / [0, n_rows) are clamped.
 * Limits: 1 <= n_nodes <= AVSR_CTC_PREFIX_NGRAM_MAX_NODES, 2 <= V <= n_arcs <= AVSR_CTC_PREFIX_NGRAM_MAX_ARCS, 0 <= start < n_nodes,
 * n_rows >= 1 (n_rows * V < 2^31), lm_weight finite and >= 0.  No beam-width limit of its own: beam search's hold (K <= 64, K * V <= 1024). */
typedef struct avsr_beam_ngram {
  int32_t n_nodes, n_arcs, V, start;
  int32_t n_rows;
  float lm_weight;
  const float* bow;
  const int32_t* backoff;
  const int32_t* arc_begin;
  const int32_t* sym;
  const float* logp;
  const int32_t* next;
  int32_t* node;       /* [2][n_rows] */
  float* lm_logp;      /* [n_rows][V] */
} avsr_beam_ngram;
/* 1 if avsr_beam_ngram_step runs this descriptor, else 0 (decided on the host; nothing is dereferenced). */
int avsr_beam_ngram_supported(const avsr_beam_ngram* ng);
/* One n-gram step over n_rows (== ng->n_rows) hypothesis rows: the transition into the other half of node, then lm_logp[r][c] =
 * lam(c | row r's context) for every c < V.  One launch, plain loads and vector stores, no atomics: two launches are bit-identical.
 * AVSR_ERR_ARG for a NULL / non-positive / inconsistent argument, AVSR_ERR_UNSUPPORTED outside the limits: both before any launch. */
int avsr_beam_ngram_step(const avsr_beam_ngram* ng, const int32_t* tok, const int32_t* parent_rows, int32_t n_rows, int32_t step, void* stream);
/* avsr_attn_rnn_fwd in mode 3 with avsr_beam_ngram_step ahead of every selection (ng->n_rows == d->B, ng->V == d->V), under every
 * avsr_attn_rnn_set_beam_kernel setting.  ctc != NULL: avsr_beam_ctc_step runs after it and the selection reads ctc->extra with weight 1,
 * exactly as avsr_attn_rnn_fwd_ctc does with an LSTM (ctc->lm_logp must be ng->lm_logp; the caller has run avsr_beam_ctc_begin;
 * ctc->weight == 0: no CTC launch).  A step queued after the search has ended (tok = EOS, parent_rows = identity) advances the nodes
 * harmlessly and its output is not read.  An LSTM and an n-gram in one search are not built. */
int avsr_attn_rnn_fwd_ngram(const avsr_attn_rnn* d, const avsr_beam_ngram* ng, const avsr_beam_ctc* ctc, int32_t l_begin, int32_t l_end,
                            void* stream);

/* Shallow fusion of the WORD-level back-off n-gram behind a lexicon trie into BEAM SEARCH over character units
 * (csrc/beam_word_ngram.hip), the counterpart of avsr_beam_ngram with avsr_ctc_prefix_word_ngram's model:
 *   step_logp[k][v] = log_softmax(logits_am[k])[v] + lm_weight * lam(v | g_k)  (+ the CTC term of avsr_beam_ctc)         (unfinished beam k)
 * lam is exactly the value of avsr_ctc_prefix_word_ngram (the table of cases above: letters, space, EOS, MASK / GO), formed by the one
 * copy of the model's side both kernels include (csrc/word_ngram_walk.h): fp32 additions in its fixed order, so ngram.py word_lam gives
 * the same bits; always finite.  EOS gets its term like any other symbol; a finished beam continues with EOS at 0 and no term;
 * lm_weight == 0 reproduces the search without a model bit for bit.  No length bonus.  The ten tables and the scalars are
 * avsr_ctc_prefix_word_ngram's (ngram.py compile_word_tables).
 * State: (h, p, hc) per hypothesis row -- the automaton node of the closed words, the trie node of the open word (0 = root, -1 = OOV)
 * and the node a space would leave (h at the root) -- as int32 state [2][3][n_rows]: step s reads half s & 1 at parent_rows[r] and
 * writes half (s + 1) & 1 at r; step 0 puts every row at (start, 0, start) and reads neither tok nor the other half.  A row whose tok
 * is EOS transitions like any other; its values are never read.  tok / parent_rows outside [0, V) / [0, n_rows) are clamped to 0, a
 * stale h or hc outside [0, n_nodes) to 0, a stale p outside [-1, n_trie_nodes) to the root: nothing outside the buffers is addressed.
 * Limits: avsr_beam_ngram's on the automaton (over Vw word ids: 2 <= Vw <= n_arcs), n_rows and lm_weight, and
 * avsr_ctc_prefix_word_ngram's on the trie and scalars: 1 <= n_trie_nodes <= AVSR_CTC_PREFIX_NGRAM_MAX_NODES, 1 <= n_trie_arcs <=
 * AVSR_CTC_PREFIX_NGRAM_MAX_ARCS, 0 <= eos_w < Vw, -1 <= unk_id < Vw, space_id, go_id and eos_id distinct classes below V, oov finite
 * and <= 0.  No beam-width limit of its own: beam search's hold (K <= 64, K * V <= 1024). */
typedef struct avsr_beam_word_ngram {
  int32_t n_nodes, n_arcs, Vw, start;
  int32_t eos_w, unk_id, n_trie_nodes, n_trie_arcs;
  int32_t V, space_id, go_id, eos_id;
  int32_t n_rows;
  float lm_weight, oov;
  int32_t pad_;
  const float* bow;
  const int32_t* backoff;
  const int32_t* arc_begin;
  const int32_t* sym;
  const float* logp;
  const int32_t* next;
  const int32_t* t_begin;
  const int32_t* t_sym;
  const int32_t* t_next;
  const int32_t* t_word;
  int32_t* state;      /* [2][3][n_rows]: h, p, hc */
  float* lm_logp;      /* [n_rows][V] */
} avsr_beam_word_ngram;
/* 1 if avsr_beam_word_ngram_step runs this descriptor, else 0 (decided on the host; nothing is dereferenced). */
int avsr_beam_word_ngram_supported(const avsr_beam_word_ngram* wn);
/* One word-model step over n_rows (== wn->n_rows) hypothesis rows: the transition into the other half of state, then lm_logp[r][c] =
 * lam(c | row r's labels) for every c < V.  One launch, plain loads and vector stores, no atomics: two launches are bit-identical.
 * AVSR_ERR_ARG for a NULL / non-positive / inconsistent argument, AVSR_ERR_UNSUPPORTED outside the limits: both before any launch. */
int avsr_beam_word_ngram_step(const avsr_beam_word_ngram* wn, const int32_t* tok, const int32_t* parent_rows, int32_t n_rows, int32_t step,
                              void* stream);
/* avsr_attn_rnn_fwd in mode 3 with avsr_beam_word_ngram_step ahead of every selection (wn->n_rows == d->B, wn->V == d->V), under every
 * avsr_attn_rnn_set_beam_kernel setting; ctc as in avsr_attn_rnn_fwd_ngram (ctc->lm_logp must be wn->lm_logp; ctc->weight == 0: no CTC
 * launch).  A step queued after the search has ended advances the states harmlessly and its output is not read.  Two fused models in
 * one search are not built. */
int avsr_attn_rnn_fwd_word_ngram(const avsr_attn_rnn* d, const avsr_beam_word_ngram* wn, const avsr_beam_ctc* ctc, int32_t l_begin,
                                 int32_t l_end, void* stream);

/* CTC forced alignment (csrc/ctc_align.hip; the rule is this project's own): the single most probable
 * alignment (Viterbi path) of a GIVEN label row to the frames of the head.  z [B * T][ld] are the head's logits over V + 1 real classes,
 * the blank is class V; in_len [B], T_b = clamp(in_len, 0, T); labels [B][L], target_len [B], U = clamp(target_len, 0, L) -- a plain
 * label count: nothing is cut off for an EOS.  Frames t >= T_b and columns >= V + 1 of a wider row are never read.
 *   score [B]          log-probability of the best alignment (0 without one)
 *   status [B]         1, or 0 when the utterance has no valid alignment -- avsr_ctc_loss's test: T_b < U + adjacent equal label
 *                      pairs, T_b == 0, or a label outside 0 .. V-1; then every per-frame and per-label output holds its padding
 *   path [B][T]        the class of every frame t < T_b (blank = V), -1 for t >= T_b
 *   frame_lp [B][T]    log_softmax(z[b, t, :V+1])[path[t]], 0 for t >= T_b
 *   start, end [B][L]  first and last frame of label j's run, inclusive; -1 for j >= U
 * Ties go to the higher state index: stay over s - 1 over s - 2, and at the end the last blank over the last label.
 * ws: avsr_ctc_align_ws_bytes(B, T, L) bytes of scratch, 8-byte aligned (row normalisers and 2-bit backpointers over all T frames
 * live there, so T is not bounded by on-chip memory).  One launch, one workgroup per utterance, no atomics (two launches on the same
 * inputs are bit-identical), no host read, no memset / memcpy: safe under stream capture.  Every output element is written by every
 * launch.  Nothing is ever NaN.  Limits: 1 <= L <= 512, any V >= 1, any T. */
#define AVSR_CTC_ALIGN_MAX_L 512
typedef struct avsr_ctc_align_args {
  int32_t B, T, L, V;
  int64_t ld;
  const float* z;
  const int32_t* labels;
  const int32_t* target_len;
  const int32_t* in_len;
  float* score;
  int32_t* status;
  int32_t* path;
  float* frame_lp;
  int32_t* start;
  int32_t* end;
  void* ws;
  int64_t ws_bytes;
} avsr_ctc_align_args;
/* 1 if avsr_ctc_align runs this shape, else 0 (decided on the host; nothing is dereferenced). */
int avsr_ctc_align_supported(int32_t V, int32_t L);
int64_t avsr_ctc_align_ws_bytes(int32_t B, int32_t T, int32_t L);
/* AVSR_ERR_ARG for a NULL pointer, a non-positive size, ld < V + 1, a misaligned ws or ws_bytes too small, AVSR_ERR_UNSUPPORTED outside
 * the limit: both before any launch. */
int avsr_ctc_align(const avsr_ctc_align_args* a, void* stream);

/* Attention rescoring of the CTC n-best (csrc/rescore.hip; the rule is this project's own).
 * avsr_seq_logprob: out[b * out_stride] = sum_{t < min(labels_len[b], L)} log_softmax(logits[b][t][:V])[labels[b][t]] -- the
 *   log-probability of a teacher-forced label row; labels_len[b] <= 0 gives 0.0.  logits [B][L][V] and labels [B][L] are read only (no
 *   d logits, no normaliser).  2 <= V <= 1024 (AVSR_ERR_UNSUPPORTED above), any remainder.  The labels are on the device and so not
 *   checked by the host: a label outside 0 .. V-1 contributes -inf and is never dereferenced.  out_stride >= 1: with
 *   out = s_att + k, out_stride = K, pass k fills column k of s_att [B][K]; no other element of out is written.
 * avsr_rescore_select: per utterance final[k] = s_att[b][k] + weight * s_ctc[b][k] (weight == 0: s_att[b][k], the product is not
 *   formed; product and sum rounded separately) for k < n[b] (clamped to 0 .. K), then order [B][K] = the k sorted by final descending,
 *   ties to the lower k, and final_out [B][K] in that order; slots >= n[b] get order -1 and final -inf.  1 <= K <= 64.
 * Both: one launch, no atomics, fixed reduction order -- bit-identical across launches.  AVSR_ERR_ARG (NULL pointer, B <= 0, L <= 0,
 * V < 2, out_stride < 1, K outside 1..64, weight negative or not finite) is decided on the host before any launch. */
int avsr_seq_logprob(const float* logits, const int32_t* labels, const int32_t* labels_len, int32_t B, int32_t L, int32_t V,
                     float* out, int64_t out_stride, void* stream);
int avsr_rescore_select(const float* s_att, const float* s_ctc, const int32_t* n, int32_t B, int32_t K, float weight,
                        int32_t* order, float* final_out, void* stream);

/* Post-loop helpers of the attention backward (see csrc/attention.hip). */
int avsr_attn_alpha_rows(float* scores, const float* dscores, const int32_t* len, const int32_t* steplen,
                         const float* g, float* rowdot, int32_t B, int32_t L, int32_t T, void* stream);
int avsr_bahdanau_dkeys(const float* keys, const float* pq, int64_t pq_sb, int64_t pq_sl, const float* dscores,
                        const float* v, const float* bq, const int32_t* len, float* dkeys, float* dv_part,
                        int32_t B, int32_t L, int32_t T, int32_t H, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Memory-bound helpers (csrc/elementwise.hip).  scratch buffers are caller-provided device floats. */
typedef struct avsr_transpose_job {
  const float* src;             /* [rows][cols] */
  float* dst;                   /* [cols][rows] */
  int32_t rows, cols;
} avsr_transpose_job;
/* jobs is a HOST array (copied into kernel arguments). */
int avsr_transpose(const avsr_transpose_job* jobs, int32_t n, void* stream);

/* out[f] = alpha * sum_r a[r][f] * (b ? b[r][f] : 1) + beta*out[f]   (bias / BN gradients); scratch >= 2*F floats */
int avsr_colsum(const avsr_mat* a, const avsr_mat* b, int32_t rows, int32_t F, float alpha, float beta, float* out,
                float* scratch, int64_t scratch_floats, void* stream);

/* tf.layers.batch_normalization(axis=-1, momentum=.99, eps=1e-3) over `rows` = B*T rows incl. padding
 * (avsr/encoder.py:44-50).  training=1: batch statistics + moving-average update; 0: moving statistics.
 * The input is rank 3, so TF 1.13 drops `fused=True` and the moving variance takes the BIASED batch variance.
 * moving_mean / moving_var may be NULL in training, both of them (no update: seq2seq.py:241-250 runs UPDATE_OPS only under
 * batch_normalisation=True); one without the other is AVSR_ERR_ARG at every door that updates them (avsr_batchnorm_fwd[_ex],
 * avsr_batchnorm_sync_apply, avsr_bn_finalize[_f64], avsr_conv3d_bn_finalize). */
int avsr_batchnorm_fwd(const float* x, float* y, int32_t rows, int32_t F, const float* gamma, const float* beta,
                       float* moving_mean, float* moving_var, float* save_mean, float* save_invstd, int32_t training,
                       float* scratch, int64_t scratch_floats, void* stream);
/* As avsr_batchnorm_fwd with explicit epsilon / momentum and an optional fused ReLU: batch_norm_relu of the lip-crop CNN
 * (avsr/video.py:4-14: epsilon 1e-5, momentum 0.98) and any tf.layers.batch_normalization(axis=-1) over [rows, F].
 * bessel=1 restates the fused kernel (rank-4 inputs): the moving variance takes var * rows / (rows - 1). */
int avsr_batchnorm_fwd_ex(const float* x, float* y, int32_t rows, int32_t F, const float* gamma, const float* beta,
                          float* moving_mean, float* moving_var, float* save_mean, float* save_invstd, int32_t training,
                          float eps, float momentum, int32_t relu, int32_t bessel, float* scratch, int64_t scratch_floats,
                          void* stream);
/* Sync batch-norm across data-parallel ranks (SURVEY 8(e) collective (3); statistics of encoder.py:44-50 over the
 * GLOBAL batch).  Three local phases; the host all-reduces sum_out (with the row count) after the first and sq_out
 * after the second:  (1) sum_out[f] = sum_rows x;  (2) mean_out = sum_global / total_rows[0], sq_out[f] = sum_rows
 * (x - mean)^2;  (3) invstd = rsqrt(sq_global / total + eps), moving-average update with the (biased, rank-3
 * non-fused path) global variance, y = (x - mean) * invstd * gamma + beta.  total_rows is a DEVICE float (the all-reduced count). */
int avsr_batchnorm_sync_sum(const float* x, int32_t rows, int32_t F, float* sum_out, float* scratch, int64_t scratch_floats,
                            void* stream);
int avsr_batchnorm_sync_sqsum(const float* x, int32_t rows, int32_t F, const float* sum_global, const float* total_rows,
                              float* mean_out, float* sq_out, float* scratch, int64_t scratch_floats, void* stream);
/* Data-parallel step, ONE small collective (the loss normalisers and the sync-batch-norm statistics fused):
 *   avsr_batchnorm_sync_moments: out64[0..F) = sum x, out64[F..2F) = sum x^2 over this rank's rows, fp64 (scratch 8-byte aligned; fp64
 *     partial rows of min(1024, ceil(rows/64)) blocks, 4*F floats each, the block count halved until they fit: at least 4*F floats); the caller packs them with its row count and the two loss normalisers into one fp64
 *     buffer and all-reduces that (sum);
 *   avsr_dp_sync_unpack: the reduced buffer -> dp_norm[0..1] and per stream mean / centred squares (sum x^2 - rows*mean^2, fp64) /
 *     rows as the float32 operands avsr_batchnorm_sync_apply and the loss kernels read.  encoder.py:44-50 statistics over the GLOBAL
 *     batch; no reference counterpart for the transport. */
int avsr_batchnorm_sync_moments(const float* x, int32_t rows, int32_t F, double* out64, float* scratch, int64_t scratch_floats, void* stream);
int avsr_dp_sync_unpack(const double* buf, float* dp_norm, int32_t nstream, const int32_t* off, const int32_t* F, float* const* mean,
                        float* const* sq, float* const* rows, void* stream);
int avsr_batchnorm_sync_apply(const float* x, float* y, int32_t rows, int32_t F, const float* gamma, const float* beta,
                              float* moving_mean, float* moving_var, const float* mean, const float* sq_global,
                              const float* total_rows, float* invstd_out, float eps, float momentum, int32_t relu, void* stream);
/* Gradient of batch normalisation with training statistics (tf.gradients through fused batch norm), optionally through
 * the ReLU after it: dy' = dy * [gamma*xhat + beta > 0];  dbeta = sum dy';  dgamma = sum dy'*xhat;
 * dx = gamma*invstd*(dy' - (sum dy' + xhat*sum dy'*xhat)/rows), written as dx = that + dx_beta*dx.  dx / dgamma / dbeta may
 * be NULL.  scratch: partial rows [blocks][2F] and the sums [2F] behind them; blocks = ceil(rows / 64), at most 2048 (the float4 kernels:
 * ceil(rows*F / 1024), at most 1024), fewer when the scratch holds fewer: any scratch of at least one partial row and the sums, 4F floats,
 * works, and one float less is AVSR_ERR_ARG.  The float4 kernels run when rows >= 4096, F divides 1024 and every operand is 16-byte
 * aligned; the sums are written straight to dgamma / dbeta when both are given and 16-byte aligned, else through the scratch. */
int avsr_batchnorm_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean,
                       const float* invstd, float* dx, float* dgamma, float* dbeta, int32_t rows, int32_t F, int32_t relu,
                       float dx_beta, float* scratch, int64_t scratch_floats, void* stream);
/* Read-only plan query of the normalisations whose launch geometry depends on their arguments: decided by the same host function the
 * entry points launch by -- nothing is dereferenced or launched, no HIP call is made (runs without a GPU).
 *   op: AVSR_BN_PLAN_FWD avsr_batchnorm_fwd(_ex), _BWD avsr_batchnorm_bwd, _SYNC_SUM / _SYNC_SQSUM / _SYNC_MOMENTS the avsr_batchnorm_sync_*
 *       entries, _BWD_STAGE1 avsr_bn_bwd_stage1 and _BWD_APPLY avsr_bn_bwd_apply (rows and F = C of their maps; no scratch).
 *   flags (avsr_batchnorm_bwd only): what the call derives from its pointers -- _ALIGNED: x, dy, dx (when given), gamma, beta, mean, invstd
 *       and scratch all 16-byte aligned; _DIRECT: dgamma and dbeta both given and 16-byte aligned; _DX: dx given.
 *   out: blocks = workgroups of the partial-sum launch(es) (= partial rows; stage 1: *nparts), rows_per_block (0 for the float4 kernels,
 *       which stride the flat map), G = row sub-groups of a block (256 / F below 256 columns, else 1; stage 1: its row lanes
 *       256 / (C/4); 0 for avsr_bn_bwd_apply), vec = the float4 kernels, direct = the sums go straight to dgamma / dbeta, apply_grid =
 *       workgroups of the pass that writes y / dx (0: none), err = the AVSR_* code the call would return on these arguments.
 * Returns err. */
#define AVSR_BN_PLAN_FWD 0
#define AVSR_BN_PLAN_BWD 1
#define AVSR_BN_PLAN_SYNC_SUM 2
#define AVSR_BN_PLAN_SYNC_SQSUM 3
#define AVSR_BN_PLAN_SYNC_MOMENTS 4
#define AVSR_BN_PLAN_BWD_STAGE1 5
#define AVSR_BN_PLAN_BWD_APPLY 6
#define AVSR_BN_PLAN_ALIGNED 1
#define AVSR_BN_PLAN_DIRECT 2
#define AVSR_BN_PLAN_DX 4
typedef struct avsr_bn_plan {
  int32_t blocks, rows_per_block, G, vec, direct, apply_grid, err, pad_;
} avsr_bn_plan;
int avsr_batchnorm_plan(int32_t op, int64_t rows, int32_t F, int64_t scratch_floats, int32_t flags, avsr_bn_plan* out);

/* ---- lip-crop CNN front-end (avsr/video.py:143-195 resnet_cnn): convolutions are im2col + avsr_gemm ----
 * im2col over NHWC maps with TF "SAME"/"VALID" geometry given explicitly: col[(n,ho,wo)][(i,j,c)] =
 * x[n, ho*stride - pad_t + i, wo*stride - pad_l + j, c] (0 outside); the TF kernel [kh,kw,cin,cout] is the GEMM's
 * [kh*kw*cin, cout] operand as stored.  col2im is its adjoint (gather form, deterministic): dx = col2im(dcol) + beta*dx. */
int avsr_im2col(const float* x, float* col, int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride,
                int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, void* stream);
int avsr_col2im(const float* dcol, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride,
                int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, float beta, void* stream);
/* Direct 3x3 convolutions on NHWC maps for the shallow layers of the lip CNN (cin*cout <= 1024, cout in {4, 8, 16, 32}, cin in {1..3, 4n};
 * avsr_conv3x3_supported), on the fp32 VALU (csrc/conv_direct.hip) -- these entry points never run the MFMA kernels below:
 * the same tf.layers.conv2d(3x3, SAME) and its gradients as the im2col + avsr_gemm route, without the 9x operand.
 *   avsr_conv3x3(flip=0): y = conv(x, w[3,3,Ci,Co]) + bias (+ beta*y).
 *   avsr_conv3x3(flip=1): stride-1 data gradient: x = dy [.,Ci = cout], y = dx [.,Co = cin], w = the FORWARD kernel [3,3,Co,Ci].
 *   avsr_conv3x3_bwd_data_s2: data gradient of a stride-2 conv (dx [N,H,W,Ci] from dy [N,Ho,Wo,Co]).
 *   avsr_conv3x3_bwd_weight: dw[3,3,Ci,Co] = beta*dw + sum x (x) dy; Co in {4, 8, 16, 32}; scratch >= ceil(N/4) * (256/(9*Ci)) * 9*Ci*Co floats (fewer blocks if smaller). */
int avsr_conv3x3_supported(int32_t Ci, int32_t Co, int32_t H, int32_t W);
/* The frame-resident MFMA kernels (csrc/conv_mfma.hip, conv_wgrad.hip: whole frames staged in LDS, implicit GEMM on
 * v_mfma_f32_16x16x4_f32) are reached through the descriptor API below and nowhere else.  The caller picks the tier per layer:
 * avsr_conv_supported -> the descriptor API; else k == 3 and avsr_conv3x3_supported -> the direct kernels above; else im2col + avsr_gemm.
 * This switch (default 1): 0 makes avsr_conv_supported and its siblings answer 0 and the descriptor entry points return
 * AVSR_ERR_UNSUPPORTED, which sends every layer to the other two tiers (A/B timing, tests). */
int avsr_conv_set_mfma(int32_t on);
/* Frame-resident MFMA convolutions of the lip CNN through ONE descriptor (csrc/conv_mfma.hip; tf.layers.conv2d of video.py:18-30 with
 * k = 1 (the stride-2 projection shortcut, video.py:70-75) or 3, stride 1 / 2, Ci in {1..3, 4n}, Co = 4n <= 64):
 *   bn_scale / bn_shift (may be NULL): the input map is the PRE-normalisation map x and the kernels apply the consumer-side
 *     batch_norm_relu (video.py:4-14) max(x*scale[c] + shift[c], 0) while staging frames in LDS -- the normalised map is never
 *     written (forward and weight gradient; the zero padding is applied after the BN-ReLU, as in the graph).
 *   avsr_conv_fwd: y = conv(x) + bias (+ res: the residual of video.py:84 `tf.add`; res_scale/res_shift != NULL: the residual is
 *     itself a lazily normalised map); stats != NULL (>= 512*2*Co floats): per-workgroup partial sums / sums of squares of y
 *     [*nparts][2*Co] for the batch norm that consumes y; avsr_bn_finalize merges them in fp64 into mean / inverse std (+ the
 *     moving averages with the Bessel-corrected variance of the fused rank-4 TF kernel) and the scale / shift vectors above.
 *   avsr_conv_bwd_data: dx = beta*dx + conv_transpose(dy); a stride-2 1x1 kernel reaches only the even pixels, so beta must be 1
 *     (any other beta: AVSR_ERR_UNSUPPORTED before anything is launched).
 *   avsr_conv_bwd_weight: dw = beta*dw + sum x (x) dy, dbias (may be NULL) = beta*dbias + column sums of dy (same pass over dy);
 *     scratch >= 256 * (k*k*Ci*Co + Co) floats.
 * AVSR_ERR_UNSUPPORTED (-3) for shapes outside the kernels' register / LDS budget (avsr_conv_supported == 0): the caller then uses
 * the direct kernels or im2col + avsr_gemm for the whole layer. */
typedef struct avsr_conv_desc {
  int32_t N, H, W, Ci, Co, k, stride, pad_t, pad_l, Ho, Wo, pad_;
  const float* bn_scale;
  const float* bn_shift;
} avsr_conv_desc;
int avsr_conv_supported(const avsr_conv_desc* c);
int avsr_conv_fwd(const avsr_conv_desc* c, const float* x, const float* w, const float* bias, const float* res, const float* res_scale,
                  const float* res_shift, float* y, float* stats, int32_t* nparts, void* stream);
int avsr_conv_bwd_data(const avsr_conv_desc* c, const float* dy, const float* w, float* dx, float beta, void* stream);
int avsr_conv_bwd_weight(const avsr_conv_desc* c, const float* x, const float* dy, float* dw, float* dbias, float beta, float* scratch,
                         int64_t scratch_floats, void* stream);
/* Data gradient with the fused forms of the lip CNN's backward pass (avsr/video.py:4-14 batch_norm_relu, :57-88 residual blocks):
 *   acc (may be NULL): dx = beta*acc + conv_transpose(dy) -- the gradient arriving over a residual connection is read where it lies
 *     instead of being copied into dx first;
 *   bn_x != NULL: dx is the gradient of y = relu(bn_x*bn_scale + bn_shift) (the lazily normalised input of the forward conv): the
 *     epilogue writes dz = dx * [y > 0] and the per-workgroup partial sums [*nparts][2*Ci] of (dz | dz*bn_x) into stats
 *     (>= 512*2*Ci floats) -- stage 1 of tf.layers.batch_normalization's backward without its own two-map pass;
 *   avsr_bn_bwd_finalize: d beta / d gamma (grad_beta = 1 accumulates) and the three coefficient vectors k [3*C];
 *   avsr_bn_bwd_apply: dx = beta*dx + k1*dz + k2*x + k3  ==  gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)).
 * AVSR_ERR_UNSUPPORTED where the data gradient needs several launches over disjoint pixel classes (avsr_conv_bwd_data_bn_supported == 0). */
int avsr_conv_bwd_data_bn(const avsr_conv_desc* c, const float* dy, const float* w, float* dx, float beta, const float* acc,
                          const float* bn_x, const float* bn_scale, const float* bn_shift, float* stats, int32_t* nparts, void* stream);
int avsr_conv_bwd_data_bn_supported(const avsr_conv_desc* c);
/* Weight (+ bias) gradient of a convolution whose OUTPUT y feeds a batch norm (video.py:4-14), with that batch norm's backward folded into
 * the operand fetch: the gradient of y, gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)) = k[0..C)*dz + k[C..2C)*y + k[2C..3C)
 * (avsr_bn_bwd_finalize's coefficient vectors), is evaluated where the kernel fetches it.  dx_out == NULL (a layer with no data gradient:
 * layer 0 of resnet_cnn, whose input are the lip crops): it is never stored; dx_out != NULL: every element is also written there by the
 * one lane that fetched it, for the layer's data gradient (issued after this call) -- either way the avsr_bn_bwd_apply pass over three
 * maps disappears.  avsr_conv_bwd_weight_bn_supported (single-launch forms only): 0 = use avsr_bn_bwd_apply + avsr_conv_bwd_weight. */
int avsr_conv_bwd_weight_bn(const avsr_conv_desc* c, const float* x, const float* dz, const float* y, const float* k, float* dx_out,
                            float* dw, float* dbias, float beta, float* scratch, int64_t scratch_floats, void* stream);
int avsr_conv_bwd_weight_bn_supported(const avsr_conv_desc* c);
/* Read-only plan query: the kernel launches one call of the descriptor API WOULD make, decided by the same host code on its dry path --
 * no pointer is dereferenced, nothing is launched, no HIP call is made (runs without a GPU).  op: 0 avsr_conv_fwd, 1 avsr_conv_bwd_data
 * (+ _bn), 2 avsr_conv_bwd_weight (+ _bn).  flags: the optional operands the real call would pass (AVSR_CONV_PLAN_*; c->bn_scale != NULL
 * stands for the BN-ReLU loader); scratch_floats: the weight gradient's scratch.  Writes up to `cap` records, one per launch in launch
 * order, and returns the number of launches (which may exceed cap), or the AVSR_ERR_* code the real call would return.
 *   kernel 0: conv_gen_kernel<m = MAXCH, ch4, ep>      1: conv_q4_kernel<m = NTAP, ntc = C4T, ch4, ep>
 *   kernel 2: conv_wgrad_kernel<m = MT, ntc = NTC, ch4, rs, fold>
 *   nsp: destination pixels per product row (data path; the pixel-pair weight gradient reports 2), ntap: taps of this launch, t0: its first
 *   tap, F: frames per pass, grid: workgroups, CsP: floats per staged pixel in LDS, lds_bytes: dynamic LDS, slab: floats per workgroup
 *   partial (weight gradient; includes the bias columns where this launch computes them). */
#define AVSR_CONV_PLAN_BIAS 1
#define AVSR_CONV_PLAN_RES 2
#define AVSR_CONV_PLAN_STATS 4
#define AVSR_CONV_PLAN_BETA 8
#define AVSR_CONV_PLAN_ACC 16
#define AVSR_CONV_PLAN_BNB 32
#define AVSR_CONV_PLAN_FOLD 64
#define AVSR_CONV_PLAN_FOLD_DX 128
#define AVSR_CONV_PLAN_DBIAS 256
typedef struct avsr_conv_launch {
  int32_t kernel, m, ntc, ch4, rs, fold, ep, nsp;
  int32_t ntap, t0, F, grid, CsP, lds_bytes, slab, pad_;
} avsr_conv_launch;
int avsr_conv_plan(const avsr_conv_desc* c, int32_t op, int32_t flags, int64_t scratch_floats, avsr_conv_launch* out, int32_t cap);
int avsr_bn_bwd_finalize(const float* part, int32_t nparts, int32_t C, int64_t count, const float* mean, const float* invstd,
                         const float* gamma, float* dgamma, float* dbeta, float grad_beta, float* k, void* stream);
int avsr_bn_bwd_apply(const float* dz, const float* x, const float* k, float* dx, int64_t rows, int32_t C, float beta, void* stream);
/* Stage 1 of the batch-norm backward as a pass of its own, for a batch norm whose output gradient several launches assembled (no single
 * epilogue to fuse it into): dz = dy * [scale*x + shift > 0] (scale == NULL: [y > 0]), part [*nparts <= 512][2*C] = (sum dz | sum dz*x) --
 * the layout avsr_bn_bwd_finalize / avsr_bn_partials_f64 read.  dz may alias dy; C % 4 == 0, C <= 1024.  Used by sync_cnn_bn for the
 * layers avsr_conv_bwd_data_bn does not cover (video.py:4-14 differentiated over the global batch). */
int avsr_bn_bwd_stage1(const float* dy, const float* x, const float* scale, const float* shift, const float* y, float* dz, int64_t rows,
                       int32_t C, float* part, int32_t* nparts, void* stream);
int avsr_bn_finalize(const float* part, int32_t nparts, int32_t C, int64_t count, float eps, float momentum, float* mean, float* invstd,
                     float* mov_mean, float* mov_var, const float* gamma, const float* beta, float* scale, float* shift, void* stream);
/* The same two finalisations from GLOBAL statistics under data parallelism (video.py:4-14 `tf.layers.batch_normalization` over the whole
 * batch; opt-in, DataParallelTrainer(sync_cnn_bn=True)): avsr_bn_partials_f64 merges a convolution's partial rows into fp64 sums
 * out64 [2*C]; the caller all-reduces [sums | rows per channel] over the ranks; avsr_bn_finalize_f64 reads sums [2*C + 1] (count last);
 * avsr_bn_bwd_finalize_f64 takes this rank's sums `local` [2*C] for d gamma / d beta (the gradient all-reduce adds the ranks' shares)
 * and the all-reduced `global` [2*C + 1] for the coefficient vectors k [3*C]. */
int avsr_bn_partials_f64(const float* part, int32_t nparts, int32_t C, double* out64, void* stream);
int avsr_bn_finalize_f64(const double* sums, int32_t C, float eps, float momentum, float* mean, float* invstd, float* mov_mean,
                         float* mov_var, const float* gamma, const float* beta, float* scale, float* shift, void* stream);
int avsr_bn_bwd_finalize_f64(const double* local, const double* global, int32_t C, const float* mean, const float* invstd,
                             const float* gamma, float* dgamma, float* dbeta, float grad_beta, float* k, void* stream);
/* scale = gamma * rsqrt(moving_variance + eps), shift = beta - moving_mean * scale: the evaluation graph's batch norm as the
 * loader-applied affine of avsr_conv_desc (no normalised map is written in evaluation either). */
int avsr_bn_eval_affine(const float* gamma, const float* beta, const float* mov_mean, const float* mov_var, float eps, float* scale,
                        float* shift, int32_t C, void* stream);
int avsr_batchnorm_apply(const float* x, float* y, int32_t rows, int32_t F, const float* gamma, const float* beta, const float* mean,
                         const float* invstd, int32_t relu, void* stream);
int avsr_conv3x3(const float* x, const float* w, const float* bias, float* y, int32_t N, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                 int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, int32_t flip, float beta, void* stream);
int avsr_conv3x3_bwd_data_s2(const float* dy, const float* w, float* dx, int32_t N, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                             int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, float beta, void* stream);
int avsr_conv3x3_bwd_weight(const float* x, const float* dy, float* dw, int32_t N, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                            int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, float beta, float* scratch,
                            int64_t scratch_floats, void* stream);
/* ---- spatio-temporal lip front-end (avsr/video.py:34-46 conv3d_wrapper, :92-105 residual_block_3d, :198-222 conv3d_cnn) ----
 * tf.layers.conv3d(use_bias=False) over NDHWC maps x [B, T, H, W, Ci] -> y [B, T, Ho, Wo, Co] with kernel w [kt, kh, kw, Ci, Co] (TF
 * layout, = the [kt*kh*kw*Ci, Co] GEMM operand), spatial stride 1 / 2, temporal stride 1; pad_f / pad_t / pad_l = zero frames / rows /
 * columns before the map (TF SAME: the odd one goes after).  Implicit GEMMs on v_mfma_f32_16x16x4_f32 (csrc/conv3d.hip).
 *   scale / shift (may be NULL): the kernels read the source of the forward and of the weight gradient as max(x*scale[c] + shift[c], 0)
 *     (relu = 1: the consumer-side batch_norm_relu of video.py:4-14; the normalised map is never written) or x*scale + shift (relu = 0:
 *     layer 0's `inputs * 2 - 1`); the zero padding comes after the transform.
 *   avsr_conv3d_fwd: y = conv(x) (+ res, itself read as max(res*res_scale + res_shift, 0) when res_scale != NULL); stats != NULL
 *     (>= 512*2*Co floats): per-workgroup partial sums / sums of squares of y [*nparts][2*Co] for the batch norm that consumes y.
 *   avsr_conv3d_bwd_data: dx = beta*dx + conv_transpose(dy) (every dx element is written).
 *   avsr_conv3d_bwd_weight: dw = beta*dw + sum x (x) dy; scratch >= avsr_conv3d_wgrad_scratch_floats(c) floats (deterministic split).
 *   avsr_conv3d_bn_finalize: avsr_bn_finalize for the NON-fused batch norm of a rank-5 map (TF 1.13 keeps fused=True for rank 4 only):
 *     the moving variance takes the biased batch variance.
 * Covered: kt, kh, kw <= 3, Ci in {1..3, 4n <= 128}, Co = 4n <= 128 (avsr_conv3d_supported); otherwise AVSR_ERR_UNSUPPORTED (-3). */
typedef struct avsr_conv3d_desc {
  int32_t B, T, H, W, Ci, Co;
  int32_t kt, kh, kw, stride;
  int32_t pad_f, pad_t, pad_l, Ho, Wo, relu;
  const float* scale;
  const float* shift;
} avsr_conv3d_desc;
int avsr_conv3d_supported(const avsr_conv3d_desc* c);
int64_t avsr_conv3d_wgrad_scratch_floats(const avsr_conv3d_desc* c);
int avsr_conv3d_fwd(const avsr_conv3d_desc* c, const float* x, const float* w, const float* res, const float* res_scale, const float* res_shift,
                    float* y, float* stats, int32_t* nparts, void* stream);
int avsr_conv3d_bwd_data(const avsr_conv3d_desc* c, const float* dy, const float* w, float* dx, float beta, void* stream);
int avsr_conv3d_bwd_weight(const avsr_conv3d_desc* c, const float* x, const float* dy, float* dw, float beta, float* scratch,
                           int64_t scratch_floats, void* stream);
int avsr_conv3d_bn_finalize(const float* part, int32_t nparts, int32_t C, int64_t count, float eps, float momentum, float* mean,
                            float* invstd, float* mov_mean, float* mov_var, const float* gamma, const float* beta, float* scale,
                            float* shift, void* stream);
/* ---- waveform audio front-end (avsr/audio.py:7-41 compute_stfts / compute_log_mel_spectrograms, avsr/dataset_writer.py:549-551
 * _stack_features): wav [B, N] (fp32 samples, wav_len[b] valid ones) -> out [B, T_out, F] in one launch (csrc/audio_frontend.hip).
 *   frames_b = 1 + (n - frame_length) / frame_step (no pad_end); frame t = wav[frame_step*t ...] * hann, zero-padded to fft_length,
 *   real FFT, magnitude, mel[m] = sum_c mel_w[mel_ptr[m] + c] * |X[mel_lo[m] + c]| (c < mel_cnt[m]: the non-zero bins of filter m are
 *   contiguous), log(mel + 1e-6); out row r = frames stride*r .. stride*r + window - 1 side by side, rows_b = (frames_b - window) /
 *   stride + 1.  Rows >= rows_b and columns >= num_mel_bins*window (F may be wider: the consumer's padded row) are written as zeros;
 *   out_len[b] = rows_b (may be NULL).  hann [frame_length], twiddle [fft_length] pairs (cos, -sin)(2 pi k / fft_length), mel_w
 *   [mel_nnz]: computed in fp64 by the caller.  Launches one kernel and nothing else (safe under stream capture).
 * Covered (avsr_logmel_supported): fft_length == 512 >= frame_length, num_mel_bins <= 128, stride <= window <= 16; otherwise
 * AVSR_ERR_UNSUPPORTED (-3). */
typedef struct avsr_logmel_args {
  int32_t B, N, T_out, F;
  int32_t frame_length, frame_step, fft_length, num_mel_bins;
  int32_t window, stride, mel_nnz, pad_;
  const float* wav;
  const int32_t* wav_len;
  const float* hann;
  const float* twiddle;
  const int32_t* mel_lo;
  const int32_t* mel_cnt;
  const int32_t* mel_ptr;
  const float* mel_w;
  float* out;
  int32_t* out_len;
} avsr_logmel_args;
int avsr_logmel_supported(int32_t frame_length, int32_t fft_length, int32_t num_mel_bins, int32_t window, int32_t stride);
int avsr_logmel_fwd(const avsr_logmel_args* a, void* stream);
/* ---- SpecAugment on an encoder's input (spec_augment; not in the reference; csrc/specaugment.hip; the rule is INTEGRATION.md
 * section 8).  x [B, T, F_in] with row stride ld (utterances T * ld apart) -> y [B, T, F] contiguous, F >= F_in, y != x.  EVERY element
 * of y is written: unmasked elements are copied bit for bit, columns >= F_in and rows >= n_b = clamp(len[b], 0, T) are zero; x is
 * never written.  All arithmetic of the draw is uint32, h(i) = hash_u32(seed[0], STREAM, i) (seed: DEVICE word, the step's key):
 *   time mask k < time_masks   cap = min(time_width, (n_b * ratio_q16) >> 16), w = h((b*64 + k)*2) % (cap + 1),
 *                              t0 = h((b*64 + k)*2 + 1) % (n_b - w + 1): rows t0 <= t < t0 + w
 *   band k < freq_masks        cap = min(freq_width, P), P = freq_bins, w and f0 likewise with P for n_b: columns with
 *                              f0 <= c % P < f0 + w (the same bin of every stacked frame)
 *   STREAM                     video == 0: 200 for the bands, 201 for the time masks; video == 1 (time masks only): 202 -- above every
 *                              dropout / sampling stream (cell id * 4 + kind, cell ids up to 43)
 *   fill                       mean_fill == 0: 0.  mean_fill == 1: the utterance's own mean of that column over its n_b rows of x
 *                              (per-chunk fp32 partial sums, added in chunk order in fp64, rounded once): masks are a plain union
 * ws: avsr_spec_augment_ws_floats(B, T, F_in) floats, 16-byte aligned (mean_fill == 1 only; may be NULL otherwise).  One launch for
 * mean_fill == 0, three for 1; no atomics (two launches on the same inputs are bit-identical), no host read, no memset / memcpy:
 * safe under stream capture.  Covered (avsr_spec_augment_supported): T <= 65535 (the n_b * ratio_q16 product), at most 8 masks of a
 * kind, B <= 65535, B * T * F < 2^31; otherwise AVSR_ERR_UNSUPPORTED (-3).  ratio_q16 = round(ratio * 65536) in [0, 65536]. */
#define AVSR_SPEC_AUGMENT_MAX_MASKS 8
#define AVSR_SPEC_AUGMENT_MAX_T 65535
typedef struct avsr_spec_augment_args {
  int32_t B, T, F_in, F;
  int32_t freq_masks, freq_width, freq_bins, time_masks;
  int32_t time_width, ratio_q16, video, mean_fill;
  int64_t ld;
  const float* x;
  const int32_t* len;
  const int32_t* seed;
  float* y;
  float* ws;
  int64_t ws_floats;
} avsr_spec_augment_args;
int avsr_spec_augment_supported(int32_t B, int32_t T, int32_t F, int32_t freq_masks, int32_t time_masks);
int64_t avsr_spec_augment_ws_floats(int32_t B, int32_t T, int32_t F_in);
int avsr_spec_augment(const avsr_spec_augment_args* a, void* stream);
/* ---- Lip-crop augmentation (video_augment; not in the reference; csrc/video_augment.hip; the rule is INTEGRATION.md section 8).
 * x [B, T, H, W, C] contiguous -> y of the same shape, y != x.  EVERY element of y is written, frames t >= n_b = clamp(len[b], 0, T) as
 * zeros; x is never written.  All draws are uint32 and PER UTTERANCE, h_s(i) = hash_u32(seed[0], s, i) (seed: DEVICE word, the step's
 * key), streams 203 (geometry) and 204 (photometric), u(h) = (h >> 8) * 2^-24:
 *   flip    iff (h_203(4b) >> 8) < flip_q24, flip_q24 = round(flip * 2^24) in [0, 2^24]
 *   shift   dx = h_203(4b+1) % (2S+1) - S, dy = h_203(4b+2) % (2S+1) - S, S = max_shift
 *   source  of output pixel (i, j, c) of frame t < n_b: x[t, ii, flip ? W-1-jj : jj, c] with jj = clamp(j - dx, 0, W-1),
 *           ii = clamp(i - dy, 0, H-1): the flip first, the shift second, edges replicated
 *   cf = 1 + contrast * (2 u(h_204(2b)) - 1), d = brightness * (2 u(h_204(2b+1)) - 1), every fp32 operation rounded on its own
 *   contrast > 0: y = cf * (v - m_c) + (m_c + d), m_c the utterance's mean of channel c over its n_b frames of x (0 when n_b = 0):
 *           fp32 partial sums of fc * H * W terms per chunk of fc frames, added in chunk order in fp64, / (n_b H W), rounded once;
 *           fc = max(4, ceil(T / min(128, ceil(1024 / B))) rounded down to a multiple of 4)
 *   contrast == 0, brightness > 0: y = v + d.  Both 0: bit copies.  No clipping.
 * ws: avsr_video_augment_ws_floats(B, T, H, W, C) floats, 16-byte aligned (contrast > 0 only; may be NULL otherwise): the partial sums
 * [B][ceil(T / fc)][C], then the means [B][C].  One launch, or three with contrast > 0; no atomics (two launches on the same inputs are
 * bit-identical), no host read, no memset / memcpy: safe under stream capture.  Covered (avsr_video_augment_supported): T <= 65535,
 * B <= 65535, C <= 64, 0 <= max_shift < min(H, W), B * T * H * W * C < 2^31; otherwise AVSR_ERR_UNSUPPORTED (-3).  contrast in [0, 1),
 * brightness finite and >= 0, else AVSR_ERR_ARG. */
#define AVSR_VIDEO_AUGMENT_MAX_T 65535
#define AVSR_VIDEO_AUGMENT_MAX_C 64
typedef struct avsr_video_augment_args {
  int32_t B, T, H, W;
  int32_t C, max_shift, flip_q24, pad_;
  float contrast, brightness;
  const float* x;
  const int32_t* len;
  const int32_t* seed;
  float* y;
  float* ws;
  int64_t ws_floats;
} avsr_video_augment_args;
int avsr_video_augment_supported(int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t max_shift);
int64_t avsr_video_augment_ws_floats(int32_t B, int32_t T, int32_t H, int32_t W, int32_t C);
int avsr_video_augment(const avsr_video_augment_args* a, void* stream);
/* ---- CTC auxiliary loss on an encoder's outputs (use_ctc; not in the reference; csrc/ctc.hip).  z [B*T, C] with row stride ld are the
 * head's logits, C = vocab_size + 1 and the BLANK IS CLASS C - 1 (tf.nn.ctc_loss's convention); columns >= C of a wider row are never
 * read or written.  Utterance b: target labels[b, :U_b] with U_b = max(min(labels_len[b], L) - 1, 0) (the label row without its EOS),
 * T_b = min(max(in_len[b], 0), T) frames.
 *   nll[b]      = -log p(target_b | log_softmax(z[b, :T_b])), the standard CTC forward-backward recursion
 *   status[b]   = 1, or 0 when the utterance has no valid alignment (T_b < U_b + adjacent equal label pairs, T_b == 0, or a label
 *                 outside [0, C - 1)): then nll[b] = 0 and its rows of dz are zero (torch's zero_infinity=True)
 *   utt_loss[b] = weight * nll[b] / (denom[0] + 1e-12)          denom: DEVICE scalar, the sequence loss's own normaliser
 *   dz[b, t, k] = weight / denom * (softmax(z)[b, t, k] - occupancy[b, t, k]) for t < T_b, exactly 0 for t >= T_b; layout of z; dz != z
 * ws: avsr_ctc_ws_floats(B, T, L) floats of scratch (alpha over all T frames lives there, so T is not bounded by on-chip memory).
 * One launch, one workgroup per utterance, no atomics (two launches on the same inputs are bit-identical), no host read, no
 * memset / memcpy: safe under stream capture.  L and C up to 1024, otherwise AVSR_ERR_UNSUPPORTED (-3). */
typedef struct avsr_ctc_args {
  int32_t B, T, L, C;
  int64_t ld;
  const float* z;
  const int32_t* labels;
  const int32_t* labels_len;
  const int32_t* in_len;
  const float* denom;
  float weight;
  int32_t pad_;
  float* nll;
  int32_t* status;
  float* utt_loss;
  float* dz;
  float* ws;
  int64_t ws_floats;
} avsr_ctc_args;
int avsr_ctc_loss(const avsr_ctc_args* a, void* stream);
int64_t avsr_ctc_ws_floats(int32_t B, int32_t T, int32_t L);
/* ids[b*T + t] = argmax_k z[b, t, k] over the C classes (the lowest index wins a tie) for t < T_b, -1 for t >= T_b: the CTC best path
 * before the host collapses repeats and drops blanks. */
int avsr_ctc_best_path(const float* z, int64_t ld, const int32_t* in_len, int32_t B, int32_t T, int32_t C, int32_t* ids, void* stream);
/* y = max(x, 0);  dx = dy * [y > 0];  out = a + b (tf.nn.relu / residual tf.add of video.py) */
int avsr_relu(const float* x, float* y, int64_t n, void* stream);
int avsr_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);
int avsr_add(const float* a, const float* b, float* out, int64_t n, void* stream);
/* tf.nn.selu and its gradient (dz = dy * selu'(z)): the optional input Dense stack of the encoders (encoder.py:148-171) */
int avsr_selu(const float* z, float* y, int64_t n, void* stream);
int avsr_selu_bwd(const float* z, const float* dy, float* dz, int64_t n, void* stream);

int avsr_batchnorm_xhat(const float* x, const float* mean, const float* invstd, float* xhat, int32_t rows, int32_t F,
                        void* stream);

/* embedding_lookup(labels_padded_GO) (avsr/decoder_unimodal.py:66-68, :170): fed[b][l] = l ? labels[b][l-1] : GO,
 * out[b][l][:] = emb[fed[b][l]] for l < n_steps (n_steps = L: all; 1: only the GO column).  Gradient: demb[v][:] = sum of
 * dx rows whose fed token is v (deterministic order; scratch >= ceil(B*L/256) * V * E floats). */
int avsr_embed_labels(const float* emb, const int32_t* labels, int32_t go_id, float* out, int32_t* fed, int32_t B,
                      int32_t L, int32_t E, int32_t n_steps, void* stream);
int avsr_embed_grad(const float* dx, const int32_t* fed, float* demb, int32_t B, int32_t L, int32_t E, int32_t V,
                    float* scratch, int64_t scratch_floats, void* stream);

/* y[r][c] = (accumulate ? y[r][c] : 0) + x[r][c] * mask(r, c) / keep for r < rows, c < cols;
 * mask index = r * idx_width + idx_coff + c (r = b*T + t), stream as in avsr_rnn_stack.  Used for input dropout of
 * hoisted operands and for the matching gradients.  seed NULL or keep >= 1 copies. */
int avsr_dropout_rows(const avsr_mat* x, const avsr_mat* y, int32_t rows, int32_t cols, const int32_t* seed,
                      int32_t stream_id, float keep, int32_t idx_width, int32_t idx_coff, int32_t accumulate, void* stream);

/* seq2seq.sequence_loss (avsr/seq2seq.py:165-171): row_loss[b*L+l] = CE * mask / (sum(mask) + 1e-12) and
 * d loss / d logits.  denom[0] = sum(mask) is computed when compute_denom=1 (single GPU) or supplied
 * (data parallel: all-reduced by the caller).  Logit rows of finished steps are zeroed in place
 * (dynamic_decode impute_finished=True, avsr/decoder_unimodal.py:344-350). */
int avsr_seq_loss(float* logits, const int32_t* labels, const int32_t* labels_len, float* denom,
                  int32_t compute_denom, float* row_loss, float* dlogits, int32_t B, int32_t L, int32_t V, void* stream);
/* The non-default per-step losses of avsr/seq2seq.py:147-163.  loss_fun: 0 sparse softmax cross-entropy (= avsr_seq_loss);
 * 1 label smoothing through tf.losses.softmax_cross_entropy (avsr/devel.py:54-61), whose default reduction turns the
 * sequence loss into the mean over ALL B*L rows -- denom is then the row count (compute_denom=1 sets B*L), padding rows
 * contribute log V each and no gradient; 2 focal_loss (gamma 2) and 3 mc_loss on the clipped softmax (avsr/devel.py:12-51). */
int avsr_seq_loss_fun(float* logits, const int32_t* labels, const int32_t* labels_len, float* denom, int32_t compute_denom,
                      float* row_loss, float* dlogits, int32_t B, int32_t L, int32_t V, int32_t loss_fun,
                      float label_smoothing, void* stream);

/* Per-utterance average of the step losses avsr_seq_loss left in row_loss (which carry the 1/denom factor):
 * out[b] = sum_l CE[b,l] w[b,l] / (sum_l w[b,l] + 1e-12) -- the language model's `average_log_likelihoods`
 * (avsr/lm.py:390-401: sequence_loss(average_across_batch=False, average_across_timesteps=True)). */
int avsr_seq_loss_per_utterance(const float* row_loss, const int32_t* labels_len, const float* denom, float* out, int32_t B,
                                int32_t L, void* stream);
/* tf.contrib.layers.instance_norm on the [B,T,F] encoder inputs (avsr/encoder.py:51-55): mean / variance over the T axis per
 * (utterance, feature), zero padding included, epsilon 1e-6, per-feature gamma / beta.  mean_out / invstd_out [B][F].
 * Backward: dx (may alias dy) and the per-utterance sums dgamma_part / dbeta_part [B][F] (column-sum them over B). */
int avsr_instnorm_fwd(const float* x, float* y, int32_t B, int32_t T, int32_t F, const float* gamma, const float* beta,
                      float* mean_out, float* invstd_out, float eps, void* stream);
int avsr_instnorm_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* invstd, float* dx,
                      float* dgamma_part, float* dbeta_part, int32_t B, int32_t T, int32_t F, void* stream);
/* tf.contrib.rnn.HighwayWrapper around an encoder cell (`highway_encoder=True`, avsr/cells.py:89-90), applied to a whole layer:
 * carry = sigmoid(carry_pre), y = x * carry + h * (1 - carry) for t < len[b], zero past the utterance.  x = the layer's raw
 * input, h = the cell's emitted output, carry_pre = x W_c + b_c (avsr_gemm).  Operands are [B*T, H] row views (avsr_mat with
 * T = rows per utterance).  Backward: dh = dy (1 - carry), dcarry_pre = dy (x - h) carry (1 - carry), dx (+)= dy carry. */
int avsr_highway_fwd(const avsr_mat* x, const avsr_mat* h, const avsr_mat* carry_pre, const avsr_mat* y, const int32_t* len,
                     int32_t B, int32_t T, int32_t H, void* stream);
int avsr_highway_bwd(const avsr_mat* x, const avsr_mat* h, const avsr_mat* carry_pre, const avsr_mat* dy, const avsr_mat* dh,
                     const avsr_mat* dcarry_pre, const avsr_mat* dx, const int32_t* len, int32_t B, int32_t T, int32_t H,
                     int32_t accumulate_dx, void* stream);
/* dst = src / dst = 0 over n 32-bit words, as KERNELS on the given stream.  The engine (and the host code around captured graphs)
 * never enqueues hipMemsetAsync / hipMemcpyAsync: as graph memset / memcpy nodes they were not reliably ordered against their
 * neighbours on ROCm 7.0.  No reference counterpart. */
int avsr_copy_words(void* dst, const void* src, int64_t n_words, void* stream);
int avsr_zero_words(void* dst, int64_t n_words, void* stream);
/* Any number of buffers zeroed eight per launch (the gradient buffers at the start of the backward pass), and
 * out[0] = a[0] + b on the device (the step's dropout / sampling RNG key = global step + per-rank offset, avsr/cells.py:46-54 masks). */
int avsr_zero_multi(void* const* ptrs, const int64_t* n_words, int32_t count, void* stream);
int avsr_add_int(const int32_t* a, int32_t b, int32_t* out, void* stream);
/* Many independent column sums (avsr_colsum semantics per job: out[f] = alpha * sum_r a[r][f] (* b[r][f]) + beta*out[f]) in two
 * launches: the bias gradients of a train step (seq2seq.py:222).  scratch >= sum_j ceil(rows_j / max(32, ceil(rows_j/256))) * F_j floats. */
typedef struct avsr_colsum_job {
  avsr_mat a;
  avsr_mat b;              /* b.ptr == NULL: plain column sums */
  float* out;
  int32_t rows, F;
  float alpha, beta;
} avsr_colsum_job;
int avsr_colsum_multi(const avsr_colsum_job* jobs, int32_t n, float* scratch, int64_t scratch_floats, void* stream);
/* Deferred weight-gradient reductions of the lip CNN (video.py:57-88 layers; seq2seq.py:222 tf.gradients of their kernels / biases):
 * between _begin and _end every avsr_conv_bwd_weight on this thread only RECORDS the final sum over its per-workgroup partial slabs;
 * _end runs all of them as one launch.  The caller passes each convolution its OWN scratch region (the slabs must survive until _end:
 * at most 512 * max(k*k*Ci*Co + Co, 12*Ci*16 + 16) floats per call) and must not read dw / dbias in between. */
int avsr_slab_defer_begin(void);
int avsr_slab_defer_end(void* stream);
/* AU regression loss (avsr/encoder.py:173-189); z = pre-sigmoid Dense(2) outputs [B][T][2]. */
int avsr_au_loss(const float* z, const float* aus, const int32_t* len, float* row_loss, float* dz, int32_t B, int32_t T,
                 float weight, void* stream);
/* Data-parallel form: the masked mean runs over the GLOBAL batch -- total_count[0] (device) = all-reduced 2 * sum_b min(len_b, T);
 * every rank then contributes its share of the numerator.  NULL = the local count (= avsr_au_loss). */
int avsr_au_loss_dp(const float* z, const float* aus, const int32_t* len, float* row_loss, float* dz, int32_t B, int32_t T,
                    float weight, const float* total_count, void* stream);

int avsr_normed_v(const float* v, const float* g, float* vn, int32_t H, void* stream);
int avsr_normed_v_bwd(const float* v, const float* g, const float* dvn, float* dv, float* dg, int32_t H, void* stream);

/* out[0] (+)= scale * (do_sqrt ? sqrt(sum part) : sum part) */
int avsr_reduce_scalar(const float* part, int32_t n, float* out, int32_t do_sqrt, int32_t accumulate, float scale,
                       void* stream);

/* l2_regularizer on the RNN kernels (avsr/seq2seq.py:175-178): grads += l2*w; loss_accum += 0.5*l2*sum w^2.
 * seg_off/seg_n are HOST arrays of flat-buffer segments; scratch >= 64*nseg floats. */
int avsr_l2_regularise(const int64_t* seg_off, const int64_t* seg_n, int32_t nseg, const float* params, float* grads,
                       float l2, float* loss_accum, float* scratch, void* stream);
/* norm_out[0] = grad_scale * ||grads||_2 ; scratch >= 1024 floats */
int avsr_global_norm(const float* grads, int64_t n, float grad_scale, float* norm_out, float* scratch, void* stream);
/* tf.clip_by_global_norm + tf.train.AdamOptimizer(eps=1e-8) + linear warm-up (avsr/seq2seq.py:195-199, :245-246,
 * :275-280).  step[0] (device int32) is read as global_step and incremented. clip_norm <= 0 disables clipping. */
int avsr_adam_step(float* params, float* grads, float* m, float* v, int64_t n, const float* global_norm, int32_t* step,
                   float lr, int32_t warmup_steps, float clip_norm, float grad_scale, void* stream);
/* Same with lr_decay=('cosine_restarts', first_decay_steps) (avsr/seq2seq.py:266-270: tf.train.cosine_decay_restarts
 * with its defaults t_mul=2, m_mul=1, alpha=0, evaluated at global_step; the warm-up factor multiplies the result).
 * first_decay_steps == 0: constant learning rate. */
int avsr_adam_step_decay(float* params, float* grads, float* m, float* v, int64_t n, const float* global_norm,
                         int32_t* step, float lr, int32_t warmup_steps, int32_t first_decay_steps, float clip_norm,
                         float grad_scale, void* stream);
/* The reference's other optimisers (avsr/seq2seq.py:195-218).  optimiser: 0 Adam (= avsr_adam_step_decay), 1 Nadam
 * (contrib.opt.NadamOptimizer: Adam with the Nesterov numerator beta1*m + (1-beta1)*g), 2 AdamW (contrib.opt.AdamWOptimizer:
 * var -= weight_decay * var, then Adam), 3 Momentum(0.9, use_nesterov=False) with the accumulator in m (v unused). */
int avsr_optimiser_step(float* params, float* grads, float* m, float* v, int64_t n, const float* global_norm, int32_t* step,
                        float lr, int32_t warmup_steps, int32_t first_decay_steps, float clip_norm, float grad_scale,
                        int32_t optimiser, float weight_decay, void* stream);

/* Optional per-launch HIP-event timing of the engine's own kernels (bench.py roofline figures).  Between
 * begin and end every gemm / step / attention launch is bracketed by an event pair on its stream; end
 * synchronises the device and returns per-kind launch counts and summed milliseconds.
 * kinds: 0 gemm, 1 LSTM-forward step, 2 LSTM-backward step, 3 dense step, 4 attention fwd, 5 attention bwd,
 * 6 persistent RNN forward, 7 persistent RNN backward, 8 / 9 fused persistent decoder forward / backward, 10 / 11 / 12 convolution forward / data gradient / weight gradient, 13 / 14 the AV-Align attentive layer's fused persistent forward / backward.  out_flops (may be NULL): algorithmic FLOPs summed per kind
 * where the launcher knows them (gemm, persistent RNN kernels), else 0. */
#define AVSR_PROF_NKIND 15
int avsr_prof_begin(int32_t max_launches);
int avsr_prof_end(int32_t* out_count, float* out_ms, double* out_flops);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* AVSR_HIP_H */

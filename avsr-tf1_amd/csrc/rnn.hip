// Host-side wavefront scheduler for the masked multi-layer RNN (encoder stacks).
//
// tf.nn.dynamic_rnn runs layer-by-layer inside one while_loop iteration, T iterations in sequence
// (encoder.py:80, :110).  Cell (layer l, time t) only needs (l-1, t) and (l, t-1), so all cells on
// an anti-diagonal are independent: launch s runs cell (l, t = s - l) of every stack at once.  That
// cuts the sequential chain from n_layers*T launches to T + n_layers - 1, and lets the video and
// audio encoders and both directions of a bidirectional stack share launches.  The backward pass
// (BPTT) runs the mirrored wavefront.
#include "step.h"
#include "avsr_hip.h"
#include "persist.h"
#include "cell_state.h"    // the layout of `state` / `dstate`

extern "C" int avsr_step_launch_raw(const void* launch, void* stream);
int avsr_rnn_fwd_persistent(const avsr_rnn_stack* st, int32_t n, void* stream, int dry);
int avsr_rnn_bwd_persistent(const avsr_rnn_stack* st, int32_t n, void* stream, int dry);

// Persistent execution: all stacks in one launch when they fit together, else one launch per stack when every
// stack fits on its own (checked first: nothing runs unless everything can), else AVSR_ERR_UNSUPPORTED.
// dry: decide only (avsr_rnn_plan): the same conditions in the same order, nothing launched.
static int run_persistent(int (*fn)(const avsr_rnn_stack*, int32_t, void*, int), const avsr_rnn_stack* st, int32_t n, void* stream, int dry = 0) {
  for (int i = 0; i < n; ++i)                      // ResidualWrapper'd layers run through the per-step launches
    for (int l = 0; l < st[i].n_layers && l < AVSR_MAX_LAYERS; ++l)
      if (st[i].layer[l].residual) return AVSR_ERR_UNSUPPORTED;
  int rc = fn(st, n, stream, dry);
  if (rc != AVSR_ERR_UNSUPPORTED || n == 1) return rc;
  avsr::RnnPlanRec* const rec = avsr::g_rnn_plan;
  const int noted = rec ? rec->n : 0;
  for (int i = 0; i < n; ++i)
    if ((rc = fn(st + i, 1, stream, 1)) != AVSR_OK) { if (rec) rec->n = noted; return rc; }   // (a plan keeps no record of stacks that fitted)
  if (dry) return AVSR_OK;
  for (int i = 0; i < n; ++i)
    if ((rc = fn(st + i, 1, stream, 0)) != AVSR_OK) return rc;
  return AVSR_OK;
}

// launches of the per-step form: the wavefront's anti-diagonals (two phases each for a GRU)
static int wavefront_steps(const avsr_rnn_stack* st, int32_t n) {
  int nsteps = 0;
  for (int i = 0; i < n; ++i) nsteps = nsteps > st[i].T + st[i].n_layers - 1 ? nsteps : st[i].T + st[i].n_layers - 1;
  return nsteps;
}
// tasks of its widest launch (every layer of every stack): one StepLaunch holds STEP_MAX_TASKS
static int wavefront_tasks(const avsr_rnn_stack* st, int32_t n) {
  int ntask = 0;
  for (int i = 0; i < n; ++i) ntask += st[i].n_layers;
  return ntask;
}

namespace avsr {

thread_local RnnPlanRec* g_rnn_plan = nullptr;

static inline void set_cell_dropout(StepTask& tk, const avsr_rnn_stack& S, int l) {
  if (!S.seed) return;
  const uint32_t cid = (uint32_t)(S.cell_id_base + l);
  tk.seed = S.seed;
  tk.k_st = S.keep_state; tk.k_out = S.keep_out; tk.k_in = 1.0f;
  tk.r_st = cid * 4 + 1; tk.r_out = cid * 4 + 2;
  if (l + 1 < S.n_layers) {            // consumer = next layer of the stack: mask over its [units_l] wide input
    tk.k_in = S.keep_in; tk.r_in = (cid + 1) * 4; tk.in_W = S.layer[l].units; tk.in_coff = 0;
  } else if (S.consumer_width > 0) {   // consumer = attention-wrapped layer above the stack (AV-Align)
    tk.k_in = S.consumer_keep; tk.r_in = (uint32_t)S.consumer_stream; tk.in_W = S.consumer_width; tk.in_coff = 0;
  }
}

// Every argument check of the per-step forward wavefront: nothing is written before it has passed.
static int fwd_check(const avsr_rnn_stack* st, int32_t n) {
  const bool gru = st[0].cell == 1;
  for (int i = 0; i < n; ++i) {
    const avsr_rnn_stack& S = st[i];
    if (S.cell != 0 && S.cell != 1) return AVSR_ERR_UNSUPPORTED;
    if (S.cell != st[0].cell) return AVSR_ERR_ARG;            // one cell kind per call
    if (S.n_layers <= 0 || S.n_layers > AVSR_MAX_LAYERS || S.B <= 0 || S.T <= 0) return AVSR_ERR_ARG;
    for (int l = 0; l < S.n_layers; ++l) {
      const avsr_rnn_layer& Ly = S.layer[l];
      if (Ly.units % 4 || Ly.in_dim % 4 || !Ly.wt || !Ly.gates || !Ly.cs || !Ly.state) return AVSR_ERR_ARG;
      if (Ly.hoisted && l != 0) return AVSR_ERR_ARG;
      if (Ly.residual && (l == 0 || Ly.in_dim != Ly.units || !S.layer[l - 1].out)) return AVSR_ERR_ARG;
    }
  }
  if (wavefront_tasks(st, n) > STEP_MAX_TASKS) return AVSR_ERR_UNSUPPORTED;
  // what the step loop used to find on its way, in the order the wavefront reaches the layers: layer 0 of every stack, then the rest
  for (int i = 0; i < n; ++i) {
    const avsr_rnn_layer& Ly = st[i].layer[0];
    if (gru && (!Ly.wt2 || !Ly.rh_seq)) return AVSR_ERR_ARG;
    if (!Ly.hoisted) return AVSR_ERR_UNSUPPORTED;             // layer 0 input projection must be hoisted (avsr_gemm)
  }
  for (int i = 0; gru && i < n; ++i)
    for (int l = 1; l < st[i].n_layers; ++l)
      if (!st[i].layer[l].wt2 || !st[i].layer[l].rh_seq) return AVSR_ERR_ARG;
  return AVSR_OK;
}

// Likewise for the backward wavefront.  The GRU checks belong to the per-step path alone (the persistent forms take LSTM stacks
// only and decline every GRU call), so they can stand ahead of the persistent attempt without refusing a call it would accept.
static int bwd_check(const avsr_rnn_stack* st, int32_t n) {
  for (int i = 0; i < n; ++i) {
    const avsr_rnn_stack& S = st[i];
    if ((S.cell != 0 && S.cell != 1) || S.cell != st[0].cell) return AVSR_ERR_UNSUPPORTED;
    if (S.n_layers <= 0 || S.n_layers > AVSR_MAX_LAYERS) return AVSR_ERR_ARG;
    for (int l = 0; l < S.n_layers; ++l) {
      const avsr_rnn_layer& Ly = S.layer[l];
      if (!Ly.w || !Ly.dgates || !Ly.dstate || !Ly.gates || !Ly.cs) return AVSR_ERR_ARG;
    }
  }
  if (wavefront_tasks(st, n) > STEP_MAX_TASKS) return AVSR_ERR_UNSUPPORTED;
  for (int i = 0; st[0].cell == 1 && i < n; ++i)
    for (int l = 0; l < st[i].n_layers; ++l) {
      const avsr_rnn_layer& Ly = st[i].layer[l];
      if (!Ly.w2 || !Ly.dgates2) return AVSR_ERR_ARG;
      if ((st[i].seed || Ly.residual) && !Ly.hs_seq) return AVSR_ERR_ARG;   // h(t-1) as the cell consumed it, below
    }
  return AVSR_OK;
}

}  // namespace avsr

extern "C" int avsr_rnn_fwd(const avsr_rnn_stack* st, int32_t n, void* stream) {
  using namespace avsr;
  if (!st || n <= 0 || n > AVSR_MAX_STACKS) return AVSR_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int rc = run_persistent(avsr_rnn_fwd_persistent, st, n, stream);           // one launch for the whole sequence when it fits:
  if (rc != AVSR_ERR_UNSUPPORTED) return rc;                                 // 8-row groups per XCD / the agent-scope form
  if ((rc = fwd_check(st, n))) return rc;
  for (int i = 0; i < n; ++i)
    for (int l = 0; l < st[i].n_layers; ++l) {       // zero initial state: h parity 0, c parity 0
      const avsr_rnn_layer& Ly = st[i].layer[l];
      const size_t bytes = sizeof(float) * st[i].B * Ly.units;
      if (avsr::dev_zero(st_h(Ly.state, st[i].B, Ly.units, 0), bytes, s) != hipSuccess) return AVSR_ERR_HIP;
      if (avsr::dev_zero(st_c(Ly.state, st[i].B, Ly.units, 0), bytes, s) != hipSuccess) return AVSR_ERR_HIP;
    }

  static thread_local StepLaunch L;
  const bool gru = st[0].cell == 1;
  const int nsteps = wavefront_steps(st, n);
  for (int step = 0; step < nsteps; ++step) {
   for (int phase = 0; phase < (gru ? 2 : 1); ++phase) {
    L.ntask = 0;
    for (int i = 0; i < n; ++i) {
      const avsr_rnn_stack& S = st[i];
      for (int l = 0; l < S.n_layers; ++l) {
        const int t = step - l;
        if (t < 0 || t >= S.T) continue;
        const avsr_rnn_layer& Ly = S.layer[l];
        StepTask& tk = L.task[L.ntask++];
        tk = StepTask{};
        const int B = S.B, H = Ly.units, in = Ly.in_dim, p = t & 1, q = (t + 1) & 1;
        const bool cand = gru && phase == 1;                   // a GRU's second launch: the candidate, through r*h
        const float* wt = cand ? Ly.wt2 : Ly.wt;
        if (!Ly.hoisted) {
          const avsr_rnn_layer& Lo = S.layer[l - 1];
          StepSrc& x = tk.src[tk.nsrc++];
          // the lower layer's EMITTED output: its h state, unless dropout masks or a residual sum make the two differ
          x.a = (S.seed || Lo.residual) ? st_x(Lo.state, B, Lo.units, q) : st_h(Lo.state, B, Lo.units, q);
          x.sb = Lo.units; x.K = in; x.w = wt; x.ldw = in + H; x.kind = SRC_PLAIN;
        }
        StepSrc& h = tk.src[tk.nsrc++];
        h.a = cand ? st_rh(Ly.state, B, H) : st_h(Ly.state, B, H, p); h.sb = H; h.K = H; h.w = wt + in; h.ldw = in + H; h.kind = SRC_PLAIN;
        tk.B = B; tk.t = t; tk.T = S.T; tk.reverse = S.reverse; tk.len = S.len; tk.s2 = Ly.hoisted ? 1 : 0;
        tk.p4 = st_h(Ly.state, B, H, p);
        if (gru && !cand) {
          tk.N = 2 * H; tk.mode = EP_GRU_GATES; tk.bias = Ly.bias;
          tk.p0 = Ly.gates; tk.p1 = st_rh(Ly.state, B, H); tk.p2 = Ly.rh_seq;
          continue;
        }
        if (gru) { tk.N = H; tk.mode = EP_GRU_CAND; tk.bias = Ly.bias2; tk.p0 = Ly.cs; tk.p1 = Ly.gates; }
        else { tk.N = 4 * H; tk.mode = EP_LSTM_FWD; tk.bias = Ly.bias; tk.p0 = Ly.gates; tk.p1 = Ly.cs;
               tk.p3 = st_c(Ly.state, B, H, p); tk.p5 = st_c(Ly.state, B, H, q); }
        tk.p2 = Ly.out ? Ly.out + Ly.ld_out /* slot 1 = time 0 */ + Ly.out_col : nullptr;
        tk.s0 = (long)(S.T + 2) * Ly.ld_out; tk.s1 = Ly.ld_out;
        tk.p6 = st_h(Ly.state, B, H, q);
        if (Ly.residual) {   // + raw input = the lower layer's output record (slot 1 = time 0)
          const avsr_rnn_layer& Lo = S.layer[l - 1];
          tk.p8 = Lo.out + Lo.ld_out + Lo.out_col; tk.pad0 = (int)((long)(S.T + 2) * Lo.ld_out); tk.pad1 = (int)Lo.ld_out;
        }
        if (S.seed) {
          set_cell_dropout(tk, S, l);
          tk.s4 = (long)(S.T + 2) * H; tk.s5 = H;
          if (Ly.hs_seq) tk.p9 = Ly.hs_seq + H;                       // slot 1 = time 0
          if (l + 1 < S.n_layers) tk.p10 = st_x(Ly.state, B, H, q);
          if (Ly.xt_seq) tk.p11 = Ly.xt_seq + H;
        } else if (Ly.residual) {
          if (l + 1 < S.n_layers) tk.p10 = st_x(Ly.state, B, H, q);   // no masks: the plain residual sum, for the layer above
          if (Ly.hs_seq) { tk.p9 = Ly.hs_seq + H; tk.s4 = (long)(S.T + 2) * H; tk.s5 = H; }   // h itself (dWh operand): `out` holds h + x
        }
      }
    }
    if (L.ntask == 0) continue;
    if ((rc = avsr_step_launch_raw(&L, stream))) return rc;
   }
  }
  for (int i = 0; i < n; ++i) {
    const avsr_rnn_stack& S = st[i];
    for (int l = 0; l < S.n_layers; ++l) {
      const avsr_rnn_layer& Ly = S.layer[l];
      const size_t bytes = sizeof(float) * S.B * Ly.units;
      if (Ly.h_final && avsr::dev_copy(Ly.h_final, st_h(Ly.state, S.B, Ly.units, S.T & 1), bytes, s) != hipSuccess)
        return AVSR_ERR_HIP;
      if (!gru && Ly.c_final && avsr::dev_copy(Ly.c_final, st_c(Ly.state, S.B, Ly.units, S.T & 1), bytes, s) != hipSuccess)
        return AVSR_ERR_HIP;
    }
  }
  return AVSR_OK;
}

extern "C" int avsr_rnn_bwd(const avsr_rnn_stack* st, int32_t n, void* stream) {
  using namespace avsr;
  if (!st || n <= 0 || n > AVSR_MAX_STACKS) return AVSR_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int rc = bwd_check(st, n);
  if (rc) return rc;
  const bool gru = st[0].cell == 1;
  for (int i = 0; i < n; ++i) {
    const avsr_rnn_stack& S = st[i];
    for (int l = 0; l < S.n_layers; ++l) {
      const avsr_rnn_layer& Ly = S.layer[l];
      const int B = S.B, H = Ly.units, pT = S.T & 1;
      const size_t bh = sizeof(float) * B * H;
      // rolling dG (both parities), dc / dh_carry at parity T&1 = gradient of the final state
      if (avsr::dev_zero(Ly.dstate, (Ly.residual ? 14 : 12) * bh, s) != hipSuccess) return AVSR_ERR_HIP;
      if (l != S.n_layers - 1) continue;
      if (!gru && S.dc_final && avsr::dev_copy(ds_dc(Ly.dstate, B, H, pT), S.dc_final, bh, s) != hipSuccess) return AVSR_ERR_HIP;
      if (S.dh_final && avsr::dev_copy(gru ? dg_carry(Ly.dstate, B, H, pT) : ds_dh(Ly.dstate, B, H, pT), S.dh_final, bh, s) != hipSuccess)
        return AVSR_ERR_HIP;
    }
  }
  rc = run_persistent(avsr_rnn_bwd_persistent, st, n, stream);              // one launch for the whole BPTT when it fits
  if (rc != AVSR_ERR_UNSUPPORTED) return rc;

  static thread_local StepLaunch L;
  const int nsteps = wavefront_steps(st, n);
  for (int step = 0; step < nsteps; ++step) {
   for (int phase = 0; phase < (gru ? 2 : 1); ++phase) {
    L.ntask = 0;
    for (int i = 0; i < n; ++i) {
      const avsr_rnn_stack& S = st[i];
      const int nl = S.n_layers;
      for (int l = nl - 1; l >= 0; --l) {
        const int t = S.T - 1 - (step - (nl - 1 - l));
        if (t < 0 || t >= S.T) continue;
        const avsr_rnn_layer& Ly = S.layer[l];
        StepTask& tk = L.task[L.ntask++];
        tk = StepTask{};
        const int B = S.B, H = Ly.units, in = Ly.in_dim, p = t & 1, q = (t + 1) & 1;
        const int G = gru ? 2 : 4;                         // gate pre-activations per unit
        float* const ds = Ly.dstate;
        tk.B = B; tk.N = H; tk.t = t; tk.T = S.T; tk.reverse = S.reverse; tk.len = S.len;
        tk.p0 = Ly.gates;
        if (gru) {
          // h(t-1) as the cell consumed it: the state-dropped sequence under dropout, else the output sequence
          const bool own_h = S.seed || Ly.residual;        // (a residual layer's output record holds h + x)
          const float* hseq = own_h ? Ly.hs_seq : Ly.out + Ly.out_col;
          const long hld = own_h ? H : Ly.ld_out;
          tk.p2 = const_cast<float*>(hseq) + (S.reverse ? 2 * hld : 0); tk.s2 = (long)(S.T + 2) * hld; tk.s3 = hld;
          tk.p6 = dg_tmp(ds, B, H, 0); tk.p7 = dg_tmp(ds, B, H, 1);
          if (phase == 1) {
            tk.mode = EP_GRU_BWD_GATES;
            StepSrc& a = tk.src[tk.nsrc++];
            a.a = dg_dpc(ds, B, H, p); a.sb = H; a.K = H; a.w = Ly.w2 + (long)in * H; a.ldw = H; a.kind = SRC_PLAIN;
            tk.p5 = dg_carry(ds, B, H, p); tk.p3 = Ly.dgates; tk.p1 = dg_dgg(ds, B, H, p);
            continue;
          }
        }
        // dh[b,u] = dG_{t+1}(own) . Wh[u,:]  +  dG_t(upper layer) . Wx_upper[u,:]  (a GRU above: its gate and its candidate kernel)
        StepSrc& a = tk.src[tk.nsrc++];
        a.a = gru ? dg_dgg(ds, B, H, q) : ds_dg(ds, B, H, q); a.sb = G * H; a.K = G * H; a.w = Ly.w + (long)in * G * H; a.ldw = G * H; a.kind = SRC_PLAIN;
        if (l + 1 < nl) {
          const avsr_rnn_layer& Up = S.layer[l + 1];
          const int HU = Up.units;
          StepSrc& u = tk.src[tk.nsrc++];
          u.a = gru ? dg_dgg(Up.dstate, B, HU, p) : ds_dg(Up.dstate, B, HU, p); u.sb = G * HU; u.K = G * HU; u.w = Up.w; u.ldw = G * HU; u.kind = SRC_PLAIN;
          if (gru) {
            StepSrc& u2 = tk.src[tk.nsrc++];
            u2.a = dg_dpc(Up.dstate, B, HU, p); u2.sb = HU; u2.K = HU; u2.w = Up.w2; u2.ldw = HU; u2.kind = SRC_PLAIN;
          }
        }
        tk.p1 = Ly.cs;
        if (gru) {
          tk.mode = EP_GRU_BWD_CAND;
          tk.p4 = dg_carry(ds, B, H, q); tk.p5 = dg_dpc(ds, B, H, p); tk.p3 = Ly.dgates2;
        } else {
          tk.mode = EP_LSTM_BWD;
          tk.p2 = Ly.dgates; tk.p3 = ds_dg(ds, B, H, p);
          tk.p4 = ds_dc(ds, B, H, q); tk.p5 = ds_dc(ds, B, H, p);
          tk.p6 = ds_dh(ds, B, H, q); tk.p7 = ds_dh(ds, B, H, p);
        }
        if (Ly.dout) {
          tk.p8 = const_cast<float*>(Ly.dout) + Ly.ld_dout + Ly.dout_col;  // slot 1 = time 0
          tk.s0 = (long)(S.T + 2) * Ly.ld_dout; tk.s1 = Ly.ld_dout;
        } else if (l + 1 < nl && S.layer[l + 1].residual) {
          tk.p8 = ds_dres(S.layer[l + 1].dstate, B, S.layer[l + 1].units, p); tk.s0 = H; tk.s1 = 0;   // d(output) through the upper layer's residual sum
        }
        if (Ly.residual) tk.p10 = ds_dres(ds, B, H, p);
        if (S.seed) {
          set_cell_dropout(tk, S, l);
          if (l + 1 >= nl) tk.k_in = 1.0f;   // no upper layer inside the stack: external d out is already wrt the output
        }
      }
    }
    if (L.ntask == 0) continue;
    if ((rc = avsr_step_launch_raw(&L, stream))) return rc;
   }
  }
  return AVSR_OK;
}

// What a call would launch (avsr_hip.h): run_persistent's dry path under the asked-for mode and scratch sizes, with this thread's recorder
// set.  The scratch addresses are dummies that nothing dereferences (the dry paths only offset them).
extern "C" int avsr_rnn_plan(const avsr_rnn_stack* st, int32_t n, int32_t bwd, int32_t mode, int64_t sync_ints, int64_t scratch_floats,
                             avsr_rnn_launch* out, int32_t cap) {
  using namespace avsr;
  if (!st || n <= 0 || n > AVSR_MAX_STACKS || cap < 0 || (cap > 0 && !out) || sync_ints < 0 || scratch_floats < 0) return AVSR_ERR_ARG;
  for (int i = 0; i < n; ++i)
    if (st[i].n_layers <= 0 || st[i].n_layers > AVSR_MAX_LAYERS || st[i].B <= 0 || st[i].T <= 0) return AVSR_ERR_ARG;
  static int32_t dummy_sync[1];
  static float dummy_scratch[1];
  int32_t* const sync0 = g_sync; const int64_t ints0 = g_sync_ints; const int mode0 = g_persist_mode;
  float* const scr0 = g_persist_scratch; const int64_t floats0 = g_persist_scratch_floats;
  g_sync = sync_ints ? dummy_sync : nullptr; g_sync_ints = sync_ints; g_persist_mode = mode;
  g_persist_scratch = scratch_floats ? dummy_scratch : nullptr; g_persist_scratch_floats = scratch_floats;
  RnnPlanRec R = {out, cap, 0};
  g_rnn_plan = &R;
  const int rc = run_persistent(bwd ? avsr_rnn_bwd_persistent : avsr_rnn_fwd_persistent, st, n, nullptr, 1);
  g_rnn_plan = nullptr;
  g_sync = sync0; g_sync_ints = ints0; g_persist_mode = mode0; g_persist_scratch = scr0; g_persist_scratch_floats = floats0;
  // avsr_rnn_bwd sizes its per-step launch before it tries the persistent forms, avsr_rnn_fwd only when it needs it
  if ((bwd || rc == AVSR_ERR_UNSUPPORTED) && wavefront_tasks(st, n) > STEP_MAX_TASKS) return AVSR_ERR_UNSUPPORTED;
  if (rc == AVSR_ERR_UNSUPPORTED) {
    if (cap > 0) out[0] = avsr_rnn_launch{AVSR_RNN_FORM_PER_STEP, n, 0, 0, wavefront_steps(st, n) * (st[0].cell == 1 ? 2 : 1), 0, 0, 0};
    return 1;
  }
  return rc < 0 ? rc : R.n;
}

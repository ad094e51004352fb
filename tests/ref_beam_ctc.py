"""References for joint CTC / attention scoring in beam search (include/avsr_hip.h avsr_beam_ctc).

The prefix scorer is written once, in NumPy, over a dtype: float64 is the reference, float32 is a RESTATEMENT of the same recursion that
is used only to size tolerances (how far an fp32 evaluation of this recursion lies from fp64 on the very inputs a test uses).  It works
on rows: row r is one hypothesis, y[r] the log_softmax [T, V + 1] of its utterance's head logits (blank = class V), Tb[r] its frames.

    state   rn, rb [R, T]  log-probability of the alignments of frames 0..t that collapse to exactly g, ending in a non-blank / a blank
            psi [R]        log-probability of all label sequences that start with g;  last [R]  g's last symbol, -1 for the empty prefix
    term[r][v] = psi(g_r . v) - psi(g_r);  0 where psi(g_r) = -inf, Tb[r] = 0 or the row is dead (finished);  psi(g . EOS) = log p_ctc(g | x)

`step` is one avsr_beam_ctc_step: rows gather their parent, step 0 / EOS / finished rows copy it through, the others extend it.
`beam_search_decode_ctc` is ref_beam_lm.beam_search_decode_lm's loop with the term added (and the language model optional); the head
logits come from ref_ctc's head on the oracle's memory.  Entries of the state at t >= Tb are never read and hold no meaning."""
import dataclasses

import numpy as np
import torch

import ref_beam_lm as RL
import ref_ctc as RC
from oracle import avsr_oracle as O

NEG = -np.inf


def lae(a, b):
    """log-add-exp; (-inf) + (-inf) = -inf, never NaN."""
    return np.logaddexp(a, b)


def lse(x, axis):
    """max-shifted log-sum-exp along `axis`; -inf where every entry is -inf (or there is none)."""
    m = np.max(x, axis=axis, initial=NEG)
    ms = np.where(np.isfinite(m), m, 0).astype(x.dtype)
    with np.errstate(divide="ignore"):
        out = ms + np.log(np.sum(np.exp(x - np.expand_dims(ms, axis)), axis=axis, dtype=x.dtype))
    return np.where(m == NEG, NEG, out).astype(x.dtype)


def log_softmax(z, dt=np.float64):
    z = np.asarray(z).astype(dt)
    m = z.max(axis=-1, keepdims=True)
    return (z - (m + np.log(np.sum(np.exp(z - m), axis=-1, keepdims=True, dtype=dt)))).astype(dt)


def _tmask(Tb, T):
    return np.arange(T)[None, :] < np.asarray(Tb)[:, None]


def empty_state(y, Tb):
    R, T, C = y.shape
    dt = y.dtype
    return dict(rn=np.full((R, T), NEG, dt), rb=np.cumsum(y[:, :, C - 1], axis=1, dtype=dt), psi=np.zeros(R, dt), last=np.full(R, -1, np.int64))


def extend(y, Tb, st, c):
    """The state of g . c for every row (c [R], none of them EOS)."""
    R, T, C = y.shape
    dt = y.dtype
    c = np.asarray(c, np.int64)
    rn, rb, last = st["rn"], st["rb"], st["last"]
    phi = np.where((c == last)[:, None], rb, lae(rn, rb))
    yc = y[np.arange(R), :, c]
    yb = y[:, :, C - 1]
    nn, nb = np.full((R, T), NEG, dt), np.full((R, T), NEG, dt)
    nn[:, 0] = np.where(last < 0, yc[:, 0], NEG)
    for t in range(1, T):
        nn[:, t] = lae(nn[:, t - 1], phi[:, t - 1]) + yc[:, t]
        nb[:, t] = lae(nn[:, t - 1], nb[:, t - 1]) + yb[:, t]
    x = np.concatenate([nn[:, :1], phi[:, :-1] + yc[:, 1:]], axis=1)
    psi = lse(np.where(_tmask(Tb, T), x, NEG).astype(dt), 1)
    return dict(rn=nn, rb=nb, psi=psi, last=c.copy())


def psi_ext(y, Tb, st, eos):
    """psi(g . v) [R, V] for every symbol v, EOS included (eos=None: no symbol is EOS) -- a log-sum-exp over t, no recursion."""
    R, T, C = y.shape
    V, dt = C - 1, y.dtype
    Tb = np.asarray(Tb)
    rn, rb, last = st["rn"], st["rb"], st["last"]
    pa = lae(rn, rb)
    same = np.arange(V)[None, :] == last[:, None]                                       # [R, V]
    phi = np.where(same[:, None, :], rb[:, :, None], pa[:, :, None])                    # [R, T, V]
    first = np.where((last < 0)[:, None], y[:, 0, :V], NEG)
    x = np.concatenate([first[:, None, :], phi[:, :-1] + y[:, 1:, :V]], axis=1)
    out = lse(np.where(_tmask(Tb, T)[:, :, None], x, NEG).astype(dt), 1)
    if eos is not None:
        out[:, eos] = np.where(Tb > 0, pa[np.arange(R), np.maximum(Tb - 1, 0)], NEG)
    return out


def term(y, Tb, st, eos, dead=None):
    pe = psi_ext(y, Tb, st, eos)
    psi = st["psi"]
    zero = (psi == NEG) | (np.asarray(Tb) <= 0)
    if dead is not None:
        zero = zero | np.asarray(dead, bool)
    with np.errstate(invalid="ignore"):
        tm = pe - psi[:, None]
    return np.where(zero[:, None], 0, tm).astype(y.dtype)


def step(y, Tb, st, tok, parent, fin, step_idx, eos):
    """One avsr_beam_ctc_step: (new state, term [R, V])."""
    tok, parent, fin = np.asarray(tok, np.int64), np.asarray(parent, np.int64), np.asarray(fin).astype(bool)
    par = {k: v[parent].copy() for k, v in st.items()}
    dead = fin | ((tok == eos) if step_idx > 0 else np.zeros_like(fin))
    copy = dead if step_idx > 0 else np.ones_like(fin)
    if copy.all():
        new = par
    else:
        ext = extend(y, Tb, par, np.where(copy, 0, tok))
        new = {k: np.where(copy.reshape((-1,) + (1,) * (v.ndim - 1)), par[k], ext[k]) for k, v in par.items()}
    return new, term(y, Tb, new, eos, dead)


def prefix_state(y1, Tb, g, dt=np.float64):
    """State of label prefix g (a list) on ONE utterance y1 [T, C]."""
    y = np.asarray(y1, dt)[None]
    st = empty_state(y, [Tb])
    for c in g:
        st = extend(y, [Tb], st, [c])
    return y, st


def brute_force_psi(logp, prefix, blank):
    """log of the sum over ALL C^T frame labellings whose collapsed sequence STARTS WITH `prefix` (tiny T only)."""
    import itertools
    T, C = logp.shape
    tot = 0.0
    for path in itertools.product(range(C), repeat=T):
        seq, prev = [], -1
        for k in path:
            if k != prev and k != blank:
                seq.append(k)
            prev = k
        if seq[:len(prefix)] == list(prefix):
            tot += float(np.exp(sum(logp[t, k] for t, k in enumerate(path))))
    return np.log(tot) if tot > 0 else NEG


# ---- the search ---------------------------------------------------------------------------------------------------------------------
def head_logits(P, m, cfg):
    """ref_ctc's head on the oracle's memory: (z [B, T, V + 1] fp64 numpy, T_b [B])."""
    s = RC.ctc_stream(cfg)
    kn, bn = RC.head_names(s)
    z = (m.enc[s].outputs @ P[kn] + P[bn]).numpy()
    lens = np.asarray(m.lens[s].numpy() if hasattr(m.lens[s], "numpy") else m.lens[s])
    return z, np.clip(lens, 0, z.shape[1]).astype(np.int64)


@torch.no_grad()
def beam_search_decode_ctc(P_np, cfg, batch, ctc_weight, lm_np=None, lcfg=None, lm_weight=0.0, beam_width=10, length_penalty_weight=None,
                           max_steps=None, follow=None, term_dtype=np.float64):
    """Returns ids [B, T, K], logp [B, K], lengths [B, K], trace (as ref_beam_lm.beam_search_decode_lm; trace['terms'] holds every
    step's term [B * K, V]).  P_np holds the head's two variables.  term_dtype=np.float32: the CTC term alone comes from the float32
    restatement (everything else stays fp64) -- with follow=None that is the search an exact fp32 kernel would make."""
    dtype = torch.float64
    P = O.to_torch(P_np, dtype)
    PL = O.to_torch(lm_np, dtype) if lm_np is not None else None
    m = O._Model(P, cfg, batch, False, dtype)
    B, K, V, eos = m.B, beam_width, cfg.vocab_size, cfg.eos_id
    w = length_penalty_weight if length_penalty_weight is not None else (0.5 if cfg.architecture == "bimodal" else 0.6)
    max_steps = cfg.max_label_length if max_steps is None else max_steps
    z, Tb_u = head_logits(P, m, cfg)
    y = np.repeat(log_softmax(z.astype(term_dtype), term_dtype), K, axis=0)
    Tb = np.repeat(Tb_u, K)
    cst = empty_state(y, Tb)
    tile = lambda t: t.repeat_interleave(K, dim=0)
    for mech in m.mechs:
        mech.values, mech.keys, mech.mask = tile(mech.values), tile(mech.keys), tile(mech.mask)
    state = tuple(tile(s) for s in m.init_state)
    lm_state = RL.lm_zero_state(lcfg, B * K, dtype) if PL is not None else None
    att = torch.zeros(B * K, m.att_dim, dtype=dtype)
    tok = torch.full((B * K,), cfg.go_id, dtype=torch.int64)
    logp = torch.full((B, K), -float("inf"), dtype=dtype)
    logp[:, 0] = 0.0
    finished = torch.zeros(B, K, dtype=torch.bool)
    lengths = torch.zeros(B, K, dtype=torch.int64)
    rows = torch.arange(B * K)
    step_ids, parent_ids, step_gaps, terms = [], [], [], []
    f_dev, f_same, f_distinct, f_short = [], [], [], False
    for t in range(max_steps):
        out, state, att, _ = m.step(O._embedding(P, cfg)[tok], state, att, t)
        step_lp = torch.log_softmax(m.logits(out), dim=-1)
        if PL is not None:
            lm_lp, lm_state = RL.lm_step(PL, lcfg, tok, lm_state)
            if lm_weight != 0.0:
                step_lp = step_lp + lm_weight * lm_lp
        if ctc_weight != 0.0:
            cst, tm = step(y, Tb, cst, tok.numpy(), rows.numpy(), finished.reshape(-1).numpy(), t, eos)
            terms.append(tm.copy())
            step_lp = step_lp + ctc_weight * torch.as_tensor(tm.astype(np.float64))
        total, scores = O.beam_candidates(logp, finished, lengths, step_lp.reshape(B, K, V), w, eos)
        order_all = torch.argsort(scores, dim=1, descending=True, stable=True)
        order = order_all[:, :K]
        top = torch.gather(scores, 1, order_all[:, :K + 1])
        gap = top[:, :-1] - top[:, 1:]
        gap = torch.where((top[:, :-1] == top[:, 1:]) | torch.isnan(gap), torch.full_like(gap, float("inf")), gap)
        step_gaps.append(gap.min(dim=1).values.numpy())
        if follow is not None:
            if t >= follow[0].shape[0]:
                f_short = True
                break
            eng = torch.as_tensor(follow[1][t].astype(np.int64)) * V + torch.as_tensor(follow[0][t].astype(np.int64))
            s_eng, s_ref = torch.gather(scores, 1, eng), torch.gather(scores, 1, order)
            both_inf = torch.isinf(s_eng) & torch.isinf(s_ref) & (s_eng == s_ref)
            dev = torch.where(both_inf, torch.zeros_like(s_ref), (s_eng - s_ref).abs() / torch.clamp(s_ref.abs(), min=1.0))
            dev = torch.where(torch.isnan(dev), torch.full_like(dev, float("inf")), dev)
            f_dev.append(dev.max(dim=1).values.numpy())
            f_same.append((eng == order).all(dim=1).numpy())
            srt = torch.sort(eng, dim=1).values
            f_distinct.append(((srt[:, 1:] != srt[:, :-1]).all(dim=1) if K > 1 else torch.ones(B, dtype=torch.bool)).numpy())
            order = eng
        word, parent = order % V, order // V
        logp, finished, lengths = O.beam_advance(total, finished, lengths, order, V, eos)
        rows = (torch.arange(B)[:, None] * K + parent).reshape(-1)
        state = tuple(s[rows] for s in state)
        if lm_state is not None:
            lm_state = [(c[rows], h[rows]) for c, h in lm_state]
        att = att[rows]
        tok = word.reshape(-1)
        step_ids.append(word.numpy().astype(np.int32))
        parent_ids.append(parent.numpy().astype(np.int32))
        if bool(finished.all()):
            break
    sid, pid = np.stack(step_ids), np.stack(parent_ids)
    beams = O.gather_tree(sid, pid, lengths.max(dim=1).values.numpy(), eos)
    ids = np.ascontiguousarray(beams.transpose(1, 0, 2))
    tr = dict(step_ids=sid, parent_ids=pid, gaps=np.stack(step_gaps)[:sid.shape[0]], finished=finished.numpy(), terms=terms)
    if follow is not None:
        tr.update(follow_dev=np.stack(f_dev), follow_same=np.stack(f_same), follow_distinct=np.stack(f_distinct), follow_short=f_short)
    return ids, logp.numpy(), lengths.numpy(), tr


# ---- the small search cases shared by tests/test_beam_ctc_cpu.py and tests/test_gpu_beam_ctc.py -------------------------------------
ARCHS = RL.ARCHS
WEIGHTS = (0.3, 1.0)          # the weights of the GPU test's full search
MAX_STEPS = 14                # > the longest T_b + 1 (T_a = 12), and not a multiple of the check_every (3) the GPU test uses
HEAD_SCALE, BLANK_BIAS = 6.0, 1.5
_cases = {}


def search_case(case, lm="1x10"):
    """(ocfg, mcfg, W, batch, lcfg, lmcfg, WL) of ref_beam_lm.search_case with use_ctc=True and the head's variables in W: the kernel
    scaled by HEAD_SCALE (the term must be able to change a selection), the bias leaning to the blank (so that short label sequences,
    hence EOS, stay reachable).  Built once per (case, lm) and shared; nothing in it is modified afterwards."""
    if (case, lm) not in _cases:
        ocfg, mcfg, W, batch, lcfg, lmcfg, WL = RL.search_case(case, lm)
        s = RC.ctc_stream(ocfg)
        W = RC.add_head(W, ocfg, s, seed=23)
        kn, bn = RC.head_names(s)
        W[kn] = (W[kn] * HEAD_SCALE).astype(np.float32)
        W[bn] = W[bn].copy()
        W[bn][ocfg.vocab_size] += BLANK_BIAS
        _cases[(case, lm)] = (ocfg, dataclasses.replace(mcfg, use_ctc=True), W, batch, lcfg, lmcfg, WL)
    return _cases[(case, lm)]


# ---- the step kernels on given logits, states and parents (tests/test_gpu_beam_ctc.py; sized on the CPU by tests/test_beam_ctc_cpu.py) -
# name -> utterances U, beam width K (R = U * K rows), symbols V, frames T, T_b per utterance, row stride of the head's logits
KERNEL_CASES = {
    "r9_v15": dict(U=3, K=3, V=15, T=70, Tb=[0, 1, 65], ld=16),
    "r30_v31": dict(U=3, K=10, V=31, T=260, Tb=[2, 3, 257], ld=32),
    "r30_v41_stride44": dict(U=3, K=10, V=41, T=66, Tb=[63, 64, 65], ld=44),
    "r30_k3_v31": dict(U=10, K=3, V=31, T=66, Tb=[0, 1, 2, 3, 63, 64, 65, 5, 9, 33], ld=32),
    "r64_v31": dict(U=16, K=4, V=31, T=66, Tb=[0, 1, 2, 3, 63, 64, 65, 4, 5, 7, 11, 17, 23, 31, 47, 66], ld=32),
    "t500_r20": dict(U=2, K=10, V=31, T=500, Tb=[500, 431], ld=32),
}
C_TOL = 37.0      # 4 x the worst ratio of the float32 restatement on KERNEL_CASES (9.24, t500_r20 step 2), rounded up; test_beam_ctc_cpu checks it


def kernel_case(name):
    """Deterministic inputs of one case: z [U, T, ld] float32 (pad columns hold 50: a leaking pad would dominate the softmax), the
    rows' prefixes (lengths 0, 1, 4 ending in a repeated symbol, 4 -- longer than the short utterances' T_b), and two chained steps
    (tok, parent_rows, fin) with non-identity parents (a permutation inside each utterance, one parent twice), symbols that repeat the
    parent's last one, EOS rows and finished rows (one of them with a symbol other than EOS)."""
    c = KERNEL_CASES[name]
    U, K, V, T, ld = c["U"], c["K"], c["V"], c["T"], c["ld"]
    R_, eos = U * K, V - 2
    rng = np.random.default_rng(sum(map(ord, name)))
    z = np.full((U, T, ld), 50.0, np.float32)
    z[:, :, :V + 1] = (rng.standard_normal((U, T, V + 1)) * 3.0).astype(np.float32)
    z[:, :, V] += 2.0
    prefixes = []
    for r in range(R_):
        a, b, d = (int(x) for x in rng.choice([v for v in range(V) if v != eos], 3, replace=False))
        prefixes.append([[], [a], [a, b, d, d], [a, b, a, d]][r % 4])
    steps, fin = [], np.zeros(R_, bool)
    last = np.array([p[-1] if p else -1 for p in prefixes])
    for s in range(2):
        par = np.concatenate([u * K + rng.permutation(K) for u in range(U)])
        par[1] = par[0]
        fin = fin[par] | (rng.random(R_) < 0.15)
        tok = rng.integers(0, V, R_)
        rep = rng.random(R_) < 0.25
        tok = np.where(rep & (last[par] >= 0), last[par], tok)
        tok = np.where(fin | (rng.random(R_) < 0.1), eos, tok)
        if fin.any():
            tok[np.nonzero(fin)[0][0]] = 0                        # a finished row that did not take EOS: copied through all the same
        steps.append((tok.astype(np.int32), par.astype(np.int32), fin.astype(np.int32)))
        last = np.where((tok == eos) | fin, last[par], tok)
        fin = fin | (tok == eos)
    return dict(c, z=z, Tb=np.asarray(c["Tb"], np.int32), eos=eos, prefixes=prefixes, steps=steps)


def kernel_reference(case, dt=np.float64):
    """(y [U, T, C], start state as the kernel is given it (fp64 state of the prefixes, rounded to float32), [(state, term) per step]) in
    `dt`: float64 is the reference, float32 the restatement."""
    U, K, V, T, eos = case["U"], case["K"], case["V"], case["T"], case["eos"]
    Tb = np.repeat(case["Tb"].astype(np.int64), K)
    y64 = log_softmax(case["z"][:, :, :V + 1], np.float64)
    yr = np.repeat(y64, K, axis=0)
    st = empty_state(yr, Tb)
    for j in range(4):
        has = np.array([len(p) > j for p in case["prefixes"]])
        ext = extend(yr, Tb, st, np.array([p[j] if len(p) > j else 0 for p in case["prefixes"]]))
        st = {k: np.where(has.reshape((-1,) + (1,) * (v.ndim - 1)), ext[k], v) for k, v in st.items()}
    start = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in st.items()}
    y = log_softmax(case["z"][:, :, :V + 1].astype(dt), dt)
    yd = np.repeat(y, K, axis=0)
    cur = {k: (v.astype(dt) if v.dtype == np.float32 else v) for k, v in start.items()}
    outs = []
    for s, (tok, par, fin) in enumerate(case["steps"]):
        cur, tm = step(yd, Tb, cur, tok, par, fin, s + 1, eos)
        outs.append(({k: v.copy() for k, v in cur.items()}, tm, psi_ext(yd, Tb, cur, eos)))
    return y, start, outs


def deviation(got, ref, Tb, what=""):
    """got / ref: (state dict, term[, psi_ext]).  Checks that the -inf patterns of state (t < T_b), psi and term agree EXACTLY and that
    `last` is equal; returns the worst |got - ref| / (2^-23 * scale) over the finite values, scale = max(1, max |finite reference
    value|) taken over the state for the state, and over psi(g) and every psi(g . v) for psi and term."""
    (gs, gt), (rs, rt, rpe) = got[:2], ref
    m = _tmask(Tb, rs["rn"].shape[1])
    assert np.array_equal(gs["last"], rs["last"]), what
    worst = 0.0
    fin_abs = lambda a: float(np.abs(a[np.isfinite(a)]).max()) if np.isfinite(a).any() else 0.0
    s_state = max(1.0, fin_abs(rs["rn"][m]), fin_abs(rs["rb"][m]))
    s_psi = max(1.0, fin_abs(rs["psi"]), fin_abs(rpe))
    for name, g, r, sc in (("rn", gs["rn"][m], rs["rn"][m], s_state), ("rb", gs["rb"][m], rs["rb"][m], s_state),
                           ("psi", gs["psi"], rs["psi"], s_psi), ("term", gt, rt, s_psi)):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        assert not np.isnan(g).any(), (what, name)
        assert np.array_equal(np.isneginf(g), np.isneginf(r)) and not np.isposinf(g).any(), (what, name, "-inf pattern")
        f = np.isfinite(r)
        if f.any():
            worst = max(worst, float(np.abs(g[f] - r[f]).max()) / (2.0 ** -23 * sc))
    return worst

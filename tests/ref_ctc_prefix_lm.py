"""References for the CTC prefix beam search with a fused language model (include/avsr_hip.h avsr_ctc_prefix_search_lm, INTEGRATION.md
section 8).  The rule is written once, literally, over ref_ctc_prefix's `select` / `log_softmax` / `lae` and a dtype:

    extend g by c < V while len(g) < L_max:  next[g.c].p_nb (+)= (p_b if c == last(g) else p) + y[t][c] + (w * lam(c | g) + beta)
    stays, merging, candidate indices, selection on p, ties, "p = -inf is never kept": ref_ctc_prefix's
    after the last frame: final[g] = p + w * lam(EOS | g), the beam re-sorted by final, descending, ties to the earlier slot
    s_lm[g] = sum_i lam(g_i | g_0 .. g_{i-1}) + lam(EOS | g)

lam(. | g) is `ref_beam_lm.lm_step` (avsr.LM's evaluate graph in the oracle's cells) fed GO, g_0 .. g_{n-1} from the zero state, memoised
per label tuple (class `LM`).  float64 is the reference; the float32 form (the search in np.float32 over an LM evaluated in torch.float32)
is a RESTATEMENT used only to size tolerances.  Nothing here knows how the kernel stores the model's state.

`check_trace_lm` follows the ENGINE's branch frame by frame, as ref_ctc_prefix.check_trace does: candidates in fp64 from the engine's own
(p_b, p_nb) and the fp64 lam; then the final re-sort, s_lm, and lm_steps == the number of trace frames with a kept symbol < V.

Tolerances: 8 x what the float32 restatement measured on the tests' inputs (`measure_tolerances` reproduces the numbers) plus the
language model's share.  1e-4 is the project's parity target for the engine's lm_logp (tests/test_gpu_beam_lm.py), so a quantity that
holds n lam terms may move by w * 1e-4 * n:
    one frame from the engine's own state   one term per candidate             TOL_STEP_LM (or _LONG) + w * 1e-4
    final = p + w lam(EOS | g) from the engine's own p                         the same
    a whole search's final score            len(g) + 1 terms                   TOL_SEARCH_LM + w * 1e-4 * (len(g) + 1)
    TOL_STEP_LM       T <= 40 kernel inputs, all three LMs, both (w, beta): measured 1.28e-05
    TOL_STEP_LM_LONG  the T = 300 inputs (|p| reaches 1.4e3):               measured 1.15e-04
    TOL_SEARCH_LM     final scores over the compared seeds of 0..63 of the four whole-search configurations, both LMs, w = beta = 0.5:
                      measured 6.63e-05
Separately the debug lm_logp rows and s_lm of the kernel are held to 1e-4 and (len + 1) * 1e-4 against fp64 recomputation from the
returned ids: this is what catches a state that followed the wrong slot."""
import numpy as np
import torch

import ref_beam_lm as RB
import ref_ctc_prefix as R

NEG = -np.inf
LM_PARITY = 1e-4
TOL_STEP_LM = 8 * 1.28e-05
TOL_STEP_LM_LONG = 8 * 1.15e-04
TOL_SEARCH_LM = 8 * 6.63e-05

# (V, T, W, L_max, s): ref_ctc_prefix's shapes with V <= 64 and W <= 16 in the fifth; s of the width-10 searches raised so that the
# fp64 reference alone leaves out at most a third of 64 seeds under the fused rule
SEARCH_CONFIGS = [(15, 24, 4, 12, 2), (31, 40, 10, 16, 4), (41, 40, 10, 16, 5), (31, 40, 1, 16, 2)]
KERNEL_CONFIGS = SEARCH_CONFIGS + [(64, 8, 16, 8, 2), (20, 300, 4, 40, 2)]
LM_SHAPES = {"1x12e8": (1, 12, 8, False), "2x64e8": (2, 64, 8, False), "1x12onehot": (1, 12, 0, True)}      # (layers, H, E, one_hot)
WEIGHTS = [(0.5, 0.5), (0.3, 0.0)]


def lm_params(name, V, seed=31):
    """Random model in TF layout (what tests/test_gpu_beam_lm.py's step test draws): (P, layers, H, E, one_hot); one-hot rows are
    np.eye(V, E) with E = V rounded up to 4, the table the engine keeps for embedding_size <= 0."""
    nl, H, E, one_hot = LM_SHAPES[name]
    rng = np.random.default_rng(seed + 7 * V + nl + H)
    if one_hot:
        E = (V + 3) // 4 * 4
    P = {"dec/embedding": np.eye(V, E, dtype=np.float32) if one_hot else rng.standard_normal((V, E)).astype(np.float32)}
    for j in range(nl):
        kin = (E if j == 0 else H) + H
        P["dec/l%d/kernel" % j] = (rng.standard_normal((kin, 4 * H)) * (1.5 / np.sqrt(kin))).astype(np.float32)
        P["dec/l%d/bias" % j] = (rng.standard_normal(4 * H) * 0.3).astype(np.float32)
    P["dec/out/kernel"] = (rng.standard_normal((H, V)) * (3.0 / np.sqrt(H))).astype(np.float32)
    P["dec/out/bias"] = rng.standard_normal(V).astype(np.float32)
    return P, nl, H, E, one_hot


class LM:
    """lam(. | g) [V] per label tuple, memoised together with the state it leaves."""

    def __init__(self, P, nl, H, V, go_id, eos_id, dtype=torch.float64):
        self.P = {k: torch.as_tensor(v).to(dtype) for k, v in P.items()}
        self.V, self.go, self.eos, self.dtype = V, int(go_id), int(eos_id), dtype

        class Cfg:
            decoder_units, vocab_size = (H,) * nl, V
        self.cfg = Cfg
        self.memo = {}

    def _node(self, g):
        e = self.memo.get(g)
        if e is None:
            if g:
                state, tok = self._node(g[:-1])[1], g[-1]
            else:
                state, tok = RB.lm_zero_state(self.cfg, 1, self.dtype), self.go
            with torch.no_grad():
                lp, new = RB.lm_step(self.P, self.cfg, torch.as_tensor([tok]), state)
            e = self.memo[g] = (lp[0].numpy(), new)
        return e

    def lam(self, g):
        return self._node(tuple(g))[0]

    def s_lm(self, g):
        g = tuple(g)
        return float(sum(float(self.lam(g[:i])[g[i]]) for i in range(len(g))) + float(self.lam(g)[self.eos]))


_LMS = {}


def shared_lm(name, V, dtype=torch.float64):
    """One LM (and one memo) per (shape, V, dtype) for all tests; GO = V - 1, EOS = V - 2 as in the project's unit lists."""
    key = (name, V, dtype)
    if key not in _LMS:
        P, nl, H, E, one_hot = lm_params(name, V)
        _LMS[key] = (LM(P, nl, H, V, V - 1, V - 2, dtype), P, nl, H, E, one_hot)
    return _LMS[key]


def frame_lm(beam, yt, L_max, lm, w, beta, dt=np.float64):
    """ref_ctc_prefix.frame with the term: {labels: [p_b, p_nb, candidate index]}."""
    C = len(yt)
    V = C - 1
    yt = np.asarray(yt, dt)
    neg = dt(NEG)
    w, beta = dt(w), dt(beta)
    nxt = {}

    def add(g, which, val, idx, stay):
        e = nxt.get(g)
        if e is None:
            e = nxt[g] = [neg, neg, idx]
        elif stay:
            e[2] = idx                                    # a merged entry takes its stay index
        e[which] = R.lae(e[which], val)

    for k, (g, pb, pnb) in enumerate(beam):
        pb, pnb = dt(pb), dt(pnb)
        p = R.lae(pb, pnb)
        add(g, 0, p + yt[V], k * C + V, True)
        if g:
            add(g, 1, pnb + yt[g[-1]], k * C + V, True)
        if len(g) < L_max:
            lam = np.asarray(lm.lam(g), dt)
            for c in range(V):
                add(g + (c,), 1, (pb if (g and c == g[-1]) else p) + yt[c] + (w * lam[c] + beta), k * C + c, False)
    return nxt


def finals(beam, lm, w, dt=np.float64):
    """[(g, final)] of a beam [(g, p_b, p_nb)], re-sorted by final descending, ties to the earlier slot."""
    rows = [(g, dt(R.lae(dt(pb), dt(pnb))) + dt(w) * dt(lm.lam(g)[lm.eos])) for g, pb, pnb in beam]
    order = sorted(range(len(rows)), key=lambda r: (-rows[r][1], r))
    return [rows[r] for r in order]


def search_lm(z, Tb, W, L_max, lm, w, beta, dt=np.float64):
    """The fused rule on one utterance's logits z [T, V + 1].  dict(beam=[(g, final)] sorted by final, margin=smallest gap between the
    last kept and the best rejected candidate over the frames and between the two largest finals, beams=the per-frame beams)."""
    z = np.asarray(z)
    Tb = min(max(int(Tb), 0), z.shape[0])
    y = R.log_softmax(z[:Tb], dt)
    beam = [((), dt(0), dt(NEG))]
    margin = np.inf
    beams = [beam]
    for t in range(Tb):
        kept, ps, rej = R.select(frame_lm(beam, y[t], L_max, lm, w, beta, dt), W)
        if rej > NEG:
            margin = min(margin, float(ps[-1]) - float(rej))
        beam = kept
        beams.append(beam)
    out = finals(beam, lm, w, dt)
    if len(out) > 1:
        margin = min(margin, float(out[0][1]) - float(out[1][1]))
    return dict(beam=out, margin=margin, beams=beams)


def step_deviation_lm(z, Tb, W, L_max, lm64, lm32, w, beta):
    """Largest |fp32 - fp64| of any finite candidate's p_b / p_nb over the frames, each frame started from the fp64 search's beam."""
    z = np.asarray(z)
    Tb = min(max(int(Tb), 0), z.shape[0])
    y64, y32 = R.log_softmax(z[:Tb]), R.log_softmax(z[:Tb].astype(np.float32), np.float32)
    beam, dev = [((), 0.0, NEG)], 0.0
    for t in range(Tb):
        c64 = frame_lm(beam, y64[t], L_max, lm64, w, beta)
        c32 = frame_lm([(g, np.float32(a), np.float32(b)) for g, a, b in beam], y32[t], L_max, lm32, w, beta, np.float32)
        for g, e in c64.items():
            for i in (0, 1):
                if e[i] > NEG:
                    dev = max(dev, abs(float(c32[g][i]) - float(e[i])))
        beam = [(g, float(np.float32(a)), float(np.float32(b))) for g, a, b in R.select(c64, W)[0]]
    return dev


def search_deviation_lm(z, Tb, W, L_max, lm64, lm32, w, beta):
    """Largest |fp32 - fp64| final score over the label sequences both searches end with."""
    a = search_lm(z, Tb, W, L_max, lm64, w, beta)
    b = search_lm(np.asarray(z, np.float32), Tb, W, L_max, lm32, w, beta, np.float32)
    fb = dict(b["beam"])
    return max([abs(float(fb[g]) - float(p)) for g, p in a["beam"] if g in fb] or [0.0])


def check_trace_lm(z, Tb, W, L_max, parent, sym, pb, pnb, lm, w, beta, tol):
    """ref_ctc_prefix.check_trace under the fused rule (tol already holds the language model's share of one term).  Returns
    (the final beam [(g, p_b, p_nb)] with the engine's numbers in slot order, the number of frames that kept a symbol < V)."""
    z = np.asarray(z, np.float64)
    C = z.shape[1]
    V = C - 1
    Tb = min(max(int(Tb), 0), z.shape[0])
    y = R.log_softmax(z[:Tb])
    beam = [((), 0.0, NEG)]
    steps = 0

    def close(a, b):
        return (a == NEG and b == NEG) or (a > NEG and b > NEG and abs(a - b) <= tol)

    for t in range(Tb):
        cands = frame_lm(beam, y[t], L_max, lm, w, beta)
        new, used, ps = [], set(), []
        stepped = False
        for r in range(W):
            k, c = int(parent[t, r]), int(sym[t, r])
            if k < 0:
                assert c == -1 and pb[t, r] == NEG and pnb[t, r] == NEG, (t, r)
                assert (parent[t, r:] == -1).all(), ("an empty slot before a filled one", t, r)
                break
            assert 0 <= k < len(beam) and 0 <= c <= V, (t, r, k, c)
            g = beam[k][0] if c == V else beam[k][0] + (c,)
            assert c == V or len(beam[k][0]) < L_max, ("extension past L_max", t, r)
            assert g in cands and g not in used, ("duplicate or unknown label sequence", t, r, g)
            assert cands[g][2] == k * C + c, ("a merged entry must be reported as its stay", t, r, g)
            used.add(g)
            stepped |= c < V
            eb, enb = float(pb[t, r]), float(pnb[t, r])
            assert not np.isnan(eb) and not np.isnan(enb)
            assert close(eb, float(cands[g][0])) and close(enb, float(cands[g][1])), (t, r, g, eb, enb, cands[g])
            p = float(R.lae(eb, enb))
            assert p > NEG, ("p = -inf kept", t, r)
            assert not ps or p <= ps[-1] + tol, ("selection order", t, r)
            ps.append(p)
            new.append((g, eb, enb))
        rest = [float(R.lae(e[0], e[1])) for g, e in cands.items() if g not in used]
        best = max(rest, default=NEG)
        if len(new) < W:
            assert best == NEG, ("a finite candidate left out of a beam that is not full", t, best)
        else:
            assert best <= ps[-1] + tol, ("a rejected candidate beats the lowest kept one", t, best, ps[-1])
        beam = new
        steps += int(stepped)
    return beam, steps


def check_final_lm(got, s_lm, final_beam, lm, w, tol):
    """got [(g, final)] in the kernel's output order and s_lm per entry, against the engine's own last beam [(g, p_b, p_nb)] (slot order):
    the same label sequences, final = p + w lam(EOS | g) within tol, output sorted by the engine's final with equal finals in slot order,
    no inversion of the fp64 finals beyond 2 tol, and s_lm within (len + 1) * 1e-4 of the fp64 sum."""
    slot = {g: r for r, (g, _a, _b) in enumerate(final_beam)}
    assert sorted(slot) == sorted(g for g, _f in got) and len(got) == len(final_beam)
    ref = {g: float(R.lae(a, b)) + w * float(lm.lam(g)[lm.eos]) for g, a, b in final_beam}
    for r, (g, f) in enumerate(got):
        assert abs(f - ref[g]) <= tol, ("final", r, g, f, ref[g])
        assert abs(float(s_lm[r]) - lm.s_lm(g)) <= (len(g) + 1) * LM_PARITY, ("s_lm", r, g, float(s_lm[r]), lm.s_lm(g))
        if r:
            g0, f0 = got[r - 1]
            assert f0 > f or (f0 == f and slot[g0] < slot[g]), ("re-sort order", r)
            assert ref[g0] >= ref[g] - 2 * tol, ("re-sort against fp64", r)


def measure_tolerances():
    """Reproduces the measured numbers of the docstring (some minutes of Python; not run by the tests)."""
    step = {False: 0.0, True: 0.0}
    for V, T, W, L, s in KERNEL_CONFIGS:
        for name in LM_SHAPES:
            lm64, lm32 = shared_lm(name, V)[0], shared_lm(name, V, torch.float32)[0]
            for shift in R.BLANK_SHIFTS:
                for w, beta in WEIGHTS:
                    step[T > 40] = max(step[T > 40], step_deviation_lm(R.kernel_inputs(V, T, s, 0, shift), T, W, L, lm64, lm32, w, beta))
    srch, left = 0.0, {}
    for V, T, W, L, s in SEARCH_CONFIGS:
        for name in ("1x12e8", "2x64e8"):
            lm64, lm32 = shared_lm(name, V)[0], shared_lm(name, V, torch.float32)[0]
            out = 0
            for seed in range(64):
                z = R.kernel_inputs(V, T, s, seed)
                ref = search_lm(z, T, W, L, lm64, 0.5, 0.5)
                tol = TOL_SEARCH_LM + 0.5 * LM_PARITY * (max(len(g) for g, _p in ref["beam"]) + 1)
                if ref["margin"] > tol:
                    srch = max(srch, search_deviation_lm(z, T, W, L, lm64, lm32, 0.5, 0.5))
                else:
                    out += 1
            left[(V, T, W, L, s, name)] = out
    return step[False], step[True], srch, left


if __name__ == "__main__":
    a, b, c, left = measure_tolerances()
    print("one-frame deviation %.3g (T <= 40), %.3g (T = 300); final-score deviation %.3g" % (a, b, c))
    print("left out by the reference alone:", left)

"""References for the CTC prefix beam search (include/avsr_hip.h avsr_ctc_prefix_search).

The search is written once, literally as the rule states it -- a dictionary keyed by label TUPLES per frame -- over a dtype: float64 is
the reference, float32 a RESTATEMENT of the same arithmetic that is used only to size tolerances (how far an fp32 evaluation of this
rule lies from fp64 on the inputs the tests use).  Nothing here knows how the kernel finds equal label sequences.

    y[t][c] = log_softmax(z[t, :V + 1])[c], blank = class V;  a beam is an ordered list of (g, p_b, p_nb), g a tuple over the V classes;
    candidate index of slot k: k (V + 1) + V for its stay, k (V + 1) + c for its extension by c; a merged entry takes its stay index;
    the new beam: the W entries of largest p = p_b (+) p_nb, p = -inf never kept, ties to the lower index, in that order.

`check_trace` follows the ENGINE's branch: from the kernel's trace it rebuilds the engine's beam at frame t - 1, recomputes every
candidate of frame t in fp64 from the engine's own (p_b, p_nb), and requires the kept entries to match and no rejected candidate to beat
the lowest kept one.  It therefore checks every frame of every input whatever the margins are.

Tolerances: 8 x what the float32 restatement measured (`measure_tolerances` below reproduces the numbers; the margin covers another
order of the (+) terms and another expf / logf):
    TOL_STEP       one frame from the same state: the largest deviation of any finite candidate's p_b / p_nb over the kernel-level
                   inputs of tests/test_gpu_ctc_prefix.py with T <= 40 (|p| up to 170, one fp32 ulp there is 1.5e-5): measured 1.05e-5.
    TOL_STEP_LONG  the same on the T = 300 inputs, where |p| reaches 1.3e3 (one ulp 1.2e-4): measured 1.11e-4.
    TOL_SEARCH     final scores of a whole search: the largest deviation over the compared seeds of 0..63 of the four whole-search
                   configurations, on the label sequences both searches end with: measured 4.99e-5."""
import numpy as np

NEG = -np.inf
TOL_STEP = 8 * 1.05e-5
TOL_STEP_LONG = 8 * 1.11e-4
TOL_SEARCH = 8 * 4.99e-5


def log_softmax(z, dt=np.float64):
    z = np.asarray(z).astype(dt)
    m = z.max(axis=-1, keepdims=True)
    return (z - (m + np.log(np.sum(np.exp(z - m), axis=-1, keepdims=True, dtype=dt)))).astype(dt)


def lae(a, b):
    """log-add-exp; (-inf) (+) (-inf) = -inf, never NaN."""
    return np.logaddexp(a, b)


def frame(beam, yt, L_max, dt=np.float64):
    """All candidates of one frame: {labels: [p_b, p_nb, candidate index]} from a beam [(g, p_b, p_nb)] and the frame's row yt [V + 1]."""
    C = len(yt)
    V = C - 1
    yt = np.asarray(yt, dt)
    neg = dt(NEG)
    nxt = {}

    def add(g, which, val, idx, stay):
        e = nxt.get(g)
        if e is None:
            e = nxt[g] = [neg, neg, idx]
        elif stay:
            e[2] = idx                                    # a merged entry takes its stay index
        e[which] = lae(e[which], val)

    for k, (g, pb, pnb) in enumerate(beam):
        pb, pnb = dt(pb), dt(pnb)
        p = lae(pb, pnb)
        add(g, 0, p + yt[V], k * C + V, True)
        if g:
            add(g, 1, pnb + yt[g[-1]], k * C + V, True)
        if len(g) < L_max:
            for c in range(V):
                add(g + (c,), 1, (pb if (g and c == g[-1]) else p) + yt[c], k * C + c, False)
    return nxt


def select(cands, W):
    """(kept [(g, p_b, p_nb)], their p, p of the best rejected finite candidate or -inf)."""
    rows = sorted(((-lae(e[0], e[1]), e[2], g) for g, e in cands.items() if lae(e[0], e[1]) > NEG), key=lambda r: (r[0], r[1]))
    kept = [(g, cands[g][0], cands[g][1]) for _mp, _i, g in rows[:W]]
    return kept, [-r[0] for r in rows[:W]], (-rows[W][0] if len(rows) > W else NEG)


def search(z, Tb, W, L_max, dt=np.float64):
    """The rule on one utterance's logits z [T, >= V + 1 columns already cut to V + 1].  Returns dict(beam=[(g, p)] sorted,
    margin=smallest gap between the last kept and the best rejected candidate over the frames and between the final top two,
    replaced=True if some frame kept g . c while g, kept a frame earlier, was not (and so on: see `reentered`))."""
    z = np.asarray(z)
    T = z.shape[0]
    Tb = min(max(int(Tb), 0), T)
    y = log_softmax(z[:Tb], dt)
    beam = [((), dt(0), dt(NEG))]
    margin = np.inf
    beams = [beam]
    for t in range(Tb):
        kept, ps, rej = select(frame(beam, y[t], L_max, dt), W)
        if rej > NEG:
            margin = min(margin, float(ps[-1]) - float(rej))
        beam = kept
        beams.append(beam)
    out = [(g, lae(pb, pnb)) for g, pb, pnb in beam]
    if len(out) > 1:
        margin = min(margin, float(out[0][1]) - float(out[1][1]))
    return dict(beam=out, margin=margin, beams=beams)


def reentered(beams):
    """Frames t at which a prefix g is in the beam, was NOT in the beam of frame t - 1 but was in an earlier one, while one of its
    one-symbol extensions g . c was in the beams of both t - 1 and t: the case a parent link alone merges wrongly."""
    hits = []
    seen = set()
    for t in range(1, len(beams)):
        prev, cur = {g for g, _a, _b in beams[t - 1]}, {g for g, _a, _b in beams[t]}
        for g in cur:
            if g not in prev and g in seen and any(h[:-1] == g and h in prev for h in cur if h):
                hits.append((t, g))
        seen |= prev
    return hits


def step_deviation(z, Tb, W, L_max):
    """Largest |fp32 - fp64| of any finite candidate's p_b / p_nb over the frames, each frame started from the fp64 search's beam."""
    z = np.asarray(z)
    Tb = min(max(int(Tb), 0), z.shape[0])
    y64, y32 = log_softmax(z[:Tb]), log_softmax(z[:Tb].astype(np.float32), np.float32)
    beam, dev = [((), 0.0, NEG)], 0.0
    for t in range(Tb):
        c64 = frame(beam, y64[t], L_max)
        c32 = frame([(g, np.float32(a), np.float32(b)) for g, a, b in beam], y32[t], L_max, np.float32)
        for g, e in c64.items():
            for w in (0, 1):
                if e[w] > NEG:
                    dev = max(dev, abs(float(c32[g][w]) - float(e[w])))
        beam = [(g, float(np.float32(a)), float(np.float32(b))) for g, a, b in select(c64, W)[0]]      # states the kernel could hold
    return dev


def search_deviation(z, Tb, W, L_max):
    """Largest |fp32 - fp64| final score over the label sequences both searches end with."""
    a, b = search(z, Tb, W, L_max), search(np.asarray(z, np.float32), Tb, W, L_max, np.float32)
    fb = dict(b["beam"])
    return max([abs(float(fb[g]) - float(p)) for g, p in a["beam"] if g in fb] or [0.0])


def check_trace(z, Tb, W, L_max, parent, sym, pb, pnb, tol=TOL_STEP):
    """Follow the engine's branch through its trace (parent / sym / pb / pnb [T, W] of ONE utterance; z [T, V + 1]).  Asserts, per frame:
    every kept slot names a candidate that exists (a distinct label sequence, by the index the rule gives it), its (p_b, p_nb) match the
    fp64 recomputation from the engine's previous beam within tol, the slots are in selection order, and no candidate that was not kept
    lies above the lowest kept p by more than tol (none at all is finite if the beam is not full).  Returns the final beam [(g, p_b, p_nb)]
    with the engine's numbers."""
    z = np.asarray(z, np.float64)
    C = z.shape[1]
    V = C - 1
    Tb = min(max(int(Tb), 0), z.shape[0])
    y = log_softmax(z[:Tb])
    beam = [((), 0.0, NEG)]

    def close(a, b):
        return (a == NEG and b == NEG) or (a > NEG and b > NEG and abs(a - b) <= tol)

    for t in range(Tb):
        cands = frame(beam, y[t], L_max)
        new, used, ps = [], set(), []
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
            eb, enb = float(pb[t, r]), float(pnb[t, r])
            assert not np.isnan(eb) and not np.isnan(enb)
            assert close(eb, float(cands[g][0])) and close(enb, float(cands[g][1])), (t, r, g, eb, enb, cands[g])
            p = float(lae(eb, enb))
            assert p > NEG, ("p = -inf kept", t, r)
            assert not ps or p <= ps[-1] + tol, ("selection order", t, r)
            ps.append(p)
            new.append((g, eb, enb))
        rest = [float(lae(e[0], e[1])) for g, e in cands.items() if g not in used]
        best = max(rest, default=NEG)
        if len(new) < W:
            assert best == NEG, ("a finite candidate left out of a beam that is not full", t, best)
        else:
            assert best <= ps[-1] + tol, ("a rejected candidate beats the lowest kept one", t, best, ps[-1])
        beam = new
    return beam


def brute_force(y):
    """{labels: log p(labels | x)} over ALL (V + 1)^T alignments of y [T, V + 1] (tiny T only)."""
    import itertools
    T, C = y.shape
    tot = {}
    for path in itertools.product(range(C), repeat=T):
        seq, prev = [], -1
        for k in path:
            if k != prev and k != C - 1:
                seq.append(k)
            prev = k
        lp = float(sum(y[t, k] for t, k in enumerate(path)))
        g = tuple(seq)
        tot[g] = np.logaddexp(tot.get(g, NEG), lp)
    return tot


def kernel_inputs(V, T, s, seed, blank_shift=0.0):
    """The tests' logits: z = default_rng(seed).normal(0, s, (T, V + 1)), float32; blank_shift is added to the blank column."""
    z = np.random.default_rng(seed).normal(0, s, (T, V + 1))
    z[..., V] += blank_shift
    return z.astype(np.float32)


SEARCH_CONFIGS = [(15, 24, 4, 12, 2), (31, 40, 10, 16, 2), (41, 40, 10, 16, 3), (31, 40, 1, 16, 2)]      # (V, T, W, L_max, s)
KERNEL_CONFIGS = SEARCH_CONFIGS + [(256, 8, 64, 8, 2), (20, 300, 4, 40, 2)]
BLANK_SHIFTS = (0.0, 3.0, 8.0)            # + 8: the blank wins most frames, so the beam's lengths spread well below L_max


def measure_tolerances():
    """Reproduces the measured numbers of the docstring (half a minute of Python; not run by the tests)."""
    step = {False: 0.0, True: 0.0}
    for V, T, W, L, s in KERNEL_CONFIGS:
        for shift in BLANK_SHIFTS:
            step[T > 40] = max(step[T > 40], step_deviation(kernel_inputs(V, T, s, 0, shift), T, W, L))
    srch = 0.0
    for V, T, W, L, s in SEARCH_CONFIGS:
        for seed in range(64):
            z = kernel_inputs(V, T, s, seed)
            if search(z, T, W, L)["margin"] > TOL_SEARCH:
                srch = max(srch, search_deviation(z, T, W, L))
    return step[False], step[True], srch


if __name__ == "__main__":
    print("one-frame deviation %.3g (T <= 40), %.3g (T = 300); final-score deviation %.3g" % measure_tolerances())

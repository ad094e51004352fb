"""References for the CTC forced alignment (include/avsr_hip.h avsr_ctc_align).

The rule is written once, vectorised over the 2U + 1 states, over a dtype: float64 is the reference, float32 a RESTATEMENT of the same
arithmetic -- log-softmax rows in float32, one float32 accumulator per state, no shift -- that is used only to size tolerances (how far a
plain fp32 evaluation of this rule lies from fp64 on the inputs the tests use).  Nothing here knows how the kernel stores backpointers.

    y[t][c] = log_softmax(z[t, :V + 1])[c], blank = class V;  states s = 0 .. 2U, even = blank, odd = g[(s - 1) / 2]
    d[0][0] = y[0][V], d[0][1] = y[0][g[0]], else -inf
    d[t][s] = y[t][cls(s)] + max(d[t-1][s], d[t-1][s-1], d[t-1][s-2] if s odd, s >= 3 and g[(s-1)/2] != g[(s-3)/2])
    ties: the higher source state wins (stay, then s - 1, then s - 2); at the end the last blank wins over the last label.

`margin` is the gap between the optimum and the best alignment that differs from the returned one: any other alignment leaves the best
one at some (t, s), so it is best - max over (t, s) off the path of forward[t][s] + backward[t][s].  A path is compared with the
reference's only where that gap exceeds the tolerance -- an argmax is discontinuous at a tie; `check` leaves out nothing else.

Tolerances: 8 x the largest deviation of the float32 restatement's score from fp64 on the very inputs of the test configurations
(`measure_tolerances` below reproduces the numbers):
    TOL_ALIGN       T <= 64: the 64 seeds of each of SEED_CONFIGS, the mixed batch and every case of KERNEL_CASES and TIE_CASES with
                    T <= 64: measured 6.44e-5.
    TOL_ALIGN_LONG  longer inputs (T = 80 .. 1100 of KERNEL_CASES and TIE_CASES): measured 2.27e-3.
    TOL_LP          one log-softmax entry, float32 against fp64, over all those inputs: measured 7.25e-7."""
import numpy as np

NEG = -np.inf
TOL_ALIGN = 8 * 6.44e-5
TOL_ALIGN_LONG = 8 * 2.27e-3
TOL_LP = 8 * 7.25e-7
BLOCK = 128                                # frames per backtrace block of csrc/ctc_align.hip (CA_BLOCK): the T cases straddle it
MAX_L = 512


def tol_for(T):
    return TOL_ALIGN if T <= 64 else TOL_ALIGN_LONG


def log_softmax(z, dt=np.float64):
    z = np.asarray(z).astype(dt)
    m = z.max(axis=-1, keepdims=True)
    return (z - (m + np.log(np.sum(np.exp(z - m), axis=-1, keepdims=True, dtype=dt)))).astype(dt)


def repeats(g):
    g = list(g)
    return sum(1 for a, b in zip(g[1:], g[:-1]) if a == b)


def feasible(g, Tb, V):
    """avsr_ctc_loss's test: T_b >= 1, every label in 0 .. V-1, T_b >= U + adjacent equal pairs."""
    return bool(Tb >= 1 and all(0 <= int(c) < V for c in g) and Tb >= len(g) + repeats(g))


def _states(g, V):
    U = len(g)
    cls = np.full(2 * U + 1, V, np.int64)
    cls[1::2] = g
    skip = np.zeros(2 * U + 1, bool)
    for s in range(3, 2 * U + 1, 2):
        skip[s] = g[(s - 1) // 2] != g[(s - 3) // 2]
    return cls, skip


def collapse(path, V):
    seq, prev = [], -1
    for k in path:
        k = int(k)
        if k != prev and k != V:
            seq.append(k)
        prev = k
    return seq


def runs(path, V):
    """[(label, first frame, last frame)] of the label runs of a frame labelling."""
    out, prev = [], -1
    for t, k in enumerate(path):
        k = int(k)
        if k != V and k != prev:
            out.append([k, t, t])
        elif k != V:
            out[-1][2] = t
        prev = k
    return [tuple(r) for r in out]


def align(z, g, Tb, dt=np.float64, want_margin=False):
    """The rule on one utterance: z [T, V + 1] (already cut to the real classes), g the label list (no EOS).  Returns dict(status, score,
    path [T_b], states [T_b], start / end [U], frame_lp [T_b], and margin if asked for); status 0: no valid alignment, score 0."""
    z = np.asarray(z)
    T, C = z.shape
    V = C - 1
    g = [int(c) for c in g]
    U = len(g)
    Tb = min(max(int(Tb), 0), T)
    if not feasible(g, Tb, V):
        return dict(status=0, score=0.0, path=[], states=[], start=[], end=[], frame_lp=[], margin=np.inf)
    y = log_softmax(z[:Tb], dt)
    cls, skip = _states(g, V)
    S = 2 * U + 1
    neg = dt(NEG)
    d = np.full((Tb, S), neg, dt)
    bp = np.zeros((Tb, S), np.int8)
    d[0, 0] = y[0, V]
    if U > 0:
        d[0, 1] = y[0, g[0]]
    for t in range(1, Tb):
        p0 = d[t - 1]
        p1 = np.concatenate(([neg], p0[:-1]))
        p2 = np.where(skip, np.concatenate(([neg, neg], p0[:-2]))[:S], neg)
        best, k = p0.copy(), np.zeros(S, np.int8)
        k[p1 > best] = 1
        best = np.maximum(best, p1)
        k[p2 > best] = 2
        best = np.maximum(best, p2)
        d[t] = (y[t, cls] + best).astype(dt)
        bp[t] = k
    s = 2 * U
    if U > 0 and d[Tb - 1, 2 * U - 1] > d[Tb - 1, 2 * U]:
        s = 2 * U - 1
    score = float(d[Tb - 1, s])
    states = [0] * Tb
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    path = [int(cls[s]) for s in states]
    rr = runs(path, V)
    out = dict(status=1, score=score, path=path, states=states, start=[r[1] for r in rr], end=[r[2] for r in rr],
               frame_lp=[float(y[t, k]) for t, k in enumerate(path)])
    if want_margin:
        bw = np.full((Tb, S), neg, dt)                  # best completion from (t, s), the emission of frame t not included
        bw[Tb - 1, 2 * U] = 0
        if U > 0:
            bw[Tb - 1, 2 * U - 1] = 0
        for t in range(Tb - 2, -1, -1):
            n = y[t + 1, cls] + bw[t + 1]
            n1 = np.concatenate((n[1:], [neg]))
            n2 = np.concatenate((np.where(skip, n, neg)[2:], [neg, neg]))[:S]
            bw[t] = np.maximum(np.maximum(n, n1), n2)
        tot = d + bw
        tot[np.arange(Tb), states] = neg
        other = float(tot.max()) if tot.size else NEG
        out["margin"] = np.inf if other == NEG else score - other
    return out


def path_score(z, path):
    """fp64 log-probability of a frame labelling."""
    y = log_softmax(np.asarray(z)[:len(path)])
    return float(sum(y[t, int(k)] for t, k in enumerate(path)))


def check(z, g, Tb, got, tol, ref=None, lp_tol=TOL_LP):
    """What avsr_ctc_align returned for ONE utterance against the rule.  z [T, V + 1]; got: dict(status, score, path [T], frame_lp [T],
    start [L], end [L]) with the padding still on.  tol: the score tolerance, lp_tol: that of one frame_lp entry.  Asserts: the padding rules; the path has T_b frames,
    collapses to the target, starts and ends legally; frame_lp is y along it; start / end are its runs; the fp64 score of the returned
    path is within tol of the fp64 optimum (for EVERY input) and `score` within tol of it; the path equals the reference's wherever the
    margin exceeds tol.  Returns (reference, compared)."""
    z = np.asarray(z, np.float64)
    T, C = z.shape
    V = C - 1
    g = [int(c) for c in g]
    U = len(g)
    Tb = min(max(int(Tb), 0), T)
    ref = ref or align(z, g, Tb, want_margin=True)
    path, lp = np.asarray(got["path"]), np.asarray(got["frame_lp"])
    start, end = np.asarray(got["start"]), np.asarray(got["end"])
    assert path.shape == (T,) and lp.shape == (T,) and start.shape == end.shape
    assert not np.isnan(lp).any() and not np.isnan(got["score"])
    assert int(got["status"]) == ref["status"], (got["status"], ref["status"])
    if not ref["status"]:
        assert got["score"] == 0.0 and (path == -1).all() and (lp == 0.0).all() and (start == -1).all() and (end == -1).all()
        return ref, False
    assert (path[Tb:] == -1).all() and (lp[Tb:] == 0.0).all(), "padding past T_b"
    assert (start[U:] == -1).all() and (end[U:] == -1).all(), "padding past U"
    p = [int(k) for k in path[:Tb]]
    assert all(0 <= k <= V for k in p), "a frame without a class"
    assert collapse(p, V) == g, ("the path does not collapse to the target", collapse(p, V), g)
    assert p[0] == V or p[0] == g[0], "illegal first frame"
    assert p[-1] == V or p[-1] == g[-1], "illegal last frame"
    y = log_softmax(z[:Tb])
    want_lp = y[np.arange(Tb), p]
    assert np.abs(lp[:Tb] - want_lp).max() <= lp_tol, "frame_lp is not y along the path"
    rr = runs(p, V)
    assert [r[0] for r in rr] == g
    assert [int(v) for v in start[:U]] == [r[1] for r in rr], ("start", list(start[:U]), rr)
    assert [int(v) for v in end[:U]] == [r[2] for r in rr], ("end", list(end[:U]), rr)
    ps = float(want_lp.sum())
    assert ps <= ref["score"] + 1e-9 * max(1.0, abs(ref["score"])), "a path better than the optimum"
    assert ps >= ref["score"] - tol, ("the returned path is not optimal", ps, ref["score"])
    assert abs(float(got["score"]) - ps) <= tol, ("score", got["score"], ps)
    assert abs(float(got["score"]) - ref["score"]) <= tol, ("score", got["score"], ref["score"])
    if ref["margin"] > tol:
        assert p == ref["path"], "the path differs from the reference's although the margin exceeds the tolerance"
        return ref, True
    return ref, False


def brute_force(y, g):
    """(best score, its frame labelling) over ALL (V + 1)^T labellings of y [T, V + 1] that collapse to g (tiny T only); (-inf, None)
    where there is none."""
    import itertools
    T, C = y.shape
    best, arg = NEG, None
    for path in itertools.product(range(C), repeat=T):
        if collapse(path, C - 1) != list(g):
            continue
        lp = float(sum(y[t, k] for t, k in enumerate(path)))
        if lp > best:
            best, arg = lp, list(path)
    return best, arg


# ---- the tests' inputs ------------------------------------------------------------------------------------------------------------
def logits(V, T, seed, s=1.0):
    """z = default_rng(seed).normal(0, s, (T, V + 1)), float32."""
    return np.random.default_rng(seed).normal(0, s, (T, V + 1)).astype(np.float32)


def labels(V, U, seed, kind="rand"):
    """'rand': uniform labels (adjacent repeats as they fall); 'equal': one label U times; 'rep': every second label repeats its
    predecessor."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "equal":
        return [int(rng.integers(V))] * U
    g = [int(c) for c in rng.integers(0, V, U)]
    if kind == "rep":
        for j in range(1, U, 2):
            g[j] = g[j - 1]
    return g


SEED_CONFIGS = [(5, 12, 4), (30, 40, 12), (30, 64, 31)]                 # (V, T, U): 64 seeds each, path equality
# (V, T, L, U, T_b, kind); T_b = None: T; T_b = 'min': U + repeats (one alignment only)
KERNEL_CASES = [(30, 150, 66, U, None, "rand") for U in (0, 1, 31, 32, 33, 63, 64, 65)] + [
    (30, 80, 20, 20, None, "rand"),                                      # U = L
    (5, 12, 4, 1, 1, "rand"), (5, 12, 4, 0, 1, "rand"),                  # T_b = 1
    (5, 40, 12, 12, "min", "rep"), (30, 40, 12, 12, "min", "rand"),      # T_b = U + repeats
    (30, 40, 12, 12, 29, "rand"),                                        # T_b < T
    (20, BLOCK - 1, 12, 10, None, "rand"), (20, BLOCK, 12, 10, None, "rand"), (20, BLOCK + 1, 12, 10, None, "rand"),
    (20, 2 * BLOCK + 1, 12, 10, None, "rand"),
    (5, 40, 10, 10, None, "equal"), (5, 40, 10, 10, "min", "equal"),     # all-equal labels
    (40, 500, 40, 40, None, "rand"),                                     # long
    (30, 1100, MAX_L, MAX_L, None, "rand"),                              # at the limit
]


def case_inputs(case, seed=0):
    """(z [T, V + 1] float32, g, T_b) of a KERNEL_CASES entry."""
    V, T, _L, U, Tb, kind = case
    g = labels(V, U, seed, kind)
    Tb = T if Tb is None else (U + repeats(g) if Tb == "min" else Tb)
    return logits(V, T, seed + 7 * U + T), g, Tb


TIE_CASES = [(3, 5, 2, "rand"), (7, 40, 9, "rep"), (30, 150, 65, "rand"), (5, 2 * BLOCK + 1, 10, "equal")]      # (V, T, U, kind)


def tie_inputs(V, T, U, kind):
    """Row-constant logits: every class of a frame is equally probable, so every comparison of the rule is an exact tie."""
    z = np.repeat(np.random.default_rng(V + T).normal(0, 1, (T, 1)).astype(np.float32), V + 1, axis=1)
    return z, labels(V, U, 0, kind), T


def mixed_batch():
    """(V, T, L, clean logits [B, T, V + 1], label lists, target_len, in_len) of the GPU test's mixed batch: too few frames for the
    repeats (3), T_b = 0 (1), a label out of range (4), T_b < T, T_b > T, target_len > L and < 0 (both clamped)."""
    V, T, L = 30, 40, 12
    gs = [labels(V, 12, 1), labels(V, 7, 2), labels(V, 5, 3), labels(V, 12, 4, "rep"), [3, V, 5], labels(V, 12, 6), []]
    return V, T, L, np.stack([logits(V, T, 200 + b) for b in range(len(gs))]), gs, [12, 7, 5, 12, 3, L + 7, -4], [T, 0, 23, 12, T, T + 9, 5]


def measure_tolerances():
    """Reproduces the measured numbers of the docstring (a minute of Python; not run by the tests)."""
    dev, lp = {False: 0.0, True: 0.0}, 0.0

    def one(z, g, Tb):
        nonlocal lp
        a, b = align(z, g, Tb), align(z, g, Tb, np.float32)
        dev[z.shape[0] > 64] = max(dev[z.shape[0] > 64], abs(a["score"] - b["score"]))
        lp = max(lp, float(np.abs(log_softmax(z, np.float32).astype(np.float64) - log_softmax(z)).max()))

    for V, T, U in SEED_CONFIGS:
        for seed in range(64):
            one(logits(V, T, seed), labels(V, U, seed), T)
    for case in KERNEL_CASES:
        one(*case_inputs(case))
    for case in TIE_CASES:
        one(*tie_inputs(*case))
    _V, _T, _L, zs, gs, _tl, Tbs = mixed_batch()
    for z, g, Tb in zip(zs, gs, Tbs):
        one(z, g, Tb)
    return dev[False], dev[True], lp


if __name__ == "__main__":
    print("score deviation %.3g (T <= 64), %.3g (longer); log-softmax entry %.3g" % measure_tolerances())

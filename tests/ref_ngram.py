"""Reference for back-off n-gram language models (avsr-tf1_amd/ngram.py, csrc/ctc_prefix_ngram.hip) and the
models the n-gram tests share.

`NGramRef` is the textbook rule over the parsed n-gram lists, dictionaries only -- it knows nothing of the compiled automaton:

    h = the last N-1 symbols of (GO, g);   lam(c | h) = listed(h.c)  else  bow(h) + lam(c | h[1:]),  bow of an unlisted h = 0;
    an unlisted class at the empty context: FLOOR = -99 ln 10

with the interface tests/ref_ctc_prefix_lm.py's search takes (`lam(g)` [V], `s_lm(g)`, `eos`; GO = V - 1, EOS = V - 2).  float64 is the
reference.  The float32 form is a RESTATEMENT in the kernel's order (values rounded to float32 once; acc = 0, acc += bow per level left,
then acc + logp), used to size the tolerances -- and, since the kernel performs exactly these additions, equal to the kernel's rows bit
for bit on models whose contexts are all listed (the estimator's).

Tolerances, by the project's convention 8 x what the float32 restatement deviates from float64 on the tests' own inputs
(`measure_tolerances` reproduces the numbers):
    NGRAM_PARITY      |lam32 - lam64| over every context and class of the shared models (orders 1, 2, 4; V = 15, 20, 31, 41, 64, 256) and
                      the sparse one: measured 1.46e-05 -- one float32 ulp at |FLOOR| = 228 is 1.5e-5, and a floor reached through a
                      back-off weight is rounded once more.  8 x 1.46e-05 = 1.17e-04 takes the place of ref_ctc_prefix_lm.LM_PARITY
                      (1e-4) wherever a quantity holds lam terms: w * NGRAM_PARITY per term.
    TOL_STEP_LM / TOL_STEP_LM_LONG / TOL_SEARCH_LM are ref_ctc_prefix_lm's, reused as they are.  For the record, the float32
    restatement of the search under the shared n-grams (all three orders, both weight pairs, every blank shift) measured 1.96e-05 per
    frame at T <= 40 (the bound is 8 x 1.28e-05), 1.15e-04 at T = 300 (8 x 1.15e-04) and 7.71e-05 on final scores (8 x 6.63e-05).
Whole searches against the float64 rule leave out near-tie seeds (margin not above the tolerance).  With the shared Witten-Bell models
the float64 reference ALONE leaves out, of 64 seeds at w = beta = 0.5, orders (1, 2, 4):
    (15, 24, 4, 12, 2): 3, 0, 3    (31, 40, 10, 16, 4): 12, 14, 16    (41, 40, 10, 16, 5): 10, 16, 15    (31, 40, 1, 16, 2): 2, 3, 2
-- at most 64 // 3 = 21 everywhere (`left_out_by_the_reference`)."""
import numpy as np

import ref_ctc_prefix as R
import ref_ctc_prefix_lm as RL

LN10 = float(np.log(10.0))
FLOOR = -99.0 * LN10
NGRAM_PARITY = 8 * 1.46e-05
ORDERS = (1, 2, 4)


def unit_dict(V):
    """io_utils.create_unit_dict's shape for V classes: MASK = 0, V - 3 real units with multi-character names, EOS = V - 2, GO = V - 1."""
    d = {0: "MASK", -1: "END", V - 2: "EOS", V - 1: "GO"}
    for i in range(1, V - 2):
        d[i] = " " if i == 1 else "u%d" % i
    return d


class NGramRef:
    def __init__(self, model, V, dtype=np.float64):
        self.V, self.go, self.eos, self.dtype, self.N = V, V - 1, V - 2, dtype, model.order
        self.lp, self.bw = {}, {}
        for g in model.grams:
            for gram, (a, b) in g.items():
                self.lp[gram], self.bw[gram] = dtype(a * LN10), dtype(b * LN10)          # float64 product, rounded once
        self.memo = {}

    def context(self, g):
        h = (self.go,) + tuple(int(s) for s in g)
        return h[max(len(h) - (self.N - 1), 0):] if self.N > 1 else ()

    def value(self, c, h):
        dt = self.dtype
        acc = dt(0.0)
        while True:
            if h + (c,) in self.lp:
                return dt(acc + self.lp[h + (c,)])
            if not h:
                return dt(acc + dt(FLOOR))
            if h in self.bw:
                acc = dt(acc + self.bw[h])
            h = h[1:]

    def lam(self, g):
        h = self.context(g)
        if h not in self.memo:
            self.memo[h] = np.array([self.value(c, h) for c in range(self.V)], self.dtype)
        return self.memo[h]

    def s_lm(self, g):
        g = tuple(g)
        return float(sum(float(self.lam(g[:i])[g[i]]) for i in range(len(g))) + float(self.lam(g)[self.eos]))


def sentences(V, n=200, seed=5):
    """n short random label sequences over the real units 1 .. V - 3 with a skewed unigram and some repetition, so that higher orders
    have something to hold."""
    rng = np.random.default_rng(seed + 13 * V)
    U = V - 3
    p = 1.0 / (1.0 + np.arange(U))
    p /= p.sum()
    out = []
    for _ in range(n):
        L = int(rng.integers(1, 9))
        s = list(rng.choice(U, size=L, p=p) + 1)
        if L > 2 and rng.random() < 0.5:
            s[2:] = s[:L - 2]                                   # repeated stretches
        out.append([int(x) for x in s])
    return out


_MODELS = {}


def shared_model(order, V):
    """One Witten-Bell model per (order, V) for all tests: dict(model, ref (float64), ref32, tables)."""
    from avsr_tf1_amd import ngram
    key = (order, V)
    if key not in _MODELS:
        m = ngram.estimate(sentences(V), order, unit_dict(V))
        _MODELS[key] = dict(model=m, ref=NGramRef(m, V), ref32=NGramRef(m, V, np.float32), tables=ngram.compile_tables(m, V, V - 1, V - 2))
    return _MODELS[key]


def sparse_model(V=12, seed=3):
    """Order 4 with holes: a Witten-Bell model on few sentences with a random 40 % of its bigrams and trigrams taken out again, the
    prefixes of kept higher-order entries among them -- so walks back off more than one level, contexts appear only inside higher-order
    entries, and some contexts keep a single continuation."""
    from avsr_tf1_amd import ngram
    m = ngram.estimate(sentences(V, n=40, seed=seed), 4, unit_dict(V))
    rng = np.random.default_rng(seed)
    grams = [dict(g) for g in m.grams]
    for k in (1, 2):
        for gram in sorted(grams[k]):
            if rng.random() < 0.4:
                del grams[k][gram]
    return ngram.NGramModel(4, grams)


def left_out_by_the_reference(order, cfg, w=0.5, beta=0.5):
    """How many of the seeds 0..63 of a whole-search configuration the float64 reference alone leaves out as near-ties."""
    V, T, W, L, s = cfg
    ref = shared_model(order, V)["ref"]
    out = 0
    for seed in range(64):
        r = RL.search_lm(R.kernel_inputs(V, T, s, seed), T, W, L, ref, w, beta)
        out += not r["margin"] > search_tol(r, w)
    return out


def search_tol(ref, w):
    return RL.TOL_SEARCH_LM + w * NGRAM_PARITY * (max(len(g) for g, _p in ref["beam"]) + 1)


def measure_tolerances():
    """Reproduces the docstring's numbers (minutes of Python; not run by the tests)."""
    par = 0.0
    models = [(shared_model(o, V)["model"], V) for o in ORDERS for V in (15, 20, 31, 41, 64, 256)] + [(sparse_model(), 12)]
    for m, V in models:
        a, b = NGramRef(m, V), NGramRef(m, V, np.float32)
        ctxs = {()} | {g[i:] for t in m.grams for g in t for i in range(len(g) + 1) if len(g) - i < m.order}
        for h in ctxs:
            for c in range(V):
                par = max(par, abs(float(b.value(c, h)) - float(a.value(c, h))))
    step = {False: 0.0, True: 0.0}
    for V, T, W, L, s in RL.KERNEL_CONFIGS:
        for o in ORDERS:
            e = shared_model(o, V)
            for shift in R.BLANK_SHIFTS:
                for w, beta in RL.WEIGHTS:
                    step[T > 40] = max(step[T > 40], RL.step_deviation_lm(R.kernel_inputs(V, T, s, 0, shift), T, W, L, e["ref"], e["ref32"], w, beta))
    srch, left = 0.0, {}
    for cfg in RL.SEARCH_CONFIGS:
        V, T, W, L, s = cfg
        for o in ORDERS:
            e = shared_model(o, V)
            left[cfg + (o,)] = left_out_by_the_reference(o, cfg)
            for seed in range(64):
                z = R.kernel_inputs(V, T, s, seed)
                r = RL.search_lm(z, T, W, L, e["ref"], 0.5, 0.5)
                if r["margin"] > search_tol(r, 0.5):
                    srch = max(srch, RL.search_deviation_lm(z, T, W, L, e["ref"], e["ref32"], 0.5, 0.5))
    return par, step[False], step[True], srch, left


if __name__ == "__main__":
    par, a, b, c, left = measure_tolerances()
    print("lam deviation %.3g; one-frame deviation %.3g (T <= 40), %.3g (T = 300); final-score deviation %.3g" % (par, a, b, c))
    print("left out by the reference alone:", left)

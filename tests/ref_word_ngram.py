"""Reference for the word-level n-gram behind a lexicon trie in the CTC prefix beam search (avsr-tf1_amd/ngram.py compile_word_tables,
csrc/ctc_prefix_word_ngram.hip; the rule and its table of cases are INTEGRATION.md section 8) and the setup its tests share.

`WordRef` restates that table over the parsed n-gram lists (keyed by word STRINGS) and a Python set of the lexicon's word prefixes --
strings and dictionaries only; it knows nothing of the compiled trie or automaton.  The state of a label sequence g is (hist, cur):
hist the last N-1 closed words (starting as (<s>,); () after an unknown word closed without <unk> in the model), cur the letters since
the last space.  It has the interface tests/ref_ctc_prefix_lm.py's search takes (`lam(g)` [V], `s_lm(g)`, `eos`).  float64 is the
reference; the float32 form is a RESTATEMENT in the kernel's order (values rounded to float32 once; acc = 0, acc += bow per level left,
then acc + logp; oov + U; close + walk), used to size the tolerances and -- the estimator's models list every context -- equal to the
kernel's rows bit for bit.

The shared setup for V classes (MASK 0, space 1, the single-character letters 2 .. V-3, EOS V-2, GO V-1): a lexicon of up to 120 random
words of 1-4 letters with a skewed letter distribution, a Witten-Bell word model (ngram.estimate) on 300 random sentences of 1-5 words,
orders 1 and 3, with <unk> (a tenth of the sentences' words replaced by it) and without, oov = -4.  Inputs: flat random logits almost
never spell a word, so `inputs` adds 4 s to ref_ctc_prefix.kernel_inputs on the classes of a CTC alignment (spaces between words,
blanks between repeats, random stays) of a random in-lexicon sentence that fits L_max and T.

Tolerances, by the project's convention 8 x what the float32 restatement deviates from float64 on the tests' own inputs
(`measure_tolerances` reproduces the numbers):
    WORD_PARITY       |lam32 - lam64| over every state the fp64 searches of the kernel tests keep (all KERNEL_CONFIGS, blank shifts and
                      the four models) and every label sequence of the exhaustive CPU test: measured 6.85e-06 (half a float32 ulp at
                      |FLOOR| = 228 is 7.6e-6).  8 x 6.85e-06 = 5.48e-05 takes NGRAM_PARITY's place per lam term.
    TOL_STEP_LM / TOL_STEP_LM_LONG / TOL_SEARCH_LM are ref_ctc_prefix_lm's, reused as they are: the float32 restatement of the search
    under the word models measured 1.61e-05 per frame at T <= 40 (the bound is 8 x 1.28e-05), 5.33e-05 at T = 300 (8 x 1.15e-04) and
    2.94e-05 on final scores (8 x 6.63e-05).
Whole searches against the float64 rule leave out near-tie seeds (margin not above the tolerance).  The float64 reference ALONE leaves
out, of 64 seeds at w = beta = 0.5, for the models (order 1 without <unk>, order 3 with <unk>):
    (15, 24, 4, 12, 2): 3, 5    (31, 40, 10, 16, 4): 1, 5    (41, 40, 10, 16, 5): 3, 6    (31, 40, 1, 16, 2): 0, 0
-- at most 64 // 3 = 21 everywhere (`left_out_by_the_reference`)."""
import numpy as np

import ref_ctc_prefix as R
import ref_ctc_prefix_lm as RL

LN10 = float(np.log(10.0))
FLOOR = -99.0 * LN10
WORD_PARITY = 8 * 6.85e-06
OOV = -4.0
SPACE = 1
ORDERS = (1, 3)
MODELS = [(1, False), (1, True), (3, False), (3, True)]                    # (order, <unk> in the model)
SEARCH_MODELS = [(1, False), (3, True)]                                     # the whole-search tests: every order, <unk> both ways
BOS, EOS_W, UNK = "<s>", "</s>", "<unk>"


def letter(i):
    """The character of letter class i >= 2."""
    return chr(ord("a") + i - 2) if i < 28 else chr(0x100 + i)


def unit_dict(V):
    d = {0: "MASK", -1: "END", SPACE: " ", V - 2: "EOS", V - 1: "GO"}
    d.update({i: letter(i) for i in range(2, V - 2)})
    return d


class WordRef:
    def __init__(self, model, vocabulary, V, oov=OOV, dtype=np.float64):
        self.V, self.go, self.eos, self.space, self.dtype, self.N = V, V - 1, V - 2, SPACE, dtype, model.order
        self.lp, self.bw = {}, {}
        for g in model.grams:
            for gram, (a, b) in g.items():
                key = tuple(vocabulary[i] for i in gram)
                self.lp[key], self.bw[key] = dtype(a * LN10), dtype(b * LN10)     # float64 product, rounded once
        self.unk = next((u for u in ("<unk>", "<UNK>") if u in vocabulary), None)
        self.chars = {i: letter(i) for i in range(2, V - 2)}
        alphabet = set(self.chars.values())
        self.words = {w for w in vocabulary if w not in (BOS, EOS_W, "<unk>", "<UNK>") and w and set(w) <= alphabet}
        self.prefixes = {w[:k] for w in self.words for k in range(len(w) + 1)}
        self.oov = dtype(oov)
        self.memo = {}

    def trunc(self, h):
        return tuple(h[max(len(h) - (self.N - 1), 0):]) if self.N > 1 else ()

    def value(self, w, h):
        """The textbook back-off value of word w after the words h."""
        dt = self.dtype
        acc = dt(0.0)
        while True:
            if h + (w,) in self.lp:
                return dt(acc + self.lp[h + (w,)])
            if not h:
                return dt(acc + dt(FLOOR))
            if h in self.bw:
                acc = dt(acc + self.bw[h])
            h = h[1:]

    def close(self, hist, cur):
        """(what a space costs, the history it leaves, the row of the rule's table) at cur != ''."""
        dt = self.dtype
        if cur in self.words:
            return self.value(cur, hist), self.trunc(hist + (cur,)), "word"
        u, h2 = (self.value(self.unk, hist), self.trunc(hist + (self.unk,))) if self.unk else (dt(0.0), ())
        if cur in self.prefixes:
            return dt(self.oov + u), h2, "prefix"
        return u, h2, "sink"

    def state(self, g):
        """(hist, cur) of a label sequence; cur is None once the letters have left every spelling."""
        hist, cur = self.trunc((BOS,)), ""
        for c in g:
            c = int(c)
            if c == self.space:
                if cur != "":
                    hist, cur = self.close(hist, cur)[1], ""
            elif c == self.eos:
                if cur != "":
                    hist = self.close(hist, cur)[1]
                hist, cur = self.trunc(hist + (EOS_W,)), ""
            elif c in self.chars:
                cur = None if cur is None or cur + self.chars[c] not in self.prefixes else cur + self.chars[c]
        return hist, cur

    def lam(self, g):
        key = self.state(g)
        if key not in self.memo:
            hist, cur = key
            dt = self.dtype
            row = np.zeros(self.V, dt)
            for c, ch in self.chars.items():
                row[c] = dt(0.0) if cur is None or cur + ch in self.prefixes else self.oov
            cl, h2 = (dt(0.0), hist) if cur == "" else self.close(hist, cur)[:2]
            row[self.space] = cl
            row[self.eos] = dt(cl + self.value(EOS_W, h2))
            row[0] = row[self.go] = dt(FLOOR)
            self.memo[key] = row
        return self.memo[key]

    def s_lm(self, g):
        g = tuple(g)
        return float(sum(float(self.lam(g[:i])[g[i]]) for i in range(len(g))) + float(self.lam(g)[self.eos]))


def lexicon(V, n=120, seed=11):
    """Up to n distinct random words of 1-4 letters over the letters of V classes, skewed towards the first letters."""
    rng = np.random.default_rng(seed + 13 * V)
    U = V - 4
    p = 1.0 / (1.0 + np.arange(U))
    p /= p.sum()
    words = []
    for _ in range(n):
        w = "".join(letter(int(c) + 2) for c in rng.choice(U, size=int(rng.integers(1, 5)), p=p))
        if w not in words:
            words.append(w)
    return words


def sentences(V, unk, n=300, seed=5):
    """n random sentences of 1-5 lexicon words with a skewed word distribution; with unk, a tenth of the words become <unk>."""
    words = lexicon(V)
    rng = np.random.default_rng(seed + 13 * V)
    p = 1.0 / (1.0 + np.arange(len(words)))
    p /= p.sum()
    out = []
    for _ in range(n):
        s = [words[int(i)] for i in rng.choice(len(words), size=int(rng.integers(1, 6)), p=p)]
        out.append([UNK if unk and rng.random() < 0.1 else w for w in s])
    return out


_MODELS = {}


def shared_model(order, V, unk):
    """One Witten-Bell word model per (order, V, unk) for all tests: dict(model, vocabulary, ref (float64), ref32, tables)."""
    from avsr_tf1_amd import ngram
    key = (order, V, bool(unk))
    if key not in _MODELS:
        vocabulary = [BOS, EOS_W] + sorted(lexicon(V) + ([UNK] if unk else []))
        ids = {w: i for i, w in enumerate(vocabulary)}
        m = ngram.estimate([[ids[w] for w in s] for s in sentences(V, unk)], order, ngram.word_dict(vocabulary))
        _MODELS[key] = dict(model=m, vocabulary=vocabulary, ref=WordRef(m, vocabulary, V), ref32=WordRef(m, vocabulary, V, dtype=np.float32),
                            tables=ngram.compile_word_tables(m, vocabulary, unit_dict(V), OOV))
    return _MODELS[key]


def inputs(V, T, s, seed, L_max, blank_shift=0.0):
    """ref_ctc_prefix.kernel_inputs plus 4 s on the classes of a CTC alignment of a random in-lexicon sentence (see the docstring)."""
    z = R.kernel_inputs(V, T, s, seed, blank_shift).copy()
    rng = np.random.default_rng(1000 + seed)
    words, cap, labels = lexicon(V), min(L_max - 2, T // 2), []
    index = {letter(i): i for i in range(2, V - 2)}
    while True:
        fits = [w for w in words if len(labels) + bool(labels) + len(w) <= cap]
        if not fits:
            break
        labels += ([SPACE] if labels else []) + [index[ch] for ch in fits[int(rng.integers(len(fits)))]]
    path = []
    for c in labels:
        if path and path[-1] == c:
            path.append(V)                                  # the blank between repeats
        path.append(c)
    while path and len(path) < T:                           # random stays
        i = int(rng.integers(len(path)))
        path.insert(i, path[i])
    for t, c in enumerate(path[:T]):
        z[t, c] += 4 * s
    return z


def search_tol(ref, w):
    return RL.TOL_SEARCH_LM + w * WORD_PARITY * (max(len(g) for g, _p in ref["beam"]) + 1)


_REFS = {}


def references(cfg, order, unk, w=0.5, beta=0.5):
    """(zs [64, T, V + 1], the fp64 searches of the seeds 0..63) of a whole-search configuration: computed once, shared, read-only."""
    key = (cfg, order, bool(unk), w, beta)
    if key not in _REFS:
        V, T, W, L_max, s = cfg
        lm = shared_model(order, V, unk)["ref"]
        zs = np.stack([inputs(V, T, s, seed, L_max) for seed in range(64)])
        zs.setflags(write=False)
        _REFS[key] = (zs, [RL.search_lm(zs[i], T, W, L_max, lm, w, beta) for i in range(64)])
    return _REFS[key]


def left_out_by_the_reference(order, unk, cfg, w=0.5):
    """How many of the seeds 0..63 of a whole-search configuration the float64 reference alone leaves out as near-ties."""
    return sum(not r["margin"] > search_tol(r, w) for r in references(cfg, order, unk, w)[1])


def all_sequences(V, n):
    """Every label sequence of up to n classes."""
    out, layer = [()], [()]
    for _ in range(n):
        layer = [g + (c,) for g in layer for c in range(V)]
        out += layer
    return out


def measure_tolerances():
    """Reproduces the docstring's numbers (minutes of Python; not run by the tests)."""
    par = 0.0
    for order, unk in MODELS:
        e = shared_model(order, 6, unk)
        for g in all_sequences(6, 5):
            par = max(par, float(np.abs(e["ref32"].lam(g).astype(np.float64) - e["ref"].lam(g)).max()))
    step = {False: 0.0, True: 0.0}
    for V, T, W, L, s in RL.KERNEL_CONFIGS:
        for order, unk in MODELS:
            e = shared_model(order, V, unk)
            for shift in R.BLANK_SHIFTS:
                for w, beta in RL.WEIGHTS:
                    z = inputs(V, T, s, 0, L, shift)
                    step[T > 40] = max(step[T > 40], RL.step_deviation_lm(z, T, W, L, e["ref"], e["ref32"], w, beta))
                    for beam in RL.search_lm(z, T, W, L, e["ref"], w, beta)["beams"]:
                        for g, _a, _b in beam:
                            par = max(par, float(np.abs(e["ref32"].lam(g).astype(np.float64) - e["ref"].lam(g)).max()))
    srch, left = 0.0, {}
    for cfg in RL.SEARCH_CONFIGS:
        V, T, W, L, s = cfg
        for order, unk in SEARCH_MODELS:
            e = shared_model(order, V, unk)
            left[cfg + (order, unk)] = left_out_by_the_reference(order, unk, cfg)
            zs, refs = references(cfg, order, unk)
            for z, r in zip(zs, refs):
                if r["margin"] > search_tol(r, 0.5):
                    srch = max(srch, RL.search_deviation_lm(z, T, W, L, e["ref"], e["ref32"], 0.5, 0.5))
    return par, step[False], step[True], srch, left


if __name__ == "__main__":
    par, a, b, c, left = measure_tolerances()
    print("lam deviation %.3g; one-frame deviation %.3g (T <= 40), %.3g (T = 300); final-score deviation %.3g" % (par, a, b, c))
    print("left out by the reference alone:", left)

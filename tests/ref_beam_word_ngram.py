"""Reference side of beam search with a shallow-fusion WORD-level n-gram behind a lexicon trie (include/avsr_hip.h avsr_beam_word_ngram,
csrc/beam_word_ngram.hip; the rule is INTEGRATION.md section 8, the table under ctc_word_ngram_lm) and the setup its tests share.

The fp64 search is ref_beam_ngram.beam_search_decode_ngram AS IT IS, called with a ref_word_ngram.WordRef (strings and dictionaries; it
has NGramRef's `lam(g)` interface and knows nothing of the compiled trie or automaton):
    step_lp[k, v] = log_softmax(logits_am[k])[v] + lm_weight * lam(v | g_k)  (+ ctc_weight * term)

Models: ref_word_ngram.shared_model(order, V, unk) for ref_word_ngram.MODELS, oov = -4, the space is class 1.

The search cases.  Random recognisers almost never emit a space, so the whole-search tests use the SPACED setup: ref_beam_ngram's long
setup (EOS bias -2.0, 9 steps) with a copy of dec/out/bias raised by SPACE_SHIFT = 3.0 at the space.  EXCLUDED lists the configurations
(architecture, K, weight, model) whose fp64 cut gap (the K-th against the (K+1)-th candidate, the smallest over steps and utterances)
does not exceed 4 TIE = 8e-5, with the measured gap; tests/test_beam_word_ngram_cpu.py recomputes every gap and asserts the list is
exactly those, at most a quarter of the configurations, never a whole architecture or a whole model.

`host_step` / `host_rows` restate the device step on the compiled tables with ngram.word_step and ngram.word_lam (float32, the kernel's
additions in the kernel's order), hc and the clamps included: the state of a row is (h, p, hc); a space takes its parent's hc, EOS walks
from it; tok / parent_rows outside [0, V) / [0, R) become 0, a stale h or hc outside [0, n_nodes) 0, a stale p outside
[-1, n_trie_nodes) the root.

`chain` draws the symbols and parents of the step-kernel test.  Random classes alone fall into the sink within two steps, so each
row's next symbol is drawn from its parent's state: with probability 0.55 a child of its trie prefix, 0.2 a space, 0.05 EOS, else any
class in [0, V); every fourth step one row gets MASK and one GO.  Parents are random: duplicates, dropped rows, no identity.

Tolerance of the rows against WordRef: ref_word_ngram.WORD_PARITY (8 x 6.85e-06, measured on the prefix search's states).  Over this
file's own states -- every state of every chain of KERNEL_CASES and every row the spaced fp64 searches use -- the float32 restatement
deviates from float64 by at most 6.848e-06 (tests/test_beam_word_ngram_cpu.py measures and asserts <= 6.85e-06), so the constant is
used as it is."""
import numpy as np

import ref_beam_ngram as RB
import ref_word_ngram as RW
from ref_beam_ngram import beam_search_decode_ngram  # noqa: F401  (the fp64 search, unchanged)

ARCHS = RB.ARCHS
WEIGHTS = (0.3, 1.0)
KS = (1, 3, 10)
V = 31
LONG_STEPS = RB.LONG_STEPS
MAX_STEPS = RB.MAX_STEPS
SPACE_SHIFT = 3.0
PLAIN = dict(key=(1, False), K=3, weight=0.3, check_every=4)        # the unmodified setup: the run that ends early in every architecture
MODELS = RW.MODELS
SEARCH_MODELS = RW.SEARCH_MODELS
OOV, SPACE = RW.OOV, RW.SPACE
WORD_PARITY = RW.WORD_PARITY
MEASURED_PARITY = 6.85e-06                      # what WORD_PARITY is 8 x of; this file's own states must stay below it

KERNEL_RNS = (1, 9, 30, 65)
KERNEL_VS = (15, 31, 41)
KERNEL_CASES = [(m, v, rn) for m in MODELS for v in KERNEL_VS for rn in KERNEL_RNS]
CHAIN_STEPS = 14

# (architecture, K, weight, (order, unk)): the fp64 cut gap, not above 4 TIE
EXCLUDED = {("c5_av_align", 1, 0.3, (3, True)): 6.48e-05}

_spaced = {}


def model(key, V=V):
    """key = (order, <unk> in the model): dict(model, vocabulary, ref (float64), ref32, tables)."""
    return RW.shared_model(key[0], V, key[1])


def spaced_case(case):
    """(ocfg, mcfg, W, batch) of the spaced setup; built once per case and shared, ref_beam_ngram's weights are not touched."""
    if case not in _spaced:
        ocfg, mcfg, W, batch = RB.long_case(case)
        W = dict(W)
        W["dec/out/bias"] = W["dec/out/bias"].copy()
        W["dec/out/bias"][SPACE] += np.float32(SPACE_SHIFT)
        _spaced[case] = (ocfg, mcfg, W, batch)
    return _spaced[case]


def plain_case(case):
    return RB.plain_case(case)


def ctc_case(case):
    return RB.ctc_case(case)


def configurations():
    """Every whole-search configuration of the suite, the excluded ones included."""
    return [(case, K, w, m) for case in ARCHS for K in KS for w in WEIGHTS for m in SEARCH_MODELS]


# ---- the device step restated on the compiled tables ------------------------------------------------------------------------------
def clamp_state(tables, h, p, hc):
    n, nt = int(tables["n_nodes"]), int(tables["n_trie_nodes"])
    return (h if 0 <= h < n else 0), (p if -1 <= p < nt else 0), (hc if 0 <= hc < n else 0)


def host_hc(tables, h, p):
    """The automaton node a space leaves at (h, p): h at the root."""
    from avsr_tf1_amd import ngram
    return int(ngram.word_step(tables, (h, p), tables["space_id"])[0])


def host_step(tables, state, tok, parent_rows, step):
    """One avsr_beam_word_ngram_step on the host: the new state int32 [3, R] = (h, p, hc) of the rows from the state [3, R] before."""
    from avsr_tf1_amd import ngram
    t, R, V = tables, len(tok), int(tables["V"])
    out = np.empty((3, R), np.int32)
    for r in range(R):
        if step == 0:
            h, p = ngram.word_start(t)
        else:
            par, c = int(parent_rows[r]), int(tok[r])
            par, c = (par if 0 <= par < R else 0), (c if 0 <= c < V else 0)
            h, p, hc = clamp_state(t, *(int(x) for x in state[:, par]))
            if c == t["space_id"]:
                h, p = hc, 0
            elif c == t["eos_id"]:
                h, p = int(t["next"][ngram.walk(t, hc, t["eos_w"])[1]]), 0
            else:
                h, p = ngram.word_step(t, (h, p), c)
        out[:, r] = h, p, host_hc(t, h, p)
    return out


def host_state(tables, g):
    """(h, p) of the label history g by ngram.word_step alone."""
    from avsr_tf1_amd import ngram
    s = ngram.word_start(tables)
    for c in g:
        s = ngram.word_step(tables, s, c)
    return int(s[0]), int(s[1])


_rows = {}


def host_rows(tables, hs, ps):
    """lam(. | (h, p)) [len(hs), V] float32 by ngram.word_lam (memoised per table object and state)."""
    from avsr_tf1_amd import ngram
    memo = _rows.setdefault(id(tables), {})
    out = []
    for h, p in zip(hs, ps):
        k = (int(h), int(p))
        if k not in memo:
            memo[k] = ngram.word_lam(tables, k)
        out.append(memo[k])
    return np.stack(out)


# ---- the symbol chains of the step-kernel test --------------------------------------------------------------------------------------
def chain_seed(key, V, Rn):
    return 100000 * Rn + 100 * V + 10 * key[0] + int(key[1])


def draw(rng, tables, state, step):
    """(tok, parent_rows) int32 [R] of step `step` >= 1 from the host state [3, R] that step - 1 left (see the docstring)."""
    t, R, V = tables, state.shape[1], int(tables["V"])
    par = rng.integers(0, R, size=R).astype(np.int32)
    if R > 1:
        par[1] = par[0]
    tok = np.empty(R, np.int32)
    for r in range(R):
        p, u = int(state[1, par[r]]), rng.random()
        kids = t["t_sym"][int(t["t_begin"][p]):int(t["t_begin"][p + 1])] if p >= 0 else ()
        if u < 0.55 and len(kids):
            tok[r] = int(kids[int(rng.integers(len(kids)))])
        elif u < 0.75:
            tok[r] = t["space_id"]
        elif u < 0.80:
            tok[r] = t["eos_id"]
        else:
            tok[r] = int(rng.integers(0, V))
    if step % 4 == 3 and R > 2:
        a, b = rng.choice(R, size=2, replace=False)
        tok[a], tok[b] = 0, t["go_id"]
    return tok, par


def chain(key, V, Rn, steps=CHAIN_STEPS):
    """The chained steps of one step-kernel case: a list of dict(tok, par, state [3, R] after the step, hist (the label history of every
    row after the step)), step 0 first (its tok / par are drawn but must be ignored by the device)."""
    tables = model(key, V)["tables"]
    rng = np.random.default_rng(chain_seed(key, V, Rn))
    state, hist, out = np.zeros((3, Rn), np.int32), [()] * Rn, []
    for step in range(steps):
        if step == 0:
            tok, par = rng.integers(0, V, size=Rn).astype(np.int32), rng.integers(0, Rn, size=Rn).astype(np.int32)
        else:
            tok, par = draw(rng, tables, state, step)
        state = host_step(tables, state, tok, par, step)
        hist = [()] * Rn if step == 0 else [hist[p] + (int(c),) for p, c in zip(par, tok)]
        out.append(dict(tok=tok, par=par, state=state, hist=hist))
    return out


def kind(ref, g):
    """The row of the rule's table a label history is in: 'root', 'prefix', 'word' or 'sink' (read from WordRef's own state)."""
    _hist, cur = ref.state(g)
    return "root" if cur == "" else "sink" if cur is None else "word" if cur in ref.words else "prefix"


def symbol(ref, g, c):
    """What the class c is at the history g: 'stay' / 'leave' (a letter), 'space', 'eos', 'mask', 'go'."""
    c = int(c)
    if c == ref.space:
        return "space"
    if c == ref.eos:
        return "eos"
    if c == 0:
        return "mask"
    if c == ref.go:
        return "go"
    _hist, cur = ref.state(g)
    return "stay" if cur is None or cur + ref.chars[c] in ref.prefixes else "leave"


def closed_words(ref, g):
    """How many words the history g has closed (a space or EOS taken away from the root)."""
    return sum(1 for i, c in enumerate(g) if int(c) in (ref.space, ref.eos) and kind(ref, g[:i]) != "root")

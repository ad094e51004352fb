"""Word-level n-gram behind a lexicon trie in beam search, the parts that need no GPU: the fp64 reference (tests/ref_beam_word_ngram.py)
against the oracle's own search, the host restatement of the device step against the string-and-dictionary rule, the conditions that
the GPU test's chains and search cases rest on (recomputed here from the same seeds, so they cannot rot), the argument checks of the
new C entry points (decided on the host before any launch), and the refusals of `AVSR(word_ngram_lm=...)` and `LM(word_ngram_lm=...)`,
which are raised before an engine is built."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_beam_word_ngram as R
from oracle import avsr_oracle as O
from test_beam_lm_cpu import _lm_checkpoint, _unit_file
from test_gpu_beam import TIE
from test_word_ngram_cpu import _word_arpa


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("setup", ["plain", "spaced"])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_weight_zero_is_the_oracles_search(case, setup, K):
    ocfg, _m, W, batch = R.plain_case(case) if setup == "plain" else R.spaced_case(case)
    steps = R.MAX_STEPS if setup == "plain" else R.LONG_STEPS
    ids0, lp0, ln0, tr0 = O.beam_search_decode(W, ocfg, batch, beam_width=K, max_steps=steps, return_trace=True)
    ids, lp, ln, tr = R.beam_search_decode_ngram(W, ocfg, batch, R.model((3, True))["ref"], 0.0, beam_width=K, max_steps=steps)
    assert np.array_equal(ids, ids0) and np.array_equal(lp, lp0) and np.array_equal(ln, ln0)
    assert np.array_equal(tr["step_ids"], tr0["step_ids"]) and np.array_equal(tr["parent_ids"], tr0["parent_ids"])


_chains = {}


def _chain(key, V, Rn):
    if (key, V, Rn) not in _chains:
        _chains[(key, V, Rn)] = R.chain(key, V, Rn)
    return _chains[(key, V, Rn)]


@pytest.mark.parametrize("key", R.MODELS)
def test_host_restatement_follows_the_rule_on_every_chain_state(key):
    """Per model, over every (V, Rn) chain of the GPU test: the chained (h, p, hc) state is the state ngram.word_step reaches from the
    row's own label history (the parents' cached hc changes nothing), its rows lie within WORD_PARITY of WordRef's, and the float32
    restatement of the rule itself stays within the 6.85e-06 that WORD_PARITY is eight times of."""
    worst = worst32 = 0.0
    for V in R.KERNEL_VS:
        e = R.model(key, V)
        for Rn in R.KERNEL_RNS:
            for st in _chain(key, V, Rn):
                for r, g in enumerate(st["hist"]):
                    h, p, hc = (int(x) for x in st["state"][:, r])
                    assert (h, p) == R.host_state(e["tables"], g) and hc == R.host_hc(e["tables"], h, p), (V, Rn, g)
                lam64 = np.stack([e["ref"].lam(g) for g in st["hist"]])
                rows = R.host_rows(e["tables"], st["state"][0], st["state"][1])
                assert np.isfinite(rows).all()
                worst = max(worst, float(np.abs(rows.astype(np.float64) - lam64).max()))
                worst32 = max(worst32, float(np.abs(np.stack([e["ref32"].lam(g) for g in st["hist"]]).astype(np.float64) - lam64).max()))
    print(key, "host rows against the fp64 rule", worst, "float32 rule against the fp64 rule", worst32)
    assert worst32 <= R.MEASURED_PARITY and worst <= R.WORD_PARITY


def test_host_step_clamps_stale_states_symbols_and_parents():
    """Whatever the previous half holds, the restated step indexes inside the tables: foreign h / hc become node 0, a foreign p the root,
    foreign tok / parents 0 -- and the new state is again a valid one."""
    t = R.model((3, True))["tables"]
    big = max(t["n_nodes"], t["n_trie_nodes"]) + 1000
    for fill in (big, -5, 1 << 30):
        stale = np.full((3, 4), fill, np.int32)
        out = R.host_step(t, stale, [2, R.SPACE, t["eos_id"], 77], [0, 1, 9, -3], 1)
        assert (0 <= out[0]).all() and (out[0] < t["n_nodes"]).all() and (0 <= out[2]).all() and (out[2] < t["n_nodes"]).all()
        assert (-1 <= out[1]).all() and (out[1] < t["n_trie_nodes"]).all()
        assert np.isfinite(R.host_rows(t, out[0], out[1])).all()
        assert tuple(out[:, 1]) == (0, 0, 0)                               # a space from the clamped (0, root, 0): the cached hc, the root
    assert R.clamp_state(t, 3, -1, 2) == (3, -1, 2) and R.clamp_state(t, 3, -2, 2) == (3, 0, 2)
    assert R.clamp_state(t, t["n_nodes"], t["n_trie_nodes"], -1) == (0, 0, 0)
    assert (R.host_step(t, np.zeros((3, 2), np.int32), [5, 6], [1, 1], 0) == np.array([[t["start"]] * 2, [0, 0], [t["start"]] * 2])).all()


def test_chain_conditions_of_the_gpu_test():
    """What tests/test_gpu_beam_word_ngram.py relies on, over the union of its (model, V, Rn) chains, read from WordRef's own states:
    every (state, symbol) pair that can occur does occur -- a letter cannot leave from the sink, where every letter is free --, MASK and
    GO are symbols, an unknown word is closed with and without <unk> in the model, and at order 3 some row has closed three words."""
    pairs, unk_closed, three, steps = set(), set(), False, set()
    for key, V, Rn in R.KERNEL_CASES:
        ref, ch = R.model(key, V)["ref"], _chain(key, V, Rn)
        steps.add(len(ch))
        for st in ch[1:]:
            assert 0 <= st["tok"].min() and st["tok"].max() < V and 0 <= st["par"].min() and st["par"].max() < Rn
            if Rn > 2:
                assert len(set(st["par"].tolist())) < Rn                   # duplicates and dropped rows: no identity
            for g in st["hist"]:
                k, s = R.kind(ref, g[:-1]), R.symbol(ref, g[:-1], g[-1])
                pairs.add((k, s))
                if s in ("space", "eos") and k in ("prefix", "sink"):
                    unk_closed.add(key[1])
                three = three or (key[0] == 3 and R.closed_words(ref, g) >= 3)
    want = {(k, s) for k in ("root", "prefix", "word", "sink") for s in ("stay", "leave", "space", "eos")} - {("sink", "leave")}
    assert want <= pairs, want - pairs
    assert {s for _k, s in pairs} >= {"mask", "go"}
    assert unk_closed == {False, True} and three and min(steps) >= 12


_runs = {}


def _run(case, key, K, w):
    if (case, key, K, w) not in _runs:
        ocfg, _m, W, batch = R.spaced_case(case)
        _runs[(case, key, K, w)] = R.beam_search_decode_ngram(W, ocfg, batch, R.model(key)["ref"], w, beam_width=K, max_steps=R.LONG_STEPS)
    return _runs[(case, key, K, w)]


def _taken(ref, tr):
    """The (state, symbol) pairs of the rows the search kept: an unfinished parent's history and the symbol selected from it."""
    out, T = set(), tr["step_ids"].shape[0]
    B, K = tr["step_ids"].shape[1:]
    for t in range(T):
        for b in range(B):
            for k in range(K):
                g = tr["hists"][t][b * K + int(tr["parent_ids"][t][b, k])]
                if not (g and g[-1] == ref.eos):                           # a finished beam continues with EOS and no term
                    out.add((R.kind(ref, g), R.symbol(ref, g, tr["step_ids"][t][b, k])))
    return out


def test_spaced_setup_conditions_of_the_gpu_test():
    """What the whole-search cases rest on, on the fp64 reference alone over K (1, 3, 10) x weights (0.3, 1.0) x SEARCH_MODELS: every
    architecture runs all 9 steps; the kept rows take a space from a word end and from the sink and EOS away from the root; the term
    changes every result against weight 0; the cut gap exceeds 4 TIE everywhere but in the configurations of EXCLUDED, which are exactly
    the ones that do not, at most a quarter of all, never a whole architecture or a whole model; and the float32 rule stays within
    6.85e-06 of the float64 rule on every row the searches use."""
    taken, low, worst32 = {}, {}, 0.0
    for case, K, w, key in R.configurations():
        e = R.model(key)
        ocfg, _m, W, batch = R.spaced_case(case)
        ids0, lp0 = R.beam_search_decode_ngram(W, ocfg, batch, e["ref"], 0.0, beam_width=K, max_steps=R.LONG_STEPS)[:2]
        ids, lp, _ln, tr = _run(case, key, K, w)
        assert tr["step_ids"].shape[0] == R.LONG_STEPS, (case, K, w, key)
        assert ids.shape != ids0.shape or not np.array_equal(ids, ids0) or not np.allclose(lp, lp0), (case, K, w, key)
        cut = float(tr["cuts"].min())
        print(case, K, w, key, "cut gap", cut)
        if not cut > 4 * TIE:
            low[(case, K, w, key)] = cut
        taken.setdefault(case, set()).update(_taken(e["ref"], tr))
        for hs in tr["hists"]:
            for g in set(hs):
                worst32 = max(worst32, float(np.abs(e["ref32"].lam(g).astype(np.float64) - e["ref"].lam(g)).max()))
    assert set(low) == set(R.EXCLUDED), (low, R.EXCLUDED)
    assert all(abs(low[c] - R.EXCLUDED[c]) <= 0.01 * R.EXCLUDED[c] for c in low), low
    conf = R.configurations()
    assert 4 * len(R.EXCLUDED) <= len(conf)
    for case in R.ARCHS:
        assert any(c[0] == case and c not in R.EXCLUDED for c in conf)
    for key in R.SEARCH_MODELS:
        assert any(c[3] == key and c not in R.EXCLUDED for c in conf)
    every = set().union(*taken.values())
    assert {("word", "space"), ("sink", "space")} <= every, every
    assert any(s == "eos" and k != "root" for k, s in every)
    assert sum(("word", "space") in v for v in taken.values()) >= 2 and sum(("sink", "space") in v for v in taken.values()) >= 2
    assert worst32 <= R.MEASURED_PARITY, worst32


@pytest.mark.parametrize("case", list(R.ARCHS))
def test_plain_setup_search_ends_inside_a_chunk(case):
    """The unmodified setup at the GPU test's configuration (the word model makes EOS dear: most other configurations run to
    MAX_STEPS): the search ends after 3-5 steps, inside a chunk of four, so the engine's last chunk runs past the end."""
    ocfg, _m, W, batch = R.plain_case(case)
    P = R.PLAIN
    tr = R.beam_search_decode_ngram(W, ocfg, batch, R.model(P["key"])["ref"], P["weight"], beam_width=P["K"], max_steps=R.MAX_STEPS)[3]
    T = tr["step_ids"].shape[0]
    assert tr["finished"].all() and 3 <= T <= 5 and T % P["check_every"] != 0
    assert float(tr["cuts"].min()) > 4 * TIE


def test_reference_with_the_ctc_term_ends_and_both_terms_matter():
    ocfg, _m, W, batch = R.ctc_case("c1_audio_uni_luong")
    ref = R.model((3, True))["ref"]
    run = lambda lmw, cw: R.beam_search_decode_ngram(W, ocfg, batch, ref, lmw, ctc_weight=cw, beam_width=10, max_steps=R.RB.RC.MAX_STEPS)
    both, wn, ctc = run(0.3, 0.3), run(0.3, 0.0), run(0.0, 0.3)
    assert both[3]["finished"].all() and both[3]["step_ids"].shape[0] < R.RB.RC.MAX_STEPS
    assert float(both[3]["cuts"].min()) > 4 * TIE
    for other in (wn, ctc):
        assert both[0].shape != other[0].shape or not np.array_equal(both[0], other[0]) or not np.allclose(both[1], other[1])


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    p = 64                                          # any non-NULL address: the checks return before a launch could read it
    MN, MA = _lib.CTC_PREFIX_NGRAM_MAX_NODES, _lib.CTC_PREFIX_NGRAM_MAX_ARCS
    PTRS = ("bow", "backoff", "arc_begin", "sym", "logp", "next", "t_begin", "t_sym", "t_next", "t_word", "state", "lm_logp")

    def wn(**over):
        g = _lib.BeamWordNgram()
        g.n_nodes, g.n_arcs, g.Vw, g.start, g.eos_w, g.unk_id, g.n_trie_nodes, g.n_trie_arcs = 5, 50, 40, 1, 1, 2, 9, 8
        g.V, g.space_id, g.go_id, g.eos_id, g.n_rows, g.lm_weight, g.oov = 31, 1, 30, 29, 30, 0.3, -4.0
        for k in PTRS:
            setattr(g, k, p)
        for k, v in over.items():
            setattr(g, k, v)
        return g

    ok = wn()
    sup = lambda g: lib.avsr_beam_word_ngram_supported(None if g is None else C.byref(g))
    assert sup(ok) == 1 and sup(None) == 0 and sup(wn(lm_weight=0.0)) == 1 and sup(wn(n_arcs=40)) == 1 and sup(wn(unk_id=-1)) == 1
    assert sup(wn(oov=0.0)) == 1 and sup(wn(n_trie_nodes=1, n_trie_arcs=1)) == 1
    bad_arg = [dict(n_nodes=0), dict(n_arcs=39), dict(Vw=1), dict(V=1), dict(start=5), dict(start=-1), dict(n_rows=0), dict(lm_weight=-0.1),
               dict(lm_weight=float("inf")), dict(lm_weight=float("nan")), dict(eos_w=40), dict(eos_w=-1), dict(unk_id=40), dict(unk_id=-2),
               dict(space_id=31), dict(space_id=-1), dict(space_id=30), dict(space_id=29), dict(go_id=29), dict(go_id=31), dict(eos_id=-1),
               dict(n_trie_nodes=0), dict(n_trie_arcs=0), dict(oov=0.5), dict(oov=float("nan")), dict(oov=float("-inf")),
               dict(oov=float("inf"))] + [{k: None} for k in PTRS]
    big = [dict(n_nodes=MN + 1), dict(n_arcs=MA + 1), dict(n_trie_nodes=MN + 1), dict(n_trie_arcs=MA + 1)]
    for bad in bad_arg + big:
        assert sup(wn(**bad)) == 0, bad
    step = lambda g, tok=p, par=p, n=30, s=0: lib.avsr_beam_word_ngram_step(None if g is None else C.byref(g), tok, par, n, s, None)
    assert step(None) == -1 and step(ok, tok=None) == -1 and step(ok, par=None) == -1           # AVSR_ERR_ARG
    assert step(ok, n=0) == -1 and step(ok, n=29) == -1 and step(ok, s=-1) == -1
    for bad in bad_arg:
        assert step(wn(**bad)) == -1, bad
    for bad in big:
        assert step(wn(**bad)) == -3, bad                                                       # AVSR_ERR_UNSUPPORTED
    assert step(wn(n_trie_nodes=MN + 1, start=5)) == -1                                         # an argument error comes first
    # the fused search: NULL descriptors, a non-beam mode, vocabulary / row-count mismatch, a CTC step that reads another buffer
    d = _lib.AttnRnn()
    d.mode, d.V, d.B, d.beam_width, d.eos_id = 3, 31, 30, 10, 29
    fwd = lambda dd, g, c=None: lib.avsr_attn_rnn_fwd_word_ngram(None if dd is None else C.byref(dd), None if g is None else C.byref(g),
                                                                 None if c is None else C.byref(c), 0, 1, None)
    assert fwd(None, ok) == -1 and fwd(d, None) == -1
    assert fwd(d, wn(V=15, go_id=14, eos_id=13)) == -1 and fwd(d, wn(n_rows=20)) == -1 and fwd(d, wn(n_trie_arcs=MA + 1)) == -3
    assert fwd(d, wn(oov=1.0)) == -1 and fwd(d, wn(space_id=29)) == -1
    c = _lib.BeamCtc()
    c.n_utt, c.beam_width, c.T, c.V, c.eos_id, c.weight, c.ld = 3, 10, 12, 31, 29, 0.3, 32
    c.z = c.in_len = c.y = c.state = c.psi = c.last = c.term = c.extra = p
    assert lib.avsr_beam_ctc_supported(C.byref(c)) == 1
    c.lm_logp = 128                                                                              # not the word model's buffer
    assert fwd(d, ok, c) == -1
    c.lm_logp, c.beam_width, c.n_utt = p, 3, 10                                                  # another beam width than the decoder's
    assert fwd(d, ok, c) == -1
    d.mode = 1
    assert fwd(d, ok) == -1
    assert lib.avsr_sizeof(b"avsr_beam_word_ngram") == C.sizeof(_lib.BeamWordNgram) and lib.avsr_abi_version() == 2


def test_avsr_refuses_what_the_word_ngram_fusion_does_not_cover(tmp_path, monkeypatch):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import _lib, ngram
    from avsr_tf1_amd.io_utils import create_unit_dict
    uf = _unit_file(tmp_path)
    arpa = _word_arpa(tmp_path)
    kw = dict(unit="character", unit_file=uf, word_ngram_lm=arpa)
    for algo in ("greedy", "ctc_prefix_beam_search", "attention_rescoring"):
        with pytest.raises(ValueError, match="word_ngram_lm needs decoding_algorithm='beam_search'.*ctc_word_ngram_lm"):
            avsr.AVSR(decoding_algorithm=algo, use_ctc=True, **kw)
    ck = _lm_checkpoint(tmp_path, uf, units_per_layer=(12,), embedding_size=8)
    with pytest.raises(ValueError, match="word_ngram_lm and lm_checkpoint are two language models"):
        avsr.AVSR(lm_checkpoint=ck, lm_units_per_layer=(12,), lm_embedding_size=8, **kw)
    ud = create_unit_dict(unit_file=uf)
    units = os.path.join(str(tmp_path), "units.arpa")
    ngram.write_arpa(units, ngram.estimate([[3, 4, 5]], 2, ud), ud)
    with pytest.raises(ValueError, match="word_ngram_lm and ngram_lm are two language models"):
        avsr.AVSR(ngram_lm=units, **kw)
    with pytest.raises(ValueError, match="needs the unit ' '"):
        avsr.AVSR(**dict(kw, unit_file=_unit_file(tmp_path, "'abcdefghijklmnopqrstuvwxyz")))
    phones = os.path.join(str(tmp_path), "phones")
    open(phones, "w").write("\n".join([" ", "aa", "b", "k"]) + "\n")
    with pytest.raises(ValueError, match="single-character units"):
        avsr.AVSR(**dict(kw, unit_file=phones))
    with pytest.raises(ValueError, match="no word of the model can be spelled"):
        avsr.AVSR(**dict(kw, unit_file=_unit_file(tmp_path, " xyz")))
    for bad in (1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="out-of-vocabulary score"):
            avsr.AVSR(word_oov_score=bad, **kw)
    bad = os.path.join(str(tmp_path), "bad.arpa")
    open(bad, "w").write("\\data\\\nngram 2=1\n\n\\2-grams:\n-1.0 a b\n\n\\end\\\n")
    with pytest.raises(ValueError, match="1-grams"):
        avsr.AVSR(**dict(kw, word_ngram_lm=bad))
    with pytest.raises((ValueError, OSError)):
        avsr.AVSR(**dict(kw, word_ngram_lm=os.path.join(str(tmp_path), "no_such.arpa")))
    for w in (float("nan"), -0.5, float("inf")):
        with pytest.raises(ValueError, match="lm_weight"):
            avsr.AVSR(lm_weight=w, **kw)
    with pytest.raises(ValueError, match="word_ngram_lm"):
        avsr.LM(unit="character", unit_file=uf, word_ngram_lm=arpa)
    monkeypatch.setattr(_lib, "CTC_PREFIX_NGRAM_MAX_ARCS", 5)        # tables outside avsr_beam_word_ngram_supported
    with pytest.raises(ValueError, match="avsr_beam_word_ngram_supported covers word automata and lexicon tries of up to"):
        avsr.AVSR(**kw)


def test_model_refuses_what_the_word_ngram_fusion_does_not_cover():
    """The engine's own refusals that are decided before anything touches a device."""
    import types
    import torch
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    m = object.__new__(Seq2SeqModel)
    m.cfg, m.dev = ModelConfig(), torch.device("cpu")
    V = m.cfg.vocab_size
    g = dict(V=V, go_id=m.cfg.go_id, eos_id=m.cfg.eos_id, space_id=1)
    batch = types.SimpleNamespace(audio=torch.zeros(2, 5, 3), video=None, labels=torch.zeros(2, 4, dtype=torch.int32))
    lm = types.SimpleNamespace(cfg=types.SimpleNamespace(architecture="lm"), onehot=None)
    for other in (dict(lm=lm), dict(ngram=dict(g))):
        with pytest.raises(ValueError, match="word_ngram \\(word-level tables behind a lexicon\\) cannot be combined with lm or ngram"):
            m._beam_search_decode(batch, word_ngram=g, **other)
    with pytest.raises(ValueError, match="takes one language model: lm \\(an avsr.LM network\\) or ngram \\(back-off tables\\), not both"):
        m._beam_search_decode(batch, lm=lm, ngram=dict(g))                 # the existing pair keeps its text
    with pytest.raises(ValueError, match="the word n-gram tables were compiled for V = %d, GO = 5, EOS = %d" % (V + 2, m.cfg.eos_id)):
        m._beam_search_decode(batch, word_ngram=dict(g, V=V + 2, go_id=5), lm_weight=0.3)
    for space in (0, m.cfg.go_id, m.cfg.eos_id, V):
        with pytest.raises(ValueError, match="hold the space as class %d" % space):
            m._beam_search_decode(batch, word_ngram=dict(g, space_id=space), lm_weight=0.3)
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_weight must be a finite number >= 0"):
            m._beam_search_decode(batch, word_ngram=g, lm_weight=w)
    with pytest.raises(ValueError, match="word n-gram fusion is defined on the beam"):
        m.greedy_decode(batch, word_ngram=g)

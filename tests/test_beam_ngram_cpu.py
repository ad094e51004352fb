"""Back-off n-gram in beam search, the parts that need no GPU: the fp64 reference (tests/ref_beam_ngram.py) against the oracle's own
search and against the compiled automaton, the conditions that the GPU test's search cases rest on (recomputed here, so they cannot
rot), the argument checks of the new C entry points (decided on the host before any launch), and the refusals of `AVSR(ngram_lm=...)`
and `LM(ngram_lm=...)`, which are raised before an engine is built."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_beam_ngram as R
import ref_ngram as RN
from oracle import avsr_oracle as O
from test_beam_lm_cpu import _lm_checkpoint, _unit_file
from test_gpu_beam import TIE
from test_ngram_cpu import _arpa


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("setup", ["plain", "long"])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_weight_zero_is_the_oracles_search(case, setup, K):
    ocfg, _m, W, batch = R.plain_case(case) if setup == "plain" else R.long_case(case)
    steps = R.MAX_STEPS if setup == "plain" else R.LONG_STEPS
    ids0, lp0, ln0, tr0 = O.beam_search_decode(W, ocfg, batch, beam_width=K, max_steps=steps, return_trace=True)
    ids, lp, ln, tr = R.beam_search_decode_ngram(W, ocfg, batch, R.model(4)["ref"], 0.0, beam_width=K, max_steps=steps)
    assert np.array_equal(ids, ids0) and np.array_equal(lp, lp0) and np.array_equal(ln, ln0)
    assert np.array_equal(tr["step_ids"], tr0["step_ids"]) and np.array_equal(tr["parent_ids"], tr0["parent_ids"])


def _lam_rows_follow_the_automaton(tr, tables):
    """Every row lam(. | GO, history) the reference used, against ngram.walk from the node the host transitions lead to: the worst
    deviation (the reference is the dictionary rule in fp64; the automaton holds float32 values added in the kernel's order)."""
    worst = 0.0
    for hist, lam in zip(tr["hists"], tr["lams"]):
        nodes = [R.host_node(tables, g) for g in hist]
        worst = max(worst, float(np.abs(R.host_rows(tables, nodes).astype(np.float64) - lam).max()))
    return worst


_long_runs = {}


def _long_run(case, order, K, w):
    key = (case, order, K, w)
    if key not in _long_runs:
        ocfg, _m, W, batch = R.long_case(case)
        _long_runs[key] = R.beam_search_decode_ngram(W, ocfg, batch, R.model(order)["ref"], w, beam_width=K, max_steps=R.LONG_STEPS)
    return _long_runs[key]


@pytest.mark.parametrize("case", list(R.ARCHS))
def test_long_setup_conditions_of_the_gpu_test(case):
    """What tests/test_gpu_beam_ngram.py relies on, per architecture over orders (1, 2, 4) x K (1, 3, 10) x weights (0.3, 1.0): no
    selection is a near-tie at the cut (the K-th against the (K+1)-th candidate stays above 4 TIE at every step), the n-gram changes every
    result, the histories outgrow the order (c1 / c2 run all 9 steps; c4 / c5 end early in some configurations and run to 9 in others),
    and the rows the reference used are the automaton's within NGRAM_PARITY."""
    ocfg, _m, W, batch = R.long_case(case)
    steps, cut = [], np.inf
    for order in R.ORDERS:
        e = R.model(order)
        for K in R.KS:
            ids0, lp0, _ln0, tr0 = R.beam_search_decode_ngram(W, ocfg, batch, e["ref"], 0.0, beam_width=K, max_steps=R.LONG_STEPS)
            for w in R.WEIGHTS:
                ids, lp, _ln, tr = _long_run(case, order, K, w)
                T = tr["step_ids"].shape[0]
                steps.append(T)
                cut = min(cut, float(tr["cuts"].min()))
                assert ids.shape != ids0.shape or not np.array_equal(ids, ids0) or not np.allclose(lp, lp0), (order, K, w)
                dev = _lam_rows_follow_the_automaton(tr, e["tables"])
                assert dev <= RN.NGRAM_PARITY, (order, K, w, dev)
                assert max(len(g) for g in tr["hists"][-1]) == T - 1
    print(case, "steps", sorted(set(steps)), "smallest cut gap", cut)
    assert cut > 4 * TIE, cut
    if case.startswith(("c1", "c2")):
        assert set(steps) == {R.LONG_STEPS}
    else:
        assert min(steps) < R.LONG_STEPS and max(steps) == R.LONG_STEPS
    assert R.LONG_STEPS - 1 > max(R.ORDERS) - 1                      # a full run's history is longer than the longest context


STEP_LIMIT = {("c1_audio_uni_luong", 4, 3, 1.0), ("c1_audio_uni_luong", 4, 10, 1.0)}     # these reach MAX_STEPS; every other search ends early


@pytest.mark.parametrize("case", list(R.ARCHS))
def test_plain_setup_searches_end_early(case):
    """The unmodified setup: searches end after 1-5 steps (the engine's last chunk then runs past the end), the two of STEP_LIMIT apart."""
    ocfg, _m, W, batch = R.plain_case(case)
    for order in R.ORDERS:
        for K in R.KS:
            for w in R.WEIGHTS:
                _i, _lp, _ln, tr = R.beam_search_decode_ngram(W, ocfg, batch, R.model(order)["ref"], w, beam_width=K, max_steps=R.MAX_STEPS)
                T = tr["step_ids"].shape[0]
                if (case, order, K, w) in STEP_LIMIT:
                    assert T == R.MAX_STEPS, (order, K, w, T)
                else:
                    assert tr["finished"].all() and 1 <= T <= 5, (order, K, w, T)


@pytest.mark.parametrize("case", ["c1_audio_uni_luong", "c5_av_align"])
def test_reference_with_the_ctc_term_ends_and_both_terms_matter(case):
    ocfg, _m, W, batch = R.ctc_case(case)
    ref = R.model(4)["ref"]
    run = lambda lmw, cw: R.beam_search_decode_ngram(W, ocfg, batch, ref, lmw, ctc_weight=cw, beam_width=3, max_steps=R.RC.MAX_STEPS)
    both, ng, ctc = run(0.3, 0.3), run(0.3, 0.0), run(0.0, 0.3)
    assert both[3]["finished"].all() and both[3]["step_ids"].shape[0] < R.RC.MAX_STEPS
    ids_c, lp_c = R.RC.beam_search_decode_ctc(W, ocfg, batch, 0.3, beam_width=3, max_steps=R.RC.MAX_STEPS)[:2]
    assert np.array_equal(ctc[0], ids_c) and np.array_equal(ctc[1], lp_c)          # weight 0: ref_beam_ctc's search
    for other in (ng, ctc):
        assert both[0].shape != other[0].shape or not np.array_equal(both[0], other[0]) or not np.allclose(both[1], other[1])


def test_host_transitions_keep_the_last_symbols():
    """The node the host transitions reach is the longest suffix of (GO, g) that is a context: its recorded context is a suffix of the
    history, and its rows are the reference's for that history (the sparse model backs off through more than one level)."""
    from avsr_tf1_amd import ngram
    rng = np.random.default_rng(11)
    for m, V in [(R.model(o, 15)["model"], 15) for o in R.ORDERS] + [(RN.sparse_model(), 12)]:
        tables, ref = ngram.compile_tables(m, V, V - 1, V - 2), RN.NGramRef(m, V)
        for _ in range(40):
            g = tuple(int(x) for x in rng.integers(0, V, size=int(rng.integers(0, 8))))
            n = R.host_node(tables, g)
            ctx, full = tables["contexts"][n], (V - 1,) + g
            assert full[len(full) - len(ctx):] == ctx
            assert np.abs(R.host_rows(tables, [n])[0].astype(np.float64) - ref.lam(g)).max() <= RN.NGRAM_PARITY


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    p = 64                                          # any non-NULL address: the checks return before a launch could read it
    MN, MA = _lib.CTC_PREFIX_NGRAM_MAX_NODES, _lib.CTC_PREFIX_NGRAM_MAX_ARCS

    def ng(**over):
        g = _lib.BeamNgram()
        g.n_nodes, g.n_arcs, g.V, g.start, g.n_rows, g.lm_weight = 5, 40, 31, 1, 30, 0.3
        g.bow = g.backoff = g.arc_begin = g.sym = g.logp = g.next = g.node = g.lm_logp = p
        for k, v in over.items():
            setattr(g, k, v)
        return g

    ok = ng()
    sup = lambda g: lib.avsr_beam_ngram_supported(None if g is None else C.byref(g))
    assert sup(ok) == 1 and sup(None) == 0 and sup(ng(lm_weight=0.0)) == 1 and sup(ng(n_arcs=31)) == 1 and sup(ng(V=2)) == 1
    for bad in (dict(n_nodes=0), dict(n_arcs=30), dict(V=1), dict(start=5), dict(start=-1), dict(n_rows=0), dict(lm_weight=-0.1),
                dict(lm_weight=float("inf")), dict(lm_weight=float("nan")), dict(node=None), dict(lm_logp=None), dict(sym=None),
                dict(n_nodes=MN + 1), dict(n_arcs=MA + 1)):
        assert sup(ng(**bad)) == 0, bad
    step = lambda g, tok=p, par=p, n=30, s=0: lib.avsr_beam_ngram_step(None if g is None else C.byref(g), tok, par, n, s, None)
    assert step(None) == -1 and step(ok, tok=None) == -1 and step(ok, par=None) == -1           # AVSR_ERR_ARG
    assert step(ok, n=0) == -1 and step(ok, n=29) == -1 and step(ok, s=-1) == -1
    assert step(ng(start=5)) == -1 and step(ng(n_arcs=30)) == -1 and step(ng(lm_weight=float("nan"))) == -1 and step(ng(logp=None)) == -1
    assert step(ng(n_nodes=MN + 1)) == -3 and step(ng(n_arcs=MA + 1)) == -3                     # AVSR_ERR_UNSUPPORTED
    # the fused search: NULL descriptors, a non-beam mode, vocabulary / row-count mismatch, a CTC step that reads another buffer
    d = _lib.AttnRnn()
    d.mode, d.V, d.B, d.beam_width, d.eos_id = 3, 31, 30, 10, 29
    fwd = lambda dd, g, c=None: lib.avsr_attn_rnn_fwd_ngram(None if dd is None else C.byref(dd), None if g is None else C.byref(g),
                                                            None if c is None else C.byref(c), 0, 1, None)
    assert fwd(None, ok) == -1 and fwd(d, None) == -1
    assert fwd(d, ng(V=15)) == -1 and fwd(d, ng(n_rows=20)) == -1 and fwd(d, ng(n_nodes=MN + 1)) == -3
    c = _lib.BeamCtc()
    c.n_utt, c.beam_width, c.T, c.V, c.eos_id, c.weight, c.ld = 3, 10, 12, 31, 29, 0.3, 32
    c.z = c.in_len = c.y = c.state = c.psi = c.last = c.term = c.extra = p
    assert lib.avsr_beam_ctc_supported(C.byref(c)) == 1
    c.lm_logp = 128                                                                              # not the n-gram's buffer
    assert fwd(d, ok, c) == -1
    c.lm_logp, c.beam_width, c.n_utt = p, 3, 10                                                  # another beam width than the decoder's
    assert fwd(d, ok, c) == -1
    d.mode = 1
    assert fwd(d, ok) == -1
    assert lib.avsr_sizeof(b"avsr_beam_ngram") == C.sizeof(_lib.BeamNgram) and lib.avsr_abi_version() == 2


def test_avsr_refuses_what_the_ngram_fusion_does_not_cover(tmp_path, monkeypatch):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import _lib
    uf = _unit_file(tmp_path)
    arpa = _arpa(tmp_path, uf)
    kw = dict(unit="character", unit_file=uf, ngram_lm=arpa)
    for algo in ("greedy", "ctc_prefix_beam_search", "attention_rescoring"):
        with pytest.raises(ValueError, match="ngram_lm needs decoding_algorithm='beam_search'.*ctc_ngram_lm"):
            avsr.AVSR(decoding_algorithm=algo, use_ctc=True, **kw)
    ck = _lm_checkpoint(tmp_path, uf, units_per_layer=(12,), embedding_size=8)
    with pytest.raises(ValueError, match="two language models"):
        avsr.AVSR(lm_checkpoint=ck, lm_units_per_layer=(12,), lm_embedding_size=8, **kw)
    with pytest.raises(ValueError, match="is not a unit"):        # a model over symbols the unit file lacks
        avsr.AVSR(**dict(kw, unit_file=_unit_file(tmp_path, "abcdefghijkl")))
    bad = os.path.join(str(tmp_path), "bad.arpa")
    open(bad, "w").write("\\data\\\nngram 2=1\n\n\\2-grams:\n-1.0 a b\n\n\\end\\\n")
    with pytest.raises(ValueError, match="1-grams"):
        avsr.AVSR(**dict(kw, ngram_lm=bad))
    with pytest.raises((ValueError, OSError)):
        avsr.AVSR(**dict(kw, ngram_lm=os.path.join(str(tmp_path), "no_such.arpa")))
    for w in (float("nan"), -0.5, float("inf")):
        with pytest.raises(ValueError, match="lm_weight"):
            avsr.AVSR(lm_weight=w, **kw)
    with pytest.raises(ValueError, match="ngram_lm"):
        avsr.LM(unit="character", unit_file=uf, ngram_lm=arpa)
    monkeypatch.setattr(_lib, "CTC_PREFIX_NGRAM_MAX_ARCS", 40)       # tables outside avsr_beam_ngram_supported
    with pytest.raises(ValueError, match="arcs"):
        avsr.AVSR(**kw)

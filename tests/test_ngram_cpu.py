"""Back-off n-gram language models, the parts that need no GPU (avsr-tf1_amd/ngram.py): the ARPA format out and in, the Witten-Bell
estimator against its formula, the compiled automaton walked in numpy against the dictionary reference of tests/ref_ngram.py, the
fused search rule of tests/ref_ctc_prefix_lm.py run with an n-gram, the C entry points' argument and limit answers, and what
`AVSR(ctc_ngram_lm=...)` refuses on the host."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ref_ctc_prefix as R
import ref_ctc_prefix_lm as RL
import ref_ngram as RN
from test_beam_lm_cpu import _lm_checkpoint, _unit_file

LN10 = math.log(10.0)
# found by searching seeds 0..199 with R.reentered under the fused rule with the shared n-grams of orders 1, 2 and 4 (V = 5: two real
# units; seed 119 is the first that all three orders share)
REENTRY_NGRAM = dict(V=5, T=12, W=3, L_max=8, s=1.0, seed=119, w=0.5, beta=0.5)


# ------------------------------------------------------------------------------------------------
# 1. ARPA
@pytest.mark.parametrize("order", [1, 2, 3])
def test_arpa_round_trip_gives_the_identical_model(tmp_path, order):
    from avsr_tf1_amd import ngram
    V = 15
    ud = RN.unit_dict(V)
    m = ngram.estimate(RN.sentences(V, n=60), order, ud)
    path = str(tmp_path / "m.arpa")
    ngram.write_arpa(path, m, ud)
    back = ngram.read_arpa(path, ud)
    assert back == m and back.order == order and [len(g) for g in back.grams] == [len(g) for g in m.grams]
    text = open(path).read()
    assert text.startswith("\\data\\\nngram 1=%d\n" % len(m.grams[0])) and text.rstrip().endswith("\\end\\")
    assert "<space>" in text and "<s>" in text and "</s>" in text and "\tu2" in text          # the unit ' ', GO, EOS, a multi-character unit
    ngram.write_arpa(path, back, ud)
    assert open(path).read() == text


HAND = """some toolkit's banner

\\data\\
ngram 1=6
ngram 2=4
ngram 3=2

\\1-grams:
-99\t<s>\t-0.30103
-1.0\t</s>
-0.5 <space> -0.25
-0.75\tu2\t-0.125
-2.0\t<unk>\t-0.5
-1.25 u3

\\2-grams:
-0.25\t<s> u2\t-0.0625
-0.5\tu2 <space>
-0.125\t<unk> u2\t-0.5
-0.375\t<space> </s>

\\3-grams:
-0.0625\t<s> u2 <space>
-0.03125\tu2 <unk> u3

\\end\\
"""


def test_a_hand_written_file_with_missing_backoff_columns_unk_entries_and_space(tmp_path):
    from avsr_tf1_amd import ngram
    V = 8                                                       # MASK, ' ', u2 .. u5, EOS = 6, GO = 7
    ud = RN.unit_dict(V)
    path = str(tmp_path / "hand.arpa")
    open(path, "w").write(HAND)
    m = ngram.read_arpa(path, ud)
    assert m.order == 3
    assert m.grams[0] == {(7,): (-99.0, -0.30103), (6,): (-1.0, 0.0), (1,): (-0.5, -0.25), (2,): (-0.75, -0.125), (3,): (-1.25, 0.0)}
    assert m.grams[1] == {(7, 2): (-0.25, -0.0625), (2, 1): (-0.5, 0.0), (1, 6): (-0.375, 0.0)}        # the <unk> bigram is dropped
    assert m.grams[2] == {(7, 2, 1): (-0.0625, 0.0)}
    ref = RN.NGramRef(m, V)
    lam = ref.lam(())                                            # context (GO): u2 listed, the others back off with bow(GO)
    assert lam[2] == -0.25 * LN10 and lam[1] == (-0.30103 - 0.5) * LN10 and lam[6] == (-0.30103 - 1.0) * LN10
    assert lam[0] == -0.30103 * LN10 + RN.FLOOR and lam[4] == lam[0] and lam[7] == -0.30103 * LN10 + -99.0 * LN10     # MASK, a unit the model lacks, GO
    assert ref.lam((2,))[1] == -0.0625 * LN10                    # the trigram <s> u2 <space>
    assert ref.lam((2, 1))[6] == -0.375 * LN10 and ref.lam((2, 1))[2] == (-0.25 - 0.75) * LN10      # context (u2, ' ') is unlisted: bow 0
    # the same file through the automaton
    t = ngram.compile_tables(m, V, 7, 6)
    _automaton_equals_reference(t, ref, RN.NGramRef(m, V, np.float32), V, exact32=True)
    ngram.write_arpa(path, m, ud)
    assert ngram.read_arpa(path, ud) == m


@pytest.mark.parametrize("bad,match", [
    (HAND.replace("-1.25 u3", "-1.25 zz"), "'zz'"),
    (HAND.replace("\\1-grams:", "\\one-grams:"), "section header"),
    (HAND[:HAND.index("\\1-grams:")] + HAND[HAND.index("\\2-grams:"):], "1-grams"),
    (HAND.replace("ngram 2=4", "ngram 2=5"), "announces"),
    (HAND.replace("-0.5\tu2 <space>", "-0.5\tu2"), "fields"),
    (HAND.replace("-1.0\t</s>", "x\t</s>"), "number"),
    ("no model here\n", "1-grams"),
])
def test_read_arpa_refuses_what_is_no_model_over_the_units(tmp_path, bad, match):
    from avsr_tf1_amd import ngram
    path = str(tmp_path / "bad.arpa")
    open(path, "w").write(bad)
    with pytest.raises(ValueError, match=match):
        ngram.read_arpa(path, RN.unit_dict(8))


# ------------------------------------------------------------------------------------------------
# 2. the estimator
def _counts(seqs, order, go, eos):
    n = {}
    for g in seqs:
        ev = [go] + list(g) + [eos]
        for i in range(1, len(ev)):
            for k in range(1, order + 1):
                if i - k + 1 >= 0:
                    n.setdefault(tuple(ev[i - k + 1:i]), {}).setdefault(ev[i], 0)
                    n[tuple(ev[i - k + 1:i])][ev[i]] += 1
    return n


@pytest.mark.parametrize("order", [1, 2, 4])
def test_estimator_is_witten_bell_and_sums_to_one(order):
    from avsr_tf1_amd import ngram
    V = 15
    seqs = RN.sentences(V, n=300)
    m = ngram.estimate(seqs, order, RN.unit_dict(V))
    ref = RN.NGramRef(m, V)
    go, eos = V - 1, V - 2
    events = list(range(1, V - 2)) + [eos]
    n = _counts(seqs, order, go, eos)

    def p(c, h):                                                 # the formula, recursively, from the counts
        low = 1.0 / len(events) if not h else p(c, h[1:])
        d = n.get(h)
        if not d:
            return low
        tot, t = sum(d.values()), len(d)
        return (d.get(c, 0) + t * low) / (tot + t)

    contexts = [h for h in n if len(h) == order - 1 or (h and h[0] == go)]        # what a label sequence can have as its context
    rng = np.random.default_rng(1)
    unseen = [tuple(int(x) for x in rng.integers(1, V - 2, size=order - 1)) for _ in range(20)] if order > 1 else []
    assert contexts and (order < 4 or any(h not in n for h in unseen))
    for h in contexts + unseen:
        vals = np.array([ref.value(c, h) for c in events])
        assert abs(np.exp(vals).sum() - 1.0) <= 1e-9, (h, np.exp(vals).sum())
        for c, v in zip(events, vals):
            assert abs(v - math.log(p(c, h))) <= 1e-12, (h, c)
    for h, d in n.items():                                       # what is listed: the seen k-grams, every unit and EOS, GO as -99
        for c in d:
            assert h + (c,) in m.grams[len(h)]
        if h and len(h) < order:
            t = len(d)
            assert abs(m.grams[len(h) - 1][h][1] * LN10 - math.log(t / (sum(d.values()) + t))) <= 1e-12
    assert set(m.grams[0]) == {(c,) for c in events} | {(go,)} and m.grams[0][(go,)][0] == -99.0
    assert all(len(g) == k + 1 for k, t in enumerate(m.grams) for g in t)
    with pytest.raises(ValueError, match="order"):
        ngram.estimate(seqs, 0, RN.unit_dict(V))
    with pytest.raises(ValueError, match="real unit"):
        ngram.estimate([[1, V - 1]], 2, RN.unit_dict(V))


# ------------------------------------------------------------------------------------------------
# 3. the compiled automaton
def _automaton_equals_reference(t, ref, ref32, V, exact32, rng=None, n_seq=0):
    """Every node and class: the numpy walk against the dictionary rule (float64 within NGRAM_PARITY; the float32 dictionary form bit
    for bit where every context is listed).  Then the node the transitions reach after label sequences longer than the order."""
    from avsr_tf1_amd import ngram
    assert t["n_nodes"] == len(t["contexts"]) == len(t["bow"]) == len(t["backoff"]) == len(t["arc_begin"]) - 1
    assert t["n_arcs"] == len(t["sym"]) == len(t["logp"]) == len(t["next"]) == t["arc_begin"][-1]
    assert t["contexts"][0] == () and t["arc_begin"][1] == V and (t["sym"][:V] == np.arange(V)).all()
    assert t["bow"].dtype == t["logp"].dtype == np.float32 and all(t[k].dtype == np.int32 for k in ("backoff", "arc_begin", "sym", "next"))
    assert not np.isnan(t["logp"]).any() and np.isfinite(t["logp"]).all() and np.isfinite(t["bow"]).all()
    for i, h in enumerate(t["contexts"]):
        lo, hi = t["arc_begin"][i], t["arc_begin"][i + 1]
        assert (np.diff(t["sym"][lo:hi]) > 0).all() and hi >= lo              # (a listed context may have no continuation)
        assert t["contexts"][t["backoff"][i]] == (h[1:] if i else ()) or len(t["contexts"][t["backoff"][i]]) < len(h) - 1
        for c in range(V):
            v, arc = ngram.walk(t, i, c)
            assert v.dtype == np.float32
            assert abs(float(v) - float(ref.value(c, h))) <= RN.NGRAM_PARITY, (h, c, v, ref.value(c, h))
            if exact32:
                assert v == ref32.value(c, h), (h, c)
            nh = t["contexts"][t["next"][arc]]                    # a suffix of h.c, and the longest that is a node
            hc = h + (c,)
            assert hc[len(hc) - len(nh):] == nh or nh == ()
            assert not any(hc[j:] in t["contexts"] for j in range(max(len(hc) - (t["order"] - 1), 0), len(hc) - len(nh))) or t["order"] == 1
    for _ in range(n_seq):
        g = [int(x) for x in rng.integers(1, V - 2, size=int(rng.integers(t["order"] + 1, t["order"] + 6)))]
        node = t["start"]
        for i, c in enumerate(g):
            row = np.array([ngram.walk(t, node, k)[0] for k in range(V)])
            assert np.abs(row - ref.lam(g[:i])).max() <= RN.NGRAM_PARITY, (g, i)
            node = int(t["next"][ngram.walk(t, node, c)[1]])
        h = ref.context(g)                                      # the node: the longest suffix of the context that is a node
        assert t["contexts"][node] == next(h[j:] for j in range(len(h) + 1) if h[j:] in t["contexts"])


@pytest.mark.parametrize("order", [1, 2, 4])
def test_automaton_equals_the_dictionary_rule_on_the_shared_models(order):
    V = 31
    e = RN.shared_model(order, V)
    t = e["tables"]
    _automaton_equals_reference(t, e["ref"], e["ref32"], V, exact32=True, rng=np.random.default_rng(order), n_seq=30)
    width = np.diff(t["arc_begin"])
    if order == 1:
        assert t["n_nodes"] == 1 and t["n_arcs"] == V and t["start"] == 0
    else:
        assert t["contexts"][t["start"]] == (V - 1,) and width[1:].max() > 16                            # a node with more than 16 arcs
    if order == 4:
        assert (width[1:] == 1).any()                                                                    # a node with a single arc
        eos_only = [i for i in range(1, t["n_nodes"]) if width[i] == 1 and t["sym"][t["arc_begin"][i]] == V - 2]
        assert eos_only, "no context whose only continuation is EOS"
    assert t["logp"][0] == np.float32(RN.FLOOR) and t["logp"][V - 1] == np.float32(RN.FLOOR) and t["next"][0] == 0      # MASK, GO at the root


def test_automaton_on_a_sparse_order_4_model_backs_off_more_than_one_level():
    from avsr_tf1_amd import ngram
    V = 12
    m = RN.sparse_model(V)
    ref, ref32 = RN.NGramRef(m, V), RN.NGramRef(m, V, np.float32)
    t = ngram.compile_tables(m, V, V - 1, V - 2)
    implied = [h for h in t["contexts"] if h and h not in m.grams[len(h) - 1]]
    assert implied, "no context that appears only inside higher-order entries"
    _automaton_equals_reference(t, ref, ref32, V, exact32=False, rng=np.random.default_rng(4), n_seq=60)
    depth = first = last = 0
    for i, h in enumerate(t["contexts"]):                        # walks that leave two or more levels; hits on a node's first and last arc
        for c in range(V):
            node, d = i, 0
            while node:
                lo, hi = t["arc_begin"][node], t["arc_begin"][node + 1]
                if c in t["sym"][lo:hi]:
                    first += hi - lo > 1 and t["sym"][lo] == c
                    last += hi - lo > 1 and t["sym"][hi - 1] == c
                    break
                node, d = t["backoff"][node], d + 1
            depth = max(depth, d)
    assert depth >= 3 and first and last
    for h in [h for h in implied if h in t["contexts"]][:5]:       # a listed-nowhere context carries no weight
        assert t["bow"][t["contexts"].index(h)] == 0.0


def test_compile_tables_refuses_what_does_not_fit():
    from avsr_tf1_amd import ngram
    m = RN.shared_model(2, 15)["model"]
    with pytest.raises(ValueError, match="classes"):
        ngram.compile_tables(m, 10, 9, 8)
    with pytest.raises(ValueError, match="GO and EOS"):
        ngram.compile_tables(m, 15, 15, 13)
    with pytest.raises(ValueError, match="16"):
        ngram.compile_tables(ngram.NGramModel(17, [m.grams[0]] + [{}] * 16), 15, 14, 13)
    with pytest.raises(ValueError, match="one table per order"):
        ngram.NGramModel(2, [m.grams[0]])


# ------------------------------------------------------------------------------------------------
# 4. the search rule with an n-gram
@pytest.mark.parametrize("order", [1, 2, 4])
def test_weight_zero_is_the_plain_search(order):
    V, T, W, L, s = RL.SEARCH_CONFIGS[0]
    ref = RN.shared_model(order, V)["ref"]
    for seed in range(4):
        z = R.kernel_inputs(V, T, s, seed)
        a, b = R.search(z, T, W, L), RL.search_lm(z, T, W, L, ref, 0.0, 0.0)
        assert a["beam"] == b["beam"] and a["margin"] == b["margin"]               # FLOOR is finite: 0 * lam is an exact zero


@pytest.mark.parametrize("order", [1, 2, 4])
@pytest.mark.parametrize("w,beta", [(0.5, 0.5), (0.3, 0.0)])
def test_unpruned_final_is_ctc_plus_weighted_lm_plus_length_bonus(order, w, beta):
    V, T = 5, 3                                                 # classes 0 .. 4 may all be emitted: MASK, GO and EOS get their floor / value
    m = RN.shared_model(order, 15)["model"]
    from avsr_tf1_amd import ngram
    small = ngram.NGramModel(m.order, [{g: v for g, v in t.items() if all(c in (1, 2, 13, 14) for c in g)} for t in m.grams])
    small = ngram.NGramModel(m.order, [{tuple({13: 3, 14: 4}.get(c, c) for c in g): v for g, v in t.items()} for t in small.grams])
    ref = RN.NGramRef(small, V)
    z = R.kernel_inputs(V, T, 2.0, 11)
    want = R.brute_force(R.log_softmax(z))
    out = RL.search_lm(z, T, 256, T, ref, w, beta)
    got = dict(out["beam"])
    assert set(got) == set(want)
    for g, f in got.items():
        assert abs(f - (want[g] + w * ref.s_lm(g) + beta * len(g))) <= 1e-12 * max(1.0, abs(f)), (g, f)
    assert any(abs(f) > 50 for f in got.values())                # sequences through MASK or GO carry the floor


def test_the_ngram_changes_what_is_kept():
    V, T, W, L, s = RL.SEARCH_CONFIGS[0]
    moved = 0
    for order in (1, 2, 4):
        ref = RN.shared_model(order, V)["ref"]
        for seed in range(8):
            z = R.kernel_inputs(V, T, s, seed)
            moved += [g for g, _p in R.search(z, T, W, L)["beam"]] != [g for g, _p in RL.search_lm(z, T, W, L, ref, 0.5, 0.5)["beam"]]
    assert moved >= 12, moved


@pytest.mark.parametrize("order", [1, 2, 4])
def test_the_reentry_input_holds_a_prefix_that_leaves_the_beam_and_returns(order):
    c = REENTRY_NGRAM
    ref = RN.shared_model(order, c["V"])["ref"]
    z = R.kernel_inputs(c["V"], c["T"], c["s"], c["seed"])
    out = RL.search_lm(z, c["T"], c["W"], c["L_max"], ref, c["w"], c["beta"])
    hits = R.reentered(out["beams"])
    assert hits and hits[0][0] < c["T"], hits                                     # ... with a frame left in which its extension merges
    assert out["margin"] > RN.search_tol(out, c["w"])                             # the GPU test may compare the whole search
    for beam in out["beams"]:
        assert len({g for g, _a, _b in beam}) == len(beam)


@pytest.mark.parametrize("order", [1, 2, 4])
def test_the_reference_alone_leaves_out_at_most_a_third_of_the_seeds(order):
    """The cap of the GPU whole-search test is a condition on the inputs: checked here on the smallest configuration (the others are in
    tests/ref_ngram.py's docstring; the GPU test asserts the cap on all of them)."""
    assert RN.left_out_by_the_reference(order, RL.SEARCH_CONFIGS[0]) <= 64 // 3


# ------------------------------------------------------------------------------------------------
# 5. entry points and refusals
def test_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    sup = lib.avsr_ctc_prefix_ngram_supported                   # (V, beam_width, L_max, n_nodes, n_arcs)
    MN, MA = _lib.CTC_PREFIX_NGRAM_MAX_NODES, _lib.CTC_PREFIX_NGRAM_MAX_ARCS
    assert sup(_lib.CTC_PREFIX_MAX_V, 16, _lib.CTC_PREFIX_MAX_L, MN, MA) == 1 and sup(1, 1, 1, 1, 1) == 1 and sup(31, 10, 150, 1, 31) == 1
    assert sup(_lib.CTC_PREFIX_MAX_V + 1, 16, 512, 1, 1000) == 0 and sup(256, 17, 512, 1, 256) == 0 and sup(256, 16, 513, 1, 256) == 0
    assert sup(256, 16, 512, MN + 1, MA) == 0 and sup(256, 16, 512, MN, MA + 1) == 0
    assert sup(31, 10, 150, 0, 31) == 0 and sup(31, 10, 150, 1, 30) == 0 and sup(0, 10, 150, 1, 31) == 0      # the root alone holds V arcs
    p = 64                                                      # any non-NULL address: the checks return before a launch could read it

    def args(**over):
        a = _lib.CtcPrefixArgs()
        a.B, a.T, a.V, a.beam_width, a.L_max, a.ld = 3, 50, 31, 10, 150, 32
        a.z = a.in_len = a.ids = a.lens = a.score = p
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def ng(**over):
        g = _lib.CtcPrefixNgram()
        g.n_nodes, g.n_arcs, g.V, g.start, g.go_id, g.eos_id, g.weight, g.bonus = 5, 60, 31, 1, 30, 29, 0.3, 0.0
        g.bow = g.backoff = g.arc_begin = g.sym = g.logp = g.next = g.s_lm = g.lm_steps = p
        for k, v in over.items():
            setattr(g, k, v)
        return g

    run = lambda a, g: lib.avsr_ctc_prefix_search_ngram(None if a is None else C.byref(a), None if g is None else C.byref(g), None)
    assert run(None, ng()) == -1 and run(args(), None) == -1
    for n in ("z", "in_len", "ids", "lens", "score"):
        assert run(args(**{n: None}), ng()) == -1, n
    for n in ("bow", "backoff", "arc_begin", "sym", "logp", "next", "s_lm", "lm_steps"):
        assert run(args(), ng(**{n: None})) == -1, n
    assert run(args(B=0), ng()) == -1 and run(args(T=0), ng()) == -1 and run(args(ld=31), ng()) == -1
    assert run(args(trace_parent=p), ng()) == -1
    assert run(args(), ng(V=15)) == -1 and run(args(), ng(go_id=31)) == -1 and run(args(), ng(eos_id=-1)) == -1
    assert run(args(), ng(start=5)) == -1 and run(args(), ng(start=-1)) == -1 and run(args(), ng(n_arcs=30)) == -1 and run(args(), ng(n_nodes=0)) == -1
    assert run(args(), ng(weight=-0.1)) == -1 and run(args(), ng(weight=float("inf"))) == -1 and run(args(), ng(weight=float("nan"))) == -1
    assert run(args(), ng(bonus=float("nan"))) == -1 and run(args(), ng(bonus=float("-inf"))) == -1
    assert run(args(beam_width=17), ng()) == -3 and run(args(L_max=513), ng()) == -3
    assert run(args(), ng(n_nodes=MN + 1)) == -3 and run(args(), ng(n_arcs=MA + 1)) == -3
    assert run(args(V=257, ld=258), ng(V=257, go_id=256, eos_id=255, n_arcs=300)) == -3
    assert run(args(beam_width=17, z=None), ng()) == -1          # an argument error comes first
    assert lib.avsr_sizeof(b"avsr_ctc_prefix_ngram") == C.sizeof(_lib.CtcPrefixNgram) and lib.avsr_abi_version() == 2


def _arpa(tmp_path, uf, order=2):
    from avsr_tf1_amd import ngram
    from avsr_tf1_amd.io_utils import create_unit_dict
    ud = create_unit_dict(unit_file=uf)
    path = os.path.join(str(tmp_path), "lm%d.arpa" % order)
    rng = np.random.default_rng(0)
    ngram.write_arpa(path, ngram.estimate([[int(x) for x in rng.integers(1, len(ud) - 3, size=5)] for _ in range(30)], order, ud), ud)
    return path


def test_avsr_refuses_what_the_ngram_search_does_not_cover(tmp_path, monkeypatch):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import _lib
    uf = _unit_file(tmp_path)
    arpa = _arpa(tmp_path, uf)
    kw = dict(unit="character", unit_file=uf, use_ctc=True, decoding_algorithm="ctc_prefix_beam_search", ctc_ngram_lm=arpa)
    for algo in ("greedy", "beam_search", "attention_rescoring"):
        with pytest.raises(ValueError, match="ctc_ngram_lm needs decoding_algorithm='ctc_prefix_beam_search'"):
            avsr.AVSR(**dict(kw, decoding_algorithm=algo))
    ck = _lm_checkpoint(tmp_path, uf, units_per_layer=(12,), embedding_size=8)
    with pytest.raises(ValueError, match="two language models"):
        avsr.AVSR(ctc_lm_checkpoint=ck, lm_units_per_layer=(12,), lm_embedding_size=8, **kw)
    with pytest.raises(ValueError, match="16"):
        avsr.AVSR(beam_width=17, **kw)
    with pytest.raises(ValueError, match="is not a unit"):        # a model over symbols the unit file lacks
        avsr.AVSR(**dict(kw, unit_file=_unit_file(tmp_path, "abcdefghijkl")))
    bad = os.path.join(str(tmp_path), "bad.arpa")
    open(bad, "w").write("\\data\\\nngram 2=1\n\n\\2-grams:\n-1.0 a b\n\n\\end\\\n")
    with pytest.raises(ValueError, match="1-grams"):
        avsr.AVSR(**dict(kw, ctc_ngram_lm=bad))
    for name in ("ctc_lm_weight", "ctc_lm_length_bonus"):
        with pytest.raises(ValueError, match=name):
            avsr.AVSR(**{name: float("nan")}, **kw)
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(**dict(kw, use_ctc=False))
    monkeypatch.setattr(_lib, "CTC_PREFIX_NGRAM_MAX_ARCS", 40)       # tables outside avsr_ctc_prefix_ngram_supported
    with pytest.raises(ValueError, match="arcs"):
        avsr.AVSR(**kw)


def test_train_ngram_tool_writes_an_arpa_from_a_label_record_and_from_text(tmp_path):
    import importlib.util
    from avsr_tf1_amd import io_utils as IO, ngram
    spec = importlib.util.spec_from_file_location("train_ngram", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                              "tools", "train_ngram.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    uf = _unit_file(tmp_path)
    ud = IO.create_unit_dict(unit_file=uf)
    rev = {s: i for i, s in ud.items()}
    lines = ["a cab", "abba a", "cab", "b"]
    rec, txt = str(tmp_path / "labels.tfrecord"), str(tmp_path / "text.txt")
    with IO.TFRecordFileWriter(rec) as f:
        for i, l in enumerate(lines):
            f.write(IO.make_label_example("utt%d" % i, [rev[c] for c in l], "character"))
    open(txt, "w").write("\n".join(lines) + "\n")
    want = ngram.estimate([[rev[c] for c in l] for l in lines], 3, ud)
    for src in (rec, txt):
        out = str(tmp_path / "out.arpa")
        assert tool.main([uf, src, "3", out]) == 0
        assert ngram.read_arpa(out, ud) == want

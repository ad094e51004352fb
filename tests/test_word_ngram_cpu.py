"""The word-level n-gram behind a lexicon trie, host side (avsr-tf1_amd/ngram.py: read_word_arpa / write_word_arpa /
compile_word_tables / word_step / word_lam), without a GPU: word ARPA files, the compiled tables against the
string-and-dictionary reference of tests/ref_word_ngram.py exhaustively over a small alphabet, the identity s_lm telescopes to, the
conditions the GPU tests put on their inputs (every row of the rule's table is met; the near-tie cap), and every refusal by message."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import ref_ctc_prefix_lm as RL
import ref_ngram as RN
import ref_word_ngram as RW
from test_beam_lm_cpu import _lm_checkpoint, _unit_file

HAND = """\\data\\
ngram 1=6
ngram 2=3

\\1-grams:
-99\t<s>\t-0.3
-0.9\t</s>
-0.7\tcab\t-0.25
-0.8\ta\t-0.5
-1.1\tdon't
-1.2\t<unk>\t-0.1

\\2-grams:
-0.2\t<s> cab
-0.4\tcab a
-0.6\ta </s>

\\end\\
"""


def _hand(tmp_path, text=HAND, name="hand.arpa"):
    path = os.path.join(str(tmp_path), name)
    open(path, "w").write(text)
    return path


# ------------------------------------------------------------------------------------------------
# 1. word ARPA files
@pytest.mark.parametrize("order,unk", RW.MODELS)
def test_word_arpa_round_trip_gives_the_identical_model(tmp_path, order, unk):
    from avsr_tf1_amd import ngram
    e = RW.shared_model(order, 15, unk)
    path = str(tmp_path / "w.arpa")
    ngram.write_word_arpa(path, e["model"], e["vocabulary"])
    back, vocabulary = ngram.read_word_arpa(path)
    assert back == e["model"] and vocabulary == e["vocabulary"] and (RW.UNK in vocabulary) == unk
    text = open(path).read()
    ngram.write_word_arpa(path, back, vocabulary)
    assert open(path).read() == text and "<s>" in text and "</s>" in text


def test_word_arpa_reads_a_hand_written_file_and_keeps_unk(tmp_path):
    from avsr_tf1_amd import ngram
    m, voc = ngram.read_word_arpa(_hand(tmp_path))
    assert voc == ["<s>", "</s>", "<unk>", "a", "cab", "don't"] and m.order == 2 and [len(g) for g in m.grams] == [6, 3]
    assert m.grams[0][(2,)] == (-1.2, -0.1) and m.grams[1][(0, 4)] == (-0.2, 0.0)
    ud = RW.unit_dict(7)                                                    # letters a, b, c: "don't" cannot be spelled
    t = ngram.compile_word_tables(m, voc, ud, -3.0)
    assert t["n_unspellable"] == 1 and t["unk_id"] == 2 and (t["Vw"], t["go_w"], t["eos_w"]) == (6, 0, 1)
    assert (t["V"], t["space_id"], t["eos_id"], t["go_id"]) == (7, 1, 5, 6) and t["oov_score"] == -3.0
    assert t["n_trie_nodes"] == 5 and t["n_trie_arcs"] == 4                   # root, a, c, ca, cab
    assert list(t["t_begin"]) == [0, 2, 2, 3, 4, 4] and list(t["t_sym"]) == [2, 4, 2, 3] and list(t["t_next"]) == [1, 2, 3, 4]
    assert list(t["t_word"]) == [-1, 3, -1, -1, 4]


def test_word_arpa_file_refusals(tmp_path):
    from avsr_tf1_amd import ngram
    for text, match in ((HAND.replace("\\1-grams:", "\\one-grams:"), "not a section header"),
                        ("\\data\\\nngram 2=1\n\n\\2-grams:\n-1.0 a b\n\n\\end\\\n", "1-grams"),
                        (HAND.replace("-0.8\ta\t-0.5", "-0.8\ta b\t-0.5\t7"), "fields"),
                        (HAND.replace("-0.8\ta", "zero\ta"), "not a number"),
                        (HAND.replace("ngram 2=3", "ngram 2=4"), "announces 4 2-grams"),
                        ("\\data\\\n\n\\1-grams:\n-1.0 a\n\n\\3-grams:\n-1.0 a a a\n\n\\end\\\n", "no \\\\2-grams: section")):
        with pytest.raises(ValueError, match=match):
            ngram.read_word_arpa(_hand(tmp_path, text, "bad.arpa"))


def test_compile_word_tables_refusals(tmp_path):
    from avsr_tf1_amd import ngram
    m, voc = ngram.read_word_arpa(_hand(tmp_path))
    ud = RW.unit_dict(7)
    with pytest.raises(ValueError, match="needs the unit ' '"):
        ngram.compile_word_tables(m, voc, {k: ("_" if v == " " else v) for k, v in ud.items()})
    with pytest.raises(ValueError, match="single-character units"):
        ngram.compile_word_tables(m, voc, RN.unit_dict(7))                   # "u2", "u3": a phoneme-style list
    with pytest.raises(ValueError, match="no word of the model can be spelled"):
        ngram.compile_word_tables(m, voc, {k: (v.upper() if len(v) == 1 else v) for k, v in ud.items()})
    for bad in (0.5, float("nan"), float("-inf"), float("inf")):
        with pytest.raises(ValueError, match="out-of-vocabulary score"):
            ngram.compile_word_tables(m, voc, ud, bad)
    deep = ngram.NGramModel(17, [{(3,) * k: (-1.0, 0.0)} for k in range(1, 18)])
    with pytest.raises(ValueError, match="orders of up to 16"):
        ngram.compile_word_tables(deep, voc, ud)
    assert ngram.compile_word_tables(m, voc, ud, 0.0)["oov_score"] == 0.0 and ngram.load_word_tables(_hand(tmp_path), ud)["oov_score"] == -10.0


# ------------------------------------------------------------------------------------------------
# 2. the compiled tables against the reference, exhaustively: V = 6 (a 7-class alphabet with the blank; two letters), every label
# sequence of up to 5 classes -- MASK, GO and EOS inside a sequence included
def _trie_strings(t):
    """trie node -> the letters that lead to it (test-side knowledge of the compiled trie; WordRef has none)."""
    out, todo = {0: ""}, [0]
    while todo:
        n = todo.pop()
        for a in range(int(t["t_begin"][n]), int(t["t_begin"][n + 1])):
            out[int(t["t_next"][a])] = out[n] + RW.letter(int(t["t_sym"][a]))
            todo.append(int(t["t_next"][a]))
    return out


@pytest.mark.parametrize("order,unk", RW.MODELS)
def test_tables_equal_the_reference_on_every_short_label_sequence(order, unk):
    from avsr_tf1_amd import ngram
    V = 6
    e = RW.shared_model(order, V, unk)
    t, ref, ref32, voc = e["tables"], e["ref"], e["ref32"], e["vocabulary"]
    strings = _trie_strings(t)
    assert len(strings) == t["n_trie_nodes"] and {s for n, s in strings.items() if t["t_word"][n] >= 0} == ref.words
    contexts = set(t["contexts"])
    states, worst = {(): ngram.word_start(t)}, 0.0
    for g in RW.all_sequences(V, 5):
        if g:
            states[g] = ngram.word_step(t, states[g[:-1]], g[-1])
        h, p = states[g]
        hist, cur = ref.state(g)
        assert (strings[p] if p >= 0 else None) == cur, (g, p, cur)
        ids = tuple(voc.index(w) for w in hist)
        want = next(ids[i:] for i in range(len(ids) + 1) if ids[i:] in contexts)     # the longest suffix that is a node
        assert t["contexts"][h] == want, (g, h, hist)
        row = ngram.word_lam(t, states[g])
        assert row.dtype == np.float32 and np.isfinite(row).all()
        worst = max(worst, float(np.abs(row.astype(np.float64) - ref.lam(g)).max()))
        assert np.array_equal(row, ref32.lam(g)), (g, row, ref32.lam(g))          # the estimator lists every context: bit-equal
    print(order, unk, "largest |lam32 - lam64|", worst)
    assert worst <= RW.WORD_PARITY


# ------------------------------------------------------------------------------------------------
# 3. what s_lm telescopes to, computed independently: the decoded string split on spaces, its words scored by ref_ngram.NGramRef
def _independent_s_lm(e, g, V):
    model, voc = e["model"], e["vocabulary"]
    nref = RN.NGramRef(model, len(voc))
    N, ids, lexicon = model.order, {w: i for i, w in enumerate(voc)}, e["ref"].words
    text = "".join(" " if c == 1 else RW.letter(c) for c in g if 1 <= c < V - 2)
    non_units = sum(1 for c in g if c == 0 or c == V - 1)
    hist, total, n_oov = (ids["<s>"],), 0.0, 0
    for w in text.split(" ") + ["</s>"]:
        if w == "":
            continue                                                      # leading, trailing and doubled spaces close nothing
        if w in lexicon or w == "</s>":
            k = ids[w]
        else:
            n_oov += 1                                                    # paid on leaving the lexicon, or at the close of a proper prefix
            k = ids.get("<unk>")
        if k is None:
            hist = ()                                                     # no <unk>: nothing is scored, the context is emptied
            continue
        h = hist[max(len(hist) - (N - 1), 0):] if N > 1 else ()
        total += float(nref.value(k, h))
        hist = hist + (k,)
    return total + RW.OOV * n_oov + RW.FLOOR * non_units, n_oov


@pytest.mark.parametrize("order,unk", RW.MODELS)
def test_s_lm_is_the_word_score_of_the_decoded_string(order, unk):
    V = 15
    e = RW.shared_model(order, V, unk)
    rng = np.random.default_rng(3)
    words = sorted(e["ref"].words)
    letters = list(range(2, V - 2))
    seen_oov = 0
    for _ in range(300):
        g = []
        for _w in range(int(rng.integers(0, 5))):
            kind = rng.random()
            if kind < 0.6:
                g += [ord(ch) - ord("a") + 2 for ch in words[int(rng.integers(len(words)))]]
            else:
                g += [int(c) for c in rng.choice(letters, size=int(rng.integers(1, 5)))]
            g += [1] * int(rng.integers(0, 3)) + ([0] if rng.random() < 0.1 else []) + ([V - 1] if rng.random() < 0.1 else [])
        want, n_oov = _independent_s_lm(e, g, V)
        seen_oov += n_oov
        assert abs(e["ref"].s_lm(g) - want) <= 1e-9 * max(1.0, abs(want)), (g, e["ref"].s_lm(g), want)
    assert seen_oov


# ------------------------------------------------------------------------------------------------
# 4. conditions on the inputs of the GPU tests, decided by the fp64 reference alone
def _rows_met(cfg, order, unk):
    """How often each row of the rule's table is taken by an extension the fp64 search KEEPS, over the 64 shared inputs."""
    V, T, W, L_max, _s = cfg
    ref = RW.shared_model(order, V, unk)["ref"]
    n = dict(word=0, prefix=0, sink=0, enter_sink=0, root_space=0)
    for r in RW.references(cfg, order, unk)[1]:
        for prev, cur in zip(r["beams"], r["beams"][1:]):
            old = {g for g, _a, _b in prev}
            for g, _a, _b in cur:
                if not g or g in old:
                    continue
                (hist, before), c = ref.state(g[:-1]), g[-1]
                if c == RW.SPACE:
                    n["root_space" if before == "" else ref.close(hist, before)[2]] += 1
                elif c in ref.chars and before is not None and ref.state(g)[1] is None:
                    n["enter_sink"] += 1
    return n


@pytest.mark.parametrize("order,unk", RW.SEARCH_MODELS)
def test_the_kept_beams_of_the_shared_inputs_meet_every_row_of_the_rule(order, unk):
    n = _rows_met(RL.SEARCH_CONFIGS[0], order, unk)
    print(order, unk, n)
    assert all(v > 0 for v in n.values()), n
    assert (RW.shared_model(order, 15, unk)["ref"].unk is not None) == unk    # <unk> present in one model, absent in the other


@pytest.mark.parametrize("order,unk", RW.SEARCH_MODELS)
@pytest.mark.parametrize("cfg", RL.SEARCH_CONFIGS, ids=lambda c: "V%d_T%d_W%d_L%d_s%d" % c)
def test_the_reference_alone_leaves_out_at_most_a_third_of_the_seeds(cfg, order, unk):
    left = RW.left_out_by_the_reference(order, unk, cfg)
    print(cfg, order, unk, "left out", left, "of 64")
    assert left <= 64 // 3


def test_the_inputs_spell_lexicon_words():
    """The boosted alignment decodes to an in-lexicon sentence: the best entry of the fp64 search holds closed lexicon words."""
    V, T, W, L_max, s = RL.SEARCH_CONFIGS[1]
    ref = RW.shared_model(3, V, True)["ref"]
    closed = 0
    for r in RW.references(RL.SEARCH_CONFIGS[1], 3, True)[1][:16]:
        text = "".join(" " if c == 1 else ref.chars.get(c, "?") for c in r["beam"][0][0])
        closed += sum(w in ref.words for w in text.split(" "))
    assert closed >= 16


# ------------------------------------------------------------------------------------------------
# 5. entry points and refusals
def test_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    sup = lib.avsr_ctc_prefix_word_ngram_supported      # (V, beam_width, L_max, n_nodes, n_arcs, Vw, n_trie_nodes, n_trie_arcs)
    MN, MA = _lib.CTC_PREFIX_NGRAM_MAX_NODES, _lib.CTC_PREFIX_NGRAM_MAX_ARCS
    assert sup(_lib.CTC_PREFIX_MAX_V, 16, _lib.CTC_PREFIX_MAX_L, MN, MA, 1000, MN, MA) == 1 and sup(31, 10, 150, 1, 2, 2, 1, 1) == 1
    assert sup(257, 16, 512, 1, 1000, 10, 5, 5) == 0 and sup(256, 17, 512, 1, 256, 10, 5, 5) == 0 and sup(256, 16, 513, 1, 256, 10, 5, 5) == 0
    assert sup(31, 10, 150, MN + 1, MA, 10, 5, 5) == 0 and sup(31, 10, 150, MN, MA + 1, 10, 5, 5) == 0
    assert sup(31, 10, 150, 5, 60, 10, MN + 1, 5) == 0 and sup(31, 10, 150, 5, 60, 10, 5, MA + 1) == 0
    assert sup(31, 10, 150, 0, 60, 10, 5, 5) == 0 and sup(31, 10, 150, 5, 9, 10, 5, 5) == 0 and sup(31, 10, 150, 5, 60, 1, 5, 5) == 0
    assert sup(31, 10, 150, 5, 60, 10, 0, 5) == 0 and sup(31, 10, 150, 5, 60, 10, 5, 0) == 0
    p = 64                                                      # any non-NULL address: the checks return before a launch could read it

    def args(**over):
        a = _lib.CtcPrefixArgs()
        a.B, a.T, a.V, a.beam_width, a.L_max, a.ld = 3, 50, 31, 10, 150, 32
        a.z = a.in_len = a.ids = a.lens = a.score = p
        for k, v in over.items():
            setattr(a, k, v)
        return a

    tables = ("bow", "backoff", "arc_begin", "sym", "logp", "next", "t_begin", "t_sym", "t_next", "t_word", "s_lm", "lm_steps")

    def wg(**over):
        g = _lib.CtcPrefixWordNgram()
        g.n_nodes, g.n_arcs, g.Vw, g.start, g.eos_w, g.unk_id, g.n_trie_nodes, g.n_trie_arcs = 5, 60, 40, 1, 1, -1, 7, 6
        g.V, g.space_id, g.go_id, g.eos_id, g.weight, g.bonus, g.oov = 31, 1, 30, 29, 0.3, 0.0, -10.0
        for k in tables:
            setattr(g, k, p)
        for k, v in over.items():
            setattr(g, k, v)
        return g

    run = lambda a, g: lib.avsr_ctc_prefix_search_word_ngram(None if a is None else C.byref(a), None if g is None else C.byref(g), None)
    assert run(None, wg()) == -1 and run(args(), None) == -1
    for n in ("z", "in_len", "ids", "lens", "score"):
        assert run(args(**{n: None}), wg()) == -1, n
    for n in tables:
        assert run(args(), wg(**{n: None})) == -1, n
    assert run(args(B=0), wg()) == -1 and run(args(T=0), wg()) == -1 and run(args(ld=31), wg()) == -1 and run(args(trace_parent=p), wg()) == -1
    assert run(args(), wg(V=15)) == -1 and run(args(), wg(go_id=31)) == -1 and run(args(), wg(eos_id=-1)) == -1
    assert run(args(), wg(start=5)) == -1 and run(args(), wg(start=-1)) == -1 and run(args(), wg(n_arcs=39)) == -1 and run(args(), wg(n_nodes=0)) == -1
    assert run(args(), wg(eos_w=40)) == -1 and run(args(), wg(eos_w=-1)) == -1 and run(args(), wg(unk_id=40)) == -1 and run(args(), wg(unk_id=-2)) == -1
    assert run(args(), wg(space_id=31)) == -1 and run(args(), wg(space_id=-1)) == -1 and run(args(), wg(space_id=30)) == -1
    assert run(args(), wg(space_id=29)) == -1 and run(args(), wg(go_id=29)) == -1
    assert run(args(), wg(n_trie_nodes=0)) == -1 and run(args(), wg(n_trie_arcs=0)) == -1
    for bad in (0.5, float("nan"), float("-inf"), float("inf")):
        assert run(args(), wg(oov=bad)) == -1, bad
    assert run(args(), wg(weight=-0.1)) == -1 and run(args(), wg(weight=float("inf"))) == -1 and run(args(), wg(weight=float("nan"))) == -1
    assert run(args(), wg(bonus=float("nan"))) == -1 and run(args(), wg(bonus=float("-inf"))) == -1
    assert run(args(beam_width=17), wg()) == -3 and run(args(L_max=513), wg()) == -3
    assert run(args(), wg(n_nodes=MN + 1)) == -3 and run(args(), wg(n_arcs=MA + 1)) == -3
    assert run(args(), wg(n_trie_nodes=MN + 1)) == -3 and run(args(), wg(n_trie_arcs=MA + 1)) == -3
    assert run(args(V=257, ld=258), wg(V=257, go_id=256, eos_id=255)) == -3
    assert run(args(beam_width=17, z=None), wg()) == -1          # an argument error comes first
    assert lib.avsr_sizeof(b"avsr_ctc_prefix_word_ngram") == C.sizeof(_lib.CtcPrefixWordNgram)


def _word_arpa(tmp_path, order=2):
    from avsr_tf1_amd import ngram
    voc = ["<s>", "</s>", "<unk>", "a", "cab", "don't", "it's"]
    rng = np.random.default_rng(0)
    m = ngram.estimate([[int(x) for x in rng.integers(3, len(voc), size=3)] for _ in range(30)], order, ngram.word_dict(voc))
    path = os.path.join(str(tmp_path), "words%d.arpa" % order)
    ngram.write_word_arpa(path, m, voc)
    return path


def test_avsr_refuses_what_the_word_ngram_search_does_not_cover(tmp_path, monkeypatch):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import _lib
    uf = _unit_file(tmp_path)
    arpa = _word_arpa(tmp_path)
    kw = dict(unit="character", unit_file=uf, use_ctc=True, decoding_algorithm="ctc_prefix_beam_search", ctc_word_ngram_lm=arpa)
    for algo in ("greedy", "beam_search", "attention_rescoring"):
        with pytest.raises(ValueError, match="ctc_word_ngram_lm needs decoding_algorithm='ctc_prefix_beam_search'"):
            avsr.AVSR(**dict(kw, decoding_algorithm=algo))
    ck = _lm_checkpoint(tmp_path, uf, units_per_layer=(12,), embedding_size=8)
    with pytest.raises(ValueError, match="ctc_word_ngram_lm and ctc_lm_checkpoint are two language models"):
        avsr.AVSR(ctc_lm_checkpoint=ck, lm_units_per_layer=(12,), lm_embedding_size=8, **kw)
    from avsr_tf1_amd import ngram
    from avsr_tf1_amd.io_utils import create_unit_dict
    ud = create_unit_dict(unit_file=uf)
    units = os.path.join(str(tmp_path), "units.arpa")
    ngram.write_arpa(units, ngram.estimate([[3, 4, 5]], 2, ud), ud)
    with pytest.raises(ValueError, match="ctc_word_ngram_lm and ctc_ngram_lm are two language models"):
        avsr.AVSR(ctc_ngram_lm=units, **kw)
    with pytest.raises(ValueError, match="beam widths of up to 16 \\(got beam_width 17\\)"):
        avsr.AVSR(beam_width=17, **kw)
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
            avsr.AVSR(ctc_word_oov_score=bad, **kw)
    bad = os.path.join(str(tmp_path), "bad.arpa")
    open(bad, "w").write("\\data\\\nngram 2=1\n\n\\2-grams:\n-1.0 a b\n\n\\end\\\n")
    with pytest.raises(ValueError, match="1-grams"):
        avsr.AVSR(**dict(kw, ctc_word_ngram_lm=bad))
    for name in ("ctc_lm_weight", "ctc_lm_length_bonus"):
        with pytest.raises(ValueError, match=name):
            avsr.AVSR(**{name: float("nan")}, **kw)
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(**dict(kw, use_ctc=False))
    monkeypatch.setattr(_lib, "CTC_PREFIX_NGRAM_MAX_ARCS", 5)        # tables outside avsr_ctc_prefix_word_ngram_supported
    with pytest.raises(ValueError, match="word automata and lexicon tries of up to"):
        avsr.AVSR(**kw)


def test_model_refuses_what_the_word_ngram_search_does_not_cover():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    m = object.__new__(Seq2SeqModel)
    m.cfg, m.dev = ModelConfig(use_ctc=True), torch.device("cpu")
    V = m.cfg.vocab_size
    g = dict(V=V, go_id=m.cfg.go_id, eos_id=m.cfg.eos_id, n_nodes=10, n_arcs=50, Vw=40, n_trie_nodes=9, n_trie_arcs=8)
    batch = types.SimpleNamespace(audio=torch.zeros(2, 5, 3), video=None, labels=torch.zeros(2, 4, dtype=torch.int32))
    run = lambda beam_width=4, **kw: m._ctc_prefix_beam_search(batch, beam_width, None, False, **kw)
    lm = types.SimpleNamespace(cfg=types.SimpleNamespace(architecture="lm"), onehot=None)
    for other in (dict(lm=lm), dict(ngram=dict(g))):
        with pytest.raises(ValueError, match="word_ngram \\(word-level tables behind a lexicon\\) cannot be combined with lm or ngram"):
            run(word_ngram=g, **other)
    with pytest.raises(ValueError, match="takes one language model: lm \\(an avsr.LM network\\) or ngram \\(back-off tables\\), not both"):
        run(lm=lm, ngram=dict(g))                                          # the existing pair keeps its text
    with pytest.raises(ValueError, match="the word n-gram tables were compiled for V = %d, GO = 5, EOS = %d" % (V + 2, m.cfg.eos_id)):
        run(word_ngram=dict(g, V=V + 2, go_id=5))
    with pytest.raises(ValueError, match="with a word n-gram avsr_ctc_prefix_search_word_ngram covers beam widths of up to 16 .*got beam width 17"):
        run(beam_width=17, word_ngram=g)
    with pytest.raises(ValueError, match="8 trie arcs"):
        run(word_ngram=dict(g, n_trie_nodes=(1 << 24) + 1))
    with pytest.raises(ValueError, match="lm_weight must be a finite number >= 0"):
        run(word_ngram=g, lm_weight=-1.0)
    with pytest.raises(ValueError, match="length_bonus must be finite"):
        run(word_ngram=g, length_bonus=float("nan"))
    # the public method is keyword-only for the new argument and passes it on only when it is given
    calls = []
    m._redo_if_flagged = lambda fn, *a, **k: calls.append((a, k))
    with pytest.raises(TypeError):
        m.ctc_prefix_beam_search(batch, 4, 9, True, None, 0.5, 0.1, None, g)
    m.ctc_prefix_beam_search(batch, 4, 9, True, None, 0.5, 0.1, None)
    m.ctc_prefix_beam_search(batch, 4, 9, True, None, 0.5, 0.1, None, word_ngram=g)
    assert calls == [((batch, 4, 9, True, None, 0.5, 0.1, None), {}), ((batch, 4, 9, True, None, 0.5, 0.1, None), dict(word_ngram=g))]


def test_train_ngram_tool_writes_a_word_arpa_from_text(tmp_path):
    import importlib.util
    from avsr_tf1_amd import ngram
    spec = importlib.util.spec_from_file_location("train_ngram", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                              "tools", "train_ngram.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    lines = ["a cab", "abba a  cab", "", "cab", "don't a"]
    txt, out = str(tmp_path / "text.txt"), str(tmp_path / "out.arpa")
    open(txt, "w").write("\n".join(lines) + "\n")
    assert tool.main(["--words", txt, "3", out]) == 0
    voc = ["<s>", "</s>", "<unk>", "a", "abba", "cab", "don't"]
    ids = {w: i for i, w in enumerate(voc)}
    want = ngram.estimate([[ids[w] for w in l.split()] for l in lines if l], 3, ngram.word_dict(voc))
    assert ngram.read_word_arpa(out) == (want, voc)

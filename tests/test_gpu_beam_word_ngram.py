"""Word-level n-gram behind a lexicon trie in beam search on the GPU (csrc/beam_word_ngram.hip, avsr_attn_rnn_fwd_word_ngram,
Seq2SeqModel.beam_search_decode(word_ngram=...), AVSR(word_ngram_lm=...)), against the references of tests/ref_beam_word_ngram.py.

* the step kernel alone over the chained steps of ref_beam_word_ngram.chain (symbols drawn from each parent's own state, random
  parents): the (h, p, hc) state equals the host restatement exactly, the rows equal ngram.word_lam BIT FOR BIT (the kernel performs the
  same fp32 additions in the same order: derivable, not a tolerance) and lie within WORD_PARITY of the fp64 string-and-dictionary rule;
  nothing is written past the end, the tables are unchanged, two runs are bit-identical whatever the buffers held, and step 0 ignores tok
  and the stale half;
* tok / parent_rows outside their ranges are clamped;
* the whole search by test_gpu_beam_ngram._follow (unchanged; it is handed the word tables and the word search) in the spaced long setup
  over every architecture, beam-kernel setting, weight and search model minus ref_beam_word_ngram.EXCLUDED; one run per architecture in
  the unmodified setup, where a chunk is queued past the end; one with the CTC term;
* weight 0 and word_ngram=None: byte-identical to the plain search under all three avsr_attn_rnn_set_beam_kernel settings;
* the engine's refusals, the single upload shared with ctc_prefix_beam_search(word_ngram=...), and end to end through
  tools/train_ngram.py --words and AVSR.evaluate.
tests/test_beam_word_ngram_cpu.py recomputes, on the CPU, what the chains and the search cases rest on."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import ref_beam_word_ngram as R
import test_gpu_beam_ngram as TN
from test_gpu_beam_lm import SETTINGS

pytestmark = pytest.mark.gpu
TABLES = ("bow", "backoff", "arc_begin", "sym", "logp", "next", "t_begin", "t_sym", "t_next", "t_word")
SCALARS = ("n_nodes", "n_arcs", "Vw", "start", "eos_w", "unk_id", "n_trie_nodes", "n_trie_arcs", "space_id", "go_id", "eos_id")


def _desc(tables, V, Rn, dev, state, logp, weight=0.3):
    from avsr_tf1_amd import _lib, ops
    D = {k: torch.as_tensor(np.ascontiguousarray(tables[k])).to(dev) for k in TABLES}
    g = _lib.BeamWordNgram()
    for k in SCALARS:
        setattr(g, k, int(tables[k]))
    g.V, g.n_rows, g.lm_weight, g.oov = V, Rn, weight, float(tables["oov_score"])
    for k in TABLES:
        setattr(g, k, ops.fptr(D[k]))
    g.state, g.lm_logp = ops.fptr(state), ops.fptr(logp)
    return g, D


@pytest.mark.parametrize("key", R.MODELS)
@pytest.mark.parametrize("V", R.KERNEL_VS)
@pytest.mark.parametrize("Rn", R.KERNEL_RNS)
def test_step_kernel_state_exact_rows_bit_for_bit(Rn, V, key):
    from avsr_tf1_amd import ops
    dev = torch.device("cuda:0")
    e = R.model(key, V)
    tables, ref = e["tables"], e["ref"]
    steps = R.chain(key, V, Rn)
    assert len(steps) >= 12
    tail = 64
    runs = []
    for stale in (5, max(tables["n_nodes"], tables["n_trie_nodes"]) + 1000):       # what the buffers hold before step 0: small or far outside
        state = torch.full((6 * Rn + tail,), stale, dtype=torch.int32, device=dev)
        logp = torch.full((Rn * V + tail,), 77.0, device=dev)
        g, D = _desc(tables, V, Rn, dev, state, logp)
        assert ops.beam_word_ngram_supported(g)
        before = {k: D[k].clone() for k in TABLES}
        rec = dict(states=[], rows=[])
        for step, st in enumerate(steps):
            if step == 0:                                                  # step 0 reads neither tok ... nor the stale half
                tok_d = torch.full((Rn,), -7 if stale == 5 else V + 50, dtype=torch.int32, device=dev)
            else:
                tok_d = torch.as_tensor(st["tok"]).to(dev)
            ops.beam_word_ngram_step(g, tok_d, torch.as_tensor(st["par"]).to(dev), Rn, step)
            torch.cuda.synchronize()
            sd, lp = state.cpu().numpy(), logp.cpu().numpy()
            assert (sd[6 * Rn:] == stale).all() and (lp[Rn * V:] == 77.0).all(), "written past the end"
            half = (step + 1) & 1
            got_s, got = sd[half * 3 * Rn:(half + 1) * 3 * Rn].reshape(3, Rn), lp[:Rn * V].reshape(Rn, V)
            assert np.array_equal(got_s, st["state"]), (step, got_s, st["state"])
            want = R.host_rows(tables, st["state"][0], st["state"][1])
            assert got.tobytes() == want.tobytes(), (step, np.argwhere(got != want)[:4])
            lam64 = np.stack([ref.lam(h) for h in st["hist"]])
            dev64 = float(np.abs(got.astype(np.float64) - lam64).max())
            assert np.isfinite(got).all() and dev64 <= R.WORD_PARITY, (step, dev64)
            rec["states"].append(got_s.copy())
            rec["rows"].append(got.copy())
        assert all(torch.equal(before[k], D[k]) for k in TABLES), "the tables are read-only"
        runs.append(rec)
    for a, b in zip(runs[0]["states"] + runs[0]["rows"], runs[1]["states"] + runs[1]["rows"]):
        assert a.tobytes() == b.tobytes()                                  # two runs, whatever the buffers held before: bit-identical


def test_step_clamps_foreign_symbols_and_parents():
    """tok / parent_rows outside their ranges are clamped to 0 (nothing outside the buffers is addressed): class 0 is MASK, which leaves
    the state alone, so every row ends at row 0's state."""
    from avsr_tf1_amd import ops
    dev = torch.device("cuda:0")
    V, Rn = 31, 9
    tables = R.model((3, True), V)["tables"]
    state, logp = torch.zeros(6 * Rn, dtype=torch.int32, device=dev), torch.zeros(Rn * V, device=dev)
    g, _D = _desc(tables, V, Rn, dev, state, logp)
    i32 = lambda a: np.asarray(a, np.int32)
    first = int(tables["t_sym"][0])                                        # a letter that starts a word
    seq = [(i32([0] * Rn), i32(range(Rn))), (i32([first] * Rn), i32(range(Rn))),
           (i32([R.SPACE] + [first] * (Rn - 1)), i32(range(Rn))), (i32([-1, V, 1 << 20] * 3), i32([-1, Rn, 1 << 30] * 3))]
    host = np.zeros((3, Rn), np.int32)
    for step, (tok, par) in enumerate(seq):
        ops.beam_word_ngram_step(g, torch.as_tensor(tok).to(dev), torch.as_tensor(par).to(dev), Rn, step)
        host = R.host_step(tables, host, tok, par, step)
    torch.cuda.synchronize()
    row0 = R.host_step(tables, R.host_step(tables, R.host_step(tables, np.zeros((3, 1), np.int32), [0], [0], 0), [first], [0], 1),
                       [R.SPACE], [0], 2)[:, 0]
    assert (host == row0[:, None]).all() and row0[1] == 0 and row0[0] != tables["start"]        # one word closed, MASK changed nothing
    got = state.cpu().numpy().reshape(2, 3, Rn)[0]                         # step 3 wrote half (3 + 1) & 1 = 0
    assert np.array_equal(got, host)
    assert logp.cpu().numpy().reshape(Rn, V).tobytes() == R.host_rows(tables, host[0], host[1]).tobytes()


def _search(model, db, K, tables, lmw, max_steps, check_every=3, ctc_weight=0.0):
    """test_gpu_beam_ngram._search with the tables handed to word_ngram=."""
    out = model.beam_search_decode(db, beam_width=K, max_steps=max_steps, check_every=check_every, return_all=True, word_ngram=tables,
                                   lm_weight=lmw, ctc_weight=ctc_weight)
    torch.cuda.synchronize()
    assert not model.check_persistent()
    X = model._beam_ws[2]
    return dict(out=out.cpu().numpy().copy(), T=out.shape[1], sid=X["sid"].cpu().numpy().copy(), pid=X["pid"].cpu().numpy().copy(),
                logp=X["logp"].cpu().numpy().copy(), ln=X["ln"].cpu().numpy().copy(), fin=X["fin"].cpu().numpy().copy())


@pytest.fixture
def follow(monkeypatch):
    """test_gpu_beam_ngram._follow as it is, with the word model in the two places it looks its model up: `order` is a key of
    ref_beam_word_ngram.model, the search is called with word_ngram=, and the fp64 reference gets the WordRef."""
    # _follow looks its model up in exactly two places: `e = R.model(order)` (its tables for the engine, its `ref` for
    # ref_beam_ngram.beam_search_decode_ngram) and `_search(model, db, K, e["tables"], ...)` (which passes them as ngram=).  Both are
    # replaced here, and `order` travels through _follow untouched, so it may be an (order, unk) key.  A third lookup added to _follow
    # would reach the unit model: it then has to be replaced here too.
    monkeypatch.setattr(TN.R, "model", R.model)
    monkeypatch.setattr(TN, "_search", _search)
    return TN._follow


SEARCHES = [(case, setting, K, lmw, key) for case in R.ARCHS for setting, K in SETTINGS for lmw in R.WEIGHTS for key in R.SEARCH_MODELS
            if (case, K, lmw, key) not in R.EXCLUDED]      # a near-tie at the cut in fp64 is listed, with its gap, in the ref file


@pytest.mark.parametrize("case,setting,K,lmw,key", SEARCHES)
def test_full_search_follows_the_reference(follow, case, setting, K, lmw, key):
    """The spaced long setup: spaces are taken from word ends and from the sink, EOS away from the root (test_beam_word_ngram_cpu.py)."""
    follow(R.spaced_case(case), setting, K, lmw, key, R.LONG_STEPS, what=case)


@pytest.mark.parametrize("case", list(R.ARCHS))
def test_full_search_with_a_chunk_queued_past_the_end(follow, case):
    """The unmodified setup: the search ends after 3-5 steps (tests/test_beam_word_ngram_cpu.py), inside a chunk of four."""
    P = R.PLAIN
    follow(R.plain_case(case), 1, P["K"], P["weight"], P["key"], R.MAX_STEPS, check_every=P["check_every"], past_the_end=True, what=case)


def test_full_search_with_the_ctc_term(follow):
    follow(R.ctc_case("c1_audio_uni_luong"), 1, 10, 0.3, (3, True), R.RB.RC.MAX_STEPS, ctc_weight=0.3, what="ctc")


@pytest.mark.parametrize("setting", [1, 0, 2])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_weight_zero_and_no_tables_are_the_plain_search(case, setting):
    from avsr_tf1_amd import ops
    tables = R.model((3, True))["tables"]
    try:
        ops.attn_rnn_set_beam_kernel(setting)
        model, db = TN._model(R.spaced_case(case))
        a = _search(model, db, 10, None, 0.0, R.LONG_STEPS)
        n = _search(model, db, 10, None, 0.7, R.LONG_STEPS)                # a weight without tables: nothing to weigh
        b = _search(model, db, 10, tables, 0.0, R.LONG_STEPS)
        c = _search(model, db, 10, tables, 1.0, R.LONG_STEPS)
    finally:
        ops.attn_rnn_set_beam_kernel(1)
    T = a["T"]
    for other in (n, b):
        assert other["T"] == T
        for k in ("out", "logp", "ln", "fin"):
            assert a[k].tobytes() == other[k].tobytes(), k
        assert a["sid"][:T].tobytes() == other["sid"][:T].tobytes() and a["pid"][:T].tobytes() == other["pid"][:T].tobytes()
    assert c["T"] != T or c["logp"].tobytes() != a["logp"].tobytes()      # ... and the model is really in the loop


def test_refusals_on_the_engine_and_one_upload_shared_with_the_prefix_search():
    from avsr_tf1_amd import ngram
    from avsr_tf1_amd.model import Seq2SeqModel
    import ref_word_ngram as RW
    case = R.ctc_case("c1_audio_uni_luong")                                # a use_ctc model: both searches run on it
    model, db = TN._model(case)
    e = R.model((1, False))
    tables = e["tables"]
    lmcfg, WL = R.RB.RL.search_case("c1_audio_uni_luong")[5:7]
    run = lambda **kw: model.beam_search_decode(db, beam_width=3, max_steps=4, **kw)
    with pytest.raises(ValueError, match="word_ngram \\(word-level tables behind a lexicon\\) cannot be combined with lm or ngram"):
        run(lm=Seq2SeqModel(lmcfg, weights=WL), word_ngram=tables, lm_weight=0.3)
    with pytest.raises(ValueError, match="word_ngram \\(word-level tables behind a lexicon\\) cannot be combined with lm or ngram"):
        run(ngram=R.RB.model(2)["tables"], word_ngram=tables, lm_weight=0.3)
    with pytest.raises(ValueError, match="lm \\(an avsr.LM network\\) or ngram \\(back-off tables\\), not both"):      # keeps its text
        run(lm=Seq2SeqModel(lmcfg, weights=WL), ngram=R.RB.model(2)["tables"], lm_weight=0.3)
    with pytest.raises(ValueError, match="compiled for"):
        run(word_ngram=R.model((1, False), 15)["tables"], lm_weight=0.3)
    ud = RW.unit_dict(31)
    ud[29], ud[30] = "GO", "EOS"                                           # the same model with GO and EOS swapped
    with pytest.raises(ValueError, match="compiled for"):
        run(word_ngram=ngram.compile_word_tables(e["model"], e["vocabulary"], ud, R.OOV), lm_weight=0.3)
    with pytest.raises(ValueError, match="space"):
        run(word_ngram=dict(tables, space_id=30), lm_weight=0.3)
    for w in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_weight"):
            run(word_ngram=tables, lm_weight=w)
    for bad in (dict(start=tables["n_nodes"]), dict(eos_w=tables["Vw"]), dict(unk_id=-2), dict(oov_score=1.0)):
        with pytest.raises(ValueError, match="avsr_beam_word_ngram_supported"):
            run(word_ngram=dict(tables, **bad), lm_weight=0.3)
    with pytest.raises(ValueError, match="beam"):
        model.greedy_decode(db, max_steps=4, word_ngram=tables)
    out = run(word_ngram=tables, lm_weight=0.3)                            # ... and the model still decodes
    up = model._ngram_tables[id(tables)][1]
    run(word_ngram=tables, lm_weight=0.3, ctc_weight=0.3)
    model.ctc_prefix_beam_search(db, beam_width=3, max_steps=6, word_ngram=tables, lm_weight=0.3)
    assert out.shape[0] == 3 and len(model._ngram_tables) == 1
    assert all(model._ngram_tables[id(tables)][1][k] is up[k] for k in TABLES)      # the ten arrays went to the device once, for both searches


def test_end_to_end_train_ngram_tool_words_then_fused_evaluate(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import ngram
    from test_gpu_avsr import _dataset
    spec = importlib.util.spec_from_file_location("train_ngram", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                              "tools", "train_ngram.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=6)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"], audio_test_record=p["audio"],
              labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4), encoder_units_per_layer=((16,), (16,)),
              decoder_units_per_layer=(16,), embedding_size=8, beam_width=4, required_grahps=('eval',), shuffle_seed=0)
    plain = avsr.AVSR(**kw)
    assert plain._word_ngram is None
    ud = plain._unit_dict
    text = str(tmp_path / "text.txt")
    open(text, "w").write("\n".join("".join(ud[s] for s in seq) for seq in ngram.label_sequences(ud, label_record=p["labels"])) + "\n")
    arpa = str(tmp_path / "words.arpa")
    assert tool.main(["--words", text, "2", arpa]) == 0
    plain.save("checkpoints/am/checkpoint.ckp-1")
    plain.evaluate("checkpoints/am/checkpoint.ckp-1", epoch=0)
    assert "word_ngram" not in plain._model._beam_ws[2] and not hasattr(plain._model, "_ngram_tables")  # nothing allocated, nothing uploaded
    out = {}
    for epoch, lmw in ((1, 0.5), (2, 0.0)):
        exp = avsr.AVSR(word_ngram_lm=arpa, word_oov_score=-4.0, lm_weight=lmw, **kw)
        assert exp._word_ngram["order"] == 2 and exp._word_ngram["oov_score"] == -4.0 and exp._word_ngram["n_trie_nodes"] > 1
        err = exp.evaluate("checkpoints/am/checkpoint.ckp-1", epoch=epoch)
        assert set(err) == {"character", "word"} and np.isfinite(err["character"])
        assert "word_ngram" in exp._model._beam_ws[2] and len(exp._model._ngram_tables) == 1
        out[epoch] = open("predictions/am/predicted_epoch_%d.mlf" % epoch).read()
    assert out[2] == open("predictions/am/predicted_epoch_0.mlf").read() and len(out[1].splitlines()) >= 6
    default = avsr.AVSR(word_ngram_lm=arpa, **kw)
    assert default._lm_weight == 0.3 and default._word_ngram["oov_score"] == -10.0

"""Back-off n-gram in beam search on the GPU (csrc/beam_ngram.hip, avsr_attn_rnn_fwd_ngram, Seq2SeqModel.beam_search_decode(ngram=...),
AVSR(ngram_lm=...)), against the references of tests/ref_beam_ngram.py.

* the step kernel alone over six chained steps of random symbols and parents: the nodes equal the host transitions exactly, the rows
  equal ngram.walk BIT FOR BIT (the kernel performs the same fp32 additions in the same order: derivable, not a tolerance) and lie within
  ref_ngram.NGRAM_PARITY of the fp64 dictionary rule; two runs are bit-identical; step 0 ignores tok and the stale half;
* the whole search by `follow` in the long setup (histories longer than the order), conditions of tests/test_gpu_beam_lm.py's _follow;
  one run per architecture in the unmodified setup, where a chunk is queued past the end; with the CTC term next to it;
* weight 0 and ngram=None: byte-identical to the plain search under all three avsr_attn_rnn_set_beam_kernel settings;
* the engine's refusals, and end to end through tools/train_ngram.py and AVSR.evaluate.
tests/test_beam_ngram_cpu.py recomputes, on the CPU, what the search cases rest on (no near-tie at the cut, the term matters, lengths)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import ref_beam_ngram as R
import ref_ngram as RN
from test_gpu_beam import TIE
from test_gpu_beam_lm import SETTINGS

pytestmark = pytest.mark.gpu
TABLES = ("bow", "backoff", "arc_begin", "sym", "logp", "next")
_sparse = {}


def _kernel_model(name):
    """(tables, fp64 NGramRef, V)"""
    from avsr_tf1_amd import ngram
    if name == "sparse":
        if not _sparse:
            m = RN.sparse_model()
            _sparse.update(tables=ngram.compile_tables(m, 12, 11, 10), ref=RN.NGramRef(m, 12))
        return _sparse["tables"], _sparse["ref"], 12
    order, V = name
    e = RN.shared_model(order, V)
    return e["tables"], e["ref"], V


def _desc(tables, V, Rn, dev, node, logp, weight=0.3):
    from avsr_tf1_amd import _lib, ops
    D = {k: torch.as_tensor(np.ascontiguousarray(tables[k])).to(dev) for k in TABLES}
    g = _lib.BeamNgram()
    g.n_nodes, g.n_arcs, g.V, g.start, g.n_rows, g.lm_weight = tables["n_nodes"], tables["n_arcs"], V, tables["start"], Rn, weight
    for k in TABLES:
        setattr(g, k, ops.fptr(D[k]))
    g.node, g.lm_logp = ops.fptr(node), ops.fptr(logp)
    return g, D


@pytest.mark.parametrize("name", [(o, V) for V in (15, 31, 41) for o in R.ORDERS] + ["sparse"])
@pytest.mark.parametrize("Rn", [1, 9, 30, 65])
def test_step_kernel_nodes_exact_rows_bit_for_bit(Rn, name):
    from avsr_tf1_amd import ops
    dev = torch.device("cuda:0")
    tables, ref, V = _kernel_model(name)
    seed = 1000 * Rn + 10 * V + (0 if name == "sparse" else name[0])
    tail = 64
    runs = []
    for stale in (5, tables["n_nodes"] + 1000):                           # what the buffers hold before step 0: ignored, out of range or not
        node = torch.full((2 * Rn + tail,), stale, dtype=torch.int32, device=dev)
        logp = torch.full((Rn * V + tail,), 77.0, device=dev)
        g, D = _desc(tables, V, Rn, dev, node, logp)
        assert ops.beam_ngram_supported(g)
        before = {k: D[k].clone() for k in TABLES}
        srng, rec = np.random.default_rng(seed), dict(nodes=[], rows=[])            # both runs see the same symbols and parents
        host = np.zeros(Rn, np.int32)
        hist = [() for _ in range(Rn)]
        for step in range(6):
            tok = srng.integers(0, V, size=Rn).astype(np.int32)           # any class: MASK, EOS and GO included
            tok[srng.integers(0, Rn)] = V - 2
            tok[srng.integers(0, Rn)] = V - 1
            par = srng.integers(0, Rn, size=Rn).astype(np.int32)          # random parents: duplicates, dropped rows, no identity
            if Rn > 1:
                par[1] = par[0]
            if step == 0:
                tok_d = torch.full((Rn,), -7 if stale == 5 else V + 50, dtype=torch.int32, device=dev)   # step 0 reads neither tok ...
            else:
                tok_d = torch.as_tensor(tok).to(dev)
            ops.beam_ngram_step(g, tok_d, torch.as_tensor(par).to(dev), Rn, step)
            torch.cuda.synchronize()
            host = R.host_step(tables, host, tok, par, step)
            hist = [()] * Rn if step == 0 else [hist[p] + (int(c),) for p, c in zip(par, tok)]
            nd, lp = node.cpu().numpy(), logp.cpu().numpy()
            assert (nd[2 * Rn:] == stale).all() and (lp[Rn * V:] == 77.0).all(), "written past the end"
            half = (step + 1) & 1
            got_n, got = nd[half * Rn:(half + 1) * Rn], lp[:Rn * V].reshape(Rn, V)
            assert np.array_equal(got_n, host), (step, got_n, host)
            want = R.host_rows(tables, host)
            assert got.tobytes() == want.tobytes(), (step, np.argwhere(got != want)[:4])
            lam64 = np.stack([ref.lam(h) for h in hist])
            dev64 = float(np.abs(got.astype(np.float64) - lam64).max())
            assert np.isfinite(got).all() and dev64 <= RN.NGRAM_PARITY, (step, dev64)
            rec["nodes"].append(got_n.copy())
            rec["rows"].append(got.copy())
        assert all(torch.equal(before[k], D[k]) for k in TABLES), "the tables are read-only"
        runs.append(rec)
    for a, b in zip(runs[0]["nodes"] + runs[0]["rows"], runs[1]["nodes"] + runs[1]["rows"]):
        assert a.tobytes() == b.tobytes()                                  # two runs, whatever the buffers held before: bit-identical


def test_step_clamps_foreign_symbols_and_parents():
    """tok / parent_rows outside their ranges are clamped to 0 (nothing outside the buffers is addressed): the rows are those of class 0
    from row 0's node."""
    from avsr_tf1_amd import ops
    dev = torch.device("cuda:0")
    tables, _ref, V = _kernel_model((4, 31))
    Rn = 9
    node, logp = torch.zeros(2 * Rn, dtype=torch.int32, device=dev), torch.zeros(Rn * V, device=dev)
    g, _D = _desc(tables, V, Rn, dev, node, logp)
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32)).to(dev)
    ops.beam_ngram_step(g, i32([0] * Rn), i32(range(Rn)), Rn, 0)
    ops.beam_ngram_step(g, i32([5] * Rn), i32(range(Rn)), Rn, 1)
    ops.beam_ngram_step(g, i32([-1, V, 1 << 20] * 3), i32([-1, Rn, 1 << 30] * 3), Rn, 2)
    torch.cuda.synchronize()
    n1 = R.host_transition(tables, tables["start"], 5)
    want = R.host_transition(tables, n1, 0)
    assert (node.cpu().numpy()[Rn:] == want).all()
    assert logp.cpu().numpy().reshape(Rn, V).tobytes() == R.host_rows(tables, [want] * Rn).tobytes()


def _search(model, db, K, tables, lmw, max_steps, check_every=3, ctc_weight=0.0):
    out = model.beam_search_decode(db, beam_width=K, max_steps=max_steps, check_every=check_every, return_all=True, ngram=tables,
                                   lm_weight=lmw, ctc_weight=ctc_weight)
    torch.cuda.synchronize()
    assert not model.check_persistent()
    X = model._beam_ws[2]
    return dict(out=out.cpu().numpy().copy(), T=out.shape[1], sid=X["sid"].cpu().numpy().copy(), pid=X["pid"].cpu().numpy().copy(),
                logp=X["logp"].cpu().numpy().copy(), ln=X["ln"].cpu().numpy().copy(), fin=X["fin"].cpu().numpy().copy())


def _model(case_tuple):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    _ocfg, mcfg, W, batch = case_tuple
    return Seq2SeqModel(mcfg, weights=W), Batch.from_numpy(batch)


def _follow(case_tuple, setting, K, lmw, order, max_steps, check_every=3, ctc_weight=0.0, past_the_end=False, what=""):
    from avsr_tf1_amd import ops
    ocfg, _mcfg, W, batch = case_tuple
    e = R.model(order)
    try:
        ops.attn_rnn_set_beam_kernel(setting)
        model, db = _model(case_tuple)
        g = _search(model, db, K, e["tables"], lmw, max_steps, check_every, ctc_weight)
    finally:
        ops.attn_rnn_set_beam_kernel(1)
    B, T = g["out"].shape[0], g["T"]
    sid, pid = g["sid"].reshape(-1, B, K)[:T], g["pid"].reshape(-1, B, K)[:T]
    ref, lp, ln, tr = R.beam_search_decode_ngram(W, ocfg, batch, e["ref"], lmw, ctc_weight=ctc_weight, beam_width=K, max_steps=max_steps,
                                                 follow=(sid, pid))
    if past_the_end:
        assert T < max_steps                                             # a chunk was queued past the end
    assert not tr["follow_short"] and tr["step_ids"].shape[0] == T, ("the searches stop at different steps", T, tr["step_ids"].shape[0])
    assert tr["follow_distinct"].all()
    worst = float(tr["follow_dev"].max())
    print(what, setting, K, lmw, order, "steps", T, "follow_dev", worst, "identical selections", float(tr["follow_same"].mean()))
    assert worst < TIE, (worst, np.argwhere(tr["follow_dev"] >= TIE)[:4])
    assert (g["out"] == ref).all()
    par = T & 1
    assert (g["ln"][par].reshape(B, K) == ln).all()
    glp = g["logp"][par].reshape(B, K)
    fin = np.isfinite(lp)
    assert (np.isfinite(glp) == fin).all() and np.abs(glp[fin] - lp[fin]).max() < 1e-4 * max(1.0, np.abs(lp[fin]).max())
    return T


@pytest.mark.parametrize("lmw", R.WEIGHTS)
@pytest.mark.parametrize("setting,K", SETTINGS)
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_full_search_follows_the_reference(case, setting, K, lmw):
    """The long setup at order 4: the histories outgrow the three symbols of context."""
    _follow(R.long_case(case), setting, K, lmw, 4, R.LONG_STEPS, what=case)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_full_search_at_orders_one_and_two(case, order):
    _follow(R.long_case(case), 1, 10, 0.3, order, R.LONG_STEPS, what=case)


@pytest.mark.parametrize("case", list(R.ARCHS))
def test_full_search_with_a_chunk_queued_past_the_end(case):
    """The unmodified setup: the search ends after a few steps (tests/test_beam_ngram_cpu.py), inside a chunk of three."""
    _follow(R.plain_case(case), 1, 10, 0.3, 4, R.MAX_STEPS, check_every=3, past_the_end=True, what=case)


@pytest.mark.parametrize("setting,K", [(1, 10), (0, 3)])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_full_search_with_the_ctc_term(case, setting, K):
    _follow(R.ctc_case(case), setting, K, 0.3, 4, R.RC.MAX_STEPS, ctc_weight=0.3, what=case)


@pytest.mark.parametrize("setting", [1, 0, 2])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_weight_zero_and_no_tables_are_the_plain_search(case, setting):
    from avsr_tf1_amd import ops
    tables = R.model(4)["tables"]
    try:
        ops.attn_rnn_set_beam_kernel(setting)
        model, db = _model(R.long_case(case))
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


def test_refusals_on_the_engine():
    from avsr_tf1_amd import ngram
    from avsr_tf1_amd.model import Seq2SeqModel
    case = R.long_case("c1_audio_uni_luong")
    model, db = _model(case)
    tables = R.model(2)["tables"]
    lmcfg, WL = R.RL.search_case("c1_audio_uni_luong")[5:7]
    with pytest.raises(ValueError, match="one language model"):
        model.beam_search_decode(db, beam_width=3, max_steps=4, lm=Seq2SeqModel(lmcfg, weights=WL), ngram=tables, lm_weight=0.3)
    with pytest.raises(ValueError, match="compiled for"):
        model.beam_search_decode(db, beam_width=3, max_steps=4, ngram=RN.shared_model(2, 15)["tables"], lm_weight=0.3)
    with pytest.raises(ValueError, match="compiled for"):                 # the same model with GO and EOS swapped
        model.beam_search_decode(db, beam_width=3, max_steps=4, ngram=ngram.compile_tables(R.model(2)["model"], 31, 29, 30), lm_weight=0.3)
    for w in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_weight"):
            model.beam_search_decode(db, beam_width=3, max_steps=4, ngram=tables, lm_weight=w)
    with pytest.raises(ValueError, match="avsr_beam_ngram_supported"):
        model.beam_search_decode(db, beam_width=3, max_steps=4, ngram=dict(tables, start=tables["n_nodes"]), lm_weight=0.3)
    with pytest.raises(ValueError, match="beam"):
        model.greedy_decode(db, max_steps=4, ngram=tables)
    out = model.beam_search_decode(db, beam_width=3, max_steps=4, ngram=tables, lm_weight=0.3)      # ... and the model still decodes
    up = model._ngram_tables[id(tables)][1]["logp"]
    model.beam_search_decode(db, beam_width=3, max_steps=4, ngram=tables, lm_weight=0.3)
    assert out.shape[0] == 3 and model._ngram_tables[id(tables)][1]["logp"] is up       # the tables went to the device once


def test_end_to_end_train_ngram_tool_then_fused_evaluate(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from test_gpu_avsr import _dataset
    spec = importlib.util.spec_from_file_location("train_ngram", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                              "tools", "train_ngram.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=6)
    arpa = str(tmp_path / "lm.arpa")
    assert tool.main([unit_file, p["labels"], "3", arpa]) == 0
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"], audio_test_record=p["audio"],
              labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4), encoder_units_per_layer=((16,), (16,)),
              decoder_units_per_layer=(16,), embedding_size=8, beam_width=4, required_grahps=('eval',), shuffle_seed=0)
    plain = avsr.AVSR(**kw)
    assert plain._ngram is None
    plain.save("checkpoints/am/checkpoint.ckp-1")
    plain.evaluate("checkpoints/am/checkpoint.ckp-1", epoch=0)
    assert "ngram" not in plain._model._beam_ws[2] and not hasattr(plain._model, "_ngram_tables")      # nothing allocated, nothing uploaded
    out = {}
    for epoch, lmw in ((1, 0.5), (2, 0.0)):
        exp = avsr.AVSR(ngram_lm=arpa, lm_weight=lmw, **kw)
        assert exp._ngram["order"] == 3
        err = exp.evaluate("checkpoints/am/checkpoint.ckp-1", epoch=epoch)
        assert set(err) == {"character", "word"} and np.isfinite(err["character"])
        out[epoch] = open("predictions/am/predicted_epoch_%d.mlf" % epoch).read()
    assert out[2] == open("predictions/am/predicted_epoch_0.mlf").read() and len(out[1].splitlines()) >= 6
    assert avsr.AVSR(ngram_lm=arpa, **kw)._lm_weight == 0.3

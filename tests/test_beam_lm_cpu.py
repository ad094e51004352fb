"""Shallow-fusion language model in beam search, the parts that need no GPU: the fp64 reference (tests/ref_beam_lm.py) against the
oracle's own search and against hand-written expectations, the argument checks of the new C entry points (decided on the host before
any launch), and the refusals of `AVSR(lm_checkpoint=...)`, which are raised before an engine is built."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ref_beam_lm as R
from oracle import avsr_oracle as O


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_weight_zero_is_the_oracles_search(case, K):
    ocfg, _m, W, batch, lcfg, _lm, WL = R.search_case(case)
    ids0, lp0, ln0, tr0 = O.beam_search_decode(W, ocfg, batch, beam_width=K, max_steps=R.MAX_STEPS, return_trace=True)
    ids, lp, ln, tr = R.beam_search_decode_lm(W, ocfg, batch, WL, lcfg, 0.0, beam_width=K, max_steps=R.MAX_STEPS)
    assert np.array_equal(ids, ids0) and np.array_equal(lp, lp0) and np.array_equal(ln, ln0)
    assert np.array_equal(tr["step_ids"], tr0["step_ids"]) and np.array_equal(tr["parent_ids"], tr0["parent_ids"])


@pytest.mark.parametrize("lm_weight", [0.3, 1.0])
@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_reference_finishes_within_max_steps_and_the_model_matters(case, K, lm_weight):
    """The seeds of the GPU test's cases: the fp64 reference itself ends before max_steps (so the engine's last chunk runs past the end),
    and the language-model term changes what is kept (else the GPU comparison would not see it)."""
    ocfg, _m, W, batch, lcfg, _lm, WL = R.search_case(case)
    ids, lp, ln, tr = R.beam_search_decode_lm(W, ocfg, batch, WL, lcfg, lm_weight, beam_width=K, max_steps=R.MAX_STEPS)
    assert tr["finished"].all() and tr["step_ids"].shape[0] < R.MAX_STEPS
    _i, lp0, _l, tr0 = R.beam_search_decode_lm(W, ocfg, batch, WL, lcfg, 0.0, beam_width=K, max_steps=R.MAX_STEPS)
    assert tr["step_ids"].shape != tr0["step_ids"].shape or not np.array_equal(tr["step_ids"], tr0["step_ids"]) or not np.allclose(lp, lp0)


@pytest.mark.parametrize("case", ["c1_audio_uni_luong", "c4_bimodal_uni"])
def test_reference_finishes_with_the_two_layer_one_hot_model(case):
    ocfg, _m, W, batch, lcfg, _lm, WL = R.search_case(case, "2x10_onehot")
    assert "dec/embedding" not in WL and WL["dec/l1/kernel"].shape == (20, 40) and WL["dec/l0/kernel"].shape == (31 + 10, 40)
    _i, _lp, _ln, tr = R.beam_search_decode_lm(W, ocfg, batch, WL, lcfg, 0.3, beam_width=3, max_steps=R.MAX_STEPS)
    assert tr["finished"].all() and tr["step_ids"].shape[0] < R.MAX_STEPS


def _state(K):
    logp = torch.full((1, K), -float("inf"), dtype=torch.float64)
    logp[0, 0] = 0.0
    return logp, torch.zeros(1, K, dtype=torch.bool), torch.zeros(1, K, dtype=torch.int64)


def test_the_language_model_decides_an_acoustic_tie():
    """Symbols a = 0, b = 1, EOS = 2; width 2.  The acoustic model gives a and b the same probability at both steps; the language model
    prefers b after GO and a after b.  Expected, written out: step 0 keeps (b, a); step 1 keeps (b a, b b) -- path probabilities
    0.27 * 0.45 * {0.7, 0.2} against 0.135 * 0.45 * 0.3 for "a a" / "a b": strictly ordered, no tie involved."""
    V, K, eos, w = 3, 2, 2, 0.6
    am = torch.log(torch.tensor([0.45, 0.45, 0.10], dtype=torch.float64)).expand(1, K, V)
    lm0 = torch.log(torch.tensor([0.3, 0.6, 0.1], dtype=torch.float64)).expand(1, K, V)
    logp, fin, ln = _state(K)
    total, scores = R.fused_candidates(logp, fin, ln, am, lm0, 1.0, w, eos)
    order = torch.argsort(scores, dim=1, descending=True, stable=True)[:, :K]
    assert (order % V).tolist() == [[1, 0]] and (order // V).tolist() == [[0, 0]]
    _t, s_am = R.fused_candidates(logp, fin, ln, am, lm0, 0.0, w, eos)                 # without the model: the tie goes to the lower index
    assert (torch.argsort(s_am, dim=1, descending=True, stable=True)[:, :K] % V).tolist() == [[0, 1]]
    logp, fin, ln = O.beam_advance(total, fin, ln, order, V, eos)
    assert np.allclose(logp.numpy(), [[np.log(0.45) + np.log(0.6), np.log(0.45) + np.log(0.3)]])
    lm1 = torch.log(torch.tensor([[[0.7, 0.2, 0.1], [0.3, 0.3, 0.4]]], dtype=torch.float64))     # after b | after a
    total, scores = R.fused_candidates(logp, fin, ln, am, lm1, 1.0, w, eos)
    order = torch.argsort(scores, dim=1, descending=True, stable=True)[:, :K]
    assert (order % V).tolist() == [[0, 1]] and (order // V).tolist() == [[0, 0]]      # "b a", then "b b"


def test_a_finished_beam_ignores_the_language_model():
    V, K, eos, w = 4, 2, 2, 0.6
    rng = np.random.default_rng(0)
    am = torch.log_softmax(torch.as_tensor(rng.standard_normal((1, K, V))), dim=-1)
    logp = torch.tensor([[-1.5, -2.0]], dtype=torch.float64)
    fin, ln = torch.tensor([[True, False]]), torch.tensor([[3, 4]])
    outs = []
    for seed in (1, 2):
        lm = torch.log_softmax(torch.as_tensor(np.random.default_rng(seed).standard_normal((1, K, V)) * 5.0), dim=-1)
        outs.append(R.fused_candidates(logp, fin, ln, am, lm, 0.7, w, eos))
    (t1, s1), (t2, s2) = outs
    assert torch.equal(t1[0, 0], t2[0, 0]) and torch.equal(s1[0, :V], s2[0, :V])      # the finished beam: identical whatever the model says
    assert float(t1[0, 0, eos]) == -1.5 and float(s1[0, eos]) == -1.5 / ((5.0 + 3.0) / 6.0) ** w
    assert not torch.equal(t1[0, 1], t2[0, 1])                                         # the unfinished one moves with it


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    p = 64                                          # any non-NULL address: the checks return before a launch could read it

    def lm(**over):
        m = _lib.BeamLm()
        m.n_layers, m.H, m.E, m.V, m.one_hot, m.n_rows, m.lm_weight = 1, 12, 8, 31, 0, 30, 0.3
        m.embedding = m.wout_t = m.bout = m.state_c = m.state_h = m.lm_logp = p
        for j in range(_lib.MAX_LM_LAYERS):
            m.wt[j] = m.bias[j] = p
        for k, v in over.items():
            setattr(m, k, v)
        return m

    ok = lm()
    assert lib.avsr_beam_lm_supported(C.byref(ok)) == 1
    assert lib.avsr_beam_lm_supported(None) == 0
    assert lib.avsr_beam_lm_supported(C.byref(lm(n_layers=5))) == 0 and lib.avsr_beam_lm_supported(C.byref(lm(H=10))) == 0
    assert lib.avsr_beam_lm_supported(C.byref(lm(lm_logp=None))) == 0 and lib.avsr_beam_lm_supported(C.byref(lm(one_hot=1))) == 0
    step = lambda m, tok=p, par=p, n=30, s=0: lib.avsr_beam_lm_step(None if m is None else C.byref(m), tok, par, n, s, None)
    assert step(None) == -1 and step(ok, tok=None) == -1 and step(ok, par=None) == -1           # AVSR_ERR_ARG
    assert step(ok, n=0) == -1 and step(ok, n=-3) == -1 and step(ok, n=29) == -1 and step(ok, s=-1) == -1
    assert step(lm(n_layers=5)) == -3 and step(lm(n_layers=0)) == -1 and step(lm(embedding=None)) == -1   # AVSR_ERR_UNSUPPORTED / ARG
    # the fused search: NULL descriptors, a non-beam mode, vocabulary / row-count mismatch
    d = _lib.AttnRnn()
    d.mode, d.V, d.B = 3, 31, 30
    fwd = lambda dd, m: lib.avsr_attn_rnn_fwd_lm(None if dd is None else C.byref(dd), None if m is None else C.byref(m), 0, 1, None)
    assert fwd(None, ok) == -1 and fwd(d, None) == -1
    assert fwd(d, lm(V=15)) == -1 and fwd(d, lm(n_rows=20)) == -1 and fwd(d, lm(n_layers=5)) == -3
    d.mode = 1
    assert fwd(d, ok) == -1
    # the selection with the term: the checks of avsr_beam_search_step
    sel = lambda logits=p, K=10, V=31: lib.avsr_beam_search_step_lm(logits, 2, K, V, 0, 29, 0.6, p, p, p, p, p, p, p, p, p, p, p, None, 0, 0, None, None,
                                                                     p, 0.3, None)
    assert sel(logits=None) == -1 and sel(K=0) == -1 and sel(K=40) == -3


def _unit_file(tmp_path, symbols="' abcdefghijklmnopqrstuvwxyz"):
    f = os.path.join(str(tmp_path), "units_%d" % len(symbols))
    open(f, "w").write("\n".join(list(symbols)) + "\n")
    return f


def _lm_checkpoint(tmp_path, unit_file, **kw):
    """A checkpoint as LM.train writes it (TF-layout weights under 'params:'), made on the host."""
    from avsr_tf1_amd import lm, params as PR
    from avsr_tf1_amd.io_utils import create_unit_dict
    cfg = lm.fusion_config(create_unit_dict(unit_file=unit_file), **kw)
    path = os.path.join(str(tmp_path), "lm.ckp-1")
    np.savez(path + ".npz", step=np.array(0, np.int64), **{"params:" + k: v for k, v in PR.initialise(cfg, seed=3).items()})
    return path


def test_avsr_refuses_what_the_fusion_does_not_cover(tmp_path):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import lm
    uf = _unit_file(tmp_path)
    ck = _lm_checkpoint(tmp_path, uf, units_per_layer=(12,), embedding_size=8)
    kw = dict(unit="character", unit_file=uf, lm_checkpoint=ck, lm_units_per_layer=(12,), lm_embedding_size=8)
    with pytest.raises(ValueError, match="beam"):
        avsr.AVSR(decoding_algorithm="greedy", **kw)
    with pytest.raises(NotImplementedError, match="LSTM"):
        avsr.AVSR(lm_cell_type="gru", **kw)
    with pytest.raises(ValueError, match="symbols"):
        avsr.AVSR(**dict(kw, unit_file=_unit_file(tmp_path, "abcdefghijklm")))
    with pytest.raises(ValueError, match="shape"):
        avsr.AVSR(**dict(kw, lm_units_per_layer=(16,)))
    with pytest.raises(ValueError, match="missing"):
        avsr.AVSR(**dict(kw, lm_units_per_layer=(12, 12)))
    W = lm.checkpoint_weights(lm.fusion_config(avsr.AVSR.__init__.__globals__["create_unit_dict"](unit_file=uf), (12,), 8), ck)
    assert W["dec/l0/kernel"].shape == (8 + 12, 48)

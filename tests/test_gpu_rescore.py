"""Attention rescoring on the GPU: the two kernels of csrc/rescore.hip through the C ABI against tests/ref_rescore.py, then
Seq2SeqModel.attention_rescoring against the oracle's evaluation-mode teacher-forced decoder run on the engine's own n-best, its missing
footprint on training state, and the AVSR front door.

Tolerances: R.TOL_SCORE for a score from given logits (8 x what the float32 restatement of the rule deviates from fp64 on the kernel
test's own inputs, measured at import).  The engine's logits are its own fp32 products and differ from the oracle's by some d (read back
from the workspace and held to the project's 1e-4); a row's log-softmax then moves by at most 2 d, the score of a hypothesis of `len` rows
by at most 2 len d: TOL_SCORE + 2 len d."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_rescore as R  # noqa: E402

pytestmark = pytest.mark.gpu
NEG = -np.inf
FILL, TAIL = 77.0, 64


# ------------------------------------------------------------------------------------------------
# 1. avsr_seq_logprob
def _logprob(z, labels, lens, stride=1, col=0):
    """One launch into column `col` of an out [B, stride] that is allocated TAIL elements too long and pre-filled: returns the column
    after checking that nothing else was written."""
    from avsr_tf1_amd import ops
    B, L, V = z.shape
    dev = "cuda"
    zd, ld, nd = torch.tensor(np.array(z), device=dev), torch.tensor(np.array(labels), device=dev), torch.tensor(np.array(lens), device=dev)
    out = torch.full((B * stride + TAIL,), FILL, device=dev)
    ops.seq_logprob(zd, ld, nd, B, L, V, out, out_stride=stride, out_offset=col)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[B * stride:] == np.float32(FILL)).all(), "written past the end of out"
    o = o[:B * stride].reshape(B, stride)
    assert (np.delete(o, col, axis=1) == np.float32(FILL)).all(), "a neighbouring column was written"
    return o[:, col].copy()


@pytest.mark.parametrize("V", R.KERNEL_V)
def test_seq_logprob_against_fp64(V):
    worst = 0.0
    for L in R.KERNEL_L:
        for B in R.KERNEL_B:
            z, labels, lens = R.kernel_case(V, L, B)
            ref = R.kernel_reference(V, L, B)
            a = _logprob(z, labels, lens)
            b = _logprob(z, labels, lens, stride=10, col=3)
            err = float(np.abs(a.astype(np.float64) - ref).max())
            worst = max(worst, err)
            print("V %d L %d B %d: err %.3g (TOL_SCORE %.3g)" % (V, L, B, err, R.TOL_SCORE))
            assert np.array_equal(a, b) and np.array_equal(a, _logprob(z, labels, lens))     # same bits: any column, any launch
            assert np.isfinite(a).all() and err <= R.TOL_SCORE, (V, L, B, err)
            assert (a[np.asarray(lens) <= 0] == 0.0).all()                                   # no labels: exactly 0
    print("V %d: worst err %.3g" % (V, worst))


def test_seq_logprob_peaked_rows_and_labels_out_of_range():
    for V in R.KERNEL_V:
        z, labels, lens = R.kernel_case(V, 7, 3, peaked=True)
        ref = R.kernel_reference(V, 7, 3, True)
        a = _logprob(z, labels, lens)
        print("peaked V %d: got %s reference %s" % (V, a, ref))
        assert np.isfinite(a).all() and np.abs(a.astype(np.float64) - ref).max() <= R.TOL_SCORE
        assert np.array_equal(a, _logprob(z, labels, lens, stride=10, col=9))
    z, labels, lens = R.kernel_case(31, 7, 3)
    bad = np.array(labels)
    bad[0, 0], bad[2, 6] = -1, 31                                                            # defined as -inf, never read
    a, good = _logprob(z, bad, lens), _logprob(z, labels, lens)
    assert a[0] == NEG and a[2] == NEG and a[1] == good[1] and not np.isnan(a).any()


# ------------------------------------------------------------------------------------------------
# 2. avsr_rescore_select
def _select(s_att, s_ctc, n, weight):
    from avsr_tf1_amd import ops
    B, K = s_att.shape
    dev = "cuda"
    order = torch.full((B * K + TAIL,), int(FILL), dtype=torch.int32, device=dev)
    final = torch.full((B * K + TAIL,), FILL, device=dev)
    ops.rescore_select(torch.tensor(s_att, device=dev), torch.tensor(s_ctc, device=dev), torch.tensor(np.asarray(n, np.int32), device=dev),
                       B, K, weight, order, final)
    torch.cuda.synchronize()
    o, f = order.cpu().numpy(), final.cpu().numpy()
    assert (o[B * K:] == int(FILL)).all() and (f[B * K:] == np.float32(FILL)).all(), "written past the end"
    return o[:B * K].reshape(B, K), f[:B * K].reshape(B, K)


@pytest.mark.parametrize("weight", [0.0, 0.5])
@pytest.mark.parametrize("K", [1, 4, 10, 64])
def test_rescore_select_equals_the_reference_exactly(K, weight):
    """Scores are multiples of 1/8 and 1/4 below 16 and the weight is 1/2: every final is exact in fp32, so the whole output is compared
    for equality.  Utterance b has n = b + 1 hypotheses (1 .. K); the drawn values repeat (64 slots, 128 values) and further ties are
    planted: equal finals from different (s_att, s_ctc) pairs."""
    rng = np.random.default_rng(K)
    B = K
    s_att = (-rng.integers(0, 128, (B, K)) / 8.0).astype(np.float32)
    s_ctc = (-rng.integers(0, 64, (B, K)) / 4.0).astype(np.float32)
    n = np.arange(1, K + 1, dtype=np.int32)
    for b in range(1, B):
        k0, k1 = 0, int(n[b]) - 1                                                           # first and last real slot tie ...
        s_att[b, k1], s_ctc[b, k1] = s_att[b, k0] - 1.0, s_ctc[b, k0] + (2.0 if weight else 0.0)
        if not weight:
            s_att[b, k1] = s_att[b, k0]
        if n[b] >= 4:                                                                       # ... and two in the middle, identically
            s_att[b, 2], s_ctc[b, 2] = s_att[b, 1], s_ctc[b, 1]
    for b in range(B):
        s_ctc[b, n[b]:] = NEG                                                               # unused slots poisoned: 0 * -inf must not be formed
        s_att[b, n[b]:] = 99.0
    order, final = _select(s_att, s_ctc, n, weight)
    ro, rf = R.select(s_att, s_ctc, n, weight)
    ties = sum(int(len(set(rf[b, :n[b]].tolist())) < n[b]) for b in range(B))
    print("K %d weight %g: %d of %d utterances hold ties" % (K, weight, ties, B))
    assert K == 1 or ties >= B - 1
    assert not np.isnan(final).any()
    assert np.array_equal(order, ro), (order, ro)
    assert np.array_equal(final, rf)
    o2, f2 = _select(s_att, s_ctc, n, weight)
    assert np.array_equal(order, o2) and np.array_equal(final, f2)


def test_rescore_select_clamps_n():
    s_att = np.array([[-1.0, -2.0, -0.5], [-1.0, -2.0, -0.5]], np.float32)
    s_ctc = np.zeros((2, 3), np.float32)
    order, final = _select(s_att, s_ctc, [-4, 9], 0.0)
    assert order.tolist() == [[-1, -1, -1], [2, 0, 1]] and final[0].tolist() == [NEG] * 3 and final[1].tolist() == [-0.5, -1.0, -2.0]


# ------------------------------------------------------------------------------------------------
# 3. the engine
ENGINE_CASES = {
    "c1_audio_uni_luong": ("c1_audio_uni_luong", {}),
    "c5_av_align": ("c5_av_align", {}),
    "bimodal": ("c4_bimodal_uni", {}),
    "gru_dec2_bahdanau": ("dec2_gru_unimodal", dict(attention_type=(("bahdanau",), ("bahdanau",)))),
}


def _engine(name, **over):
    from test_gpu_ctc import _make
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    case, kw = ENGINE_CASES[name]
    O, ocfg, mcfg, W, batch, _stream = _make(case, **dict(kw, **over))
    model = Seq2SeqModel(dataclasses.replace(mcfg, use_ctc=True), weights=W)
    return O, ocfg, W, batch, model, Batch.from_numpy(batch)


def _f32_final(s_att, s_ctc, w):
    if w == 0.0:
        return np.float32(s_att)
    return np.float32(np.float32(s_att) + np.float32(np.float32(w) * np.float32(s_ctc)))


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_engine_rescoring_against_the_oracle_on_its_own_nbest(name):
    O, ocfg, W, batch, model, bt = _engine(name)
    P, m = R.oracle_eval_model(O, W, ocfg, batch)
    B = bt.labels.shape[0]
    ref_cache = {}
    worst_d = worst_e = 0.0
    for K in (1, 4, 10):
        for max_steps in (None, 6):
            nb_ctc = model.ctc_prefix_beam_search(bt, beam_width=K, max_steps=max_steps, nbest=True)
            for w in (0.0, 0.3):
                got = model.attention_rescoring(bt, beam_width=K, max_steps=max_steps, ctc_weight=w, nbest=True)
                lr = model._last_rescore
                lg = lr["ws"]["dec"]["logits_k"].cpu().numpy()
                labels, llen, n = lr["labels"], lr["labels_len"], lr["n"]
                assert lr["Lh"] % 8 == 0 and labels.shape == (K, B, lr["Lh"]) and (llen.max() <= lr["Lh"])
                best = model.attention_rescoring(bt, beam_width=K, max_steps=max_steps, ctc_weight=w)
                assert len(got) == len(best) == B
                # reference logits of every pass, from the oracle on the engine's own label rows
                ref_att, dmax = np.zeros((K, B)), np.zeros((K, B))
                for k in range(int(n.max())):
                    key = (labels[k].tobytes(), llen[k].tobytes())
                    if key not in ref_cache:
                        rl = R.teacher_forced_logits(O, P, m, ocfg, labels[k], llen[k])
                        ref_cache[key] = (rl, R.seq_logprob(rl, labels[k], llen[k]))
                    rl, ref_att[k] = ref_cache[key]
                    for b in range(B):
                        if llen[k, b]:
                            dmax[k, b] = np.abs(lg[k, b, :llen[k, b]] - rl[b, :llen[k, b]]).max()
                assert dmax.max() <= 1e-4, dmax.max()
                worst_d = max(worst_d, float(dmax.max()))
                for b in range(B):
                    assert n[b] == len(nb_ctc[b]) == len(got[b]) >= 1
                    rank = {tuple(g): k for k, (g, _p) in enumerate(nb_ctc[b])}
                    ks = [rank[tuple(e[0])] for e in got[b]]
                    assert sorted(ks) == list(range(n[b]))                                  # every hypothesis of the n-best, once
                    tol = {}
                    for (ids, final, s_att, s_ctc), k in zip(got[b], ks):
                        assert s_ctc == nb_ctc[b][k][1] and np.isfinite(s_ctc) and np.isfinite(s_att) and not np.isnan(final)
                        assert llen[k, b] == len(ids) + 1 and list(labels[k, b, :len(ids)]) == ids and labels[k, b, len(ids)] == ocfg.eos_id
                        tol[k] = R.TOL_SCORE + 2 * llen[k, b] * dmax[k, b]
                        e = abs(s_att - ref_att[k, b])
                        worst_e = max(worst_e, e)
                        assert e <= tol[k], (K, max_steps, w, b, k, e, tol[k])
                        assert np.float32(final) == _f32_final(s_att, s_ctc, w)            # the fp32 combination of its own two scores
                    finals = [e[1] for e in got[b]]
                    assert [k for _f, k in sorted(zip([-f for f in finals], ks))] == ks    # stable sort of its own finals
                    assert best[b] == got[b][0][0] and all(isinstance(s, int) for s in best[b])
                    ref_final = {k: ref_att[k, b] + w * nb_ctc[b][k][1] for k in ks}
                    kb = max(ref_final, key=lambda k: ref_final[k])
                    # the chosen one's engine final is no smaller than the reference best's; each is within its tolerance of the reference
                    assert ref_final[ks[0]] >= ref_final[kb] - (tol[ks[0]] + tol[kb]), (K, max_steps, w, b, ref_final)
                    if max_steps is not None:
                        assert all(len(e[0]) <= max_steps for e in got[b])
    print("%s: largest logit difference %.3g, largest score error %.3g (TOL_SCORE %.3g)" % (name, worst_d, worst_e, R.TOL_SCORE))


@pytest.mark.parametrize("name", ["c1_audio_uni_luong", "c5_av_align"])
def test_rescoring_ignores_dropout_and_sampling_settings(name):
    """The pass is the evaluation graph's: teacher forcing and keep-probabilities of 1 whatever the model was built with."""
    _O, _ocfg, _W, _batch, plain, bt = _engine(name, use_dropout=False, sampling_probability=0.0)
    _O, _ocfg, _W2, _batch, noisy, _bt = _engine(name, use_dropout=True, sampling_probability=0.25)
    assert noisy.cfg.use_dropout and noisy.cfg.sampling_probability == 0.25 and not plain.cfg.use_dropout
    noisy.train_step(bt)                                                                     # leaves training settings behind (_dropping, seed)
    noisy.load_tf_weights(_W)
    for K, w in ((4, 0.0), (10, 0.3)):
        a = plain.attention_rescoring(bt, beam_width=K, ctc_weight=w, nbest=True)
        b = noisy.attention_rescoring(bt, beam_width=K, ctc_weight=w, nbest=True)
        assert a == b


def test_refusals_of_the_model_level_call():
    from avsr_tf1_amd.model import Seq2SeqModel
    from test_gpu_ctc import _make
    _O, _ocfg, mcfg, W, _batch, _stream = _make("c1_audio_uni_luong")
    from avsr_tf1_amd.model import Batch
    bt = Batch.from_numpy(_batch)
    with pytest.raises(ValueError, match="use_ctc"):
        Seq2SeqModel(mcfg, weights={k: v for k, v in W.items() if "/ctc/" not in k}).attention_rescoring(bt)
    model = Seq2SeqModel(dataclasses.replace(mcfg, use_ctc=True), weights=W)
    with pytest.raises(ValueError, match="512"):
        model.attention_rescoring(bt, max_steps=513)
    with pytest.raises(ValueError, match="64"):
        model.attention_rescoring(bt, beam_width=65)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ctc_weight"):
            model.attention_rescoring(bt, ctc_weight=bad)


# ------------------------------------------------------------------------------------------------
# 4. no footprint
def test_rescoring_leaves_no_footprint_on_training_or_the_other_decodes():
    """With dropout and scheduled sampling on, a train step depends on the step counter and the seed: had the rescoring call advanced
    either, or written the loss, the gradient buffers or the moving statistics, the two engines below would part."""
    over = dict(use_dropout=True, sampling_probability=0.3)
    _O, _ocfg, _W, _batch, a, bt = _engine("c1_audio_uni_luong", **over)
    _O, _ocfg, _W, _batch, b, _bt = _engine("c1_audio_uni_luong", **over)
    for mdl in (a, b):
        mdl.train_step(bt)                                                                   # step 1: counter, Adam slots, moving statistics move
    beam0 = a.beam_search_decode(bt, beam_width=4, max_steps=8).cpu().numpy()
    ctc0 = a.ctc_prefix_beam_search(bt, beam_width=10, nbest=True)
    state0 = (int(a.step.item()), int(a.seed.item()), float(a.loss.item()), a.grads.clone(), a.stats.clone(), a._cur)
    out = a.attention_rescoring(bt, beam_width=10, ctc_weight=0.3, nbest=True)
    assert len(out) == bt.labels.shape[0]
    assert (int(a.step.item()), int(a.seed.item()), float(a.loss.item())) == state0[:3] and a._cur is state0[5]
    assert torch.equal(a.grads, state0[3]) and torch.equal(a.stats, state0[4])
    assert np.array_equal(a.beam_search_decode(bt, beam_width=4, max_steps=8).cpu().numpy(), beam0)
    assert a.ctc_prefix_beam_search(bt, beam_width=10, nbest=True) == ctc0
    la, ga = a.train_step(bt)
    lb, gb = b.train_step(bt)
    torch.cuda.synchronize()
    assert float(la.item()) == float(lb.item()) and float(ga.item()) == float(gb.item())
    assert torch.equal(a.grads, b.grads) and torch.equal(a.params, b.params) and torch.equal(a.stats, b.stats)
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v) and int(a.step.item()) == int(b.step.item()) == 2
    pa, pb = a.export_tf_weights("params"), b.export_tf_weights("params")
    assert any("moving" in k for k in pa) and all(np.array_equal(pa[k], pb[k]) for k in pa)


# ------------------------------------------------------------------------------------------------
# 5. the front door
def test_avsr_trains_and_evaluates_with_attention_rescoring(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd.utils import _strip_extra_chars
    from test_gpu_avsr import _dataset
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=8)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"],
              audio_test_record=p["audio"], labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4),
              encoder_units_per_layer=((32,), (32, 32)), decoder_units_per_layer=(32,), embedding_size=16, warmup_steps=0,
              learning_rate=0.01, shuffle_seed=0, use_ctc=True, decoding_algorithm="attention_rescoring", beam_width=10,
              ctc_decode_weight=0.3)
    exp = avsr.AVSR(**kw)
    exp.train(logfile="logs/rescore", num_epochs=3)                        # two epochs
    losses = [float(l.split()[-1]) for l in open("logs/rescore").read().splitlines() if l.startswith("Average")]
    assert len(losses) == 2 and np.isfinite(losses).all()
    exp.save("checkpoints/rescore/checkpoint.ckp-2")

    def no_steps(*a, **k):
        raise AssertionError("the step-by-step decoders must not run under attention_rescoring")
    monkeypatch.setattr(exp._model, "beam_search_decode", no_steps)
    monkeypatch.setattr(exp._model, "greedy_decode", no_steps)
    err = exp.evaluate("checkpoints/rescore/checkpoint.ckp-2", epoch=2)
    assert set(err) == {"character", "word", "ctc_character"}
    assert all(np.isfinite(v) and v >= 0.0 for v in err.values())
    mlf = open(os.path.join("predictions", "rescore", "predicted_epoch_2.mlf")).read().splitlines()
    assert len(mlf) == 8
    lines = {l.split(" ", 1)[0]: l for l in mlf}
    seen = 0
    for bd in exp._iterator("evaluate"):                                   # the same predictions as the model-level call
        batch, names = exp._to_batch(bd)
        ids = exp._model.attention_rescoring(batch, beam_width=10, max_steps=exp._cfg.max_label_length, ctc_weight=0.3)
        for name, seq in zip(names, ids):
            hyp = "".join(_strip_extra_chars([exp._unit_dict[s] for s in seq]))
            assert lines[name.decode("utf-8")].startswith("%s %s [" % (name.decode("utf-8"), hyp)), (name, hyp)
            seen += 1
    assert seen == 8

"""The engine where softmaxes are peaked and cells saturate: train step, greedy decode and beam search on the fixtures of
tests/test_regime_cpu.py (sharpened weights: alignments near one-hot with peaks in the first and the last chunk of a chunked memory,
10 % and more of the LSTM cells at the clip, logits tens apart, softmax entries outside the focal / mc clamp) against the fp64 oracle.
Every other model-level test runs an instant after initialisation, where the running-maximum subtraction, the rescale of chunk partials,
the clip mask of the cell gradient and the clamp branch of the losses are no-ops.
"vs CPU restatement of TF-1.13.1 semantics; TF parity unpinned".

Tolerances: for each quantity max(T_suite, 8 x noise).  T_suite is what tests/test_gpu_model.py uses for it (logits / loss 1e-4 absolute,
global norm 1e-4 of max(1, norm), gradients 2e-4 of the tensor's largest entry, parameters 2e-5, alignments 1e-5); noise is the fixture's
`regime.fp32_noise` figure -- the fp32 oracle against the fp64 oracle, never anything measured from the engine; the engine sums in
other orders than torch's fp32 (MFMA chains, split-K, chunked softmax), i.e. it is another fp32 rounding of the same graph, hence the
factor.  tests/test_regime_cpu.py caps the relative noise at 1.25e-5, so for gradients the bound stays at T_suite.  Ids are bit-exact."""
import numpy as np
import pytest
import torch

import regime as R
from test_regime_cpu import FIXTURES

pytestmark = pytest.mark.gpu

PATHS = ["auto", "per_step"]                            # fused decoder + persistent encoders as the engine picks them / one launch per step


def _bound(t_suite, noise_abs):
    return max(t_suite, 8.0 * noise_abs)


def _model(fx, path, monkeypatch):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = R.build(fx)
    if path == "per_step":
        monkeypatch.setenv("AVSR_PERSISTENT_RNN", "0")
    model = Seq2SeqModel(mcfg, weights=W)
    if path == "per_step":
        assert not model.persistent_rnn and not model.fused_decode
    return model, Batch.from_numpy(batch)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("fx", FIXTURES, ids=[fx.name for fx in FIXTURES])
def test_regime_train_step(fx, path, monkeypatch):
    from avsr_tf1_amd import ops
    O, ocfg, mcfg, W, batch = R.build(fx)
    noise = R.reference(fx)
    ref = noise["ref"]
    try:
        model, db = _model(fx, path, monkeypatch)
        logits = model.forward_train(db)
        torch.cuda.synchronize()
        fed = model._cur[0]["dec"]["fed"].cpu().numpy()
        model.backward()
        model.apply_update()
        torch.cuda.synchronize()
        assert not ops.rnn_persistent_error()
    finally:
        ops.rnn_set_persistent(False)
    consumed = np.arange(batch.labels.shape[1])[None, :] < batch.labels_len[:, None]
    assert (fed[consumed] == ref["fed_tokens"][consumed]).all()                 # the sampler at peaked distributions
    lg = logits.cpu().numpy()
    assert np.isfinite(lg).all()
    err = np.abs(lg - ref["logits"]).max()
    print("logits", err, "noise", noise["logits"]["abs"])
    assert err < _bound(1e-4, noise["logits"]["abs"]), (err, noise["logits"])
    loss, gnorm = float(model.loss.item()), float(model.gnorm.item())
    assert np.isfinite(loss) and np.isfinite(gnorm)
    print("loss", abs(loss - ref["loss"]), "global norm", abs(gnorm - ref["global_norm"]), ref["global_norm"])
    assert abs(loss - ref["loss"]) < _bound(1e-4, noise["loss"]["abs"]), (loss, ref["loss"])
    assert abs(gnorm - ref["global_norm"]) < _bound(1e-4 * max(1.0, ref["global_norm"]), noise["global_norm"]["abs"]), (gnorm, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        assert np.isfinite(grads[k]).all(), k
        err = np.abs(grads[k] - g).max()
        print("grad %-32s %.2e of %.2e (%.2e rel, noise %.2e rel)" % (k, err, scale, err / scale, noise["grads"][k]["rel"]))
        assert err < _bound(2e-4 * scale + 1e-6, noise["grads"][k]["abs"]), (k, err, scale, noise["grads"][k])
    newp = model.export_tf_weights("params")
    for k, v in ref["params"].items():
        assert np.isfinite(newp[k]).all(), k
        err = np.abs(newp[k] - v).max()
        assert err < _bound(2e-5, noise["params"][k]["abs"]), (k, err)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("fx", FIXTURES, ids=[fx.name for fx in FIXTURES])
def test_regime_greedy_decode(fx, path, monkeypatch):
    from avsr_tf1_amd import ops
    O, ocfg, mcfg, W, batch = R.build(fx)
    noise = R.reference(fx)
    ids_ref, lg_ref, al_ref = noise["greedy_ref"]
    try:
        model, db = _model(fx, path, monkeypatch)
        ids = model.greedy_decode(db, max_steps=R.DECODE_STEPS).cpu().numpy()
        ws, t_out = model._last_greedy
        lg = ws["dec"]["logits"][:, :t_out].cpu().numpy()
        al = model.attention_alignments()
        torch.cuda.synchronize()
        assert not ops.rnn_persistent_error()
    finally:
        ops.rnn_set_persistent(False)
    assert ids.shape == ids_ref.shape, (ids.shape, ids_ref.shape)
    assert (ids == ids_ref).all()
    assert np.isfinite(lg).all()
    err = np.abs(lg - lg_ref).max()
    print("greedy logits", err, "noise", noise["greedy_logits"]["abs"])
    assert err < _bound(1e-4, noise["greedy_logits"]["abs"]), (err, noise["greedy_logits"])
    tol = _bound(1e-5, noise["align"]["abs"])
    assert len(al["decoder"]) == len(al_ref["decoder"])
    for a, r in zip(al["decoder"], al_ref["decoder"]):
        a = a.cpu().numpy()
        assert a.shape == r.shape and np.isfinite(a).all()
        print("alignments", np.abs(a - r).max(), "noise", noise["align"]["abs"], "largest", r.max())
        assert np.abs(a - r).max() < tol, (np.abs(a - r).max(), tol)
        live = r.sum(-1) > 0
        assert np.abs(a.sum(-1)[live] - 1.0).max() < tol
    if ocfg.architecture == "av_align":
        a = al["encoder"].cpu().numpy()
        assert a.shape == al_ref["encoder"].shape and np.isfinite(a).all()
        assert np.abs(a - al_ref["encoder"]).max() < tol, (np.abs(a - al_ref["encoder"]).max(), tol)


@pytest.mark.parametrize("K", [4, 10])
@pytest.mark.parametrize("fx", FIXTURES, ids=[fx.name for fx in FIXTURES])
def test_regime_beam_search(fx, K):
    """Under avsr_attn_rnn_set_beam_kernel 0, 1 and 2: every step's selections, the kept beams, lengths and accumulated log-probabilities
    against the oracle (tests/test_gpu_beam.py `_beam_check`: strictly up to a step at which the ORACLE saw two candidate scores within
    2e-5, and along the engine's own branch from there); settings 0 and 2 bit-identical to each other, as include/avsr_hip.h promises."""
    from avsr_tf1_amd import ops
    from test_gpu_beam import _beam_check
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = R.build(fx)
    db = Batch.from_numpy(batch)
    raw = {}
    try:
        for setting in (0, 1, 2):
            ops.attn_rnn_set_beam_kernel(setting)
            _beam_check(O, ocfg, mcfg, W, batch, K, R.DECODE_STEPS, (fx.name, K, setting))
            m = Seq2SeqModel(mcfg, weights=W)
            out = m.beam_search_decode(db, beam_width=K, max_steps=R.DECODE_STEPS, check_every=4, return_all=True)
            D, T = m._last_beam
            X = m._beam_ws[2]
            torch.cuda.synchronize()
            assert not ops.rnn_persistent_error()
            raw[setting] = (out.cpu().numpy().copy(), X["logp"].cpu().numpy().copy(), X["ln"].cpu().numpy().copy(),
                            D["logits"][:, :T].cpu().numpy().copy(), T)
            assert np.isfinite(raw[setting][3]).all() and not np.isnan(raw[setting][1]).any()
    finally:
        ops.attn_rnn_set_beam_kernel(1)
    a, b = raw[0], raw[2]
    assert a[4] == b[4] and np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert raw[1][4] == a[4] and np.array_equal(raw[1][0], a[0])                 # the MFMA path: same beams, scores to rounding (_beam_check)

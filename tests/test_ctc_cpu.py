"""CTC auxiliary loss (use_ctc), CPU side: the reference the GPU tests compare against is pinned here against a brute-force sum over
all frame labellings and against the oracle's own train step; plus the configuration refusals and the parameter inventory."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_ctc as R  # noqa: E402


# (T_b, target): C = 3 classes, blank = 2; a repeated label and an infeasible case ('a a' in 2 frames needs a blank between them)
SMALL = [(1, []), (3, []), (1, [0]), (3, [0]), (2, [0, 1]), (4, [0, 1]), (5, [1, 0]), (3, [0, 0]), (5, [1, 1]), (2, [0, 0]), (1, [0, 1])]


@pytest.mark.parametrize("Tb,target", SMALL)
def test_reference_nll_equals_brute_force_over_all_labellings(Tb, target):
    C, blank, T, L = 3, 2, 5, 3
    rng = np.random.default_rng(100 * Tb + len(target))
    z = rng.standard_normal((1, T, C))
    labels = np.zeros((1, L), np.int32)
    labels[0, :len(target)] = target
    labels_len = np.array([len(target) + 1], np.int32)            # + EOS, which the CTC target drops
    nll, U, Tbt = R.ctc_nll(torch.tensor(z), labels, labels_len, np.array([Tb]), blank)
    assert int(U[0]) == len(target) and int(Tbt[0]) == Tb
    logp = torch.log_softmax(torch.tensor(z[0, :Tb]), dim=-1).numpy()
    want = R.brute_force_nll(logp, target, blank)
    status = R.feasible(labels, labels_len, np.array([Tb]), T)
    if np.isinf(want):                                           # zero_infinity: the utterance is left out
        assert float(nll[0]) == 0.0 and status[0] == 0
    else:
        assert abs(float(nll[0]) - want) < 1e-12 * max(1.0, want) and status[0] == 1


def test_kernel_reference_zero_rows_and_infeasible_utterances():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((3, 4, 5))
    labels = np.array([[1, 1, 2, 0], [1, 1, 2, 0], [3, 0, 0, 0]], np.int32)
    ref = R.kernel_reference(z, labels, np.array([4, 4, 2]), np.array([4, 3, 2]), denom=10.0)
    assert list(ref["status"]) == [1, 0, 1]
    assert ref["nll"][1] == 0.0 and not ref["dz"][1].any()          # 'a a b' in 3 frames: no alignment
    assert ref["nll"][0] > 0 and ref["dz"][0].any()
    assert not ref["dz"][2, 2:].any() and ref["dz"][2, :2].any()    # frames past T_b
    # 'a a b' in 4 frames has exactly one path family: a - a b
    lp = torch.log_softmax(torch.tensor(z[0]), -1).numpy()
    assert abs(ref["nll"][0] + (lp[0, 1] + lp[1, 4] + lp[2, 1] + lp[3, 2])) < 1e-12


CASES = {
    "audio_uni": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32,)),
    "video_bi": dict(architecture="unimodal", encoder_type="bidirectional", video_units=(32, 32), audio_units=None,
                     attention_type=(("normed_bahdanau",), ("normed_bahdanau",))),
    "av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_reference_total_minus_term_is_the_oracle_loss(case):
    from oracle import avsr_oracle as O
    ocfg = O.OracleConfig(decoder_units=(32,), embedding_size=16, video_feat=12, audio_feat=20, **CASES[case])
    W = O.init_params(ocfg, seed=2001)
    batch = O.synthetic_batch(ocfg, B=5, T_a=21, T_v=9, L=7, ragged=True)
    stream = R.ctc_stream(ocfg)
    ref = R.ctc_reference(R.add_head(W, ocfg, stream), ocfg, batch, stream, 0.3)
    base = O.train_step(W, None, ocfg, batch)
    assert abs((ref["loss"] - 0.3 * ref["ctc"]) - base["loss"]) < 1e-12
    assert abs(ref["base_loss"] - base["loss"]) < 1e-12
    assert np.abs(ref["logits"] - base["logits"]).max() == 0.0
    kn, bn = R.head_names(stream)
    assert np.abs(ref["grads"][kn]).max() > 0 and np.abs(ref["grads"][bn]).max() > 0
    # the CTC gradient reaches the layer-0 encoder kernels: they differ from the base step's
    k0 = f"{stream}/enc/fw/l0/kernel"
    assert np.abs(ref["grads"][k0] - base["grads"][k0]).max() > 1e-6
    assert ref["ctc"] > 0 and np.isfinite(ref["loss"])


def test_validate_refusals():
    from avsr_tf1_amd.config import ModelConfig
    ModelConfig(use_ctc=True).validate()
    ModelConfig(use_ctc=True, ctc_weight=0.0).validate()
    with pytest.raises(ValueError, match="language model"):
        ModelConfig(architecture="lm", video_units=None, audio_units=None, use_ctc=True).validate()
    with pytest.raises(ValueError, match="label_smoothing"):
        ModelConfig(use_ctc=True, label_smoothing=0.1).validate()
    with pytest.raises(ValueError, match="ctc_weight"):
        ModelConfig(use_ctc=True, ctc_weight=-0.1).validate()
    with pytest.raises(NotImplementedError, match="enable_attention"):
        ModelConfig(use_ctc=True, enable_attention=False).validate()
    # off: none of the above is looked at
    ModelConfig(label_smoothing=0.1, ctc_weight=-1.0).validate()
    assert ModelConfig().use_ctc is False and ModelConfig().ctc_weight == 0.3


def test_inventory_has_the_head_only_when_use_ctc():
    from avsr_tf1_amd import params as PR
    from avsr_tf1_amd.config import ModelConfig
    V = 41
    kw = dict(vocab_size=V, go_id=40, eos_id=39)
    for cfg, stream, depth in (
            (ModelConfig(audio_units=(24, 48), video_units=None, **kw), "audio", 48),
            (ModelConfig(audio_units=(24, 48), video_units=(16,), architecture="bimodal", **kw), "audio", 48),
            (ModelConfig(audio_units=None, video_units=(16, 20), encoder_type="bidirectional", **kw), "video", 40),
            (ModelConfig(audio_units=(24, 28), video_units=(16,), architecture="av_align", **kw), "audio", 28)):
        off = PR.inventory(cfg)
        assert not [n for n in off if "/ctc/" in n]
        on = PR.inventory(dataclasses.replace(cfg, use_ctc=True))
        assert [n for n in on if "/ctc/" in n] == [f"{stream}/ctc/kernel", f"{stream}/ctc/bias"]
        assert on[f"{stream}/ctc/kernel"] == ((depth, V + 1), "plain", "glorot")
        assert on[f"{stream}/ctc/bias"] == ((V + 1,), "plain", "zeros")
        assert [n for n in on if "/ctc/" not in n] == list(off)
        assert not PR.is_l2(f"{stream}/ctc/kernel") and not PR.is_dense_l2(f"{stream}/ctc/kernel")
        # the decoder's variables stay one contiguous block behind the encoders' (decoder_grad_bucket)
        names = list(on)
        first_dec = min(i for i, n in enumerate(names) if n.startswith("dec/"))
        assert all(n.startswith("dec/") for n in names[first_dec:])
        # the engine configuration pads the memory depth, never the class axis
        eng = PR.inventory(dataclasses.replace(cfg, use_ctc=True).engine())
        assert eng[f"{stream}/ctc/kernel"][0][1] == V + 1


def test_best_path_reference():
    z = np.full((2, 5, 4), -1.0)
    for t, k in enumerate([0, 0, 3, 0, 1]):
        z[0, t, k] = 1.0
    z[1, 0, 2] = z[1, 0, 1] = 1.0               # a tie: the lowest index wins
    z[1, 1, 3] = 1.0
    z[1, 2:, 0] = 5.0                           # frames past T_b = 2
    assert R.best_path(z, [5, 2], blank=3) == [[0, 0, 1], [1]]

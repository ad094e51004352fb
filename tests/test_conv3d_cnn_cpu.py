"""CPU tests of video_processing='3dconv_cnn' (avsr/video.py:198-222): construction, layer list, parameter shapes and TF names against
the independent restatement (tests/ref_conv3d_cnn.py), the restatement's TF SAME geometry and gradients, and the documented deviation."""
import os

import numpy as np
import pytest
import torch

import ref_conv3d_cnn as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_config_constructs_with_the_3d_front_end():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd import params as PR
    cfg = ModelConfig(architecture="unimodal", video_units=(32,), audio_units=None, video_processing="3dconv_cnn", cnn_filters=(8, 16, 32, 64),
                      cnn_dense_units=16, video_feat=16)
    inv = PR.inventory(cfg)
    names = [k for k in inv if k.startswith("video/cnn/")]
    assert names and not [k for k in names if k.endswith("/bias")]          # conv3d_wrapper: use_bias=False
    W = PR.initialise(cfg, seed=3)
    k = W["video/cnn/res_block_1_conv1/kernel"]
    assert k.shape == (3, 3, 3, 8, 16)
    std = np.sqrt(2.0 / (27 * 8))                                           # variance scaling (2, fan_in) over kt*kh*kw*cin
    assert abs(k.std() / std - 1.0) < 0.15 and np.abs(k).max() <= 2 * std / 0.87962566103423978 + 1e-6


def test_avsr_constructs_with_3dconv_cnn(tmp_path):
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import io_utils as IO
    unit_file = os.path.join(str(tmp_path), "character_list")
    open(unit_file, "w").write("\n".join(list("' abcdefghijklmnopqrstuvwxyz")) + "\n")
    vrec, lrec = os.path.join(str(tmp_path), "v.tfrecord"), os.path.join(str(tmp_path), "l.tfrecord")
    with IO.TFRecordFileWriter(vrec) as fv, IO.TFRecordFileWriter(lrec) as fl:
        fv.write(IO.make_video_example("u0", np.zeros((4, 20, 20, 3), np.float32)))
        fl.write(IO.make_label_example("u0", [3, 4], "character"))
    kw = dict(unit="character", unit_file=unit_file, video_processing="3dconv_cnn", video_train_record=vrec, labels_train_record=lrec,
              encoder_units_per_layer=((16,), (16,)), decoder_units_per_layer=(16,), cnn_filters=(4, 8), cnn_dense_units=8)
    if not torch.cuda.is_available():
        # every option check passes; the engine itself then refuses to run without the GPU
        with pytest.raises(RuntimeError, match="needs an MI355X GPU"):
            avsr.AVSR(**kw)
    else:
        exp = avsr.AVSR(**kw)
        assert exp._cfg.video_processing == "3dconv_cnn" and exp._cfg.video_hw == (20, 20, 3)
        assert exp._model.export_tf_weights()["video/cnn/res_block_1_conv1/kernel"].shape == (3, 3, 3, 4, 8)


@pytest.mark.parametrize("hw,filters,msg", [((20, 20, 6), (4, 8), "channels"), ((20, 20, 3), (4, 256), "128"), ((20, 20, 3), (4, 6), "multiples of 4")])
def test_config_refuses_what_the_3d_kernels_do_not_cover(hw, filters, msg):
    from avsr_tf1_amd.config import ModelConfig
    cfg = ModelConfig(architecture="unimodal", video_units=(16,), audio_units=None, video_processing="3dconv_cnn", cnn_filters=filters,
                      cnn_dense_units=8, video_feat=8, video_hw=hw)
    with pytest.raises(ValueError, match=msg):
        cfg.validate()


def test_tf_variable_names_cover_exactly_the_3d_front_end():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd import params as PR
    cfg = ModelConfig(architecture="unimodal", video_units=(16,), audio_units=None, video_processing="3dconv_cnn", cnn_filters=(4, 8),
                      cnn_dense_units=8, video_feat=8, video_hw=(20, 20, 3))
    ren = PR.tf_variable_names(cfg)
    assert set(ren) == {k for k in PR.inventory(cfg) if k.startswith("video/cnn/")}
    assert ren["video/cnn/flatten/kernel"] == "video/cnn/conv3d_6/kernel" and len(set(ren.values())) == len(ren)
    assert PR.tf_variable_names(ModelConfig(video_units=(16,), video_processing="resnet_cnn")) == {}


@pytest.mark.parametrize("hw,filters,dense", [((36, 36, 3), (8, 16, 32, 64), 128), ((35, 29, 1), (4, 12, 20), 8), ((20, 20, 3), (4, 8), 8)])
def test_layer_list_parameter_shapes_and_tf_names(hw, filters, dense):
    from avsr_tf1_amd import cnn3d
    ops_, shapes = cnn3d.layout(hw, filters, dense)
    eng = cnn3d.param_shapes(hw, filters, dense)
    ref = R.param_shapes(hw, filters, dense)
    assert [(n, tuple(s)) for n, s, _r in eng] == ref                       # same names, shapes and graph order
    assert cnn3d.tf_names(hw, filters, dense) == R.tf_names(hw, filters, dense)
    names = cnn3d.tf_names(hw, filters, dense)
    nconv = 3 + 3 * (len(filters) - 1) + 1
    assert names["layer0/kernel"] == "conv3d/kernel" and names["flatten/kernel"] == "conv3d_%d/kernel" % (nconv - 1)
    assert names["layer0_bn/gamma"] == "batch_normalization/gamma"
    if len(filters) > 1:                                                    # a block's leading BN and shortcut come first
        assert names["res_block_1_first_bn/beta"] == "batch_normalization_2/beta"
        assert names["res_block_1_shortcut/kernel"] == "conv3d_3/kernel" and names["res_block_1_conv1/kernel"] == "conv3d_4/kernel"
    H, W = hw[0], hw[1]
    for _ in filters[1:]:
        H, W = -(-H // 2), -(-W // 2)
    assert shapes["out"] == (1, 1, dense) and ops_[-1][4:6] == (H, W)


@pytest.mark.parametrize("n,k,s", [(36, 3, 1), (36, 3, 2), (18, 3, 2), (9, 3, 2), (35, 3, 2), (29, 3, 2), (5, 3, 2), (9, 1, 2), (35, 1, 2),
                                   (75, 3, 1), (1, 3, 1), (2, 3, 1)])
def test_restatement_same_padding_is_the_tf_rule(n, k, s):
    out, a, b = R.same_pad(n, k, s)
    assert out == -(-n // s)
    assert a + b == max((out - 1) * s + k - n, 0) and b - a in (0, 1)       # the odd pixel goes after
    # every output's window starts at o*s - a and stays within the padded axis
    assert (out - 1) * s - a + k <= n + b
    # the restatement's conv on a ones map equals the count of in-range taps (zeros outside), axis by axis
    x = torch.ones(1, n if k == 3 and s == 1 else 1, n, 1, 1, dtype=torch.float64)
    w = torch.ones(1, k, 1, 1, 1, dtype=torch.float64)
    y = R.conv3d_same(x, w, s)[0, 0, :, 0, 0]
    want = [sum(1 for j in range(k) if 0 <= o * s - a + j < n) for o in range(out)]
    assert y.tolist() == want


def test_restatement_gradients_pass_a_finite_difference_check():
    torch.manual_seed(0)
    hw, filters, dense = (5, 4, 2), (4, 4), 4
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in R.init_params(hw, filters, dense).items()}
    x = torch.rand(2, 3, 5, 4, 2, dtype=torch.float64)
    x[1, 2] = 0.0                                                           # a padding frame

    def f(inp, *kern):
        Q = dict(P)
        for (k, _), v in zip(kk, kern):
            Q[k] = v
        return (R.forward(Q, hw, filters, dense, inp, True, None) ** 2).sum()

    kk = [(k, v) for k, v in P.items() if k.endswith(("/kernel", "/gamma", "/beta"))]
    assert torch.autograd.gradcheck(f, (x.requires_grad_(),) + tuple(v.detach().clone().requires_grad_() for _, v in kk), eps=1e-6, atol=1e-5)


def test_restatement_moving_statistics_take_the_biased_variance():
    hw, filters, dense = (6, 6, 1), (4,), 4
    P = {k: torch.tensor(v, dtype=torch.float64) for k, v in R.init_params(hw, filters, dense).items()}
    x = torch.rand(2, 3, 6, 6, 1, dtype=torch.float64)
    upd = {}
    R.forward(P, hw, filters, dense, x, True, upd)
    a0 = R.conv3d_same(x * 2 - 1, P["video/cnn/layer0/kernel"], 1).reshape(-1, 4)
    want = 0.98 * 1.0 + 0.02 * a0.var(dim=0, unbiased=False)
    assert torch.allclose(upd["video/cnn/layer0_bn/moving_variance"], want)


def test_the_final_stride_deviation_is_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "3dconv_cnn" in doc and "(1, 1, 1)" in doc and "strides=(1, 1)" in doc

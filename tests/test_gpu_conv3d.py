"""video_processing='3dconv_cnn' on the GPU: the conv3d kernels (csrc/conv3d.hip) against CPU torch.nn.functional.conv3d in fp64, the
whole front-end (cnn3d.py) against the restatement of tests/ref_conv3d_cnn.py, and full-model train / greedy / beam-search parity against
the oracle with its lip-CNN front-end routed through that restatement."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import ref_conv3d_cnn as R

pytestmark = pytest.mark.gpu


def _close(a, b, tol=2e-5):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


def _pads(T, H, W, k, s):
    Ho, pt, _ = R.same_pad(H, k[1], s)
    Wo, pl, _ = R.same_pad(W, k[2], s)
    return Ho, Wo, (R.same_pad(T, k[0], 1)[1], pt, pl)


# (B, T, H, W, Ci, Co, k, s): every geometry of the default front-end (36x36x3, filters 8-16-32-64) and odd ones (35x29, filters 4-12-20,
# T in {1, 2, 3, 75}: both temporal borders and T < kt)
GEOS = [(2, 3, 36, 36, 3, 8, (1, 3, 3), 1), (2, 3, 36, 36, 8, 8, (3, 3, 3), 1), (2, 3, 36, 36, 8, 16, (1, 1, 1), 2),
        (2, 3, 36, 36, 8, 16, (3, 3, 3), 2), (2, 3, 18, 18, 16, 16, (3, 3, 3), 1), (2, 3, 18, 18, 16, 32, (3, 3, 3), 2),
        (2, 3, 18, 18, 16, 32, (1, 1, 1), 2), (2, 3, 9, 9, 32, 64, (3, 3, 3), 2), (2, 3, 5, 5, 64, 64, (3, 3, 3), 1),
        (2, 2, 35, 29, 1, 4, (1, 3, 3), 1), (1, 1, 35, 29, 4, 12, (3, 3, 3), 2), (3, 2, 18, 15, 12, 20, (3, 3, 3), 2),
        (1, 75, 9, 8, 20, 20, (3, 3, 3), 1), (2, 1, 9, 9, 20, 20, (3, 3, 3), 1), (2, 2, 9, 8, 12, 20, (1, 1, 1), 2),
        # more than 512 tiles of 128 destination positions: every forward / data-gradient workgroup walks many tiles (statistics carried
        # from tile to tile), and the weight gradient runs its full 512-way split of the positions
        (2, 75, 36, 36, 8, 8, (3, 3, 3), 1), (2, 75, 36, 36, 8, 16, (3, 3, 3), 2), (4, 75, 18, 18, 16, 32, (3, 3, 3), 2),
        (2, 75, 9, 9, 64, 64, (3, 3, 3), 1)]


@pytest.mark.parametrize("geo", GEOS, ids=["B%dT%d_%dx%d_%d-%d_k%d%d%d_s%d" % (g[:6] + g[6] + (g[7],)) for g in GEOS])
@pytest.mark.parametrize("variant", ["plain", "bn", "affine", "res", "bnres"])
def test_conv3d_forward_data_and_weight_gradients(geo, variant):
    from avsr_tf1_amd import ops
    B, T, H, W, Ci, Co, k, s = geo
    Ho, Wo, pads = _pads(T, H, W, k, s)
    g = torch.Generator().manual_seed(GEOS.index(geo) * 7 + len(variant))
    x = torch.randn(B, T, H, W, Ci, generator=g, dtype=torch.float64)
    w = torch.randn(k + (Ci, Co), generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(B, T, Ho, Wo, Co, generator=g, dtype=torch.float64)
    sc = torch.rand(Ci, generator=g, dtype=torch.float64) + 0.5
    sh = torch.randn(Ci, generator=g, dtype=torch.float64) * 0.3
    rs = torch.rand(Co, generator=g, dtype=torch.float64) + 0.5
    rh = torch.randn(Co, generator=g, dtype=torch.float64) * 0.3
    res = torch.randn(B, T, Ho, Wo, Co, generator=g, dtype=torch.float64)
    tf = {"bn": 1, "bnres": 1, "affine": 0}.get(variant)
    xr = x.clone().requires_grad_()
    wr = w.clone().requires_grad_()
    src = xr if tf is None else (xr * sc + sh if tf == 0 else torch.relu(xr * sc + sh))
    y = R.conv3d_same(src, wr, s)
    if variant == "res":
        y = y + res
    elif variant == "bnres":
        y = y + torch.relu(res * rs + rh)
    y_conv = R.conv3d_same(xr, wr, s)
    dx_ref, = torch.autograd.grad(y_conv, xr, dy)                           # data gradient: of the raw conv (no loader transform)
    dw_ref, = torch.autograd.grad(y, wr, dy)
    cu = lambda t: t.to(torch.float32).cuda().contiguous()
    X, Wt, DY = cu(x), cu(w), cu(dy)
    tfv = (cu(sc), cu(sh)) if tf is not None else None
    d = ops.conv3d_desc(B, T, H, W, Ci, Co, k, s, pads, Ho, Wo, tf=tfv, relu=1 if tf is None else tf)
    assert ops.conv3d_supported(d)
    Y = torch.full((B, T, Ho, Wo, Co), float("nan"), device="cuda")
    stats = torch.zeros(512 * 2 * Co, device="cuda")
    resg = cu(res) if variant in ("res", "bnres") else None
    res_tf = (cu(rs), cu(rh)) if variant == "bnres" else None
    n = ops.conv3d_fwd(d, X, Wt, Y, res=resg, res_tf=res_tf, stats=stats)
    d0 = ops.conv3d_desc(B, T, H, W, Ci, Co, k, s, pads, Ho, Wo)
    DX = torch.full_like(X, 0.25)
    beta = 0.5 if variant == "res" else 0.0
    ops.conv3d_bwd_data(d0, DY, Wt, DX, beta=beta)
    DW = torch.full_like(Wt, 0.125)
    scratch = torch.empty(ops.conv3d_wgrad_scratch_floats(d), device="cuda")
    ops.conv3d_bwd_weight(d, X, DY, DW, scratch, beta=1.0)
    torch.cuda.synchronize()
    yr = y.detach().numpy()
    assert _close(Y.cpu().numpy(), yr), np.abs(Y.cpu().numpy() - yr).max()
    st = stats[:n * 2 * Co].view(n, 2, Co).double().sum(0).cpu().numpy()
    yf = yr.reshape(-1, Co)
    assert _close(st[0], yf.sum(0), 1e-5) and _close(st[1], (yf ** 2).sum(0), 1e-5)
    assert _close(DX.cpu().numpy(), dx_ref.numpy() + beta * 0.25), np.abs(DX.cpu().numpy() - dx_ref.numpy() - beta * 0.25).max()
    assert _close(DW.cpu().numpy(), dw_ref.numpy() + 0.125), np.abs(DW.cpu().numpy() - dw_ref.numpy() - 0.125).max()


def test_conv3d_bn_finalize_takes_the_biased_variance():
    from avsr_tf1_amd import ops
    C, rows = 12, 1000
    y = torch.randn(rows, C, device="cuda") * 2 + 1
    part = torch.cat([y.sum(0), (y * y).sum(0)]).view(1, 2 * C).contiguous()
    mean, invstd, mm, mv = (torch.zeros(C, device="cuda") for _ in range(4))
    mv += 1
    gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    scale, shift = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    ops.conv3d_bn_finalize(part, 1, C, rows, 1e-5, 0.98, mean, invstd, mm, mv, gamma, beta, scale, shift)
    yd = y.double()
    var = yd.var(0, unbiased=False)
    assert torch.allclose(mv.double(), 0.98 + 0.02 * var, atol=1e-5)
    assert torch.allclose(mm.double(), 0.02 * yd.mean(0), atol=1e-6)
    assert torch.allclose(invstd.double(), torch.rsqrt(var + 1e-5), rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------------------------------
# the front-end alone

def engine_masks(cnn, B, T):
    """{layer name: float64 0/1 tensor} of the ReLU masks the engine's front-end took in its last training forward (read from its
    pre-normalisation maps and the batch norms' scale / shift, as its backward does); call before backward (it reuses pre_act)."""
    out = {}
    for op in cnn.ops:
        if op[0] == "bnrelu":
            name, src = op[1], op[2]
            _mean, _inv, sc, sh = cnn.bn[name]
            z = torch.addcmul(sh.view(1, 1, 1, -1), cnn.maps[src], sc.view(1, 1, 1, -1))     # fp32, as the engine evaluates it
            out[name] = (z > 0).double().cpu().reshape((B, T) + tuple(z.shape[1:]))
        elif op[0] == "flatten":
            out["flatten"] = (cnn.pre_act > 0).double().cpu().reshape(B, T, -1)
    return out


def _small_model(filters, dense, hw=(36, 36, 3), batch_normalisation=True):
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    cfg = ModelConfig(architecture="unimodal", encoder_type="unidirectional", video_units=(16,), audio_units=None, decoder_units=(16,),
                      embedding_size=8, video_processing="3dconv_cnn", cnn_filters=filters, cnn_dense_units=dense, video_feat=dense,
                      video_hw=hw, batch_normalisation=batch_normalisation)
    return Seq2SeqModel(cfg, seed=3)


@pytest.mark.parametrize("filters,dense,hw,B,T", [((8, 16, 32, 64), 16, (36, 36, 3), 3, 4), ((4, 12, 20), 8, (35, 29, 1), 2, 3),
                                                  ((8, 8), 8, (20, 20, 3), 2, 1), ((8, 16, 32, 64), 16, (36, 36, 3), 6, 75)])
@pytest.mark.parametrize("training", [True, False])
def test_front_end_features_gradients_and_moving_statistics(filters, dense, hw, B, T, training):
    from avsr_tf1_amd.cnn3d import LipCNN3D
    model = _small_model(filters, dense, hw)
    rng = np.random.default_rng(11)
    W = model.export_tf_weights("params")
    for k in W:                                                             # non-trivial batch-norm parameters and moving statistics
        if k.startswith("video/cnn/") and not k.endswith("/kernel"):
            base = {"gamma": 1.0, "beta": 0.0, "moving_mean": 0.0, "moving_variance": 1.0}[k.rsplit("/", 1)[1]]
            W[k] = (base + rng.standard_normal(W[k].shape) * (0.1 if "variance" not in k else 0.05) + (0.2 if "variance" in k else 0)).astype(np.float32)
    model.load_tf_weights(W)
    lens = np.array([T] + [max(1, T - 1 - i) for i in range(B - 1)])
    x = rng.random((B, T) + hw).astype(np.float32)
    x *= (np.arange(T)[None, :] < lens[:, None]).reshape(B, T, 1, 1, 1)       # padding frames are zeros, as the batcher writes them
    cnn = LipCNN3D(model, B, T)
    X = torch.from_numpy(x).cuda().view(B * T, *hw).contiguous()
    model.grads.zero_()
    out = cnn.forward(X, training).view(B, T, -1)
    dfeat = rng.standard_normal((B, T, dense)).astype(np.float32)
    masks = engine_masks(cnn, B, T) if training else None
    if training:
        cnn.backward(torch.from_numpy(dfeat).cuda().view(B * T, dense).contiguous())
    torch.cuda.synchronize()
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in W.items() if k.startswith("video/cnn/")}
    upd = {}
    # (training: the restatement takes the engine's ReLU masks, so that an input within fp32 rounding of zero -- thousands of them
    # among the 10^8 ReLU inputs of the 75-frame case -- cannot flip an element's whole gradient contribution)
    ref = R.forward(P, hw, filters, dense, torch.tensor(x, dtype=torch.float64), training, upd, masks)
    assert _close(out.cpu().numpy(), ref.detach().numpy(), 1e-5), np.abs(out.cpu().numpy() - ref.detach().numpy()).max()
    if not training:
        return
    keys = [k for k in P if not k.endswith(("moving_mean", "moving_variance"))]
    gref = torch.autograd.grad((ref * torch.tensor(dfeat, dtype=torch.float64)).sum(), [P[k] for k in keys])
    G = model.export_tf_weights("grads")
    for k, gr in zip(keys, gref):
        g = gr.numpy()
        err = np.abs(G[k] - g).max()
        assert err <= 1e-4 * max(1.0, np.abs(g).max()), (k, err)
    newp = model.export_tf_weights("params")
    for k, v in upd.items():
        assert np.abs(newp[k] - v.detach().numpy()).max() < 1e-5, k


# ------------------------------------------------------------------------------------------------------------------------------------
# the full model against the oracle, its lip-CNN front-end routed through the restatement

def _make3d(monkeypatch, case, **over):
    from test_gpu_model import make
    O, ocfg, mcfg, W, batch = make(case, **over)
    mcfg = dataclasses.replace(mcfg, video_processing="3dconv_cnn")
    W = R.swap_params(W, ocfg.video_hw, ocfg.cnn_filters, ocfg.cnn_dense_units)
    rng = np.random.default_rng(7)
    for k in W:
        if k.startswith("video/cnn/") and k.endswith("beta"):
            W[k] = (rng.standard_normal(W[k].shape) * 0.1).astype(np.float32)
        if k.startswith("video/cnn/") and k.endswith("gamma"):
            W[k] = (1.0 + rng.standard_normal(W[k].shape) * 0.1).astype(np.float32)
    R.patch_oracle(monkeypatch, ocfg, batch.video.shape[1])
    return O, ocfg, mcfg, W, batch


CASES3D = ["c3_video_cnn_bi", "c4_bimodal_cnn"]


@pytest.mark.parametrize("case", CASES3D)
def test_train_step_parity(case, monkeypatch):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = _make3d(monkeypatch, case)
    assert (batch.video_len < batch.video.shape[1]).any()                   # padded frames take part
    O.RELU_MARGIN[0] = float("inf")
    ref = O.train_step(W, None, ocfg, batch)
    model = Seq2SeqModel(mcfg, weights=W)
    logits = model.forward_train(Batch.from_numpy(batch))
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    assert np.isfinite(lg).all() and np.abs(lg - ref["logits"]).max() < 1e-4, np.abs(lg - ref["logits"]).max()
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4, (float(model.loss.item()), ref["loss"])
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    tol = 2e-3 if O.RELU_MARGIN[0] < 1e-5 else 2e-4
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        err = np.abs(grads[k] - g).max()
        assert err < tol * scale + 1e-6, (k, err, scale)
    newp = model.export_tf_weights("params")
    for k, v in ref["params"].items():
        assert np.abs(newp[k] - v).max() < 2e-5, (k, np.abs(newp[k] - v).max())


@pytest.mark.parametrize("case", CASES3D)
def test_greedy_decode_parity(case, monkeypatch):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = _make3d(monkeypatch, case)
    ids_ref, lg_ref = O.greedy_decode(W, ocfg, batch, max_steps=12, return_logits=True)
    model = Seq2SeqModel(mcfg, weights=W)
    ids = model.greedy_decode(Batch.from_numpy(batch), max_steps=12).cpu().numpy()
    assert ids.shape == ids_ref.shape and (ids == ids_ref).all()
    ws, t_out = model._last_greedy
    assert np.abs(ws["dec"]["logits"][:, :t_out].cpu().numpy() - lg_ref).max() < 1e-4


@pytest.mark.parametrize("case", CASES3D)
def test_beam_search_parity_width_10(case, monkeypatch):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = _make3d(monkeypatch, case)
    r = O.train_step(W, None, ocfg, batch)                                  # moving statistics and weights off their initial values
    W2 = {k: v.copy() for k, v in r["params"].items()}
    W2["dec/out/bias"][ocfg.eos_id] += 1.2
    ref = O.beam_search_decode(W2, ocfg, batch, beam_width=10, max_steps=14, return_all=True)[0]
    model = Seq2SeqModel(mcfg, weights=W2)
    out = model.beam_search_decode(Batch.from_numpy(batch), beam_width=10, max_steps=14, check_every=3, return_all=True).cpu().numpy()
    assert out.shape == ref.shape and (out == ref).all()


def test_graph_replay_equals_eager_steps(monkeypatch):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    O, ocfg, mcfg, W, batch = _make3d(monkeypatch, "c4_bimodal_cnn", B=6, Tv=7)
    mcfg = dataclasses.replace(mcfg, use_dropout=True, sampling_probability=0.2)
    db = Batch.from_numpy(batch)
    out = {}
    for mode in ("eager", "graph"):
        m = Seq2SeqModel(mcfg, weights=W)
        t = DataParallelTrainer(m, None, use_graph=(mode == "graph"))
        for _ in range(4):
            t.train_step(db)
        torch.cuda.synchronize()
        assert mode == "eager" or t.mode == "hipgraph"
        out[mode] = (float(m.loss.item()), float(m.gnorm.item()), m.export_tf_weights("params"))
        del t, m
    assert out["eager"][:2] == out["graph"][:2]
    for k, v in out["eager"][2].items():
        assert (v == out["graph"][2][k]).all(), k


def test_avsr_train_resume_and_evaluate_from_lip_crops(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import io_utils as IO
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(1)
    unit_file = os.path.join(str(tmp_path), "character_list")
    open(unit_file, "w").write("\n".join(list("' abcdefghijklmnopqrstuvwxyz")) + "\n")
    vrec, lrec = os.path.join(str(tmp_path), "video.tfrecord"), os.path.join(str(tmp_path), "labels.tfrecord")
    with IO.TFRecordFileWriter(vrec) as fv, IO.TFRecordFileWriter(lrec) as fl:
        for i in range(8):
            L = int(rng.integers(2, 5))
            lab = rng.integers(3, 10, size=L)
            T = 3 * L + int(rng.integers(0, 3))
            frames = rng.random((T, 20, 20, 3)).astype(np.float32) * 0.1
            for j, c in enumerate(lab):
                frames[3 * j:3 * j + 3, int(c) * 2:int(c) * 2 + 2, :, :] += 0.8
            fv.write(IO.make_video_example("utt%02d" % i, frames))
            fl.write(IO.make_label_example("utt%02d" % i, lab.tolist(), "character"))
    kw = dict(unit="character", unit_file=unit_file, video_processing="3dconv_cnn", video_train_record=vrec, video_test_record=vrec,
              labels_train_record=lrec, labels_test_record=lrec, batch_size=(4, 4), encoder_units_per_layer=((32,), (32,)),
              decoder_units_per_layer=(32,), embedding_size=16, decoding_algorithm="greedy", cnn_filters=(8, 16), cnn_dense_units=32,
              warmup_steps=0, learning_rate=0.01, shuffle_seed=0, architecture="unimodal")
    exp = avsr.AVSR(**kw)
    exp.train(logfile="logs/v3d", num_epochs=11)                 # 10 epochs -> checkpoint + evaluation at epoch 10
    assert os.path.exists("checkpoints/v3d/checkpoint.ckp-10.npz") and os.path.exists("predictions/v3d/predicted_epoch_10.mlf")
    losses = [float(l.split()[-1]) for l in open("logs/v3d").read().splitlines() if l.startswith("Average")]
    assert len(losses) == 10 and np.isfinite(losses).all() and losses[-1] < losses[0]
    w = np.load("checkpoints/v3d/checkpoint.ckp-10.npz")
    assert w["params:video/cnn/flatten/kernel"].shape == (1, 10, 10, 16, 32)
    assert w["params:video/cnn/res_block_1_conv1/kernel"].shape == (3, 3, 3, 8, 16)
    err = exp.evaluate("checkpoints/v3d/checkpoint.ckp-10", epoch=10)     # greedy decoding with the moving statistics
    assert set(err) == {"character", "word"} and np.isfinite(err["character"])
    exp2 = avsr.AVSR(**kw)
    exp2.train(logfile="logs/v3d", num_epochs=2, try_restore_latest_checkpoint=True)
    assert "Average batch_loss as epoch 11" in open("logs/v3d").read()
    assert int(exp2._model.step.item()) > 20
    a, b = exp._model.export_tf_weights("params"), exp2._model.export_tf_weights("params")
    assert not np.array_equal(a["video/cnn/layer0/kernel"], b["video/cnn/layer0/kernel"])   # resumed training moved the front-end


def test_full_size_train_step_and_greedy(monkeypatch):
    """The headline shape (B=64, T_v=75 x 36x36x3, T_a=500, L=40, widths 256) with the 3-D front-end: every launch of the conv3d kernels
    walks many tiles per workgroup and the weight gradients their widest split."""
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    over = dict(video_units=(256,), audio_units=(256, 256, 256), decoder_units=(256,), embedding_size=128, audio_feat=80, video_feat=128,
                use_dropout=True, sampling_probability=0.1, video_processing="resnet_cnn", cnn_filters=(8, 16, 32, 64), cnn_dense_units=128)
    O, ocfg, mcfg, W, batch = _make3d(monkeypatch, "c4_bimodal_cnn", B=64, Ta=500, Tv=75, L=40, ragged=True, **over)
    model = Seq2SeqModel(mcfg, weights=W)
    logits = model.forward_train(Batch.from_numpy(batch))
    torch.cuda.synchronize()
    # the oracle's front-end takes the engine's ReLU masks (see test_front_end_features_gradients_and_moving_statistics)
    R.patch_oracle(monkeypatch, ocfg, batch.video.shape[1], engine_masks(model._cur[0]["enc"]["video"]["cnn"], 64, batch.video.shape[1]))
    ref = O.train_step(W, None, ocfg, batch)
    consumed = np.arange(batch.labels.shape[1])[None, :] < batch.labels_len[:, None]
    assert (model._cur[0]["dec"]["fed"].cpu().numpy()[consumed] == ref["fed_tokens"][consumed]).all()
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    assert np.isfinite(lg).all() and np.abs(lg - ref["logits"]).max() < 1e-4, np.abs(lg - ref["logits"]).max()
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4, (float(model.loss.item()), ref["loss"])
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        # (as test_gpu_model's full-size case: a convolution kernel's gradient is an fp32 sum of millions of largely cancelling products)
        rel = 2e-3 if "/cnn/" in k else 5e-4
        err = np.abs(grads[k] - g).max()
        assert err < rel * scale + 1e-6, (k, err, scale)
    newp = model.export_tf_weights("params")
    for k, v in ref["params"].items():
        assert np.abs(newp[k] - v).max() < 2e-5, (k, np.abs(newp[k] - v).max())
    R.patch_oracle(monkeypatch, ocfg, batch.video.shape[1])
    ids_ref = O.greedy_decode(W, ocfg, batch, max_steps=8)
    ids = Seq2SeqModel(mcfg, weights=W).greedy_decode(Batch.from_numpy(batch), max_steps=8).cpu().numpy()
    assert ids.shape == ids_ref.shape and (ids == ids_ref).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# data parallelism: two engine ranks over gloo on one GPU, per-rank batch norms (sync_cnn_bn is refused for this front-end)
CASE_DP = dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32), decoder_units=(32,),
               embedding_size=16, audio_feat=20, regress_aus=True, use_dropout=False, warmup_steps=0, video_processing="resnet_cnn",
               cnn_filters=(8, 16, 32, 64), cnn_dense_units=16, video_feat=16)


def _setup_dp(duplicate):
    from avsr_tf1_amd.config import ModelConfig
    from oracle import avsr_oracle as O
    ocfg = O.OracleConfig(**CASE_DP)
    mcfg = ModelConfig(**{f.name: getattr(ocfg, f.name) for f in dataclasses.fields(ModelConfig) if hasattr(ocfg, f.name)})
    mcfg = dataclasses.replace(mcfg, video_processing="3dconv_cnn")
    W = R.swap_params(O.init_params(ocfg, seed=7), ocfg.video_hw, ocfg.cnn_filters, ocfg.cnn_dense_units)
    if duplicate:
        half = O.synthetic_batch(ocfg, B=2, T_a=15, T_v=5, L=5, ragged=True)
        full = O.Batch(**{k: np.concatenate([getattr(half, k)] * 2) for k in ("audio", "audio_len", "video", "video_len", "aus", "labels", "labels_len")})
    else:
        full = O.synthetic_batch(ocfg, B=4, T_a=15, T_v=5, L=5, ragged=True)
    return O, mcfg, W, full


def _worker_dp(rank, world, port, out_dir, duplicate):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["AVSR_PERSISTENT_RNN"] = "0"
    import torch.distributed as dist
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    O, mcfg, W, full = _setup_dp(duplicate)
    model = Seq2SeqModel(mcfg, weights=W)
    trainer = DataParallelTrainer(model, dist, use_graph=True)
    sl = slice(2 * rank, 2 * rank + 2)
    batch = Batch.from_numpy(O.Batch(**{k: (None if getattr(full, k) is None else np.ascontiguousarray(getattr(full, k)[sl]))
                                        for k in ("audio", "audio_len", "video", "video_len", "aus", "labels", "labels_len")}))
    for _ in range(3):
        trainer.train_step(batch)
    torch.cuda.synchronize()
    try:
        DataParallelTrainer(model, dist, use_graph=False, sync_cnn_bn=True)
        refused = False
    except NotImplementedError:
        refused = True
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), mode=np.array(trainer.mode), refused=np.array(refused),
             **model.export_tf_weights("params"))
    dist.destroy_process_group()


@pytest.mark.parametrize("duplicate", [True, False])
def test_two_ranks_with_the_3d_front_end(tmp_path, duplicate, monkeypatch):
    import socket
    import torch.multiprocessing as mp
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker_dp, args=(2, port, str(tmp_path), duplicate), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert str(r0["mode"]).startswith("hipgraph") and bool(r0["refused"]) and bool(r1["refused"])
    names = [k for k in r0.files if k not in ("mode", "refused")]
    assert any(k.endswith("moving_variance") and "cnn" in k for k in names)
    W0 = _setup_dp(duplicate)[2]
    for k in names:
        assert np.array_equal(r0[k], r1[k]), k                       # replicas stay bit-identical, moving statistics included
    assert not np.array_equal(r0["video/cnn/layer0_bn/moving_mean"], W0["video/cnn/layer0_bn/moving_mean"])
    if not duplicate:
        return
    # the ranks hold the same utterances: per-rank statistics are the global ones, so two ranks equal one engine on the whole batch
    monkeypatch.setenv("AVSR_PERSISTENT_RNN", "0")
    O, mcfg, W, full = _setup_dp(True)
    model = Seq2SeqModel(mcfg, weights=W)
    batch = Batch.from_numpy(full)
    for _ in range(3):
        model.train_step(batch)
    torch.cuda.synchronize()
    for k, v in model.export_tf_weights("params").items():
        assert np.abs(r0[k] - v).max() <= 2e-5 + 1e-4 * np.abs(v).max(), (k, np.abs(r0[k] - v).max(), np.abs(v).max())


def test_export_under_the_reference_graph_names():
    model = _small_model((8, 16), 8, (20, 20, 3))
    W = model.export_tf_weights("params")
    T = model.export_tf_weights("params", tf_names=True)
    assert len(T) == len(W) and "video/cnn/conv3d_3/kernel" in T and "video/cnn/batch_normalization_2/moving_variance" in T
    assert np.array_equal(T["video/cnn/conv3d_4/kernel"], W["video/cnn/res_block_1_conv1/kernel"])
    assert [k for k in W if not k.startswith("video/cnn/")] == [k for k in T if not k.startswith("video/cnn/")]

"""Lip-crop augmentation on the GPU (csrc/video_augment.hip): the kernel against the numpy restatement of the rule
(tests/ref_video_augment.py), then the sharp statement of the feature -- a train step with augmentation equals, bit for bit, a train step
without it on crops that were augmented beforehand -- for both lip front-ends and together with SpecAugment's video time masks; that
nothing but the train graph augments; that a captured graph replays with fresh draws; that off is free; and two data-parallel ranks.

Tolerance of the channel means (contrast > 0 only; everything else is exact): the kernel adds fc * H * W terms into every fp32 partial
sum (fc frames per chunk, in some fixed order), the partials in fp64, and rounds once.  An fp32 sum of m terms deviates from the exact
one by at most (m - 1) * 2^-24 * sum|x_i| to first order, the final rounding adds 2^-24 * |mean|: the device's mean lies within
m * 2^-24 * mean|x| of the fp64 mean, m = fc * H * W, mean|x| over the same elements.  The pixels are then compared bit for bit with the
restatement evaluated at the DEVICE's means."""
import dataclasses
import os
import socket

import numpy as np
import pytest
import torch

import ref_video_augment as R
from test_gpu_specaugment import LIP_MODEL, SPEC_VIDEO, _assert_same_step, _batch, _check, _step_results, _weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 64
HALF = 1 << 23                                                # flip = 0.5


def _chunking(B, T):
    """(fc, chunks) of include/avsr_hip.h: fc = max(4, ceil(T / min(128, ceil(1024 / B))) rounded down to a multiple of 4)."""
    want = min(128, -(-1024 // B))
    fc = max(4, -(-T // want) // 4 * 4)
    return fc, -(-T // fc)


def _condition(seed, lens, T, S):
    """What the seeds of the kernel tests must show ON THE RESTATEMENT, among the utterances that have frames: a flipped and an
    unflipped one and, with S > 0, a dx of each sign and a dy of each sign."""
    g = [R.geometry(seed, b, HALF, S) for b, n in enumerate(lens) if R.clamp_len(n, T) > 0]
    ok = {f for f, _, _ in g} == {True, False}
    if S > 0:
        ok = ok and min(dx for _, dx, _ in g) < 0 < max(dx for _, dx, _ in g) and min(dy for _, _, dy in g) < 0 < max(dy for _, _, dy in g)
    return ok


def _pick_seed(lens, T, S, start=1):
    """The first seed from `start` whose draws meet _condition: chosen on the CPU, from the restatement alone."""
    for seed in range(start, start + 5000):
        if _condition(seed, lens, T, S):
            return seed
    raise AssertionError("no seed below %d meets the condition" % (start + 5000))


def _launch(x, lens, seed, S, contrast, brightness, q24=HALF):
    """One avsr_video_augment launch: y is allocated TAIL elements too long and pre-filled with NaN, and so is the workspace; returns
    (y, the device's channel means [B, C] | None) as numpy."""
    from avsr_tf1_amd import ops
    B, T, H, W, C = x.shape
    xd = torch.tensor(x, device="cuda")
    ld = torch.tensor(np.asarray(lens, np.int32), device="cuda")
    sd = torch.tensor([seed], dtype=torch.int32, device="cuda")
    flat = torch.full((x.size + TAIL,), float("nan"), device="cuda")
    y = flat[:x.size].view(x.shape)
    nws = ops.video_augment_ws_floats(B, T, H, W, C)
    assert nws == B * _chunking(B, T)[1] * C + B * C
    ws = torch.full((nws + TAIL,), float("nan"), device="cuda") if contrast > 0 else None
    ops.video_augment(xd, ld, sd, y, None if ws is None else ws[:nws], flip_q24=q24, max_shift=S, contrast=contrast, brightness=brightness)
    torch.cuda.synchronize()
    assert torch.isnan(flat[x.size:]).all(), "written past the end of y"
    assert ws is None or (torch.isnan(ws[nws:]).all() and not torch.isnan(ws[:nws]).any()), "the workspace: written past its end, or not all of it"
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the input was modified"
    return y.cpu().numpy(), None if ws is None else ws[nws - B * C:nws].cpu().numpy().reshape(B, C)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_means(x, lens, means):
    """The device's channel means against the fp64 means at the bound of the docstring; returns the worst error / bound."""
    B, T, H, W, C = x.shape
    m = _chunking(B, T)[0] * H * W                                                        # terms per fp32 partial
    want = R.channel_means(x, lens)
    worst = 0.0
    for b in range(B):
        n = R.clamp_len(lens[b], T)
        if not n:
            assert not means[b].any()
            continue
        bound = m * 2.0 ** -24 * np.abs(x[b, :n].astype(np.float64)).mean(axis=(0, 1, 2))
        err = np.abs(means[b].astype(np.float64) - want[b])
        assert (err <= bound).all(), (b, err, bound)
        worst = max(worst, float((err / bound).max()))
    return worst


def _check_launches(x, lens, seed, S):
    """Geometry only, brightness only and contrast + brightness at one seed, each against the restatement bit for bit."""
    y, _ = _launch(x, lens, seed, S, 0.0, 0.0)
    assert not np.isnan(y).any()
    assert _same_bits(y, R.apply(x, lens, seed, q24=HALF, S=S))                            # zero rows beyond len included
    assert _same_bits(y, _launch(x, lens, seed, S, 0.0, 0.0)[0])                           # two launches: identical bits
    yb, _ = _launch(x, lens, seed, S, 0.0, 0.3)
    assert _same_bits(yb, R.apply(x, lens, seed, q24=HALF, S=S, brightness=0.3)) and not _same_bits(yb, y)
    yc, means = _launch(x, lens, seed, S, 0.2, 0.3)
    worst = _check_means(x, lens, means)
    assert _same_bits(yc, R.apply(x, lens, seed, q24=HALF, S=S, contrast=0.2, brightness=0.3, means=means))
    yc2, means2 = _launch(x, lens, seed, S, 0.2, 0.3)
    assert _same_bits(yc, yc2) and _same_bits(means, means2)
    y0, _ = _launch(x, lens, seed, S, 0.2, 0.0)                                            # contrast alone: d = 0
    assert _same_bits(y0, R.apply(x, lens, seed, q24=HALF, S=S, contrast=0.2, means=means))
    return worst


@pytest.mark.parametrize("shift", ["none", "one", "widest"])
@pytest.mark.parametrize("H,W,C", [(36, 36, 3), (5, 7, 1), (6, 4, 4)])                     # lip crops; odd, non-square, scalar stores; 16-byte path
def test_kernel_against_the_restatement(H, W, C, shift):
    B, T, lens = 4, 5, [5, 3, 0, 1]
    S = {"none": 0, "one": 1, "widest": min(H, W) - 1}[shift]
    seed = _pick_seed(lens, T, S)
    assert _condition(seed, lens, T, S)
    x = np.random.default_rng(H * 100 + C).random((B, T, H, W, C)).astype(np.float32) - np.float32(0.25)
    x[0, 0, 0, 0, 0] = -0.0
    worst = _check_launches(x, lens, seed, S)
    print("%dx%dx%d, S %d, seed %d: draws %s; worst mean error / bound %.3f"
          % (H, W, C, S, seed, [R.geometry(seed, b, HALF, S) for b in range(B)], worst))
    other, _ = _launch(x, lens, seed + 1, S, 0.0, 0.3)
    assert not _same_bits(other, _launch(x, lens, seed, S, 0.0, 0.3)[0])                   # another key: other draws


@pytest.mark.parametrize("H,W,C", [(36, 36, 3), (5, 7, 1)])
def test_kernel_with_utterances_that_span_several_frame_chunks(H, W, C):
    B, T, lens = 2, 40, [40, 23]
    assert _chunking(B, T) == (4, 10)                                                     # a length inside a chunk, chunks beyond a length
    S = 2
    seed = _pick_seed(lens, T, S)
    assert _condition(seed, lens, T, S)
    x = np.random.default_rng(11).random((B, T, H, W, C)).astype(np.float32)
    _check_launches(x, lens, seed, S)


def test_flip_probabilities_zero_and_one_and_lengths_outside_the_batch():
    x = np.random.default_rng(5).random((3, 5, 6, 4, 4)).astype(np.float32)
    lens = [9, -1, 4]                                                                     # clamped to [0, T]
    y1, _ = _launch(x, lens, 3, 0, 0.0, 0.0, q24=1 << 24)
    assert _same_bits(y1[0], x[0, :, :, ::-1, :]) and not y1[1].any() and _same_bits(y1[2, :4], x[2, :4, :, ::-1, :]) and not y1[2, 4:].any()
    y0, _ = _launch(x, lens, 3, 0, 0.0, 0.0, q24=0)                                       # (every value 0: the host launches nothing; the
    assert _same_bits(y0[0], x[0]) and _same_bits(y0[2, :4], x[2, :4])                    # kernel copies)


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
VAUG = dict(vaug_flip_q24=HALF, vaug_max_shift=3, vaug_contrast=0.2, vaug_brightness=0.2)
MODELS = {"resnet_cnn": LIP_MODEL, "3dconv_cnn": dict(LIP_MODEL, video_processing="3dconv_cnn", cnn_filters=(8, 16))}


def _augmented(m):
    """(the augmented crops, the device's channel means | None) of the model's last train step."""
    from avsr_tf1_amd import ops
    E = m._cur[0]["enc"]["video"]
    y = E["va_x"].cpu().numpy().copy()
    if "va_ws" not in E:
        return y, None
    B, T, H, W, C = y.shape
    nws = ops.video_augment_ws_floats(B, T, H, W, C)
    return y, E["va_ws"][nws - B * C:nws].cpu().numpy().reshape(B, C).copy()


def _check_augmented(raw, lens, y, means, key, cfg):
    """y against the restatement under `key`, at the device's means (themselves within their bound); returns the draws."""
    a = cfg.video_augment_args()
    if means is not None:
        _check_means(raw, lens, means)
    assert _same_bits(y, R.apply(raw, lens, key, q24=a["flip_q24"], S=a["max_shift"], contrast=a["contrast"], brightness=a["brightness"],
                                 means=means))
    return [R.geometry(key, b, a["flip_q24"], a["max_shift"]) for b in range(len(lens))]


@pytest.mark.parametrize("spec", [False, True], ids=["alone", "with_spec_augment"])
@pytest.mark.parametrize("proc", ["resnet_cnn", "3dconv_cnn"])
def test_step_with_augmentation_equals_step_on_preaugmented_crops(proc, spec):
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    plain = ModelConfig(**MODELS[proc])
    aug = dataclasses.replace(plain, **VAUG, **(SPEC_VIDEO if spec else {}))
    W = _weights(plain)
    batch = _batch(plain, B=3)
    raw, lens = batch.video.cpu().numpy().copy(), batch.video_len.cpu().numpy()
    ma = Seq2SeqModel(aug, weights=W)
    ra = _step_results(ma, batch)
    y, means = _augmented(ma)
    assert _same_bits(batch.video.cpu().numpy(), raw)                                     # the batch is never written
    draws = _check_augmented(raw, lens, y, means, 0, ma.cfg)                              # step 0, rank 0: key 0
    assert any(f or dx or dy for f, dx, dy in draws) and not np.array_equal(y, raw)
    fed = y
    if spec:        # exactly "spec-augment the augmented crops": the time masks of key 0 on y, filled with y's own column means
        E = ma._cur[0]["enc"]["video"]
        fed = E["sa_x"].cpu().numpy().reshape(y.shape).copy()
        mask, _ = _check(y.reshape(y.shape[0], y.shape[1], -1), lens, fed.reshape(y.shape[0], y.shape[1], -1), 0,
                         ma.cfg.spec_augment_args("video"), True)
        assert mask.any()
    mb = Seq2SeqModel(plain, weights=W)
    rb = _step_results(mb, dataclasses.replace(batch, video=torch.tensor(fed).cuda()))
    assert not any(k.startswith("va_") for k in mb._cur[0]["enc"]["video"])
    _assert_same_step(ra, rb)
    # and it IS another step than the one on the raw batch
    rc = _step_results(Seq2SeqModel(plain, weights=W), batch)
    assert not np.array_equal(rc["grads"], ra["grads"])


def test_only_the_train_graph_augments():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    plain = ModelConfig(**LIP_MODEL)
    aug = dataclasses.replace(plain, **VAUG)
    W = _weights(plain)
    batch = _batch(plain, B=3)
    out = {}
    for name, cfg in (("plain", plain), ("aug", aug)):
        m = Seq2SeqModel(cfg, weights=W)
        out[name] = dict(greedy=m.greedy_decode(batch, max_steps=8).cpu().numpy(),
                         beam=m.beam_search_decode(batch, beam_width=4, max_steps=8).cpu().numpy(),
                         prefix=m.ctc_prefix_beam_search(batch, beam_width=4, max_steps=8, nbest=True),
                         rescore=m.attention_rescoring(batch, beam_width=4, max_steps=8, ctc_weight=0.3, nbest=True),
                         align=m.ctc_align(batch), best=m.ctc_best_path(batch))
        assert not any(k.startswith("va_") for ws in m._ws_cache.values() for k in ws["enc"]["video"])   # evaluation workspaces: no buffer
    a, b = out["plain"], out["aug"]
    assert np.array_equal(a["greedy"], b["greedy"]) and np.array_equal(a["beam"], b["beam"])
    assert a["prefix"] == b["prefix"] and a["rescore"] == b["rescore"] and a["align"] == b["align"] and a["best"] == b["best"]


def test_evaluate_is_the_same_with_and_without_the_keyword(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import io_utils as IO
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(1)
    unit_file = os.path.join(str(tmp_path), "character_list")
    open(unit_file, "w").write("\n".join(list("' abcdefghijklmnopqrstuvwxyz")) + "\n")
    vrec, lrec = os.path.join(str(tmp_path), "video.tfrecord"), os.path.join(str(tmp_path), "labels.tfrecord")
    with IO.TFRecordFileWriter(vrec) as fv, IO.TFRecordFileWriter(lrec) as fl:
        for i in range(4):
            fv.write(IO.make_video_example("utt%02d" % i, rng.random((int(rng.integers(4, 8)), 20, 20, 3)).astype(np.float32)))
            fl.write(IO.make_label_example("utt%02d" % i, rng.integers(3, 10, size=3).tolist(), "character"))
    kw = dict(unit="character", unit_file=unit_file, video_processing="resnet_cnn", video_train_record=vrec, video_test_record=vrec,
              labels_train_record=lrec, labels_test_record=lrec, batch_size=(4, 4), encoder_units_per_layer=((16,), (16,)),
              decoder_units_per_layer=(16,), embedding_size=8, cnn_dense_units=16, warmup_steps=0, shuffle_seed=0, architecture="unimodal")
    res = {}
    for algo in ("greedy", "beam_search"):
        plain = avsr.AVSR(decoding_algorithm=algo, **kw)
        plain.save("checkpoints/va/checkpoint.ckp-0")
        exp = avsr.AVSR(decoding_algorithm=algo, video_augment=dict(flip=0.5, max_shift=3, contrast=0.2, brightness=0.2), **kw)
        assert exp._cfg.video_augment_args() is not None
        for name, e in (("plain", plain), ("aug", exp)):
            err = e.evaluate("checkpoints/va/checkpoint.ckp-0", epoch=name)
            res[algo, name] = (err, open("predictions/va/predicted_epoch_%s.mlf" % name).read())
        assert res[algo, "plain"] == res[algo, "aug"]


def test_a_captured_graph_replays_with_fresh_draws():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    aug = ModelConfig(**LIP_MODEL, **VAUG)
    W = _weights(aug)
    batch = _batch(aug, B=3)
    raw, lens = batch.video.cpu().numpy().copy(), batch.video_len.cpu().numpy()
    out = {}
    for mode in ("eager", "graph"):
        m = Seq2SeqModel(aug, weights=W)
        t = DataParallelTrainer(m, None, use_graph=(mode == "graph"), graph_after=2)
        trace, bufs = [], []
        for _ in range(4):
            loss, gnorm = t.train_step(batch)
            torch.cuda.synchronize()
            trace.append((loss.cpu().numpy().tobytes(), gnorm.cpu().numpy().tobytes()))
            bufs.append(_augmented(m))
        assert mode == "eager" or t.mode == "hipgraph"
        out[mode] = (trace, bufs, m.params.cpu().numpy().copy())
    assert out["eager"][0] == out["graph"][0]                                             # losses and norms, step by step, bit for bit
    assert np.array_equal(out["eager"][2], out["graph"][2])
    bufs = out["graph"][1]                                                                # steps 3 and 4 were replays
    assert not np.array_equal(bufs[2][0], bufs[3][0])
    draws = []
    for step in (2, 3):
        draws.append(_check_augmented(raw, lens, bufs[step][0], bufs[step][1], step, aug.engine()))
        assert _same_bits(bufs[step][0], out["eager"][1][step][0])
    assert draws[0] != draws[1]
    assert _same_bits(batch.video.cpu().numpy(), raw)


def test_off_is_free():
    from avsr_tf1_amd.config import ModelConfig, video_augment_fields
    from avsr_tf1_amd.model import Seq2SeqModel
    plain = ModelConfig(**LIP_MODEL)
    W = _weights(plain)
    batch = _batch(plain, B=3)
    ref = _step_results(Seq2SeqModel(plain, weights=W), batch)
    for spec in (None, dict(flip=0, max_shift=0, contrast=0.0, brightness=0.0)):
        cfg = ModelConfig(**LIP_MODEL, **video_augment_fields(spec))
        assert cfg.video_augment_args() is None
        m = Seq2SeqModel(cfg, weights=W)
        _assert_same_step(ref, _step_results(m, batch))
        assert not any(k.startswith("va_") for ws in m._ws_cache.values() for k in ws["enc"]["video"])


def test_a_batch_outside_the_kernels_limits_is_refused_when_it_arrives():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    m = Seq2SeqModel(ModelConfig(**LIP_MODEL, **VAUG), weights=_weights(ModelConfig(**LIP_MODEL)))
    with pytest.raises(ValueError, match="video_augment.*65535"):
        m._get_ws(1, 12, 65536, 5, False)                                                 # (refused ahead of the CNN's buffers)


# ---- two data-parallel ranks ---------------------------------------------------------------------------------------------------------
DP_STEPS, DP_CUT = 2, [0, 2, 4]


def _dp_setup():
    from avsr_tf1_amd.config import ModelConfig
    cfg = ModelConfig(**LIP_MODEL, **VAUG)
    return cfg, _weights(cfg), _batch(cfg, B=4, seed=11)


def _dp_shard(batch, lo, hi):
    keys = ("audio", "audio_len", "video", "video_len", "labels", "labels_len")
    return dataclasses.replace(batch, **{k: getattr(batch, k)[lo:hi].contiguous() for k in keys})


def _dp_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["AVSR_PERSISTENT_RNN"] = "0"                  # two processes on ONE GPU do not both claim the chip
    import torch.distributed as dist
    from avsr_tf1_amd.model import Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, W, full = _dp_setup()
    model = Seq2SeqModel(cfg, weights=W)
    trainer = DataParallelTrainer(model, dist, use_graph=False)
    batch = _dp_shard(full, DP_CUT[rank], DP_CUT[rank + 1])
    saved = {}
    for step in range(DP_STEPS):
        trainer.train_step(batch)
        torch.cuda.synchronize()
        saved["aug%d" % step], saved["means%d" % step] = _augmented(model)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=model.params.cpu().numpy(), stats=model.stats.cpu().numpy(), **saved)
    dist.destroy_process_group()


def test_two_ranks_draw_under_different_keys_and_stay_identical(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r = [np.load(tmp_path / ("rank%d.npz" % k)) for k in range(2)]
    cfg, W, full = _dp_setup()
    raw, lens = full.video.cpu().numpy(), full.video_len.cpu().numpy()
    assert np.array_equal(r[0]["params"], r[1]["params"]) and np.array_equal(r[0]["stats"], r[1]["stats"])    # replicas stay bit-identical
    a = cfg.video_augment_args()
    for step in range(DP_STEPS):
        for k in range(2):
            lo, hi = DP_CUT[k], DP_CUT[k + 1]
            key = step + (k << 24)                                                        # this rank's key: step + (rank << 24)
            _check_augmented(raw[lo:hi], lens[lo:hi], r[k]["aug%d" % step], r[k]["means%d" % step], key, cfg)
        # rows 0, 1 of the two ranks draw differently: rank 1's shard under rank 0's key is not what rank 1 computed
        d0 = [R.geometry(step, b, a["flip_q24"], a["max_shift"]) + R.photometric(step, b, a["contrast"], a["brightness"]) for b in range(2)]
        d1 = [R.geometry(step + (1 << 24), b, a["flip_q24"], a["max_shift"]) + R.photometric(step + (1 << 24), b, a["contrast"], a["brightness"])
              for b in range(2)]
        assert d0 != d1
        other = R.apply(raw[2:4], lens[2:4], step, q24=a["flip_q24"], S=a["max_shift"], contrast=a["contrast"], brightness=a["brightness"],
                        means=r[1]["means%d" % step])
        assert not np.array_equal(other, r[1]["aug%d" % step])

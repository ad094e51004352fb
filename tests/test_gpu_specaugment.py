"""SpecAugment on the GPU (csrc/specaugment.hip): the kernel against the numpy restatement of the rule (tests/ref_specaugment.py), then the
sharp statement of the feature -- a train step with augmentation equals, bit for bit, a train step without it on inputs that were masked
beforehand -- for a feature model, a lip-crop model and a waveform model; that nothing but the train graph augments; that a captured
graph replays with fresh masks; and two data-parallel ranks with synchronised input batch norm.

Tolerance of the 'mean' fill: a column mean over n rows formed in fp32 in any order deviates from the fp64 mean by at most
n * 2^-23 * max|x| of that column (a-priori bound of an fp32 sum); everything else is exact."""
import dataclasses
import os
import socket

import numpy as np
import pytest
import torch

import ref_specaugment as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 64


def _streams():
    from avsr_tf1_amd import config as CF
    return CF.SPEC_STREAM_AUDIO_FREQ, CF.SPEC_STREAM_AUDIO_TIME, CF.SPEC_STREAM_VIDEO_TIME


def _ref_mask(seed, lens, T, F_in, p, parts=False):
    """The restatement's mask for the draw parameters p (the dict ModelConfig.spec_augment_args returns, or one like it)."""
    sf, st, sv = _streams()
    kw = dict(n_time=p.get("time_masks", 0), time_width=p.get("time_width", 0), time_ratio=p.get("ratio_q16", 65536) / 65536.0)
    stream = sv if p.get("video") else st
    if not parts:
        return R.mask(seed, lens, T, F_in, stream, freq_stream=sf, n_freq=p.get("freq_masks", 0), freq_width=p.get("freq_width", 0),
                      freq_bins=p.get("freq_bins") or None, **kw)
    out = [R.mask(seed, lens, T, F_in, stream, n_time=0)]                        # one boolean mask per drawn mask
    for k in range(kw["n_time"]):
        m = np.zeros_like(out[0])
        for b in range(len(lens)):
            n = int(min(max(int(lens[b]), 0), T))
            t0, w = R.time_masks(seed, stream, b, n, kw["n_time"], kw["time_width"], kw["time_ratio"])[k]
            m[b, t0:t0 + w] = True
        out.append(m)
    P = p.get("freq_bins") or F_in
    for k in range(p.get("freq_masks", 0)):
        m = np.zeros_like(out[0])
        cm = np.arange(F_in) % P
        for b in range(len(lens)):
            n = int(min(max(int(lens[b]), 0), T))
            f0, w = R.freq_masks(seed, sf, b, P, p["freq_masks"], p["freq_width"])[k]
            m[b, :n, (cm >= f0) & (cm < f0 + w)] = True
        out.append(m)
    return out[1:]


def _condition(seed, lens, T, F_in, p):
    """What the seeds of the kernel test must show ON THE RESTATEMENT: in every utterance with n >= 5 a non-empty time mask and (audio) a
    non-empty band, and somewhere an element that two masks cover."""
    parts = _ref_mask(seed, lens, T, F_in, p, parts=True)
    nt = p.get("time_masks", 0)
    for b, n in enumerate(lens):
        if min(max(int(n), 0), T) >= 5:
            if not any(m[b].any() for m in parts[:nt]):
                return False
            if p.get("freq_masks", 0) and not any(m[b].any() for m in parts[nt:]):
                return False
    return bool((np.sum(parts, axis=0) >= 2).any())


def _pick_seed(lens, T, F_in, p, start=1):
    """The first seed from `start` whose draws meet _condition: chosen on the CPU, from the restatement alone."""
    for seed in range(start, start + 2000):
        if _condition(seed, lens, T, F_in, p):
            return seed
    raise AssertionError("no seed below %d meets the condition" % (start + 2000))


def _launch(x, lens, F, seed, p, mean):
    """One avsr_spec_augment launch: y is allocated TAIL elements too long and pre-filled with NaN; returns y [B, T, F] (numpy)."""
    from avsr_tf1_amd import ops
    B, T, F_in = x.shape
    xd = torch.tensor(x, device="cuda")
    ld = torch.tensor(np.asarray(lens, np.int32), device="cuda")
    sd = torch.tensor([seed], dtype=torch.int32, device="cuda")
    flat = torch.full((B * T * F + TAIL,), float("nan"), device="cuda")
    y = flat[:B * T * F].view(B, T, F)
    ws = torch.full((ops.spec_augment_ws_floats(B, T, F_in) + TAIL,), float("nan"), device="cuda") if mean else None
    kw = {k: v for k, v in p.items() if k != "mean_fill"}
    ops.spec_augment(xd, F_in, ld, sd, y, None if ws is None else ws[:ws.numel() - TAIL], mean_fill=mean, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(flat[B * T * F:]).all(), "written past the end of y"
    assert ws is None or torch.isnan(ws[ws.numel() - TAIL:]).all(), "written past the end of the workspace"
    assert np.array_equal(xd.cpu().numpy(), x), "the input was modified"
    return y.cpu().numpy()


def _check(x, lens, y, seed, p, mean):
    """y against the restatement at `seed`: the masked set exactly, unmasked elements bit for bit, padding and rows beyond len exactly
    zero, nothing NaN, 'zero' exact, 'mean' within n * 2^-23 * max|x| of the fp64 mean."""
    B, T, F_in = x.shape
    F = y.shape[2]
    assert not np.isnan(y).any()
    m = _ref_mask(seed, lens, T, F_in, p)
    ref, mu = R.apply(x, lens, F, m, "mean" if mean else "zero")
    assert not y[:, :, F_in:].any()
    worst = 0.0
    for b in range(B):
        n = int(min(max(int(lens[b]), 0), T))
        assert not y[b, n:].any()
        yb, xb, mb = y[b, :n, :F_in], x[b, :n], m[b, :n]
        assert np.array_equal(yb[~mb].view(np.uint32), xb[~mb].view(np.uint32))           # bit for bit (signed zeros included)
        if not mean:
            assert not yb[mb].any()
            continue
        if n:
            bound = n * 2.0 ** -23 * np.abs(xb).max(axis=0)
            err = np.abs(yb.astype(np.float64) - ref[b, :n, :F_in])
            assert (err <= bound[None, :])[mb].all(), (b, float((err - bound[None, :])[mb].max()))
            worst = max(worst, float((err[mb] / np.maximum(np.broadcast_to(bound, err.shape)[mb], 1e-300)).max()) if mb.any() else 0.0)
        # the masked set: a masked element holds the fill, not its input (random inputs never equal the mean of >= 2 rows)
        assert n < 2 or (yb[mb] != xb[mb]).all()
    return m, worst


AUDIO_P = dict(video=False, time_masks=2, time_width=6, ratio_q16=R.ratio_q16(0.5), freq_masks=2, freq_width=2)
KERNEL_CASES = [(12, 12, 4), (10, 12, 5)]                    # (F_in, F, P): three stacked frames of 4 bins; an odd leading dimension + padding
KERNEL_LENS = [(17, 5, 0), (17, 1, 9)]


@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("lens", KERNEL_LENS)
@pytest.mark.parametrize("F_in,F,P", KERNEL_CASES)
def test_kernel_against_the_restatement(F_in, F, P, lens, mean):
    B, T = 3, 17
    p = dict(AUDIO_P, freq_bins=P)
    seed = _pick_seed(lens, T, F_in, p)
    assert _condition(seed, lens, T, F_in, p)
    x = np.random.default_rng(100 + F_in).standard_normal((B, T, F_in)).astype(np.float32)
    y = _launch(x, lens, F, seed, p, mean)
    m, worst = _check(x, lens, y, seed, p, mean)
    print("F_in %d -> %d, P %d, lens %s, seed %d: %d masked of %d; worst fill error / bound %.3f" % (F_in, F, P, lens, seed, m.sum(), m.size, worst))
    assert np.array_equal(y, _launch(x, lens, F, seed, p, mean))                          # two runs: identical bits
    other = _launch(x, lens, F, seed + 1, p, mean)
    assert not np.array_equal(y, other)                                                   # another key: other masks


@pytest.mark.parametrize("mean", [True, False])
def test_kernel_on_lip_crops_time_masks_only(mean):
    B, T, HWC = 2, 6, 8 * 8 * 3
    lens = (6, 5)
    p = dict(video=True, time_masks=2, time_width=3, ratio_q16=65536)
    seed = _pick_seed(lens, T, HWC, p)
    x = np.random.default_rng(7).random((B, T, HWC)).astype(np.float32)
    y = _launch(x, lens, HWC, seed, p, mean)
    m, worst = _check(x, lens, y, seed, p, mean)
    assert (m == m[:, :, :1]).all() and m.any()                                           # whole frames
    # the audio stream's time masks under the same key are other draws (independent streams)
    assert not np.array_equal(m, _ref_mask(seed, lens, T, HWC, dict(p, video=False)))


def test_kernel_with_several_row_chunks_and_wide_rows():
    """More than one row chunk per utterance, rows wider than a workgroup's 256 column quads, a length inside a chunk."""
    B, T, F_in = 2, 41, 1100
    lens = (41, 23)
    p = dict(video=False, time_masks=3, time_width=9, ratio_q16=65536, freq_masks=2, freq_width=30, freq_bins=110)
    seed = _pick_seed(lens, T, F_in, p)
    x = np.random.default_rng(9).standard_normal((B, T, F_in)).astype(np.float32)
    for mean in (True, False):
        _check(x, lens, _launch(x, lens, F_in, seed, p, mean), seed, p, mean)


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
SPEC_AUDIO = dict(spec_freq_masks=2, spec_freq_width=2, spec_freq_bins=4, spec_time_masks=2, spec_time_width=4, spec_time_ratio=0.5)
SPEC_VIDEO = dict(spec_video_time_masks=2, spec_video_time_width=2, spec_video_time_ratio=1.0)
AUDIO_MODEL = dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(16,), decoder_units=(16,),
                   embedding_size=8, audio_feat=12, warmup_steps=0, use_ctc=True, use_dropout=True, sampling_probability=0.2)
LIP_MODEL = dict(architecture="av_align", encoder_type="unidirectional", video_units=(16,), audio_units=(16, 16), decoder_units=(16,),
                 embedding_size=8, audio_feat=12, warmup_steps=0, use_ctc=True,
                 video_processing="resnet_cnn", cnn_filters=(8, 16, 32, 64), cnn_dense_units=16, video_feat=16)
WAV_MODEL = dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(16,), decoder_units=(16,),
                 embedding_size=8, audio_feat=240, warmup_steps=0, use_ctc=True, use_dropout=True, sampling_probability=0.2)


def _weights(cfg, seed=5):
    from avsr_tf1_amd import params as PR
    return PR.initialise(cfg, seed=seed)


def _batch(cfg, B=4, Ta=12, Tv=5, L=5, seed=3, audio_lens=None):
    from avsr_tf1_amd.model import Batch
    rng = np.random.default_rng(seed)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    lab = rng.integers(1, cfg.eos_id, size=(B, L)).astype(np.int32)
    ll = rng.integers(2, 4, size=B).astype(np.int32)                     # short rows: the CTC head has an alignment on every utterance
    for i in range(B):
        lab[i, ll[i] - 1] = cfg.eos_id
        lab[i, ll[i]:] = 0
    f = dict(labels=t(lab, torch.int32), labels_len=t(ll, torch.int32))
    if cfg.audio_units is not None:
        al = np.asarray(audio_lens if audio_lens is not None else [Ta] + list(rng.integers(6, Ta + 1, size=B - 1)))
        a = rng.standard_normal((B, Ta, cfg.audio_feat)).astype(np.float32) + 0.5
        a *= (np.arange(Ta)[None, :] < al[:, None])[:, :, None]
        f.update(audio=t(a, torch.float32), audio_len=t(al, torch.int32))
    if cfg.video_units is not None:
        vl = np.asarray([Tv] + list(rng.integers(3, Tv + 1, size=B - 1)))
        v = rng.random((B, Tv) + (tuple(cfg.video_hw) if cfg.video_processing != "features" else (cfg.video_feat,))).astype(np.float32)
        v *= (np.arange(Tv)[None, :] < vl[:, None]).reshape((B, Tv) + (1,) * (v.ndim - 2))
        f.update(video=t(v, torch.float32), video_len=t(vl, torch.int32))
    return Batch(**f)


def _step_results(m, batch):
    loss, gnorm = m.train_step(batch)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu().numpy().copy(), gnorm=gnorm.cpu().numpy().copy(), grads=m.grads.cpu().numpy().copy(),
                params=m.params.cpu().numpy().copy(), stats=m.stats.cpu().numpy().copy())


def _assert_same_step(a, b):
    for k in ("loss", "gnorm", "grads", "params", "stats"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.isfinite(a["loss"]).all() and np.abs(a["grads"]).max() > 0


def _augmented(m, s):
    E = m._cur[0]["enc"][s]
    return E["sa_x"].cpu().numpy().copy(), E


def test_step_with_augmentation_equals_step_on_premasked_features():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    plain = ModelConfig(**AUDIO_MODEL)
    aug = dataclasses.replace(plain, **SPEC_AUDIO)
    W = _weights(plain)
    batch = _batch(plain)
    raw = batch.audio.cpu().numpy().copy()
    ma = Seq2SeqModel(aug, weights=W)
    ra = _step_results(ma, batch)
    y, _ = _augmented(ma, "audio")
    assert np.array_equal(batch.audio.cpu().numpy(), raw)                                 # the batch is never written
    lens = batch.audio_len.cpu().numpy()
    m, _ = _check(raw, lens, y, 0, ma.cfg.spec_augment_args("audio"), True)               # step 0, rank 0: key 0
    assert m.any() and not np.array_equal(y, raw)
    mb = Seq2SeqModel(plain, weights=W)
    assert "sa_x" not in mb.prepare_workspace(batch)["enc"]["audio"]                      # off: nothing allocated
    rb = _step_results(mb, dataclasses.replace(batch, audio=torch.tensor(y).cuda()))
    _assert_same_step(ra, rb)
    # and it IS another step than the one on the raw batch
    rc = _step_results(Seq2SeqModel(plain, weights=W), batch)
    assert not np.array_equal(rc["grads"], ra["grads"])
    # 'zero' fill through the engine
    mz = Seq2SeqModel(dataclasses.replace(aug, spec_mask_value="zero"), weights=W)
    rz = _step_results(mz, batch)
    yz, _ = _augmented(mz, "audio")
    _check(raw, lens, yz, 0, mz.cfg.spec_augment_args("audio"), False)
    _assert_same_step(rz, _step_results(Seq2SeqModel(plain, weights=W), dataclasses.replace(batch, audio=torch.tensor(yz).cuda())))


def test_step_with_augmentation_equals_step_on_premasked_lip_crops():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    plain = ModelConfig(**LIP_MODEL)
    aug = dataclasses.replace(plain, **SPEC_AUDIO, **SPEC_VIDEO)
    W = _weights(plain)
    batch = _batch(plain, B=3)
    ma = Seq2SeqModel(aug, weights=W)
    ra = _step_results(ma, batch)
    ya, _ = _augmented(ma, "audio")
    yv, _ = _augmented(ma, "video")
    rawv = batch.video.cpu().numpy().reshape(yv.shape)
    mv, _ = _check(rawv, batch.video_len.cpu().numpy(), yv, 0, ma.cfg.spec_augment_args("video"), True)
    _check(batch.audio.cpu().numpy(), batch.audio_len.cpu().numpy(), ya, 0, ma.cfg.spec_augment_args("audio"), True)
    assert mv.any()
    pre = dataclasses.replace(batch, audio=torch.tensor(ya).cuda(), video=torch.tensor(yv.reshape(batch.video.shape)).cuda())
    _assert_same_step(ra, _step_results(Seq2SeqModel(plain, weights=W), pre))


def test_step_from_waveforms_with_augmentation_equals_step_on_premasked_features():
    """The waveform model augments what its front-end produced, with that front-end's device-side row counts; a 'features' model fed the
    read-back buffer runs the same kernels on the same values from there on: compared bit for bit (not at the tolerance of
    tests/test_gpu_logmel.py, which compares the front-end itself against the restatement's features)."""
    from avsr_tf1_amd.audio_frontend import LogmelSpec
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    feat = ModelConfig(**WAV_MODEL)
    wav = dataclasses.replace(feat, audio_processing="wav", spec_freq_masks=2, spec_freq_width=7, spec_time_masks=2, spec_time_width=4,
                              spec_time_ratio=0.5)
    W = _weights(feat)
    spec = LogmelSpec()
    rows = [12, 7, 1, 9]
    rng = np.random.default_rng(4)
    N = spec.samples_for_rows(max(rows))
    ns = np.minimum([spec.samples_for_rows(r) + 5 for r in rows], N)
    x = np.zeros((len(rows), N), np.float32)
    for i, n in enumerate(ns):
        x[i, :n] = rng.standard_normal(int(n)) * 0.1
    bf = _batch(feat, B=4, Ta=12)
    bw = dataclasses.replace(bf, audio=torch.tensor(x).cuda(), audio_len=torch.tensor(ns.astype(np.int32)).cuda())
    mw = Seq2SeqModel(wav, weights=W)
    rw = _step_results(mw, bw)
    y, E = _augmented(mw, "audio")
    rows_dev = E["wav_len"].cpu().numpy()
    assert list(rows_dev) == rows
    assert mw.cfg.spec_augment_args("audio")["freq_bins"] == 30
    m, _ = _check(E["wav_x"].cpu().numpy()[:, :, :240], rows_dev, y, 0, mw.cfg.spec_augment_args("audio"), True)
    cols = m[0, :12].all(axis=0).reshape(8, 30)                                           # (the spans cover at most 8 of the 12 rows)
    assert m.any() and cols.any() and (cols == cols[:1]).all()                            # a band hits the same bin of every stacked frame
    pre = dataclasses.replace(bf, audio=torch.tensor(y[:, :, :240]).cuda(), audio_len=torch.tensor(rows_dev).cuda())
    _assert_same_step(rw, _step_results(Seq2SeqModel(feat, weights=W), pre))


def test_only_the_train_graph_augments():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    plain = ModelConfig(**dict(AUDIO_MODEL, use_dropout=False, sampling_probability=0.0))
    aug = dataclasses.replace(plain, **SPEC_AUDIO)
    W = _weights(plain)
    batch = _batch(plain)
    out = {}
    for name, cfg in (("plain", plain), ("aug", aug)):
        m = Seq2SeqModel(cfg, weights=W)
        out[name] = dict(greedy=m.greedy_decode(batch, max_steps=8).cpu().numpy(),
                         beam=m.beam_search_decode(batch, beam_width=4, max_steps=8).cpu().numpy(),
                         prefix=m.ctc_prefix_beam_search(batch, beam_width=4, max_steps=8, nbest=True),
                         rescore=m.attention_rescoring(batch, beam_width=4, max_steps=8, ctc_weight=0.3, nbest=True),
                         align=m.ctc_align(batch))
        assert all("sa_x" not in E for ws in m._ws_cache.values() for E in ws["enc"].values())   # evaluation workspaces: no buffer
    a, b = out["plain"], out["aug"]
    assert np.array_equal(a["greedy"], b["greedy"]) and np.array_equal(a["beam"], b["beam"])
    assert a["prefix"] == b["prefix"] and a["rescore"] == b["rescore"] and a["align"] == b["align"]


def test_a_captured_graph_replays_with_fresh_masks():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    aug = ModelConfig(**AUDIO_MODEL, **SPEC_AUDIO)
    W = _weights(aug)
    batch = _batch(aug)
    raw, lens = batch.audio.cpu().numpy().copy(), batch.audio_len.cpu().numpy()
    out = {}
    for mode in ("eager", "graph"):
        m = Seq2SeqModel(aug, weights=W)
        t = DataParallelTrainer(m, None, use_graph=(mode == "graph"), graph_after=2)
        trace, bufs = [], []
        for _ in range(4):
            loss, gnorm = t.train_step(batch)
            torch.cuda.synchronize()
            trace.append((loss.cpu().numpy().tobytes(), gnorm.cpu().numpy().tobytes()))
            bufs.append(_augmented(m, "audio")[0])
        assert mode == "eager" or t.mode == "hipgraph"
        out[mode] = (trace, bufs, m.params.cpu().numpy().copy())
    assert out["eager"][0] == out["graph"][0]                                             # losses and norms, step by step, bit for bit
    assert np.array_equal(out["eager"][2], out["graph"][2])
    bufs = out["graph"][1]                                                                # steps 3 and 4 were replays
    assert not np.array_equal(bufs[2], bufs[3])
    for step in (2, 3):
        m, _ = _check(raw, lens, bufs[step], step, aug.engine().spec_augment_args("audio"), True)
        assert m.any() and np.array_equal(bufs[step], out["eager"][1][step])
    assert np.array_equal(batch.audio.cpu().numpy(), raw)


# ---- two data-parallel ranks, synchronised input batch norm --------------------------------------------------------------------------
DP_MODEL = dict(AUDIO_MODEL, use_dropout=False, sampling_probability=0.0)
DP_STEPS, DP_CUT = 2, [0, 2, 6]


def _dp_setup():
    from avsr_tf1_amd.config import ModelConfig
    cfg = ModelConfig(**DP_MODEL, **SPEC_AUDIO)
    return cfg, _weights(cfg), _batch(cfg, B=6, seed=11)


def _dp_shard(batch, lo, hi):
    return dataclasses.replace(batch, **{k: getattr(batch, k)[lo:hi].contiguous() for k in ("audio", "audio_len", "labels", "labels_len")})


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
        saved["aug%d" % step] = _augmented(model, "audio")[0]
        o = model.bn_sync["off"]["audio"]
        saved["mean%d" % step] = model.bn_sync["mean"][o:o + model.cfg.audio_feat].cpu().numpy().copy()
    assert trainer.sync_bn
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=model.params.cpu().numpy(), stats=model.stats.cpu().numpy(), **saved)
    dist.destroy_process_group()


def test_two_ranks_with_synchronised_input_batch_norm(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r = [np.load(tmp_path / ("rank%d.npz" % k)) for k in range(2)]
    cfg, _, full = _dp_setup()
    p = cfg.engine().spec_augment_args("audio")
    raw, lens = full.audio.cpu().numpy(), full.audio_len.cpu().numpy()
    assert np.array_equal(r[0]["params"], r[1]["params"]) and np.array_equal(r[0]["stats"], r[1]["stats"])    # replicas stay bit-identical
    for step in range(DP_STEPS):
        shards = []
        for k in range(2):
            lo, hi = DP_CUT[k], DP_CUT[k + 1]
            y = r[k]["aug%d" % step]
            m, _ = _check(raw[lo:hi], lens[lo:hi], y, step + (k << 24), p, True)         # this rank's key: step + (rank << 24)
            assert m.any()
            shards.append(y)
        # rows 0, 1 of the two ranks hold different utterances AND draw different masks
        assert not np.array_equal(_ref_mask(step, lens[2:4], raw.shape[1], raw.shape[2], p),
                                  _ref_mask(step + (1 << 24), lens[2:4], raw.shape[1], raw.shape[2], p))
        rows = np.concatenate([y.reshape(-1, y.shape[2]) for y in shards]).astype(np.float64)
        want = rows.mean(axis=0)
        got = r[0]["mean%d" % step]
        assert np.array_equal(got, r[1]["mean%d" % step])
        tol = 2.0 ** -22 * np.abs(rows).max()
        assert np.abs(got - want).max() <= tol, (np.abs(got - want).max(), tol)
        # ... which the moments of the RAW batch would miss by far
        assert np.abs(raw.reshape(-1, raw.shape[2]).astype(np.float64).mean(axis=0) - want)[:raw.shape[2]].max() > 100 * tol

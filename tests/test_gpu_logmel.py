"""GPU tests of audio_processing='wav' (csrc/audio_frontend.hip): the kernel against the fp64 restatement of the dataset writer's
pipeline (tests/ref_logmel.py), and the engine fed with waveforms against the same engine fed with the restatement's features.

Limits of the kernel comparison.  log() amplifies fp32 rounding wherever a mel value is near the 1e-6 offset, so no fixed limit fits
every signal.  Each limit is taken from the signal itself: the restatement is evaluated in fp32 on the CPU, its largest deviation from
the fp64 evaluation is measured, and the kernel may deviate four times as far (the GPU's butterfly order and logf differ from the CPU's
by a few ulp).  Broadband signals are compared in the log domain; tonal and silent ones, whose empty bands sit at the offset, in the
linear domain: |exp(out) - exp(ref)| relative to the largest mel value of the entry's frame.  (Deviations measured on an MI355X:
DESIGN.md, the audio front-end's section.)"""
import dataclasses
import os

import numpy as np
import pytest
import torch

import ref_logmel as R

pytestmark = pytest.mark.gpu

TRANSFORMATIONS = ["logmel_stack_w8s3", "logmel_stack_w3s3", "logmel"]


def _broadband(kind, n, rng):
    t = np.arange(n) / 16000.0
    if kind == "gauss":
        return rng.standard_normal(n) * 0.1
    if kind == "int16":
        return np.round(rng.standard_normal(n) * 3000.0).clip(-32768, 32767) / 32768.0
    assert kind == "chirp_noise"                    # a modulated chirp over a noise floor of 0.003
    return 0.3 * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) * np.sin(2 * np.pi * (200.0 * t + 1500.0 * t * t)) + 0.003 * rng.standard_normal(n)


def _tonal(kind, n, rng):
    t = np.arange(n) / 16000.0
    if kind == "tone":
        return 0.5 * np.sin(2 * np.pi * 440.0 * t)
    assert kind == "chirp_silence"                  # a clean chirp between silences
    x = 0.4 * np.sin(2 * np.pi * (300.0 * t + 2000.0 * t * t))
    x[:n // 4] = 0.0
    x[3 * n // 4:] = 0.0
    return x


def _run_kernel(waves, transformation, M, pad_rows=0):
    """Kernel output [B, T, F] (T = rows of the canonical sample count + pad_rows), row counts, and the padded inputs."""
    from avsr_tf1_amd.audio_frontend import LogmelFrontend, LogmelSpec
    spec = LogmelSpec(transformation, M)
    N = spec.samples_for_rows(max(spec.rows(len(w)) for w in waves))
    wav = np.zeros((len(waves), N), np.float32)
    for i, w in enumerate(waves):
        wav[i, :min(N, len(w))] = w[:N]
    lens = np.array([min(N, len(w)) for w in waves], np.int32)
    T, F = spec.rows(N) + pad_rows, (spec.feat + 3) // 4 * 4
    out = torch.full((len(waves), T, F), float("nan"), device="cuda")
    out_len = torch.full((len(waves),), -1, dtype=torch.int32, device="cuda")
    LogmelFrontend(spec, "cuda").forward(torch.as_tensor(wav).cuda(), torch.as_tensor(lens).cuda(), out, out_len)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_len.cpu().numpy(), wav, lens, spec


def _compare(waves, transformation, M, domain, label):
    out, out_len, wav, lens, spec = _run_kernel(waves, transformation, M, pad_rows=2)
    assert np.isfinite(out).all()                                    # every element was written
    worst_cpu, worst_gpu = 0.0, 0.0
    for i in range(len(waves)):
        x32 = wav[i, :lens[i]]
        ref = R.logmel_features(x32.astype(np.float64), transformation, M)
        cpu = R.logmel_features(x32, transformation, M, dtype=np.float32)
        rows = ref.shape[0]
        assert out_len[i] == rows == spec.rows(len(waves[i]))
        got = out[i, :rows, :spec.feat].astype(np.float64)
        assert not out[i, rows:].any() and not out[i, :, spec.feat:].any()      # padded rows and padding columns: exactly zero
        if domain == "log":
            d_cpu, d_gpu = np.abs(cpu - ref).max(), np.abs(got - ref).max()
        else:
            peak = np.maximum(R.frame_peak_mel(x32.astype(np.float64), transformation, M), 1e-6)
            d_cpu = (np.abs(np.exp(cpu.astype(np.float64)) - np.exp(ref)) / peak).max()
            d_gpu = (np.abs(np.exp(got) - np.exp(ref)) / peak).max()
        worst_cpu, worst_gpu = max(worst_cpu, d_cpu), max(worst_gpu, d_gpu)
    limit = 4.0 * worst_cpu
    print("logmel %s %s M=%d (%s domain): fp32 CPU restatement deviates %.3e, limit %.3e, kernel deviates %.3e"
          % (label, transformation, M, domain, worst_cpu, limit, worst_gpu))
    assert worst_gpu <= limit, (label, transformation, M, domain, worst_gpu, limit)


@pytest.mark.parametrize("M", [30, 80, 13])
@pytest.mark.parametrize("transformation", TRANSFORMATIONS)
def test_kernel_against_the_restatement_broadband(transformation, M):
    from avsr_tf1_amd.audio_frontend import LogmelSpec
    rng = np.random.default_rng(11)
    one_row = LogmelSpec(transformation, M).samples_for_rows(1)          # an utterance of exactly one output row, and one sample short of two
    lens = [one_row, 16000, 7001, 23456, LogmelSpec(transformation, M).samples_for_rows(2) - 1]
    for kind in ("gauss", "int16", "chirp_noise"):
        _compare([_broadband(kind, n, rng).astype(np.float32) for n in lens], transformation, M, "log", kind)


@pytest.mark.parametrize("M", [30, 80, 13])
@pytest.mark.parametrize("transformation", TRANSFORMATIONS)
def test_kernel_against_the_restatement_tonal_and_silent(transformation, M):
    rng = np.random.default_rng(12)
    for kind in ("tone", "chirp_silence"):
        _compare([_tonal(kind, n, rng).astype(np.float32) for n in (16000, 9000, 30000)], transformation, M, "linear", kind)


def test_kernel_at_the_benchmark_shape():
    rng = np.random.default_rng(13)
    n = 241040                                                           # 500 stacked rows
    lens = rng.integers(n // 2, n + 1, size=64)
    lens[0] = n
    _compare([_broadband("gauss", int(k), rng).astype(np.float32) for k in lens], "logmel_stack_w8s3", 30, "log", "benchmark shape")


@pytest.mark.parametrize("transformation", TRANSFORMATIONS)
def test_silence_gives_the_log_offset_and_padding_is_zero(transformation):
    waves = [np.zeros(16000, np.float32), np.zeros(5000, np.float32)]
    out, out_len, _, _, spec = _run_kernel(waves, transformation, 30, pad_rows=3)
    want = np.float32(R.logmel_features(np.zeros(16000), transformation, 30)[0, 0])
    assert want == np.float32(np.log(1e-6))
    for i in range(2):
        rows = int(out_len[i])
        live = out[i, :rows, :spec.feat]
        ulps = np.abs(live.view(np.int32).astype(np.int64) - np.array(want).view(np.int32).astype(np.int64))
        assert rows == spec.rows(len(waves[i])) and ulps.max() <= 1, ulps.max()          # equal up to the last bit
        assert (out[i, rows:] == 0).all() and (out[i, :, spec.feat:] == 0).all()


def test_unsupported_configurations_are_refused_by_the_library():
    from avsr_tf1_amd import ops
    assert ops.logmel_supported(400, 512, 30, 8, 3) and ops.logmel_supported(500, 512, 128, 1, 1)
    assert not ops.logmel_supported(400, 1024, 30, 8, 3) and not ops.logmel_supported(400, 512, 129, 8, 3)
    assert not ops.logmel_supported(600, 512, 30, 8, 3) and not ops.logmel_supported(400, 512, 30, 3, 8)


# ---- the engine from waveforms against the engine from the restatement's features --------------------------------------------------
MODELS = {
    "c2_audio": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32), decoder_units=(32,),
                     embedding_size=16, warmup_steps=0),
    "av_align_lip_crops": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                               decoder_units=(32,), embedding_size=16, warmup_steps=0, video_processing="resnet_cnn",
                               cnn_filters=(8, 16, 32, 64), cnn_dense_units=16, video_feat=16),
}


def _configs(case, transformation="logmel_stack_w8s3", M=30, **over):
    from avsr_tf1_amd.config import ModelConfig
    window = R.TRANSFORMATIONS[transformation][0]
    kw = dict(MODELS[case], audio_feat=M * window)
    kw.update(over)
    feat = ModelConfig(**kw)
    wav = dataclasses.replace(feat, audio_processing="wav", audio_transformation=transformation, num_mel_bins=M)
    return feat, wav


def _batches(cfg, transformation, M, lens_rows, L=6, seed=21, Tv=5):
    """The same utterances as a waveform batch and as the feature batch the restatement makes of them (zero-padded alike)."""
    from avsr_tf1_amd.audio_frontend import LogmelSpec
    from avsr_tf1_amd.model import Batch
    spec = LogmelSpec(transformation, M)
    rng = np.random.default_rng(seed)
    B = len(lens_rows)
    lens = np.array([spec.samples_for_rows(r) + int(rng.integers(0, spec.frame_step * spec.stride)) for r in lens_rows])
    N = spec.samples_for_rows(max(lens_rows))
    lens = np.minimum(lens, N)
    wav = np.zeros((B, N), np.float32)
    for i, n in enumerate(lens):
        wav[i, :n] = _broadband("chirp_noise" if i % 2 else "gauss", int(n), rng)
    feats, flen = R.batch_features([wav[i, :lens[i]].astype(np.float64) for i in range(B)], transformation, M, T=max(lens_rows))
    assert list(flen) == list(lens_rows)
    lab = rng.integers(1, cfg.eos_id, size=(B, L)).astype(np.int32)
    ll = rng.integers(L // 2, L + 1, size=B).astype(np.int32)
    ll[0] = L
    for i in range(B):
        lab[i, ll[i] - 1] = cfg.eos_id
        lab[i, ll[i]:] = 0
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    common = dict(labels=t(lab, torch.int32), labels_len=t(ll, torch.int32))
    if cfg.video_units is not None:
        vl = rng.integers((Tv + 1) // 2, Tv + 1, size=B)
        vl[0] = Tv
        video = rng.random((B, Tv) + tuple(cfg.video_hw)).astype(np.float32)
        video *= (np.arange(Tv)[None, :] < vl[:, None]).reshape(B, Tv, 1, 1, 1)
        common.update(video=t(video, torch.float32), video_len=t(vl, torch.int32))
    bw = Batch(audio=t(wav, torch.float32), audio_len=t(lens, torch.int32), **common)
    bf = Batch(audio=t(feats, torch.float32), audio_len=t(flen, torch.int32), **common)
    return bw, bf


def _weights(cfg, seed=5):
    from avsr_tf1_amd import params as PR
    return PR.initialise(cfg, seed=seed)


@pytest.mark.parametrize("case,transformation,M", [("c2_audio", "logmel_stack_w8s3", 30), ("c2_audio", "logmel", 13),
                                                   ("av_align_lip_crops", "logmel_stack_w8s3", 30), ("av_align_lip_crops", "logmel_stack_w3s3", 30)])
def test_train_step_and_decodes_from_waveforms_equal_those_from_features(case, transformation, M):
    from avsr_tf1_amd.model import Seq2SeqModel
    cf, cw = _configs(case, transformation, M)
    W = _weights(cf)
    bw, bf = _batches(cf, transformation, M, [19, 12, 1, 16])
    res = {}
    for name, cfg, batch in (("features", cf, bf), ("wav", cw, bw)):
        m = Seq2SeqModel(cfg, weights=W)
        m.forward_train(batch)
        m.backward()
        m.apply_update()
        torch.cuda.synchronize()
        res[name] = dict(loss=float(m.loss.item()), gnorm=float(m.gnorm.item()), grads=m.export_tf_weights("grads"))
        m2 = Seq2SeqModel(cfg, weights=W)
        res[name]["greedy"] = m2.greedy_decode(batch, max_steps=12).cpu().numpy()
        res[name]["beam"] = m2.beam_search_decode(batch, beam_width=10, max_steps=12).cpu().numpy()
    a, b = res["features"], res["wav"]
    print("loss %.7f / %.7f, global norm %.7f / %.7f" % (a["loss"], b["loss"], a["gnorm"], b["gnorm"]))
    # the full-model tolerances of tests/test_gpu_model.py::test_train_step_parity: everything downstream of the features is unchanged code
    assert abs(a["loss"] - b["loss"]) < 1e-4
    assert abs(a["gnorm"] - b["gnorm"]) < 1e-4 * max(1.0, a["gnorm"])
    assert set(a["grads"]) == set(b["grads"])
    for k, g in a["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        err = np.abs(b["grads"][k] - g).max()
        assert err < 2e-4 * scale + 1e-6, (k, err, scale)
    assert a["greedy"].shape == b["greedy"].shape and (a["greedy"] == b["greedy"]).all()
    assert a["beam"].shape == b["beam"].shape and (a["beam"] == b["beam"]).all()


def test_graph_replay_equals_eager_steps_over_several_lengths():
    from avsr_tf1_amd.model import Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    cf, cw = _configs("c2_audio", use_dropout=True, sampling_probability=0.2)
    W = _weights(cf)
    batches = [_batches(cf, "logmel_stack_w8s3", 30, rows, seed=30 + i)[0] for i, rows in enumerate(([14, 9, 11], [22, 3, 20], [7, 7, 1], [30, 18, 25]))]
    out = {}
    for mode in ("eager", "graph"):
        m = Seq2SeqModel(cw, weights=W)
        t = DataParallelTrainer(m, None, use_graph=(mode == "graph"))
        trace = []
        for _ in range(4):                                              # every shape is seen four times: captured, then replayed
            for b in batches:
                loss, gnorm = t.train_step(b)
                trace.append((float(loss.item()), float(gnorm.item())))
        torch.cuda.synchronize()
        assert mode == "eager" or t.mode == "hipgraph"
        out[mode] = (trace, m.export_tf_weights("params"))
        del t, m
    assert out["eager"][0] == out["graph"][0]
    for k, v in out["eager"][1].items():
        assert (v == out["graph"][1][k]).all(), k


def _write_records(tmp_path, n=8, seed=1):
    from avsr_tf1_amd import io_utils as IO
    rng = np.random.default_rng(seed)
    unit_file = os.path.join(str(tmp_path), "character_list")
    open(unit_file, "w").write("\n".join(list("' abcdefghijklmnopqrstuvwxyz")) + "\n")
    arec, lrec = os.path.join(str(tmp_path), "wav.tfrecord"), os.path.join(str(tmp_path), "labels.tfrecord")
    with IO.TFRecordFileWriter(arec) as fa, IO.TFRecordFileWriter(lrec) as fl:
        for i in range(n):
            L = int(rng.integers(2, 5))
            lab = rng.integers(3, 10, size=L)
            seg = 4800                                                   # 0.3 s per symbol: a tone whose pitch is the symbol
            t = np.arange(seg) / 16000.0
            x = np.concatenate([0.3 * np.sin(2 * np.pi * (300.0 + 350.0 * int(c)) * t) for c in lab]) + 0.01 * rng.standard_normal(seg * L)
            fa.write(IO.make_feature_example("utt%02d" % i, x.astype(np.float32)[:, None]))
            fl.write(IO.make_label_example("utt%02d" % i, lab.tolist(), "character"))
    return unit_file, arec, lrec


def test_avsr_train_save_restore_and_evaluate_from_a_waveform_record(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    monkeypatch.chdir(tmp_path)
    unit_file, arec, lrec = _write_records(tmp_path)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="wav", audio_train_record=arec, audio_test_record=arec,
              labels_train_record=lrec, labels_test_record=lrec, batch_size=(4, 4), encoder_units_per_layer=((32,), (32, 32)),
              decoder_units_per_layer=(32,), embedding_size=16, warmup_steps=0, learning_rate=0.01, shuffle_seed=0, architecture="unimodal")
    exp = avsr.AVSR(**kw)
    assert exp._cfg.audio_processing == "wav" and exp._cfg.audio_feat == 240
    exp.train(logfile="logs/wav", num_epochs=3)                          # two epochs
    losses = [float(l.split()[-1]) for l in open("logs/wav").read().splitlines() if l.startswith("Average")]
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[1] < losses[0]
    ckpt = exp.save("checkpoints/wav/checkpoint.ckp-2")
    meta = np.load(ckpt + ".npz")["meta:audio_frontend"]
    assert [str(v) for v in meta] == ["logmel_stack_w8s3", "30", "16000"]
    first = exp.evaluate(ckpt, epoch=2)
    pred1 = open("predictions/wav/predicted_epoch_2.mlf").read()
    assert set(first) == {"character", "word"} and np.isfinite(first["character"])
    exp2 = avsr.AVSR(**kw)                                               # a fresh object: restores inside evaluate
    second = exp2.evaluate(ckpt, epoch=3)
    assert second == first and open("predictions/wav/predicted_epoch_3.mlf").read() == pred1
    with pytest.raises(ValueError, match="audio front-end"):
        avsr.AVSR(**dict(kw, audio_transformation="logmel_stack_w3s3")).restore(ckpt)


def _setup_dp():
    cf, cw = _configs("av_align_lip_crops")
    W = _weights(cf, seed=7)
    return cw, W


def _worker_dp(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["AVSR_PERSISTENT_RNN"] = "0"
    import torch.distributed as dist
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cw, W = _setup_dp()
    model = Seq2SeqModel(cw, weights=W)
    trainer = DataParallelTrainer(model, dist, use_graph=True)
    full, _ = _batches(cw, "logmel_stack_w8s3", 30, [15, 9, 12, 6], seed=41)
    sl = slice(2 * rank, 2 * rank + 2)
    batch = Batch(**{f.name: (None if getattr(full, f.name) is None else getattr(full, f.name)[sl].contiguous()) for f in dataclasses.fields(Batch)})
    for _ in range(3):
        trainer.train_step(batch)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), mode=np.array(trainer.mode), **model.export_tf_weights("params"))
    dist.destroy_process_group()


def test_two_ranks_with_the_waveform_front_end(tmp_path):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker_dp, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert str(r0["mode"]).startswith("hipgraph")
    W0 = _setup_dp()[1]
    names = [k for k in r0.files if k != "mode"]
    for k in names:
        assert np.array_equal(r0[k], r1[k]), k                       # replicas stay bit-identical, moving statistics included
    assert not np.array_equal(r0["audio/bn/moving_mean"], W0["audio/bn/moving_mean"])

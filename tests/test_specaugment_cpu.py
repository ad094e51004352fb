"""SpecAugment, the parts that need no GPU: properties of the numpy restatement of the rule (tests/ref_specaugment.py), the period of the
frequency axis, every host-side refusal (config, AVSR, LM, the C entry points) and the RNG stream constants."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ref_specaugment as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _streams():
    from avsr_tf1_amd import config as CF
    return CF.SPEC_STREAM_AUDIO_FREQ, CF.SPEC_STREAM_AUDIO_TIME, CF.SPEC_STREAM_VIDEO_TIME


def test_restatement_hash_is_the_oracles():
    from oracle import avsr_oracle as O
    rng = np.random.default_rng(0)
    for seed, stream, idx in rng.integers(0, 2 ** 32, size=(200, 3)):
        got = O.hash_u32(np.uint32(seed), np.uint32(stream), np.asarray([idx], np.uint32))
        assert int(np.asarray(got).reshape(-1)[0]) == R.hash_u32(int(seed), int(stream), int(idx))


def test_masks_lie_inside_their_axis_and_within_their_caps():
    sf, st, sv = _streams()
    T = 40
    seen_full, seen_nonempty = False, 0
    for seed in range(300):
        for b, n in enumerate((0, 1, 5, 17, T)):
            for width, ratio in ((7, 0.2), (40, 1.0), (3, 0.5), (0, 1.0), (9, 0.0)):
                for t0, w in R.time_masks(seed, st, b, n, 3, width, ratio):
                    assert 0 <= w <= min(width, (n * R.ratio_q16(ratio)) >> 16) and 0 <= t0 and t0 + w <= n
                    seen_nonempty += w > 0
                    seen_full |= (w == n and n > 1)
            for P, width in ((4, 2), (30, 7), (5, 9), (1, 1)):
                for f0, w in R.freq_masks(seed, sf, b, P, 3, width):
                    assert 0 <= w <= min(width, P) and 0 <= f0 and f0 + w <= P
    assert seen_nonempty > 1000 and seen_full           # (ratio 1 and a wide cap: a span may cover a whole utterance)


def test_lengths_zero_one_and_full_work():
    sf, st, _ = _streams()
    T, F = 9, 8
    for seed in range(50):
        m = R.mask(seed, [0, 1, T, T + 5, -3], T, F, st, 2, 4, 1.0, sf, 2, 3, 4)
        assert not m[0].any() and not m[4].any() and not m[1, 1:].any()
        x = np.random.default_rng(seed).standard_normal((5, T, F)).astype(np.float32)
        y, mean = R.apply(x, [0, 1, T, T + 5, -3], F + 4, m, "mean")
        assert not y[0].any() and not y[4].any() and not y[:, :, F:].any() and not y[1, 1:].any()
        assert (y[1, 0, :F] == x[1, 0]).all()            # one row: its mean is the row itself
        assert (mean[2] == x[2].astype(np.float64).mean(0)).all()
        z, _ = R.apply(x, [0, 1, T, T + 5, -3], F, m, "zero")
        assert (z[2][m[2]] == 0).all() and (z[2][~m[2]] == x[2][~m[2]]).all()


def test_draws_repeat_for_equal_keys_and_differ_between_rows_seeds_and_streams():
    sf, st, sv = _streams()
    d = lambda seed, stream, b: tuple(R.time_masks(seed, stream, b, 1000, 4, 1000, 1.0))
    assert d(7, st, 3) == d(7, st, 3)
    keys = [(seed, stream, b) for seed in range(20) for stream in (sf, st, sv) for b in range(8)]
    draws = [d(*k) for k in keys]
    assert len(set(draws)) == len(draws)                 # 4 x 2 draws below 1000 each: a repeat would be a structural collision
    # the same row on two data-parallel ranks (seed = step + (rank << 24))
    assert d(5, st, 0) != d(5 + (1 << 24), st, 0)


def test_a_band_hits_the_same_bin_of_every_stacked_frame():
    sf, st, _ = _streams()
    P, stack, T = 30, 8, 6
    hit = 0
    for seed in range(100):
        m = R.mask(seed, [T], T, P * stack, st, 0, 0, 1.0, sf, 2, 7, P)
        cols = m[0, 0]
        assert (m[0] == cols[None, :]).all()             # bands only: every valid row alike
        per_frame = cols.reshape(stack, P)
        assert (per_frame == per_frame[0][None, :]).all()
        bins = set(np.nonzero(per_frame[0])[0])
        want = set()
        for f0, w in R.freq_masks(seed, sf, 0, P, 2, 7):
            want |= set(range(f0, f0 + w))
        assert bins == want
        hit += bool(bins)
    assert hit > 50


def test_stream_constants_collide_with_no_dropout_or_sampling_stream():
    from avsr_tf1_amd import config as CF, _lib
    used = set()
    for s in ("video", "audio"):
        for d in ("fw", "bw"):
            for l in range(_lib.MAX_LAYERS + 1):         # (+ 1: the attentive top layer's consumer stream)
                used |= {CF.encoder_cell_id(s, d, l) * 4 + k for k in range(4)}
    for j in range(_lib.MAX_DEC_EXTRA + 1):
        used |= {(CF.CELL_ID_DECODER + j) * 4 + k for k in range(4)}
    spec = _streams()
    assert len(set(spec)) == 3 and not set(spec) & used and min(spec) > max(used)
    text = open(os.path.join(ROOT, "avsr-tf1_amd", "csrc", "common.h")).read()
    names = ("RNG_STREAM_SPEC_AUDIO_FREQ", "RNG_STREAM_SPEC_AUDIO_TIME", "RNG_STREAM_SPEC_VIDEO_TIME")
    assert tuple(int(re.search(r"#define %s (\d+)u" % n, text).group(1)) for n in names) == spec


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    for sym in ("avsr_spec_augment", "avsr_spec_augment_supported", "avsr_spec_augment_ws_floats"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
    assert lib.avsr_sizeof(b"avsr_spec_augment_args") == C.sizeof(_lib.SpecAugmentArgs)
    sup = lib.avsr_spec_augment_supported
    assert sup(64, 500, 240, 2, 2) == 1 and sup(64, 75, 3888, 0, 1) == 1 and sup(1, 65535, 4, 8, 8) == 1
    assert sup(1, 65536, 4, 1, 1) == 0                   # T: the n * ratio_q16 product
    assert sup(4, 10, 8, 9, 0) == 0 and sup(4, 10, 8, 0, 9) == 0
    assert sup(64, 65535, 512, 1, 1) == 1 and sup(64, 65535, 516, 1, 1) == 0 and sup(64, 32768, 1024, 1, 1) == 0 and sup(64, 32767, 1024, 1, 1) == 1   # B*T*F < 2^31
    assert sup(0, 10, 8, 1, 1) == 0 and sup(4, 0, 8, 1, 1) == 0 and sup(4, 10, 0, 1, 1) == 0 and sup(4, 10, 8, -1, 1) == 0
    wsf = lib.avsr_spec_augment_ws_floats
    assert wsf(0, 10, 8) == 0 and wsf(3, 17, 12) >= 3 * 12 * 2 and wsf(64, 500, 240) >= 64 * 240 * 2
    p = 64

    def args(**over):
        a = _lib.SpecAugmentArgs(B=3, T=17, F_in=12, F=12, freq_masks=2, freq_width=2, freq_bins=4, time_masks=2, time_width=5,
                                 ratio_q16=65536, video=0, mean_fill=1, ld=12, x=p, len=p, seed=p, y=2 * p, ws=p, ws_floats=wsf(3, 17, 12))
        for k, v in over.items():
            setattr(a, k, v)
        return a

    run = lambda a: lib.avsr_spec_augment(None if a is None else C.byref(a), None)
    assert run(None) == -1
    for n in ("x", "len", "seed", "y", "ws"):
        assert run(args(**{n: None})) == -1, n
    assert run(args(y=p)) == -1                                           # never in place: the batch is the captured graph's input
    assert run(args(F=8)) == -1 and run(args(ld=11)) == -1 and run(args(F_in=0)) == -1
    assert run(args(ratio_q16=65537)) == -1 and run(args(ratio_q16=-1)) == -1 and run(args(freq_width=-1)) == -1
    assert run(args(freq_bins=0)) == -1 and run(args(mean_fill=2)) == -1 and run(args(video=1)) == -1   # video: time masks only
    assert run(args(ws_floats=wsf(3, 17, 12) - 1)) == -1 and run(args(ws=68)) == -1
    assert run(args(time_masks=9)) == -3 and run(args(freq_masks=9)) == -3 and run(args(T=65536)) == -3
    assert run(args(T=65536, x=None)) == -1                               # an argument error comes first


def test_config_fields_and_validation():
    from avsr_tf1_amd.config import ModelConfig, spec_augment_fields
    assert ModelConfig().spec_augment_args("audio") is None and spec_augment_fields(None) == {}
    f = spec_augment_fields(dict(freq_masks=2, freq_width=7, time_masks=2, time_width=40, time_ratio=0.2, video_time_masks=1,
                                 video_time_width=10, video_time_ratio=0.2, freq_bins=None, mask_value="mean"))
    cfg = ModelConfig(architecture="bimodal", video_units=(16,), audio_units=(16,), audio_feat=240, video_feat=12, **f)
    cfg.validate()
    e = cfg.engine()
    e.validate()
    assert e.spec_freq_bins == 240
    a, v = e.spec_augment_args("audio"), e.spec_augment_args("video")
    assert a == dict(video=False, time_masks=2, time_width=40, ratio_q16=13107, freq_masks=2, freq_width=7, freq_bins=240, mean_fill=True)
    assert v == dict(video=True, time_masks=1, time_width=10, ratio_q16=13107, mean_fill=True)
    # all counts 0, or masks that are empty by construction: nothing to launch
    for off in (dict(), dict(spec_freq_width=7, spec_time_width=9), dict(spec_time_masks=2), dict(spec_time_masks=2, spec_time_width=4, spec_time_ratio=0.0)):
        assert ModelConfig(**off).spec_augment_args("audio") is None
    assert ModelConfig(spec_time_masks=1, spec_time_width=3).spec_augment_args("video") is None       # no video stream
    # the period: the reference's width, settled before the engine pads it
    c = ModelConfig(audio_feat=10, spec_freq_masks=1, spec_freq_width=2, spec_freq_bins=5)
    c.validate(), c.engine().validate()
    assert c.engine().spec_freq_bins == 5 and c.engine().audio_feat == 12
    w = ModelConfig(audio_processing="wav", audio_feat=240, spec_freq_masks=1, spec_freq_width=2)
    w.validate()
    assert w.engine().spec_freq_bins == 30
    for bad, key in ((dict(spec_freq_masks=-1), "spec_freq_masks"), (dict(spec_time_width=1.5), "spec_time_width"),
                     (dict(spec_time_masks=9), "spec_time_masks"), (dict(spec_video_time_masks=9, video_units=(8,)), "spec_video_time_masks"),
                     (dict(spec_time_ratio=1.5), "spec_time_ratio"), (dict(spec_video_time_ratio=-0.1), "spec_video_time_ratio"),
                     (dict(spec_mask_value="median"), "spec_mask_value"), (dict(spec_video_time_masks=1), "video stream"),
                     (dict(spec_freq_masks=1, audio_units=None, video_units=(8,)), "audio stream"),
                     (dict(audio_feat=240, spec_freq_bins=7 * 11), "spec_freq_bins"),
                     (dict(audio_processing="wav", audio_feat=240, spec_freq_bins=240), "spec_freq_bins")):
        with pytest.raises(ValueError, match=key):
            ModelConfig(**bad).validate()


def _write_records(tmp):
    from avsr_tf1_amd import io_utils as IO
    rng = np.random.default_rng(3)
    unit_file = os.path.join(str(tmp), "character_list")
    open(unit_file, "w").write("\n".join(list("' abcdefghijklmnopqrstuvwxyz")) + "\n")
    paths = {k: os.path.join(str(tmp), k + ".tfrecord") for k in ("audio", "video", "wav", "labels")}
    with IO.TFRecordFileWriter(paths["audio"]) as fa, IO.TFRecordFileWriter(paths["video"]) as fv, \
            IO.TFRecordFileWriter(paths["wav"]) as fw, IO.TFRecordFileWriter(paths["labels"]) as fl:
        for i in range(2):
            name = "spk/u%03d" % i
            fa.write(IO.make_feature_example(name, rng.standard_normal((9, 12)).astype(np.float32)))
            fv.write(IO.make_feature_example(name, rng.standard_normal((4, 8)).astype(np.float32)))
            fw.write(IO.make_feature_example(name, (rng.standard_normal((2000, 1)) * 0.05).astype(np.float32)))
            fl.write(IO.make_label_example(name, [1, 2, 3], "character"))
    return unit_file, paths


def _construct(monkeypatch, kw):
    """AVSR(**kw); without a GPU the engine (not the configuration) is replaced by a stub, so that the options are still resolved."""
    import avsr_tf1_amd as avsr
    if not torch.cuda.is_available():
        from avsr_tf1_amd import avsr as A

        class _NoEngine:
            def __init__(self, cfg, *a, **k):
                cfg.validate()
                cfg.engine().validate()
        monkeypatch.setattr(A, "Seq2SeqModel", _NoEngine)
        monkeypatch.setattr(A, "DataParallelTrainer", lambda *a, **k: None)
    return avsr.AVSR(**kw)


def _kw(unit_file, paths, audio="features", video=None, **extra):
    kw = dict(unit="character", unit_file=unit_file, labels_train_record=paths["labels"], audio_processing=audio, video_processing=video,
              encoder_units_per_layer=((16,), (16,)), decoder_units_per_layer=(16,), architecture="bimodal" if (audio and video) else "unimodal")
    if audio:
        kw["audio_train_record"] = paths["wav" if audio == "wav" else "audio"]
    if video:
        kw["video_train_record"] = paths["video"]
    kw.update(extra)
    return kw


def test_avsr_parses_the_keyword_and_refuses_on_the_host(tmp_path, monkeypatch):
    unit_file, paths = _write_records(tmp_path)
    exp = _construct(monkeypatch, _kw(unit_file, paths, video="features", spec_augment=dict(
        freq_masks=2, freq_width=2, time_masks=2, time_width=40, time_ratio=0.2, video_time_masks=1, video_time_width=10,
        video_time_ratio=0.2, freq_bins=4, mask_value="zero")))
    c = exp._cfg
    assert (c.spec_freq_masks, c.spec_freq_width, c.spec_freq_bins, c.spec_time_masks, c.spec_time_width, c.spec_time_ratio) == (2, 2, 4, 2, 40, 0.2)
    assert (c.spec_video_time_masks, c.spec_video_time_width, c.spec_video_time_ratio, c.spec_mask_value) == (1, 10, 0.2, "zero")
    off = _construct(monkeypatch, _kw(unit_file, paths))._cfg
    assert off.spec_augment_args("audio") is None and off == _construct(monkeypatch, _kw(unit_file, paths, spec_augment=None))._cfg
    assert _construct(monkeypatch, _kw(unit_file, paths, spec_augment={}))._cfg.spec_augment_args("audio") is None
    wav = _construct(monkeypatch, _kw(unit_file, paths, audio="wav", spec_augment=dict(freq_masks=1, freq_width=3)))._cfg
    assert wav.engine().spec_freq_bins == 30 and wav.spec_mask_value == "mean"
    assert _construct(monkeypatch, _kw(unit_file, paths, audio="wav", spec_augment=dict(freq_masks=1, freq_width=3, freq_bins=30)))
    refused = [
        (dict(spec_augment=dict(freq_mask=2)), "freq_mask"),                                  # unknown key
        (dict(spec_augment=[2, 7]), "dict"),
        (dict(spec_augment=dict(freq_masks=-1)), "freq_masks"),
        (dict(spec_augment=dict(time_width=2.5)), "time_width"),
        (dict(spec_augment=dict(time_masks=True)), "time_masks"),
        (dict(spec_augment=dict(time_masks=9, time_width=2)), "time_masks"),                  # the kernel's limit
        (dict(spec_augment=dict(freq_masks=9, freq_width=2)), "freq_masks"),
        (dict(spec_augment=dict(time_ratio=1.01)), "time_ratio"),
        (dict(spec_augment=dict(time_ratio=-0.5)), "time_ratio"),
        (dict(spec_augment=dict(video_time_masks=1, video_time_width=2)), "video_time_masks"),  # no video stream
        (dict(spec_augment=dict(video_time_ratio=0.5)), "video_time_ratio"),
        (dict(spec_augment=dict(freq_bins=5)), "freq_bins"),                                  # does not divide 12
        (dict(spec_augment=dict(freq_bins=0)), "freq_bins"),
        (dict(spec_augment=dict(mask_value="noise")), "mask_value"),
        (dict(audio="wav", spec_augment=dict(freq_masks=1, freq_width=3, freq_bins=240)), "freq_bins"),   # contradicts 'wav'
        (dict(audio=None, video="features", spec_augment=dict(time_masks=1, time_width=2)), "time_masks"),  # no audio stream
        (dict(audio=None, video="features", spec_augment=dict(freq_bins=4)), "freq_bins"),
    ]
    for extra, key in refused:
        with pytest.raises(ValueError, match=key):
            _construct(monkeypatch, _kw(unit_file, paths, **extra))
    assert _construct(monkeypatch, _kw(unit_file, paths, audio=None, video="features",
                                       spec_augment=dict(video_time_masks=1, video_time_width=2)))._cfg.spec_video_time_masks == 1


def test_the_language_model_refuses_the_keyword(tmp_path):
    import avsr_tf1_amd as avsr
    unit_file, paths = _write_records(tmp_path)
    with pytest.raises(ValueError, match="spec_augment"):
        avsr.LM(unit="character", unit_file=unit_file, labels_train_record=paths["labels"], spec_augment=dict(time_masks=1))


def test_experiment_passes_the_keyword_through(monkeypatch, tmp_path):
    from avsr_tf1_amd import experiment as X
    seen = []

    class _Fake:
        def __init__(self, **kw):
            seen.append(kw.get("spec_augment"))

        def train(self, **kw):
            pass
    monkeypatch.setattr(X, "AVSR", _Fake)
    monkeypatch.chdir(tmp_path)
    os.makedirs("logs")
    sa = dict(time_masks=1, time_width=5)
    X.run_experiment(audio_train_records=["a"], audio_test_records=["b"], iterations=[(1, 1)], learning_rates=[(1e-3, 1e-4)], spec_augment=sa)
    assert seen == [sa, sa]

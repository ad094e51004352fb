"""Lip-crop augmentation, the parts that need no GPU: properties of the numpy restatement of the rule (tests/ref_video_augment.py), every
host-side refusal (config, AVSR, LM, the C entry points) and the RNG stream constants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref_video_augment as R
from test_specaugment_cpu import _construct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q1 = 1 << 24


def _x(shape, seed=0):
    return np.random.default_rng(seed).random(shape).astype(np.float32)


def test_flip_alone_reverses_the_second_spatial_axis_of_valid_frames():
    x = _x((3, 4, 5, 7, 3))
    lens = [4, 2, 0]
    for seed in range(5):
        y = R.apply(x, lens, seed, q24=Q1)
        for b, n in enumerate(lens):
            assert np.array_equal(y[b, :n], x[b, :n, :, ::-1, :]) and not y[b, n:].any()
        assert np.array_equal(R.apply(x, lens, seed, q24=0)[0], x[0])              # flip = 0 never flips
    flips = [R.geometry(seed, b, R.flip_q24(0.5), 0)[0] for seed in range(40) for b in range(10)]
    assert 120 < sum(flips) < 280                                                 # about half of 400


def test_shift_alone_is_a_roll_away_from_the_edges_and_replicates_at_them():
    x = _x((6, 2, 9, 8, 2), 1)
    lens = [2] * 6
    S = 3
    seen = set()
    for seed in range(30):
        y = R.apply(x, lens, seed, S=S)
        for b in range(6):
            flip, dx, dy = R.geometry(seed, b, 0, S)
            assert not flip and -S <= dx <= S and -S <= dy <= S
            seen.add((dx, dy))
            rolled = np.roll(x[b], (dy, dx), axis=(1, 2))
            i0, i1, j0, j1 = max(dy, 0), 9 + min(dy, 0), max(dx, 0), 8 + min(dx, 0)
            assert np.array_equal(y[b][:, i0:i1, j0:j1], rolled[:, i0:i1, j0:j1])
            # the rim: the nearest row / column of the input, repeated
            for i in range(9):
                for j in range(8):
                    assert np.array_equal(y[b][:, i, j], x[b][:, min(max(i - dy, 0), 8), min(max(j - dx, 0), 7)])
    assert len({d[0] for d in seen}) == 2 * S + 1 and len({d[1] for d in seen}) == 2 * S + 1


def test_dx_moves_along_w_and_dy_along_h_on_a_non_square_frame():
    H, W = 4, 9
    x = np.zeros((1, 1, H, W, 1), np.float32)
    x[0, 0, 1, 4, 0] = 1.0
    for dx, dy in ((2, 0), (-3, 0), (0, 1), (0, -1), (4, 2)):
        y = R.gather(x[0], False, dx, dy)
        assert y.shape == x[0].shape and y.sum() == 1.0 and y[0, 1 + dy, 4 + dx, 0] == 1.0
    y = R.gather(x[0], True, 2, 0)                                                # the flip first, the shift second
    assert y[0, 1, (W - 1 - 4) + 2, 0] == 1.0


def test_no_photometric_value_is_a_bit_copy_and_zero_length_rows_are_zero():
    x = _x((3, 3, 6, 4, 4), 2) - 0.5
    x[0, 0, 0, 0, 0] = -0.0
    lens = [3, 0, -2]
    y = R.apply(x, lens, 9, q24=0, S=0)
    assert np.array_equal(y[0].view(np.uint32), x[0].view(np.uint32)) and not y[1].any() and not y[2].any()
    g = R.apply(x, lens, 9, q24=Q1, S=2)
    flip, dx, dy = R.geometry(9, 0, Q1, 2)
    assert np.array_equal(g[0].view(np.uint32), R.gather(x[0], flip, dx, dy).view(np.uint32)) and not g[1:].any()
    assert not R.channel_means(x, lens)[1:].any()


def test_photometric_draws_and_formula():
    x = _x((2, 3, 5, 5, 3), 3)
    lens = [3, 2]
    for seed in range(20):
        for b in range(2):
            cf, d = R.photometric(seed, b, 0.2, 0.1)
            assert cf.dtype == np.float32 and np.float32(0.8) <= cf <= np.float32(1.2) and abs(d) <= np.float32(0.1)
    y = R.apply(x, lens, 4, contrast=0.2, brightness=0.1)
    m = R.channel_means(x, lens)
    for b, n in enumerate(lens):
        cf, d = R.photometric(4, b, 0.2, 0.1)
        want = float(cf) * (x[b, :n].astype(np.float64) - m[b]) + m[b] + float(d)
        assert np.abs(y[b, :n] - want).max() < 1e-6 and not y[b, n:].any()
        # contrast about the utterance's own means: the channel means move by d alone
        assert np.abs(y[b, :n].astype(np.float64).mean(axis=(0, 1, 2)) - (m[b] + float(d))).max() < 1e-6
    yb = R.apply(x, lens, 4, brightness=0.1)
    assert np.array_equal(yb[0], x[0] + R.photometric(4, 0, 0.0, 0.1)[1])
    # draws are per utterance, and other keys (another step, another data-parallel rank) draw differently
    assert R.photometric(4, 0, 0.2, 0.1) != R.photometric(4, 1, 0.2, 0.1) and R.photometric(4, 0, 0.2, 0.1) != R.photometric(4 + (1 << 24), 0, 0.2, 0.1)


def test_stream_constants_follow_the_specaugment_ones():
    from avsr_tf1_amd import config as CF
    assert (CF.VIDEO_AUG_STREAM_GEOMETRY, CF.VIDEO_AUG_STREAM_PHOTOMETRIC) == (203, 204) == (R.GEOMETRY, R.PHOTOMETRIC)
    assert CF.VIDEO_AUG_STREAM_GEOMETRY == CF.SPEC_STREAM_VIDEO_TIME + 1
    text = open(os.path.join(ROOT, "avsr-tf1_amd", "csrc", "common.h")).read()
    names = ("RNG_STREAM_VIDEO_AUG_GEOMETRY", "RNG_STREAM_VIDEO_AUG_PHOTOMETRIC")
    assert tuple(int(re.search(r"#define %s (\d+)u" % n, text).group(1)) for n in names) == (203, 204)


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    assert lib.avsr_abi_version() == 2
    for sym in ("avsr_video_augment", "avsr_video_augment_supported", "avsr_video_augment_ws_floats"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
    assert lib.avsr_sizeof(b"avsr_video_augment_args") == C.sizeof(_lib.VideoAugmentArgs)
    sup = lib.avsr_video_augment_supported
    assert sup(64, 75, 36, 36, 3, 3) == 1 and sup(1, 65535, 5, 7, 1, 4) == 1 and sup(65535, 1, 6, 4, 4, 0) == 1
    assert sup(1, 65536, 5, 7, 1, 0) == 0 and sup(65536, 1, 5, 7, 1, 0) == 0 and sup(2, 2, 4, 4, 65, 0) == 0
    assert sup(2, 2, 5, 7, 1, 5) == 0 and sup(2, 2, 7, 5, 1, 5) == 0 and sup(2, 2, 5, 7, 1, -1) == 0      # max_shift < min(H, W)
    assert sup(64, 8192, 64, 64, 1, 0) == 0 and sup(64, 8191, 64, 64, 1, 0) == 1                          # fewer than 2^31 elements
    assert sup(1, 1, 2 ** 31 - 1, 2 ** 31 - 1, 64, 0) == 0
    assert sup(0, 2, 4, 4, 1, 0) == 0 and sup(2, 0, 4, 4, 1, 0) == 0 and sup(2, 2, 0, 4, 1, 0) == 0 and sup(2, 2, 4, 4, 0, 0) == 0
    wsf = lib.avsr_video_augment_ws_floats
    assert wsf(0, 5, 4, 4, 3) == 0 and wsf(4, 5, 36, 36, 3) == 4 * 2 * 3 + 4 * 3 and wsf(2, 40, 5, 7, 1) == 2 * 10 + 2
    p = 64

    def args(**over):
        a = _lib.VideoAugmentArgs(B=4, T=5, H=6, W=4, C=4, max_shift=1, flip_q24=1 << 23, pad_=0, contrast=0.2, brightness=0.2,
                                  x=p, len=p, seed=p, y=2 * p, ws=p, ws_floats=wsf(4, 5, 6, 4, 4))
        for k, v in over.items():
            setattr(a, k, v)
        return a

    run = lambda a: lib.avsr_video_augment(None if a is None else C.byref(a), None)
    assert run(None) == -1
    for n in ("x", "len", "seed", "y", "ws"):
        assert run(args(**{n: None})) == -1, n
    assert run(args(y=p)) == -1                                           # never in place: the batch is the captured graph's input
    assert run(args(flip_q24=-1)) == -1 and run(args(flip_q24=(1 << 24) + 1)) == -1
    assert run(args(contrast=1.0)) == -1 and run(args(contrast=-0.1)) == -1 and run(args(contrast=float("nan"))) == -1
    assert run(args(brightness=-1.0)) == -1 and run(args(brightness=float("inf"))) == -1 and run(args(brightness=float("nan"))) == -1
    assert run(args(ws_floats=wsf(4, 5, 6, 4, 4) - 1)) == -1 and run(args(ws=68)) == -1
    assert run(args(max_shift=4)) == -3 and run(args(T=65536)) == -3 and run(args(C=65)) == -3
    assert run(args(T=65536, x=None)) == -1                               # an argument error comes first


LIP = dict(architecture="unimodal", video_units=(16,), audio_units=None, video_processing="resnet_cnn", cnn_dense_units=16, video_feat=16)


def test_config_fields_and_validation():
    from avsr_tf1_amd.config import ModelConfig, video_augment_fields
    assert video_augment_fields(None) == {} and ModelConfig(**LIP).video_augment_args() is None
    f = video_augment_fields(dict(flip=0.5, max_shift=3, contrast=0.2, brightness=0.2))
    assert f == dict(vaug_flip_q24=1 << 23, vaug_max_shift=3, vaug_contrast=0.2, vaug_brightness=0.2)
    assert video_augment_fields(dict(flip=1))["vaug_flip_q24"] == 1 << 24 and video_augment_fields(dict(flip=0))["vaug_flip_q24"] == 0
    for proc in ("resnet_cnn", "3dconv_cnn"):
        cfg = ModelConfig(**dict(LIP, video_processing=proc), **f)
        cfg.validate()
        cfg.engine().validate()
        assert cfg.engine().video_augment_args() == dict(flip_q24=1 << 23, max_shift=3, contrast=0.2, brightness=0.2)
    # every value 0: nothing to launch -- and no pixels, nothing either
    assert ModelConfig(**LIP, **video_augment_fields({})).video_augment_args() is None
    assert ModelConfig(**LIP, **video_augment_fields(dict(flip=0, max_shift=0, contrast=0.0, brightness=0))).video_augment_args() is None
    assert ModelConfig(**LIP, vaug_max_shift=1).video_augment_args() == dict(flip_q24=0, max_shift=1, contrast=0.0, brightness=0.0)
    assert ModelConfig(vaug_max_shift=1).video_augment_args() is None
    for bad, key in ((dict(vaug_flip_q24=-1), "vaug_flip_q24"), (dict(vaug_flip_q24=(1 << 24) + 1), "vaug_flip_q24"),
                     (dict(vaug_flip_q24=0.5), "vaug_flip_q24"), (dict(vaug_max_shift=36), "vaug_max_shift"),
                     (dict(vaug_max_shift=-1), "vaug_max_shift"), (dict(vaug_max_shift=1.0), "vaug_max_shift"),
                     (dict(vaug_max_shift=5, video_hw=(36, 5, 3)), "vaug_max_shift"), (dict(vaug_contrast=1.0), "vaug_contrast"),
                     (dict(vaug_contrast=-0.1), "vaug_contrast"), (dict(vaug_brightness=-0.1), "vaug_brightness"),
                     (dict(vaug_brightness=float("inf")), "vaug_brightness"), (dict(vaug_brightness=float("nan")), "vaug_brightness")):
        with pytest.raises(ValueError, match=key):
            ModelConfig(**dict(LIP, **bad)).validate()
    for nopix in (dict(video_processing="features"), dict(video_units=None, audio_units=(16,))):
        with pytest.raises(ValueError, match="no pixels"):
            ModelConfig(**dict(LIP, vaug_max_shift=1, **nopix)).validate()


def _write_records(tmp):
    from avsr_tf1_amd import io_utils as IO
    rng = np.random.default_rng(3)
    unit_file = os.path.join(str(tmp), "character_list")
    open(unit_file, "w").write("\n".join(list("' abcdefghijklmnopqrstuvwxyz")) + "\n")
    paths = {k: os.path.join(str(tmp), k + ".tfrecord") for k in ("audio", "crops", "video", "labels")}
    with IO.TFRecordFileWriter(paths["audio"]) as fa, IO.TFRecordFileWriter(paths["crops"]) as fc, \
            IO.TFRecordFileWriter(paths["video"]) as fv, IO.TFRecordFileWriter(paths["labels"]) as fl:
        for i in range(2):
            name = "spk/u%03d" % i
            fa.write(IO.make_feature_example(name, rng.standard_normal((9, 12)).astype(np.float32)))
            fc.write(IO.make_video_example(name, rng.random((4, 12, 8, 3)).astype(np.float32)))
            fv.write(IO.make_feature_example(name, rng.standard_normal((4, 8)).astype(np.float32)))
            fl.write(IO.make_label_example(name, [1, 2, 3], "character"))
    return unit_file, paths


def _kw(unit_file, paths, video="resnet_cnn", audio=None, **extra):
    kw = dict(unit="character", unit_file=unit_file, labels_train_record=paths["labels"], audio_processing=audio, video_processing=video,
              encoder_units_per_layer=((16,), (16,)), decoder_units_per_layer=(16,), architecture="bimodal" if (audio and video) else "unimodal",
              cnn_dense_units=16)
    if audio:
        kw["audio_train_record"] = paths["audio"]
    if video:
        kw["video_train_record"] = paths["video" if video == "features" else "crops"]
    kw.update(extra)
    return kw


def test_avsr_parses_the_keyword_and_refuses_on_the_host(tmp_path, monkeypatch):
    unit_file, paths = _write_records(tmp_path)
    for proc in ("resnet_cnn", "3dconv_cnn"):
        c = _construct(monkeypatch, _kw(unit_file, paths, video=proc,
                                        video_augment=dict(flip=0.5, max_shift=3, contrast=0.2, brightness=0.2)))._cfg
        assert tuple(c.video_hw) == (8, 12, 3)                                         # the record's [width, height, channels]
        assert (c.vaug_flip_q24, c.vaug_max_shift, c.vaug_contrast, c.vaug_brightness) == (1 << 23, 3, 0.2, 0.2)
    off = _construct(monkeypatch, _kw(unit_file, paths))._cfg
    assert off.video_augment_args() is None and off == _construct(monkeypatch, _kw(unit_file, paths, video_augment=None))._cfg
    assert off == _construct(monkeypatch, _kw(unit_file, paths, video_augment={}))._cfg
    assert off == _construct(monkeypatch, _kw(unit_file, paths, video_augment=dict(flip=0, max_shift=0, contrast=0, brightness=0)))._cfg
    assert _construct(monkeypatch, _kw(unit_file, paths, video_augment=dict(max_shift=7)))._cfg.vaug_max_shift == 7   # < min(8, 12)
    refused = [
        (dict(video_augment=dict(flipp=0.5)), "flipp"),                                       # unknown key
        (dict(video_augment=[0.5, 3]), "dict"),
        (dict(video_augment=dict(flip=1.5)), "flip"),
        (dict(video_augment=dict(flip=-0.1)), "flip"),
        (dict(video_augment=dict(flip=True)), "flip"),
        (dict(video_augment=dict(flip="0.5")), "flip"),
        (dict(video_augment=dict(max_shift=8)), "max_shift"),                                 # min(H, W) = 8
        (dict(video_augment=dict(max_shift=-1)), "max_shift"),
        (dict(video_augment=dict(max_shift=2.0)), "max_shift"),
        (dict(video_augment=dict(max_shift=True)), "max_shift"),
        (dict(video_augment=dict(contrast=1.0)), "contrast"),
        (dict(video_augment=dict(contrast=-0.2)), "contrast"),
        (dict(video_augment=dict(contrast=False)), "contrast"),
        (dict(video_augment=dict(brightness=-0.2)), "brightness"),
        (dict(video_augment=dict(brightness=float("inf"))), "brightness"),
        (dict(video_augment=dict(brightness=float("nan"))), "brightness"),
        (dict(video_augment=dict(brightness=True)), "brightness"),
        (dict(video="features", video_augment=dict(flip=0.5)), "no pixels"),
        (dict(video="features", video_augment={}), "no pixels"),
        (dict(video=None, audio="features", video_augment=dict(flip=0.5)), "no pixels"),
    ]
    for extra, key in refused:
        with pytest.raises(ValueError, match="video_augment.*" + key):
            _construct(monkeypatch, _kw(unit_file, paths, **extra))


def test_the_language_model_refuses_the_keyword(tmp_path):
    import avsr_tf1_amd as avsr
    unit_file, paths = _write_records(tmp_path)
    with pytest.raises(ValueError, match="video_augment"):
        avsr.LM(unit="character", unit_file=unit_file, labels_train_record=paths["labels"], video_augment=dict(flip=0.5))


def test_the_limits_python_quotes_are_the_headers():
    """(the refusal at the first unsupported batch, which names them, needs an engine: tests/test_gpu_video_augment.py)"""
    from avsr_tf1_amd import _lib
    text = open(os.path.join(ROOT, "include", "avsr_hip.h")).read()
    assert int(re.search(r"#define AVSR_VIDEO_AUGMENT_MAX_T (\d+)", text).group(1)) == _lib.VIDEO_AUGMENT_MAX_T
    assert int(re.search(r"#define AVSR_VIDEO_AUGMENT_MAX_C (\d+)", text).group(1)) == _lib.VIDEO_AUGMENT_MAX_C

"""CPU tests of audio_processing='wav': the fp64 restatement of the dataset writer's log-mel pipeline (tests/ref_logmel.py) against
scipy.signal.stft and the mel formula, the engine's host tables and length arithmetic against the restatement, waveform TFRecords
through the input pipeline against the feature records made from them, and the public surface (AVSR keywords, refusals)."""
import math
import os

import numpy as np
import pytest
import torch

import ref_logmel as R


def _signal(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 0.1


def test_restatement_magnitudes_agree_with_scipy_stft():
    import scipy.signal
    x = _signal(16000, 1)
    mag = R.stft_magnitude(x)
    win = R.hann_periodic(400)
    _, _, Z = scipy.signal.stft(x, fs=16000, window=win, nperseg=400, noverlap=240, nfft=512, boundary=None, padded=False)
    ref = np.abs(Z).T * win.sum()                                      # scipy scales by 1 / sum(window)
    assert ref.shape == mag.shape == (98, 257)
    err = np.abs(mag - ref).max()
    print("restatement vs scipy.signal.stft: max |diff| = %.3e" % err)
    assert err < 1e-12


@pytest.mark.parametrize("M", [13, 30, 80])
def test_mel_matrix_is_one_triangle_per_filter(M):
    from avsr_tf1_amd.audio_frontend import mel_weight_matrix
    W = R.mel_matrix(M)
    assert W.shape == (257, M) and (W[0] == 0).all()                   # the DC row is zero
    for m in range(M):                                                 # rises to one peak, then falls
        col = W[:, m]
        nz = np.nonzero(col)[0]
        assert nz.size and (np.diff(nz) == 1).all()
        p = int(col.argmax())
        assert (np.diff(col[nz[0]:p + 1]) > 0).all() and (np.diff(col[p:nz[-1] + 1]) < 0).all()
        assert 0 < col.max() <= 1.0
    # a handful of entries from the formula by hand
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    lo, hi = mel(125.0), mel(7600.0)
    edge = lambda i: lo + (hi - lo) * i / (M + 1)
    for k, m in ((5, 0), (40, M // 3), (100, M // 2), (200, M - 2), (240, M - 1)):
        fm = mel(8000.0 * k / 256)
        want = max(0.0, min((fm - edge(m)) / (edge(m + 1) - edge(m)), (edge(m + 2) - fm) / (edge(m + 2) - edge(m + 1))))
        assert abs(W[k, m] - want) < 1e-12
    # the engine's own (vectorised) table code gives the same matrix
    assert np.abs(mel_weight_matrix(M, 257, 16000) - W).max() < 1e-12


@pytest.mark.parametrize("M", [13, 30, 80, 128])
def test_mel_rows_have_at_most_two_nonzeros_and_the_sparse_tables_rebuild_the_matrix(M):
    from avsr_tf1_amd.audio_frontend import LogmelSpec
    W = R.mel_matrix(M)
    assert ((W != 0).sum(axis=1) <= 2).all()
    t = LogmelSpec("logmel", M).tables()
    back = np.zeros_like(W)
    for m in range(M):
        lo, cnt, p = int(t["mel_lo"][m]), int(t["mel_cnt"][m]), int(t["mel_ptr"][m])
        assert 0 <= lo and lo + cnt <= 257 and p + cnt <= t["mel_w"].size
        back[lo:lo + cnt, m] = t["mel_w"][p:p + cnt]
    assert np.abs(back - W).max() < 1e-7                               # fp32 rounding of the fp64 weights
    empty = [m for m in range(M) if not W[:, m].any()]
    if M == 128:                                                       # as in TensorFlow: one filter narrower than the bin spacing
        assert len(empty) == 1 and int(t["mel_cnt"][empty[0]]) == 0
        x = _signal(2000, 3)
        assert np.all(R.logmel_features(x, "logmel", 128)[:, empty[0]] == np.log(1e-6))
    else:
        assert not empty


def test_length_arithmetic_at_the_boundaries():
    from avsr_tf1_amd.audio_frontend import LogmelSpec
    s8, s3, s1 = LogmelSpec("logmel_stack_w8s3"), LogmelSpec("logmel_stack_w3s3"), LogmelSpec("logmel")
    assert (s8.frame_length, s8.frame_step, s8.fft_length, s8.feat, s3.feat, s1.feat) == (400, 160, 512, 240, 90, 30)
    assert [s8.frames(n) for n in (399, 400, 559, 560)] == [0, 1, 1, 2]
    assert [s8.rows_of_frames(f) for f in (7, 8, 10, 11)] == [0, 1, 1, 2]
    assert [s3.rows_of_frames(f) for f in (2, 3, 5, 6)] == [0, 1, 1, 2]
    assert [s1.rows_of_frames(f) for f in (0, 1, 2)] == [0, 1, 2]
    for s, tr in ((s8, "logmel_stack_w8s3"), (s3, "logmel_stack_w3s3"), (s1, "logmel")):
        for n in (0, 399, 400, 559, 560, 1519, 1520, 1999, 2000, 16000, 48321):
            assert s.frames(n) == R.num_frames(n) and s.rows(n) == R.num_rows(n, tr)
            assert s.rows(n) == R.logmel_features(np.zeros(n), tr).shape[0]
        for rows in (1, 2, 45, 500):                                   # the canonical padded sample count: the fewest samples of `rows` rows
            n = s.samples_for_rows(rows)
            assert s.rows(n) == rows and s.rows(n - 1) == rows - 1
    assert s8.samples_for_rows(1) == 1520 and s8.samples_for_rows(500) == 241040


def test_host_tables_are_the_restatements():
    from avsr_tf1_amd.audio_frontend import LogmelSpec
    t = LogmelSpec().tables()
    assert np.abs(t["hann"] - R.hann_periodic(400)).max() < 1e-7
    k = np.arange(512)
    assert np.abs(t["twiddle"][:, 0] - np.cos(2 * np.pi * k / 512)).max() < 1e-7
    assert np.abs(t["twiddle"][:, 1] + np.sin(2 * np.pi * k / 512)).max() < 1e-7


def _write_wav_dataset(tmp, n=23, seed=5, short=None):
    from avsr_tf1_amd import io_utils as IO
    rng = np.random.default_rng(seed)
    unit_file = os.path.join(str(tmp), "character_list")
    open(unit_file, "w").write("\n".join(list("' abcdefghijklmnopqrstuvwxyz")) + "\n")
    ud = IO.create_unit_dict(unit_file)
    w, f, l = (os.path.join(str(tmp), x) for x in ("wav.tfrecord", "feat.tfrecord", "lab.tfrecord"))
    waves = {}
    with IO.TFRecordFileWriter(w) as fw, IO.TFRecordFileWriter(f) as ff, IO.TFRecordFileWriter(l) as fl:
        for i in range(n):
            ns = int(rng.integers(1520, 120000)) if i != short else 1519
            x = (rng.standard_normal(ns) * 0.05).astype(np.float32)
            name = "spk/u%03d" % i
            waves[name] = x
            fw.write(IO.make_feature_example(name, x[:, None]))
            if i != short:
                ff.write(IO.make_feature_example(name, R.logmel_features(x.astype(np.float64)).astype(np.float32)))
            fl.write(IO.make_label_example(name, [int(v) for v in rng.integers(1, 27, size=int(rng.integers(2, 9)))], "character"))
    return w, f, l, ud, unit_file, waves


@pytest.mark.parametrize("native", [True, False])
def test_waveform_records_batch_like_the_feature_records_made_from_them(tmp_path, monkeypatch, native):
    from avsr_tf1_amd import io_utils as IO, _io_native
    from avsr_tf1_amd.audio_frontend import LogmelSpec
    if not native:
        monkeypatch.setattr(_io_native, "load", lambda: None)
    w, f, l, ud, _, waves = _write_wav_dataset(tmp_path)
    assert IO._get_input_shape_from_record(w) == ([1], {"stream": "feature"})
    spec = LogmelSpec()
    for shuffle in (False, True):
        kw = dict(batch_size=4, shuffle=shuffle, bucket_width=45, seed=11)
        bw = list(IO.make_iterator_from_one_record(w, l, ud, audio_frontend=spec, **kw))
        bf = list(IO.make_iterator_from_one_record(f, l, ud, **kw))
        assert len(bw) == len(bf) > 3
        shapes = set()
        for a, b in zip(bw, bf):
            assert [bytes(x) for x in a.inputs_filenames] == [bytes(x) for x in b.inputs_filenames]        # same batches, same order
            assert (a.labels == b.labels).all() and (a.labels_length == b.labels_length).all()
            T = b.inputs.shape[1]
            assert a.inputs.ndim == 2 and a.inputs.dtype == np.float32
            assert a.inputs.shape == (b.inputs.shape[0], spec.samples_for_rows(T))                        # padded size: a function of T alone
            assert [spec.rows(int(n)) for n in a.inputs_length] == [int(t) for t in b.inputs_length]
            for i, name in enumerate(a.inputs_filenames):
                x, n = waves[bytes(name).decode()], int(a.inputs_length[i])
                assert n == min(len(x), a.inputs.shape[1]) and (a.inputs[i, :n] == x[:n]).all() and not a.inputs[i, n:].any()
            shapes.add(a.inputs.shape[1])
        assert len(shapes) == len({b.inputs.shape[1] for b in bf})


def test_an_utterance_too_short_for_one_row_is_an_error_that_names_the_file(tmp_path):
    from avsr_tf1_amd import io_utils as IO
    from avsr_tf1_amd.audio_frontend import LogmelSpec
    w, _, l, ud, _, _ = _write_wav_dataset(tmp_path, n=6, short=4)
    with pytest.raises(ValueError, match="spk/u004"):
        list(IO.make_iterator_from_one_record(w, l, ud, batch_size=4, bucket_width=45, audio_frontend=LogmelSpec()))


def _avsr_kwargs(tmp_path, **extra):
    w, _, l, _, unit_file, _ = _write_wav_dataset(tmp_path, n=3)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="wav", audio_train_record=w, labels_train_record=l,
              encoder_units_per_layer=((16,), (16, 16)), decoder_units_per_layer=(16,))
    kw.update(extra)
    return kw


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


def test_avsr_constructs_from_a_waveform_record(tmp_path, monkeypatch):
    exp = _construct(monkeypatch, _avsr_kwargs(tmp_path))
    cfg = exp._cfg
    assert cfg.audio_processing == "wav" and cfg.audio_feat == 240
    assert (cfg.audio_transformation, cfg.num_mel_bins, cfg.sample_rate) == ("logmel_stack_w8s3", 30, 16000)


@pytest.mark.parametrize("extra,feat", [(dict(audio_transformation="logmel_stack_w3s3"), 90), (dict(audio_transformation="logmel", num_mel_bins=13), 13),
                                        (dict(num_mel_bins=80), 640), (dict(sample_rate=20000), 240)])
def test_avsr_front_end_keywords(tmp_path, monkeypatch, extra, feat):
    exp = _construct(monkeypatch, _avsr_kwargs(tmp_path, **extra))
    assert exp._cfg.audio_feat == feat and exp._cfg.engine().audio_feat == (feat + 3) // 4 * 4


@pytest.mark.parametrize("extra,exc", [(dict(audio_transformation="mfcc"), NotImplementedError), (dict(audio_transformation="mfcc_d_a"), NotImplementedError),
                                       (dict(audio_transformation="logmel_d_a"), NotImplementedError), (dict(sample_rate=8000), NotImplementedError),
                                       (dict(sample_rate=44100), NotImplementedError), (dict(sample_rate=12000), ValueError),
                                       (dict(num_mel_bins=0), ValueError), (dict(num_mel_bins=129), ValueError)])
def test_refused_transformations_and_sample_rates_raise_at_configuration(tmp_path, monkeypatch, extra, exc):
    from avsr_tf1_amd.config import ModelConfig
    with pytest.raises(exc):
        _construct(monkeypatch, _avsr_kwargs(tmp_path, **extra))
    with pytest.raises(exc):
        ModelConfig(audio_units=(16,), audio_processing="wav", audio_feat=240, **extra).validate()


def test_config_ties_audio_feat_to_the_front_end():
    from avsr_tf1_amd.config import ModelConfig
    ModelConfig(audio_units=(16,), audio_processing="wav", audio_feat=240).validate()
    with pytest.raises(ValueError, match="audio_feat"):
        ModelConfig(audio_units=(16,), audio_processing="wav", audio_feat=80).validate()
    assert ModelConfig().audio_processing == "features"


def test_a_feature_record_is_refused_as_a_waveform_record(tmp_path, monkeypatch):
    w, f, l, _, unit_file, _ = _write_wav_dataset(tmp_path, n=3)
    with pytest.raises(ValueError, match="input_size == 1"):
        _construct(monkeypatch, dict(unit="character", unit_file=unit_file, audio_processing="wav", audio_train_record=f, labels_train_record=l))


def test_wav_to_record_tool(tmp_path):
    import subprocess
    import sys
    import wave
    from avsr_tf1_amd import io_utils as IO
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(2)
    d = tmp_path / "wavs" / "spk"
    d.mkdir(parents=True)
    pcm = {}
    for name, rate in (("a", 16000), ("b", 16000)):
        x = rng.integers(-20000, 20000, size=3000 + len(pcm) * 500).astype("<i2")
        pcm["spk/" + name] = x
        with wave.open(str(d / (name + ".wav")), "wb") as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(rate)
            f.writeframes(x.tobytes())
    out = str(tmp_path / "out.tfrecord")
    tool = os.path.join(root, "tools", "wav_to_record.py")
    subprocess.check_call([sys.executable, tool, str(tmp_path / "wavs"), out])
    recs = [IO._parse_input(p, [1]) for p in IO.read_tfrecord(out)]
    assert [r[3].decode() for r in recs] == ["spk/a", "spk/b"]
    for x, _, T, name in recs:
        assert T == len(pcm[name.decode()]) and (x[:, 0] == pcm[name.decode()].astype(np.float32) / 32768.0).all()
    with wave.open(str(d / "c.wav"), "wb") as f:                       # another sample rate: refused, no resampling
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(8000)
        f.writeframes(pcm["spk/a"].tobytes())
    r = subprocess.run([sys.executable, tool, str(tmp_path / "wavs"), out], stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"8000" in r.stderr

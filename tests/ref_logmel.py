"""Restatement of the dataset writer's audio pipeline (avsr/audio.py compute_stfts / compute_log_mel_spectrograms,
avsr/dataset_writer.py _build_audio_engine / _stack_features) in numpy, independent of the engine's own table code.

`logmel_features(x, ...)` evaluates it in fp64 (the yardstick) or, with dtype=np.float32, with every array and every operation in
fp32 (scipy.fft keeps single precision): the fp32 evaluation shows how far a correct single-precision implementation may sit from the
fp64 one on a given signal, which is where the GPU tests take their limits from.
"""
import math

import numpy as np

TRANSFORMATIONS = {"logmel_stack_w8s3": (8, 3), "logmel_stack_w3s3": (3, 3), "logmel": (1, 1)}


def geometry(sample_rate=16000):
    frame_length = int((sample_rate / 1000) * 25)
    frame_step = int((sample_rate / 1000) * 10)
    fft_length = 1
    while fft_length < frame_length:
        fft_length *= 2
    return frame_length, frame_step, fft_length


def num_frames(n, sample_rate=16000):
    fl, fs, _ = geometry(sample_rate)
    return 1 + (n - fl) // fs if n >= fl else 0


def num_rows(n, transformation="logmel_stack_w8s3", sample_rate=16000):
    window, stride = TRANSFORMATIONS[transformation]
    f = num_frames(n, sample_rate)
    return (f - window) // stride + 1 if f >= window else 0


def hann_periodic(n, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)).astype(dtype)


def stft_magnitude(x, sample_rate=16000, dtype=np.float64):
    """|rfft| of the Hann-windowed frames, [frames, fft_length // 2 + 1]."""
    import scipy.fft
    fl, fs, nfft = geometry(sample_rate)
    x = np.asarray(x, dtype)
    frames = num_frames(x.shape[0], sample_rate)
    if frames == 0:
        return np.zeros((0, nfft // 2 + 1), dtype)
    idx = fs * np.arange(frames)[:, None] + np.arange(fl)[None, :]
    fr = x[idx] * hann_periodic(fl, dtype)[None, :]
    assert fr.dtype == dtype
    spec = scipy.fft.rfft(fr, n=nfft, axis=-1)
    mag = np.abs(spec)
    assert mag.dtype == dtype
    return mag


def mel_matrix(num_mel_bins=30, num_bins=257, sample_rate=16000, lower=125.0, upper=7600.0):
    """tf.contrib.signal.linear_to_mel_weight_matrix, written out entry by entry in fp64."""
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    lo, hi = mel(lower), mel(upper)
    edges = [lo + (hi - lo) * i / (num_mel_bins + 1) for i in range(num_mel_bins + 2)]
    W = np.zeros((num_bins, num_mel_bins), np.float64)
    for k in range(1, num_bins):                                     # the DC bin is dropped: row 0 stays zero
        fm = mel((sample_rate / 2.0) * k / (num_bins - 1))
        for m in range(num_mel_bins):
            up = (fm - edges[m]) / (edges[m + 1] - edges[m])
            down = (edges[m + 2] - fm) / (edges[m + 2] - edges[m + 1])
            W[k, m] = max(0.0, min(up, down))
    return W


def stack_features(mat, window, stride):
    nrows = (mat.shape[0] - window) // stride + 1 if mat.shape[0] >= window else 0
    if nrows <= 0:
        return np.zeros((0, window * mat.shape[1]), mat.dtype)
    return mat[stride * np.arange(nrows)[:, None] + np.arange(window)].reshape(nrows, -1)


def logmel_frames(x, num_mel_bins=30, sample_rate=16000, dtype=np.float64):
    """(log-mel [frames, num_mel_bins], mel [frames, num_mel_bins])."""
    mag = stft_magnitude(x, sample_rate, dtype)
    W = mel_matrix(num_mel_bins, mag.shape[1], sample_rate).astype(dtype)
    mel = mag @ W
    out = np.log(mel + dtype(1e-6))
    assert out.dtype == dtype
    return out, mel


def logmel_features(x, transformation="logmel_stack_w8s3", num_mel_bins=30, sample_rate=16000, dtype=np.float64):
    window, stride = TRANSFORMATIONS[transformation]
    lm, _ = logmel_frames(x, num_mel_bins, sample_rate, dtype)
    return stack_features(lm, window, stride)


def frame_peak_mel(x, transformation="logmel_stack_w8s3", num_mel_bins=30, sample_rate=16000):
    """Per stacked feature entry, the largest mel value (fp64) of the frame the entry comes from: the scale of the linear-domain
    comparison |exp(out) - exp(ref)| / peak."""
    window, stride = TRANSFORMATIONS[transformation]
    _, mel = logmel_frames(x, num_mel_bins, sample_rate, np.float64)
    peak = np.repeat(mel.max(axis=1, keepdims=True), num_mel_bins, axis=1)
    return stack_features(peak, window, stride)


def batch_features(waves, transformation="logmel_stack_w8s3", num_mel_bins=30, sample_rate=16000, dtype=np.float64, T=None, F=None):
    """Zero-padded [B, T, F] features and [B] row counts of a list of waveforms, as the feature pipeline pads them."""
    feats = [logmel_features(w, transformation, num_mel_bins, sample_rate, dtype) for w in waves]
    T = max(f.shape[0] for f in feats) if T is None else T
    F = feats[0].shape[1] if F is None else F
    out = np.zeros((len(feats), T, F), dtype)
    for i, f in enumerate(feats):
        out[i, :f.shape[0], :f.shape[1]] = f
    return out, np.array([f.shape[0] for f in feats], np.int32)

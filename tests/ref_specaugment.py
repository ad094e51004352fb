"""SpecAugment on an encoder's input, restated in numpy from the rule of INTEGRATION.md section 8 (not from the kernel): every draw in
uint32 arithmetic, so it matches the device bit for bit; the 'mean' fill in fp64.

  h(i) = hash_u32(seed, STREAM, i)                                     (oracle/avsr_oracle.py, csrc/common.h)
  time mask k of utterance b, n = clamp(len[b], 0, T):  cap = min(time_width, (n * ratio_q16) >> 16), w = h((b*64 + k)*2) % (cap + 1),
                                                        t0 = h((b*64 + k)*2 + 1) % (n - w + 1); rows t0 <= t < t0 + w
  band k, period P:                                     cap = min(freq_width, P), w and f0 likewise with P for n; columns f0 <= c % P < f0 + w
  fill: 0, or the utterance's own column mean over its n rows of the unmasked input; rows >= n and padding columns are zero."""
import numpy as np

M32 = 0xFFFFFFFF


def hash_u32(seed, stream, idx):
    key = ((seed & M32) * 0x9E3779B9 + (stream & M32) * 0x85EBCA6B) & M32
    x = (idx ^ key) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def ratio_q16(ratio):
    return int(round(ratio * 65536.0))


def draw(seed, stream, b, k, span, width, limit=None):
    """(start, width) of mask k of utterance b over [0, span): width <= min(`width`, `limit`, span)."""
    cap = min(width, span if limit is None else limit)
    i = (((b * 64 + k) & M32) * 2) & M32
    w = hash_u32(seed, stream, i) % (cap + 1)
    a = hash_u32(seed, stream, (i + 1) & M32) % (span - w + 1)
    return a, w


def time_masks(seed, stream, b, n, count, width, ratio):
    lim = ((n * ratio_q16(ratio)) & M32) >> 16
    return [draw(seed, stream, b, k, n, width, lim) for k in range(count)]


def freq_masks(seed, stream, b, P, count, width):
    return [draw(seed, stream, b, k, P, width) for k in range(count)]


def mask(seed, lens, T, F_in, time_stream, n_time=0, time_width=0, time_ratio=1.0, freq_stream=None, n_freq=0, freq_width=0, freq_bins=None):
    """Boolean [B, T, F_in]: the union of every mask; nothing beyond an utterance's n rows."""
    B = len(lens)
    m = np.zeros((B, T, F_in), bool)
    P = freq_bins or F_in
    for b in range(B):
        n = int(min(max(int(lens[b]), 0), T))
        for t0, w in time_masks(seed, time_stream, b, n, n_time, time_width, time_ratio):
            m[b, t0:t0 + w, :] = True
        if n_freq:
            cm = np.arange(F_in) % P
            for f0, w in freq_masks(seed, freq_stream, b, P, n_freq, freq_width):
                m[b, :n, (cm >= f0) & (cm < f0 + w)] = True
        assert not m[b, n:].any()
    return m


def apply(x, lens, F, m, mask_value="mean"):
    """x [B, T, F_in] (any float dtype) -> (y [B, T, F] fp64 with the fill exact, mean [B, F_in] fp64)."""
    B, T, F_in = x.shape
    y = np.zeros((B, T, F), np.float64)
    mean = np.zeros((B, F_in), np.float64)
    for b in range(B):
        n = int(min(max(int(lens[b]), 0), T))
        if n:
            mean[b] = x[b, :n].astype(np.float64).mean(axis=0)
        fill = mean[b] if mask_value == "mean" else np.zeros(F_in)
        y[b, :n, :F_in] = np.where(m[b, :n], fill[None, :], x[b, :n].astype(np.float64))
    return y, mean

"""Lip-crop augmentation, restated in numpy from the rule of INTEGRATION.md section 8 (not from the kernel): every draw in uint32
arithmetic and the photometric part in np.float32 operations, each rounded on its own, so it matches the device bit for bit.

  h_s(i) = hash_u32(seed, s, i), s = 203 (geometry) | 204 (photometric); u(h) = (h >> 8) * 2^-24; per utterance b, n = clamp(len[b], 0, T)
  flip iff (h_203(4b) >> 8) < flip_q24;  dx = h_203(4b+1) % (2S+1) - S;  dy = h_203(4b+2) % (2S+1) - S
  frame t < n, output pixel (i, j, c):  x[t, clamp(i - dy, 0, H-1), flip ? W-1-jj : jj, c] with jj = clamp(j - dx, 0, W-1)
  cf = 1 + contrast * (2 u(h_204(2b)) - 1);  d = brightness * (2 u(h_204(2b+1)) - 1)
  contrast > 0: y = cf * (v - m_c) + (m_c + d), m_c the utterance's channel mean of the un-augmented input (0 when n = 0)
  contrast == 0 < brightness: y = v + d;  both 0: bit copies;  frames t >= n: zeros."""
import numpy as np

from ref_specaugment import M32, hash_u32

GEOMETRY, PHOTOMETRIC = 203, 204
f32 = np.float32


def flip_q24(flip):
    return int(round(flip * 16777216.0))


def clamp_len(n, T):
    return int(min(max(int(n), 0), T))


def geometry(seed, b, q24, S):
    """(flip, dx, dy) of utterance b."""
    i = (4 * b) & M32
    flip = (hash_u32(seed, GEOMETRY, i) >> 8) < q24
    dx = hash_u32(seed, GEOMETRY, (i + 1) & M32) % (2 * S + 1) - S
    dy = hash_u32(seed, GEOMETRY, (i + 2) & M32) % (2 * S + 1) - S
    return bool(flip), int(dx), int(dy)


def _pm1(h):
    u = f32(h >> 8) * f32(2.0 ** -24)
    return f32(2.0) * u + f32(-1.0)


def photometric(seed, b, contrast, brightness):
    """(cf, d) of utterance b, np.float32."""
    i = (2 * b) & M32
    cf = f32(1.0) + f32(contrast) * _pm1(hash_u32(seed, PHOTOMETRIC, i))
    d = f32(brightness) * _pm1(hash_u32(seed, PHOTOMETRIC, (i + 1) & M32))
    return f32(cf), f32(d)


def gather(frames, flip, dx, dy):
    """frames [..., H, W, C] -> the flipped, then shifted frames (edge replication)."""
    H, W = frames.shape[-3], frames.shape[-2]
    ii = np.clip(np.arange(H) - dy, 0, H - 1)
    jj = np.clip(np.arange(W) - dx, 0, W - 1)
    if flip:
        jj = W - 1 - jj
    return frames[..., ii, :, :][..., jj, :]


def channel_means(x, lens):
    """[B, C] fp64: the mean of every channel over an utterance's n valid frames and all pixels; 0 when n = 0."""
    B, T = x.shape[:2]
    m = np.zeros((B, x.shape[4]), np.float64)
    for b in range(B):
        n = clamp_len(lens[b], T)
        if n:
            m[b] = x[b, :n].astype(np.float64).mean(axis=(0, 1, 2))
    return m


def apply(x, lens, seed, q24=0, S=0, contrast=0.0, brightness=0.0, means=None):
    """x [B, T, H, W, C] float32 -> y float32 of the same shape.  means [B, C]: the channel means the contrast reads (float32 values;
    default: the fp64 means rounded once)."""
    assert x.dtype == np.float32 and x.ndim == 5
    B, T = x.shape[:2]
    y = np.zeros_like(x)
    if contrast > 0 and means is None:
        means = channel_means(x, lens)
    for b in range(B):
        n = clamp_len(lens[b], T)
        if not n:
            continue
        flip, dx, dy = geometry(seed, b, q24, S)
        v = gather(x[b, :n], flip, dx, dy)
        cf, d = photometric(seed, b, contrast, brightness)
        if contrast > 0:
            m = np.asarray(means[b]).astype(np.float32)
            t = (v - m).astype(np.float32)
            t = (cf * t).astype(np.float32)
            v = (t + (m + d).astype(np.float32)).astype(np.float32)
        elif brightness > 0:
            v = (v + d).astype(np.float32)
        y[b, :n] = v
    return y

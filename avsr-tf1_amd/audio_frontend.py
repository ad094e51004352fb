"""Waveform audio front-end (`audio_processing='wav'`): raw samples -> the dataset writer's log-mel features, on the GPU.

The reference's own 'wav' branch (avsr/avsr.py:719-724) calls `process_audio` without `need_logmel`, so its encoder would receive the
complex STFT with lengths still counted in samples: it cannot train.  What every shipped experiment trained on is the WRITER's pipeline
(avsr/audio.py:7-41 compute_stfts / compute_log_mel_spectrograms, avsr/dataset_writer.py:392-414 _build_audio_engine, :549-551
_stack_features, :371-380 transformations), and that is what this front-end computes inside the model:

  frames = 1 + (n - frame_length) // frame_step          25 ms frames, 10 ms step, periodic Hann, zero-padded to the next power of two
  |rfft| -> num_mel_bins HTK-mel triangles between 125 and 7600 Hz (tf.contrib.signal.linear_to_mel_weight_matrix) -> log(x + 1e-6)
  rows = (frames - window) // stride + 1                 `window` frames side by side, every `stride` frames

`LogmelSpec` is the host side: length arithmetic and the tables (window, twiddles, mel weights), all computed in fp64.  It needs numpy
only, so the input pipeline uses it without a GPU.  `LogmelFrontend` uploads the tables once and launches csrc/audio_frontend.hip
(avsr_logmel_fwd): one kernel, no host synchronisation -- it runs inside the captured train step.  Forward only: nothing trains here.
"""
import numpy as np

TRANSFORMATIONS = {"logmel_stack_w8s3": (8, 3), "logmel_stack_w3s3": (3, 3), "logmel": (1, 1)}
REFUSED_TRANSFORMATIONS = ("mfcc", "mfcc_d_a", "logmel_d_a")          # the writer's other transformations (dataset_writer.py:347-369)
MEL_LOWER_HZ, MEL_UPPER_HZ = 125.0, 7600.0
FRAME_MSEC, STEP_MSEC = 25, 10
LOG_OFFSET = 1e-6
KERNEL_FFT_LENGTH = 512                                                # avsr_logmel_supported
MAX_MEL_BINS = 128


def _hz_to_mel(f):
    return 1127.0 * np.log1p(np.asarray(f, np.float64) / 700.0)


def mel_weight_matrix(num_mel_bins, num_spectrogram_bins, sample_rate, lower_edge_hertz=MEL_LOWER_HZ, upper_edge_hertz=MEL_UPPER_HZ):
    """tf.contrib.signal.linear_to_mel_weight_matrix in fp64: [num_spectrogram_bins, num_mel_bins]; the DC row is zero."""
    nyquist = sample_rate / 2.0
    bins_hz = np.linspace(0.0, nyquist, num_spectrogram_bins)[1:]
    spec_mel = _hz_to_mel(bins_hz)[:, None]
    edges = np.linspace(_hz_to_mel(lower_edge_hertz), _hz_to_mel(upper_edge_hertz), num_mel_bins + 2)
    lower, center, upper = edges[None, :-2], edges[None, 1:-1], edges[None, 2:]
    lower_slopes = (spec_mel - lower) / (center - lower)
    upper_slopes = (upper - spec_mel) / (upper - center)
    w = np.maximum(0.0, np.minimum(lower_slopes, upper_slopes))
    return np.concatenate([np.zeros((1, num_mel_bins)), w], axis=0)


class LogmelSpec:
    """One configuration of the pipeline: lengths, feature width, fp64 tables.  Raises at construction for what is not built."""

    def __init__(self, transformation="logmel_stack_w8s3", num_mel_bins=30, sample_rate=16000):
        if transformation in REFUSED_TRANSFORMATIONS:
            raise NotImplementedError("audio_transformation=%r: MFCC and delta features are not built; the waveform front-end computes %s"
                                      % (transformation, ", ".join(sorted(TRANSFORMATIONS))))
        if transformation not in TRANSFORMATIONS:
            raise Exception("unsupported transformation")                                      # dataset_writer.py:383
        if int(num_mel_bins) != num_mel_bins or not 1 <= num_mel_bins <= MAX_MEL_BINS:
            raise ValueError("num_mel_bins must be an integer from 1 to %d" % MAX_MEL_BINS)
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError("sample_rate must be a positive integer")
        self.transformation, self.num_mel_bins, self.sample_rate = transformation, int(num_mel_bins), int(sample_rate)
        self.window, self.stride = TRANSFORMATIONS[transformation]
        self.frame_length = int((self.sample_rate / 1000) * FRAME_MSEC)                          # avsr/audio.py:8-9
        self.frame_step = int((self.sample_rate / 1000) * STEP_MSEC)
        self.fft_length = 1 << max(0, int(self.frame_length - 1).bit_length())                  # tf.contrib.signal.stft's default
        self.num_bins = self.fft_length // 2 + 1
        if self.fft_length != KERNEL_FFT_LENGTH or self.frame_step < 1:
            raise NotImplementedError("sample_rate=%d needs a %d-point FFT; the waveform front-end's kernel covers %d points "
                                      "(10241 to 20480 Hz)" % (self.sample_rate, self.fft_length, KERNEL_FFT_LENGTH))
        if MEL_UPPER_HZ > self.sample_rate / 2.0:
            raise ValueError("sample_rate=%d: the mel filters reach %g Hz, above the Nyquist frequency" % (self.sample_rate, MEL_UPPER_HZ))
        self.feat = self.num_mel_bins * self.window
        self._tables = None

    def key(self):
        return (self.transformation, self.num_mel_bins, self.sample_rate)

    # ---- length arithmetic ----
    def frames(self, n):
        n = int(n)
        return 1 + (n - self.frame_length) // self.frame_step if n >= self.frame_length else 0

    def rows_of_frames(self, frames):
        frames = int(frames)
        return (frames - self.window) // self.stride + 1 if frames >= self.window else 0

    def rows(self, n):
        """Feature rows of an utterance of n samples."""
        return self.rows_of_frames(self.frames(n))

    def samples_for_rows(self, rows):
        """The canonical padded sample count of a batch whose longest utterance has `rows` feature rows: the fewest samples that give
        exactly `rows` rows.  A function of the feature length alone, so waveform batches have as many distinct shapes as feature batches."""
        rows = int(rows)
        if rows < 1:
            raise ValueError("a batch needs at least one feature row")
        return ((rows - 1) * self.stride + self.window - 1) * self.frame_step + self.frame_length

    # ---- tables ----
    def hann(self):
        k = np.arange(self.frame_length, dtype=np.float64)
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / self.frame_length)                          # periodic (tf.contrib.signal.hann_window)

    def mel_matrix(self):
        return mel_weight_matrix(self.num_mel_bins, self.num_bins, self.sample_rate)

    def tables(self):
        """fp32 / int32 host arrays the kernel reads, rounded once from fp64: hann [frame_length], twiddle [fft_length, 2] =
        (cos, -sin)(2 pi k / fft_length), and the mel matrix by filter: the non-zero bins of filter m are mel_lo[m] .. mel_lo[m] +
        mel_cnt[m] - 1 with weights mel_w[mel_ptr[m] ...] (an empty filter has mel_cnt 0: its output is log(1e-6), as in TensorFlow)."""
        if self._tables is None:
            k = np.arange(self.fft_length, dtype=np.float64)
            ang = 2.0 * np.pi * k / self.fft_length
            tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
            W = self.mel_matrix()
            lo, cnt, ptr, w = [], [], [], []
            for m in range(self.num_mel_bins):
                nz = np.nonzero(W[:, m])[0]
                if nz.size:
                    a, b = int(nz[0]), int(nz[-1]) + 1
                    assert nz.size == b - a, "a mel triangle's bins are contiguous"
                else:
                    a = b = 0
                lo.append(a), cnt.append(b - a), ptr.append(len(w))
                w.extend(W[a:b, m])
            if not w:
                w = [0.0]
            self._tables = dict(hann=self.hann().astype(np.float32), twiddle=tw.astype(np.float32), mel_lo=np.asarray(lo, np.int32),
                                mel_cnt=np.asarray(cnt, np.int32), mel_ptr=np.asarray(ptr, np.int32), mel_w=np.asarray(w, np.float32))
        return self._tables


def spec_from_config(cfg):
    return LogmelSpec(cfg.audio_transformation, cfg.num_mel_bins, cfg.sample_rate)


class LogmelFrontend:
    """Device side: the uploaded tables and the launch."""

    def __init__(self, spec, device):
        import torch
        from . import ops
        self.spec = spec
        if not ops.logmel_supported(spec.frame_length, spec.fft_length, spec.num_mel_bins, spec.window, spec.stride):
            raise NotImplementedError("the waveform front-end's kernel does not cover this configuration (avsr_logmel_supported)")
        self.t = {k: torch.as_tensor(v).to(device).contiguous() for k, v in spec.tables().items()}

    def forward(self, wav, wav_len, out, out_len=None):
        """wav [B, N] fp32, wav_len [B] int32 (samples) -> out [B, T_out, F] (every element written; F >= spec.feat), out_len [B] int32."""
        import torch
        from . import ops
        s = self.spec
        assert wav.dim() == 2 and wav.is_contiguous() and wav.dtype == torch.float32
        assert wav_len.dtype == torch.int32 and wav_len.is_contiguous() and wav_len.numel() == wav.shape[0]
        assert out.dim() == 3 and out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == wav.shape[0] and out.shape[2] >= s.feat
        assert out_len is None or (out_len.dtype == torch.int32 and out_len.is_contiguous() and out_len.numel() == wav.shape[0])
        ops.logmel_fwd(s, self.t, wav, wav_len, out, out_len)
        return out

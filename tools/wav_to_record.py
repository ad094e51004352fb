#!/usr/bin/env python
"""Directory of 16-bit PCM .wav files -> one waveform TFRecord for AVSR(audio_processing='wav').

    python tools/wav_to_record.py WAV_DIR OUT.tfrecord [--sample-rate 16000]

Every *.wav below WAV_DIR becomes one record: `input_size` 1, one float per sample (int16 / 32768), the sentence id = the path below
WAV_DIR without the extension; files are written in sorted order (write the label record in the same order).  Mono, 16-bit, and exactly
--sample-rate: anything else is refused -- nothing is resampled here."""
import argparse
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_pcm16(path, sample_rate):
    with wave.open(path, "rb") as f:
        if f.getframerate() != sample_rate:
            raise SystemExit("%s: sample rate %d, expected %d (resample it first)" % (path, f.getframerate(), sample_rate))
        if f.getsampwidth() != 2 or f.getnchannels() != 1 or f.getcomptype() != "NONE":
            raise SystemExit("%s: need mono 16-bit PCM (got %d channel(s), %d-byte samples)" % (path, f.getnchannels(), f.getsampwidth()))
        data = f.readframes(f.getnframes())
    return np.frombuffer(data, dtype="<i2").astype(np.float32) / 32768.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("wav_dir")
    ap.add_argument("out")
    ap.add_argument("--sample-rate", type=int, default=16000)
    a = ap.parse_args()
    from avsr_tf1_amd import io_utils as IO
    files = sorted(os.path.join(d, n) for d, _, ns in os.walk(a.wav_dir) for n in ns if n.lower().endswith(".wav"))
    if not files:
        raise SystemExit("no .wav files below %s" % a.wav_dir)
    waves = [(os.path.splitext(os.path.relpath(p, a.wav_dir))[0].replace(os.sep, "/"), read_pcm16(p, a.sample_rate)) for p in files]
    with IO.TFRecordFileWriter(a.out) as w:
        for name, x in waves:
            w.write(IO.make_feature_example(name, x[:, None]))
    print("%d utterances, %d samples -> %s" % (len(waves), sum(len(x) for _, x in waves), a.out))


if __name__ == "__main__":
    main()

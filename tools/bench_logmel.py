"""Waveform audio front-end (audio_processing='wav', csrc/audio_frontend.hip) at the benchmark shape (B=64, T_a=500 stacked rows =
241 040 samples per utterance): the kernel's time alone with its fraction of the HBM roofline on the bytes it must move (samples in,
features out), and the c2 train step (bench.py WORKLOADS["c2"], audio_feat 240, dropout and sampling on, hipGraph replay) from
waveforms against the same step from the features the kernel makes of them.  Prints one JSON line.
Usage: python tools/bench_logmel.py [--steps 20] [--warmup 5] [--kernel-only]"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

PEAK_HBM_TBPS = 8.0                    # MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    from avsr_tf1_amd.audio_frontend import LogmelFrontend, LogmelSpec
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    wl = bench.WORKLOADS["c2"]
    B, T = wl["B"], bench.TA
    spec = LogmelSpec()
    N = spec.samples_for_rows(T)
    rng = np.random.default_rng(1001)
    wav = torch.as_tensor((rng.standard_normal((B, N)) * 0.1).astype(np.float32)).cuda()
    wav_len = torch.full((B,), N, dtype=torch.int32, device="cuda")
    feats = torch.zeros(B, T, spec.feat, device="cuda")
    fe = LogmelFrontend(spec, "cuda")
    for _ in range(10):
        fe.forward(wav, wav_len, feats)
    torch.cuda.synchronize()
    reps = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fe.forward(wav, wav_len, feats)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    nbytes = wav.numel() * 4 + feats.numel() * 4
    frames = B * spec.frames(N)
    out = dict(kernel="logmel_kernel", B=B, samples=N, rows=T, feat=spec.feat, frames=frames, kernel_us=round(us, 2), bytes_moved=nbytes,
               achieved_tbps=round(nbytes / us / 1e6, 3), hbm_roofline_fraction=round(nbytes / us / 1e6 / PEAK_HBM_TBPS, 4),
               peak_hbm_tbps=PEAK_HBM_TBPS)
    if not args.kernel_only:
        cfg_f = ModelConfig(audio_feat=spec.feat, use_dropout=True, sampling_probability=0.1, **wl["cfg"])
        cfg_w = dataclasses.replace(cfg_f, audio_processing="wav")
        d = bench.synth(cfg_f, B, 0)
        labels = {k: torch.as_tensor(d[k]).cuda() for k in ("labels", "labels_len")}
        bf = Batch(audio=feats.clone(), audio_len=torch.full((B,), T, dtype=torch.int32, device="cuda"), **labels)
        bw = Batch(audio=wav, audio_len=wav_len, **labels)
        steps = {}
        for name, cfg, batch in (("features", cfg_f, bf), ("wav", cfg_w, bw)):
            model = Seq2SeqModel(cfg, seed=2001)
            trainer = DataParallelTrainer(model, None, use_graph=True)
            batch = trainer.static_batch(batch)
            for _ in range(args.warmup):
                trainer.train_step(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                trainer.train_step(batch)
            torch.cuda.synchronize()
            steps[name] = dict(ms_per_step=round((time.perf_counter() - t0) * 1e3 / args.steps, 3), mode=trainer.mode, loss=float(model.loss.item()))
            del trainer, model
        out.update(workload="c2 (audio_feat 240)", steps=args.steps, train_step=steps,
                   wav_minus_features_us=round((steps["wav"]["ms_per_step"] - steps["features"]["ms_per_step"]) * 1e3, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

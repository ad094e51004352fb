"""Train-step time of the headline c4 workload (bench.py WORKLOADS["c4"]: B=64, T_v=75 x 36x36x3 lip crops, T_a=500, L=40, dropout
and scheduled sampling on, hipGraph replay) with video_processing='3dconv_cnn' in place of resnet_cnn, plus the per-class times of the
conv3d kernels (csrc/conv3d.hip) from one eagerly launched, event-timed step and their fraction of the fp32 MFMA peak.
Prints one JSON line.  Usage: python tools/bench_cnn3d.py [--steps 10] [--warmup 3] [--filters 8,16,32,64] [--eager-only]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3          # MI355X: 256 CUs x 4 SIMD x 64 FLOP/clk x 2.4 GHz (v_mfma_f32_16x16x4_f32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--filters", default="8,16,32,64")
    ap.add_argument("--eager-only", action="store_true", help="only the two eager steps (a rocprofv3 --pmc pass)")
    args = ap.parse_args()
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    wl = bench.WORKLOADS["c4"]
    filters = tuple(int(f) for f in args.filters.split(","))
    common = dict(audio_feat=bench.FA, video_feat=128, cnn_dense_units=128, cnn_filters=filters, use_dropout=True, sampling_probability=0.1,
                  **wl["cfg"])
    data = bench.synth(ModelConfig(video_processing="resnet_cnn", **common), wl["B"], 0)     # the same [B, 75, 36, 36, 3] crops
    cfg = ModelConfig(video_processing="3dconv_cnn", **common)
    batch = Batch.from_numpy(bench.NS(data))
    model = Seq2SeqModel(cfg, seed=2001)
    # per-class kernel times: one eager step under the event profiler
    eager = DataParallelTrainer(model, None, use_graph=False)
    eager.train_step(batch)
    torch.cuda.synchronize()
    ops.prof_begin()
    eager.train_step(batch)
    prof = ops.prof_end()
    names = {"conv_fwd": "conv3d_fwd", "conv_bwd_data": "conv3d_bwd_data", "conv_bwd_weight": "conv3d_bwd_weight"}
    kinds = {}
    for k, nm in names.items():
        cnt, ms, fl = prof.get(k, (0, 0.0, 0.0))
        kinds[nm] = dict(launches=cnt, ms=round(ms, 3), gflop=round(fl / 1e9, 2),
                         mfma_fraction=round(fl / (ms * 1e-3) / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4) if ms > 0 else None)
    del eager
    if args.eager_only:
        print(json.dumps(dict(workload="c4_3dconv_cnn", mode="eager", kernels=kinds)))
        return
    trainer = DataParallelTrainer(model, None, use_graph=True)
    for _ in range(args.warmup):
        trainer.train_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        trainer.train_step(batch)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    print(json.dumps(dict(workload="c4_3dconv_cnn", B=wl["B"], T_v=bench.TV, T_a=bench.TA, L=bench.LDEC, cnn_filters=list(filters),
                          mode=trainer.mode, steps=args.steps, ms_per_step=round(ms, 2), loss=float(model.loss.item()),
                          kernels=kinds, peak_fp32_mfma_tflops=PEAK_FP32_MFMA_TFLOPS)))


if __name__ == "__main__":
    main()

"""What the lip-crop augmentation in the train step (video_augment, csrc/video_augment.hip) costs: the launch next to the engine's copy
kernel and avsr_spec_augment on the same buffer, the c4 train step with the keyword on and off, and the switch-off step against another
checkout.

    python tools/video_augment_cost.py                       # this tree: launches and steps by device events, ONE process per mode
    python tools/video_augment_cost.py --compare-root DIR    # + the switch-off step of another checkout (built; the parent commit),
                                                             #   child processes ALTERNATED with this tree's, never two at once

Every result line is printed and appended to --out (default profiles/video_augment_cost.txt, rewritten by each run).

Shape: the lip crops of the c4 workload, B = 64, T_v = 75, 36 x 36 x 3 (74.6 MB).  "launch": avsr_video_augment geometry only (flip 0.5,
max_shift 3: one kernel, one read, one write) and with contrast and brightness on top (three kernels, the valid frames read twice); the
yardsticks in the same process on the same buffer: the engine's copy kernel (one read, one write) and avsr_spec_augment with one video
time mask, 'zero' fill (one read, one write) and 'mean' fill (the valid rows read twice).  All alternate, device events around runs of 200
eager launches after a warm-up.  "step_on" / "step_off": eager train steps of the c4 model (bimodal, lip crops through resnet_cnn, video
1 x 256 + audio 3 x 256 LSTM encoders, regress_aus) with and without the keyword, device events around runs of 5 steps.  Not measured:
the step under a captured graph, '3dconv_cnn', more than one GPU."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TV, HWC = 64, 75, (36, 36, 3)
GEO = dict(flip_q24=1 << 23, max_shift=3)
FULL = dict(GEO, contrast=0.2, brightness=0.2)
VAUG = dict(vaug_flip_q24=1 << 23, vaug_max_shift=3, vaug_contrast=0.2, vaug_brightness=0.2)


def launches(reps):
    import numpy as np
    import torch
    from avsr_tf1_amd import ops
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.uniform(-1.0, 1.0, (B, TV) + HWC), dtype=torch.float32).cuda()
    lens = torch.as_tensor(rng.integers(TV // 2, TV + 1, B), dtype=torch.int32).cuda()
    seed = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = torch.empty_like(x)
    F = int(np.prod(HWC))
    x3, y3 = x.view(B, TV, F), y.view(B, TV, F)
    ws = torch.zeros(ops.video_augment_ws_floats(B, TV, *HWC), device="cuda")
    sws = torch.zeros(ops.spec_augment_ws_floats(B, TV, F), device="cuda")
    sp = dict(video=True, time_masks=1, time_width=10, ratio_q16=13107)
    fns = {"geometry": lambda: ops.video_augment(x, lens, seed, y, None, **GEO),
           "contrast": lambda: ops.video_augment(x, lens, seed, y, ws, **FULL),
           "copy": lambda: ops.copy_(y, x),
           "spec_zero": lambda: ops.spec_augment(x3, F, lens, seed, y3, None, mean_fill=False, **sp),
           "spec_mean": lambda: ops.spec_augment(x3, F, lens, seed, y3, sws, mean_fill=True, **sp)}
    res = {"mode": "launch", "shape": "c4", "B": B, "T": TV, "HWC": list(HWC), "MB": round(x.numel() * 4 / 1e6, 1),
           "valid_frames": round(float(lens.float().mean().item()) / TV, 3)}
    for _ in range(5):
        for f in fns.values():
            f()
    for _ in range(reps):                                         # the five alternate, so all see the same machine state
        for k, f in fns.items():
            e0.record()
            for _ in range(200):
                f()
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(k + "_us", []).append(round(1e3 * e0.elapsed_time(e1) / 200, 1))
    med = lambda k: sorted(res[k + "_us"])[len(res[k + "_us"]) // 2]
    res["ratios_of_medians"] = {"geometry/copy": round(med("geometry") / med("copy"), 2),
                                "geometry/spec_zero": round(med("geometry") / med("spec_zero"), 2),
                                "geometry/spec_mean": round(med("geometry") / med("spec_mean"), 2),
                                "contrast/spec_mean": round(med("contrast") / med("spec_mean"), 2)}
    print(json.dumps(res), flush=True)


def step(root, on, reps):
    import numpy as np
    import torch
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    TA, FA, L = 500, 80, 40
    cfg = ModelConfig(architecture="bimodal", encoder_type="unidirectional", video_units=(256,), audio_units=(256, 256, 256),
                      attention_type=(("scaled_luong",), ("scaled_luong",)), regress_aus=True, audio_feat=FA, video_feat=128,
                      video_processing="resnet_cnn", use_dropout=True, sampling_probability=0.1, **(VAUG if on else {}))
    model = Seq2SeqModel(cfg, seed=0)
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    labels = rng.integers(1, 29, (B, L))
    labels[:, -1] = 29
    batch = Batch(audio=t(rng.standard_normal((B, TA, FA)), torch.float32), audio_len=t(np.full(B, TA), torch.int32),
                  video=t(rng.uniform(-1.0, 1.0, (B, TV) + HWC), torch.float32), video_len=t(np.full(B, TV), torch.int32),
                  aus=t(rng.uniform(0, 3, (B, TV, 2)), torch.float32), labels=t(labels, torch.int32), labels_len=t(np.full(B, L), torch.int32))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        model.train_step(batch)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0.record()
        for _ in range(5):
            model.train_step(batch)
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1) / 5, 3))
    print(json.dumps({"mode": "step_on" if on else "step_off", "root": os.path.relpath(root, HERE), "shape": "c4", "B": B, "T_v": TV,
                      "step_ms": ms, "loss": round(float(model.loss.item()), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "video_augment_cost.txt"))
    a = ap.parse_args()
    if a.one:
        sys.path.insert(0, os.path.abspath(a.root))
        if a.one == "launch":
            launches(a.reps)
        else:
            step(os.path.abspath(a.root), a.one == "step_on", a.reps)
        return
    me = os.path.abspath(__file__)
    runs = [(HERE, "launch"), (HERE, "step_off"), (HERE, "step_on"), (HERE, "step_off"), (HERE, "step_on")]
    if a.compare_root:                                        # other, this, other, this, ...: fresh child processes, never two at once
        for _ in range(a.rounds):
            runs += [(os.path.abspath(a.compare_root), "step_off"), (HERE, "step_off")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for root, mode in runs:
            p = subprocess.run([sys.executable, me, "--one", mode, "--root", root, "--reps", str(a.reps)], check=True, timeout=280,
                               stdout=subprocess.PIPE)
            for line in p.stdout.decode().strip().splitlines():
                if line.startswith("{"):
                    print(line, flush=True)
                    f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()

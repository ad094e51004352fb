"""What SpecAugment in the train step (spec_augment, csrc/specaugment.hip) costs: the launch next to a device-to-device copy of the same
buffer, the train step with the switch on and off, and the switch-off step against another checkout.

    python tools/specaugment_cost.py                         # this tree: launches and steps by device events, ONE process per mode
    python tools/specaugment_cost.py --compare-root DIR      # + the switch-off step of another checkout (built; the parent commit),
                                                             #   child processes ALTERNATED with this tree's, never two at once

Every result line is printed and appended to --out (default profiles/specaugment_cost.txt, rewritten by each run).

Shapes: c2 = the audio features of the c2 workload (B = 64, T_a = 500, 240 columns = 8 stacked frames of 30 mel bins), c4 = its lip
crops (B = 64, T_v = 75, 36 x 36 x 3 = 3888 columns).  "launch": avsr_spec_augment ('mean': three kernels, 'zero': one) and the engine's
copy kernel on a buffer of the same size, alternating, device events around runs of 200 eager launches after a warm-up; the yardstick is
the copy (one read, one write), 'mean' reads the valid rows twice.  "step_on" / "step_off": eager train steps of the c2 audio model
(3 x 256 bidirectional LSTM encoder, use_ctc) with and without the keyword, device events around runs of 10 steps.  The c4 model's step is
not timed here."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c2": (64, 500, 240, dict(video=False, time_masks=2, time_width=40, ratio_q16=13107, freq_masks=2, freq_width=7, freq_bins=30)),
          "c4": (64, 75, 36 * 36 * 3, dict(video=True, time_masks=1, time_width=10, ratio_q16=13107))}
SPEC = dict(spec_freq_masks=2, spec_freq_width=7, spec_freq_bins=30, spec_time_masks=2, spec_time_width=40, spec_time_ratio=0.2)


def launches(reps):
    import numpy as np
    import torch
    from avsr_tf1_amd import ops
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, (B, T, F, p) in SHAPES.items():
        rng = np.random.default_rng(0)
        x = torch.as_tensor(rng.standard_normal((B, T, F)), dtype=torch.float32).cuda()
        lens = torch.as_tensor(rng.integers(T // 2, T + 1, B), dtype=torch.int32).cuda()
        seed = torch.zeros(1, dtype=torch.int32, device="cuda")
        y = torch.empty_like(x)
        ws = torch.zeros(ops.spec_augment_ws_floats(B, T, F), device="cuda")
        fns = {"mean": lambda: ops.spec_augment(x, F, lens, seed, y, ws, mean_fill=True, **p),
               "zero": lambda: ops.spec_augment(x, F, lens, seed, y, None, mean_fill=False, **p),
               "copy": lambda: ops.copy_(y, x)}
        res = {"mode": "launch", "shape": name, "B": B, "T": T, "F": F, "MB": round(x.numel() * 4 / 1e6, 1),
               "valid_rows": round(float(lens.float().mean().item()) / T, 3)}
        for _ in range(5):
            for f in fns.values():
                f()
        for _ in range(reps):                                     # the three alternate, so all see the same machine state
            for k, f in fns.items():
                e0.record()
                for _ in range(200):
                    f()
                e1.record()
                torch.cuda.synchronize()
                res.setdefault(k + "_us", []).append(round(1e3 * e0.elapsed_time(e1) / 200, 1))
        print(json.dumps(res), flush=True)


def step(root, on, reps):
    import numpy as np
    import torch
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    B, T, F, L = 64, 500, 240, 40
    cfg = ModelConfig(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(256, 256, 256),
                      decoder_units=(256,), embedding_size=128, audio_feat=F, attention_type=(("bahdanau",), ("bahdanau",)),
                      use_dropout=True, sampling_probability=0.1, use_ctc=True, **(SPEC if on else {}))
    model = Seq2SeqModel(cfg, seed=0)
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    labels = rng.integers(1, 29, (B, L))
    labels[:, -1] = 29
    batch = Batch(audio=t(rng.standard_normal((B, T, F)), torch.float32), audio_len=t(rng.integers(T // 2, T + 1, B), torch.int32),
                  labels=t(labels, torch.int32), labels_len=t(np.full(B, L), torch.int32))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        model.train_step(batch)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0.record()
        for _ in range(10):
            model.train_step(batch)
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1) / 10, 3))
    print(json.dumps({"mode": "step_on" if on else "step_off", "root": os.path.relpath(root, HERE), "shape": "c2", "B": B, "T": T, "F": F,
                      "step_ms": ms, "loss": round(float(model.loss.item()), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "specaugment_cost.txt"))
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

"""What the CTC auxiliary loss (use_ctc) costs per train step, and that it costs nothing when it is off.

    python tools/ctc_cost.py                         # this tree: step time with use_ctc off and on, avsr_ctc_loss alone (device events)
    python tools/ctc_cost.py --compare-root DIR      # + the use_ctc=False step time of another checkout (built; the parent commit), child
                                                     #   processes ALTERNATED with this tree's, so both see the same machine state

Shape: the c2 workload (audio-only, 3 x 256 bidirectional LSTM encoder, Bahdanau decoder, B = 64, T_a = 500 x 80, L = 40), a resident
batch, eager launches.  Step times are host-clock times around runs of train steps that end in a device synchronise, after warm-up
steps; the kernel is timed by device events around 200 launches on the step's own buffers.  One JSON line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, L, FA = 64, 500, 40, 80


def one(root, modes, reps):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    labels = rng.integers(1, 29, (B, L))
    labels[:, -1] = 29
    batch = Batch(audio=t(rng.standard_normal((B, TA, FA)), torch.float32), audio_len=t(np.full(B, TA), torch.int32),
                  labels=t(labels, torch.int32), labels_len=t(np.full(B, L), torch.int32))
    res = {"root": os.path.relpath(root, HERE), "B": B, "T_a": TA, "L": L}
    for mode in modes:
        kw = dict(use_ctc=True) if mode == "ctc" else {}
        cfg = ModelConfig(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(256, 256, 256),
                          decoder_units=(256,), embedding_size=128, audio_feat=FA, attention_type=(("bahdanau",), ("bahdanau",)),
                          use_dropout=False, sampling_probability=0.0, **kw)
        model = Seq2SeqModel(cfg, seed=0)
        for _ in range(5):
            model.train_step(batch)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(10):
                model.train_step(batch)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / 10)
        res["step_ms_" + mode] = [round(x, 3) for x in ms]
        if mode == "ctc":
            from avsr_tf1_amd import ops
            E, Cc = model._cur[0]["enc"]["audio"], cfg.vocab_size + 1
            launch = lambda: ops.ctc_loss(E["ctc_z"], Cc, batch.labels, batch.labels_len, E["len"], model.denom, cfg.ctc_weight, E["ctc_nll"],
                                          E["ctc_status"], E["ctc_utt"], E["ctc_dz"], E["ctc_ws"], B, TA, L, Cc)
            for _ in range(5):
                launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            us = []
            for _ in range(reps):
                e0.record()
                for _ in range(200):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / 200)
            res["ctc_loss_us"] = [round(u, 1) for u in us]
            res["ctc_nll_mean"] = round(float(E["ctc_nll"].mean().item()), 3)
        del model
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="off,ctc")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.one or not a.compare_root:
        one(os.path.abspath(a.root), a.modes.split(","), a.reps)
        return
    me = os.path.abspath(__file__)
    for r in range(a.rounds):                                 # other, this, other, this, ...: fresh child processes, never two at once
        for root, modes in ((os.path.abspath(a.compare_root), "off"), (HERE, "off,ctc" if r == 0 else "off")):
            subprocess.run([sys.executable, me, "--one", "--root", root, "--modes", modes, "--reps", str(a.reps)], check=True, timeout=280)


if __name__ == "__main__":
    main()

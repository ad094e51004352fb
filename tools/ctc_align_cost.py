"""What CTC forced alignment (Seq2SeqModel.ctc_align, csrc/ctc_align.hip) costs next to the CTC loss launch, and that adding it left the
decodes where they were.

    python tools/ctc_align_cost.py                         # this tree: avsr_ctc_align and avsr_ctc_loss by device events in ONE process,
                                                           #   utterances/s of ctc_align and of the three decodes
    python tools/ctc_align_cost.py --compare-root DIR      # + greedy / beam / prefix decodes of another checkout (built; the parent
                                                           #   commit), child processes ALTERNATED with this tree's, never two at once

Every result line is printed and appended to --out (default profiles/ctc_align_cost.txt, rewritten by each run).

Shape: the c2 workload (audio-only, 3 x 256 bidirectional LSTM encoder, Bahdanau decoder, use_ctc=True, B = 64, T_a = 500 x 80, label
rows of L = 40 with the EOS last, so 39 labels are aligned), V = 31, random weights.  The two launches are timed by device events around
runs of 200 eager launches on the same head logits (those a train step left in the workspace), after a warm-up; the rates are host-clock
times around whole model-level calls (encoders included) that end with the result on the host."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, L, FA, K, STEPS = 64, 500, 40, 80, 10, 150


def one(root, modes, reps):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    cfg = ModelConfig(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(256, 256, 256),
                      decoder_units=(256,), embedding_size=128, audio_feat=FA, attention_type=(("bahdanau",), ("bahdanau",)),
                      use_dropout=False, sampling_probability=0.0, use_ctc=True)
    model = Seq2SeqModel(cfg, seed=0)
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    labels = rng.integers(1, 29, (B, L))
    labels[:, -1] = 29
    batch = Batch(audio=t(rng.standard_normal((B, TA, FA)), torch.float32), audio_len=t(np.full(B, TA), torch.int32),
                  labels=t(labels, torch.int32), labels_len=t(np.full(B, L), torch.int32))
    res = {"root": os.path.relpath(root, HERE), "B": B, "T_a": TA, "L": L, "K": K, "max_steps": STEPS}
    decode = {"beam": lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS).cpu(),
              "greedy": lambda: model.greedy_decode(batch, max_steps=STEPS).cpu(),
              "prefix": lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS),
              "align": lambda: model.ctc_align(batch)}
    for mode in modes:
        if mode == "launch":
            continue
        decode[mode]()
        torch.cuda.synchronize()
        rates = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(5):
                decode[mode]()
            torch.cuda.synchronize()
            rates.append(5 * B / (time.perf_counter() - t0))
        res[mode + "_utt_per_s"] = [round(r, 1) for r in rates]
    if "launch" in modes:
        for _ in range(3):
            model.train_step(batch)
        torch.cuda.synchronize()
        E, V = model._cur[0]["enc"]["audio"], cfg.vocab_size
        Cc, T = V + 1, E["T"]
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
        tlen = (batch.labels_len - 1).clamp(min=0).to(torch.int32)
        out = (torch.zeros(B, device="cuda"), i32(B), i32(B, T), torch.zeros(B, T, device="cuda"), i32(B, L), i32(B, L))
        ws = torch.zeros(ops.ctc_align_ws_bytes(B, T, L) // 8, dtype=torch.int64, device="cuda")
        launches = {"ctc_loss": lambda: ops.ctc_loss(E["ctc_z"], Cc, batch.labels, batch.labels_len, E["len"], model.denom, cfg.ctc_weight,
                                                     E["ctc_nll"], E["ctc_status"], E["ctc_utt"], E["ctc_dz"], E["ctc_ws"], B, T, L, Cc),
                    "ctc_align": lambda: ops.ctc_align(E["ctc_z"], Cc, batch.labels, tlen, E["len"], B, T, L, V, *out, ws)}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            for f in launches.values():
                f()
        for r in range(reps):                                     # the two launches alternate, so both see the same machine state
            for name, f in launches.items():
                e0.record()
                for _ in range(200):
                    f()
                e1.record()
                torch.cuda.synchronize()
                res.setdefault(name + "_us", []).append(round(1e3 * e0.elapsed_time(e1) / 200, 1))
        res["T"], res["U"] = T, L - 1
        res["ctc_align_frame_us"] = [round(u / T, 3) for u in res["ctc_align_us"]]
        res["aligned"] = int(out[1].sum().item())
        res["ctc_nll_mean"] = round(float(E["ctc_nll"].mean().item()), 3)
        res["align_score_mean"] = round(float(out[0].mean().item()), 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="launch,align,greedy,beam,prefix")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ctc_align_cost.txt"))
    a = ap.parse_args()
    if a.one:
        one(os.path.abspath(a.root), a.modes.split(","), a.reps)
        return
    me = os.path.abspath(__file__)
    runs = [(HERE, a.modes)]
    if a.compare_root:                                        # other, this, other, this, ...: fresh child processes, never two at once
        runs = []
        for r in range(a.rounds):
            runs += [(os.path.abspath(a.compare_root), "greedy,beam,prefix"), (HERE, a.modes if r == 0 else "greedy,beam,prefix")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for root, modes in runs:
            p = subprocess.run([sys.executable, me, "--one", "--root", root, "--modes", modes, "--reps", str(a.reps)], check=True, timeout=280,
                               stdout=subprocess.PIPE)
            line = p.stdout.decode().strip().splitlines()[-1]
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()

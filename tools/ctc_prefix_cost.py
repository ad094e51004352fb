"""What CTC prefix beam search (decoding_algorithm='ctc_prefix_beam_search') costs next to the two attention decodes, and that adding it
left beam search where it was.

    python tools/ctc_prefix_cost.py                         # this tree: the launch by device events; utterances/s of the three decodes
    python tools/ctc_prefix_cost.py --compare-root DIR      # + 'beam_search' of another checkout (built; the parent commit), child
                                                            #   processes ALTERNATED with this tree's, so both see the same machine state

Shape: the c2 workload (audio-only, 3 x 256 bidirectional LSTM encoder, Bahdanau decoder, use_ctc=True, B = 64, T_a = 500 x 80), beam
width 10, V = 31, max_steps = 150 as `evaluate` passes it.  Random weights: the attention decodes never emit EOS and run all 150 steps,
and the head's rows are nearly flat, so the prefix beam holds label sequences that grow to L_max -- the dearest case for all three.
Rates are host-clock times around whole model-level decodes (encoders included) that end with the ids on the host, after a warm-up;
avsr_ctc_prefix_search alone is timed by device events around runs of launches on the model's own head logits, per launch and per
frame.  One JSON line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, FA, K, STEPS = 64, 500, 80, 10, 150


def one(root, modes, reps):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    cfg = ModelConfig(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(256, 256, 256),
                      decoder_units=(256,), embedding_size=128, audio_feat=FA, attention_type=(("bahdanau",), ("bahdanau",)),
                      use_dropout=False, sampling_probability=0.0, use_ctc=True)
    model = Seq2SeqModel(cfg, seed=0)
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    batch = Batch(audio=t(rng.standard_normal((B, TA, FA)), torch.float32), audio_len=t(np.full(B, TA), torch.int32))
    res = {"root": os.path.relpath(root, HERE), "B": B, "K": K, "T_a": TA, "max_steps": STEPS}
    decode = {"beam": lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS).cpu(),
              "greedy": lambda: model.greedy_decode(batch, max_steps=STEPS).cpu(),
              "prefix": lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS)}
    for mode in modes:
        out = decode[mode]()
        torch.cuda.synchronize()
        res["len_" + mode] = int(out.shape[1]) if mode != "prefix" else max(len(s) for s in out)
        rates = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(5):
                decode[mode]()
            torch.cuda.synchronize()
            rates.append(5 * B / (time.perf_counter() - t0))
        res[mode + "_utt_per_s"] = [round(r, 1) for r in rates]
    if "prefix" in modes:
        from avsr_tf1_amd import ops
        V = cfg.vocab_size
        ws = model._get_ws(B, model._audio_rows(batch), 0, 1, True)
        E = ws["enc"]["audio"]                                                # the head logits the decode above left there
        ids, lens, score = E[("ctc_prefix", K, STEPS)]
        T = E["T"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us = []
        for _ in range(reps):
            e0.record()
            for _ in range(10):
                ops.ctc_prefix_search(E["ctc_z"], V + 1, E["len"], B, T, V, K, STEPS, ids, lens, score)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / 10)
        res["prefix_launch_us"] = [round(u, 1) for u in us]
        res["prefix_frame_us"] = [round(u / T, 2) for u in us]
        res["prefix_launches"], res["T"] = 1, T
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="beam,greedy,prefix")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.one or not a.compare_root:
        one(os.path.abspath(a.root), a.modes.split(","), a.reps)
        return
    me = os.path.abspath(__file__)
    for r in range(a.rounds):                                 # other, this, other, this, ...: fresh child processes, never two at once
        for root, modes in ((os.path.abspath(a.compare_root), "beam"), (HERE, "beam,greedy,prefix" if r == 0 else "beam")):
            subprocess.run([sys.executable, me, "--one", "--root", root, "--modes", modes, "--reps", str(a.reps)], check=True, timeout=280)


if __name__ == "__main__":
    main()

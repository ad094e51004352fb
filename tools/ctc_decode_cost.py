"""What joint CTC / attention scoring (ctc_decode_weight) costs per beam-search step, and that it costs nothing when it is off.

    python tools/ctc_decode_cost.py                         # this tree: decode rate with the term off and on, the new launches (device events)
    python tools/ctc_decode_cost.py --compare-root DIR      # + the rate of another checkout (built; the parent commit) with the term off,
                                                            #   child processes ALTERNATED with this tree's, so both see the same machine state

Shape: the c2 workload (audio-only, 3 x 256 bidirectional LSTM encoder, Bahdanau decoder, use_ctc=True, B = 64, T_a = 500 x 80), beam
width 10, V = 31, 40 steps (random weights never emit EOS, so every step runs and every row is extended and scored: the dearest case).
Rates are host-clock times around whole decodes that end in a device synchronise, after a warm-up decode; avsr_beam_ctc_step and
avsr_beam_ctc_begin are timed by device events around runs of launches on the search's own buffers (R = 640 rows).  One JSON line per
result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, FA, K, STEPS = 64, 500, 80, 10, 40


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
    res = {"root": os.path.relpath(root, HERE), "B": B, "K": K, "T_a": TA, "steps": STEPS}
    for mode in modes:
        kw = dict(ctc_weight=0.3) if mode == "ctc" else {}
        out = model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, **kw)
        torch.cuda.synchronize()
        res["steps_run_" + mode] = int(out.shape[1])
        rates = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(5):
                model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, **kw)
            torch.cuda.synchronize()
            rates.append(5 * B / (time.perf_counter() - t0))
        res[mode + "_utt_per_s"] = [round(r, 1) for r in rates]
    if "ctc" in modes:
        from avsr_tf1_amd import ops
        R, V = B * K, cfg.vocab_size
        ws = model._get_ws(B, model._audio_rows(batch), 0, 1, True)
        c = model._beam_ctc_desc(ws, 0.3, model._beam_ws[2], B, K, None)      # the descriptor the search itself fills; queues the begin launch
        sym = [v for v in range(V) if v != cfg.eos_id]
        toks = [torch.as_tensor([sym[(r + s) % len(sym)] for r in range(R)], dtype=torch.int32).cuda() for s in range(2)]
        par = torch.arange(R, dtype=torch.int32, device="cuda")
        fin = torch.zeros(R, dtype=torch.int32, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us, bus = [], []
        for _ in range(reps):
            ops.beam_ctc_begin(c)
            ops.beam_ctc_step(c, toks[0], par, fin, 0)
            e0.record()
            for s in range(1, STEPS):                                         # prefixes of 1 .. 39 symbols, as in the search
                ops.beam_ctc_step(c, toks[s & 1], par, fin, s)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / (STEPS - 1))
            e0.record()
            for _ in range(50):
                ops.beam_ctc_begin(c)
            e1.record()
            torch.cuda.synchronize()
            bus.append(1e3 * e0.elapsed_time(e1) / 50)
        res["ctc_step_us"] = [round(u, 1) for u in us]
        res["ctc_begin_us"] = [round(u, 1) for u in bus]
        res["ctc_step_launches"] = 1
        res["state_bytes"] = 4 * (2 * R * TA * 2 + 4 * R + 2 * R * V + B * TA * (V + 1))
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

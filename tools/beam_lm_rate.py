"""Beam-search rate with and without the shallow-fusion language model, and the language-model step on its own.

    python tools/beam_lm_rate.py                         # this tree: no-LM rate, LM rate, LM step microseconds
    python tools/beam_lm_rate.py --compare-root DIR      # + the no-LM rate of another checkout (built), child processes ALTERNATED
                                                         #   with this tree's, so both see the same machine state

Shape: the c4 evaluation batch (bimodal, 256 units, B = 64, T_a = 500, T_v = 75, beam width 10, V = 31, 40 steps; random weights never
emit EOS, so every step runs) with a 1 x 256 language model (embedding 128).  Rates are host-clock times around whole decodes that end
in a device synchronise, after a warm-up decode; the LM step is timed by device events around a run of steps.  One JSON line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, TV, K, STEPS = 64, 500, 75, 10, 40


def one(root, with_lm, reps):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    cfg = ModelConfig(architecture="bimodal", video_units=(256,), audio_units=(256, 256, 256), decoder_units=(256,), embedding_size=128,
                      video_feat=128, audio_feat=80, use_dropout=False, sampling_probability=0.0)
    model = Seq2SeqModel(cfg, seed=0)
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    batch = Batch(audio=t(rng.standard_normal((B, TA, 80)), torch.float32), audio_len=t(np.full(B, TA), torch.int32),
                  video=t(rng.standard_normal((B, TV, 128)), torch.float32), video_len=t(np.full(B, TV), torch.int32))
    res = {"root": os.path.relpath(root, HERE), "B": B, "K": K, "steps": STEPS}
    kws = [("no_lm", {})]
    lm = None
    if with_lm:
        lcfg = ModelConfig(architecture="lm", video_units=None, audio_units=None, decoder_units=(256,), embedding_size=128, use_dropout=False,
                           sampling_probability=0.0, warmup_steps=0)
        lm = Seq2SeqModel(lcfg, seed=1)
        kws.append(("lm", dict(lm=lm, lm_weight=0.3)))
    for name, kw in kws:
        model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, **kw)
        torch.cuda.synchronize()
        rates = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(5):
                model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, **kw)
            torch.cuda.synchronize()
            rates.append(5 * B / (time.perf_counter() - t0))
        res[name + "_utt_per_s"] = [round(r, 1) for r in rates]
    if with_lm:
        R = B * K
        m = model._beam_lm_desc(lm, 0.3, model._beam_ws[2], R)       # the descriptor the search itself fills (buffers of the cached workspace)
        tok = torch.zeros(R, dtype=torch.int32, device="cuda")
        par = torch.arange(R, dtype=torch.int32, device="cuda")
        for s in range(4):
            ops.beam_lm_step(m, tok, par, R, s)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us = []
        for _ in range(reps):
            e0.record()
            for s in range(200):
                ops.beam_lm_step(m, tok, par, R, s + 1)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / 200)
        lc = lm.cfg
        nl, H, E, V = len(lc.decoder_units), lc.decoder_units[0], lc.embedding_size, lc.vocab_size
        wbytes = 4 * (sum(((E if j == 0 else H) + H) * 4 * H + 4 * H for j in range(nl)) + H * V + V)
        res["lm_step_us"] = [round(u, 2) for u in us]
        res["lm_step_launches"] = nl + 1
        res["lm_weight_bytes"] = wbytes
        res["lm_weight_read_once_us_at_8TBps"] = round(wbytes / 8e12 * 1e6, 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--no-lm", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.one or not a.compare_root:
        one(os.path.abspath(a.root), not a.no_lm, a.reps)
        return
    me = os.path.abspath(__file__)
    for r in range(a.rounds):                                 # other, this, other, this, ...: fresh child processes, never two at once
        for root, extra in ((os.path.abspath(a.compare_root), ["--no-lm"]), (HERE, [] if r == 0 else ["--no-lm"])):
            subprocess.run([sys.executable, me, "--one", "--root", root, "--reps", str(a.reps)] + extra, check=True, timeout=280)


if __name__ == "__main__":
    main()

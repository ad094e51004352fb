"""What a back-off n-gram fused into beam search costs (Seq2SeqModel.beam_search_decode(ngram=...), csrc/beam_ngram.hip) next to the plain
search and the LSTM-fused one, and that adding it left the searches that existed where they were.

    python tools/beam_ngram_cost.py                      # this tree, ONE process: plain, LSTM and n-gram (orders 2 and 4) decodes/s, and
                                                         #   the LSTM's and the n-gram's step launches by device events
    python tools/beam_ngram_cost.py --compare-root DIR   # + another checkout (built; the parent commit), child processes ALTERNATED with
                                                         #   this tree's: plain 'beam_search', 'beam_search' with the LSTM, and the CTC prefix
                                                         #   search with its n-gram

Shape: the c2 evaluation batch (unimodal, bidirectional 3 x 256 audio encoder, Bahdanau, 256-unit decoder, use_ctc; B = 64, T_a = 500 x 80,
beam width 10 -> 640 hypothesis rows, V = 31, 40 steps; random weights never emit EOS, so every step runs), the 1 x 256 / 128 LSTM
language model, and tools/ctc_prefix_ngram_cost.py's Witten-Bell n-grams on 2000 random label rows (the arc counts are reported).  Rates
are host-clock times around whole decodes that end in a device synchronise, after a warm-up decode; a step launch is timed by device
events around 200 launches whose symbols and parents are random (so the walks start from many nodes).  One JSON line per result."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, FA, K, STEPS, PREFIX_STEPS, LMW = 64, 500, 80, 10, 40, 150, 0.3


def _ngram_tables(cfg, order):
    spec = importlib.util.spec_from_file_location("ctc_prefix_ngram_cost", os.path.join(HERE, "tools", "ctc_prefix_ngram_cost.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool._ngram_tables(cfg, order)


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
    batch = Batch(audio=t(rng.standard_normal((B, TA, FA)), torch.float32), audio_len=t(np.full(B, TA), torch.int32))
    res = {"root": os.path.relpath(root, HERE), "B": B, "K": K, "T_a": TA, "steps": STEPS, "lm_weight": LMW}
    lm, tables = None, {}
    if "lm" in modes:
        lcfg = ModelConfig(architecture="lm", video_units=None, audio_units=None, decoder_units=(256,), embedding_size=128,
                           vocab_size=cfg.vocab_size, go_id=cfg.go_id, eos_id=cfg.eos_id, use_dropout=False, sampling_probability=0.0,
                           warmup_steps=0)
        lm = Seq2SeqModel(lcfg, seed=1)
        res["lm"] = "1x256/128"
    for mode in modes:
        if "ngram" in mode:
            o = int(mode[-1])
            if o not in tables:
                tables[o] = _ngram_tables(cfg, o)
                res["ngram%d_nodes_arcs" % o] = [int(tables[o]["n_nodes"]), int(tables[o]["n_arcs"])]

    def decoder(mode):
        if mode == "plain":
            return lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS)
        if mode == "lm":
            return lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, lm=lm, lm_weight=LMW)
        if mode.startswith("prefix_ngram"):
            return lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=PREFIX_STEPS, ngram=tables[int(mode[-1])], lm_weight=LMW)
        return lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, ngram=tables[int(mode[-1])], lm_weight=LMW)

    for mode in modes:
        dec = decoder(mode)
        dec()
        torch.cuda.synchronize()
        rates = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(5):
                dec()
            torch.cuda.synchronize()
            rates.append(5 * B / (time.perf_counter() - t0))
        res[mode + "_utt_per_s"] = [round(r, 1) for r in rates]
    # the step launches alone, on the descriptors the search itself fills (buffers of the cached beam workspace)
    R = B * K
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(1, cfg.vocab_size - 2, (R,), generator=g, dtype=torch.int32).cuda()
    par = torch.randint(0, R, (R,), generator=g, dtype=torch.int32).cuda()
    steps = {}
    if "lm" in modes:
        m = model._beam_lm_desc(lm, LMW, model._beam_ws[2], R)
        steps["lm"] = lambda s: ops.beam_lm_step(m, tok, par, R, s)
    for mode in modes:
        if mode.startswith("ngram"):
            d = model._beam_ngram_desc(tables[int(mode[-1])], LMW, model._beam_ws[2], R)
            steps[mode] = (lambda d: lambda s: ops.beam_ngram_step(d, tok, par, R, s))(d)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for mode, fn in steps.items():
        for s in range(8):
            fn(s)
        us = []
        for _ in range(reps):
            e0.record()
            for s in range(200):
                fn(s + 8)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / 200)
        res[mode + "_step_us"] = [round(u, 2) for u in us]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="plain,lm,ngram2,ngram4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.one:
        one(os.path.abspath(a.root), a.modes.split(","), a.reps)
        return
    me = os.path.abspath(__file__)
    run = lambda root, modes: subprocess.run([sys.executable, me, "--one", "--root", root, "--modes", modes, "--reps", str(a.reps)],
                                             check=True, timeout=280)
    run(HERE, a.modes)                                        # fresh child processes, never two at once
    if a.compare_root:
        for _ in range(a.rounds):                             # other, this, other, this, ...
            for root in (os.path.abspath(a.compare_root), HERE):
                run(root, "plain,lm,prefix_ngram4")


if __name__ == "__main__":
    main()

"""What a back-off n-gram fused into the CTC prefix beam search costs (Seq2SeqModel.ctc_prefix_beam_search(ngram=...),
csrc/ctc_prefix_ngram.hip) next to the plain search and the LSTM-fused one, and that sharing the search between the two fused kernels
(now csrc/ctc_prefix_search.h) left the plain and the LSTM-fused search where they were.

    python tools/ctc_prefix_ngram_cost.py                      # this tree: in ONE process per head the plain, the LSTM-fused and the
                                                               #   n-gram launches (orders 2 and 4) by device events, and decodes/s
    python tools/ctc_prefix_ngram_cost.py --compare-root DIR   # + the plain and the LSTM-fused search of another checkout (built; the
                                                               #   parent commit), child processes ALTERNATED with this tree's

Shape: tools/ctc_prefix_lm_cost.py's c2 workload (B = 64, T_a = 500 x 80, beam width 10, V = 31, max_steps = 150), its 1 x 256 / 128 LSTM
language model, all of random weights, and its two heads: the random one (flat rows: nearly every frame keeps an extension, so nearly
every frame runs the model's step -- the dearest case) and the same with + 8 on the blank's bias.  The n-grams are ngram.estimate
(Witten-Bell) on 2000 random label rows of 5 to 40 units drawn from a first-order chain with a skewed unigram; the arc counts are
reported.  Rates are host-clock times around whole model-level decodes (encoders included) that end with the ids on the host, after a
warm-up; the launches alone are timed by device events on the model's own head logits.  One JSON line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, FA, K, STEPS, LMW = 64, 500, 80, 10, 150, 0.3


def _ngram_tables(cfg, order):
    import numpy as np
    from avsr_tf1_amd import ngram
    V = cfg.vocab_size
    ud = {0: "MASK", -1: "END", cfg.eos_id: "EOS", cfg.go_id: "GO"}
    real = [i for i in range(1, V) if i not in (cfg.eos_id, cfg.go_id)]
    ud.update({i: "u%d" % i for i in real})
    rng = np.random.default_rng(7)
    p = 1.0 / (1.0 + np.arange(len(real)))
    p /= p.sum()
    rows = []
    for _ in range(2000):
        n = int(rng.integers(5, 41))
        s = [int(rng.choice(len(real), p=p))]
        for _ in range(n - 1):                                 # a chain: half the time the successor is tied to the unit before it
            s.append((s[-1] * 7 + 3) % len(real) if rng.random() < 0.5 else int(rng.choice(len(real), p=p)))
        rows.append([real[i] for i in s])
    return ngram.compile_tables(ngram.estimate(rows, order, ud), V, cfg.go_id, cfg.eos_id)


def one(root, modes, reps, shift):
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
    if shift:
        W = model.export_tf_weights()
        W["audio/ctc/bias"] = W["audio/ctc/bias"].copy()
        W["audio/ctc/bias"][cfg.vocab_size] += shift
        model = Seq2SeqModel(cfg, seed=0, weights=W)
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    batch = Batch(audio=t(rng.standard_normal((B, TA, FA)), torch.float32), audio_len=t(np.full(B, TA), torch.int32))
    res = {"root": os.path.relpath(root, HERE), "B": B, "K": K, "T_a": TA, "max_steps": STEPS, "blank_shift": shift, "lm_weight": LMW}
    lm, tables = None, {}
    if "prefix_lm" in modes:
        lcfg = ModelConfig(architecture="lm", video_units=None, audio_units=None, decoder_units=(256,), embedding_size=128,
                           vocab_size=cfg.vocab_size, go_id=cfg.go_id, eos_id=cfg.eos_id, use_dropout=False, sampling_probability=0.0,
                           warmup_steps=0)
        lm = Seq2SeqModel(lcfg, seed=1)
        res["lm"] = "1x256/128"
    for mode in modes:
        if mode.startswith("prefix_ngram"):
            o = int(mode[len("prefix_ngram"):])
            tables[mode] = _ngram_tables(cfg, o)
            res["ngram%d_nodes_arcs" % o] = [int(tables[mode]["n_nodes"]), int(tables[mode]["n_arcs"])]

    def decoder(mode):
        if mode == "prefix":
            return lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS)
        if mode == "prefix_lm":
            return lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS, lm=lm, lm_weight=LMW)
        return lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS, ngram=tables[mode], lm_weight=LMW)

    for mode in modes:
        dec = decoder(mode)
        out = dec()
        torch.cuda.synchronize()
        res["len_" + mode] = max(len(s) for s in out)
        if mode != "prefix":
            res["steps_mean_" + mode] = round(float(model._last_ctc_lm_steps.float().mean()), 1)
        rates = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(5):
                dec()
            torch.cuda.synchronize()
            rates.append(5 * B / (time.perf_counter() - t0))
        res[mode + "_utt_per_s"] = [round(r, 1) for r in rates]
    # the launches alone, on the head logits the decodes left in the workspace
    ws = model._get_ws(B, model._audio_rows(batch), 0, 1, True)
    E = ws["enc"]["audio"]
    ids, lens, score = E[("ctc_prefix", K, STEPS)]
    T, V = E["T"], cfg.vocab_size
    launch = {"prefix": lambda: ops.ctc_prefix_search(E["ctc_z"], V + 1, E["len"], B, T, V, K, STEPS, ids, lens, score),
              "prefix_lm": lambda: model._ctc_prefix_lm_launch(E, V + 1, B, V, K, STEPS, ids, lens, score, lm, LMW, 0.0)}
    for mode in tables:
        launch[mode] = (lambda m: lambda: model._ctc_prefix_ngram_launch(E, V + 1, B, V, K, STEPS, ids, lens, score, tables[m], LMW, 0.0))(mode)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for mode in modes:
        launch[mode]()
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            e0.record()
            for _ in range(5):
                launch[mode]()
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / 5)
        res[mode + "_launch_us"] = [round(u, 1) for u in us]
    res["T"] = T
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="prefix,prefix_lm,prefix_ngram2,prefix_ngram4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shift", type=float, default=0.0)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.one:
        one(os.path.abspath(a.root), a.modes.split(","), a.reps, a.shift)
        return
    me = os.path.abspath(__file__)
    run = lambda root, modes, shift: subprocess.run([sys.executable, me, "--one", "--root", root, "--modes", modes, "--reps", str(a.reps),
                                                     "--shift", str(shift)], check=True, timeout=280)
    for shift in (0.0, 8.0):                                  # fresh child processes, never two at once
        run(HERE, a.modes, shift)
    if a.compare_root:
        for _ in range(a.rounds):                             # other, this, other, this, ...
            for root in (os.path.abspath(a.compare_root), HERE):
                run(root, "prefix,prefix_lm", 0.0)


if __name__ == "__main__":
    main()

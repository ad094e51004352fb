"""What the language model fused into the CTC prefix beam search costs (Seq2SeqModel.ctc_prefix_beam_search(lm=...),
csrc/ctc_prefix_lm.hip), and that adding it left the plain search where it was.

    python tools/ctc_prefix_lm_cost.py                      # this tree: the fused launch by device events, mean lm_steps, decodes/s next to
                                                            #   the plain prefix search and 'beam_search' with the same model fused
    python tools/ctc_prefix_lm_cost.py --compare-root DIR   # + the plain prefix search of another checkout (built; the parent commit),
                                                            #   child processes ALTERNATED with this tree's
    python tools/ctc_prefix_lm_cost.py --one --modes prefix_lm --lm-units 512 --lm-emb 128     # one process, another model width

Shape: tools/ctc_prefix_cost.py's c2 workload (B = 64, T_a = 500 x 80, beam width 10, V = 31, max_steps = 150) and a 1 x 256 LSTM language
model with 128-wide embeddings, all of random weights.  Two heads: the random one (flat rows: nearly every frame keeps an extension, so
nearly every frame runs the model's step -- the dearest case) and the same with + 8 on the blank's bias (the blank wins most frames, as on
a trained head; tests/ref_ctc_prefix.py BLANK_SHIFTS).  Rates are host-clock times around whole model-level decodes (encoders included) that
end with the ids on the host, after a warm-up; the launches alone are timed by device events on the model's own head logits.  One JSON
line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, FA, K, STEPS, LMW = 64, 500, 80, 10, 150, 0.3


def one(root, modes, reps, shift, lm_units=256, lm_emb=128):
    sys.path.insert(0, root)
    import numpy as np
    import torch
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
    res = {"root": os.path.relpath(root, HERE), "B": B, "K": K, "T_a": TA, "max_steps": STEPS, "blank_shift": shift}
    lm = None
    if "prefix_lm" in modes or "beam_lm" in modes:
        lcfg = ModelConfig(architecture="lm", video_units=None, audio_units=None, decoder_units=(lm_units,), embedding_size=lm_emb,
                           vocab_size=cfg.vocab_size, go_id=cfg.go_id, eos_id=cfg.eos_id, use_dropout=False, sampling_probability=0.0,
                           warmup_steps=0)
        lm = Seq2SeqModel(lcfg, seed=1)
        res["lm"], res["lm_weight"] = "1x%d/%d" % (lm_units, lm_emb), LMW
    decode = {"beam_lm": lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, lm=lm, lm_weight=LMW).cpu(),
              "prefix": lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS),
              "prefix_lm": lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS, lm=lm, lm_weight=LMW)}
    for mode in modes:
        out = decode[mode]()
        torch.cuda.synchronize()
        res["len_" + mode] = int(out.shape[1]) if mode == "beam_lm" else max(len(s) for s in out)
        rates = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(5):
                decode[mode]()
            torch.cuda.synchronize()
            rates.append(5 * B / (time.perf_counter() - t0))
        res[mode + "_utt_per_s"] = [round(r, 1) for r in rates]
    if "prefix_lm" in modes:
        res["lm_steps_mean"] = round(float(model._last_ctc_lm_steps.float().mean()), 1)
        ws = model._get_ws(B, model._audio_rows(batch), 0, 1, True)
        E = ws["enc"]["audio"]                                                # the head logits the decode above left there
        ids, lens, score = E[("ctc_prefix", K, STEPS)]
        T, V = E["T"], cfg.vocab_size
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us = []
        for _ in range(reps):
            e0.record()
            for _ in range(5):
                model._ctc_prefix_lm_launch(E, V + 1, B, V, K, STEPS, ids, lens, score, lm, LMW, 0.0)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / 5)
        res["prefix_lm_launch_us"] = [round(u, 1) for u in us]
        res["prefix_lm_us_per_lm_step"] = round(min(us) / max(res["lm_steps_mean"], 1.0), 2)
        res["T"] = T
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="prefix,prefix_lm,beam_lm")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shift", type=float, default=0.0)
    ap.add_argument("--lm-units", type=int, default=256)
    ap.add_argument("--lm-emb", type=int, default=128)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.one:
        one(os.path.abspath(a.root), a.modes.split(","), a.reps, a.shift, a.lm_units, a.lm_emb)
        return
    me = os.path.abspath(__file__)
    run = lambda root, modes, shift: subprocess.run([sys.executable, me, "--one", "--root", root, "--modes", modes, "--reps", str(a.reps),
                                                     "--shift", str(shift)], check=True, timeout=280)
    for shift in (0.0, 8.0):                                  # fresh child processes, never two at once
        run(HERE, a.modes, shift)
    if a.compare_root:
        for _ in range(a.rounds):                             # other, this, other, this, ...
            for root in (os.path.abspath(a.compare_root), HERE):
                run(root, "prefix", 0.0)


if __name__ == "__main__":
    main()

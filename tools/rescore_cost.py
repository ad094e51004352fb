"""What attention rescoring (decoding_algorithm='attention_rescoring') costs next to the other three decodes, where its time goes, and
that adding it left beam search and the prefix search where they were.

    python tools/rescore_cost.py                         # this tree: the two launches and one decoder pass by device events;
                                                         #   utterances/s of the four decodes
    python tools/rescore_cost.py --compare-root DIR      # + 'beam_search' and 'ctc_prefix_beam_search' of another checkout (built; the
                                                         #   parent commit), child processes ALTERNATED with this tree's
    python tools/rescore_cost.py --attention scaled_luong   # the same shape with a Luong decoder, whose teacher-forced (mode 0) pass the
                                                         #   fused persistent decoder kernel covers (c2's Bahdanau decoder: modes 1 / 2 only)

Shape: the c2 workload (audio-only, 3 x 256 bidirectional LSTM encoder, Bahdanau decoder, use_ctc=True, B = 64, T_a = 500 x 80), beam
width 10, V = 31, max_steps = 150 as `evaluate` passes it, ctc_weight 0.3.  Random weights: the head's rows are nearly flat, so the
prefix beam holds 10 label sequences per utterance that grow to L_max -- ten teacher-forced passes of 152 steps (150 + EOS, rounded up
to a multiple of 8), the dearest case; the attention decodes never emit EOS and run all 150 steps.
Rates are host-clock times around whole model-level decodes (encoders included) that end with the ids on the host, after a warm-up.
avsr_seq_logprob, avsr_rescore_select and one teacher-forced decoder pass (embedding, input products, the block, the output layer;
keys prepared before) are timed by device events around runs of 10 on the buffers the decode left.  One JSON line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TA, FA, K, STEPS, WEIGHT = 64, 500, 80, 10, 150, 0.3


def one(root, modes, reps, attention="bahdanau"):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    cfg = ModelConfig(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(256, 256, 256),
                      decoder_units=(256,), embedding_size=128, audio_feat=FA, attention_type=((attention,), (attention,)),
                      use_dropout=False, sampling_probability=0.0, use_ctc=True)
    model = Seq2SeqModel(cfg, seed=0)
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    batch = Batch(audio=t(rng.standard_normal((B, TA, FA)), torch.float32), audio_len=t(np.full(B, TA), torch.int32))
    res = {"root": os.path.relpath(root, HERE), "attention": attention, "B": B, "K": K, "T_a": TA, "max_steps": STEPS}
    decode = {"beam": lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS).cpu(),
              "greedy": lambda: model.greedy_decode(batch, max_steps=STEPS).cpu(),
              "prefix": lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS),
              "rescore": lambda: model.attention_rescoring(batch, beam_width=K, max_steps=STEPS, ctc_weight=WEIGHT)}
    for mode in modes:
        out = decode[mode]()
        torch.cuda.synchronize()
        res["len_" + mode] = int(out.shape[1]) if mode in ("beam", "greedy") else max(len(s) for s in out)
        rates = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(5):
                decode[mode]()
            torch.cuda.synchronize()
            rates.append(5 * B / (time.perf_counter() - t0))
        res[mode + "_utt_per_s"] = [round(r, 1) for r in rates]
    if "rescore" in modes:
        from avsr_tf1_amd import ops
        V = cfg.vocab_size
        lr = model._last_rescore
        wsr, D, Lh = lr["ws"], lr["ws"]["dec"], lr["Lh"]
        labels, llen, n = (torch.from_numpy(lr[k]).cuda() for k in ("labels", "labels_len", "n"))
        s_ctc = model._get_ws(B, model._audio_rows(batch), 0, 1, True)["enc"]["audio"][("ctc_prefix", K, STEPS)][2]
        res.update(Lh=Lh, passes=int(lr["n"].max()), hypotheses=int(lr["n"].sum()),
                   decoder_pass_fused=bool(model.fused_decode and ops.attn_rnn_fused_fwd_active(D["desc"])))
        runs = {"seq_logprob_us": lambda: ops.seq_logprob(D["logits_k"][0], labels[0], llen[0], B, Lh, V, D["s_att"], out_stride=K),
                "rescore_select_us": lambda: ops.rescore_select(D["s_att"], s_ctc, n, B, K, WEIGHT, D["order"], D["final"]),
                "decoder_pass_us": lambda: model._decoder_train_pass(wsr, D, labels[0], llen[0], False, with_bwd=False, prepare=False,
                                                                     logits=D["logits_k"][0])}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for name, fn in runs.items():
            fn()
            us = []
            for _ in range(reps):
                e0.record()
                for _ in range(10):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / 10)
            res[name] = [round(u, 1) for u in us]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="beam,greedy,prefix,rescore")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--attention", default="bahdanau", choices=("bahdanau", "scaled_luong"))
    a = ap.parse_args()
    if a.one or not a.compare_root:
        one(os.path.abspath(a.root), a.modes.split(","), a.reps, a.attention)
        return
    me = os.path.abspath(__file__)
    for r in range(a.rounds):                                 # other, this, other, this, ...: fresh child processes, never two at once
        for root, modes in ((os.path.abspath(a.compare_root), "beam,prefix"), (HERE, "beam,prefix,greedy,rescore" if r == 0 else "beam,prefix")):
            subprocess.run([sys.executable, me, "--one", "--root", root, "--modes", modes, "--reps", str(a.reps), "--attention", a.attention], check=True, timeout=280)


if __name__ == "__main__":
    main()

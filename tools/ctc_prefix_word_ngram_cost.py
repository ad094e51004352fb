"""What a word-level n-gram behind a lexicon trie costs inside the CTC prefix beam search
(Seq2SeqModel.ctc_prefix_beam_search(word_ngram=...), csrc/ctc_prefix_word_ngram.hip) next to the plain search and the unit n-gram, and
that adding it left the three existing searches where they were.

    python tools/ctc_prefix_word_ngram_cost.py                      # this tree: in ONE process per head the plain, the unit n-gram
                                                                    #   (order 4) and the word n-gram launches (orders 1 and 3) by device
                                                                    #   events, and whole decodes in utterances/s
    python tools/ctc_prefix_word_ngram_cost.py --compare-root DIR   # + the plain, the LSTM-fused and the n-gram-fused search of another
                                                                    #   checkout (built; the parent commit) through
                                                                    #   tools/ctc_prefix_ngram_cost.py, child processes ALTERNATED with
                                                                    #   this tree's

Shape: tools/ctc_prefix_lm_cost.py's c2 workload (B = 64, T_a = 500 x 80, beam width 10, V = 31, max_steps = 150) of random weights and
its two heads: the random one (flat rows: nearly every frame keeps an extension, so nearly every frame runs the model's step -- the
dearest case) and the same with + 8 on the blank's bias.  The units are the character list (', space, a-z).  The vocabulary is
synthetic: 3000 distinct random words of 2 to 8 letters with a skewed letter distribution; the word models are ngram.estimate
(Witten-Bell) of orders 1 and 3 on 4000 random sentences of 3 to 12 words with a skewed word distribution, <unk> in the vocabulary; the
table sizes are reported.  No target is set: nothing about this kernel's time had been measured before.  Rates are host-clock times
around whole model-level decodes (encoders included) that end with the ids on the host, after a warm-up; the launches alone are timed
by device events on the model's own head logits.  One JSON line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
B, TA, FA, K, STEPS, LMW = 64, 500, 80, 10, 150, 0.3


def _word_tables(cfg, order):
    import numpy as np
    from avsr_tf1_amd import ngram
    ud = {0: "MASK", -1: "END", 1: "'", 2: " ", cfg.eos_id: "EOS", cfg.go_id: "GO"}
    ud.update({3 + i: chr(ord("a") + i) for i in range(26)})
    assert len(ud) - 1 == cfg.vocab_size
    rng = np.random.default_rng(11)
    p = 1.0 / (1.0 + np.arange(26))
    p /= p.sum()
    words = set()
    while len(words) < 3000:
        words.add("".join(chr(ord("a") + int(c)) for c in rng.choice(26, size=int(rng.integers(2, 9)), p=p)))
    vocabulary = [ngram.WORD_BOS, ngram.WORD_EOS] + sorted(words | {ngram.WORD_UNK[0]})
    real = [i for i, w in enumerate(vocabulary) if i >= 2 and w != ngram.WORD_UNK[0]]
    q = 1.0 / (1.0 + np.arange(len(real)))
    q /= q.sum()
    rows = [[real[int(i)] for i in rng.choice(len(real), size=int(rng.integers(3, 13)), p=q)] for _ in range(4000)]
    return ngram.compile_word_tables(ngram.estimate(rows, order, ngram.word_dict(vocabulary)), vocabulary, ud)


def one(root, modes, reps, shift):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from ctc_prefix_ngram_cost import _ngram_tables
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
    res = {"B": B, "K": K, "T_a": TA, "max_steps": STEPS, "blank_shift": shift, "lm_weight": LMW}
    tables = {}
    for mode in modes:
        if mode.startswith("prefix_ngram"):
            o = int(mode[len("prefix_ngram"):])
            tables[mode] = _ngram_tables(cfg, o)
            res["ngram%d_nodes_arcs" % o] = [int(tables[mode]["n_nodes"]), int(tables[mode]["n_arcs"])]
        if mode.startswith("prefix_word"):
            o = int(mode[len("prefix_word"):])
            g = tables[mode] = _word_tables(cfg, o)
            res["word%d_words_nodes_arcs_trie_nodes_arcs" % o] = [int(g[k]) for k in ("Vw", "n_nodes", "n_arcs", "n_trie_nodes", "n_trie_arcs")]
            res["oov_score"] = g["oov_score"]

    def decoder(mode):
        if mode == "prefix":
            return lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS)
        if mode.startswith("prefix_word"):
            return lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=STEPS, word_ngram=tables[mode], lm_weight=LMW)
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
    launch = {"prefix": lambda: ops.ctc_prefix_search(E["ctc_z"], V + 1, E["len"], B, T, V, K, STEPS, ids, lens, score)}
    for mode in tables:
        fn = model._ctc_prefix_word_ngram_launch if mode.startswith("prefix_word") else model._ctc_prefix_ngram_launch
        launch[mode] = (lambda f, m: lambda: f(E, V + 1, B, V, K, STEPS, ids, lens, score, tables[m], LMW, 0.0))(fn, mode)
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
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="prefix,prefix_ngram4,prefix_word1,prefix_word3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shift", type=float, default=0.0)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.one:
        one(HERE, a.modes.split(","), a.reps, a.shift)
        return
    me = os.path.abspath(__file__)
    for shift in (0.0, 8.0):                                  # fresh child processes, never two at once
        subprocess.run([sys.executable, me, "--one", "--modes", a.modes, "--reps", str(a.reps), "--shift", str(shift)], check=True, timeout=280)
    if a.compare_root:
        old = os.path.join(HERE, "tools", "ctc_prefix_ngram_cost.py")
        for _ in range(a.rounds):                             # other, this, other, this, ...
            for root in (os.path.abspath(a.compare_root), HERE):
                subprocess.run([sys.executable, old, "--one", "--root", root, "--modes", "prefix,prefix_lm,prefix_ngram4", "--reps", str(a.reps),
                                "--shift", "0.0"], check=True, timeout=280)


if __name__ == "__main__":
    main()

"""What a word-level n-gram behind a lexicon trie costs inside beam search (Seq2SeqModel.beam_search_decode(word_ngram=...),
csrc/beam_word_ngram.hip) next to the plain search, the unit n-gram and the LSTM, and that adding it left the searches that existed
where they were.

    python tools/beam_word_ngram_cost.py                      # this tree, ONE process: plain, LSTM, unit n-gram (order 4) and word n-gram
                                                              #   (orders 1 and 3) decodes/s, and the three models' step launches by
                                                              #   device events
    python tools/beam_word_ngram_cost.py --compare-root DIR   # + another checkout (built; the parent commit), child processes ALTERNATED
                                                              #   with this tree's: plain 'beam_search', 'beam_search' with the unit
                                                              #   n-gram, and the CTC prefix search with its word n-gram (whose kernel
                                                              #   now includes the shared header)

Shape: tools/beam_ngram_cost.py's c2 evaluation batch (B = 64, T_a = 500 x 80, beam width 10 -> 640 hypothesis rows, V = 31, 40 steps;
random weights never emit EOS, so every step runs), its 1 x 256 / 128 LSTM and its order-4 unit n-gram, and
tools/ctc_prefix_word_ngram_cost.py's synthetic vocabulary (3000 random words of 2 to 8 letters, Witten-Bell word models of orders 1
and 3 on 4000 random sentences, <unk> in the vocabulary; the table sizes are reported).  Rates are host-clock times around whole decodes
that end in a device synchronise, after a warm-up decode; a step launch is timed by device events around 200 back-to-back launches.  The
word step's symbols are drawn so that the rows sit at roots, inside words and in the sink (a random letter per row would put all of
them in the sink within two steps): before every timed block the rows are re-seeded by step 0 and walked three random letters, a
space for a quarter of them and two more letters, and the timed launches alternate letters and spaces.  No target is set.  One JSON
line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
B, TA, FA, K, STEPS, PREFIX_STEPS, LMW = 64, 500, 80, 10, 40, 150, 0.3


def one(root, modes, reps):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from ctc_prefix_ngram_cost import _ngram_tables
    from ctc_prefix_word_ngram_cost import _word_tables
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
        o = int(mode[-1]) if mode[-1].isdigit() else 0
        if mode.endswith("word%d" % o):
            g = tables[mode] = _word_tables(cfg, o)
            res["word%d_words_nodes_arcs_trie_nodes_arcs" % o] = [int(g[k]) for k in ("Vw", "n_nodes", "n_arcs", "n_trie_nodes", "n_trie_arcs")]
        elif o:
            tables[mode] = _ngram_tables(cfg, o)
            res["ngram%d_nodes_arcs" % o] = [int(tables[mode]["n_nodes"]), int(tables[mode]["n_arcs"])]

    def decoder(mode):
        if mode == "plain":
            return lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS)
        if mode == "lm":
            return lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, lm=lm, lm_weight=LMW)
        if mode.startswith("prefix_word"):
            return lambda: model.ctc_prefix_beam_search(batch, beam_width=K, max_steps=PREFIX_STEPS, word_ngram=tables[mode], lm_weight=LMW)
        if mode.startswith("word"):
            return lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, word_ngram=tables[mode], lm_weight=LMW)
        return lambda: model.beam_search_decode(batch, beam_width=K, max_steps=STEPS, ngram=tables[mode], lm_weight=LMW)

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
    R, V = B * K, cfg.vocab_size
    g = torch.Generator().manual_seed(3)
    skew = 1.0 / (1.0 + torch.arange(26, dtype=torch.float32))            # the vocabulary's own letter distribution (a is class 3)
    letters = [(3 + torch.multinomial(skew, R, replacement=True, generator=g)).to(torch.int32).cuda() for _ in range(8)]
    par = torch.randint(0, R, (R,), generator=g, dtype=torch.int32).cuda()
    ident = torch.arange(R, dtype=torch.int32).cuda()
    some_space = torch.where(torch.rand(R, generator=g).cuda() < 0.25, torch.full_like(letters[0], 2), letters[0])
    all_space = torch.full_like(letters[0], 2)
    steps, seed = {}, {}
    if "lm" in modes:
        m = model._beam_lm_desc(lm, LMW, model._beam_ws[2], R)
        steps["lm"] = lambda s: ops.beam_lm_step(m, letters[s % 8], par, R, s)
    for mode in modes:
        if mode.startswith("ngram"):
            d = model._beam_ngram_desc(tables[mode], LMW, model._beam_ws[2], R)
            steps[mode] = (lambda d: lambda s: ops.beam_ngram_step(d, letters[s % 8], par, R, s))(d)
        if mode.startswith("word"):
            d = model._beam_word_ngram_desc(tables[mode], LMW, model._beam_ws[2], R)
            # letters with identity parents keep roots, words in progress and sunk rows apart; every eighth launch closes the words
            steps[mode] = (lambda d: lambda s: ops.beam_word_ngram_step(d, all_space if s % 8 == 7 else letters[s % 8], ident, R, s))(d)

            def reseed(d=d):
                ops.beam_word_ngram_step(d, letters[0], ident, R, 0)
                for s, tk in enumerate([letters[1], letters[2], letters[3], some_space, letters[4], letters[5]]):
                    ops.beam_word_ngram_step(d, tk, ident, R, s + 1)
            seed[mode] = reseed
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for mode, fn in steps.items():
        for s in range(8):
            fn(s)
        us = []
        for _ in range(reps):
            if mode in seed:
                seed[mode]()
            e0.record()
            for s in range(200):
                fn(s + 7)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / 200)
        res[mode + "_step_us"] = [round(u, 2) for u in us]
        if mode in seed:                                      # where the rows of the timed block sat after the re-seeding
            seed[mode]()
            torch.cuda.synchronize()
            p = model._beam_ws[2]["word_ngram"]["state"][1, 1].cpu().numpy()      # six steps after step 0: the half (6 + 1) & 1 = 1
            res[mode + "_rows_root_inside_sink"] = [int((p == 0).sum()), int((p > 0).sum()), int((p < 0).sum())]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--modes", default="plain,lm,ngram4,word1,word3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--compare-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.one:
        one(os.path.abspath(a.root), a.modes.split(","), a.reps)
        return
    me = os.path.abspath(__file__)
    run = lambda root, modes: subprocess.run([sys.executable, me, "--one", "--root", root, "--modes", modes, "--reps", str(a.reps)],
                                             check=True, timeout=400)
    run(HERE, a.modes)                                        # fresh child processes, never two at once
    if a.compare_root:
        for _ in range(a.rounds):                             # other, this, other, this, ...
            for root in (os.path.abspath(a.compare_root), HERE):
                run(root, "plain,ngram4,prefix_word3")


if __name__ == "__main__":
    main()

"""The regime fixtures, checked on the CPU oracle alone (no GPU): every entry of FIXTURES must put the fp64 oracle where a TRAINED model
runs -- peaked alignments spread over the chunks of a chunked memory, cells at the clip, logits tens apart, softmax entries outside the
focal / mc clamp -- and must stay testable there: far enough from every discontinuity (clip margin, clamp bounds, argmax gaps) and
calm enough (fp32 oracle vs fp64 oracle) that an fp32 engine can be held to the suite's usual tolerances.  tests/test_gpu_regime.py
runs the engine on this table and takes, per quantity, the bound max(T_suite, 8 x noise) with the noise `regime.fp32_noise` reports.  Run with -s
to see each fixture's numbers.

Factors and seeds were chosen on the CPU until the oracle satisfied the conditions below; the caps are the conditions, not the outcome.
"""
import numpy as np
import pytest

import regime as R
from regime import Fixture

_BAHDANAU = (("v", 18.0), ("memory_kernel", 3.0), ("query_kernel", 3.0))        # v carries the score range, the kernels saturate the tanh

# What the fp64 oracle measures per fixture (train pass; noise = fp32 oracle vs fp64 oracle; run this module with -s for the full figures):
#   mean peak and rows peaking in the first / last chunk: per mechanism, video / attentive layer first | clipped, margin: share of LSTM cells at the clip, smallest | |c_pre| - 1 | |
#   worst noise: largest gap over logits, loss, global norm and every gradient, relative to max(1e-3, |ref|max) (cap 1.25e-5) |
#   logits / greedy logits / alignments noise: absolute, what the GPU module's bounds max(T_suite, 8 x noise) are made of | gaps: smallest top-1 to
#   top-2 logit gap of the greedy and of the beam steps (must be >= 100 x the logits' noise)
#
#   fixture                       mean peak  first/last    clipped  margin  max|logit|  worst    logits   greedy / align     greedy   beam
#                                            chunk peaks                               noise    noise    noise              gap      gap
#  bimodal_scaled_luong          0.91 0.58  24/7 31/0     10.9 %  1.1e-04   24.3  8.1e-06  5.7e-05  5.2e-05 / 3.8e-06  2.1e-01  1.9e-02
#      per cell kernel, clipped % (margin): video/fw/l0 8.6 (2e-04), audio/fw/l0 9.7 (1e-04), audio/fw/l1 11.8 (1e-04), dec/l0 13.3 (2e-03)
#  gru_av_align                  0.91 0.68  210/89 28/3     gru      -      22.4  7.9e-06  2.8e-05  4.8e-05 / 9.7e-06  7.4e-02  1.4e-02
#  lstm_av_align_bahdanau_luong  0.88 0.72  225/74 21/10  11.8 %  1.6e-04   19.4  4.0e-06  2.2e-05  2.9e-05 / 2.5e-06  4.7e-02  1.2e-02
#      per cell kernel, clipped % (margin): video/fw/l0 9.0 (3e-03), audio/fw/l0 16.6 (2e-04), dec/l0 9.6 (6e-04)
#  dec2_luong                    0.62       26/5          10.0 %  1.7e-04   15.8  1.1e-05  3.0e-05  4.4e-05 / 3.3e-06  2.4e-02  1.7e-02
#      per cell kernel, clipped % (margin): audio/fw/l0 10.7 (2e-04), audio/fw/l1 12.0 (2e-04), dec/l0 10.3 (5e-03), dec/l1 7.1 (9e-04)
#  loss_focal                    0.86       28/3          11.2 %  2.8e-04   18.3  9.6e-06  4.0e-05  3.5e-05 / 2.9e-06  6.5e-02  1.1e-02
#      per cell kernel, clipped % (margin): audio/fw/l0 12.0 (3e-04), dec/l0 10.4 (1e-03)
#  loss_mc_bimodal               0.76 0.79  20/11 31/0    10.9 %  1.6e-04   18.1  5.0e-06  1.8e-05  3.2e-05 / 2.7e-06  2.8e-02  1.6e-02
#      per cell kernel, clipped % (margin): video/fw/l0 8.3 (2e-04), audio/fw/l0 10.8 (4e-04), dec/l0 13.7 (2e-03)
#  label_smoothing_bahdanau      0.80       25/6          13.8 %  1.4e-04   18.9  1.8e-06  8.5e-06  2.6e-05 / 1.3e-06  5.0e-02  1.7e-02
#      per cell kernel, clipped % (margin): audio/fw/l0 12.8 (1e-04), dec/l0 14.8 (5e-04)
#  bi_bahdanau_three_chunks      0.78       22/3          13.4 %  1.8e-04   15.0  4.2e-06  3.0e-05  5.7e-05 / 5.5e-06  1.4e-02  1.4e-02
#      per cell kernel, clipped % (margin): audio/fw/l0 10.7 (4e-04), audio/bw/l0 13.4 (2e-04), dec/l0 15.9 (4e-04)
#  bimodal_dropout_sampling      0.86 0.76  26/5 31/0     10.3 %  1.7e-04   23.6  6.0e-06  3.1e-05  5.7e-05 / 2.9e-06  8.3e-02  9.9e-03
#      per cell kernel, clipped % (margin): video/fw/l0 9.8 (5e-04), audio/fw/l0 10.4 (3e-04), audio/fw/l1 11.1 (2e-04), dec/l0 9.8 (2e-03)
#
# B = 5, 32 units, L = 7; T_a = 70 -> chunks of 64 + 6 frames, T_v = 21 -> chunks of 16 + 5 frames; batch seed 1063 has ragged lengths
# with three audio memories reaching the last chunk and two ending inside the first
FIXTURES = [
    # bimodal, unidirectional LSTM, two scaled_luong mechanisms (g and the memory kernel multiply: score x 20)
    Fixture("bimodal_scaled_luong", "c4_bimodal_uni", attn=4.5, cell=3.0, out=20.0, seed=161, batch_seed=1063),
    # AV-Align, GRU: scaled_luong attentive layer (score x 32) + normed_bahdanau decoder mechanism (its g alone carries the range)
    Fixture("gru_av_align", "gru_av_align", attn=(("memory_kernel", 2.0), ("query_kernel", 2.0), ("g", 8.0), ("dec/att0/g", 70.0)),
            cell=1.5, out=20.0, seed=104, batch_seed=1063),
    # AV-Align, LSTM: bahdanau attentive layer, luong decoder mechanism (linear in the memory kernel only)
    Fixture("lstm_av_align_bahdanau_luong", "av_align_1layer_bahdanau", attn=_BAHDANAU + (("dec/att0/memory_kernel", 20.0),),
            cell=3.0, out=20.0, seed=192, batch_seed=1063),
    # two-layer decoder, luong
    Fixture("dec2_luong", "dec2_unimodal", over=(("attention_type", (("luong",), ("luong",))),), attn=20.0, cell=3.0, out=20.0, seed=24,
            batch_seed=1063),
    Fixture("loss_focal", "loss_focal", attn=5.0, cell=3.2, out=14.0, seed=172, batch_seed=1063),
    Fixture("loss_mc_bimodal", "loss_mc_bimodal", attn=4.0, cell=3.0, out=16.0, seed=92, batch_seed=1063),
    Fixture("label_smoothing_bahdanau", "label_smoothing", attn=_BAHDANAU, cell=3.5, out=20.0, seed=5, batch_seed=1063),
    # unimodal BIDIRECTIONAL encoder, bahdanau, T_a = 130: three chunks (64 + 64 + 2); three memories of 129 / 130 frames (the last chunk
    # holds one or two frames of them), one that ends inside the second chunk and one inside the first (two empty partials in one merge)
    Fixture("bi_bahdanau_three_chunks", "label_smoothing", over=(("encoder_type", "bidirectional"),), attn=_BAHDANAU, cell=3.5, out=20.0,
            seed=193, batch_seed=1232, Ta=130, audio_len=(129, 129, 130, 90, 50)),
    # DropoutWrapper on every cell + scheduled sampling: the sampler's inverse-CDF draw at peaked distributions
    Fixture("bimodal_dropout_sampling", "c4_bimodal_uni", over=(("sampling_probability", 0.25), ("use_dropout", True)), attn=4.0, cell=3.0,
            out=20.0, seed=186, batch_seed=1063),
]
IDS = [fx.name for fx in FIXTURES]

NOISE_CAP = 1.25e-5          # fp32 oracle vs fp64 oracle, relative; 8 x this = 1e-4 = half of the suite's 2e-4 gradient tolerance
CLIP_MARGIN = 1e-4           # closer to the clip than this and an fp32 kernel may legitimately land on the other side of it
GAP_FACTOR = 100.0           # argmax gaps vs the logits' fp32 noise: bit-exact ids are then a fair demand


def _describe(fx):
    s, n = R.stats(fx), R.reference(fx)
    lines = ["%s: case %s, attn %s, cell %s, out %s, seed %d / batch seed %d" % (fx.name, fx.case, fx.attn, fx.cell, fx.out, fx.seed, fx.batch_seed)]
    for p, m in s["mech"].items():
        pk, ch = m["peak"][m["valid"]], m["chunk"][m["valid"]]
        lines.append("  %-15s peak mean %.3f max %.6f min %.3f | rows peaking in chunk 0: %d, in the last of %d chunks: %d | memory lengths %s"
                     % (p, pk.mean(), pk.max(), pk.min(), (ch == 0).sum(), m["n_chunks"], (ch == m["n_chunks"] - 1).sum(), m["lens"].tolist()))
    for k, c in s["cells"].items():
        clip = "-" if c["clipped"] is None else "clipped %.1f %% margin %.2e" % (100 * c["clipped"], c["margin"])
        lines.append("  %-28s %s | gates with |z| > 4: %.1f %%" % (k, clip, 100 * c["saturated"]))
    lines.append("  logits in [%.2f, %.2f]" % (s["loss"]["logit_min"], s["loss"]["logit_max"])
                 + ("" if "clamp_outside" not in s["loss"] else " | softmax entries outside the clamp: %d of %d, nearest at a relative %.2e of a bound"
                    % (s["loss"]["clamp_outside"], s["loss"]["clamp_total"], s["loss"]["clamp_rel_dist"])))
    d = s["decode"]
    lines.append("  top-1 to top-2 gap: greedy %.2e (%d steps, %d utterances finished), beam %s | candidate score gaps %s"
                 % (d["greedy_gap"], d["greedy_steps"], d["greedy_finished"], {k: "%.2e" % v for k, v in d["beam_gap"].items()},
                    {k: "%.2e" % v for k, v in d["beam_score_gap"].items()}))
    w = R.worst_noise(n)
    lines.append("  fp32 noise: logits %.2e abs / %.2e rel, loss %.2e, global norm %.2e rel (norm %.4g), worst %.2e (%s), params %.2e abs | "
                 "greedy logits %.2e abs, alignments %.2e abs" % (n["logits"]["abs"], n["logits"]["rel"], n["loss"]["abs"], n["global_norm"]["rel"],
                                                                n["ref"]["global_norm"], w[0], w[1], max(v["abs"] for v in n["params"].values()),
                                                                n["greedy_logits"]["abs"], n["align"]["abs"]))
    return "\n".join(lines)


def _lstm(fx):
    return [c for c in R.stats(fx)["cells"].values() if c["clipped"] is not None]


def test_fixture_table_covers_the_options():
    cfgs = [R.build(fx)[1] for fx in FIXTURES]
    types = {t for c in cfgs for pair in c.attention_type for t in pair if c.enable_attention}
    used = set()
    for c in cfgs:
        used |= {t for _s, t in c.decoder_memories()}
        if c.architecture == "av_align":
            used.add(c.attention_type[0][0])
    assert used == {"luong", "scaled_luong", "bahdanau", "normed_bahdanau"}, (used, types)
    assert {c.cell_type for c in cfgs} == {"lstm", "gru"}
    assert any(c.architecture == "unimodal" and c.encoder_type == "bidirectional" for c in cfgs)
    assert {"bimodal", "av_align"} <= {c.architecture for c in cfgs}
    assert any(len(c.decoder_units) == 2 for c in cfgs)
    assert {"loss_focal", "loss_mc_bimodal", "label_smoothing"} <= {fx.case for fx in FIXTURES}
    assert any(c.use_dropout and c.sampling_probability > 0 for c in cfgs)
    assert any(fx.Ta == 130 for fx in FIXTURES) and all(fx.B == 5 and fx.L == 7 and fx.Tv == 21 for fx in FIXTURES)


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_fixture_is_in_the_regime(fx):
    s = R.stats(fx)
    msg = _describe(fx)
    print("\n" + msg)
    peaks = np.concatenate([m["peak"][m["valid"]] for m in s["mech"].values()])
    for p, m in s["mech"].items():
        assert m["peak"][m["valid"]].mean() >= 0.5, (p, msg)                      # every mechanism is peaked on average
    assert peaks.max() >= 0.99 and peaks.min() < 0.5, msg                          # one-hot rows next to spread ones
    chunked = [m for m in s["mech"].values() if m["n_chunks"] > 1]
    assert chunked, msg
    assert sum(int((m["chunk"][m["valid"]] == 0).sum()) for m in chunked) > 0, msg
    assert sum(int((m["chunk"][m["valid"]] == m["n_chunks"] - 1).sum()) for m in chunked) > 0, msg
    # a memory that ends inside the first chunk leaves every later chunk empty: the -INFINITY partials of the merge
    assert any((m["lens"] <= m["chunk_len"]).any() for m in chunked), msg
    if fx.Ta == 130:
        assert any(m["n_chunks"] == 3 for m in chunked), msg
    lstm = _lstm(fx)
    if lstm:
        assert np.mean([c["clipped"] for c in lstm]) >= 0.10, msg
        assert min(c["clipped"] for c in lstm) >= 0.05, msg                        # no cell kernel (encoder layer, decoder layer) sits the regime out
        assert min(c["margin"] for c in lstm) >= CLIP_MARGIN, msg
    assert s["loss"]["logit_absmax"] >= 10.0, msg
    if R.build(fx)[1].loss_fun in ("focal_loss", "mc_loss"):
        assert s["loss"]["clamp_outside"] >= 0.01 * s["loss"]["clamp_total"], msg
        assert s["loss"]["clamp_rel_dist"] >= 1e-3, msg


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_fixture_is_testable_in_fp32(fx):
    s, n = R.stats(fx), R.reference(fx)
    msg = _describe(fx)
    worst, where = R.worst_noise(n)
    assert worst <= NOISE_CAP, (where, worst, msg)
    assert n["fed_equal"], msg                                                     # the sampler drew the same tokens at fp32 and fp64
    assert n["greedy_ids_equal"], msg
    noise = max(n["logits"]["abs"], n["greedy_logits"]["abs"])                     # train-graph and eval-graph logits
    d = s["decode"]
    assert d["greedy_gap"] >= GAP_FACTOR * noise, msg
    for K, g in d["beam_gap"].items():
        assert g >= GAP_FACTOR * noise, (K, msg)

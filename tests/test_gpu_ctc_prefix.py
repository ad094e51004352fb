"""CTC prefix beam search on the GPU: the kernel through the C ABI (every frame of its trace followed by the fp64 checker of
tests/ref_ctc_prefix.py, then whole searches against the fp64 dictionary search where the reference's margins allow it), then
Seq2SeqModel.ctc_prefix_beam_search on the oracle's evaluation-mode head logits and the AVSR front door.

Tolerances are ref_ctc_prefix's: TOL_STEP / TOL_STEP_LONG per frame, TOL_SEARCH for final scores (8 x what the float32 restatement of
the rule deviates from fp64 on these very inputs).  A whole search is compared only where the reference's smallest pruning-boundary and
final top-1 / top-2 margin exceeds TOL_SEARCH -- a search is discontinuous at a tie -- and at most a third of a configuration's 64 seeds
may be left out for that; the trace check leaves out nothing."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_ctc as RC  # noqa: E402
import ref_ctc_prefix as R  # noqa: E402
from test_ctc_prefix_cpu import REENTRY  # noqa: E402

pytestmark = pytest.mark.gpu
NEG = -np.inf
_CACHE = {}


def _launch(z, in_len, V, W, L_max, trace=True, fill=77.0, tail=64):
    """z [B, T, ld] float32 (ld >= V + 1).  Outputs are allocated `tail` elements too long and pre-filled, so that what the kernel leaves
    alone can be seen.  Returns dict(ids [B, W, L_max], lens, score [B, W], parent / sym / pb / pnb [B, T, W], tails)."""
    from avsr_tf1_amd import ops
    B, T, ld = z.shape
    dev = "cuda"
    zd = torch.tensor(np.ascontiguousarray(z).reshape(B * T, ld), device=dev)
    ld_ = torch.tensor(np.asarray(in_len, np.int32), device=dev)
    ids = torch.full((B * W * L_max + tail,), int(fill), dtype=torch.int32, device=dev)
    lens = torch.full((B * W + tail,), int(fill), dtype=torch.int32, device=dev)
    score = torch.full((B * W + tail,), float(fill), device=dev)
    tr = None
    if trace:
        tr = (torch.full((B * T * W + tail,), int(fill), dtype=torch.int32, device=dev), torch.full((B * T * W + tail,), int(fill), dtype=torch.int32, device=dev),
              torch.full((B * T * W + tail,), float(fill), device=dev), torch.full((B * T * W + tail,), float(fill), device=dev))
    ops.ctc_prefix_search(zd, ld, ld_, B, T, V, W, L_max, ids, lens, score, trace=tr)
    torch.cuda.synchronize()
    out = dict(ids=ids.cpu().numpy(), lens=lens.cpu().numpy(), score=score.cpu().numpy())
    if trace:
        out.update(zip(("parent", "sym", "pb", "pnb"), (t.cpu().numpy() for t in tr)))
    res = {}
    for k, v in out.items():
        n = v.size - tail
        assert (v[n:] == (int(fill) if v.dtype.kind == "i" else np.float32(fill))).all(), ("written past the end of", k)
        res[k] = v[:n].reshape((B, W, L_max) if k == "ids" else (B, W) if k in ("lens", "score") else (B, T, W))
    return res


def _final_of(out, b, W):
    """[(labels, score)] of utterance b as the kernel returned it, after checking the padding rules of the output."""
    beam = []
    for r in range(W):
        n, p = int(out["lens"][b, r]), float(out["score"][b, r])
        row = out["ids"][b, r]
        assert not np.isnan(p)
        if p == NEG:
            assert n == 0 and (row == -1).all() and (out["score"][b, r:] == NEG).all(), ("an empty slot", b, r)
            continue
        assert (row[n:] == -1).all() and (row[:n] >= 0).all()
        beam.append((tuple(int(s) for s in row[:n]), p))
    return beam


def _check_utterance(out, b, z, Tb, V, W, L_max, tol):
    """Trace check of utterance b (z [T, V + 1]) plus: the returned beam IS the last frame's beam."""
    T = z.shape[0]
    Tb = min(max(int(Tb), 0), T)
    final = R.check_trace(z, Tb, W, L_max, out["parent"][b], out["sym"][b], out["pb"][b], out["pnb"][b], tol)
    got = _final_of(out, b, W)
    assert [g for g, _p in got] == [g for g, _a, _b in final]
    for (g, p), (_g, a, c) in zip(got, final):
        assert abs(p - float(np.logaddexp(a, c))) <= tol, (g, p, a, c)
    for k in ("parent", "sym", "pb", "pnb"):
        assert (out[k][b, Tb:] == 77).all(), ("trace rows past T_b are not written", k)
    return got


def _search_ok(got, ref):
    """The whole final beam against the fp64 search: the same label sequences, slot r holding one whose reference score is within
    TOL_SEARCH of the r-th best reference score (equal scores may sit either way round), every score within TOL_SEARCH."""
    want = dict(ref["beam"])
    assert {g for g, _p in got} == set(want) and len(got) == len(ref["beam"])
    assert got[0][0] == ref["beam"][0][0]                                            # (the top-1 / top-2 margin exceeds TOL_SEARCH)
    for r, (g, p) in enumerate(got):
        assert abs(p - float(want[g])) <= R.TOL_SEARCH, (r, g, p, want[g])
        assert abs(float(want[g]) - float(ref["beam"][r][1])) <= R.TOL_SEARCH, (r, g)


# ------------------------------------------------------------------------------------------------
# 1. the kernel: every frame of every input followed by the checker
@pytest.mark.parametrize("shift", R.BLANK_SHIFTS)
@pytest.mark.parametrize("cfg", R.KERNEL_CONFIGS, ids=lambda c: "V%d_T%d_W%d_L%d_s%d" % c)
def test_kernel_trace_follows_the_rule(cfg, shift):
    V, T, W, L_max, s = cfg
    z = R.kernel_inputs(V, T, s, 0, shift)
    out = _launch(z[None], [T], V, W, L_max)
    got = _check_utterance(out, 0, z, T, V, W, L_max, R.TOL_STEP_LONG if T > 40 else R.TOL_STEP)
    assert len(got) == W
    print(cfg, shift, "lengths", sorted({len(g) for g, _p in got}), "best", got[0][1])


def test_kernel_reentry_of_a_prefix_whose_extension_stayed():
    """The input of tests/test_ctc_prefix_cpu.py in which a prefix leaves the beam and is re-created while its one-symbol extension
    stayed: the next frame must merge the two (a parent link alone would not)."""
    c = REENTRY
    z = R.kernel_inputs(c["V"], c["T"], c["s"], c["seed"])
    ref = R.search(z, c["T"], c["W"], c["L_max"])
    assert R.reentered(ref["beams"])
    out = _launch(z[None], [c["T"]], c["V"], c["W"], c["L_max"])
    got = _check_utterance(out, 0, z, c["T"], c["V"], c["W"], c["L_max"], R.TOL_STEP)
    _search_ok(got, ref)


def test_kernel_mixed_lengths_wide_rows_and_poisoned_padding():
    """T_b = 0, 1, < T, = T and > T (clamped) in one batch; rows of ld = V + 5 floats whose pad columns, and whole frames past T_b, hold
    100.0 on a non-blank: neither is ever read, so the launch equals one on the clean logits bit for bit."""
    V, T, W, L_max, ld = 31, 40, 10, 16, 36
    Tbs = [0, 1, 7, 23, T, T + 9, -2]
    B = len(Tbs)
    clean = np.stack([R.kernel_inputs(V, T, 2, 100 + b) for b in range(B)])
    z = np.full((B, T, ld), 100.0, np.float32)
    z[..., :V + 1] = clean
    for b, tb in enumerate(Tbs):
        z[b, max(min(tb, T), 0):, :V] = -5.0
        z[b, max(min(tb, T), 0):, 3] = 100.0
    out = _launch(z, Tbs, V, W, L_max)
    for b, tb in enumerate(Tbs):
        got = _check_utterance(out, b, clean[b], tb, V, W, L_max, R.TOL_STEP)
        if tb <= 0:
            assert got == [((), 0.0)]
        if tb == 1:
            assert len(got) == W and max(len(g) for g, _p in got) == 1
    ref = _launch(clean, [min(max(t, 0), T) for t in Tbs], V, W, L_max)
    for k in ("ids", "lens", "score", "parent", "sym", "pb", "pnb"):
        assert np.array_equal(out[k], ref[k]), k


def test_kernel_is_deterministic_and_writes_nothing_else():
    V, T, W, L_max, s = 41, 40, 10, 16, 3
    z = np.stack([R.kernel_inputs(V, T, s, seed) for seed in range(6)])
    a = _launch(z, [T] * 6, V, W, L_max, fill=77.0)
    b = _launch(z, [T] * 6, V, W, L_max, fill=-3.0)                                  # (_launch asserts the tails kept their fill)
    for k in ("ids", "lens", "score", "parent", "sym", "pb", "pnb"):
        assert np.array_equal(a[k], b[k]), k
    c = _launch(z, [T] * 6, V, W, L_max, trace=False)                                # production form: no trace buffers
    for k in ("ids", "lens", "score"):
        assert np.array_equal(a[k], c[k]), k


# ------------------------------------------------------------------------------------------------
# 2. whole searches against the fp64 dictionary search
def _references(cfg):
    if cfg not in _CACHE:
        V, T, W, L_max, s = cfg
        zs = np.stack([R.kernel_inputs(V, T, s, seed) for seed in range(64)])
        zs.setflags(write=False)
        _CACHE[cfg] = (zs, [R.search(zs[i], T, W, L_max) for i in range(64)])
    return _CACHE[cfg]


@pytest.mark.parametrize("cfg", R.SEARCH_CONFIGS, ids=lambda c: "V%d_T%d_W%d_L%d_s%d" % c)
def test_whole_search_equals_the_fp64_reference(cfg):
    V, T, W, L_max, _s = cfg
    zs, refs = _references(cfg)
    out = _launch(zs, [T] * 64, V, W, L_max, trace=False)
    left_out = 0
    for i, ref in enumerate(refs):
        if not ref["margin"] > R.TOL_SEARCH:
            left_out += 1
            continue
        _search_ok(_final_of(out, i, W), ref)
    print(cfg, "left out", left_out, "of 64")
    assert left_out <= 64 // 3


# ------------------------------------------------------------------------------------------------
# 3. the engine: Seq2SeqModel.ctc_prefix_beam_search against the reference on the oracle's evaluation-mode head logits
@pytest.mark.parametrize("case", ["c1_audio_uni_luong", "c5_av_align"])
def test_model_search_equals_the_reference_on_the_oracle_logits(case):
    """The engine's head logits are its own fp32 product, so they differ from the oracle's by some d = max |z_engine - z_oracle| (read
    back from the workspace and held to 1e-5).  A frame's log-softmax then moves by at most 2 d, the log-probability of any alignment of
    T_b frames by at most 2 T_b d, and so does every sum over alignments: the score tolerance and the margin a compared utterance needs are
    TOL_SEARCH + 2 T_b d.  W = 1: the kept labelling never scores below the best path's own log-probability sum_t max_c y[t][c] (the
    stronger reading -- not below log p_ctc of the best path's LABELLING -- is false in the fp64 reference itself on these logits)."""
    from test_gpu_ctc import _make
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, Wt, batch, stream = _make(case)
    enc = O.encoder_outputs({k: v for k, v in Wt.items() if "/ctc/" not in k}, ocfg, batch, training=False)[stream][0]
    kn, bn = RC.head_names(stream)
    z = enc @ Wt[kn].astype(np.float64) + Wt[bn].astype(np.float64)
    lens = np.asarray(batch.audio_len if stream == "audio" else batch.video_len)
    B, T, C = z.shape
    V = C - 1
    model = Seq2SeqModel(dataclasses.replace(mcfg, use_ctc=True), weights=Wt)
    bt = Batch.from_numpy(batch)
    compared = total = 0
    for W, L_max in ((1, None), (4, None), (10, None), (10, 6)):
        got = model.ctc_prefix_beam_search(bt, beam_width=W, max_steps=L_max, nbest=True)
        best = model.ctc_prefix_beam_search(bt, beam_width=W, max_steps=L_max)
        ws = model._get_ws(B, model._audio_rows(bt), bt.video.shape[1] if bt.video is not None else 0, 1, True)
        ze = ws["enc"][stream]["ctc_z"].view(B, T, C).cpu().numpy()
        assert len(got) == len(best) == B
        for b in range(B):
            d = float(np.abs(ze[b, :lens[b]] - z[b, :lens[b]]).max())
            assert d <= 1e-5, (b, d)
            tol = R.TOL_SEARCH + 2 * lens[b] * d
            ref = R.search(z[b], lens[b], W, L_max or mcfg.max_label_length)
            assert best[b] == got[b][0][0]
            assert all(isinstance(s, int) for s in best[b]) and all(np.isfinite(p) for _g, p in got[b])
            if W == 1:
                assert got[b][0][1] >= float(R.log_softmax(z[b, :lens[b]]).max(-1).sum()) - tol
            total += 1
            if not ref["margin"] > tol:
                continue
            compared += 1
            want = dict(ref["beam"])
            assert [tuple(g) for g, _p in got[b]][0] == ref["beam"][0][0]
            assert {tuple(g) for g, _p in got[b]} == set(want)
            for r, (g, p) in enumerate(got[b]):
                assert abs(p - float(want[tuple(g)])) <= tol and abs(float(want[tuple(g)]) - float(ref["beam"][r][1])) <= tol, (W, b, r)
    print(case, "compared", compared, "of", total)
    assert 2 * compared >= total
    with pytest.raises(ValueError, match="use_ctc"):
        Seq2SeqModel(mcfg, weights={k: v for k, v in Wt.items() if "/ctc/" not in k}).ctc_prefix_beam_search(bt)
    with pytest.raises(ValueError, match="512"):
        model.ctc_prefix_beam_search(bt, max_steps=513)


# ------------------------------------------------------------------------------------------------
# 4. the front door
def test_avsr_trains_and_evaluates_with_the_prefix_search(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd.utils import _strip_extra_chars
    from test_gpu_avsr import _dataset
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=8)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"],
              audio_test_record=p["audio"], labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4),
              encoder_units_per_layer=((32,), (32, 32)), decoder_units_per_layer=(32,), embedding_size=16, warmup_steps=0,
              learning_rate=0.01, shuffle_seed=0, use_ctc=True, decoding_algorithm="ctc_prefix_beam_search", beam_width=10)
    exp = avsr.AVSR(**kw)
    exp.train(logfile="logs/prefix", num_epochs=3)                         # two epochs
    losses = [float(l.split()[-1]) for l in open("logs/prefix").read().splitlines() if l.startswith("Average")]
    assert len(losses) == 2 and np.isfinite(losses).all()
    exp.save("checkpoints/prefix/checkpoint.ckp-2")

    def no_decoder(*a, **k):
        raise AssertionError("the attention decoder must not run under ctc_prefix_beam_search")
    monkeypatch.setattr(exp._model, "beam_search_decode", no_decoder)
    monkeypatch.setattr(exp._model, "greedy_decode", no_decoder)
    err = exp.evaluate("checkpoints/prefix/checkpoint.ckp-2", epoch=2)
    assert set(err) == {"character", "word", "ctc_character"}
    assert all(np.isfinite(v) and v >= 0.0 for v in err.values())
    mlf = open(os.path.join("predictions", "prefix", "predicted_epoch_2.mlf")).read().splitlines()
    assert len(mlf) == 8
    lines = {l.split(" ", 1)[0]: l for l in mlf}
    seen = 0
    for bd in exp._iterator("evaluate"):                                   # the same predictions as the model-level call
        batch, names = exp._to_batch(bd)
        ids = exp._model.ctc_prefix_beam_search(batch, beam_width=10, max_steps=exp._cfg.max_label_length)
        for name, seq in zip(names, ids):
            hyp = "".join(_strip_extra_chars([exp._unit_dict[s] for s in seq]))
            assert lines[name.decode("utf-8")].startswith("%s %s [" % (name.decode("utf-8"), hyp)), (name, hyp)
            seen += 1
    assert seen == 8

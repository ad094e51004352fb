"""CTC forced alignment on the GPU: the kernel through the C ABI against the fp64 checker of tests/ref_ctc_align.py at the shapes that
can break it, exact ties, repeatability, path equality over 64 seeds per configuration, then Seq2SeqModel.ctc_align on the oracle's
evaluation-mode head logits and the AVSR front door.

Tolerances are ref_ctc_align's: TOL_ALIGN (T <= 64) / TOL_ALIGN_LONG for scores -- 8 x what the float32 restatement of the rule deviates
from fp64 on these very inputs -- and TOL_LP for one frame_lp entry.  The checker holds EVERY returned path to the fp64 optimum within
the tolerance; a path is compared frame by frame with the reference's only where the reference's margin (the gap to the best other
alignment) exceeds the tolerance -- an argmax is discontinuous at a tie -- and at most one eighth of a configuration's 64 seeds may be
left out of that comparison."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_ctc as RC  # noqa: E402
import ref_ctc_align as R  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("score", "status", "path", "frame_lp", "start", "end")
_CACHE = {}


def _launch(z, labels, target_len, in_len, V, fill=12345.0, tail=64):
    """z [B, T, ld] float32 (ld >= V + 1), labels [B, L].  Outputs are allocated `tail` elements too long and pre-filled with a value no
    output can take, so that what the kernel leaves alone can be seen: nothing past the end is written, everything inside is.  Returns
    dict(score, status [B], path, frame_lp [B, T], start, end [B, L])."""
    from avsr_tf1_amd import ops
    z, labels = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(labels, np.int32)
    B, T, ld = z.shape
    L = labels.shape[1]
    dev = "cuda"
    zd = torch.tensor(z.reshape(B * T, ld), device=dev)
    i32 = lambda a: torch.tensor(np.asarray(a, np.int32), device=dev)
    full = lambda n, dt: torch.full((n + tail,), fill if dt == torch.float32 else int(fill), dtype=dt, device=dev)
    bufs = dict(score=full(B, torch.float32), status=full(B, torch.int32), path=full(B * T, torch.int32), frame_lp=full(B * T, torch.float32),
                start=full(B * L, torch.int32), end=full(B * L, torch.int32))
    nws = ops.ctc_align_ws_bytes(B, T, L)
    assert nws % 8 == 0
    ws = torch.full((nws // 8 + tail,), 0x4d4d4d4d4d4d4d4d, dtype=torch.int64, device=dev)
    ops.ctc_align(zd, ld, i32(labels), i32(target_len), i32(in_len), B, T, L, V, *(bufs[k] for k in KEYS), ws[:nws // 8])
    torch.cuda.synchronize()
    assert (ws[nws // 8:] == 0x4d4d4d4d4d4d4d4d).all(), "written past the end of the workspace"
    res = {}
    for k in KEYS:
        v = bufs[k].cpu().numpy()
        n = v.size - tail
        f = int(fill) if v.dtype.kind == "i" else np.float32(fill)
        assert (v[n:] == f).all(), ("written past the end of", k)
        assert not (v[:n] == f).any(), ("an element was not written", k)
        res[k] = v[:n].reshape((B,) if k in ("score", "status") else (B, T) if k in ("path", "frame_lp") else (B, L))
    return res


def _one(out, b):
    return {k: out[k][b] for k in KEYS}


def _pad(gs, L):
    lab = np.zeros((len(gs), L), np.int32)
    for b, g in enumerate(gs):
        lab[b, :len(g)] = g
    return lab


# ------------------------------------------------------------------------------------------------
# 1. the kernel at the shapes that can break it
@pytest.mark.parametrize("case", R.KERNEL_CASES, ids=lambda c: "V%d_T%d_L%d_U%d_Tb%s_%s" % c)
def test_kernel_alignment_follows_the_rule(case):
    V, T, L, U, _Tb, _kind = case
    z, g, Tb = R.case_inputs(case)
    out = _launch(z[None], _pad([g], L), [U], [Tb], V)
    ref, compared = R.check(z, g, Tb, _one(out, 0), R.tol_for(T))
    print(case, "score", out["score"][0], "fp64", ref["score"], "margin", ref["margin"], "compared", compared)
    assert out["status"][0] == 1


def test_kernel_mixed_batch_wide_rows_and_poisoned_padding():
    """One batch with an utterance that has too few frames, one with T_b = 0, one with a label out of range, T_b < T, T_b > T (clamped),
    target_len > L (clamped) and < 0; rows of ld = V + 5 floats whose pad columns, whole frames past T_b and label slots past U hold
    values that would win or fault if read: the launch equals one on the clean inputs bit for bit."""
    V, T, L, clean, gs, tls, Tbs = R.mixed_batch()
    B, ld = len(gs), V + 5
    assert not R.feasible(gs[3], Tbs[3], V) and R.repeats(gs[3]) >= 1
    z = np.full((B, T, ld), 100.0, np.float32)
    z[..., :V + 1] = clean
    lab = _pad(gs, L)
    for b, tb in enumerate(Tbs):
        tb = max(min(tb, T), 0)
        z[b, tb:, :V + 1] = -5.0
        z[b, tb:, 3] = 100.0
        lab[b, len(gs[b]):] = 2 ** 30                                      # label slots past U are not labels
    out = _launch(z, lab, tls, Tbs, V)
    for b in range(B):
        ref, _c = R.check(clean[b], gs[b], Tbs[b], _one(out, b), R.TOL_ALIGN)
        assert ref["status"] == (0 if b in (1, 3, 4) else 1)
    ref = _launch(clean, _pad(gs, L), [len(g) for g in gs], [max(min(t, T), 0) for t in Tbs], V)
    for k in KEYS:
        assert np.array_equal(out[k], ref[k]), k


# ------------------------------------------------------------------------------------------------
# 2. exact ties, repeatability
@pytest.mark.parametrize("V,T,U,kind", R.TIE_CASES)
def test_exact_ties_follow_the_rule(V, T, U, kind):
    """Row-constant logits: every class of a frame has the same log-probability, so all reachable states of a frame are bit-equal in any
    arithmetic that adds the same numbers to them -- each comparison is an exact tie, and the path must equal the reference's with no
    tolerance: stay wins over s - 1 wins over s - 2, the last blank wins the end."""
    z, g, _Tb = R.tie_inputs(V, T, U, kind)
    ref = R.align(z, g, T, want_margin=True)
    assert ref["status"] == 1 and abs(ref["margin"]) < 1e-9
    out = _launch(z[None], _pad([g], U), [U], [T], V)
    assert [int(k) for k in out["path"][0]] == ref["path"]
    assert [int(v) for v in out["start"][0]] == ref["start"] and [int(v) for v in out["end"][0]] == ref["end"]
    R.check(z, g, T, _one(out, 0), R.tol_for(T))


def test_kernel_is_deterministic_and_writes_every_element():
    V, T, L = 40, 200, 40
    gs = [R.labels(V, 40 - b, b) for b in range(6)]
    z = np.stack([R.logits(V, T, 300 + b) for b in range(6)])
    Tbs = [T, T - 1, 150, 129, 128, 60]
    a = _launch(z, _pad(gs, L), [len(g) for g in gs], Tbs, V)
    b = _launch(z, _pad(gs, L), [len(g) for g in gs], Tbs, V, fill=-3.0)          # (_launch asserts that every element was written)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert (a["status"] == 1).all()


# ------------------------------------------------------------------------------------------------
# 3. path equality over 64 seeds per configuration
def _references(cfg):
    if cfg not in _CACHE:
        V, T, U = cfg
        zs = np.stack([R.logits(V, T, seed) for seed in range(64)])
        zs.setflags(write=False)
        gs = [R.labels(V, U, seed) for seed in range(64)]
        _CACHE[cfg] = (zs, gs, [R.align(zs[i], gs[i], T, want_margin=True) for i in range(64)])
    return _CACHE[cfg]


@pytest.mark.parametrize("cfg", R.SEED_CONFIGS, ids=lambda c: "V%d_T%d_U%d" % c)
def test_paths_equal_the_fp64_reference(cfg):
    V, T, U = cfg
    zs, gs, refs = _references(cfg)
    out = _launch(zs, _pad(gs, U), [U] * 64, [T] * 64, V)
    left_out = 0
    for i, ref in enumerate(refs):
        _r, compared = R.check(zs[i], gs[i], T, _one(out, i), R.tol_for(T), ref=ref)
        left_out += not compared
    print(cfg, "left out", left_out, "of 64")
    assert left_out <= 64 // 8


# ------------------------------------------------------------------------------------------------
# 4. the engine: Seq2SeqModel.ctc_align on the oracle's evaluation-mode head logits
@pytest.mark.parametrize("case", ["c1_audio_uni_luong", "c5_av_align"])
def test_model_alignment_on_the_oracle_logits(case):
    """The engine's head logits are its own fp32 product, so they differ from the oracle's by some d = max |z_engine - z_oracle| (read
    back from the workspace and held to 1e-5).  A frame's log-softmax then moves by at most 2 d and the log-probability of any alignment
    of T_b frames by at most 2 T_b d: the score tolerance and the margin a compared path needs are the score tolerance + 2 T_b d, one frame_lp
    entry may be off by TOL_LP + 2 d."""
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
    Ul = RC.targets(batch.labels, batch.labels_len)
    rows = [[int(s) for s in batch.labels[b, :Ul[b]]] for b in range(B)]
    found = model.ctc_prefix_beam_search(bt, beam_width=4)
    aligned = 0
    for targets, gs in ((None, rows), (found, found), (rows[::-1], rows[::-1])):
        got = model.ctc_align(bt, targets)
        ws = model._get_ws(B, model._audio_rows(bt), bt.video.shape[1] if bt.video is not None else 0, 1, True)
        ze = ws["enc"][stream]["ctc_z"].view(B, T, C).cpu().numpy()
        assert len(got) == B
        for b in range(B):
            Tb = int(min(lens[b], T))
            d = float(np.abs(ze[b, :Tb] - z[b, :Tb]).max())
            assert d <= 1e-5, (b, d)
            tol = R.tol_for(T) + 2 * Tb * d
            ref = R.align(z[b], gs[b], Tb, want_margin=True)
            a = got[b]
            assert set(a) == {"status", "score", "path", "segments"} and a["status"] == ref["status"]
            if not a["status"]:
                assert a["score"] == 0.0 and a["path"] == [] and a["segments"] == []
                continue
            aligned += 1
            assert len(a["path"]) == Tb and all(isinstance(k, int) for k in a["path"]) and len(a["segments"]) == len(gs[b])
            y = R.log_softmax(z[b, :Tb])
            kernel = dict(status=1, score=a["score"], path=np.array(a["path"] + [-1] * (T - Tb)),
                          frame_lp=np.concatenate((y[np.arange(Tb), a["path"]], np.zeros(T - Tb))),        # (the engine returns no frame_lp)
                          start=np.array([s[1] for s in a["segments"]]), end=np.array([s[2] for s in a["segments"]]))
            R.check(z[b], gs[b], Tb, kernel, tol, ref=ref, lp_tol=R.TOL_LP + 2 * d)
            for (lab, s, e, conf), want in zip(a["segments"], gs[b]):                                   # segments are consistent with path
                assert lab == want and 0 <= s <= e < Tb and a["path"][s:e + 1] == [lab] * (e - s + 1)
                assert (s == 0 or a["path"][s - 1] != lab) and (e == Tb - 1 or a["path"][e + 1] != lab)
                want_conf = float(np.exp(y[s:e + 1, lab].mean()))
                assert abs(conf - want_conf) <= want_conf * np.expm1(R.TOL_LP + 2 * d) + 1e-12 and 0.0 < conf <= 1.0
    print(case, "aligned", aligned)
    assert aligned >= B
    with pytest.raises(ValueError, match="use_ctc"):
        Seq2SeqModel(mcfg, weights={k: v for k, v in Wt.items() if "/ctc/" not in k}).ctc_align(bt)
    with pytest.raises(ValueError, match="one id list per utterance"):
        model.ctc_align(bt, rows[:-1])
    with pytest.raises(ValueError, match="512"):
        model.ctc_align(bt, [[1] * 513] + rows[1:])


# ------------------------------------------------------------------------------------------------
# 5. the front door
def _parse(text, timed):
    out, scores, name, segs = {}, {}, None, None
    for line in text.splitlines():
        if name is None:
            name, sc = line.rsplit(" ", 1)
            scores[name], segs = float(sc), []
        elif line == ".":
            out[name], name = segs, None
        elif line == "# no alignment":
            segs = None
        else:
            s, e, rest = line.split(" ", 2)
            sym, conf = rest.rsplit(" ", 1)
            segs.append((sym, float(s) if timed else int(s), float(e) if timed else int(e), float(conf)))
    assert name is None
    return out, scores


def test_avsr_align_labels_and_predictions(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from test_gpu_avsr import _dataset
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=8)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"],
              audio_test_record=p["audio"], labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4),
              encoder_units_per_layer=((32,), (32, 32)), decoder_units_per_layer=(32,), embedding_size=16, warmup_steps=0,
              learning_rate=0.01, shuffle_seed=0, use_ctc=True, decoding_algorithm="ctc_prefix_beam_search", beam_width=10)
    exp = avsr.AVSR(**kw)
    exp.train(logfile="logs/align", num_epochs=3)                          # two epochs
    ckpt = exp.save("checkpoints/align/checkpoint.ckp-2")
    fname = os.path.join("predictions", "align", "ctc_alignment_epoch_2.txt")
    eos = exp._cfg.eos_id
    want, frames = {}, {}
    for bd in exp._iterator("evaluate"):
        batch, names = exp._to_batch(bd)
        preds = exp._model.ctc_prefix_beam_search(batch, beam_width=10, max_steps=exp._cfg.max_label_length)
        for i, name in enumerate(names):
            row = [int(s) for s in bd.labels[i][:int(bd.labels_length[i])]]
            assert row[-1] == eos
            want[name.decode("utf-8")] = {"labels": [exp._unit_dict[s] for s in row[:-1]], "predictions": [exp._unit_dict[s] for s in (preds[i][:preds[i].index(eos)] if eos in preds[i] else preds[i])]}
            frames[name.decode("utf-8")] = int(bd.inputs_length[i])
    assert len(want) == 8

    def same(a, b, tol):
        assert set(a) == set(b)
        for k in a:
            assert (a[k] is None) == (b[k] is None), k
            for x, y in zip(a[k] or (), b[k] or ()):
                assert x[0] == y[0] and abs(x[1] - y[1]) <= tol and abs(x[2] - y[2]) <= tol and abs(x[3] - y[3]) <= 1e-6, (k, x, y)
            assert len(a[k] or ()) == len(b[k] or ())

    for targets in ("labels", "predictions"):
        res = exp.align(ckpt, epoch=2, targets=targets)
        assert os.path.exists(fname)
        parsed, scores = _parse(open(fname).read(), timed=False)
        same(parsed, res, 0)
        assert set(res) == set(want)
        n_aligned = 0
        for name, segs in res.items():
            if segs is None:                                               # more labels (and repeats) than frames: predictions only
                assert targets == "predictions" and scores[name] == 0.0
                continue
            n_aligned += 1
            assert [s[0] for s in segs] == want[name][targets], (name, targets)
            assert scores[name] < 0.0 or not segs
            prev = -1
            for _sym, s, e, conf in segs:                                  # monotone, inside the utterance, a probability
                assert isinstance(s, int) and prev < s <= e < frames[name] and 0.0 < conf <= 1.0
                prev = e
        assert n_aligned == 8 if targets == "labels" else n_aligned >= 1
    res = exp.align(ckpt, epoch=2, targets="labels")
    timed = exp.align(ckpt, epoch=2, targets="labels", frame_shift=0.03)
    parsed, _scores = _parse(open(fname).read(), timed=True)
    same(parsed, timed, 1e-9)
    for name, segs in res.items():
        for (sym, s, e, conf), (sym2, s2, e2, conf2) in zip(segs, timed[name]):
            assert sym == sym2 and conf == conf2
            assert abs(s2 - 0.03 * s) <= 5.01e-4 and abs(e2 - 0.03 * (e + 1)) <= 5.01e-4            # end is exclusive, three decimals
    err = exp.evaluate(ckpt, epoch=2)                                       # evaluate is as it was
    assert set(err) == {"character", "word", "ctc_character"}
    assert os.path.exists(os.path.join("predictions", "align", "predicted_epoch_2.mlf"))
    with pytest.raises(ValueError, match="targets"):
        exp.align(ckpt, epoch=2, targets="greedy")

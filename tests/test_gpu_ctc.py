"""CTC auxiliary loss (use_ctc) on the GPU: the kernel through the C ABI against fp64 torch (tests/ref_ctc.py), then the engine's
train step with the head against the oracle's graph with the same term added, the off state, graph replay, two data-parallel
ranks, the best-path decode and the AVSR front door.

Tolerances are the project's: loss 1e-4 absolute, every gradient tensor 2e-4 * max|g| + 1e-6; the raw per-utterance nll 1e-5
relative.  The long shapes (T = 500, 1501) are what a plain fp32 log-space recursion misses by 10x (torch's own fp32 ctc_loss:
2e-3 to 3e-3 of max|g| at T = 500, U = 39)."""
import dataclasses
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_ctc as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# 1. the kernel against fp64 torch
# name -> (B, T, C, ld, U per utterance, T_b per utterance or None = T, fixed label rows or None, expected status)
SHAPES = {
    "ragged": (5, 21, 32, 32, [0, 1, 3, 6, 5], [21, 1, 10, 15, 21], None, [1, 1, 1, 1, 1]),
    "stride44": (3, 9, 42, 44, [4, 4, 4], None, None, [1, 1, 1]),
    "aab": (2, 4, 32, 32, [3, 3], [4, 3], [[5, 5, 9], [5, 5, 9]], [1, 0]),        # 'a a b': 4 frames = one path family, 3 frames = none
    "empty": (2, 5, 32, 32, [2, 2], [0, 5], None, [0, 1]),
    "wave": (2, 70, 32, 32, [31, 32], None, None, [1, 1]),                        # 63 and 65 states
    "long32": (4, 500, 32, 32, [39, 39, 20, 0], None, None, [1, 1, 1, 1]),
    "long42": (2, 500, 42, 42, [149, 100], None, None, [1, 1]),
    "t1501": (2, 1501, 32, 32, [60, 149], None, None, [1, 1]),
}
_CACHE = {}


def _inputs(name, scale):
    """(z, labels, labels_len, in_len, denom, fp64 reference), computed once per (shape, scale) and never modified."""
    key = (name, scale)
    if key not in _CACHE:
        B, T, C, _ld, Us, Tbs, fixed, _st = SHAPES[name]
        rng = np.random.default_rng(sorted(SHAPES).index(name))
        L = max(Us) + 1
        labels, labels_len = np.zeros((B, L), np.int32), np.zeros(B, np.int32)
        for b, u in enumerate(Us):
            labels[b, :u] = fixed[b] if fixed is not None else rng.integers(0, C - 1, u)
            labels[b, u] = C - 2                               # the EOS slot: not part of the CTC target
            labels_len[b] = u + 1
        z = (rng.standard_normal((B, T, C)) * scale).astype(np.float32)
        in_len = np.full(B, T, np.int32) if Tbs is None else np.array(Tbs, np.int32)
        denom = float(labels_len.sum())
        ref = R.kernel_reference(z, labels, labels_len, in_len, denom, 1.0)
        for v in (z, labels, labels_len, in_len):
            v.setflags(write=False)
        _CACHE[key] = (z, labels, labels_len, in_len, denom, ref)
    return _CACHE[key]


class _Launch:
    """Device buffers of one shape; run() launches avsr_ctc_loss into them."""

    def __init__(self, z, labels, ld, pad=50.0, fill=7.0):
        B, T, C = z.shape
        self.B, self.T, self.C, self.ld, self.L = B, T, C, ld, labels.shape[1]
        zp = np.full((B * T, ld), pad, np.float32)             # a leaking pad column would dominate the softmax
        zp[:, :C] = z.reshape(B * T, C)
        dev = "cuda"
        from avsr_tf1_amd import ops
        self.ops = ops
        self.z = torch.tensor(zp, device=dev)
        self.labels = torch.tensor(np.ascontiguousarray(labels), device=dev)
        self.dz = torch.full((B * T, ld), fill, device=dev)
        self.nll, self.utt = torch.full((B,), fill, device=dev), torch.full((B,), fill, device=dev)
        self.status = torch.full((B,), 9, dtype=torch.int32, device=dev)
        self.ws = torch.full((ops.ctc_ws_floats(B, T, self.L),), fill, device=dev)
        self.fill = fill

    def run(self, labels_len, in_len, denom, weight=1.0):
        dev = "cuda"
        ll, il = torch.tensor(np.ascontiguousarray(labels_len), device=dev), torch.tensor(np.ascontiguousarray(in_len), device=dev)
        dn = torch.tensor([denom], dtype=torch.float32, device=dev)
        self.ops.ctc_loss(self.z, self.ld, self.labels, ll, il, dn, weight, self.nll, self.status, self.utt, self.dz, self.ws,
                          self.B, self.T, self.L, self.C)
        torch.cuda.synchronize()
        dz = self.dz.cpu().numpy().reshape(self.B, self.T, self.ld)
        return dict(nll=self.nll.cpu().numpy(), status=self.status.cpu().numpy(), utt_loss=self.utt.cpu().numpy(),
                    dz=dz[:, :, :self.C].copy(), pad=dz[:, :, self.C:].copy())


def _check(out, ref, tag):
    mg = np.abs(ref["dz"]).max()
    e_loss = abs(float(out["utt_loss"].astype(np.float64).sum()) - float(ref["utt_loss"].sum()))
    e_nll = np.abs(out["nll"] - ref["nll"]) / np.maximum(np.abs(ref["nll"]), 1e-30)
    e_nll = np.where(ref["nll"] == 0.0, np.abs(out["nll"]), e_nll)          # left-out utterances: exactly 0
    e_dz = np.abs(out["dz"] - ref["dz"]).max()
    print("%s: loss err %.3g | nll rel err %.3g | dz err %.3g of max|dz| %.3g (%.3g)" % (tag, e_loss, e_nll.max(), e_dz, mg, e_dz / max(mg, 1e-30)))
    assert np.array_equal(out["status"], ref["status"]), (out["status"], ref["status"])
    assert np.isfinite(out["dz"]).all() and np.isfinite(out["nll"]).all()
    assert e_loss < 1e-4, e_loss
    assert e_nll.max() < 1e-5, e_nll
    assert e_dz < 2e-4 * mg + 1e-6, (e_dz, mg)


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_against_fp64_torch(name, scale):
    z, labels, labels_len, in_len, denom, ref = _inputs(name, scale)
    B, T, C, ld, _Us, _Tbs, _fixed, status = SHAPES[name]
    assert list(ref["status"]) == status                               # exactly these rows are left out, decided on the CPU
    la = _Launch(z, labels, ld)
    out = la.run(labels_len, in_len, denom)
    _check(out, ref, "%s x%g" % (name, scale))
    assert (out["pad"] == la.fill).all()                               # columns of a padded row stride are not written
    for b in range(B):
        if not status[b]:
            assert out["nll"][b] == 0.0 and out["utt_loss"][b] == 0.0 and not out["dz"][b].any()
        assert not out["dz"][b, int(np.clip(in_len[b], 0, T)):].any()  # frames past T_b: exactly zero
    if name == "aab":                                                  # the one path a - a b
        lp = torch.log_softmax(torch.tensor(z[0].astype(np.float64)), -1).numpy()
        assert abs(out["nll"][0] + (lp[0, 5] + lp[1, 31] + lp[2, 5] + lp[3, 9])) < 1e-5 * abs(ref["nll"][0])


def test_kernel_weight_and_denominator_scale_the_outputs():
    z, labels, labels_len, in_len, denom, _ref = _inputs("ragged", 1.0)
    ref = R.kernel_reference(z, labels, labels_len, in_len, 3.0 * denom, 0.3)
    out = _Launch(z, labels, 32).run(labels_len, in_len, 3.0 * denom, weight=0.3)
    _check(out, ref, "ragged, weight 0.3, 3 x denom")


# 2. the buffers are reused across batches: nothing may survive from the previous launch
def test_kernel_rewrites_rows_past_the_length_every_launch():
    z, labels, labels_len, in_len, denom, ref = _inputs("ragged", 1.0)
    la = _Launch(z, labels, 32)
    _check(la.run(labels_len, in_len, denom), ref, "ragged, first launch")
    short = np.array([11, 1, 5, 8, 0], np.int32)                         # (row 4: no frames at all)
    ref2 = R.kernel_reference(z, labels, labels_len, short, denom, 1.0)
    assert list(ref2["status"]) == [1, 1, 1, 1, 0]
    out2 = la.run(labels_len, short, denom)
    _check(out2, ref2, "ragged, second launch, shorter")
    for b in range(5):
        assert not out2["dz"][b, short[b]:].any()
    assert (out2["pad"].size == 0) or (out2["pad"] == la.fill).all()


# 3. no atomics: bit-identical launches
def test_kernel_is_deterministic():
    z, labels, labels_len, in_len, denom, _ref = _inputs("long32", 3.0)
    a = _Launch(z, labels, 32, fill=7.0).run(labels_len, in_len, denom)
    b = _Launch(z, labels, 32, fill=-3.0).run(labels_len, in_len, denom)
    assert np.array_equal(a["dz"], b["dz"]) and np.array_equal(a["nll"], b["nll"]) and np.array_equal(a["utt_loss"], b["utt_loss"])


def test_kernel_rejects_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    a = _lib.CtcArgs()
    assert lib.avsr_ctc_loss(None, None) == -1 and lib.avsr_ctc_loss(a, None) == -1
    p = 64
    a.B, a.T, a.L, a.C, a.ld = 2, 5, 3, 8, 8
    for n in ("z", "labels", "labels_len", "in_len", "denom", "nll", "status", "utt_loss", "ws"):
        setattr(a, n, p)
    a.dz = 128
    a.ws_floats = lib.avsr_ctc_ws_floats(2, 5, 3) - 1
    assert lib.avsr_ctc_loss(a, None) == -1                              # workspace too small
    a.ws_floats += 1
    a.ld = 7
    assert lib.avsr_ctc_loss(a, None) == -1                              # row stride below the class count
    a.ld, a.L = 8, 2000
    a.ws_floats = lib.avsr_ctc_ws_floats(2, 5, 2000)
    assert lib.avsr_ctc_loss(a, None) == -3                              # more label slots than a workgroup has threads
    assert lib.avsr_ctc_ws_floats(2, 5, 3) == 2 * 5 * 7


# ------------------------------------------------------------------------------------------------
# 4. the train step with the head
def _make(case, **over):
    from test_gpu_model import make
    O, ocfg, mcfg, W, batch = make(case, **over)
    stream = R.ctc_stream(ocfg)
    W = R.add_head(W, ocfg, stream)
    return O, ocfg, mcfg, W, batch, stream


STEP_CASES = {
    "audio_uni": ("c1_audio_uni_luong", {}),
    "audio_bi_bahdanau": ("c2_audio_bi_bahdanau", {}),
    "video_bi": ("c3_video_bi_normed", {}),                                # T_v = 9: utterance 3 (5 frames, 6 labels) has no alignment
    "bimodal_aus": ("c4_bimodal_uni", {}),                                 # both auxiliary heads at once
    "av_align": ("c5_av_align", {}),
    "gru_audio": ("gru_audio_uni", {}),
    "padded_widths": ("c1_audio_uni_luong", dict(audio_units=(22, 26), decoder_units=(26,), audio_feat=39)),
    "dropout_sampling": ("c2_audio_bi_bahdanau", dict(use_dropout=True, sampling_probability=0.3)),
}


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_train_step_parity_with_the_ctc_term(name):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    case, over = STEP_CASES[name]
    O, ocfg, mcfg, W, batch, stream = _make(case, **over)
    ref = R.ctc_reference(W, ocfg, batch, stream, 0.3)
    lens = batch.audio_len if stream == "audio" else batch.video_len
    status = R.feasible(batch.labels, batch.labels_len, lens, ref["z"].shape[1])
    assert list(status) == ([1, 1, 1, 0, 1] if name == "video_bi" else [1] * 5)
    assert ref["ctc"] > 0.1                                              # the term is a visible part of the loss
    model = Seq2SeqModel(dataclasses.replace(mcfg, use_ctc=True, ctc_weight=0.3), weights=W)
    logits = model.forward_train(Batch.from_numpy(batch))
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    assert np.abs(lg - ref["logits"]).max() < 1e-4, np.abs(lg - ref["logits"]).max()
    E = model._cur[0]["enc"][stream]
    assert np.array_equal(E["ctc_status"].cpu().numpy(), status)
    nll = E["ctc_nll"].cpu().numpy()
    assert np.abs(nll - ref["nll"]).max() < 1e-4 * max(1.0, np.abs(ref["nll"]).max()), (nll, ref["nll"])
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    print("%s: loss %.6f (reference %.6f, of which ctc term %.6f)" % (name, float(model.loss.item()), ref["loss"], 0.3 * ref["ctc"]))
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4, (float(model.loss.item()), ref["loss"])
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    kn, bn = R.head_names(stream)
    assert kn in grads and bn in grads
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        err = np.abs(grads[k] - g).max()
        assert err < 2e-4 * scale + 1e-6, (k, err, scale)
    bucket = model.decoder_grad_bucket()                                  # still one block of dec/... only
    assert bucket is not None
    assert all(n.startswith("dec/") == (bucket[0] <= g.off < bucket[1]) for n, g in model.Gr.items())


# 5. the head with weight 0 changes nothing else
def test_zero_weight_leaves_every_other_parameter_bit_identical():
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    # clip_gradients=False: the global norm is an fp32 sum whose blocking follows the parameter COUNT, so its last bit may differ between
    # the two engines; unclipped, the update does not read it and every other operation is independent of the two extra variables
    O, ocfg, mcfg, W, batch, stream = _make("c4_bimodal_uni", clip_gradients=False)
    dbatch = Batch.from_numpy(batch)
    off = Seq2SeqModel(mcfg, weights=W)
    off.train_step(dbatch)
    on = Seq2SeqModel(dataclasses.replace(mcfg, use_ctc=True, ctc_weight=0.0), weights=W)
    on.train_step(dbatch)
    torch.cuda.synchronize()
    assert not [n for n in off.inv if "/ctc/" in n] and "ctc_z" not in off._cur[0]["enc"][stream]
    assert float(on.loss.item()) == float(off.loss.item())
    assert abs(float(on.gnorm.item()) - float(off.gnorm.item())) <= 1e-6 * float(off.gnorm.item())
    a, b = off.export_tf_weights("params"), on.export_tf_weights("params")
    assert set(b) - set(a) == set(R.head_names(stream))
    for k, v in a.items():
        assert np.array_equal(b[k], v), k
    for k in R.head_names(stream):
        assert np.array_equal(b[k], W[k]), k                              # a zero gradient: Adam leaves the head where it was


# 6. graph replay
def test_captured_steps_equal_eager_steps(monkeypatch):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    monkeypatch.setenv("AVSR_PERSISTENT_RNN", "0")
    O, ocfg, mcfg, W, batch, stream = _make("c4_bimodal_uni", warmup_steps=0)
    mcfg = dataclasses.replace(mcfg, use_ctc=True)
    dbatch = Batch.from_numpy(batch)
    eager = Seq2SeqModel(mcfg, weights=W)
    losses = []
    for _ in range(3):
        loss, _g = eager.train_step(dbatch)
        losses.append(float(loss.item()))
    model = Seq2SeqModel(mcfg, weights=W)
    trainer = DataParallelTrainer(model, None, use_graph=True)
    glosses = []
    for _ in range(3):
        loss, _g = trainer.train_step(dbatch)
        glosses.append(float(loss.item()))
    torch.cuda.synchronize()
    assert str(trainer.mode).startswith("hipgraph"), trainer.mode
    assert glosses == losses, (glosses, losses)
    a, b = eager.export_tf_weights("params"), model.export_tf_weights("params")
    for k, v in a.items():
        assert np.array_equal(b[k], v), k


# 7. two data-parallel ranks on one GPU (the worker pattern of tests/test_gpu_dp.py)
DP_CASE = dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32), decoder_units=(32,),
               embedding_size=16, video_feat=12, audio_feat=20, regress_aus=True, use_dropout=False, warmup_steps=0)
DP_STEPS = 4


def _dp_setup():
    from avsr_tf1_amd.config import ModelConfig
    from oracle import avsr_oracle as O
    ocfg = O.OracleConfig(**DP_CASE)
    mcfg = ModelConfig(**{f.name: getattr(ocfg, f.name) for f in dataclasses.fields(ModelConfig) if hasattr(ocfg, f.name)})
    mcfg = dataclasses.replace(mcfg, use_ctc=True)
    W = R.add_head(O.init_params(ocfg, seed=5), ocfg, "audio")
    full = O.synthetic_batch(ocfg, B=6, T_a=17, T_v=7, L=6, ragged=True)
    return O, mcfg, W, full


def _dp_shard(O, b, lo, hi):
    return O.Batch(**{k: (None if getattr(b, k) is None else np.ascontiguousarray(getattr(b, k)[lo:hi]))
                      for k in ("audio", "audio_len", "video", "video_len", "aus", "labels", "labels_len")})


def _dp_worker(rank, world, port, out_dir, use_graph):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["AVSR_PERSISTENT_RNN"] = "0"                  # two processes on ONE GPU do not both claim the chip
    import torch.distributed as dist
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    from avsr_tf1_amd.parallel import DataParallelTrainer
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    O, mcfg, W, full = _dp_setup()
    cut = [0, 2, 6]                                           # unequal shards
    model = Seq2SeqModel(mcfg, weights=W)
    trainer = DataParallelTrainer(model, dist, use_graph=use_graph)
    batch = Batch.from_numpy(_dp_shard(O, full, cut[rank], cut[rank + 1]))
    losses = []
    for _ in range(DP_STEPS):
        loss, _g = trainer.train_step(batch)
        losses.append(float(loss.item()))
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), mode=np.array(trainer.mode), step_losses=np.array(losses),
             **model.export_tf_weights("params"))
    dist.destroy_process_group()


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_ranks_equal_one_engine_with_the_ctc_term(tmp_path, use_graph, monkeypatch):
    import torch.multiprocessing as mp
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path), use_graph), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert str(r0["mode"]).startswith("hipgraph" if use_graph else "eager")
    monkeypatch.setenv("AVSR_PERSISTENT_RNN", "0")
    O, mcfg, W, full = _dp_setup()
    model = Seq2SeqModel(mcfg, weights=W)
    batch = Batch.from_numpy(full)
    losses = []
    for _ in range(DP_STEPS):
        loss, _g = model.train_step(batch)
        losses.append(float(loss.item()))
    torch.cuda.synchronize()
    ref = model.export_tf_weights("params")
    assert "audio/ctc/kernel" in ref
    assert np.array_equal(r0["step_losses"], r1["step_losses"])
    assert np.abs(r0["step_losses"] - np.array(losses)).max() < 2e-5 * max(1.0, max(losses)), (r0["step_losses"], losses)
    for k, v in ref.items():
        assert np.array_equal(r0[k], r1[k]), k                       # replicas stay bit-identical
        assert np.abs(r0[k] - v).max() < 5e-6 + 1e-4 * np.abs(v).max() * 0.01, (k, np.abs(r0[k] - v).max())


# ------------------------------------------------------------------------------------------------
# 8. best path
def test_best_path_kernel_and_model():
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch, stream = _make("c1_audio_uni_luong")
    ref = R.ctc_reference(W, ocfg, batch, stream, 0.3)
    z = ref["z"].astype(np.float32).copy()
    B, T, C = z.shape
    lens = np.asarray(batch.audio_len)
    z[0, 2, 3] = z[0, 2, 7] = z[0, 2].max() + 1.0                          # a tie: the lower index wins
    z[0, 3, C - 1] = z[0, 3, 5] = z[0, 3].max() + 1.0                      # a tie with the blank
    for b in range(B):
        z[b, lens[b]:, 4] = 100.0                                          # frames past T_b with a non-blank argmax
    want = R.best_path(z, lens, C - 1)
    assert want[0][:1] != [] and any(len(w) for w in want)
    zd = torch.tensor(z.reshape(B * T, C), device="cuda")
    ids = torch.full((B * T,), 77, dtype=torch.int32, device="cuda")
    ops.ctc_best_path(zd, C, torch.tensor(lens, device="cuda"), B, T, C, ids)
    ids = ids.cpu().numpy().reshape(B, T)
    got = []
    for b in range(B):
        assert (ids[b, lens[b]:] == -1).all() and (ids[b, :lens[b]] >= 0).all()
        assert np.array_equal(ids[b, :lens[b]], np.argmax(z[b, :lens[b]], -1))
        seq, prev = [], -1
        for k in ids[b, :lens[b]]:
            if k != prev and k != C - 1:
                seq.append(int(k))
            prev = k
        got.append(seq)
    assert got == want
    assert ids[0, 2] == 3 and ids[0, 3] == 5
    # the model's entry point: encoders in evaluation mode + the head, against the oracle's evaluation-mode outputs
    model = Seq2SeqModel(dataclasses.replace(mcfg, use_ctc=True), weights=W)
    out = model.ctc_best_path(Batch.from_numpy(batch))
    enc = O.encoder_outputs({k: v for k, v in W.items() if "/ctc/" not in k}, ocfg, batch, training=False)[stream][0]
    kn, bn = R.head_names(stream)
    z_eval = enc @ W[kn].astype(np.float64) + W[bn].astype(np.float64)
    top2 = np.sort(z_eval, -1)[..., -2:]
    assert (top2[..., 1] - top2[..., 0]).min() > 1e-4                      # no frame where fp32 could pick another class
    assert out == R.best_path(z_eval, lens, C - 1)
    with pytest.raises(ValueError):
        Seq2SeqModel(mcfg, weights=W).ctc_best_path(Batch.from_numpy(batch))


# ------------------------------------------------------------------------------------------------
# 9. the front door
def test_avsr_trains_saves_restores_and_evaluates_with_use_ctc(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from test_gpu_avsr import _dataset
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=8)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"],
              audio_test_record=p["audio"], labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4),
              encoder_units_per_layer=((32,), (32, 32)), decoder_units_per_layer=(32,), embedding_size=16, decoding_algorithm="greedy",
              warmup_steps=0, learning_rate=0.01, shuffle_seed=0)
    exp = avsr.AVSR(use_ctc=True, **kw)
    assert exp._cfg.use_ctc and exp._cfg.ctc_weight == 0.3
    exp.train(logfile="logs/ctc", num_epochs=3)                            # two epochs
    losses = [float(l.split()[-1]) for l in open("logs/ctc").read().splitlines() if l.startswith("Average")]
    assert len(losses) == 2 and np.isfinite(losses).all()
    exp.save("checkpoints/ctc/checkpoint.ckp-2")
    ck = np.load("checkpoints/ctc/checkpoint.ckp-2.npz")
    V = exp._cfg.vocab_size
    assert ck["params:audio/ctc/kernel"].shape == (32, V + 1) and ck["params:audio/ctc/bias"].shape == (V + 1,)
    assert "adam_m:audio/ctc/kernel" in ck.files and np.abs(ck["adam_m:audio/ctc/kernel"]).max() > 0      # the head is being trained
    exp2 = avsr.AVSR(use_ctc=True, ctc_weight=0.5, **kw)
    err = exp2.evaluate("checkpoints/ctc/checkpoint.ckp-2", epoch=2)
    assert set(err) == {"character", "word", "ctc_character"}
    assert np.isfinite(err["ctc_character"]) and err["ctc_character"] >= 0.0
    assert np.array_equal(exp2._model.export_tf_weights("params")["audio/ctc/kernel"], ck["params:audio/ctc/kernel"])
    # the same records without the option: the old key set, and a checkpoint without the head is refused by a use_ctc model
    plain = avsr.AVSR(**kw)
    plain.train(logfile="logs/plain", num_epochs=2)
    plain.save("checkpoints/plain/checkpoint.ckp-1")
    assert set(plain.evaluate("checkpoints/plain/checkpoint.ckp-1", epoch=1)) == {"character", "word"}
    assert not [k for k in np.load("checkpoints/plain/checkpoint.ckp-1.npz").files if "/ctc/" in k]
    with pytest.raises(ValueError, match="audio/ctc/kernel"):
        exp2.restore("checkpoints/plain/checkpoint.ckp-1")

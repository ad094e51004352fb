"""Shallow-fusion language model in beam search on the GPU (csrc/beam_lm.hip, beam_step_kernel's language-model term,
avsr_attn_rnn_fwd_lm, AVSR(lm_checkpoint=...)), against the fp64 reference of tests/ref_beam_lm.py.

* the language-model step kernel alone: log-probabilities and every layer's state to 1e-4 (the project's parity target for logits) at
  row counts under one 16-row tile, with a partial second tile and of whole tiles, widths of 12 and 64, one and two layers, embedded
  and one-hot inputs, over three steps whose parents permute rows, repeat one and drop another;
* the selection with the term on given logits, and its NULL form bit for bit against avsr_beam_search_step;
* the whole search by `follow` (every step of every utterance scored from the engine's own branch; conditions of tests/test_gpu_beam.py);
* weight 0 with a model present: bit-identical to the search without one, under all three avsr_attn_rnn_set_beam_kernel settings;
* end to end through avsr.LM.train and AVSR.evaluate."""
import os

import numpy as np
import pytest
import torch

import ref_beam_lm as R
from oracle import avsr_oracle as O
from test_gpu_beam import TIE

pytestmark = pytest.mark.gpu


def _engine_lm(rng, nl, H, E, V, one_hot, Rn, dev):
    """Random model in TF layout (fp64 reference) and as the avsr_beam_lm descriptor over engine-layout device buffers."""
    from avsr_tf1_amd import _lib, ops, params as PR
    P = {"dec/embedding": np.eye(V, E, dtype=np.float32) if one_hot else rng.standard_normal((V, E)).astype(np.float32)}
    for j in range(nl):
        kin = (E if j == 0 else H) + H
        P["dec/l%d/kernel" % j] = (rng.standard_normal((kin, 4 * H)) * (1.5 / np.sqrt(kin))).astype(np.float32)
        P["dec/l%d/bias" % j] = (rng.standard_normal(4 * H) * 0.3).astype(np.float32)
    P["dec/out/kernel"] = (rng.standard_normal((H, V)) * (3.0 / np.sqrt(H))).astype(np.float32)
    P["dec/out/bias"] = rng.standard_normal(V).astype(np.float32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)
    keep = dict(emb=t(P["dec/embedding"]), wout_t=t(P["dec/out/kernel"].T), bout=t(P["dec/out/bias"]),
                c=torch.full((2, nl, Rn, H), 7.0, device=dev), h=torch.full((2, nl, Rn, H), 7.0, device=dev),    # step 0 must zero what it reads
                logp=torch.zeros(Rn, V, device=dev))
    m = _lib.BeamLm()
    m.n_layers, m.H, m.E, m.V, m.one_hot, m.n_rows, m.lm_weight = nl, H, E, V, int(one_hot), Rn, 0.3
    m.embedding, m.wout_t, m.bout = ops.fptr(keep["emb"]), ops.fptr(keep["wout_t"]), ops.fptr(keep["bout"])
    for j in range(nl):
        keep["wt%d" % j] = t(PR.lstm_kernel_to_engine(P["dec/l%d/kernel" % j]).T)           # [4H][K], gate columns unit-interleaved
        keep["b%d" % j] = t(PR.lstm_bias_to_engine(P["dec/l%d/bias" % j]))
        m.wt[j], m.bias[j] = ops.fptr(keep["wt%d" % j]), ops.fptr(keep["b%d" % j])
    m.state_c, m.state_h, m.lm_logp = ops.fptr(keep["c"]), ops.fptr(keep["h"]), ops.fptr(keep["logp"])
    return P, m, keep


@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("V", [15, 31])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("H", [12, 64])
@pytest.mark.parametrize("Rn", [9, 30, 64])
def test_lm_step_kernel_against_fp64(Rn, H, nl, V, one_hot):
    from avsr_tf1_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1000 * Rn + 10 * H + nl + V)
    E = (V + 3) // 4 * 4 if one_hot else 8
    P, m, keep = _engine_lm(rng, nl, H, E, V, one_hot, Rn, dev)
    assert ops.beam_lm_supported(m)
    Pt = O.to_torch(P, torch.float64)

    class Cfg:
        decoder_units, vocab_size = (H,) * nl, V
    state = R.lm_zero_state(Cfg, Rn)
    guard = torch.full((Rn + 16, V), -123.0, device=dev)                # the step writes rows < R of its output only
    m.lm_logp = ops.fptr(guard)
    for step in range(3):
        tok = rng.integers(0, V, size=Rn)
        par = rng.permutation(Rn)
        par[1] = par[0]                                                  # one parent twice, another one dropped
        state = [(c[par], h[par]) for c, h in state]
        ref_lp, state = R.lm_step(Pt, Cfg, torch.as_tensor(tok), state)
        ops.beam_lm_step(m, torch.as_tensor(tok, dtype=torch.int32).to(dev), torch.as_tensor(par, dtype=torch.int32).to(dev), Rn, step)
        torch.cuda.synchronize()
        got = guard.cpu().numpy()
        assert (got[Rn:] == -123.0).all()
        d_lp = float(np.abs(got[:Rn] - ref_lp.numpy()).max())
        half = (step + 1) & 1
        d_st = max(max(float(np.abs(keep["c"][half, j].cpu().numpy() - state[j][0].numpy()).max()),
                       float(np.abs(keep["h"][half, j].cpu().numpy() - state[j][1].numpy()).max())) for j in range(nl))
        print("step", step, "lm_logp dev", d_lp, "state dev", d_st)
        assert d_lp < 1e-4 and d_st < 1e-4, (step, d_lp, d_st)


def _sel_state(rng, U, K, V, eos, dev, finished):
    logp = np.sort(rng.uniform(-6.0, -1.0, (U, K)))[:, ::-1].copy()
    fin = (rng.random((U, K)) < 0.3) if finished else np.zeros((U, K), bool)
    ln = rng.integers(1, 6, (U, K))
    return logp, fin, ln


@pytest.mark.parametrize("inside", [False, True])
@pytest.mark.parametrize("finished", [False, True])
@pytest.mark.parametrize("K", [3, 10])
def test_selection_with_the_term_on_given_logits(K, finished, inside):
    """inside: the form with the output layer in the step (beam_step_kernel<2, LM>), the one the 256-unit evaluation path launches."""
    from avsr_tf1_amd import ops
    dev = torch.device("cuda:0")
    U, V, eos, w, lmw = 3, 31, 29, 0.6, 0.7
    rng = np.random.default_rng(50 + K + int(finished))
    logits = (rng.standard_normal((U * K, V)) * 3.0).astype(np.float32)
    extra = {}
    if inside:
        Od = 256
        x = rng.standard_normal((U * K, Od)).astype(np.float32)
        wout_t = (rng.standard_normal((V, Od)) * (3.0 / 16.0)).astype(np.float32)
        bout = rng.standard_normal(V).astype(np.float32)
        logits = (x.astype(np.float64) @ wout_t.astype(np.float64).T + bout).astype(np.float32)
        extra = dict(x=torch.as_tensor(x).to(dev), x_stride=Od, O=Od, wout_t=torch.as_tensor(wout_t).to(dev), bout=torch.as_tensor(bout).to(dev))
    lm_lp = torch.log_softmax(torch.as_tensor(rng.standard_normal((U * K, V)) * 3.0), dim=-1).numpy().astype(np.float32)
    logp, fin, ln = _sel_state(rng, U, K, V, eos, dev, finished)
    i32 = dict(dtype=torch.int32, device=dev)
    f = lambda a: torch.as_tensor(a, dtype=torch.float32).to(dev)
    ins = (f(logp.astype(np.float32)).view(-1), torch.as_tensor(fin.astype(np.int32)).to(dev).view(-1), torch.as_tensor(ln.astype(np.int32)).to(dev).view(-1))

    def run(fn, *lm_args):
        out = (torch.zeros(U * K, device=dev), torch.zeros(U * K, **i32), torch.zeros(U * K, **i32))
        tok, prow, sid, pid, nun = (torch.zeros(U * K, **i32), torch.zeros(U * K, **i32), torch.zeros(2, U * K, **i32), torch.zeros(2, U * K, **i32),
                                    torch.zeros(2, **i32))
        fn(f(logits), U, K, V, 0, eos, w, *ins, *out, tok, prow, sid, pid, nun, *lm_args, **extra)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (*out, tok, prow, sid, pid, nun)]

    base = run(ops.beam_search_step)
    null = run(ops.beam_search_step_lm, None, lmw)
    for a, b in zip(base, null):
        assert a.tobytes() == b.tobytes()                               # NULL lm_logp: avsr_beam_search_step bit for bit
    zero = run(ops.beam_search_step_lm, f(lm_lp), 0.0)
    for a, b in zip(base, zero):
        assert a.tobytes() == b.tobytes()                               # weight 0: the same
    got = run(ops.beam_search_step_lm, f(lm_lp), lmw)
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    am = torch.log_softmax(t64(logits.astype(np.float64)), dim=-1).reshape(U, K, V)
    total, scores = R.fused_candidates(t64(logp.astype(np.float32)), torch.as_tensor(fin), torch.as_tensor(ln), am,
                                       t64(lm_lp).reshape(U, K, V), lmw, w, eos)
    order_all = torch.argsort(scores, dim=1, descending=True, stable=True)
    top = torch.gather(scores, 1, order_all[:, :K + 1]).numpy()
    order = order_all[:, :K].numpy()
    sid, pid, glp = got[5][0].reshape(U, K), got[6][0].reshape(U, K), got[0].reshape(U, K)
    strict = 0
    for u in range(U):
        for j in range(K):
            clear = (j == 0 or top[u, j - 1] - top[u, j] > TIE) and top[u, j] - top[u, j + 1] > TIE
            if clear:
                strict += 1
                assert sid[u, j] == order[u, j] % V and pid[u, j] == order[u, j] // V, (u, j)
                assert abs(glp[u, j] - float(total.reshape(U, -1)[u, order[u, j]])) < 1e-4
    assert strict >= U * K // 2
    assert not all(a.tobytes() == b.tobytes() for a, b in zip(base, got))   # the term moved something


def _search(model, db, K, lm, lmw, check_every=3):
    out = model.beam_search_decode(db, beam_width=K, max_steps=R.MAX_STEPS, check_every=check_every, return_all=True, lm=lm, lm_weight=lmw)
    torch.cuda.synchronize()
    assert not model.check_persistent()
    X = model._beam_ws[2]
    T = out.shape[1]
    return dict(out=out.cpu().numpy().copy(), T=T, sid=X["sid"].cpu().numpy().copy(), pid=X["pid"].cpu().numpy().copy(),
                logp=X["logp"].cpu().numpy().copy(), ln=X["ln"].cpu().numpy().copy(), fin=X["fin"].cpu().numpy().copy())


def _models(case, lm="1x10"):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    ocfg, mcfg, W, batch, lcfg, lmcfg, WL = R.search_case(case, lm)
    return Seq2SeqModel(mcfg, weights=W), Seq2SeqModel(lmcfg, weights=WL), Batch.from_numpy(batch)


SETTINGS = [(1, 1), (1, 3), (1, 10), (0, 10), (2, 10), (0, 3), (2, 1)]      # (avsr_attn_rnn_set_beam_kernel setting, K): every K and every mode


@pytest.mark.parametrize("lmw", [0.3, 1.0])
@pytest.mark.parametrize("setting,K", SETTINGS)
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_full_search_follows_the_reference(case, setting, K, lmw):
    _follow(case, setting, K, lmw, "1x10")


@pytest.mark.parametrize("case", ["c1_audio_uni_luong", "c4_bimodal_uni"])
def test_full_search_with_a_two_layer_one_hot_model(case):
    """The host path of deeper models (`dec/l1` kernels, the one-hot input table) through beam_search_decode."""
    _follow(case, 1, 3, 0.3, "2x10_onehot")


def _follow(case, setting, K, lmw, lmname):
    from avsr_tf1_amd import ops
    ocfg, mcfg, W, batch, lcfg, lmcfg, WL = R.search_case(case, lmname)
    try:
        ops.attn_rnn_set_beam_kernel(setting)
        model, lm, db = _models(case, lmname)
        g = _search(model, db, K, lm, lmw)
    finally:
        ops.attn_rnn_set_beam_kernel(1)
    B, T = g["out"].shape[0], g["T"]
    sid, pid = g["sid"].reshape(-1, B, K)[:T], g["pid"].reshape(-1, B, K)[:T]
    ref, lp, ln, tr = R.beam_search_decode_lm(W, ocfg, batch, WL, lcfg, lmw, beam_width=K, max_steps=R.MAX_STEPS, follow=(sid, pid))
    assert T < R.MAX_STEPS                                               # a chunk was queued past the end
    assert not tr["follow_short"] and tr["step_ids"].shape[0] == T, ("the searches stop at different steps", T, tr["step_ids"].shape[0])
    assert tr["follow_distinct"].all()
    worst = float(tr["follow_dev"].max())
    print(case, setting, K, lmw, "follow_dev", worst, "identical selections", float(tr["follow_same"].mean()))
    assert worst < TIE, (worst, np.argwhere(tr["follow_dev"] >= TIE)[:4])
    assert (g["out"] == ref).all()
    par = T & 1
    assert (g["ln"][par].reshape(B, K) == ln).all()
    glp = g["logp"][par].reshape(B, K)
    fin = np.isfinite(lp)
    assert (np.isfinite(glp) == fin).all() and np.abs(glp[fin] - lp[fin]).max() < 1e-4 * max(1.0, np.abs(lp[fin]).max())


@pytest.mark.parametrize("setting", [1, 0, 2])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_weight_zero_is_bit_identical_to_no_model(case, setting):
    from avsr_tf1_amd import ops
    try:
        ops.attn_rnn_set_beam_kernel(setting)
        model, lm, db = _models(case)
        a = _search(model, db, 10, None, 0.0)
        b = _search(model, db, 10, lm, 0.0)
        c = _search(model, db, 10, lm, 1.0)
    finally:
        ops.attn_rnn_set_beam_kernel(1)
    assert a["T"] == b["T"]
    T = a["T"]
    for k in ("out", "logp", "ln", "fin"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["sid"][:T].tobytes() == b["sid"][:T].tobytes() and a["pid"][:T].tobytes() == b["pid"][:T].tobytes()
    assert c["T"] != T or c["logp"].tobytes() != a["logp"].tobytes()      # ... and the model is really in the loop


def test_refusals_on_the_engine():
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    import dataclasses
    model, lm, db = _models("c1_audio_uni_luong")
    lmcfg = R.search_case("c1_audio_uni_luong")[5]
    with pytest.raises(NotImplementedError):
        model.beam_search_decode(db, beam_width=3, max_steps=4, lm=Seq2SeqModel(dataclasses.replace(lmcfg, cell_type="gru")), lm_weight=0.3)
    with pytest.raises(ValueError):
        model.beam_search_decode(db, beam_width=3, max_steps=4, lm=Seq2SeqModel(dataclasses.replace(lmcfg, vocab_size=15, eos_id=13, go_id=14)), lm_weight=0.3)
    with pytest.raises(ValueError):
        model.beam_search_decode(db, beam_width=3, max_steps=4, lm=model, lm_weight=0.3)
    with pytest.raises(ValueError):
        model.greedy_decode(db, max_steps=4, lm=lm)


def test_end_to_end_lm_train_then_fused_evaluate(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import io_utils as IO
    from test_gpu_avsr import _dataset
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=6)
    lkw = dict(unit="character", unit_file=unit_file, labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4),
               decoder_units_per_layer=(12,), embedding_size=8, learning_rate=0.02, shuffle_seed=0)
    avsr.LM(**lkw).train(logfile="logs/lm", num_epochs=2)             # one epoch -> checkpoints/lm/checkpoint.ckp-1
    ck = "checkpoints/lm/checkpoint.ckp-1"
    assert os.path.exists(ck + ".npz")
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"], audio_test_record=p["audio"],
              labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4), encoder_units_per_layer=((16,), (16,)),
              decoder_units_per_layer=(16,), embedding_size=8, beam_width=4, required_grahps=('eval',), shuffle_seed=0)
    plain = avsr.AVSR(**kw)
    plain.save("checkpoints/am/checkpoint.ckp-1")
    err0 = plain.evaluate("checkpoints/am/checkpoint.ckp-1", epoch=0)
    lmkw = dict(lm_checkpoint=ck, lm_units_per_layer=(12,), lm_embedding_size=8)
    out = {}
    for epoch, lmw in ((1, 0.5), (2, 0.0)):
        exp = avsr.AVSR(lm_weight=lmw, **lmkw, **kw)
        err = exp.evaluate("checkpoints/am/checkpoint.ckp-1", epoch=epoch)
        assert set(err) == {"character", "word"} and np.isfinite(err["character"])
        out[epoch] = open("predictions/am/predicted_epoch_%d.mlf" % epoch).read()
    assert out[2] == open("predictions/am/predicted_epoch_0.mlf").read() and len(out[1].splitlines()) >= 6
    with pytest.raises(ValueError):
        avsr.AVSR(lm_units_per_layer=(16,), lm_checkpoint=ck, lm_embedding_size=8, **kw)
    assert avsr.AVSR(**lmkw, **kw)._lm_weight == 0.3

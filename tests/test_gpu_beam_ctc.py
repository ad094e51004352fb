"""Joint CTC / attention scoring in beam search on the GPU (csrc/beam_ctc.hip, avsr_beam_search_step_ctc, avsr_attn_rnn_fwd_ctc,
AVSR(ctc_decode_weight=...)), against the fp64 reference of tests/ref_beam_ctc.py.

* the begin and step kernels alone, on given logits, states and parents (ref_beam_ctc.KERNEL_CASES: T_b of 0, 1, 2, 3, 63, 64, 65, 257
  and 500 mixed within a batch with T above the longest, V of 15 / 31 / 41 with padded row strides, R of 9 / 30 / 64 / 20 rows at widths
  3, 10 and -- 64 rows being no multiple of 3 or 10 -- 4, prefixes of 0, 1 and 4 symbols with a repeated last one and longer than T_b,
  permuted parents with one repeated, EOS and finished rows), over two chained steps so that both halves of the ping-pong are read and
  written.  The -inf pattern of state, psi and term must be the reference's exactly; finite values stay within
  C_TOL * 2^-23 * max(1, max |finite reference value|) (the maximum over the state for the state, over psi(g) and all psi(g . v) for psi
  and term).  C_TOL = 37 = 4 x 9.24, the worst ratio of the float32 restatement against fp64 on these same inputs (t500_r20, step 2;
  measured and checked by tests/test_beam_ctc_cpu.py; the kernel's own worst ratio on an MI355X is 2.45, same case); two launches on the same inputs are bit-identical;
* the selection with the term on given logits: NULL / weight 0 bit for bit avsr_beam_search_step_lm, the fused scores against
  oracle.beam_candidates, and -inf terms that leave fewer than K finite candidates;
* the whole search by `follow` at weights 0.3 and 1.0, every architecture and every avsr_attn_rnn_set_beam_kernel setting, and once
  with a language model and the term together;
* weight 0 and use_ctc=False: bit-identical to the plain search; refusals; end to end through AVSR.train / AVSR.evaluate."""
import numpy as np
import pytest
import torch

import ref_beam_ctc as R
import ref_beam_lm as RL
from oracle import avsr_oracle as O
from test_gpu_beam import TIE
from test_gpu_beam_lm import SETTINGS

pytestmark = pytest.mark.gpu
GUARD = 7.0


def _desc(case, dev, weight=0.3, lm=None):
    """avsr_beam_ctc over device buffers filled with GUARD (whatever a kernel must not write stays GUARD)."""
    from avsr_tf1_amd import _lib, ops
    U, K, V, T, ld = case["U"], case["K"], case["V"], case["T"], case["ld"]
    Rn = U * K
    f = lambda *s: torch.full(s, GUARD, device=dev)
    keep = dict(z=torch.as_tensor(case["z"]).reshape(U * T, ld).to(dev), in_len=torch.as_tensor(case["Tb"]).to(dev),
                y=f(U, T, V + 1), state=f(2, Rn, T, 2), psi=f(2, Rn),
                last=torch.full((2, Rn), 77, dtype=torch.int32, device=dev), term=f(Rn + 4, V), extra=f(Rn + 4, V))
    c = _lib.BeamCtc()
    c.n_utt, c.beam_width, c.T, c.V, c.eos_id, c.weight, c.ld = U, K, T, V, case["eos"], weight, ld
    c.z, c.in_len, c.y, c.state = ops.fptr(keep["z"]), ops.fptr(keep["in_len"]), ops.fptr(keep["y"]), ops.fptr(keep["state"])
    c.psi, c.last, c.term, c.extra = ops.fptr(keep["psi"]), ops.fptr(keep["last"]), ops.fptr(keep["term"]), ops.fptr(keep["extra"])
    if lm is not None:
        keep["lm"] = torch.as_tensor(lm).to(dev)
        c.lm_logp, c.lm_weight = ops.fptr(keep["lm"]), 0.7
    return c, keep


@pytest.mark.parametrize("name", list(R.KERNEL_CASES))
def test_begin_and_step_kernels_against_fp64(name):
    from avsr_tf1_amd import ops
    dev = torch.device("cuda:0")
    case = R.kernel_case(name)
    U, K, V, T, eos = case["U"], case["K"], case["V"], case["T"], case["eos"]
    Rn = U * K
    Tb = np.repeat(case["Tb"].astype(np.int64), K)
    m = np.arange(T)[None, :] < Tb[:, None]
    y64, start, outs = R.kernel_reference(case)
    lm = torch.log_softmax(torch.as_tensor(np.random.default_rng(1).standard_normal((Rn, V)) * 2.0), dim=-1).numpy().astype(np.float32) \
        if name == "r30_v31" else None
    c, keep = _desc(case, dev, lm=lm)
    assert ops.beam_ctc_supported(c)
    # ---- once per decode: y, and the empty prefix in half 0 ----
    ops.beam_ctc_begin(c)
    torch.cuda.synchronize()
    y = keep["y"].cpu().numpy()
    mu = np.arange(T)[None, :] < case["Tb"][:, None]
    dy = float(np.abs(y[mu] - y64[mu]).max()) / (2.0 ** -23 * max(1.0, float(np.abs(y64[mu]).max()))) if mu.any() else 0.0
    st = keep["state"].cpu().numpy()
    ref0 = R.empty_state(np.repeat(y64, K, axis=0), Tb)
    d0 = float(np.abs(st[0, :, :, 1][m] - ref0["rb"][m]).max()) / (2.0 ** -23 * max(1.0, float(np.abs(ref0["rb"][m]).max())))
    print(name, "begin: y ratio %.2f, blank prefix sum ratio %.2f (C_TOL %.0f)" % (dy, d0, R.C_TOL))
    assert (y[~mu] == GUARD).all() and (st[0][~m] == GUARD).all() and (st[1] == GUARD).all()        # rows t >= T_b, the other half: untouched
    assert np.isneginf(st[0, :, :, 0][m]).all() and dy <= R.C_TOL and d0 <= R.C_TOL
    assert (keep["psi"][0].cpu().numpy() == 0).all() and (keep["last"][0].cpu().numpy() == -1).all()
    # ---- the given state goes into half 1; step 1 reads it and writes half 0, step 2 reads half 0 and writes half 1 ----
    up = np.full((Rn, T, 2), GUARD, np.float32)
    up[:, :, 0][m], up[:, :, 1][m] = start["rn"][m], start["rb"][m]
    keep["state"][1].copy_(torch.as_tensor(up))
    keep["psi"][1].copy_(torch.as_tensor(start["psi"]))
    keep["last"][1].copy_(torch.as_tensor(start["last"].astype(np.int32)))
    i32 = lambda a: torch.as_tensor(a, dtype=torch.int32).to(dev)

    def run(s):
        tok, par, fin = case["steps"][s - 1]
        ops.beam_ctc_step(c, i32(tok), i32(par), i32(fin), s)
        torch.cuda.synchronize()
        h = (s + 1) & 1
        stt = keep["state"][h].cpu().numpy()
        return (dict(rn=stt[:, :, 0].copy(), rb=stt[:, :, 1].copy(), psi=keep["psi"][h].cpu().numpy().copy(),
                     last=keep["last"][h].cpu().numpy().astype(np.int64)), keep["term"].cpu().numpy().copy(), keep["extra"].cpu().numpy().copy())

    first = run(1)
    again = run(1)
    for a, b in zip((first[0]["rn"], first[0]["rb"], first[0]["psi"], first[1], first[2]),
                    (again[0]["rn"], again[0]["rb"], again[0]["psi"], again[1], again[2])):
        assert a.tobytes() == b.tobytes()                                  # two launches on the same inputs: bit-identical
    for s, got in ((1, first), (2, run(2))):
        gs, gt, ge = got
        assert (gt[Rn:] == GUARD).all() and (ge[Rn:] == GUARD).all()
        assert (gs["rn"][~m] == GUARD).all() and (gs["rb"][~m] == GUARD).all()
        ratio = R.deviation((gs, gt[:Rn]), outs[s - 1], Tb, (name, s))
        print(name, "step", s, "worst |got - fp64| / (2^-23 scale) = %.2f (C_TOL %.0f)" % (ratio, R.C_TOL))
        assert ratio <= R.C_TOL, (name, s, ratio)
        # extra: the pre-combined buffer the selection reads
        fin = case["steps"][s - 1][2].astype(bool) | (case["steps"][s - 1][0] == eos)
        want = np.float32(0.3) * gt[:Rn]
        if lm is not None:
            want = np.where(fin[:, None], 0.0, want.astype(np.float64) + np.float64(np.float32(0.7)) * lm)
        assert np.array_equal(np.isneginf(ge[:Rn]), np.isneginf(want)) and not np.isnan(ge).any()
        f = np.isfinite(want)
        assert np.abs(ge[:Rn][f] - want[f]).max() <= 1e-6 * max(1.0, np.abs(want[f]).max())


def _sel_inputs(U, K, V, seed, finished):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((U * K, V)) * 3.0).astype(np.float32)
    lm_lp = torch.log_softmax(torch.as_tensor(rng.standard_normal((U * K, V)) * 3.0), dim=-1).numpy().astype(np.float32)
    term = (-np.abs(rng.standard_normal((U * K, V))) * 4.0).astype(np.float32)
    term[rng.random((U * K, V)) < 0.2] = -np.inf
    logp = np.sort(rng.uniform(-6.0, -1.0, (U, K)))[:, ::-1].copy()
    fin = (rng.random((U, K)) < 0.3) if finished else np.zeros((U, K), bool)
    ln = rng.integers(1, 6, (U, K))
    return logits, lm_lp, term, logp, fin, ln


def _run_sel(fn, logits, U, K, V, eos, w, logp, fin, ln, *args):
    dev = torch.device("cuda:0")
    i32 = dict(dtype=torch.int32, device=dev)
    f = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float32).to(dev)
    ins = (f(logp.astype(np.float32)).view(-1), torch.as_tensor(fin.astype(np.int32)).to(dev).view(-1), torch.as_tensor(ln.astype(np.int32)).to(dev).view(-1))
    out = (torch.zeros(U * K, device=dev), torch.zeros(U * K, **i32), torch.zeros(U * K, **i32))
    tok, prow, sid, pid, nun = (torch.zeros(U * K, **i32), torch.zeros(U * K, **i32), torch.zeros(2, U * K, **i32), torch.zeros(2, U * K, **i32),
                                torch.zeros(2, **i32))
    args = [f(a) if isinstance(a, np.ndarray) else a for a in args]
    fn(f(logits), U, K, V, 0, eos, w, *ins, *out, tok, prow, sid, pid, nun, *args)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (*out, tok, prow, sid, pid, nun)]


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("finished", [False, True])
@pytest.mark.parametrize("K", [3, 10])
def test_selection_with_the_term_on_given_logits(K, finished, with_lm):
    from avsr_tf1_amd import ops
    U, V, eos, w, lmw, cw = 3, 31, 29, 0.6, 0.7, 0.5
    logits, lm_lp, term, logp, fin, ln = _sel_inputs(U, K, V, 70 + K + int(finished), finished)
    lm_arg = lm_lp if with_lm else None
    scratch = np.full((U * K, V), GUARD, np.float32)
    run = lambda fn, *a: _run_sel(fn, logits, U, K, V, eos, w, logp, fin, ln, *a)
    base = run(ops.beam_search_step_lm, lm_arg, lmw)
    for a, b in zip(base, run(ops.beam_search_step_ctc, lm_arg, lmw, None, cw, scratch)):
        assert a.tobytes() == b.tobytes()                               # NULL term: today's entry bit for bit
    for a, b in zip(base, run(ops.beam_search_step_ctc, lm_arg, lmw, term, 0.0, scratch)):
        assert a.tobytes() == b.tobytes()                               # weight 0: the same
    got = run(ops.beam_search_step_ctc, lm_arg, lmw, term, cw, scratch)
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    am = torch.log_softmax(t64(logits.astype(np.float64)), dim=-1).reshape(U, K, V)
    step_lp = am + (lmw * t64(lm_lp).reshape(U, K, V) if with_lm else 0.0) + cw * t64(term).reshape(U, K, V)
    total, scores = O.beam_candidates(t64(logp.astype(np.float32)), torch.as_tensor(fin), torch.as_tensor(ln), step_lp, w, eos)
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


def test_selection_with_fewer_than_K_finite_candidates():
    """Step 0 of a search (only beam 0 alive) with a term that leaves two symbols possible: K = 3 distinct selections, the two finite
    ones first in score order, the third an -inf candidate in index order (beam 0, symbol 0)."""
    from avsr_tf1_amd import ops
    U, K, V, eos, w = 2, 3, 15, 13, 0.6
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((U * K, V)) * 2.0).astype(np.float32)
    term = np.full((U * K, V), -np.inf, np.float32)
    term[:, 4], term[:, 9] = -1.0, -0.25
    logp = np.full((U, K), -np.inf)
    logp[:, 0] = 0.0
    fin, ln = np.zeros((U, K), bool), np.zeros((U, K), np.int64)
    got = _run_sel(ops.beam_search_step_ctc, logits, U, K, V, eos, w, logp, fin, ln, None, 0.0, term, 1.0, np.zeros((U * K, V), np.float32))
    glp, sid, pid = got[0].reshape(U, K), got[5][0].reshape(U, K), got[6][0].reshape(U, K)
    am = torch.log_softmax(torch.as_tensor(logits.astype(np.float64)), dim=-1).numpy().reshape(U, K, V)
    for u in range(U):
        cand = sorted(((am[u, 0, v] + float(term[u * K, v]), v) for v in (4, 9)), reverse=True)
        assert len({(int(p), int(s)) for p, s in zip(pid[u], sid[u])}) == K
        assert [int(s) for s in sid[u, :2]] == [v for _s, v in cand] and (pid[u, :2] == 0).all()
        assert np.allclose(glp[u, :2], [s for s, _v in cand], atol=1e-5) and np.isneginf(glp[u, 2])
        assert (int(pid[u, 2]), int(sid[u, 2])) == (0, 0)
    assert not np.isnan(glp).any()


def _search(model, db, K, cw, lm=None, lmw=0.0, check_every=3):
    out = model.beam_search_decode(db, beam_width=K, max_steps=R.MAX_STEPS, check_every=check_every, return_all=True, lm=lm, lm_weight=lmw,
                                   ctc_weight=cw)
    torch.cuda.synchronize()
    assert not model.check_persistent()
    X = model._beam_ws[2]
    return dict(out=out.cpu().numpy().copy(), T=out.shape[1], sid=X["sid"].cpu().numpy().copy(), pid=X["pid"].cpu().numpy().copy(),
                logp=X["logp"].cpu().numpy().copy(), ln=X["ln"].cpu().numpy().copy(), fin=X["fin"].cpu().numpy().copy())


def _models(case, lm="1x10"):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    ocfg, mcfg, W, batch, lcfg, lmcfg, WL = R.search_case(case, lm)
    return Seq2SeqModel(mcfg, weights=W), Seq2SeqModel(lmcfg, weights=WL), Batch.from_numpy(batch)


def _follow(case, setting, K, cw, lmname=None, lmw=0.0):
    from avsr_tf1_amd import ops
    ocfg, mcfg, W, batch, lcfg, lmcfg, WL = R.search_case(case, lmname or "1x10")
    try:
        ops.attn_rnn_set_beam_kernel(setting)
        model, lm, db = _models(case, lmname or "1x10")
        g = _search(model, db, K, cw, lm if lmname else None, lmw)
    finally:
        ops.attn_rnn_set_beam_kernel(1)
    B, T = g["out"].shape[0], g["T"]
    sid, pid = g["sid"].reshape(-1, B, K)[:T], g["pid"].reshape(-1, B, K)[:T]
    lmargs = dict(lm_np=WL, lcfg=lcfg, lm_weight=lmw) if lmname else {}
    ref, lp, ln, tr = R.beam_search_decode_ctc(W, ocfg, batch, cw, beam_width=K, max_steps=R.MAX_STEPS, follow=(sid, pid), **lmargs)
    assert T < R.MAX_STEPS                                               # a chunk was queued past the end
    assert not tr["follow_short"] and tr["step_ids"].shape[0] == T, ("the searches stop at different steps", T, tr["step_ids"].shape[0])
    assert tr["follow_distinct"].all()
    worst = float(tr["follow_dev"].max())
    print(case, setting, K, cw, lmname, "follow_dev", worst, "identical selections", float(tr["follow_same"].mean()))
    assert worst < TIE, (worst, np.argwhere(tr["follow_dev"] >= TIE)[:4])
    assert (g["out"] == ref).all()
    par = T & 1
    assert (g["ln"][par].reshape(B, K) == ln).all()
    glp = g["logp"][par].reshape(B, K)
    fin = np.isfinite(lp)
    assert (np.isfinite(glp) == fin).all() and np.abs(glp[fin] - lp[fin]).max() < 1e-4 * max(1.0, np.abs(lp[fin]).max())


@pytest.mark.parametrize("cw", list(R.WEIGHTS))
@pytest.mark.parametrize("setting,K", SETTINGS)
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_full_search_follows_the_reference(case, setting, K, cw):
    _follow(case, setting, K, cw)


@pytest.mark.parametrize("setting,K", [(1, 10), (0, 3)])
def test_full_search_with_a_language_model_and_the_term(setting, K):
    _follow("c2_audio_bi_bahdanau", setting, K, 0.5, "1x10", 0.3)


@pytest.mark.parametrize("setting", [1, 0, 2])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_weight_zero_and_no_head_are_bit_identical_to_the_plain_search(case, setting):
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.model import Seq2SeqModel
    try:
        ops.attn_rnn_set_beam_kernel(setting)
        model, lm, db = _models(case)
        _o, plain_cfg, plain_W = RL.search_case(case)[:3]
        a = _search(Seq2SeqModel(plain_cfg, weights=plain_W), db, 10, 0.0)      # use_ctc=False: the search as it was
        b = _search(model, db, 10, 0.0)
        c = _search(model, db, 10, 1.0)
    finally:
        ops.attn_rnn_set_beam_kernel(1)
    assert not plain_cfg.use_ctc and a["T"] == b["T"]
    T = a["T"]
    for k in ("out", "logp", "ln", "fin"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["sid"][:T].tobytes() == b["sid"][:T].tobytes() and a["pid"][:T].tobytes() == b["pid"][:T].tobytes()
    # ... and the term is really in the loop (tests/test_beam_ctc_cpu.py: the reference alone satisfies this)
    assert c["T"] != T or c["sid"][:T].tobytes() != a["sid"][:T].tobytes() or c["pid"][:T].tobytes() != a["pid"][:T].tobytes()
    assert c["logp"].tobytes() != a["logp"].tobytes()


def test_refusals_on_the_engine():
    from avsr_tf1_amd.model import Seq2SeqModel
    model, lm, db = _models("c1_audio_uni_luong")
    _o, plain_cfg, plain_W = RL.search_case("c1_audio_uni_luong")[:3]
    with pytest.raises(ValueError, match="use_ctc"):
        Seq2SeqModel(plain_cfg, weights=plain_W).beam_search_decode(db, beam_width=3, max_steps=4, ctc_weight=0.3)
    with pytest.raises(ValueError, match=">= 0"):
        model.beam_search_decode(db, beam_width=3, max_steps=4, ctc_weight=-0.5)
    with pytest.raises(ValueError, match="beam"):
        model.greedy_decode(db, max_steps=4, ctc_weight=0.3)
    assert model.greedy_decode(db, max_steps=4, ctc_weight=0.0).shape[0] == 3


def test_end_to_end_train_with_use_ctc_then_joint_evaluate(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from test_gpu_avsr import _dataset
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=6)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"], audio_test_record=p["audio"],
              labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4), encoder_units_per_layer=((16,), (16,)),
              decoder_units_per_layer=(16,), embedding_size=8, beam_width=4, warmup_steps=0, learning_rate=0.01, shuffle_seed=0, use_ctc=True)
    exp = avsr.AVSR(**kw)
    assert exp._ctc_decode_weight == 0.0
    exp.train(logfile="logs/j", num_epochs=3)                             # two epochs
    exp.save("checkpoints/j/checkpoint.ckp-2")
    err0 = exp.evaluate("checkpoints/j/checkpoint.ckp-2", epoch=0)        # built without the option
    out = {}
    for epoch, cw in ((1, 0.5), (2, 0.0)):
        e = avsr.AVSR(ctc_decode_weight=cw, **kw)
        assert e._ctc_decode_weight == cw
        err = e.evaluate("checkpoints/j/checkpoint.ckp-2", epoch=epoch)
        assert set(err) == {"character", "word", "ctc_character"} and all(np.isfinite(v) for v in err.values())
        out[epoch] = open("predictions/j/predicted_epoch_%d.mlf" % epoch).read()
    assert out[2] == open("predictions/j/predicted_epoch_0.mlf").read() and len(out[1].splitlines()) >= 6
    assert err["ctc_character"] == err0["ctc_character"]
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(ctc_decode_weight=0.5, **dict(kw, use_ctc=False))

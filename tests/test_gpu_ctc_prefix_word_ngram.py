"""CTC prefix beam search over characters with a fused word-level n-gram behind a lexicon trie, on the GPU
(csrc/ctc_prefix_word_ngram.hip): the kernel through the C ABI -- every frame of its trace followed by the fp64 checker of
tests/ref_ctc_prefix_lm.py with the string-and-dictionary model of tests/ref_word_ngram.py, the final re-sort, s_lm, lm_steps and the
debug lam rows; whole searches against the fp64 rule where the reference's margins allow it; the limit shape -- then
Seq2SeqModel.ctc_prefix_beam_search(word_ngram=...) on the oracle's evaluation-mode head logits and the AVSR front door
(ctc_word_ngram_lm).

Tolerances are ref_ctc_prefix_lm's search tolerances with ref_word_ngram.WORD_PARITY as the model's share of one term (both docstrings
derive them).  The debug rows are also held, bit for bit, to ngram.word_lam, the numpy restatement of the kernel's step over the same
tables.  A whole search is compared only where the reference's smallest margin exceeds the tolerance, and at most a third of a
configuration's 64 seeds may be left out (tests/test_word_ngram_cpu.py checks that cap on the reference alone)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_ctc as RC  # noqa: E402
import ref_ctc_prefix as R  # noqa: E402
import ref_ctc_prefix_lm as RL  # noqa: E402
import ref_word_ngram as RW  # noqa: E402

pytestmark = pytest.mark.gpu
NEG = -np.inf
_DEV = {}
TABLES = ("bow", "backoff", "arc_begin", "sym", "logp", "next", "t_begin", "t_sym", "t_next", "t_word")
SCALARS = ("n_nodes", "n_arcs", "Vw", "start", "eos_w", "unk_id", "n_trie_nodes", "n_trie_arcs", "V", "space_id", "go_id", "eos_id")
# found by searching seeds 0..199 with R.reentered under the fused rule with both SEARCH_MODELS on RW.inputs (V = 6: two letters; seed
# 12 is the first that both models share)
REENTRY_WORD = dict(V=6, T=12, W=3, L_max=8, s=1.0, seed=12, w=0.5, beta=0.5)
MODEL_IDS = dict(ids=lambda m: "order%d_%s" % (m[0], "unk" if m[1] else "nounk"))


def _device_tables(order, V, unk):
    key = (order, V, unk)
    if key not in _DEV:
        t = RW.shared_model(order, V, unk)["tables"]
        _DEV[key] = {k: torch.as_tensor(np.ascontiguousarray(t[k])).to("cuda") for k in TABLES}
    return _DEV[key]


def _descriptor(t, D, w, beta, **over):
    from avsr_tf1_amd import _lib, ops
    g = _lib.CtcPrefixWordNgram()
    for k in SCALARS:
        setattr(g, k, int(over.get(k, t[k])))
    g.weight, g.bonus, g.oov = w, beta, float(t["oov_score"])
    for k in TABLES:
        setattr(g, k, ops.fptr(D[k]))
    return g


def _launch(z, in_len, V, W, L_max, model, w, beta, trace=True, fill=77.0, tail=64, debug=True):
    """z [B, T, ld] float32 (ld >= V + 1).  Outputs are allocated `tail` elements too long and pre-filled, so that what the kernel leaves
    alone can be seen.  Returns dict(ids [B, W, L_max], lens, score, s_lm [B, W], lm_steps [B], lm_logp [B, W, V], parent / sym / pb /
    pnb [B, T, W])."""
    from avsr_tf1_amd import ops
    B, T, ld = z.shape
    dev = "cuda"
    t, D = RW.shared_model(model[0], V, model[1])["tables"], _device_tables(model[0], V, model[1])
    zd = torch.tensor(np.ascontiguousarray(z).reshape(B * T, ld), device=dev)
    ld_ = torch.tensor(np.asarray(in_len, np.int32), device=dev)
    fi = lambda n: torch.full((n + tail,), int(fill), dtype=torch.int32, device=dev)
    ff = lambda n: torch.full((n + tail,), float(fill), device=dev)
    bufs = dict(ids=fi(B * W * L_max), lens=fi(B * W), score=ff(B * W), s_lm=ff(B * W), lm_steps=fi(B))
    if debug:
        bufs["lm_logp"] = ff(B * W * V)
    if trace:
        bufs.update(parent=fi(B * T * W), sym=fi(B * T * W), pb=ff(B * T * W), pnb=ff(B * T * W))
    assert ops.ctc_prefix_word_ngram_supported(V, W, L_max, t["n_nodes"], t["n_arcs"], t["Vw"], t["n_trie_nodes"], t["n_trie_arcs"])
    g = _descriptor(t, D, w, beta)
    g.s_lm, g.lm_steps = ops.fptr(bufs["s_lm"]), ops.fptr(bufs["lm_steps"])
    if debug:
        g.lm_logp = ops.fptr(bufs["lm_logp"])
    tr = tuple(bufs[k] for k in ("parent", "sym", "pb", "pnb")) if trace else None
    before = {k: D[k].clone() for k in TABLES}
    ops.ctc_prefix_search_word_ngram(zd, ld, ld_, B, T, V, W, L_max, bufs["ids"], bufs["lens"], bufs["score"], g, trace=tr)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], D[k]) for k in TABLES), "the tables are read-only"
    shapes = dict(ids=(B, W, L_max), lens=(B, W), score=(B, W), s_lm=(B, W), lm_steps=(B,), lm_logp=(B, W, V))
    res = {}
    for k, tt in bufs.items():
        v = tt.cpu().numpy()
        n = v.size - tail
        assert (v[n:] == (int(fill) if v.dtype.kind == "i" else np.float32(fill))).all(), ("written past the end of", k)
        res[k] = v[:n].reshape(shapes.get(k, (B, T, W)))
    return res


def _final_of(out, b, W):
    """[(labels, final)] of utterance b as the kernel returned it, after checking the padding rules of the output."""
    beam = []
    for r in range(W):
        n, p = int(out["lens"][b, r]), float(out["score"][b, r])
        row = out["ids"][b, r]
        assert not np.isnan(p) and not np.isnan(out["s_lm"][b, r])
        if p == NEG:
            assert n == 0 and (row == -1).all() and (out["score"][b, r:] == NEG).all() and out["s_lm"][b, r] == 0.0, ("an empty slot", b, r)
            if "lm_logp" in out:
                assert (out["lm_logp"][b, r] == 0.0).all()
            continue
        assert (row[n:] == -1).all() and (row[:n] >= 0).all()
        beam.append((tuple(int(s) for s in row[:n]), p))
    return beam


def _state_of(t, g):
    from avsr_tf1_amd import ngram
    st = ngram.word_start(t)
    for c in g:
        st = ngram.word_step(t, st, c)
    return st


def _check_rows(out, b, got, e):
    """The debug lam rows and s_lm against fp64 recomputation from the returned ids (WORD_PARITY per term), and the rows against
    ngram.word_lam over the same tables bit for bit: a state that followed the wrong slot fails both."""
    from avsr_tf1_amd import ngram
    for r, (g, _f) in enumerate(got):
        row = out["lm_logp"][b, r]
        assert not np.isnan(row).any() and np.isfinite(row).all()
        d = float(np.abs(row - e["ref"].lam(g)).max())
        assert d <= RW.WORD_PARITY, ("lam row of the wrong label sequence?", b, r, g, d)
        assert np.array_equal(row, ngram.word_lam(e["tables"], _state_of(e["tables"], g))), (b, r, g)
        assert abs(float(out["s_lm"][b, r]) - e["ref"].s_lm(g)) <= (len(g) + 1) * RW.WORD_PARITY, (b, r, g)


def _check_utterance(out, b, z, Tb, V, W, L_max, e, w, beta, tol):
    """Trace check of utterance b (z [T, V + 1]), then the final re-sort, s_lm, the lam rows and lm_steps."""
    T = z.shape[0]
    Tb = min(max(int(Tb), 0), T)
    tol = tol + w * RW.WORD_PARITY
    lm = e["ref"]
    final, steps = RL.check_trace_lm(z, Tb, W, L_max, out["parent"][b], out["sym"][b], out["pb"][b], out["pnb"][b], lm, w, beta, tol)
    got = _final_of(out, b, W)
    RL.check_final_lm(got, out["s_lm"][b], final, lm, w, tol)
    _check_rows(out, b, got, e)
    assert int(out["lm_steps"][b]) == steps, (int(out["lm_steps"][b]), steps)
    for k in ("parent", "sym", "pb", "pnb"):
        assert (out[k][b, Tb:] == 77).all(), ("trace rows past T_b are not written", k)
    return got


def _search_ok(got, ref, w):
    want = dict(ref["beam"])
    assert {g for g, _p in got} == set(want) and len(got) == len(ref["beam"])
    assert got[0][0] == ref["beam"][0][0]
    for r, (g, p) in enumerate(got):
        tol = RL.TOL_SEARCH_LM + w * RW.WORD_PARITY * (len(g) + 1)
        assert abs(p - float(want[g])) <= tol, (r, g, p, want[g])
        assert abs(float(want[g]) - float(ref["beam"][r][1])) <= tol, (r, g)


# ------------------------------------------------------------------------------------------------
# 1. the kernel: every frame of every input followed by the checker
@pytest.mark.parametrize("wb", RL.WEIGHTS, ids=lambda p: "w%g_b%g" % p)
@pytest.mark.parametrize("shift", R.BLANK_SHIFTS)
@pytest.mark.parametrize("model", RW.MODELS, **MODEL_IDS)
@pytest.mark.parametrize("cfg", RL.KERNEL_CONFIGS, ids=lambda c: "V%d_T%d_W%d_L%d_s%d" % c)
def test_kernel_trace_follows_the_fused_rule(cfg, model, shift, wb):
    V, T, W, L_max, s = cfg
    w, beta = wb
    e = RW.shared_model(model[0], V, model[1])
    z = RW.inputs(V, T, s, 0, L_max, shift)
    out = _launch(z[None], [T], V, W, L_max, model, w, beta)
    got = _check_utterance(out, 0, z, T, V, W, L_max, e, w, beta, RL.TOL_STEP_LM_LONG if T > 40 else RL.TOL_STEP_LM)
    assert len(got) == W
    print(cfg, model, shift, wb, "lengths", sorted({len(g) for g, _p in got}), "best", got[0][1], "lm_steps", int(out["lm_steps"][0]))
    assert 0 < int(out["lm_steps"][0]) <= T          # (the boosted alignment outweighs the blank's shift: frames keep extensions at + 8 too)


@pytest.mark.parametrize("model", RW.SEARCH_MODELS, **MODEL_IDS)
def test_kernel_reentry_of_a_prefix_whose_extension_stayed(model):
    """An input on which, under the fused rule with each of the two word models, a prefix leaves the beam and is re-created while its
    one-symbol extension stayed: the re-created prefix gets a fresh pool row (and state) and the next frame must merge the two."""
    c = REENTRY_WORD
    V, T, W, L_max = c["V"], c["T"], c["W"], c["L_max"]
    e = RW.shared_model(model[0], V, model[1])
    z = RW.inputs(V, T, c["s"], c["seed"], L_max)
    ref = RL.search_lm(z, T, W, L_max, e["ref"], c["w"], c["beta"])
    assert R.reentered(ref["beams"])
    out = _launch(z[None], [T], V, W, L_max, model, c["w"], c["beta"])
    got = _check_utterance(out, 0, z, T, V, W, L_max, e, c["w"], c["beta"], RL.TOL_STEP_LM)
    if ref["margin"] > RW.search_tol(ref, c["w"]):
        _search_ok(got, ref, c["w"])


def test_kernel_mixed_lengths_wide_rows_and_poisoned_padding():
    """T_b = 0, 1, < T, = T, > T (clamped) and negative in one batch; rows of ld = V + 5 floats whose pad columns, and whole frames past
    T_b, hold 100.0 on a non-blank: neither is ever read, so the launch equals one on the clean logits bit for bit."""
    V, T, W, L_max, ld, model, w, beta = 31, 40, 10, 16, 36, (3, True), 0.5, 0.5
    e = RW.shared_model(model[0], V, model[1])
    lm = e["ref"]
    Tbs = [0, 1, 7, 23, T, T + 9, -2]
    B = len(Tbs)
    clean = np.stack([RW.inputs(V, T, 4, 100 + b, L_max) for b in range(B)])
    z = np.full((B, T, ld), 100.0, np.float32)
    z[..., :V + 1] = clean
    for b, tb in enumerate(Tbs):
        z[b, max(min(tb, T), 0):, :V] = -5.0
        z[b, max(min(tb, T), 0):, 3] = 100.0
    out = _launch(z, Tbs, V, W, L_max, model, w, beta)
    for b, tb in enumerate(Tbs):
        got = _check_utterance(out, b, clean[b], tb, V, W, L_max, e, w, beta, RL.TOL_STEP_LM)
        if tb <= 0:                                                       # the empty sequence: final = w lam(EOS | ()), s_lm = lam(EOS | ())
            assert [g for g, _p in got] == [()] and int(out["lm_steps"][b]) == 0
            assert abs(got[0][1] - w * float(lm.lam(())[lm.eos])) <= w * RW.WORD_PARITY
        if tb == 1:
            assert max(len(g) for g, _p in got) == 1
    ref = _launch(clean, [min(max(t, 0), T) for t in Tbs], V, W, L_max, model, w, beta)
    for k in out:
        assert np.array_equal(out[k], ref[k]), k


def test_kernel_is_deterministic_and_writes_nothing_else():
    V, T, W, L_max, s, model, w, beta = 41, 40, 10, 16, 5, (3, True), 0.5, 0.5
    z = np.stack([RW.inputs(V, T, s, seed, L_max) for seed in range(6)])
    a = _launch(z, [T] * 6, V, W, L_max, model, w, beta, fill=77.0)
    b = _launch(z, [T] * 6, V, W, L_max, model, w, beta, fill=-3.0)               # (_launch asserts the tails kept their fill)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    c = _launch(z, [T] * 6, V, W, L_max, model, w, beta, trace=False, debug=False)   # production form: no trace, no debug rows
    for k in ("ids", "lens", "score", "s_lm", "lm_steps"):
        assert np.array_equal(a[k], c[k]), k


@pytest.mark.parametrize("model", RW.SEARCH_MODELS, **MODEL_IDS)
@pytest.mark.parametrize("cfg", RL.KERNEL_CONFIGS[:5], ids=lambda c: "V%d_T%d_W%d_L%d_s%d" % c)
def test_weight_zero_equals_the_plain_search_bit_for_bit(cfg, model):
    """w = 0, beta = 0 against avsr_ctc_prefix_search on the same logits: ids, lens and score (every term is finite: 0 * lam is an exact 0)."""
    from avsr_tf1_amd import ops
    V, T, W, L_max, s = cfg
    z = np.stack([RW.inputs(V, T, s, seed, L_max, shift) for seed in range(4) for shift in (0.0, 3.0)])
    B = z.shape[0]
    out = _launch(z, [T] * B, V, W, L_max, model, 0.0, 0.0, trace=False)
    zd = torch.tensor(z.reshape(B * T, V + 1), device="cuda")
    ids = torch.zeros(B, W, L_max, dtype=torch.int32, device="cuda")
    lens = torch.zeros(B, W, dtype=torch.int32, device="cuda")
    score = torch.zeros(B, W, device="cuda")
    ops.ctc_prefix_search(zd, V + 1, torch.full((B,), T, dtype=torch.int32, device="cuda"), B, T, V, W, L_max, ids, lens, score)
    torch.cuda.synchronize()
    assert np.array_equal(out["ids"], ids.cpu().numpy()) and np.array_equal(out["lens"], lens.cpu().numpy())
    assert np.array_equal(out["score"], score.cpu().numpy())


# ------------------------------------------------------------------------------------------------
# 2. whole searches against the fp64 rule
@pytest.mark.parametrize("model", RW.SEARCH_MODELS, **MODEL_IDS)
@pytest.mark.parametrize("cfg", RL.SEARCH_CONFIGS, ids=lambda c: "V%d_T%d_W%d_L%d_s%d" % c)
def test_whole_search_equals_the_fp64_rule(cfg, model):
    V, T, W, L_max, _s = cfg
    w, beta = 0.5, 0.5
    e = RW.shared_model(model[0], V, model[1])
    zs, refs = RW.references(cfg, model[0], model[1], w, beta)
    out = _launch(zs, [T] * 64, V, W, L_max, model, w, beta, trace=False)
    left_out = 0
    for i, ref in enumerate(refs):
        got = _final_of(out, i, W)
        _check_rows(out, i, got, e)                                        # (whatever the margins are)
        if not ref["margin"] > RW.search_tol(ref, w):
            left_out += 1
            continue
        _search_ok(got, ref, w)
    print(cfg, model, "left out", left_out, "of 64")
    assert left_out <= 64 // 3                                             # a condition on the inputs: the fp64 reference alone decides it


# ------------------------------------------------------------------------------------------------
# 3. the limit shape: V = 256, W = 16, L_max = 512 -- a workgroup of about 70 KiB of LDS, above the 64 KiB a kernel gets unasked
def test_limit_shape_runs_and_one_step_beyond_is_refused_before_any_launch():
    from avsr_tf1_amd import _lib, ops
    V, W, L_max, T, model = 256, 16, 512, 4, (3, True)
    e = RW.shared_model(model[0], V, model[1])
    t = e["tables"]
    z = np.stack([RW.inputs(V, T, 2, seed, L_max) for seed in range(2)])
    out = _launch(z, [T, T], V, W, L_max, model, 0.5, 0.5)
    for b in range(2):
        got = _check_utterance(out, b, z[b], T, V, W, L_max, e, 0.5, 0.5, RL.TOL_STEP_LM)
        assert len(got) == W
    D = _device_tables(model[0], V, model[1])
    buf = torch.zeros(1 << 16, device="cuda")
    ibuf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def shape(V_=V, W_=W, L_=L_max, **over):
        sizes = {k: over.get(k, t[k]) for k in ("n_nodes", "n_arcs", "Vw", "n_trie_nodes", "n_trie_arcs")}
        a = _lib.CtcPrefixArgs()
        a.B, a.T, a.V, a.beam_width, a.L_max, a.ld = 1, 1, V_, W_, L_, V_ + 1
        a.z, a.in_len, a.ids, a.lens, a.score = ops.fptr(buf), ops.fptr(ibuf), ops.fptr(ibuf), ops.fptr(ibuf), ops.fptr(buf)
        g = _descriptor(t, D, 0.5, 0.5, V=V_, go_id=V_ - 1, eos_id=V_ - 2, **sizes)
        g.s_lm, g.lm_steps = ops.fptr(buf), ops.fptr(ibuf)
        ok = ops.ctc_prefix_word_ngram_supported(V_, W_, L_, sizes["n_nodes"], sizes["n_arcs"], sizes["Vw"], sizes["n_trie_nodes"],
                                                 sizes["n_trie_arcs"])
        return ok, lib.avsr_ctc_prefix_search_word_ngram(C.byref(a), C.byref(g), None)

    before = (buf.clone(), ibuf.clone())
    MN, MA = _lib.CTC_PREFIX_NGRAM_MAX_NODES, _lib.CTC_PREFIX_NGRAM_MAX_ARCS
    for beyond in (dict(V_=V + 1), dict(W_=W + 1), dict(L_=L_max + 1), dict(n_nodes=MN + 1), dict(n_arcs=MA + 1), dict(n_trie_nodes=MN + 1),
                   dict(n_trie_arcs=MA + 1)):
        assert shape(**beyond) == (False, -3), beyond                         # AVSR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(before[0], buf) and torch.equal(before[1], ibuf)     # nothing was launched


# ------------------------------------------------------------------------------------------------
# 4. the engine: Seq2SeqModel.ctc_prefix_beam_search(word_ngram=...) against the fp64 rule on the oracle's evaluation-mode head logits
def test_model_search_equals_the_fused_rule_on_the_oracle_logits():
    """tests/test_gpu_ctc_prefix.py's allowance for the engine's own head logits (d = max |z_engine - z_oracle| <= 1e-5 moves every sum
    over alignments by at most 2 T_b d) next to the fused rule's: tol = TOL_SEARCH_LM + 2 T_b d + w * WORD_PARITY * (len + 1)."""
    from test_gpu_ctc import _make
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, Wt, batch, stream = _make("c1_audio_uni_luong")
    enc = O.encoder_outputs({k: v for k, v in Wt.items() if "/ctc/" not in k}, ocfg, batch, training=False)[stream][0]
    kn, bn = RC.head_names(stream)
    z = enc @ Wt[kn].astype(np.float64) + Wt[bn].astype(np.float64)
    lens = np.asarray(batch.audio_len if stream == "audio" else batch.video_len)
    B, T, Cc = z.shape
    V = Cc - 1
    assert (ocfg.vocab_size, ocfg.go_id, ocfg.eos_id) == (V, V - 1, V - 2) and V == 31
    model = Seq2SeqModel(dataclasses.replace(mcfg, use_ctc=True), weights=Wt)
    e = RW.shared_model(3, V, True)
    tables, ref_lm = e["tables"], e["ref"]
    bt = Batch.from_numpy(batch)
    compared = total = 0
    for W, L_max, w, beta in ((1, None, 0.5, 0.5), (4, None, 0.3, 0.0), (10, None, 0.5, 0.5), (10, 6, 0.5, 0.5), (16, None, 1.0, -0.5)):
        got = model.ctc_prefix_beam_search(bt, beam_width=W, max_steps=L_max, nbest=True, word_ngram=tables, lm_weight=w, length_bonus=beta)
        best = model.ctc_prefix_beam_search(bt, beam_width=W, max_steps=L_max, word_ngram=tables, lm_weight=w, length_bonus=beta)
        steps = model._last_ctc_lm_steps.cpu().numpy()
        ws = model._get_ws(B, model._audio_rows(bt), bt.video.shape[1] if bt.video is not None else 0, 1, True)
        ze = ws["enc"][stream]["ctc_z"].view(B, T, Cc).cpu().numpy()
        assert len(got) == len(best) == B
        for b in range(B):
            d = float(np.abs(ze[b, :lens[b]] - z[b, :lens[b]]).max())
            assert d <= 1e-5, (b, d)
            ref = RL.search_lm(z[b], lens[b], W, L_max or mcfg.max_label_length, ref_lm, w, beta)
            assert best[b] == got[b][0][0] and 0 <= steps[b] <= lens[b]
            assert all(isinstance(s, int) for s in best[b]) and all(np.isfinite(f) and np.isfinite(s) for _g, f, s in got[b])
            for g, _f, s in got[b]:                                         # whatever the margins are: s_lm belongs to the returned ids
                assert abs(s - ref_lm.s_lm(g)) <= (len(g) + 1) * RW.WORD_PARITY, (W, b, g)
            tol = RL.TOL_SEARCH_LM + 2 * lens[b] * d + w * RW.WORD_PARITY * (max(len(g) for g, _f in ref["beam"]) + 1)
            total += 1
            if not ref["margin"] > tol:
                continue
            compared += 1
            want = dict(ref["beam"])
            assert tuple(got[b][0][0]) == ref["beam"][0][0]
            assert {tuple(g) for g, _f, _s in got[b]} == set(want) and len(got[b]) == len(ref["beam"])
            for r, (g, f, _s) in enumerate(got[b]):
                assert abs(f - float(want[tuple(g)])) <= tol and abs(float(want[tuple(g)]) - float(ref["beam"][r][1])) <= tol, (W, b, r)
    print("compared", compared, "of", total)
    assert 2 * compared >= total
    assert len(model._ngram_tables) == 1                                     # uploaded once per model object
    plain = model.ctc_prefix_beam_search(bt, beam_width=10, nbest=True)        # without a model: today's pairs; weight 0: the same ids and scores
    zero = model.ctc_prefix_beam_search(bt, beam_width=10, nbest=True, word_ngram=tables, lm_weight=0.0, length_bonus=0.0)
    assert [[(g, p) for g, p, _s in u] for u in zero] == plain and all(len(e_) == 2 for u in plain for e_ in u)
    with pytest.raises(ValueError, match="16"):
        model.ctc_prefix_beam_search(bt, beam_width=17, word_ngram=tables)
    with pytest.raises(ValueError, match="cannot be combined"):
        model.ctc_prefix_beam_search(bt, word_ngram=tables, lm=model)
    with pytest.raises(ValueError, match="compiled for"):
        model.ctc_prefix_beam_search(bt, word_ngram=RW.shared_model(1, V + 2, False)["tables"])


# ------------------------------------------------------------------------------------------------
# 5. the front door
def test_avsr_evaluates_with_the_word_ngram_prefix_search(tmp_path, monkeypatch):
    import avsr_tf1_amd as avsr
    from avsr_tf1_amd import ngram
    from avsr_tf1_amd.utils import _strip_extra_chars
    from test_gpu_avsr import _dataset
    monkeypatch.chdir(tmp_path)
    unit_file, p = _dataset(str(tmp_path), n=8)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"],
              audio_test_record=p["audio"], labels_train_record=p["labels"], labels_test_record=p["labels"], batch_size=(4, 4),
              encoder_units_per_layer=((32,), (32, 32)), decoder_units_per_layer=(32,), embedding_size=16, warmup_steps=0,
              learning_rate=0.01, shuffle_seed=0, use_ctc=True, decoding_algorithm="ctc_prefix_beam_search", beam_width=10)
    exp = avsr.AVSR(**kw)
    assert exp._ctc_word_ngram is None
    exp.train(logfile="logs/prefix", num_epochs=3)                         # two epochs
    exp.save("checkpoints/prefix/checkpoint.ckp-2")
    exp.evaluate("checkpoints/prefix/checkpoint.ckp-2", epoch=0)
    mlf_plain = open(os.path.join("predictions", "prefix", "predicted_epoch_0.mlf")).read()
    ud = exp._unit_dict
    texts = ["".join(ud[s] for s in seq) for seq in ngram.label_sequences(ud, label_record=p["labels"])]
    vocabulary = ["<s>", "</s>"] + sorted({w for t in texts for w in t.split()} | {"<unk>"})
    ids = {w: i for i, w in enumerate(vocabulary)}
    arpa = str(tmp_path / "words.arpa")
    ngram.write_word_arpa(arpa, ngram.estimate([[ids[w] for w in t.split()] for t in texts], 2, ngram.word_dict(vocabulary)), vocabulary)
    default = avsr.AVSR(ctc_word_ngram_lm=arpa, **kw)
    g = default._ctc_word_ngram
    assert default._ctc_lm_weight == 0.3 and default._ctc_lm_bonus == 0.0 and g["order"] == 2 and g["oov_score"] == -10.0
    assert g["unk_id"] == ids["<unk>"] and g["n_unspellable"] == 0 and g["n_trie_nodes"] > 1

    fused = avsr.AVSR(ctc_word_ngram_lm=arpa, ctc_word_oov_score=-4.0, ctc_lm_weight=2.0, ctc_lm_length_bonus=0.5, **kw)
    assert fused._ctc_word_ngram["oov_score"] == -4.0

    def no_decoder(*a, **k):
        raise AssertionError("the attention decoder must not run under ctc_prefix_beam_search")
    monkeypatch.setattr(fused._model, "beam_search_decode", no_decoder)
    monkeypatch.setattr(fused._model, "greedy_decode", no_decoder)
    err = fused.evaluate("checkpoints/prefix/checkpoint.ckp-2", epoch=1)
    assert set(err) == {"character", "word", "ctc_character"}
    assert all(np.isfinite(v) and v >= 0.0 for v in err.values())
    mlf = open(os.path.join("predictions", "prefix", "predicted_epoch_1.mlf")).read().splitlines()
    assert len(mlf) == 8
    lines = {l.split(" ", 1)[0]: l for l in mlf}
    model, voc = ngram.read_word_arpa(arpa)
    V = len(ud) - 1
    rule = _FrontDoorRef(model, voc, ud, V, -4.0)
    seen = compared = 0
    for bd in fused._iterator("evaluate"):                                 # the .mlf holds what the fp64 rule predicts on the engine's logits
        batch, names = fused._to_batch(bd)
        ids_ = fused._model.ctc_prefix_beam_search(batch, beam_width=10, max_steps=fused._cfg.max_label_length,
                                                   word_ngram=fused._ctc_word_ngram, lm_weight=2.0, length_bonus=0.5)
        B = len(names)
        ws = fused._model._get_ws(B, fused._model._audio_rows(batch), 0, 1, True)
        E = ws["enc"]["audio"]
        ze = E["ctc_z"].view(B, E["T"], -1)[..., :V + 1].cpu().numpy().astype(np.float64)
        tl = E["len"].cpu().numpy()
        for b, (name, seq) in enumerate(zip(names, ids_)):
            hyp = "".join(_strip_extra_chars([fused._unit_dict[s] for s in seq]))
            assert lines[name.decode("utf-8")].startswith("%s %s [" % (name.decode("utf-8"), hyp)), (name, hyp)
            seen += 1
            ref = RL.search_lm(ze[b], tl[b], 10, fused._cfg.max_label_length, rule, 2.0, 0.5)
            if ref["margin"] > RL.TOL_SEARCH_LM + 2.0 * RW.WORD_PARITY * (max(len(g_) for g_, _p in ref["beam"]) + 1):
                assert tuple(seq) == ref["beam"][0][0], (name, seq, ref["beam"][0])
                compared += 1
    print("compared with the fp64 rule", compared, "of", seen)
    assert seen == 8 and 2 * compared >= seen
    zero = avsr.AVSR(ctc_word_ngram_lm=arpa, ctc_lm_weight=0.0, ctc_lm_length_bonus=0.0, **kw)
    monkeypatch.setattr(zero._model, "beam_search_decode", no_decoder)
    monkeypatch.setattr(zero._model, "greedy_decode", no_decoder)
    zero.evaluate("checkpoints/prefix/checkpoint.ckp-2", epoch=2)
    assert open(os.path.join("predictions", "prefix", "predicted_epoch_2.mlf")).read() == mlf_plain      # byte for byte


class _FrontDoorRef(RW.WordRef):
    """WordRef over a unit file's own classes (the space and the letters where the unit file puts them)."""

    def __init__(self, model, vocabulary, ud, V, oov):
        super().__init__(model, vocabulary, V, oov)
        rev = {s: i for i, s in ud.items()}
        self.space = rev[" "]
        self.chars = {i: s for i, s in ud.items() if s not in ("MASK", "END", "GO", "EOS", " ")}
        alphabet = set(self.chars.values())
        self.words = {w for w in vocabulary if w not in ("<s>", "</s>", "<unk>", "<UNK>") and w and set(w) <= alphabet}
        self.prefixes = {w[:k] for w in self.words for k in range(len(w) + 1)}

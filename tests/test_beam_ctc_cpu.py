"""Joint CTC / attention scoring in beam search, the parts that need no GPU: the prefix scorer of tests/ref_beam_ctc.py against brute
force and against the CTC loss, the -inf rules, the fp64 searches the GPU test compares with (they end, the term moves them, weight 0
is the plain search, an fp32 evaluation of the term stays a quarter of TIE away from fp64), and the refusals raised on the host."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import ref_beam_ctc as R
import ref_ctc as RC
from oracle import avsr_oracle as O

TIE = 2e-5          # tests/test_gpu_beam.py: candidate scores closer than this may be ordered either way by fp32 arithmetic


def _y(T, C, seed, scale=2.0):
    return R.log_softmax(np.random.default_rng(seed).standard_normal((T, C)) * scale)


@pytest.mark.parametrize("T,Tb", [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (5, 3)])
def test_prefix_score_against_brute_force(T, Tb):
    """Every prefix g of up to three symbols over {0, 1} (repeats included), extended by c in {0, 1} (c == last included): psi(g . c)
    from the state recursion AND from the recursion-free log-sum-exp equals the sum over all 3^T alignments."""
    Cc, blank = 3, 2
    y1 = _y(T, Cc, 10 * T + Tb)
    n = 0
    for L in range(0, 4):
        for g in itertools.product(range(2), repeat=L):
            y, st = R.prefix_state(y1, Tb, list(g))
            want_g = R.brute_force_psi(y1[:Tb], list(g), blank)
            assert np.isclose(st["psi"][0], want_g, rtol=1e-12, atol=1e-12) or (st["psi"][0] == want_g == -np.inf), (g, st["psi"], want_g)
            pe = R.psi_ext(y, [Tb], st, None)
            for c in range(2):
                want = R.brute_force_psi(y1[:Tb], list(g) + [c], blank)
                got_state = R.extend(y, [Tb], st, [c])["psi"][0]
                for got in (got_state, pe[0, c]):
                    assert (got == want == -np.inf) or np.isclose(got, want, rtol=1e-12, atol=1e-12), (g, c, got, want)
                n += 1
    assert n == 2 * (1 + 2 + 4 + 8)


def test_eos_extension_is_the_ctc_loss_and_terms_telescope():
    V, T, eos = 5, 9, 3
    rng = np.random.default_rng(3)
    z = rng.standard_normal((1, T, V + 1)) * 2.0
    y1 = R.log_softmax(z[0])
    for g, Tb in (([], 9), ([1], 9), ([1, 1], 9), ([0, 2, 2, 4], 9), ([4, 0, 4], 5), ([2, 2, 2], 5), ([0, 1, 2, 4, 0], 5)):
        labels = np.array([g + [eos] + [0] * (7 - len(g))])
        nll, _U, _Tb = RC.ctc_nll(torch.as_tensor(z), labels, [len(g) + 1], [Tb], V)
        y, st = R.prefix_state(y1, Tb, [])
        total = 0.0
        for c in g + [eos]:
            tm = R.term(y, [Tb], st, eos)[0, c]
            total += tm
            if c != eos:
                st = R.extend(y, [Tb], st, [c])
        pe = R.psi_ext(y, [Tb], st, eos)[0, eos]
        assert np.isclose(pe, -float(nll[0]), rtol=1e-10), (g, pe, nll)
        assert np.isclose(total, -float(nll[0]), rtol=1e-10), (g, total, nll)            # weight * log p_ctc(labels | x) accumulates


def test_the_minus_infinity_rules():
    V, T, eos = 4, 6, 2
    y1 = _y(T, V + 1, 7)
    # a prefix longer than the frames can carry: psi = -inf, and that (dead) row's term is 0, not NaN
    y, st = R.prefix_state(y1, 2, [0, 1, 3])
    assert st["psi"][0] == -np.inf and (R.term(y, [2], st, eos) == 0).all()
    # the last prefix that fits: every extension is impossible (-inf) except EOS
    y, st = R.prefix_state(y1, 2, [0, 1])
    tm = R.term(y, [2], st, eos)[0]
    assert np.isfinite(st["psi"][0]) and np.isfinite(tm[eos]) and (tm[np.arange(V) != eos] == -np.inf).all()
    # a repeated symbol needs a blank between: "0 0" does not fit two frames
    y, st = R.prefix_state(y1, 2, [0])
    assert R.term(y, [2], st, eos)[0, 0] == -np.inf and np.isfinite(R.term(y, [2], st, eos)[0, 1])
    # no frames at all: term 0 for every row, whatever the prefix
    for g in ([], [1]):
        y, st = R.prefix_state(y1, 0, g)
        assert (R.term(y, [0], st, eos) == 0).all()
    # a finished row gets no term; nothing anywhere is NaN, in fp64 and in the float32 restatement
    for dt in (np.float64, np.float32):
        yy = np.repeat(y1[None].astype(dt), 4, axis=0)
        Tb = np.array([6, 2, 0, 1])
        st = R.empty_state(yy, Tb)
        fin = np.zeros(4, bool)
        for s, tok in enumerate(([1, 1, 1, 1], [0, 0, 0, 0], [0, 3, 0, eos], [1, 1, 1, 1], [1, eos, 1, 1])):
            st, tm = R.step(yy, Tb, st, tok, [0, 1, 2, 3], fin, s, eos)
            fin = fin | (np.array(tok) == eos) if s > 0 else fin
            assert tm.dtype == dt and not np.isnan(tm).any() and not np.isnan(st["psi"]).any()
            assert (tm[fin] == 0).all() and (tm[2] == 0).all()
            m = np.arange(6)[None, :] < Tb[:, None]
            assert not np.isnan(st["rn"][m]).any() and not np.isnan(st["rb"][m]).any()
        assert st["psi"][1] == -np.inf or fin[1]


def test_tolerance_of_the_kernel_test_is_four_times_the_float32_restatement():
    """C_TOL of tests/test_gpu_beam_ctc.py's step-kernel comparison: the float32 restatement against fp64 on the very inputs of that
    test, worst ratio over all cases and both chained steps, times four (the margin covers another summation order)."""
    worst = 0.0
    for name in R.KERNEL_CASES:
        case = R.kernel_case(name)
        Tb = np.repeat(case["Tb"].astype(np.int64), case["K"])
        _y64, _s, o64 = R.kernel_reference(case, np.float64)
        _y32, _s, o32 = R.kernel_reference(case, np.float32)
        for s in range(2):
            r = R.deviation(o32[s][:2], o64[s], Tb, name)
            print(name, "step", s + 1, "float32 restatement / (2^-23 scale) = %.2f" % r)
            worst = max(worst, r)
        assert any(np.isneginf(o[1]).any() for o in o64) or name in ("r30_v41_stride44", "t500_r20")      # the -inf rules are exercised
    assert 4.0 * worst <= R.C_TOL < 4.0 * worst + 1.0, worst


_memo = {}


def _searches(case, K):
    """Plain, weight-0 and weighted fp64 searches of a shared case, computed once."""
    if (case, K) not in _memo:
        ocfg, mcfg, W, batch, lcfg, lmcfg, WL = R.search_case(case)
        out = {"plain": O.beam_search_decode(W, ocfg, batch, beam_width=K, max_steps=R.MAX_STEPS, return_all=True, return_trace=True)}
        for w in (0.0,) + R.WEIGHTS:
            out[w] = R.beam_search_decode_ctc(W, ocfg, batch, w, beam_width=K, max_steps=R.MAX_STEPS)
        _memo[(case, K)] = out
    return _memo[(case, K)]


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("case", list(R.ARCHS))
def test_reference_searches_end_and_the_term_moves_them(case, K):
    S = _searches(case, K)
    ids0, tr0 = S["plain"][0], S["plain"][-1]
    a = S[0.0]
    assert (a[0] == ids0).all() and a[3]["step_ids"].tobytes() == tr0["step_ids"].tobytes()        # weight 0: oracle.beam_search_decode
    assert a[3]["parent_ids"].tobytes() == tr0["parent_ids"].tobytes()
    for w in R.WEIGHTS:
        ids, lp, ln, tr = S[w]
        T = tr["step_ids"].shape[0]
        assert T < R.MAX_STEPS and tr["finished"].all(), (case, K, w, T)
        assert not any(np.isnan(t).any() for t in tr["terms"])
        # the GPU test's "the term moved something": another number of steps, or other selections
        assert T != a[3]["step_ids"].shape[0] or tr["step_ids"].tobytes() != a[3]["step_ids"].tobytes() or \
            tr["parent_ids"].tobytes() != a[3]["parent_ids"].tobytes(), (case, K, w)
        fin = np.isfinite(lp)
        assert fin[:, 0].all()


@pytest.mark.parametrize("case", list(R.ARCHS))
def test_float32_restatement_follows_fp64_within_a_quarter_of_TIE(case):
    """What entitles the GPU test to the follow_dev bound TIE: a search whose term comes from the float32 restatement, followed by the
    fp64 reference, deviates by less than TIE / 4 on every shared case, weight and beam width."""
    ocfg, mcfg, W, batch, lcfg, lmcfg, WL = R.search_case(case)
    for K in (1, 3, 10):
        for w in R.WEIGHTS:
            ids, lp, ln, tr = R.beam_search_decode_ctc(W, ocfg, batch, w, beam_width=K, max_steps=R.MAX_STEPS, term_dtype=np.float32)
            _i, _l, _n, tf = R.beam_search_decode_ctc(W, ocfg, batch, w, beam_width=K, max_steps=R.MAX_STEPS,
                                                      follow=(tr["step_ids"], tr["parent_ids"]))
            worst = float(tf["follow_dev"].max())
            print(case, K, w, "float32 restatement follow_dev", worst)
            assert not tf["follow_short"] and worst < TIE / 4, (case, K, w, worst)


def test_search_with_a_language_model_and_the_term_together():
    ocfg, mcfg, W, batch, lcfg, lmcfg, WL = R.search_case("c1_audio_uni_luong")
    import ref_beam_lm as RL
    a = RL.beam_search_decode_lm(W, ocfg, batch, WL, lcfg, 0.3, beam_width=3, max_steps=R.MAX_STEPS)
    b = R.beam_search_decode_ctc(W, ocfg, batch, 0.0, WL, lcfg, 0.3, beam_width=3, max_steps=R.MAX_STEPS)
    assert (a[0] == b[0]).all() and np.array_equal(a[1], b[1])                                   # weight 0 with a model: the LM search
    c = R.beam_search_decode_ctc(W, ocfg, batch, 0.5, WL, lcfg, 0.3, beam_width=3, max_steps=R.MAX_STEPS)
    assert c[3]["step_ids"].shape[0] < R.MAX_STEPS
    assert c[3]["step_ids"].tobytes() != b[3]["step_ids"].tobytes() or c[3]["parent_ids"].tobytes() != b[3]["parent_ids"].tobytes()


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    p = 64                                          # any non-NULL address: the checks return before a launch could read it

    def ctc(**over):
        c = _lib.BeamCtc()
        c.n_utt, c.beam_width, c.T, c.V, c.eos_id, c.weight, c.ld = 3, 10, 50, 31, 29, 0.3, 32
        c.z = c.in_len = c.y = c.state = c.psi = c.last = c.term = c.extra = p
        for k, v in over.items():
            setattr(c, k, v)
        return c

    sup = lambda c: lib.avsr_beam_ctc_supported(None if c is None else C.byref(c))
    ok = ctc()
    assert sup(ok) == 1 and sup(None) == 0
    assert sup(ctc(T=_lib.BEAM_CTC_MAX_T + 1)) == 0 and sup(ctc(T=_lib.BEAM_CTC_MAX_T)) == 1 and sup(ctc(T=0)) == 0
    assert sup(ctc(V=_lib.BEAM_CTC_MAX_V + 1, ld=300)) == 0 and sup(ctc(beam_width=65)) == 0 and sup(ctc(ld=31)) == 0
    assert sup(ctc(weight=-0.1)) == 0 and sup(ctc(weight=float("nan"))) == 0 and sup(ctc(eos_id=31)) == 0
    assert sup(ctc(term=None)) == 0 and sup(ctc(state=None)) == 0 and sup(ctc(in_len=None)) == 0
    begin = lambda c: lib.avsr_beam_ctc_begin(None if c is None else C.byref(c), None)
    assert begin(None) == -1 and begin(ctc(y=None)) == -1 and begin(ctc(T=5000)) == -3
    step = lambda c, tok=p, par=p, fin=p, s=0: lib.avsr_beam_ctc_step(None if c is None else C.byref(c), tok, par, fin, s, None)
    assert step(None) == -1 and step(ok, tok=None) == -1 and step(ok, par=None) == -1 and step(ok, fin=None) == -1 and step(ok, s=-1) == -1
    assert step(ctc(beam_width=65)) == -3
    d = _lib.AttnRnn()
    d.mode, d.V, d.B, d.beam_width, d.eos_id = 3, 31, 30, 10, 29
    fwd = lambda dd, c, m=None: lib.avsr_attn_rnn_fwd_ctc(None if dd is None else C.byref(dd), m, None if c is None else C.byref(c), 0, 1, None)
    assert fwd(None, ok) == -1 and fwd(d, None) == -1
    assert fwd(d, ctc(V=15, eos_id=3)) == -1 and fwd(d, ctc(n_utt=2)) == -1 and fwd(d, ctc(eos_id=28)) == -1 and fwd(d, ctc(T=5000)) == -3
    assert fwd(d, ctc(lm_logp=p)) == -1                                    # a language-model buffer without its descriptor
    d.mode = 1
    assert fwd(d, ok) == -1
    # the selection with the term: a term without its scratch buffer, a negative weight; then the checks of avsr_beam_search_step
    sel = lambda logits=p, K=10, term=p, w=0.3, extra=p: lib.avsr_beam_search_step_ctc(
        logits, 2, K, 31, 0, 29, 0.6, p, p, p, p, p, p, p, p, p, p, p, None, 0, 0, None, None, None, 0.0, term, w, extra, None)
    assert sel(extra=None) == -1 and sel(w=-1.0) == -1
    assert sel(logits=None, term=None) == -1 and sel(K=0, term=None) == -1 and sel(K=40, w=0.0) == -3


def _unit_file(tmp_path, symbols="' abcdefghijklmnopqrstuvwxyz"):
    f = os.path.join(str(tmp_path), "units_%d" % len(symbols))
    open(f, "w").write("\n".join(list(symbols)) + "\n")
    return f


def test_avsr_refuses_what_the_joint_scoring_does_not_cover(tmp_path):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    kw = dict(unit="character", unit_file=_unit_file(tmp_path))
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(ctc_decode_weight=0.3, **kw)
    with pytest.raises(ValueError, match=">= 0"):
        avsr.AVSR(use_ctc=True, ctc_decode_weight=-0.1, **kw)
    with pytest.raises(ValueError, match="beam"):
        avsr.AVSR(use_ctc=True, ctc_decode_weight=0.3, decoding_algorithm="greedy", **kw)
    with pytest.raises(ValueError, match="64"):
        avsr.AVSR(use_ctc=True, ctc_decode_weight=0.3, beam_width=65, **kw)
    big = "".join(chr(0x100 + i) for i in range(300))
    with pytest.raises(ValueError, match="256"):
        avsr.AVSR(use_ctc=True, ctc_decode_weight=0.3, **dict(kw, unit_file=_unit_file(tmp_path, big)))

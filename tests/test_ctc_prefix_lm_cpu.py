"""CTC prefix beam search with a fused language model, the parts that need no GPU: the fp64 rule of tests/ref_ctc_prefix_lm.py against
brute force over all alignments (the unpruned identity) and against the plain search at weight 0, the input the GPU test uses for a prefix
that leaves the beam and returns under the fused rule, its trace checker, the C entry points' argument and limit answers, and what
`AVSR(ctc_lm_checkpoint=...)` refuses on the host -- with the pinned `lm_checkpoint` refusals still in place."""
import ctypes as C

import numpy as np
import pytest

import ref_ctc_prefix as R
import ref_ctc_prefix_lm as RL
from test_beam_lm_cpu import _lm_checkpoint, _unit_file

# found by searching seeds 0..199 with R.reentered under the fused rule (the hits are seeds 13 and 133)
REENTRY_LM = dict(V=3, T=12, W=3, L_max=8, s=1.0, seed=13, lm="1x12e8", w=0.5, beta=0.5)


@pytest.mark.parametrize("w,beta", [(0.5, 0.5), (0.3, 0.0), (1.0, -0.7)])
def test_unpruned_final_is_ctc_plus_weighted_lm_plus_length_bonus(w, beta):
    """Each alignment of g takes each label's term exactly once: without pruning final = log p_ctc(g | x) + w s_lm + beta len(g).
    V = 2, T = 3: W = 16 holds all 9 label sequences."""
    V, T = 2, 3
    lm = RL.shared_lm("1x12e8", V)[0]
    z = R.kernel_inputs(V, T, 2.0, 11)
    want = R.brute_force(R.log_softmax(z))
    assert len(want) == 9
    out = RL.search_lm(z, T, 16, T, lm, w, beta)
    got = dict(out["beam"])
    assert set(got) == set(want) and len(out["beam"]) == 9
    for g, f in got.items():
        assert abs(f - (want[g] + w * lm.s_lm(g) + beta * len(g))) <= 2e-15, (g, f)
    fs = [f for _g, f in out["beam"]]
    assert fs == sorted(fs, reverse=True)


@pytest.mark.parametrize("cfg", [(5, 10, 4, 6, 2.0), (15, 24, 4, 12, 2.0), (3, 12, 3, 8, 1.0)])
def test_weight_zero_is_the_plain_search(cfg):
    V, T, W, L, s = cfg
    lm = RL.shared_lm("1x12e8", V)[0]
    for seed in range(4):
        z = R.kernel_inputs(V, T, s, seed)
        a, b = R.search(z, T, W, L), RL.search_lm(z, T, W, L, lm, 0.0, 0.0)
        assert a["beam"] == b["beam"] and a["margin"] == b["margin"]
        assert [[(g, float(x), float(y)) for g, x, y in bm] for bm in a["beams"]] == [[(g, float(x), float(y)) for g, x, y in bm] for bm in b["beams"]]


def test_no_frames_give_the_empty_sequence_with_its_eos_term():
    lm = RL.shared_lm("1x12e8", 3)[0]
    z = R.kernel_inputs(3, 6, 2.0, 7)
    for Tb in (0, -3):
        out = RL.search_lm(z, Tb, 4, 5, lm, 0.5, 0.5)
        assert out["beam"] == [((), 0.5 * lm.lam(())[lm.eos])] and out["margin"] == np.inf
    assert lm.s_lm(()) == float(lm.lam(())[lm.eos])


def test_the_language_model_changes_what_is_kept_and_the_final_order():
    """The term must matter on the tests' inputs, or the GPU comparison would not see it."""
    V, T, W, L, s = RL.SEARCH_CONFIGS[0]
    lm = RL.shared_lm("1x12e8", V)[0]
    moved = resorted = 0
    for seed in range(8):
        z = R.kernel_inputs(V, T, s, seed)
        a, b = R.search(z, T, W, L), RL.search_lm(z, T, W, L, lm, 0.5, 0.5)
        moved += [g for g, _p in a["beam"]] != [g for g, _p in b["beam"]]
        resorted += [g for g, _f in b["beam"]] != [g for g, _a, _b in b["beams"][-1]]
    assert moved >= 4 and resorted >= 1, (moved, resorted)


def test_the_reentry_input_holds_a_prefix_that_leaves_the_beam_and_returns():
    c = REENTRY_LM
    lm = RL.shared_lm(c["lm"], c["V"])[0]
    z = R.kernel_inputs(c["V"], c["T"], c["s"], c["seed"])
    out = RL.search_lm(z, c["T"], c["W"], c["L_max"], lm, c["w"], c["beta"])
    hits = R.reentered(out["beams"])
    assert hits and hits[0][0] < c["T"], hits                                     # ... with a frame left in which its extension merges
    assert out["margin"] > 10 * (RL.TOL_SEARCH_LM + c["w"] * RL.LM_PARITY * (c["L_max"] + 1))      # the GPU test may compare the whole search
    for beam in out["beams"]:
        assert len({g for g, _a, _b in beam}) == len(beam)


def _trace_of(out, z, T, V, W, L, lm, w, beta):
    par, sym = np.full((T, W), -1, np.int32), np.full((T, W), -1, np.int32)
    pb, pnb = np.full((T, W), -np.inf, np.float32), np.full((T, W), -np.inf, np.float32)
    y = R.log_softmax(z)
    for t in range(T):
        cands = RL.frame_lm(out["beams"][t], y[t], L, lm, w, beta)
        for r, (g, a, b) in enumerate(out["beams"][t + 1]):
            par[t, r], sym[t, r], pb[t, r], pnb[t, r] = cands[g][2] // (V + 1), cands[g][2] % (V + 1), a, b
    return par, sym, pb, pnb


def test_trace_checker_accepts_the_reference_and_rejects_what_it_must():
    V, T, W, L, w, beta = 5, 10, 4, 6, 0.5, 0.5
    lm = RL.shared_lm("1x12e8", V)[0]
    z = R.kernel_inputs(V, T, 2.0, 2)
    out = RL.search_lm(z, T, W, L, lm, w, beta)
    par, sym, pb, pnb = _trace_of(out, z, T, V, W, L, lm, w, beta)
    tol = RL.TOL_STEP_LM + w * RL.LM_PARITY
    final, steps = RL.check_trace_lm(z, T, W, L, par, sym, pb, pnb, lm, w, beta, tol)
    assert [g for g, _a, _b in final] == [g for g, _a, _b in out["beams"][-1]]
    assert steps == sum(bool((sym[t] >= 0).any() and (sym[t][sym[t] >= 0] < V).any()) for t in range(T)) and 0 < steps <= T
    s_lm = [lm.s_lm(g) for g, _f in out["beam"]]
    RL.check_final_lm(out["beam"], s_lm, final, lm, w, tol)
    with pytest.raises(AssertionError):                                            # the plain rule's numbers do not pass: the term is checked
        plain = R.search(z, T, W, L)
        RL.check_trace_lm(z, T, W, L, *_trace_of_plain(plain, z, T, V, W, L), lm, w, beta, tol)
    bad = pb.copy()
    bad[3, 1] += 0.01
    with pytest.raises(AssertionError):
        RL.check_trace_lm(z, T, W, L, par, sym, bad, pnb, lm, w, beta, tol)
    if len(out["beam"]) > 1:
        with pytest.raises(AssertionError):                                        # the final beam left in slot order where the re-sort moves it
            swapped = [out["beam"][1], out["beam"][0]] + out["beam"][2:]
            RL.check_final_lm(swapped, [lm.s_lm(g) for g, _f in swapped], final, lm, w, tol)
    with pytest.raises(AssertionError):                                            # s_lm of another label sequence
        RL.check_final_lm(out["beam"], s_lm[1:] + s_lm[:1], final, lm, w, tol)


def _trace_of_plain(out, z, T, V, W, L):
    par, sym = np.full((T, W), -1, np.int32), np.full((T, W), -1, np.int32)
    pb, pnb = np.full((T, W), -np.inf, np.float32), np.full((T, W), -np.inf, np.float32)
    y = R.log_softmax(z)
    for t in range(T):
        cands = R.frame(out["beams"][t], y[t], L)
        for r, (g, a, b) in enumerate(out["beams"][t + 1]):
            par[t, r], sym[t, r], pb[t, r], pnb[t, r] = cands[g][2] // (V + 1), cands[g][2] % (V + 1), a, b
    return par, sym, pb, pnb


def test_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    sup = lib.avsr_ctc_prefix_lm_supported                     # (V, beam_width, L_max, n_layers, H, E, one_hot)
    assert _lib.CTC_PREFIX_LM_MAX_W == 16
    for nl in (1, 2, 3, 4):                                    # at least every V <= 64, W <= 16, L_max <= 512 with any model the beam's LM step takes
        for H, E in ((4, 4), (12, 8), (256, 128), (1024, 512)):
            assert sup(64, 16, 512, nl, H, E, 0) == 1 and sup(1, 1, 1, nl, H, E, 0) == 1
    assert sup(64, 16, 512, 1, 256, 64, 1) == 1 and sup(41, 10, 150, 1, 256, 44, 1) == 1
    assert sup(_lib.CTC_PREFIX_MAX_V, 16, _lib.CTC_PREFIX_MAX_L, 4, 256, 128, 0) == 1
    assert sup(41, 17, 150, 1, 256, 128, 0) == 0 and sup(_lib.CTC_PREFIX_MAX_V + 1, 10, 150, 1, 256, 128, 0) == 0
    assert sup(41, 10, _lib.CTC_PREFIX_MAX_L + 1, 1, 256, 128, 0) == 0
    assert sup(41, 10, 150, 5, 256, 128, 0) == 0 and sup(41, 10, 150, 1, 10, 128, 0) == 0 and sup(41, 10, 150, 1, 256, 6, 0) == 0
    assert sup(41, 10, 150, 1, 256, 40, 1) == 0                # one-hot rows narrower than the vocabulary
    assert sup(0, 10, 150, 1, 256, 128, 0) == 0 and sup(41, 0, 150, 1, 256, 128, 0) == 0 and sup(41, 10, 150, 0, 256, 128, 0) == 0
    wsb = lib.avsr_ctc_prefix_lm_ws_bytes
    assert wsb(64, 10, 1, 256) == 4 * 64 * 2 * 20 * 256 and wsb(3, 16, 4, 12) == 4 * 3 * 2 * 32 * 4 * 12
    assert wsb(0, 10, 1, 256) == 0 and wsb(64, 0, 1, 256) == 0
    p = 64                                          # any non-NULL address: the checks return before a launch could read it

    def args(**over):
        a = _lib.CtcPrefixArgs()
        a.B, a.T, a.V, a.beam_width, a.L_max, a.ld = 3, 50, 31, 10, 150, 32
        a.z = a.in_len = a.ids = a.lens = a.score = p
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def lm(**over):
        m = _lib.CtcPrefixLm()
        m.n_layers, m.H, m.E, m.V, m.one_hot, m.go_id, m.eos_id, m.weight, m.bonus = 1, 12, 8, 31, 0, 30, 29, 0.3, 0.0
        m.embedding = m.wout_t = m.bout = m.ws = m.s_lm = m.lm_steps = p
        m.ws_bytes = wsb(3, 10, 1, 12)
        for j in range(_lib.MAX_LM_LAYERS):
            m.wt[j] = m.bias[j] = p
        for k, v in over.items():
            setattr(m, k, v)
        return m

    run = lambda a, m: lib.avsr_ctc_prefix_search_lm(None if a is None else C.byref(a), None if m is None else C.byref(m), None)
    assert run(None, lm()) == -1 and run(args(), None) == -1
    for n in ("z", "in_len", "ids", "lens", "score"):
        assert run(args(**{n: None}), lm()) == -1, n
    for n in ("embedding", "wout_t", "bout", "ws", "s_lm", "lm_steps"):
        assert run(args(), lm(**{n: None})) == -1, n
    assert run(args(B=0), lm()) == -1 and run(args(T=0), lm()) == -1 and run(args(ld=31), lm()) == -1
    assert run(args(trace_parent=p), lm()) == -1                                    # all four or none
    assert run(args(), lm(V=15)) == -1 and run(args(), lm(go_id=31)) == -1 and run(args(), lm(eos_id=-1)) == -1
    assert run(args(), lm(weight=-0.1)) == -1 and run(args(), lm(weight=float("inf"))) == -1 and run(args(), lm(weight=float("nan"))) == -1
    assert run(args(), lm(bonus=float("nan"))) == -1 and run(args(), lm(bonus=float("-inf"))) == -1
    assert run(args(), lm(ws_bytes=wsb(3, 10, 1, 12) - 4)) == -1                    # a workspace that is too small
    assert run(args(), lm(n_layers=0)) == -1 and run(args(), lm(one_hot=1)) == -1    # (E = 8 < V)
    assert run(args(beam_width=17), lm(ws_bytes=1 << 30)) == -3 and run(args(L_max=513), lm()) == -3
    assert run(args(), lm(n_layers=5)) == -3 and run(args(), lm(H=10)) == -3 and run(args(), lm(E=6)) == -3
    assert run(args(beam_width=17, z=None), lm()) == -1                             # an argument error comes first


def test_avsr_refuses_what_the_fused_search_does_not_cover(tmp_path):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    uf = _unit_file(tmp_path)
    ck = _lm_checkpoint(tmp_path, uf, units_per_layer=(12,), embedding_size=8)
    kw = dict(unit="character", unit_file=uf, use_ctc=True, decoding_algorithm="ctc_prefix_beam_search", ctc_lm_checkpoint=ck,
              lm_units_per_layer=(12,), lm_embedding_size=8)
    for algo in ("greedy", "beam_search", "attention_rescoring"):
        with pytest.raises(ValueError, match="ctc_prefix_beam_search"):
            avsr.AVSR(**dict(kw, decoding_algorithm=algo))
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ctc_lm_weight"):
            avsr.AVSR(ctc_lm_weight=bad, **kw)
    for bad in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="ctc_lm_length_bonus"):
            avsr.AVSR(ctc_lm_length_bonus=bad, **kw)
    with pytest.raises(NotImplementedError, match="LSTM"):
        avsr.AVSR(lm_cell_type="gru", **kw)
    with pytest.raises(ValueError, match="symbols"):
        avsr.AVSR(**dict(kw, unit_file=_unit_file(tmp_path, "abcdefghijklm")))
    with pytest.raises(ValueError, match="shape"):
        avsr.AVSR(**dict(kw, lm_units_per_layer=(16,)))
    with pytest.raises(ValueError, match="missing"):
        avsr.AVSR(**dict(kw, lm_units_per_layer=(12, 12)))
    with pytest.raises(ValueError, match="16"):                                    # the limit of avsr_ctc_prefix_lm_supported, named
        avsr.AVSR(beam_width=17, **kw)
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(**dict(kw, use_ctc=False))
    # the pinned refusals of lm_checkpoint stay as they were
    base = dict(unit="character", unit_file=uf, use_ctc=True, lm_checkpoint=ck, lm_units_per_layer=(12,), lm_embedding_size=8)
    for algo in ("ctc_prefix_beam_search", "attention_rescoring", "greedy"):
        with pytest.raises(ValueError, match="beam_search"):
            avsr.AVSR(decoding_algorithm=algo, **base)

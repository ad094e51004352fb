"""CTC prefix beam search, the parts that need no GPU: the dictionary search of tests/ref_ctc_prefix.py against brute force over all
alignments and against the CTC loss, its edge rules, the input the GPU test uses for a prefix that leaves the beam and returns, and what
is refused on the host (AVSR's constructor, the C entry points)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ref_ctc as RC
import ref_ctc_prefix as R

REENTRY = dict(V=3, T=12, W=3, L_max=8, s=1.0, seed=8)        # found by searching seeds 0..199 with R.reentered


@pytest.mark.parametrize("V,T", [(2, 1), (2, 4), (2, 6), (3, 3), (3, 5)])
def test_unpruned_search_equals_brute_force_over_all_alignments(V, T):
    z = R.kernel_inputs(V, T, 2.0, 100 * V + T)
    want = R.brute_force(R.log_softmax(z))
    out = R.search(z, T, W=len(want), L_max=T)
    got = dict(out["beam"])
    assert set(got) == set(want) and len(out["beam"]) == len(want)
    for g, p in got.items():
        assert np.isclose(p, want[g], rtol=1e-12, atol=1e-12), (g, p, want[g])
    best = max(want, key=lambda g: want[g])
    assert out["beam"][0][0] == best
    ps = [p for _g, p in out["beam"]]
    assert ps == sorted(ps, reverse=True)
    assert np.isclose(np.logaddexp.reduce(ps), 0.0, atol=1e-12)                     # the labellings partition the alignments


def test_final_score_is_minus_the_ctc_loss_of_that_labelling():
    V, T = 3, 6
    z = R.kernel_inputs(V, T, 2.0, 5)
    out = R.search(z, T, W=4 ** 6, L_max=T)
    beam = out["beam"][:12] + out["beam"][-3:]
    L = max(len(g) for g, _p in beam) + 1
    labels, labels_len = np.zeros((len(beam), L), np.int64), np.zeros(len(beam), np.int64)
    for i, (g, _p) in enumerate(beam):
        labels[i, :len(g)] = g
        labels_len[i] = len(g) + 1                                               # ref_ctc's rows carry an EOS slot that is not a target
    zt = torch.tensor(np.repeat(z[None].astype(np.float64), len(beam), 0))
    nll, _U, _Tb = RC.ctc_nll(zt, labels, labels_len, np.full(len(beam), T), V)
    for (g, p), n in zip(beam, nll.numpy()):
        assert np.isclose(p, -n, rtol=1e-10, atol=1e-10), (g, p, n)


def test_L_max_stops_extensions_and_no_frames_give_the_empty_sequence():
    V, T = 3, 6
    z = R.kernel_inputs(V, T, 2.0, 7)
    for L_max in (1, 2):
        out = R.search(z, T, W=100, L_max=L_max)
        assert max(len(g) for g, _p in out["beam"]) == L_max
        want = R.brute_force(R.log_softmax(z))
        for g, p in out["beam"]:                                                  # what is kept is still exact: no mass is moved
            assert np.isclose(p, want[g], rtol=1e-12, atol=1e-12)
    for Tb in (0, -3):
        out = R.search(z, Tb, W=4, L_max=5)
        assert out["beam"] == [((), 0.0)] and out["margin"] == np.inf
    assert R.search(z, 99, W=4, L_max=5)["beam"] == R.search(z, T, W=4, L_max=5)["beam"]      # T_b is clamped to T


def test_beam_is_narrower_than_W_when_fewer_sequences_exist_and_never_nan():
    z = R.kernel_inputs(2, 1, 2.0, 3)
    out = R.search(z, 1, W=10, L_max=4)
    assert [g for g, _p in out["beam"]] in ([(), (0,), (1,)], [(), (1,), (0,)], [(0,), (), (1,)], [(0,), (1,), ()], [(1,), (), (0,)], [(1,), (0,), ()])
    z = R.kernel_inputs(3, 6, 30.0, 1)                                            # peaked rows: most alignments underflow in the exp
    for dt in (np.float64, np.float32):
        out = R.search(z, 6, W=8, L_max=6, dt=dt)
        assert all(np.isfinite(p) for _g, p in out["beam"])


def test_ties_go_to_the_lower_candidate_index():
    z = np.zeros((2, 4), np.float32)                                              # every class equally likely in every frame
    out = R.search(z, 2, W=3, L_max=4)
    # frame 0: the stay of the empty prefix has index V = 3, its extensions 0, 1, 2 -- all tie, the extensions win
    assert out["beams"][1] == [((c,), -np.inf, -np.log(4.0)) for c in range(3)]
    # frame 1: the stays (blank or repeat: 2/16) beat every extension (1/16) and tie among themselves: slot order
    assert [g for g, _p in out["beam"]] == [(0,), (1,), (2,)]


def test_the_reentry_input_holds_a_prefix_that_leaves_the_beam_and_returns():
    c = REENTRY
    z = R.kernel_inputs(c["V"], c["T"], c["s"], c["seed"])
    out = R.search(z, c["T"], c["W"], c["L_max"])
    hits = R.reentered(out["beams"])
    assert hits and hits[0][0] < c["T"], hits                                     # ... with a frame left in which its extension merges
    assert out["margin"] > 10 * R.TOL_SEARCH                                      # the GPU test may compare the whole search on it
    labs = [g for g, _p in out["beam"]]
    assert len(set(labs)) == len(labs)
    for beam in out["beams"]:
        assert len({g for g, _a, _b in beam}) == len(beam)


def test_trace_checker_accepts_the_reference_and_rejects_what_it_must():
    V, T, W, L = 5, 10, 4, 6
    z = R.kernel_inputs(V, T, 2.0, 2)
    out = R.search(z, T, W, L)
    par, sym = np.full((T, W), -1, np.int32), np.full((T, W), -1, np.int32)
    pb, pnb = np.full((T, W), -np.inf, np.float32), np.full((T, W), -np.inf, np.float32)
    y = R.log_softmax(z)
    for t in range(T):
        cands = R.frame(out["beams"][t], y[t], L)
        for r, (g, a, b) in enumerate(out["beams"][t + 1]):
            par[t, r], sym[t, r], pb[t, r], pnb[t, r] = cands[g][2] // (V + 1), cands[g][2] % (V + 1), a, b
    final = R.check_trace(z, T, W, L, par, sym, pb, pnb)
    assert [g for g, _a, _b in final] == [g for g, _p in out["beam"]]
    bad = pb.copy()
    bad[3, 1] += 0.01
    with pytest.raises(AssertionError):
        R.check_trace(z, T, W, L, par, sym, bad, pnb)
    worse = par.copy()
    worse[4, 0], worse[4, 1] = par[4, 1], par[4, 0]
    with pytest.raises(AssertionError):
        R.check_trace(z, T, W, L, worse, sym, pb, pnb)
    short = (par.copy(), sym.copy(), pb.copy(), pnb.copy())                        # a kept entry dropped: a finite candidate is left out
    short[0][5, W - 1] = short[1][5, W - 1] = -1
    short[2][5, W - 1] = short[3][5, W - 1] = -np.inf
    with pytest.raises(AssertionError):
        R.check_trace(z, T, W, L, *short)


def _unit_file(tmp_path, symbols="' abcdefghijklmnopqrstuvwxyz"):
    f = os.path.join(str(tmp_path), "units_%d" % len(symbols))
    open(f, "w").write("\n".join(list(symbols)) + "\n")
    return f


def test_avsr_refuses_what_the_prefix_search_does_not_cover(tmp_path):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    kw = dict(unit="character", unit_file=_unit_file(tmp_path), decoding_algorithm="ctc_prefix_beam_search")
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(**kw)
    with pytest.raises(ValueError, match="64"):
        avsr.AVSR(use_ctc=True, beam_width=65, **kw)
    with pytest.raises(ValueError, match="64"):
        avsr.AVSR(use_ctc=True, beam_width=0, **kw)
    big = "".join(chr(0x100 + i) for i in range(300))
    with pytest.raises(ValueError, match="256"):
        avsr.AVSR(use_ctc=True, **dict(kw, unit_file=_unit_file(tmp_path, big)))
    with pytest.raises(NotImplementedError, match="write_attention_alignment"):
        avsr.AVSR(use_ctc=True, write_attention_alignment=True, **kw)
    with pytest.raises(ValueError, match="beam_search"):                          # the two beam-search options stay where they were
        avsr.AVSR(use_ctc=True, ctc_decode_weight=0.3, **kw)
    with pytest.raises(ValueError, match="beam_search"):
        avsr.AVSR(use_ctc=True, lm_checkpoint="nowhere", **kw)
    with pytest.raises(Exception, match="ctc_prefix_beam_search"):
        avsr.AVSR(**dict(kw, decoding_algorithm="viterbi"))


def test_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    sup = lib.avsr_ctc_prefix_search_supported
    assert sup(41, 10, 150) == 1 and sup(1, 1, 1) == 1
    assert sup(_lib.CTC_PREFIX_MAX_V, _lib.CTC_PREFIX_MAX_W, _lib.CTC_PREFIX_MAX_L) == 1
    assert sup(_lib.CTC_PREFIX_MAX_V + 1, 10, 150) == 0 and sup(41, _lib.CTC_PREFIX_MAX_W + 1, 150) == 0
    assert sup(41, 10, _lib.CTC_PREFIX_MAX_L + 1) == 0
    assert sup(0, 10, 150) == 0 and sup(41, 0, 150) == 0 and sup(41, 10, 0) == 0
    assert (_lib.CTC_PREFIX_MAX_V, _lib.CTC_PREFIX_MAX_W, _lib.CTC_PREFIX_MAX_L) == (256, 64, 512)
    p = 64                                          # any non-NULL address: the checks return before a launch could read it

    def args(**over):
        a = _lib.CtcPrefixArgs()
        a.B, a.T, a.V, a.beam_width, a.L_max, a.ld = 3, 50, 31, 10, 150, 32
        a.z = a.in_len = a.ids = a.lens = a.score = p
        for k, v in over.items():
            setattr(a, k, v)
        return a

    run = lambda a: lib.avsr_ctc_prefix_search(None if a is None else C.byref(a), None)
    assert run(None) == -1
    for n in ("z", "in_len", "ids", "lens", "score"):
        assert run(args(**{n: None})) == -1, n
    assert run(args(B=0)) == -1 and run(args(T=0)) == -1 and run(args(ld=31)) == -1
    assert run(args(V=0, ld=1)) == -1 and run(args(beam_width=0)) == -1 and run(args(L_max=0)) == -1
    assert run(args(trace_parent=p)) == -1 and run(args(trace_parent=p, trace_sym=p, trace_pb=p)) == -1       # all four or none
    assert run(args(V=257, ld=258)) == -3 and run(args(beam_width=65)) == -3 and run(args(L_max=513)) == -3
    assert run(args(V=257, ld=258, z=None)) == -1                                  # an argument error comes first

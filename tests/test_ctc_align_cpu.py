"""CTC forced alignment, the parts that need no GPU: the fp64 Viterbi reference of tests/ref_ctc_align.py against brute force over all
frame labellings and against the CTC loss, its edge rules, what its checker must reject, how many of the GPU test's seeds fall below
the comparison margin, and what is refused on the host (the C entry points, Seq2SeqModel.ctc_align, AVSR.align)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import ref_ctc as RC
import ref_ctc_align as R


@pytest.mark.parametrize("T", [1, 2, 4, 6])
def test_reference_equals_brute_force_over_all_frame_labellings(T):
    V = 3
    z = R.logits(V, T, 10 + T, 2.0)
    y = R.log_softmax(z)
    for U in range(0, 4):
        for g in itertools.product(range(V), repeat=U):                    # every target, repeated labels included
            want, arg = R.brute_force(y, g)
            out = R.align(z, g, T, want_margin=True)
            assert out["status"] == int(arg is not None) == int(R.feasible(g, T, V)), (g, T)
            if arg is None:
                assert out["score"] == 0.0 and out["path"] == []
                continue
            assert np.isclose(out["score"], want, rtol=1e-12, atol=1e-12), (g, out["score"], want)
            assert out["path"] == arg and out["margin"] > 0, (g, out["path"], arg)
            assert np.isclose(R.path_score(z, out["path"]), want, rtol=1e-12, atol=1e-12)


def test_best_alignment_is_no_more_probable_than_all_of_them():
    V, T = 3, 6
    z = R.logits(V, T, 5, 2.0)
    gs = [g for U in range(0, 4) for g in itertools.product(range(V), repeat=U) if R.feasible(g, T, V)]
    L = 4
    labels, labels_len = np.zeros((len(gs), L), np.int64), np.zeros(len(gs), np.int64)
    for i, g in enumerate(gs):
        labels[i, :len(g)] = g
        labels_len[i] = len(g) + 1                                        # ref_ctc's rows carry an EOS slot that is not a target
    zt = torch.tensor(np.repeat(z[None].astype(np.float64), len(gs), 0))
    nll, _U, _Tb = RC.ctc_nll(zt, labels, labels_len, np.full(len(gs), T), V)
    for g, n in zip(gs, nll.numpy()):
        s = R.align(z, g, T)["score"]
        assert s <= -n + 1e-12, (g, s, n)
        assert s >= -n - T * np.log(V + 1.0)                              # ... and no less than its share among at most (V + 1)^T


def test_edge_rules():
    V, T = 4, 9
    z = R.logits(V, T, 3)
    y = R.log_softmax(z)
    out = R.align(z, [], T)                                               # U = 0: blanks only
    assert out["status"] == 1 and out["path"] == [V] * T and out["start"] == [] and np.isclose(out["score"], y[:, V].sum())
    out = R.align(z, [], 0)                                               # no frames: nothing to align, not even the empty target
    assert out["status"] == 0 and out["score"] == 0.0
    assert R.align(z, [2], 1)["path"] in ([2],) and R.align(z, [], 1)["path"] == [V]          # T_b = 1
    assert R.align(z, [1, 2], 1)["status"] == 0
    g = [1, 1, 2, 2, 2, 0]                                                # T_b exactly U + repeats: one alignment only
    assert R.repeats(g) == 3
    out = R.align(z, g, 9, want_margin=True)
    assert out["path"] == [1, V, 1, 2, V, 2, V, 2, 0] and out["margin"] == np.inf
    assert out["start"] == out["end"] == [0, 2, 3, 5, 7, 8]
    assert R.align(z, g, 8)["status"] == 0                                # one frame short
    assert R.align(z, [1, V], T)["status"] == 0 and R.align(z, [-1], T)["status"] == 0        # a label out of range (the blank included)
    assert R.align(z, g, 99)["path"] == out["path"]                       # T_b is clamped to T
    for dt in (np.float64, np.float32):                                   # peaked rows: nothing turns NaN
        o = R.align(R.logits(V, T, 1, 40.0), [0, 3], T, dt)
        assert np.isfinite(o["score"]) and np.isfinite(o["frame_lp"]).all()


def test_ties_go_to_the_higher_state():
    V, T = 3, 5
    z = np.zeros((T, V + 1), np.float32)                                  # every alignment is equally probable
    out = R.align(z, [0, 1], T, want_margin=True)
    # the last blank wins the end; going back, staying wins over s - 1 wins over s - 2: the labels come as early and as short as possible
    assert out["states"] == [1, 3, 4, 4, 4] and out["path"] == [0, 1, V, V, V]
    assert abs(out["margin"]) < 1e-12                                     # (forward + backward sums the same terms in another order)
    assert R.align(z, [2, 2], T)["states"] == [1, 2, 3, 4, 4]


def _as_kernel_output(ref, T, L, V):
    U = len(ref["start"])
    Tb = len(ref["path"])
    got = dict(status=ref["status"], score=np.float32(ref["score"]), path=np.full(T, -1, np.int32), frame_lp=np.zeros(T, np.float32),
               start=np.full(L, -1, np.int32), end=np.full(L, -1, np.int32))
    got["path"][:Tb], got["frame_lp"][:Tb] = ref["path"], ref["frame_lp"]
    got["start"][:U], got["end"][:U] = ref["start"], ref["end"]
    return got


def test_checker_accepts_the_reference_and_rejects_what_it_must():
    V, T, L = 5, 14, 6
    z, g = R.logits(V, T, 2), [1, 3, 3, 0]
    ref = R.align(z, g, 12, want_margin=True)
    assert ref["margin"] > 10 * R.TOL_ALIGN
    good = _as_kernel_output(ref, T, L, V)
    assert R.check(z, g, 12, good, R.TOL_ALIGN)[1]

    def broken(**over):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for k, f in over.items():
            bad[k] = f(bad[k])
        return bad

    def shifted(p):                                                       # the same labelling one frame later: valid, not optimal
        q = p.copy()
        q[1:12] = p[:11]
        q[0] = V
        return q
    sh = shifted(good["path"])
    assert R.collapse(sh[:12], V) == g                                    # (the reference's last frame is a blank: the shift stays valid)
    y = R.log_softmax(z[:12])
    fix = broken(path=lambda p: sh, frame_lp=lambda l: np.concatenate((y[np.arange(12), sh[:12]], [0, 0])).astype(np.float32))
    rr = R.runs(sh[:12], V)
    fix["start"][:4], fix["end"][:4] = [r[1] for r in rr], [r[2] for r in rr]
    with pytest.raises(AssertionError, match="not optimal"):              # a valid, self-consistent alignment that is not the best
        R.check(z, g, 12, fix, R.TOL_ALIGN)
    with pytest.raises(AssertionError):                                   # a shifted path with everything else left as it was
        R.check(z, g, 12, broken(path=shifted), R.TOL_ALIGN)
    with pytest.raises(AssertionError, match="start|end"):                # a wrong run
        R.check(z, g, 12, broken(end=lambda e: np.concatenate((e[:1] + 1, e[1:]))), R.TOL_ALIGN)
    with pytest.raises(AssertionError, match="collapse"):
        R.check(z, g, 12, broken(path=lambda p: np.concatenate(([V] * 12, p[12:])).astype(np.int32)), R.TOL_ALIGN)
    with pytest.raises(AssertionError, match="score"):
        R.check(z, g, 12, broken(score=lambda s: s + np.float32(0.01)), R.TOL_ALIGN)
    with pytest.raises(AssertionError, match="padding"):
        R.check(z, g, 12, broken(frame_lp=lambda l: l + np.float32(1e-3) * (np.arange(T) >= 12)), R.TOL_ALIGN)
    with pytest.raises(AssertionError):                                   # an infeasible target reported as aligned
        R.check(z, g + [V], 12, good, R.TOL_ALIGN)


@pytest.mark.parametrize("cfg", R.SEED_CONFIGS, ids=lambda c: "V%d_T%d_U%d" % c)
def test_few_seeds_fall_below_the_comparison_margin(cfg):
    """A condition on the GPU test's inputs, met by the reference alone: at most one eighth of a configuration's 64 seeds may have a
    margin that does not exceed the tolerance (their paths are then not compared; everything else still is)."""
    V, T, U = cfg
    low = sum(not R.align(R.logits(V, T, s), R.labels(V, U, s), T, want_margin=True)["margin"] > R.tol_for(T) for s in range(64))
    print(cfg, "below the margin:", low, "of 64")
    assert low <= 64 // 8


def test_every_kernel_case_is_feasible_and_within_the_limits():
    for case in R.KERNEL_CASES:
        V, T, L, U, _Tb, _kind = case
        z, g, Tb = R.case_inputs(case)
        assert len(g) == U <= L <= R.MAX_L and 1 <= Tb <= T and R.feasible(g, Tb, V), case


def test_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    sup = lib.avsr_ctc_align_supported
    assert sup(41, 150) == 1 and sup(1, 1) == 1 and sup(100000, _lib.CTC_ALIGN_MAX_L) == 1
    assert sup(41, _lib.CTC_ALIGN_MAX_L + 1) == 0 and sup(0, 10) == 0 and sup(41, 0) == 0
    assert _lib.CTC_ALIGN_MAX_L == 512 == _lib.CTC_PREFIX_MAX_L
    assert lib.avsr_sizeof(b"avsr_ctc_align_args") == C.sizeof(_lib.CtcAlignArgs)
    nbytes = lib.avsr_ctc_align_ws_bytes
    assert nbytes(0, 50, 10) == 0 and nbytes(3, 0, 10) == 0 and nbytes(3, 50, 0) == 0
    assert nbytes(3, 50, 10) > 0 and nbytes(3, 50, 10) % 8 == 0 and nbytes(6, 50, 10) == 2 * nbytes(3, 50, 10)
    assert nbytes(64, 1000000, 512) > 2 ** 32                            # 64-bit: T is not bounded
    p = 64                                          # any non-NULL address: the checks return before a launch could read it
    ptrs = ("z", "labels", "target_len", "in_len", "score", "status", "path", "frame_lp", "start", "end", "ws")

    def args(**over):
        a = _lib.CtcAlignArgs()
        a.B, a.T, a.L, a.V, a.ld = 3, 50, 10, 31, 32
        for n in ptrs:
            setattr(a, n, p)
        a.ws_bytes = nbytes(3, 50, over.get("L", 10))
        for k, v in over.items():
            setattr(a, k, v)
        return a

    run = lambda a: lib.avsr_ctc_align(None if a is None else C.byref(a), None)
    assert run(None) == -1
    for n in ptrs:
        assert run(args(**{n: None})) == -1, n
    assert run(args(B=0)) == -1 and run(args(T=0)) == -1 and run(args(L=0)) == -1 and run(args(V=0, ld=1)) == -1
    assert run(args(B=-1)) == -1 and run(args(T=-5)) == -1 and run(args(ld=31)) == -1
    assert run(args(ws_bytes=nbytes(3, 50, 10) - 1)) == -1 and run(args(ws_bytes=0)) == -1
    assert run(args(ws=68)) == -1                                         # the scratch holds 64-bit words
    assert run(args(L=513)) == -3
    assert run(args(L=513, z=None)) == -1                                 # an argument error comes first


class _Stub:
    pass


def test_model_and_front_door_refusals_that_need_no_engine():
    from avsr_tf1_amd import avsr as A
    from avsr_tf1_amd.config import ModelConfig
    from avsr_tf1_amd.model import Seq2SeqModel
    batch = _Stub()
    batch.audio, batch.video, batch.labels = torch.zeros(2, 5, 3), None, torch.zeros(2, 4, dtype=torch.int32)
    m = object.__new__(Seq2SeqModel)
    m.cfg = ModelConfig()
    with pytest.raises(ValueError, match="use_ctc"):
        Seq2SeqModel._ctc_align(m, batch, None)
    m.cfg = ModelConfig(architecture="lm", video_units=None, audio_units=None)
    with pytest.raises(ValueError, match="lm"):
        Seq2SeqModel._ctc_align(m, batch, None)
    m.cfg = ModelConfig(use_ctc=True)
    with pytest.raises(ValueError, match="one id list per utterance"):
        Seq2SeqModel._ctc_align(m, batch, [[1, 2]])
    with pytest.raises(ValueError, match="512"):
        Seq2SeqModel._ctc_align(m, batch, [[1] * 513, [2]])
    e = object.__new__(A.AVSR)
    e._cfg = ModelConfig()
    with pytest.raises(ValueError, match="use_ctc"):
        A.AVSR.align(e, "nowhere/checkpoint.ckp-1")
    e._cfg = ModelConfig(use_ctc=True)
    with pytest.raises(ValueError, match="targets"):
        A.AVSR.align(e, "nowhere/checkpoint.ckp-1", targets="greedy")
    with pytest.raises(ValueError, match="frame_shift"):
        A.AVSR.align(e, "nowhere/checkpoint.ckp-1", frame_shift=0.0)

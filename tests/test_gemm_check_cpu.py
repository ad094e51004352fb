"""The GEMM checker of tests/ref_gemm.py has teeth: "kernel results" computed in numpy that are wrong in ONE specific way are rejected,
the honest fp32 result is accepted.  CPU only.  Also verified here: the 2^24 condition of the exact family (asserted by the builder on
its own inputs) and the K cap of the gauss family (reduced-precision operands are still rejected at GAUSS_KMAX)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_gemm as R  # noqa: E402
from ref_gemm import Case, Layout  # noqa: E402


def round_sig(x, bits):
    """fp32 values rounded (nearest even) to `bits` significant bits: 8 = bf16, 11 = an fp16-like significand."""
    drop = 24 - bits
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + ((1 << (drop - 1)) - 1) + ((u >> drop) & 1)) >> drop << drop
    return u.astype(np.uint32).view(np.float32)


def simulate(p, fault=None, k=None, row=0, bits=None):
    """The buffers a kernel would leave for problem p: operands gathered from the poisoned buffers through the layout, fp32
    accumulation in k order, the fp32 epilogue.  `fault` makes it wrong in one way."""
    c = p.case
    ia = p.idx["A"].copy()
    if fault == "neighbour_group":                  # one row of the two-level A view taken from the next group
        assert c.ta == 0 and c.A.T and row + c.A.T < c.M
        ia[:, row, :] += p.mats["A"]["ldo"]
    A, B = p.a[ia], p.b[p.idx["B"]]
    A = A.transpose(0, 2, 1) if c.ta else A
    B = B.transpose(0, 2, 1) if c.tb else B
    if fault == "round":
        A, B = round_sig(A, bits), round_sig(B, bits)
    acc = np.zeros((c.batch, c.M, c.N), np.float32)
    for kk in range(c.K):
        term = A[:, :, kk, None] * B[:, kk, None, :]
        if kk == k and fault == "drop":
            term[:, row] = 0
        if kk == k and fault == "dup":
            term[:, row] *= 2
        acc = acc + term
    v = np.float32(p.alpha_eff) * acc
    if c.beta != 0:
        v = v + np.float32(c.beta) * p.c[p.idx["C"]]
    if c.bias:
        v = v + p.bias[c.bias_offset:c.bias_offset + c.N]
    out = p.c.copy()
    out[p.idx["C"]] = v
    if fault == "col_past_n":
        out[p.idx["C"][0, row, c.N - 1] + 1] = 1.0
    cs = None
    if c.colsum:
        s = np.zeros(c.N, np.float32)
        for kk in range(c.K):
            if not (fault == "cs_missing_row" and kk == k):
                s = s + B[0, kk]
        if c.colsum_beta != 0:
            s = s + np.float32(c.colsum_beta) * p.cs[R.CS_OFFSET:R.CS_OFFSET + c.N]
        cs = p.cs.copy()
        cs[R.CS_OFFSET:R.CS_OFFSET + c.N] = s
    return out, cs


SLOT = dict(T=5, gap=2)
BASE = [
    Case(40, 36, 49, A=Layout(pad=3, offset=52, **SLOT), C=Layout(pad=3), colsum=True, colsum_beta=1.0, alpha=0.5, beta=2.0, bias=True),
    Case(33, 17, 100, ta=1, tb=0, A=Layout(pad=1), B=Layout(pad=2, offset=1), C=Layout(pad=1, T=3, gap=1, offset=18), colsum=True, splitk=3),
    Case(70, 20, 32, tb=1, A=Layout(pad=4, T=16, gap=2), C=Layout(pad=4), batch=2, beta=1.0, alpha_dev=0.25, alpha=2.0),
]
EXACT = BASE
GAUSS = [c.replace(family="gauss", alpha=0.5 if c.alpha == 0.5 else 1.0, alpha_dev=None if c.alpha_dev is None else 0.75) for c in BASE]
MANT = [Case(40, 36, 8, family=f, ta=ta, tb=tb, A=Layout(pad=3, T=5, gap=2) if not ta else Layout(pad=1), C=Layout(pad=3),
             colsum=(tb == 0), beta=1.0, bias=True) for f in ("mant_a", "mant_b") for ta, tb in ((0, 0), (1, 1))]
ids = lambda c: "%s-%dx%dx%d-%d%d" % (c.family, c.M, c.N, c.K, c.ta, c.tb)       # noqa: E731


@pytest.fixture(scope="module")
def problems():
    return {c: R.build(c) for c in EXACT + GAUSS + MANT}


def rejected(p, **fault):
    with pytest.raises(R.GemmMismatch):
        R.check(p, *simulate(p, **fault))


@pytest.mark.parametrize("case", EXACT + GAUSS + MANT, ids=ids)
def test_honest_fp32_result_is_accepted(problems, case):
    p = problems[case]
    ratio = R.check(p, *simulate(p))
    assert ratio == 0.0 if case.family != "gauss" else 0.0 < ratio <= 1.0


@pytest.mark.parametrize("case", EXACT + GAUSS, ids=ids)
def test_dropped_k_term_at_a_tile_edge_is_rejected(problems, case):
    for k in (15, 16, case.K - 1):
        rejected(problems[case], fault="drop", k=k, row=case.M - 1)


@pytest.mark.parametrize("case", EXACT + GAUSS, ids=ids)
def test_k_term_counted_twice_is_rejected(problems, case):
    for k in (15, 16, case.K - 1):
        rejected(problems[case], fault="dup", k=k, row=1)


@pytest.mark.parametrize("case", [c for c in EXACT + GAUSS + MANT if c.ta == 0 and c.A.T], ids=ids)
def test_row_from_the_neighbouring_group_is_rejected(problems, case):
    rejected(problems[case], fault="neighbour_group", row=2)


@pytest.mark.parametrize("case", EXACT + GAUSS, ids=ids)
def test_column_past_n_written_is_rejected(problems, case):
    with pytest.raises(R.GemmMismatch, match="outside the operation's output"):
        R.check(problems[case], *simulate(problems[case], fault="col_past_n", row=case.M // 2))


@pytest.mark.parametrize("case", [c for c in EXACT + GAUSS + MANT if c.colsum], ids=ids)
def test_column_sum_missing_one_row_is_rejected(problems, case):
    for k in (0, case.K - 1):
        with pytest.raises(R.GemmMismatch, match="colsum"):
            R.check(problems[case], *simulate(problems[case], fault="cs_missing_row", k=k))


@pytest.mark.parametrize("bits", [8, 11])
@pytest.mark.parametrize("case", MANT + GAUSS, ids=ids)
def test_reduced_precision_operands_are_rejected(problems, case, bits):
    rejected(problems[case], fault="round", bits=bits)


@pytest.mark.parametrize("bits", [8, 11])
@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 1)])
def test_reduced_precision_is_rejected_at_the_gauss_k_cap(ta, tb, bits):
    """The bound grows as K^2 and a rounded operand's error as sqrt(K): the cap is where 11 significant bits are still caught."""
    p = R.build(Case(64, 64, R.GAUSS_KMAX, ta=ta, tb=tb, family="gauss", splitk=8))
    assert R.check(p, *simulate(p)) <= 1.0
    rejected(p, fault="round", bits=bits)


def test_builder_refuses_inputs_that_could_round():
    R.build(Case(4, 4, 100000))                                  # 100000 * 49 < 2^24
    with pytest.raises(AssertionError):
        R.build(Case(4, 4, 400000))                              # 400000 * 49 > 2^24
    with pytest.raises(AssertionError):
        R.build(Case(4, 4, 335000, alpha=2.0 ** -8, beta=256.0))   # alpha * acc + beta * C0 needs more than 24 bits
    with pytest.raises(AssertionError):
        R.build(Case(4, 4, 16, alpha=0.3))                       # not a power of two
    with pytest.raises(AssertionError):
        R.build(Case(4, 4, 9, family="mant_a"))
    with pytest.raises(AssertionError):
        R.build(Case(4, 4, R.GAUSS_KMAX + 1, family="gauss"))


def test_poison_and_sentinel_cover_everything_not_owned():
    p = R.build(BASE[0])
    for w, buf in (("A", p.a), ("B", p.b)):
        own = np.zeros(buf.size, bool)
        own[p.idx[w].reshape(-1)] = True
        assert np.isnan(buf[~own]).all() and (~own).any() and not np.isnan(buf[own]).any()
    own = np.zeros(p.c.size, bool)
    own[p.idx["C"].reshape(-1)] = True
    assert (p.c.view(np.uint32)[~own] == R.SENTINEL).all() and (~own).any()
    q = R.build(BASE[1])                                         # beta == 0: the destination is NaN where the kernel writes
    assert np.isnan(q.c[q.idx["C"]]).all() and np.isnan(q.cs[R.CS_OFFSET:R.CS_OFFSET + q.case.N]).all()


def test_layout_class_and_reduction_path():
    assert R.layout_class(Case(8, 8, 8)) == 8 | 2 | 1
    assert R.layout_class(Case(8, 8, 8, ta=1, tb=1)) == 4 | 2 | 1
    assert R.layout_class(Case(8, 8, 7)) == 8 | 1                                   # A's contiguous extent is K
    assert R.layout_class(Case(8, 8, 8, A=Layout(pad=1))) == 8 | 1
    assert R.layout_class(Case(8, 8, 8, B=Layout(offset=1))) == 8 | 2
    assert R.layout_class(Case(8, 8, 8, B=Layout(T=2, ldo_extra=2))) == 8 | 2
    assert R.reduce_is_vector(Case(8, 8, 64, splitk=2)) and not R.reduce_is_vector(Case(8, 7, 64, splitk=2))
    assert not R.reduce_is_vector(Case(8, 8, 64, splitk=2, C=Layout(offset=1)))
    assert not R.reduce_is_vector(Case(8, 8, 64, splitk=2, bias=True, bias_offset=1))
    assert R.effective_splitk(Case(8, 8, 40, splitk=8)) == 3 and R.effective_splitk(Case(8, 8, 0, splitk=4)) == 1

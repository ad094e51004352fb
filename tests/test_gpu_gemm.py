"""Conformance grid of avsr_gemm / avsr_gemm_batch (csrc/gemm.hip) through ops.gemm: every operand-layout class as a single and as a
grouped launch, the edges of the 128x128x16 tile and of the pipelined K loop, the epilogue, two-level rows on all three matrices,
both split-K reductions, batching, the fused column sums, grouped launches and the refusals.

Inputs, reference and checker are tests/ref_gemm.py: operands are poisoned with NaN wherever the operation does not own them, outputs
carry a sentinel wherever it must not write.  The exact families are compared with np.array_equal (no tolerance); the gauss family
against the derived forward bound of an fp32 dot product.  Shapes are the smallest that reach the code in question."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_gemm as R  # noqa: E402
from ref_gemm import Case, Layout  # noqa: E402

pytestmark = pytest.mark.gpu

TT = [(0, 0), (0, 1), (1, 0), (1, 1)]
EPI = dict(alpha=0.5, beta=2.0, bias=True)            # a full epilogue; exact in both families (powers of two)
RATIOS = {}                                           # gauss family: worst err / bound per test


@functools.lru_cache(maxsize=None)
def problem(case):
    return R.build(case)          # built once, shared, never modified (to_device copies)


_ws = None


def workspace():
    global _ws
    if _ws is None:
        _ws = torch.empty(1 << 20, device="cuda")
    return _ws


def run(cases, grouped=False):
    """Issue the cases one by one or inside one ops.gemm_group() block; the buffers they leave as (C, column sums) per case."""
    from avsr_tf1_amd import ops
    ps = [problem(c) for c in cases]
    ts = [R.to_device(p, torch) for p in ps]
    if grouped:
        with ops.gemm_group():
            for p, t in zip(ps, ts):
                R.issue(p, t, ops, workspace())
    else:
        for p, t in zip(ps, ts):
            R.issue(p, t, ops, workspace())
    torch.cuda.synchronize()
    return [R.fetch(t) for t in ts]


def verify(cases, grouped=False, request=None):
    outs = run(cases, grouped)
    worst = 0.0
    for i, (c, o) in enumerate(zip(cases, outs)):
        try:
            worst = max(worst, R.check(problem(c), *o))
        except R.GemmMismatch as e:
            raise R.GemmMismatch("entry %d of %d (%s): %s" % (i, len(cases), c, e)) from None
    if request is not None and any(c.family == "gauss" for c in cases):
        RATIOS[request.node.name] = worst
        print("gauss worst err/bound %s %.4f" % (request.node.name, worst))
    return outs


def same_bits(x, y):
    return all((a is None and b is None) or np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))


def cid(c):
    return "%s-%dx%dx%d-t%d%d-sk%d-b%d-c%d" % (c.family, c.M, c.N, c.K, c.ta, c.tb, c.splitk, c.batch, R.layout_class(c))


def ids(cases):
    return ["%02d-%s" % (i, cid(c)) for i, c in enumerate(cases)]


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    yield
    if RATIOS:
        print("\ngauss family, worst err/bound over %d tests: %.4f (%s)" % (len(RATIOS), max(RATIOS.values()), max(RATIOS, key=RATIOS.get)))


# ---- classes -------------------------------------------------------------------------------------------------------------------------
VEC = dict(pad=4, offset=4)       # a vectorisable view: ld, pointer and extent multiples of four floats


def scalar_layout(way):
    """A view whose loader must be the scalar one for exactly one reason."""
    if way == "ld":
        return Layout(pad=1, offset=4)
    if way == "ptr":
        return Layout(pad=4, offset=1)
    if way == "ldo":
        return Layout(pad=4, offset=4, T=5, gap=1, ldo_extra=2)
    return Layout(pad=3, offset=4)      # "extent": the caller makes the contiguous extent 4n + 1, ld stays a multiple of four


def class_case(ta, tb, va, vb, family="exact", seed=0, wa="ld", wb="ptr"):
    M, N, K = 36, 40, 20
    c = Case(M, N, K, ta=ta, tb=tb, A=Layout(**VEC) if va else scalar_layout(wa), B=Layout(**VEC) if vb else scalar_layout(wb),
             C=Layout(pad=3, offset=2), family=family, seed=seed, **EPI)
    assert R.layout_class(c) == (8 if not ta else 0) | (4 if tb else 0) | (2 if va else 0) | (1 if vb else 0)
    return c


CLASS_GRID = [(class_case(ta, tb, va, vb), grouped) for ta, tb in TT for va in (0, 1) for vb in (0, 1) for grouped in (False, True)]


@pytest.mark.parametrize("case,grouped", CLASS_GRID, ids=["%s-%s" % (cid(c), "group" if g else "single") for c, g in CLASS_GRID])
def test_every_class_single_and_grouped_exact(case, grouped):
    verify([case, case.replace(seed=1)] if grouped else [case], grouped)


def test_class_grid_covers_all_32_combinations():
    assert {(R.layout_class(c), g) for c, g in CLASS_GRID} == {(k, g) for k in range(16) for g in (False, True)}
    assert all(c.family == "exact" for c, _ in CLASS_GRID)


@pytest.mark.parametrize("ta,tb,va,vb", [(ta, tb, va, vb) for ta, tb in TT for va in (0, 1) for vb in (0, 1)])
def test_grouped_is_bit_identical_to_single_gauss(ta, tb, va, vb, request):
    cases = [class_case(ta, tb, va, vb, family="gauss", seed=s, wa="ldo", wb="ld") for s in (0, 1)]
    single = verify(cases, False, request)
    grouped = verify(cases, True)
    assert all(same_bits(s, g) for s, g in zip(single, grouped))


def scalar_way_case(operand, way, t):
    M, N, K = 36, 40, 20
    if operand == "A":
        ta, tb = t, 0 if t == 0 else 1                 # the other operand's contiguous extent is not A's
        if way == "extent":
            M, K = (M, K + 1) if ta == 0 else (M + 1, K)
        c = Case(M, N, K, ta=ta, tb=tb, A=scalar_layout(way), B=Layout(**VEC), **EPI)
        want = (8 if not ta else 0) | (4 if tb else 0) | 1
    else:
        tb, ta = t, 1 if t == 1 else 0
        if way == "extent":
            N, K = (N, K + 1) if tb == 1 else (N + 1, K)
        c = Case(M, N, K, ta=ta, tb=tb, A=Layout(**VEC), B=scalar_layout(way), **EPI)
        want = (8 if not ta else 0) | (4 if tb else 0) | 2
    assert R.layout_class(c) == want, (operand, way, t)
    return c


SCALAR_WAYS = [scalar_way_case(o, w, t) for o in "AB" for w in ("extent", "ld", "ptr", "ldo") for t in (0, 1)]


@pytest.mark.parametrize("case", SCALAR_WAYS, ids=ids(SCALAR_WAYS))
def test_scalar_loader_forced_each_way(case):
    verify([case])


# ---- edges of the tile and of the pipeline ---------------------------------------------------------------------------------------------
KS = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100]
MNS = [(1, 1), (31, 33), (32, 64), (33, 31), (63, 129), (64, 32), (65, 127), (127, 65), (128, 128), (129, 63), (257, 1), (1, 257)]
EDGES = ([Case(MNS[i % 12][0], MNS[i % 12][1], K, ta=TT[i % 4][0], tb=TT[i % 4][1], **EPI) for i, K in enumerate(KS)] +
         [Case(M, N, KS[(5 * i + 3) % 14], ta=TT[(i + 1) % 4][0], tb=TT[(i + 1) % 4][1], **EPI) for i, (M, N) in enumerate(MNS)] +
         [Case(65, 33, K, ta=TT[(i + 2) % 4][0], tb=TT[(i + 2) % 4][1], A=Layout(pad=3), B=Layout(pad=1), C=Layout(pad=2), **EPI)
          for i, K in enumerate(KS)])
EDGES_GAUSS = [c.replace(family="gauss") for c in EDGES[:14]]
# the free-standing shapes of test_gpu_kernels.py::test_gemm_shapes, here with exact inputs
OLD_SHAPES = [Case(M, N, K, ta=ta, tb=tb, **EPI) for M, N, K, ta, tb in
              [(128, 128, 64, 0, 0), (200, 72, 100, 0, 0), (131, 31, 52, 0, 1), (64, 1024, 80, 0, 0), (48, 36, 1000, 1, 0),
               (256, 256, 256, 0, 1), (7, 5, 3, 0, 0), (33, 130, 17, 1, 0)]]


@pytest.mark.parametrize("case", EDGES + OLD_SHAPES, ids=ids(EDGES + OLD_SHAPES))
def test_tile_and_k_edges_exact(case):
    verify([case])


@pytest.mark.parametrize("case", EDGES_GAUSS, ids=ids(EDGES_GAUSS))
def test_k_edges_gauss(case, request):
    verify([case], request=request)


K0 = [Case(33, 20, 0, ta=ta, tb=tb, splitk=sk, **epi) for (ta, tb), sk, epi in
      zip(TT, (1, 4, 1, 2), (EPI, EPI, dict(bias=True), dict(beta=1.0)))] + [Case(5, 130, 0, colsum=True, colsum_beta=1.0, beta=1.0),
                                                                            Case(5, 130, 0, ta=1, colsum=True)]


@pytest.mark.parametrize("case", K0, ids=ids(K0))
def test_k_zero_gives_beta_c_plus_bias(case):
    p = problem(case)
    want = (case.beta * p.C0 if case.beta else 0.0) + (p.bias_v if case.bias else 0.0)
    assert np.array_equal(p.c_exp, np.broadcast_to(want, p.c_exp.shape))
    verify([case])


# ---- epilogue --------------------------------------------------------------------------------------------------------------------------
EPILOGUE = [Case(65, 33, 17, ta=TT[i % 4][0], tb=TT[i % 4][1], beta=beta, bias=bias, alpha=alpha, alpha_dev=ad, C=Layout(pad=i % 3))
            for i, (beta, bias, (alpha, ad)) in enumerate((b, bi, a) for b in (0.0, 2.0) for bi in (False, True)
                                                          for a in ((1.0, None), (2.0, 0.25)))]
TWO_LEVEL_C = [Case(150, 20, 8, tb=i % 2, beta=(0.0, 1.0)[i % 2], bias=True, C=Layout(T=T, gap=2, offset=20 + 4 * (i % 2), pad=4 * (i % 2)))
               for i, T in enumerate((1, 3, 16, 37, 64))]
BIG_M = Case(65536 + 3, 4, 4, beta=1.0, bias=True, C=Layout(T=37, gap=2, offset=4))
MANTISSA = [Case(M, 36, K, ta=ta, tb=tb, family=f, beta=1.0, bias=True, colsum=(tb == 0))
            for f in ("mant_a", "mant_b") for ta, tb in TT for M, K in ((33, 5), (32, 8))]


@pytest.mark.parametrize("case", EPILOGUE + TWO_LEVEL_C + [BIG_M], ids=ids(EPILOGUE + TWO_LEVEL_C + [BIG_M]))
def test_epilogue_exact(case):
    """beta == 0 cases start from a NaN-filled destination (ref_gemm.build): the result must be finite and exact."""
    verify([case])
    if case.beta == 0:
        assert np.isnan(problem(case).c[problem(case).idx["C"]]).all()


@pytest.mark.parametrize("case", MANTISSA, ids=ids(MANTISSA))
def test_full_fp32_significand_of_both_operands(case):
    verify([case])


# ---- two-level operands ----------------------------------------------------------------------------------------------------------------
def two_level_operands():
    out = []
    for i, T in enumerate((1, 3, 5, 16, 37)):
        for t in (0, 1):
            for which in "AB":
                rows_are_k = (which == "A") == (t == 1)       # A stored [K][M] / B stored [K][N]: the k-major loader walks the groups
                cols = {("A", 0): 50, ("A", 1): 45, ("B", 0): 28, ("B", 1): 50}[(which, t)]
                L = Layout(T=T, gap=2, offset=cols + (i % 2), pad=i % 2)      # the [B, T+2, F] slot view, shifted by one row
                kw = dict(ta=t, tb=(i + t) % 2, A=L) if which == "A" else dict(tb=t, ta=(i + t) % 2, B=L)
                for sk in (1, 4 if rows_are_k else 2):        # K = 50 in four slices of 16 / two of 32: slices start mid-group
                    out.append(Case(45, 28, 50, splitk=sk, **kw, **EPI))
    return out


TWO_LEVEL = two_level_operands()


@pytest.mark.parametrize("case", TWO_LEVEL, ids=ids(TWO_LEVEL))
def test_two_level_operands_exact(case):
    verify([case])


# ---- split-K ---------------------------------------------------------------------------------------------------------------------------
def splitk_cases(family="exact"):
    out = []
    variants = [("vec", dict(N=40)), ("n_odd", dict(N=41)), ("c_ptr", dict(N=40, C=Layout(offset=1))),
                ("bias_ptr", dict(N=40, bias_offset=1)), ("ldc_odd", dict(N=40, C=Layout(pad=1))),
                ("vec_two_level", dict(N=40, C=Layout(T=7, gap=1, offset=40))), ("ldoc_odd", dict(N=40, C=Layout(T=7, gap=1, ldo_extra=2)))]
    for i, (sk, K) in enumerate(((2, 100), (3, 100), (8, 100), (100, 100), (16, 200), (64, 200))):      # 2, 3, 7, 7, 13, 13 slices
        for j, (name, kw) in enumerate(variants):
            kw = dict(kw)
            N = kw.pop("N")
            ta, tb = TT[(i + j) % 4]
            c = Case(37, N, K, ta=ta, tb=tb, splitk=sk, alpha=2.0, alpha_dev=0.25, beta=2.0, bias=True, family=family, **kw)
            assert R.reduce_is_vector(c) == name.startswith("vec")
            out.append(c)
    for sk in (2, 3):                                    # with batch > 1, both reductions
        for N in (40, 41):
            out.append(Case(37, N, 100, ta=1, splitk=sk, batch=3, beta=2.0, bias=True, alpha=0.5, family=family,
                            A=Layout(bgap=8), B=Layout(bgap=4), C=Layout(bgap=8 if N == 40 else 5)))
    out.append(Case(37, 40, 100, tb=1, splitk=3, batch=3, shared_b=True, beta=1.0, family=family, C=Layout(bgap=12, pad=4)))
    return out


SPLITK = splitk_cases()
SPLITK_GAUSS = [c for c in splitk_cases("gauss")][::5]


@pytest.mark.parametrize("case", SPLITK, ids=ids(SPLITK))
def test_splitk_exact(case):
    verify([case])


def test_splitk_cases_hit_both_reductions_and_slice_counts():
    assert {R.reduce_is_vector(c) for c in SPLITK} == {True, False}
    counts = {R.effective_splitk(c) for c in SPLITK}
    assert {2, 3, 7, 13} <= counts                         # fewer than 4, the 4- and 8-wide unrolled loops and their tails
    assert any(c.splitk > c.K // 16 for c in SPLITK) and any(c.batch > 1 and not R.reduce_is_vector(c) for c in SPLITK)


@pytest.mark.parametrize("case", SPLITK_GAUSS, ids=ids(SPLITK_GAUSS))
def test_splitk_gauss_is_deterministic(case, request):
    first = verify([case], request=request)
    second = verify([case])
    assert same_bits(first[0], second[0])


# ---- batch -----------------------------------------------------------------------------------------------------------------------------
BATCH = ([Case(40, 24, 12, ta=ta, tb=tb, batch=nb, A=Layout(bgap=8), B=Layout(bgap=4), C=Layout(bgap=8, pad=4), **EPI)
          for nb in (1, 3) for ta, tb in TT] +
         [Case(41, 23, 13, ta=ta, tb=tb, batch=3, A=Layout(bgap=5, pad=1), B=Layout(bgap=3), C=Layout(bgap=7, pad=1), **EPI) for ta, tb in TT] +
         [Case(40, 24, 12, ta=ta, tb=tb, batch=3, shared_b=True, A=Layout(bgap=8), C=Layout(bgap=8), **EPI) for ta, tb in TT] +
         # vector loaders with batch strides that are no multiple of four floats (the class is decided by the first entry's view)
         [Case(40, 24, 12, ta=ta, tb=tb, batch=3, A=Layout(bgap=6), B=Layout(bgap=2), C=Layout(bgap=1), **EPI) for ta, tb in TT])


@pytest.mark.parametrize("case", BATCH, ids=ids(BATCH))
def test_batch_exact(case):
    verify([case])


# ---- column sums -----------------------------------------------------------------------------------------------------------------------
COLSUM = [Case(M, N, K, ta=ta, splitk=sk, colsum=True, colsum_beta=cb, beta=cb, bias=bool(ta))
          for (M, N, K) in ((130, 136, 50), (20, 131, 100), (130, 40, 33))
          for ta in (0, 1) for sk, cb in ((1, 0.0), (1, 1.0), (4, 0.0), (4, 1.0))]


@pytest.mark.parametrize("case", COLSUM, ids=ids(COLSUM))
def test_column_sums_exact(case):
    verify([case])


COLSUM_GAUSS = [c.replace(family="gauss") for c in COLSUM[4:12]]


@pytest.mark.parametrize("case", COLSUM_GAUSS, ids=ids(COLSUM_GAUSS))
def test_column_sums_gauss(case, request):
    verify([case], request=request)


@pytest.mark.parametrize("sk", [1, 4])
def test_column_sum_entry_among_plain_entries_of_a_group(sk):
    plain = Case(130, 136, 50, ta=1, splitk=sk, **EPI)
    cs = Case(130, 136, 50, ta=1, splitk=sk, colsum=True, colsum_beta=1.0, seed=3)
    assert R.layout_class(plain) == R.layout_class(cs)
    verify([plain, cs, plain.replace(seed=2, splitk=1)], grouped=True)


# ---- groups ----------------------------------------------------------------------------------------------------------------------------
def small(i, **kw):
    return Case(20, 24, 20 + i % 5, seed=i, **{**EPI, **kw})


@pytest.mark.parametrize("n", [9, 17])
def test_group_of_more_than_eight_entries_of_one_class(n):
    cases = [small(i, ta=1) for i in range(n)]
    assert len({R.layout_class(c) for c in cases}) == 1
    verify(cases, grouped=True)


def test_group_of_four_classes_interleaved():
    cases = [small(i, ta=TT[i % 4][0], tb=TT[i % 4][1], A=Layout(pad=i % 2)) for i in range(12)]
    assert len({R.layout_class(c) for c in cases}) >= 4
    verify(cases, grouped=True)


def test_group_of_split_and_unsplit_entries_of_one_class():
    """An unsplit entry's reduction block must do nothing; the slabs of the split entries are carved consecutively from one workspace
    (37 x 41 x 3 floats is no multiple of four: the next slab starts at the next multiple)."""
    cases = [Case(37, 41, 100, ta=1, A=Layout(pad=1), seed=0, **EPI), Case(37, 41, 100, ta=1, A=Layout(pad=1), splitk=3, seed=1, **EPI),
             Case(130, 41, 100, ta=1, A=Layout(pad=1), seed=2, **EPI), Case(37, 41, 200, ta=1, A=Layout(pad=1), splitk=16, seed=3, **EPI),
             Case(5, 41, 40, ta=1, A=Layout(pad=1), splitk=2, seed=4, C=Layout(T=2, gap=1), **EPI)]
    assert len({R.layout_class(c) for c in cases}) == 1
    verify(cases, grouped=True)


def test_group_column_sums_of_split_and_unsplit_entries_share_a_launch():
    cases = [Case(40, 136, 100, ta=1, splitk=sk, colsum=cs, colsum_beta=1.0, beta=1.0, seed=i)
             for i, (sk, cs) in enumerate(((4, True), (1, True), (3, False), (8, True), (1, False)))]
    assert len({R.layout_class(c) for c in cases}) == 1
    verify(cases, grouped=True)


@pytest.mark.parametrize("split_at", [(48, 49), (0, 20, 47, 48, 49)])
def test_group_of_fifty_entries_flushes_at_48(split_at):
    """The Python-side flush at 48 collected entries hands the whole workspace back; the 49th entry's slab must be carved after it
    (it was carved before, and then overlapped the 50th's)."""
    cases = [small(i, ta=1, splitk=3 if i in split_at else 1) for i in range(50)]
    verify(cases, grouped=True)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def descriptor(p, t, ws=None):
    from avsr_tf1_amd import ops
    from avsr_tf1_amd._lib import GemmDesc
    c = p.case
    d = GemmDesc()
    d.A, d.B, d.C = (ops.mat(t[w.lower()], g["ld"], T=g["T"], ldo=g["ldo"], offset=g["offset"]) for w, g in p.mats.items())
    d.M, d.N, d.K, d.trans_a, d.trans_b = c.M, c.N, c.K, c.ta, c.tb
    d.alpha, d.beta, d.batch, d.splitk = c.alpha, c.beta, c.batch, c.splitk
    d.stride_a, d.stride_b, d.stride_c = p.strides
    if t["bias"] is not None:
        d.bias = ops.fptr(t["bias"], c.bias_offset)
    if t["cs"] is not None:
        d.colsum, d.colsum_beta = ops.fptr(t["cs"], R.CS_OFFSET), c.colsum_beta
    if ws is not None:
        d.workspace, d.workspace_floats = ops.fptr(ws), ws.numel()
    return d


REFUSALS = {
    # name: (case, descriptor edits, expected code).  Every one of them would stay inside its buffers if it were accepted -- which is
    # why a null C, the 2 GB extent checks and a split that would really use a missing workspace are not among them.
    "M_zero": (Case(8, 8, 8), dict(M=0), ERR_ARG),
    "M_negative": (Case(8, 8, 8), dict(M=-1), ERR_ARG),
    "N_zero": (Case(8, 8, 8), dict(N=0), ERR_ARG),
    "N_negative": (Case(8, 8, 8), dict(N=-3), ERR_ARG),
    "K_negative": (Case(8, 8, 8), dict(K=-1), ERR_ARG),
    "A_null": (Case(8, 8, 0, bias=True), dict(A=None), ERR_ARG),                 # K = 0: no operand element would be fetched
    "B_null": (Case(8, 8, 0, bias=True), dict(B=None), ERR_ARG),
    "splitk_without_workspace": (Case(8, 8, 16, splitk=2), dict(), ERR_ARG),     # K = 16 runs as one slice: the workspace is never touched
    "splitk_workspace_too_small": (Case(8, 8, 64, splitk=2), dict(workspace_floats=2 * 8 * 8 - 1), ERR_ARG),
    "colsum_workspace_too_small": (Case(8, 8, 64, splitk=2, colsum=True), dict(workspace_floats=2 * 8 * 8 + 2 * 8 - 1), ERR_ARG),
    "colsum_trans_b": (Case(8, 8, 8, colsum=True), dict(trans_b=1), ERR_UNSUPPORTED),
    "colsum_batch": (Case(8, 8, 8, colsum=True), dict(batch=2), ERR_UNSUPPORTED),  # strides 0: both entries would address the one matrix
}


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_the_destination_alone(name, batched):
    from avsr_tf1_amd import _lib
    from avsr_tf1_amd._lib import GemmDesc, Mat, stream_ptr
    case, edits, code = REFUSALS[name]
    L = _lib.load()
    ps = [problem(case), problem(case.replace(seed=1))]
    ts = [R.to_device(p, torch) for p in ps]
    ws = None if name == "splitk_without_workspace" else workspace()
    good, bad = descriptor(ps[0], ts[0], ws), descriptor(ps[1], ts[1], ws)
    for k, v in edits.items():
        if v is None:
            m = getattr(bad, k)
            setattr(bad, k, Mat(None, m.ld, m.T, 0, m.ldo))
        else:
            setattr(bad, k, v)
    if batched:      # a refused entry refuses the whole call: the valid first entry is not launched either
        rc = L.avsr_gemm_batch((GemmDesc * 2)(good, bad), 2, stream_ptr())
    else:
        rc = L.avsr_gemm(ctypes.byref(bad), stream_ptr())
    torch.cuda.synchronize()
    assert rc == code
    for p, t in zip(ps, ts) if batched else [(ps[1], ts[1])]:
        assert np.array_equal(t["c"].cpu().numpy().view(np.uint32), p.c.view(np.uint32))
        if p.cs is not None:
            assert np.array_equal(t["cs"].cpu().numpy().view(np.uint32), p.cs.view(np.uint32))


def test_more_than_64_entries_are_refused():
    from avsr_tf1_amd import _lib
    from avsr_tf1_amd._lib import GemmDesc, stream_ptr
    p = problem(Case(8, 8, 8))
    t = R.to_device(p, torch)
    d = descriptor(p, t)
    L = _lib.load()
    assert L.avsr_gemm_batch((GemmDesc * 65)(*([d] * 65)), 65, stream_ptr()) == ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(t["c"].cpu().numpy().view(np.uint32), p.c.view(np.uint32))
    assert L.avsr_gemm_batch((GemmDesc * 64)(*([d] * 64)), 64, stream_ptr()) == 0          # 64 is the limit itself
    torch.cuda.synchronize()
    R.check(p, *R.fetch(t))

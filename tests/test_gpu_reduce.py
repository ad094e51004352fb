"""Column reductions (csrc/reduce.hip) against fp64 sums computed on the host from the same inputs.

avsr_colsum and avsr_colsum_multi at the shapes where the partial pass changes path (the group path with 256 and 85 row groups, F = 255
where one group is left and the wide path takes over, the first F with 16-byte loads, an F that is no multiple of 4, more than one
16-byte round per thread) and where the final pass's four-in-flight loop, its remainder loop and the tree all run; the deferred slab
reductions through avsr_conv_bwd_weight, whose partial slabs stay in the caller's scratch and are summed here in fp64.

Bounds (u = 2^-24, A = sum |terms| of a column, S = their exact sum):
  partial pass   fp32 products and a chain of at most `rows per block` additions per partial row: rpb * u * A in all
  final pass     fp64 over at most 2048 rows (2^-50 * A covers it), ONE rounding to fp32: u * |S|; alpha: u * |alpha S|; beta: u * |result|
The slab reductions have no partial pass of their own, so their bound is the final pass's alone."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROWS = (1, 32, 33, 4129)
FS = (1, 3, 255, 256, 257, 1028)
T_INNER = 7                                      # two-level addressing: 7 rows per outer slice, slices (T + 2) * ld apart
VARIANTS = list(itertools.product((0, 1), (0, 1), (0, 1), (0.0, 1.0)))      # with b, two-level, base offset by one float, beta
POOL = 6 * 1024 * 1024


@functools.lru_cache(maxsize=None)
def _pools():
    rng = np.random.default_rng(20261018)
    a = rng.standard_normal(POOL).astype(np.float32)
    b = rng.standard_normal(POOL).astype(np.float32)
    return a, b, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def _layout(rows, F, two, off):
    """(ld, T, ldo, element offset of every row) of a [rows, F] record inside the pools."""
    if not two:
        return F, 0, 0, off + np.arange(rows, dtype=np.int64) * F
    ld = F + 4
    ldo = (T_INNER + 2) * ld
    r = np.arange(rows, dtype=np.int64)
    return ld, T_INNER, ldo, off + (r // T_INNER) * ldo + (r % T_INNER) * ld


@functools.lru_cache(maxsize=None)
def _reference(rows, F, with_b, two, off):
    """fp64 column sums S and sums of magnitudes A of the record's terms a * b."""
    a, b, _, _ = _pools()
    idx = _layout(rows, F, two, off)[3][:, None] + np.arange(F, dtype=np.int64)[None, :]
    assert idx.max() < POOL
    t = a[idx].astype(np.float64)
    if with_b:
        t = t * b[idx].astype(np.float64)
    return t.sum(0), np.abs(t).sum(0)


def _mats(rows, F, with_b, two, off):
    from avsr_tf1_amd import ops
    _, _, da, db = _pools()
    ld, T, ldo, _ = _layout(rows, F, two, off)
    return ops.mat(da, ld, T=T, ldo=ldo, offset=off), (ops.mat(db, ld, T=T, ldo=ldo, offset=off) if with_b else None)


def _out_buffer(F, seed):
    """Destination of F floats at an odd offset inside a guarded buffer, with its initial contents."""
    o0 = np.random.default_rng(seed).standard_normal(F + 8).astype(np.float32)
    return torch.from_numpy(o0).cuda(), o0


def _check(got, o0, S, A, alpha, beta, rpb, what):
    F = S.shape[0]
    assert (got[:3] == o0[:3]).all() and (got[3 + F:] == o0[3 + F:]).all(), what
    res = alpha * S + beta * o0[3:3 + F].astype(np.float64)
    tol = abs(alpha) * (rpb * U * A + 2.0 * U * np.abs(S) + 2.0 ** -50 * A) + (U * np.abs(res) if beta else 0.0)
    err = np.abs(got[3:3 + F].astype(np.float64) - res)
    print("%s: max err %.3e, max err / bound %.3f" % (what, err.max(), (err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all(), (what, err.max(), tol[err.argmax()])


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("rows", ROWS)
def test_colsum(rows, F):
    from avsr_tf1_amd import ops
    scratch = torch.empty(((rows + 31) // 32) * F, device="cuda")
    for k, (with_b, two, off, beta) in enumerate(VARIANTS):
        alpha = 0.75 if beta else 1.0
        A_, B_ = _mats(rows, F, with_b, two, off)
        out, o0 = _out_buffer(F, k)
        ops.colsum(A_, rows, F, out, scratch, b=B_, alpha=alpha, beta=beta, out_offset=3)
        S, A = _reference(rows, F, with_b, two, off)
        _check(out.cpu().numpy(), o0, S, A, alpha, beta, min(rows, 32), (rows, F, with_b, two, off, beta))


def _multi(jobs):
    """jobs: (rows, F, with_b, two, off, alpha, beta) -> one avsr_colsum_multi call; every job is checked."""
    from avsr_tf1_amd import _lib, ops
    outs, arr = [], []
    need = 0
    for k, (rows, F, with_b, two, off, alpha, beta) in enumerate(jobs):
        A_, B_ = _mats(rows, F, with_b, two, off)
        out, o0 = _out_buffer(F, 100 + k)
        outs.append((out, o0))
        arr.append(_lib.ColsumJob(A_, B_ if B_ is not None else _lib.Mat(None, 0, 0, 0, 0), ops.fptr(out, 3), rows, F, alpha, beta))
        rpb = max(32, (rows + 255) // 256)
        need += ((rows + rpb - 1) // rpb) * F
    scratch = torch.empty(need, device="cuda")
    _lib.check(_lib.load().avsr_colsum_multi((_lib.ColsumJob * len(arr))(*arr), len(arr), ops.fptr(scratch), scratch.numel(), _lib.stream_ptr()),
               "avsr_colsum_multi")
    for (rows, F, with_b, two, off, alpha, beta), (out, o0) in zip(jobs, outs):
        S, A = _reference(rows, F, with_b, two, off)
        _check(out.cpu().numpy(), o0, S, A, alpha, beta, min(rows, max(32, (rows + 255) // 256)), (rows, F, with_b, two, off, beta))


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("rows", ROWS)
def test_colsum_multi(rows, F):
    """The sixteen variants of a shape as sixteen jobs of one call (4129 rows: 130 blocks of 32 rows per job)."""
    _multi([(rows, F, with_b, two, off, 0.75 if beta else 1.0, beta) for with_b, two, off, beta in VARIANTS])


def test_colsum_multi_33_jobs_of_mixed_width():
    """More than 32 jobs: two launch pairs; the partial rows of jobs of odd width leave later jobs' rows unaligned in the scratch."""
    fs, rs = (3, 256, 1, 1028, 255, 64, 257), (33, 1, 100, 32)
    _multi([(rs[k % 4], fs[k % 7], k & 1, (k >> 1) & 1, (k >> 2) & 1, 1.0, float(k % 3 == 0)) for k in range(33)])


# ------------------------------------------------------------------------------------------------
# deferred slab reductions: (Ci, Co, with bias).  Co = 8 takes the pixel-pair form (kind 1: every output is the sum of two slab columns),
# Co = 16 with a bias the one-slab form whose columns split between the weight and the bias gradient (kind 0, split < F, out2)
SLAB_CONFIGS = [(3, 8, True), (3, 8, False), (8, 8, True), (8, 8, False), (4, 16, True)]
SLAB_N, SLAB_H = 129 * 16, 6                     # >= 129 workgroups whatever number of frames (<= 16) a workgroup takes per pass


@functools.lru_cache(maxsize=None)
def _conv_operands(Ci, Co):
    rng = np.random.default_rng(Ci * 100 + Co)
    x = torch.from_numpy(rng.standard_normal((SLAB_N, SLAB_H, SLAB_H, Ci)).astype(np.float32)).cuda()
    dy = torch.from_numpy(rng.standard_normal((SLAB_N, SLAB_H, SLAB_H, Co)).astype(np.float32)).cuda()
    return x, dy


def _slab_columns(Ci, Co, bias):
    """(slab width, slab columns behind every weight-gradient entry, behind every bias-gradient entry): lists of index arrays to add."""
    if Co != 8:
        wF = 9 * Ci * Co
        return wF + (Co if bias else 0), [np.arange(wF)], [wF + np.arange(Co)]
    # pixel-pair slab (conv_wgrad.hip): rows (ti, tj', ci) of a 3 x 4 window, columns (pixel parity, co); then 2 x 8 bias columns
    f = np.arange(9 * Ci * 8)
    co, ci, t = f & 7, (f >> 3) % Ci, (f >> 3) // Ci
    ti, tj = t // 3, t % 3
    w = [((ti * 4 + tj) * Ci + ci) * 16 + co, ((ti * 4 + tj + 1) * Ci + ci) * 16 + 8 + co]
    return 12 * Ci * 16 + (16 if bias else 0), w, [12 * Ci * 16 + np.arange(8), 12 * Ci * 16 + 8 + np.arange(8)]


def _deferred(calls):
    """calls: ((Ci, Co, bias), nblk, beta).  Every call gets a scratch region of exactly nblk slabs, which is what sets its number of
    partial slabs; all run between one slab_defer_begin / _end; the slabs are then summed on the host."""
    from avsr_tf1_amd import ops
    runs = []
    ops.slab_defer_begin()
    try:
        for k, ((Ci, Co, bias), nblk, beta) in enumerate(calls):
            x, dy = _conv_operands(Ci, Co)
            slab = _slab_columns(Ci, Co, bias)[0]
            d = ops.conv_desc(SLAB_N, SLAB_H, SLAB_H, Ci, Co, 3, 1, 1, 1, SLAB_H, SLAB_H)
            scratch = torch.full((nblk * slab,), float("nan"), device="cuda")
            rng = np.random.default_rng(k)
            dw0, db0 = rng.standard_normal(9 * Ci * Co).astype(np.float32), rng.standard_normal(Co).astype(np.float32)
            dw, db = torch.from_numpy(dw0).cuda(), torch.from_numpy(db0).cuda()
            ops.conv_bwd_weight(d, x, dy, dw, db if bias else None, scratch, beta=beta)
            runs.append((scratch, dw, db, dw0, db0))
    finally:
        ops.slab_defer_end()
    torch.cuda.synchronize()
    for ((Ci, Co, bias), nblk, beta), (scratch, dw, db, dw0, db0) in zip(calls, runs):
        slab, wcols, bcols = _slab_columns(Ci, Co, bias)
        P = scratch.cpu().numpy().astype(np.float64).reshape(nblk, slab)
        for cols, got, old in ((wcols, dw, dw0), (bcols, db, db0)) if bias else ((wcols, dw, dw0),):
            S, A = sum(P[:, c].sum(0) for c in cols), sum(np.abs(P[:, c]).sum(0) for c in cols)
            assert np.isfinite(S).all() and np.abs(S).max() > 0.0
            res = S + beta * old.astype(np.float64)
            tol = U * np.abs(S) + 2.0 ** -50 * A + (U * np.abs(res) if beta else 0.0)
            err = np.abs(got.cpu().numpy().astype(np.float64) - res)
            print("slab %s nblk %d beta %g: max err %.3e, max err / bound %.3f" % ((Ci, Co, bias), nblk, beta, err.max(), (err / tol).max()))
            assert (err <= tol).all(), ((Ci, Co, bias), nblk, beta, err.max())
        if not bias:
            assert (db.cpu().numpy() == db0).all()


@pytest.mark.parametrize("cfg", SLAB_CONFIGS)
def test_deferred_slabs(cfg):
    _deferred([(cfg, nblk, beta) for nblk in (1, 31, 129) for beta in (0.0, 1.0)])


def test_deferred_slabs_more_than_32_pushes():
    """The 33rd push flushes the first 32 in the middle of the collection."""
    _deferred([(SLAB_CONFIGS[k % 5], (1, 31, 129)[k % 3], float(k & 1)) for k in range(37)])

"""Inputs, fp64 reference and checker for the conformance suite of avsr_gemm / avsr_gemm_batch (csrc/gemm.hip):

    C[M,N] = alpha * opA(A)[M,K] * opB(B)[K,N] + beta * C + bias[N]          (+ colsum[n] = colsum_beta * colsum[n] + sum_k B[k,n])

A `Case` holds every knob of one call; `build(case)` makes the operand buffers (numpy fp32, padding included), the `ops.mat`
arguments and the fp64 expectation; `check(problem, c_out, cs_out)` judges what a kernel left in the buffers.

Poison.  Every float of A, B and bias that the operation does not own (ld padding, the gap rows of a two-level layout, floats before
the view's offset, gaps between batch entries) is NaN: one stray element in an accumulator shows.  Every float of the C and column-sum
buffers that the operation does not own holds SENTINEL, compared bit for bit afterwards.  Owned floats of C are NaN when beta == 0
(the kernel must not read them) and of the column sums when colsum_beta == 0.

Families.
  exact   non-zero small integers, alpha / beta / alpha_dev powers of two, bias and old C small integers: every partial sum, in any
          order and any split, is an integer below 2^24, so the fp32 result is EXACT and is compared with np.array_equal.
  mant_a  K <= 8, A odd integers with magnitude in [2^11, 2^12) (12 significant bits), B non-zero integers of magnitude <= 2^8; sums
  mant_b  stay <= 2^23.  mant_b swaps the roles.  A path that rounds an operand to bf16 or to an 11-bit significand changes the answer.
  gauss   standard normal, K <= GAUSS_KMAX; per element |err| <= gamma_n * (|alpha| |A| |B| + |beta C0| + |bias|), gamma_n = n u / (1 - n u),
          u = 2^-24, n = K + splitk + 3 (column sums: n = K + splitk + 1): the forward bound of an fp32 dot product in any order.

numpy only.  The three helpers at the end take the torch and ops modules as arguments so that the GPU tests and tools/gemm_shapes.py
drive the library the same way."""
import dataclasses
import typing

import numpy as np

U = 2.0 ** -24
SENTINEL = np.uint32(0x7FEDBEEF)      # a NaN with a payload: nothing computes it
# K cap of the gauss family: the bound grows as K^2, a reduced-precision operand's error as sqrt(K); tests/test_gemm_check_cpu.py
# verifies that operands rounded to 11 significant bits are still rejected at this K
GAUSS_KMAX = 256
EXACT_INT = 7                         # exact family: |a|, |b| in 1..7
CS_OFFSET = 7                         # the column sums live at an odd offset of their buffer


class GemmMismatch(AssertionError):
    pass


@dataclasses.dataclass(frozen=True)
class Layout:
    """Storage of one matrix of `rows` x `cols`: ld = cols + pad; T > 0: two-level rows, group g of T rows starts at
    g * ldo with ldo = (T + gap) * ld + ldo_extra; `offset`: floats before the view; `bgap`: floats between batch entries."""
    pad: int = 0
    T: int = 0
    gap: int = 0
    ldo_extra: int = 0
    offset: int = 0
    bgap: int = 0


@dataclasses.dataclass(frozen=True)
class Case:
    M: int
    N: int
    K: int
    ta: int = 0
    tb: int = 0
    alpha: float = 1.0
    beta: float = 0.0
    bias: bool = False
    bias_offset: int = 0
    alpha_dev: typing.Optional[float] = None
    batch: int = 1
    splitk: int = 1
    A: Layout = Layout()
    B: Layout = Layout()
    C: Layout = Layout()
    shared_b: bool = False            # stride_b = 0
    colsum: bool = False
    colsum_beta: float = 0.0
    family: str = "exact"
    seed: int = 0

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


def shape_of(case, which):
    """(rows, cols) as stored."""
    if which == "A":
        return (case.K, case.M) if case.ta else (case.M, case.K)
    if which == "B":
        return (case.N, case.K) if case.tb else (case.K, case.N)
    return case.M, case.N


def _geometry(L, rows, cols, batch, shared=False):
    ld = cols + L.pad
    r = np.arange(rows, dtype=np.int64)
    if L.T:
        ldo = (L.T + L.gap) * ld + L.ldo_extra
        rowoff = (r // L.T) * ldo + (r % L.T) * ld
    else:
        ldo = 0
        rowoff = r * ld
    span = int(rowoff[-1]) + cols if rows else 0
    tail = L.gap * ld if L.T else 0                     # the gap rows after the last group
    stride = 0 if (shared or batch == 1) else span + L.pad + tail + L.bgap
    nb = 1 if shared else batch
    idx = (L.offset + np.arange(nb, dtype=np.int64)[:, None, None] * stride + rowoff[None, :, None]
           + np.arange(cols, dtype=np.int64)[None, None, :])
    length = L.offset + (nb - 1) * stride + span + tail + 5
    return dict(ld=ld, T=L.T, ldo=ldo, offset=L.offset), stride, idx, length


def layout_class(case):
    """Operand-layout class exactly as gemm_prepare computes it (akc, bkc, vec a, vec b as bits 3..0); the buffers themselves are
    16-byte aligned, so a view's alignment is its offset's."""
    def vec_ok(L, rows, cols):
        ld = cols + L.pad
        ldo = (L.T + L.gap) * ld + L.ldo_extra
        return L.offset % 4 == 0 and ld % 4 == 0 and cols % 4 == 0 and (L.T == 0 or ldo % 4 == 0)
    va = vec_ok(case.A, *shape_of(case, "A"))
    vb = vec_ok(case.B, *shape_of(case, "B"))
    return (8 if case.ta == 0 else 0) | (4 if case.tb else 0) | (2 if va else 0) | (1 if vb else 0)


def effective_splitk(case):
    """The slice count the library runs for the requested factor (gemm_prepare: slices of a multiple of 16 along K)."""
    sk = max(1, case.splitk)
    kper = ((case.K + sk - 1) // sk + 15) // 16 * 16
    return max(1, (case.K + kper - 1) // kper) if kper > 0 else 1


def reduce_is_vector(case):
    """Whether the split-K reduction takes its 16-byte path (splitk_reduce_body), given a 16-byte aligned workspace."""
    g = _geometry(case.C, case.M, case.N, case.batch)
    ldc, ldoc, sC = g[0]["ld"], g[0]["ldo"], g[1]
    return (case.N % 4 == 0 and case.C.offset % 4 == 0 and ldc % 4 == 0 and sC % 4 == 0 and (case.C.T == 0 or ldoc % 4 == 0)
            and (not case.bias or case.bias_offset % 4 == 0))


def _pow2(x):
    return x != 0 and np.frexp(abs(float(x)))[0] == 0.5


def _nonzero_ints(rng, amax, shape):
    return rng.integers(1, amax + 1, size=shape) * rng.choice([-1, 1], size=shape)


def _mantissa_ints(rng, shape):
    return (2 * rng.integers(1 << 10, 1 << 11, size=shape) + 1) * rng.choice([-1, 1], size=shape)      # odd, 2^11 < |x| < 2^12


class Problem:
    pass


def build(case):
    c = case
    assert c.family in ("exact", "mant_a", "mant_b", "gauss")
    assert c.M > 0 and c.N > 0 and c.K >= 0 and c.batch >= 1
    assert not c.colsum or (c.tb == 0 and c.batch == 1)
    rng = np.random.default_rng([c.seed, c.M, c.N, c.K, c.ta, c.tb, c.batch])
    p = Problem()
    p.case = c
    p.mats, p.strides, p.idx = {}, [], {}
    lengths = {}
    for w, L in (("A", c.A), ("B", c.B), ("C", c.C)):
        rows, cols = shape_of(c, w)
        p.mats[w], s, p.idx[w], lengths[w] = _geometry(L, rows, cols, c.batch, shared=(w == "B" and c.shared_b))
        p.strides.append(s)
    nbB = 1 if c.shared_b else c.batch
    shA, shB = (c.batch,) + shape_of(c, "A"), (nbB,) + shape_of(c, "B")
    alpha_eff = float(np.float32(c.alpha) * np.float32(c.alpha_dev)) if c.alpha_dev is not None else float(np.float32(c.alpha))
    exact = c.family != "gauss"
    if exact:
        assert _pow2(c.alpha) and (c.beta == 0 or _pow2(c.beta)) and (c.alpha_dev is None or _pow2(c.alpha_dev))
        assert c.colsum_beta in (0.0, 1.0)
        if c.family == "exact":
            amax = bmax = EXACT_INT
            Av, Bv = _nonzero_ints(rng, amax, shA), _nonzero_ints(rng, bmax, shB)
        else:
            assert c.K <= 8, "the mantissa subfamily keeps its sums at or below 2^23 with K <= 8"
            big, small = (1 << 12) - 1, 1 << 8
            amax, bmax = (big, small) if c.family == "mant_a" else (small, big)
            Av = _mantissa_ints(rng, shA) if c.family == "mant_a" else _nonzero_ints(rng, small, shA)
            Bv = _mantissa_ints(rng, shB) if c.family == "mant_b" else _nonzero_ints(rng, small, shB)
            assert c.K * amax * bmax <= 1 << 23
        cmax = bimax = 9
        C0 = rng.integers(-cmax, cmax + 1, size=(c.batch, c.M, c.N))
        bias = rng.integers(-bimax, bimax + 1, size=c.N)
        cs_old = rng.integers(-cmax, cmax + 1, size=c.N)
        # the 2^24 condition: the accumulator (any order, any split) is an integer below 2^24, and every value of the epilogue
        # chain alpha*acc (+ beta*C0) (+ bias) is a multiple of `quantum` with fewer than 2^24 quanta
        assert c.K * amax * bmax < 1 << 24
        quantum = min(1.0, abs(alpha_eff), abs(c.beta) if c.beta else 1.0)
        top = c.K * amax * bmax * abs(alpha_eff) + abs(c.beta) * cmax + (bimax if c.bias else 0)
        assert top / quantum < 1 << 24, "exact family: the epilogue would round"
        assert c.K * bmax + cmax < 1 << 24
    else:
        assert c.K <= GAUSS_KMAX, "the gauss family only guards accumulation precision at small K"
        Av, Bv = rng.standard_normal(shA), rng.standard_normal(shB)
        C0, bias, cs_old = rng.standard_normal((c.batch, c.M, c.N)), rng.standard_normal(c.N), rng.standard_normal(c.N)
    Av, Bv, C0 = Av.astype(np.float32), Bv.astype(np.float32), C0.astype(np.float32)
    bias, cs_old = bias.astype(np.float32), cs_old.astype(np.float32)

    p.a = np.full(lengths["A"], np.nan, np.float32)
    p.a[p.idx["A"]] = Av
    p.b = np.full(lengths["B"], np.nan, np.float32)
    p.b[p.idx["B"]] = Bv
    p.c = np.full(lengths["C"], SENTINEL, np.uint32).view(np.float32)
    p.c[p.idx["C"]] = C0 if c.beta != 0 else np.nan
    p.bias = None
    if c.bias:
        p.bias = np.full(c.bias_offset + c.N + 3, np.nan, np.float32)
        p.bias[c.bias_offset:c.bias_offset + c.N] = bias
    p.alpha_dev = None if c.alpha_dev is None else np.array([c.alpha_dev, np.nan, np.nan, np.nan], np.float32)
    p.cs = None
    if c.colsum:
        p.cs = np.full(CS_OFFSET + c.N + 3, SENTINEL, np.uint32).view(np.float32)
        p.cs[CS_OFFSET:CS_OFFSET + c.N] = cs_old if c.colsum_beta != 0 else np.nan

    A64 = Av.astype(np.float64).transpose(0, 2, 1) if c.ta else Av.astype(np.float64)          # [batch, M, K]
    B64 = Bv.astype(np.float64).transpose(0, 2, 1) if c.tb else Bv.astype(np.float64)          # [batch | 1, K, N]
    p.A64, p.B64, p.C0, p.bias_v, p.cs_old, p.alpha_eff = A64, B64, C0.astype(np.float64), bias.astype(np.float64), cs_old.astype(np.float64), alpha_eff
    p.c_exp, p.c_mag = epilogue(p, np.matmul(A64, B64), np.matmul(np.abs(A64), np.abs(B64)))
    p.cs_exp = p.cs_mag = None
    if c.colsum:
        p.cs_exp = B64[0].sum(0) + (c.colsum_beta * p.cs_old if c.colsum_beta != 0 else 0.0)
        p.cs_mag = np.abs(B64[0]).sum(0) + np.abs(c.colsum_beta * p.cs_old)
    return p


def epilogue(p, prod, prod_abs=None):
    """alpha * prod + beta * C0 + bias in fp64 (and the magnitude the gauss bound scales with)."""
    c = p.case
    out = p.alpha_eff * prod
    mag = None if prod_abs is None else abs(p.alpha_eff) * prod_abs
    if c.beta != 0:
        out = out + c.beta * p.C0
        mag = None if mag is None else mag + np.abs(c.beta * p.C0)
    if c.bias:
        out = out + p.bias_v
        mag = None if mag is None else mag + np.abs(p.bias_v)
    return out, mag


def gamma(n):
    return n * U / (1.0 - n * U)


def _judge(name, exact, got, want, mag, n):
    """Worst err / bound (0.0 in the exact families); raises GemmMismatch."""
    if exact:
        if not np.array_equal(got, want):
            bad = np.argwhere(~(got == want))
            i = tuple(int(v) for v in bad[0])
            raise GemmMismatch("%s: %d element(s) differ from the exact result, first at %s: got %r, want %r" % (name, len(bad), i, got[i], want[i]))
        return 0.0
    err = np.abs(got - want)
    bound = gamma(n) * mag
    ok = err <= bound                  # False for NaN
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(int(v) for v in bad[0])
        raise GemmMismatch("%s: %d element(s) outside the fp32 dot-product bound (n = %d), first at %s: err %.3g, bound %.3g"
                           % (name, len(bad), n, i, err[i], bound[i]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


def _sentinel_intact(name, buf, owned_idx):
    keep = np.ones(buf.size, bool)
    keep[np.asarray(owned_idx).reshape(-1)] = False
    bits = np.ascontiguousarray(buf).view(np.uint32)
    bad = np.flatnonzero(keep & (bits != SENTINEL))
    if bad.size:
        raise GemmMismatch("%s: %d float(s) outside the operation's output were written, first at flat index %d" % (name, bad.size, int(bad[0])))


def check(p, c_out, cs_out=None):
    """Judge the C buffer (and the column-sum buffer) a kernel left behind; returns the worst err / bound ratio."""
    c = p.case
    exact = c.family != "gauss"
    c_out = np.asarray(c_out, np.float32).reshape(-1)
    assert c_out.size == p.c.size
    _sentinel_intact("C", c_out, p.idx["C"])
    ratio = _judge("C", exact, c_out[p.idx["C"]].astype(np.float64), p.c_exp, p.c_mag, c.K + max(1, c.splitk) + 3)
    if c.colsum:
        assert cs_out is not None, "the case has column sums: pass their buffer"
        cs_out = np.asarray(cs_out, np.float32).reshape(-1)
        assert cs_out.size == p.cs.size
        own = np.arange(CS_OFFSET, CS_OFFSET + c.N)
        _sentinel_intact("colsum", cs_out, own)
        ratio = max(ratio, _judge("colsum", exact, cs_out[own].astype(np.float64), p.cs_exp, p.cs_mag, c.K + max(1, c.splitk) + 1))
    return ratio


# ---- driving the library (the torch and ops modules are the caller's) ----------------------------------------------------------------
def workspace_floats(case):
    """What ops.gemm asks of the split-K workspace for this case."""
    return case.batch * max(1, case.splitk) * (case.M * case.N + (case.N if case.colsum else 0)) if case.splitk > 1 else 0


def to_device(p, torch):
    """Device copies of the problem's buffers (bit for bit)."""
    t = {}
    for k in ("a", "b", "c", "bias", "alpha_dev", "cs"):
        v = getattr(p, k)
        t[k] = None if v is None else torch.from_numpy(v.copy()).cuda()
    return t


def issue(p, t, ops, workspace=None):
    """The case's ops.gemm call on the buffers of to_device (inside a `with ops.gemm_group()` block it is only collected)."""
    c = p.case
    m = {w: ops.mat(t[w.lower()], g["ld"], T=g["T"], ldo=g["ldo"], offset=g["offset"]) for w, g in p.mats.items()}
    bias = None if t["bias"] is None else t["bias"][c.bias_offset:]
    ops.gemm(m["A"], m["B"], m["C"], c.M, c.N, c.K, trans_a=c.ta, trans_b=c.tb, alpha=c.alpha, beta=c.beta, bias=bias,
             batch=c.batch, strides=tuple(p.strides), splitk=c.splitk, workspace=workspace, alpha_dev=t["alpha_dev"],
             colsum=(t["cs"], CS_OFFSET) if c.colsum else None, colsum_beta=c.colsum_beta)


def fetch(t):
    """(C buffer, column-sum buffer | None) as numpy, after the caller synchronised."""
    return t["c"].cpu().numpy(), None if t["cs"] is None else t["cs"].cpu().numpy()

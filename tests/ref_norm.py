"""Inputs, fp64 reference, fp32 twin and checker for the conformance suite of the normalisations: the entry points of
csrc/batchnorm.hip (row-walking forms over a [rows][F] map, partial-row forms fed by [nparts][2C] statistics rows, fp64 forms around an
all-reduce) and the instance norm of csrc/conv.hip.

A `Case` names one call, or the short chain of calls that only make sense together (the three sync phases, the fp64 pair), with every
knob; `build(case)` makes the operand and output buffers (numpy, bands included), the fp64 expectation of every output, the magnitude
of its terms and the noise of an fp32 twin; `drive(p, engine, bufs)` issues the calls -- on the library (GpuEngine) or on the numpy fp32
`Twin` --; `check(p, out)` judges what was left in the buffers.  tests/test_norm_check_cpu.py runs all of it on the twin.

Poison.  Every operand sits at offset BAND (a multiple of 4 floats) of a buffer whose other floats are NaN; one case per backward form
shifts an operand by one float.  Every output sits between bands of SENTINEL, compared bit for bit afterwards; its own floats are NaN
where the call must not read them (y, the saved and emitted vectors, dx at dx_beta == 0, dgamma / dbeta at grad_beta == 0).  A
partial-row operand is followed by SENTINEL rows past row nparts, the stage-1 rows buffer is SENTINEL throughout (512 rows), the scratch is
SENTINEL with a band behind it.  Inputs are compared bit for bit after the call; a refused call must leave every output's bits alone.

Families.
  exact   x and dy integers of magnitude <= 3; per channel a few elements of x are moved by one so that sum x is a multiple of the row
          count: the mean is an integer.  build asserts sum |x|, sum x^2, sum (x - mean)^2, sum |dy|, sum |dy*x| < 2^24: every such sum is
          an integer fp32 holds in any order, compared with np.array_equal (sum_out, sq_out, the fp64 moments, avsr_bn_partials_f64,
          the stage-1 rows summed in fp64, dbeta, mean, dz).  One dropped, doubled or foreign row is a whole-number error at any size.
          (Adjusting the last element alone would push it to 4095 at 4096 rows and its square to 2^24, so the correction is spread one
          unit per element.)
  gauss   normal * sigma_c + mu_c, |mu_c| <= sigma_c; gamma from +-[0.5, 1.5] with both signs, beta ~ 0.3 N(0, 1)
  offset  gauss with mu_c = OFFSET_RATIO * sigma_c: where s2/count - m^2 of the partial-row forms cancels
  const   gauss with column 0 all zero and column 1 a non-zero constant (widths >= 8): invstd = rsqrt(eps), xhat = 0, y = beta

ReLU kink.  Under relu every element whose fp64 pre-activation gamma*xhat + beta lies within KINK * (|gamma*xhat| + |beta|) of zero is
resampled (exact family: beta = gamma * invstd * (k + 1/2), never near an integer multiple) and build asserts none is left: the mask is
the same in whatever order a kernel rounds the pre-activation, and y is exactly zero where the reference is.

Bounds (u = 2^-24).
  sum     sums over rows: |err| <= gamma_n * sum |terms|, n = rows + 2 (+ the roundings of a term), gamma_n = n u / (1 - n u)
  sum64   the same in fp64 (the fp64 moments and merges)
  vec     per-channel vectors (mean, invstd, scale, shift, moving_*, k1..k3, dgamma / dbeta of the finalisers), each channel relative
          to the sum of the magnitudes of ITS OWN terms: |err| <= max(T_VEC * mag, 8 * noise)
  map     y, xhat, dx per element: |err| <= max(T_MAP * mag, 8 * noise)
  noise   the distance of the fp32 twin (same formulas in numpy float32, sums in runs of 64 rows merged in fp64 as the kernels merge
          them, fp64 where the kernels hold fp64) from the fp64 expectation
  T_VEC, T_MAP: 8 x the twin's worst err / mag over the whole case table (`measure()`; the CPU test re-measures and pins them):
      measured worst  vec 2.36e-07   map 2.11e-07    ->    T_VEC = 1.9e-06, T_MAP = 1.7e-06
  Every case's 8 * noise stays below 10 * T * mag (asserted by the CPU test): noise never is the licence.  With the magnitudes of the
  cancelling terms counted (s2/count + m^2 for the partial-row variance) the offset family keeps mu / sigma = OFFSET_RATIO = 8 unreduced.

numpy and CPU torch only."""
import ctypes
import dataclasses

import numpy as np
import torch

U = 2.0 ** -24
SENTINEL = np.uint32(0x7FEDBEEF)      # a NaN with a payload: nothing computes it
BAND = 256
LIMIT = float(1 << 24)
STATS_ROWS = 512
KINK = 1e-4
OFFSET_RATIO = 8.0
T_VEC = 1.9e-6
T_MAP = 1.7e-6
ARG = -1
f32, f64 = np.float32, np.float64


class NormMismatch(AssertionError):
    pass


def gamma_n(n, u=U):
    return n * u / (1.0 - n * u)


@dataclasses.dataclass(frozen=True)
class Case:
    op: str
    rows: int                         # rows of the map (partial-row forms: the count behind the rows; instance norm: T)
    F: int
    family: str = "gauss"
    opts: tuple = ()                  # sorted (name, value) pairs, see the builders

    def o(self, k, d=None):
        return dict(self.opts).get(k, d)

    def replace(self, **kw):
        o = dict(self.opts)
        top = {k: kw.pop(k) for k in ("op", "rows", "F", "family") if k in kw}
        o.update(kw)
        return dataclasses.replace(self, opts=tuple(sorted(o.items())), **top)


def case(op, rows, F, family="gauss", **kw):
    return Case(op, rows, F, family, tuple(sorted(kw.items())))


def case_id(c):
    return "%s-%dx%d-%s%s" % (c.op, c.rows, c.F, c.family, "".join("-%s=%s" % kv for kv in c.opts if kv[0] != "plan"))


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def _exact_map(rng, rows, F):
    x = rng.integers(-3, 4, size=(rows, F)).astype(np.int64)
    for f in range(F):
        r = int(x[:, f].sum() % rows)
        if r == 0:
            continue
        if r <= rows - r:
            idx = np.flatnonzero(x[:, f] > -3)[:r]
            assert len(idx) == r
            x[idx, f] -= 1
        else:
            idx = np.flatnonzero(x[:, f] < 3)[:rows - r]
            assert len(idx) == rows - r
            x[idx, f] += 1
    assert (x.sum(0) % rows == 0).all() and np.abs(x).max() <= 3
    return x.astype(f32)


def draw_map(rng, rows, F, family):
    if family == "exact":
        return _exact_map(rng, rows, F)
    sig = rng.uniform(0.5, 2.0, F)
    mu = (OFFSET_RATIO if family == "offset" else rng.uniform(-1.0, 1.0, F)) * sig
    x = (rng.standard_normal((rows, F)) * sig + mu).astype(f32)
    if family == "const" and F >= 8:
        x[:, 0] = 0.0
        x[:, 1] = f32(1.75)
    return x


def draw_grad(rng, rows, F, family):
    if family == "exact":
        return rng.integers(-3, 4, size=(rows, F)).astype(f32)
    return rng.standard_normal((rows, F)).astype(f32)


def draw_affine(rng, F):
    g = rng.uniform(0.5, 1.5, F) * np.where(np.arange(F) % 3 == 1, -1.0, 1.0) * rng.choice([1.0, -1.0], F, p=[0.7, 0.3])
    if F >= 2:
        g[0], g[1 % F] = abs(g[0]), -abs(g[1 % F])                  # both signs in every case
    return g.astype(f32), (0.3 * rng.standard_normal(F)).astype(f32)


def stats64(x):
    x = np.asarray(x, f64)
    m = x.mean(0)
    return m, ((x - m) ** 2).mean(0)


def clear_kink(rng, x, g, b, eps, family, pre_of=None):
    """Move every element off the ReLU kink of gamma*xhat + beta (module docstring); returns (x, beta)."""
    if family == "exact":
        m, v = stats64(x)
        is32 = (1.0 / np.sqrt(v + eps)).astype(f32)
        b = (g.astype(f64) * is32 * (rng.integers(-1, 2, x.shape[1]) + 0.5)).astype(f32)
    for _ in range(50):
        m, v = stats64(x)
        xh = (x.astype(f64) - m) / np.sqrt(v + eps)
        gx = g.astype(f64) * xh
        bad = np.abs(gx + b) < KINK * (np.abs(gx) + np.abs(b))
        if not bad.any():
            return x, b
        assert family != "exact"
        x = x.copy()
        x[bad] = (x[bad] + rng.standard_normal(int(bad.sum())) * 0.5).astype(f32)
    raise AssertionError("the kink band could not be cleared")


class Q:
    """One judged output: kind, fp64 expectation, magnitude of its terms, roundings (sum kinds), noise (vec / map, from the twin)."""

    def __init__(self, kind, want=None, mag=None, n=0, zero_exact=False, same_as=None, slack=0.0):
        self.kind, self.want, self.mag, self.n, self.zero_exact, self.same_as = kind, want, mag, n, zero_exact, same_as
        self.slack = slack            # sum kinds: what an operand the call computed itself (the mean under the centred squares) may add
        self.noise = None


class Problem:
    def __init__(self, c):
        self.case = c
        self.inp, self.shift, self.out, self.q = {}, {}, {}, {}
        self.tail = {}                # input name -> SENTINEL floats appended (partial rows past nparts)
        self.alias = {}               # output name -> the input buffer it is (dz over dy, dx over dy)
        self.rc = 0                   # what every call of the chain must return
        self.scratch_floats = 0
        self.info = {}

    def add_in(self, name, v, shift=0, tail=0):
        self.inp[name], self.shift[name], self.tail[name] = np.ascontiguousarray(v), shift, tail

    def add_out(self, name, shape, old, q, shift=0, dtype=f32):
        """old None: NaN before the call (must not be read)."""
        self.out[name] = (tuple(shape), None if old is None else np.asarray(old, dtype), dtype)
        self.shift[name] = shift
        self.q[name] = q


def _poisoned(v, shift, tail):
    buf = np.full(v.size + 2 * BAND + 4 + tail, np.nan, v.dtype)
    buf[BAND + shift:BAND + shift + v.size] = v.reshape(-1)
    if tail:
        t = buf[BAND + shift + v.size:BAND + shift + v.size + tail]
        t.view(np.uint32)[:] = SENTINEL
    return buf


def _guarded(shape, old, shift, dtype):
    n = int(np.prod(shape))
    if dtype == f64:
        buf = np.full(n + 2 * BAND + 4, np.nan, f64)
        buf.view(np.uint32)[:] = SENTINEL
    else:
        buf = np.full(n + 2 * BAND + 4, SENTINEL, np.uint32).view(f32)
    buf[BAND + shift:BAND + shift + n] = np.nan if old is None else old.reshape(-1)
    return buf


class Bufs:
    """The buffers of one run, on the host (numpy) or on the device (to_dev / to_host given)."""

    def __init__(self, p, to_dev=None, to_host=None):
        self.p = p
        self.to_dev = to_dev or (lambda a: a.copy())
        self.to_host = to_host or (lambda a: a)
        self.i = {n: self.to_dev(_poisoned(v, p.shift[n], p.tail[n])) for n, v in p.inp.items()}
        self.o = {n: self.to_dev(_guarded(s, old, p.shift[n], dt)) for n, (s, old, dt) in p.out.items() if n not in p.alias}
        nfl = p.scratch_floats
        self.s = self.to_dev(np.full(nfl + BAND, SENTINEL, np.uint32).view(f32)) if nfl else None
        self.rcs = []
        self.ints = {}

    def I(self, name):
        if name is None or name not in self.p.inp:
            return None
        a = BAND + self.p.shift[name]
        return self.i[name][a:a + self.p.inp[name].size]

    def O(self, name):
        if name is None or name not in self.p.out:
            return None
        if name in self.p.alias:
            return self.I(self.p.alias[name])
        a = BAND + self.p.shift[name]
        return self.o[name][a:a + int(np.prod(self.p.out[name][0]))]

    def scratch(self):
        return self.s[:self.p.scratch_floats], self.p.scratch_floats

    def result(self):
        r = {"rcs": list(self.rcs), "ints": dict(self.ints)}
        r["in"] = {n: np.asarray(self.to_host(b)) for n, b in self.i.items()}
        r["out"] = {n: np.asarray(self.to_host(b)) for n, b in self.o.items()}
        if self.s is not None:
            r["scratch_band"] = np.asarray(self.to_host(self.s[self.p.scratch_floats:]))
        return r


# ---- the plan and the scratch of a case ------------------------------------------------------------------------------------------------
PLAN_OF = {"fwd": "fwd", "bwd": "bwd", "sync": "sync_sum", "moments": "sync_moments", "stage1": "bwd_stage1", "bwd_apply": "bwd_apply"}
SCRATCH_ROW = {"fwd": (1, 2), "bwd": (2, 2), "sync": (1, 0), "moments": (4, 0)}      # floats per partial row and behind them, in units of F


def _plan(op, rows, F, scratch=1 << 40, flags=()):
    from avsr_tf1_amd import ops
    return ops.batchnorm_plan(op, rows, F, scratch, flags)


def bwd_flags(c):
    route = c.o("route", "both")
    fl = []
    if not c.o("misalign"):
        fl.append("aligned")
    if route == "both":
        fl.append("direct")
    if c.o("dx", True):
        fl.append("dx")
    return fl


def scratch_floats_of(c):
    """scratch option: None = ample (the natural grid), ("rows", k) = k partial rows and what lies behind, "short" = one float less than
    one partial row and what lies behind."""
    if c.op not in SCRATCH_ROW:
        return 0
    row, tail = SCRATCH_ROW[c.op]
    rows = max(c.o("shards", (c.rows,))) if c.op == "sync" else c.rows
    s = c.o("scratch")
    if s is None:
        nat = _plan(PLAN_OF[c.op], rows, c.F, 1 << 40, bwd_flags(c) if c.op == "bwd" else ())
        k = nat["blocks"] if not nat["err"] else 1
        return (k * row + tail) * c.F
    if s == "short":
        return (row + tail) * c.F - 1
    return (s[1] * row + tail) * c.F


def plan_of(c):
    """The plan of this case's (first) call on the scratch `build` gives it, or None where the entry point has no geometry to report."""
    if c.op not in PLAN_OF:
        return None
    rows = c.o("shards", (c.rows,))[0] if c.op == "sync" else c.rows
    return _plan(PLAN_OF[c.op], rows, c.F, scratch_floats_of(c), bwd_flags(c) if c.op == "bwd" else ())


def plan_err_of(p):
    """The code the plan must report for a built case: the call's own, but for a refusal that hangs on a pointer the plan never sees."""
    return 0 if p.case.o("moving") == "one" else p.rc


# ---- builders: operands, outputs and their fp64 expectations -----------------------------------------------------------------------------
def _rng(c):
    return np.random.default_rng([c.o("seed", 0), c.rows, c.F, sorted(BUILDERS).index(c.op), ("exact", "gauss", "offset", "const").index(c.family)])


def _fwd_q(p, x, g, b, m, v, eps, relu, names=("y",), rows_slices=None):
    """y of (x - m) * (g * is) + b, its magnitudes; per-channel A1 = mean |x| stands for the mean's own error."""
    x64, g64, b64 = x.astype(f64), g.astype(f64), b.astype(f64)
    is_ = 1.0 / np.sqrt(v + eps)
    y = (x64 - m) * (g64 * is_) + b64
    a1 = np.abs(x64).mean(0) if x64.size else 0.0
    mag = (np.abs(x64) + np.maximum(a1, np.abs(m))) * np.abs(g64 * is_) * (1.0 + 0.5 * is_ * is_ * v) + np.abs(b64)
    if relu:
        y = np.maximum(y, 0.0)
    return y, mag


def _vec_stats_q(p, x, m, v, eps, vmag=None):
    """(mean, invstd) expectations with their magnitudes: mean |x|; invstd + 0.5 invstd^3 * (the variance's terms)."""
    is_ = 1.0 / np.sqrt(v + eps)
    a1 = np.abs(np.asarray(x, f64)).mean(0)
    vm = v if vmag is None else vmag
    return (m, a1), (is_, is_ + 0.5 * is_ ** 3 * vm)


def _moving(p, name, old, new, newmag, mom):
    """momentum * old + (1 - momentum) * new, in the floats the kernels use."""
    mom32 = f64(f32(mom))
    om = f64(f32(1.0) - f32(mom))
    want = mom32 * old.astype(f64) + om * new
    p.add_out(name, old.shape, old, Q("vec", want, np.abs(mom32 * old) + om * newmag))


def _assert_exact_sums(x, dy=None, m=None):
    x = x.astype(f64)
    assert np.abs(x).sum(0).max() < LIMIT and (x * x).sum(0).max() < LIMIT
    if m is not None:
        assert np.array_equal(m, np.rint(m)), "the exact family's mean is not an integer"
        assert ((x - m) ** 2).sum(0).max() < LIMIT
    if dy is not None:
        dy = dy.astype(f64)
        assert np.abs(dy).sum(0).max() < LIMIT and np.abs(dy * x).sum(0).max() < LIMIT


def build_fwd(c, p, rng):
    """avsr_batchnorm_fwd_ex (door "ex") / avsr_batchnorm_fwd (door "plain": eps 1e-3, momentum 0.99, no relu, biased)."""
    rows, F = c.rows, c.F
    plain = c.o("door", "ex") == "plain"
    eps, mom = (1e-3, 0.99) if plain else (c.o("eps", 1e-5), c.o("momentum", 0.98))
    relu, bessel, training = (0, 0, c.o("training", 1)) if plain else (c.o("relu", 0), c.o("bessel", 1), c.o("training", 1))
    x = draw_map(rng, rows, F, c.family)
    g, b = draw_affine(rng, F)
    mm, mv = (0.2 * rng.standard_normal(F)).astype(f32), rng.uniform(0.5, 2.0, F).astype(f32)
    if relu and training:
        x, b = clear_kink(rng, x, g, b, f64(f32(eps)), c.family)
    m, v = stats64(x)
    if c.family == "exact":
        _assert_exact_sums(x, None, m)
    p.scratch_floats = scratch_floats_of(c)
    pl = _plan("fwd", rows, F, p.scratch_floats)
    p.rc = pl["err"]
    p.add_in("x", x), p.add_in("gamma", g), p.add_in("beta", b)
    p.info.update(eps=eps, momentum=mom, relu=relu, bessel=bessel, training=training, plain=plain)
    e = f64(f32(eps))
    save, moving = c.o("save", True), c.o("moving", True)
    if moving == "one":                                  # moving_mean without moving_var
        p.rc = ARG
    if p.rc:
        p.add_out("y", x.shape, None, Q("untouched"))
        if save:
            p.add_out("save_mean", (F,), None, Q("untouched")), p.add_out("save_invstd", (F,), None, Q("untouched"))
        if moving:
            p.add_out("moving_mean", (F,), mm, Q("untouched"))
            if moving != "one":
                p.add_out("moving_var", (F,), mv, Q("untouched"))
        return
    if training:
        y, ymag = _fwd_q(p, x, g, b, m, v, e, relu)
        (qm, am), (qi, ai) = _vec_stats_q(p, x, m, v, e)
        if save:
            p.add_out("save_mean", (F,), None, Q("exact" if c.family == "exact" else "vec", qm, am))
            p.add_out("save_invstd", (F,), None, Q("vec", qi, ai))
        if moving:
            fac = rows / max(1.0, rows - 1.0) if bessel else 1.0
            _moving(p, "moving_mean", mm, m, am, mom)
            _moving(p, "moving_var", mv, v * fac, v * fac, mom)
    else:
        assert moving
        for _ in range(50 if relu else 0):             # the kink of the moving statistics' pre-activation
            pre = (x.astype(f64) - mm) * (g.astype(f64) / np.sqrt(mv + e)) + b
            bad = np.abs(pre) < KINK * (np.abs(pre - b) + np.abs(b))
            if not bad.any():
                break
            x[bad] = (x[bad] + rng.standard_normal(int(bad.sum())) * 0.5).astype(f32)
        assert not relu or not bad.any()
        is_ = 1.0 / np.sqrt(mv.astype(f64) + e)
        y = (x.astype(f64) - mm) * (g.astype(f64) * is_) + b
        ymag = (np.abs(x.astype(f64)) + np.abs(mm)) * np.abs(g * is_) + np.abs(b.astype(f64))
        if relu:
            y = np.maximum(y, 0.0)
        p.add_out("moving_mean", (F,), mm, Q("untouched")), p.add_out("moving_var", (F,), mv, Q("untouched"))
        if save:
            p.add_out("save_mean", (F,), None, Q("untouched")), p.add_out("save_invstd", (F,), None, Q("untouched"))
    p.add_out("y", x.shape, None, Q("map", y, ymag, zero_exact=bool(relu)))


def drive_fwd(p, E, B):
    c, i = p.case, p.info
    s, nfl = B.scratch()
    if i["plain"]:
        B.rcs.append(E("batchnorm_fwd", B.I("x"), B.O("y"), c.rows, c.F, B.I("gamma"), B.I("beta"), B.O("moving_mean"), B.O("moving_var"),
                       B.O("save_mean"), B.O("save_invstd"), i["training"], s, nfl))
    else:
        B.rcs.append(E("batchnorm_fwd_ex", B.I("x"), B.O("y"), c.rows, c.F, B.I("gamma"), B.I("beta"), B.O("moving_mean"), B.O("moving_var"),
                       B.O("save_mean"), B.O("save_invstd"), i["training"], i["eps"], i["momentum"], i["relu"], i["bessel"], s, nfl))


def _given_stats(x, eps):
    m, v = stats64(x)
    return m.astype(f32), (1.0 / np.sqrt(v + eps)).astype(f32)


def build_apply(c, p, rng):
    """avsr_batchnorm_apply (opt xhat=True: avsr_batchnorm_xhat) on given mean / invstd."""
    rows, F, relu, eps = c.rows, c.F, c.o("relu", 0), 1e-5
    x = draw_map(rng, rows, F, c.family)
    g, b = draw_affine(rng, F)
    if relu:
        x, b = clear_kink(rng, x, g, b, eps, c.family)
    m32, is32 = _given_stats(x, eps)
    p.add_in("x", x), p.add_in("mean", m32), p.add_in("invstd", is32)
    p.info.update(relu=relu)
    x64, m, is_ = x.astype(f64), m32.astype(f64), is32.astype(f64)
    if c.o("xhat"):
        p.rc = 0
        p.add_out("xhat", x.shape, None, Q("map", (x64 - m) * is_, (np.abs(x64) + np.abs(m)) * is_))
        return
    p.rc = ARG if F % 4 else 0
    p.add_in("gamma", g), p.add_in("beta", b)
    if p.rc:
        p.add_out("y", x.shape, None, Q("untouched"))
        return
    y = (x64 - m) * (g.astype(f64) * is_) + b
    p.add_out("y", x.shape, None, Q("map", np.maximum(y, 0.0) if relu else y, (np.abs(x64) + np.abs(m)) * np.abs(g * is_) + np.abs(b.astype(f64)),
                                    zero_exact=bool(relu)))


def drive_apply(p, E, B):
    c = p.case
    if c.o("xhat"):
        B.rcs.append(E("batchnorm_xhat", B.I("x"), B.I("mean"), B.I("invstd"), B.O("xhat"), c.rows, c.F))
    else:
        B.rcs.append(E("batchnorm_apply", B.I("x"), B.O("y"), c.rows, c.F, B.I("gamma"), B.I("beta"), B.I("mean"), B.I("invstd"), p.info["relu"]))


def bn_backward64(x, dy, g, b, eps, relu):
    """(dx, dgamma, dbeta, dy') of sum(dy * relu?(batch_norm(x))) by torch fp64 autograd on the defining formula."""
    xt = torch.tensor(x.astype(f64), requires_grad=True)
    gt = torch.tensor(g.astype(f64), requires_grad=True)
    bt = torch.tensor(b.astype(f64), requires_grad=True)
    m = xt.mean(0)
    v = ((xt - m) ** 2).mean(0)
    y = (xt - m) / torch.sqrt(v + eps) * gt + bt
    mask = (y > 0).numpy() if relu else np.ones(x.shape, bool)
    if relu:
        y = torch.relu(y)
    (y * torch.tensor(dy.astype(f64))).sum().backward()
    return xt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy(), dy.astype(f64) * mask


def build_bwd(c, p, rng):
    """avsr_batchnorm_bwd.  route: both | none | one (dbeta alone) | misaligned (dgamma one float off); misalign: an operand's name."""
    rows, F, relu, eps = c.rows, c.F, c.o("relu", 0), 1e-5
    dxb, route, has_dx = c.o("dx_beta", 0.0), c.o("route", "both"), c.o("dx", True)
    x = draw_map(rng, rows, F, c.family)
    dy = draw_grad(rng, rows, F, c.family)
    g, b = draw_affine(rng, F)
    if relu:
        x, b = clear_kink(rng, x, g, b, eps, c.family)
    m32, is32 = _given_stats(x, eps)
    if c.family == "exact":
        _assert_exact_sums(x, dy, stats64(x)[0])
    sh = {c.o("misalign"): 1} if c.o("misalign") else {}
    for n, v in (("x", x), ("dy", dy), ("gamma", g), ("beta", b), ("mean", m32), ("invstd", is32)):
        p.add_in(n, v, shift=sh.get(n, 0))
    p.info.update(relu=relu, dx_beta=dxb)
    p.scratch_floats = scratch_floats_of(c)
    p.rc = _plan("bwd", rows, F, p.scratch_floats, bwd_flags(c))["err"]
    old = None if dxb == 0.0 else draw_grad(rng, rows, F, c.family) * f32(2.0 if c.family == "exact" else 1.0)
    outs = [("dx", x.shape, old)] * has_dx + [("dbeta", (F,), None)] * (route != "none") + [("dgamma", (F,), None)] * (route in ("both", "misaligned"))
    if p.rc:
        for n, s, o_ in outs:
            p.add_out(n, s, o_, Q("untouched"))
        return
    dx, dg, db, dm = bn_backward64(x, dy, g, b, eps, relu)
    x64, is_, m = x.astype(f64), is32.astype(f64), m32.astype(f64)
    xh = (x64 - m) * is_
    xhm = (np.abs(x64) + np.abs(m)) * is_
    if has_dx:
        mag = np.abs(g * is_) * (np.abs(dm) + (np.abs(dm).sum(0) + np.abs(xh) * (np.abs(dm) * xhm).sum(0)) / rows) * (1.0 + xhm / np.maximum(np.abs(xh), 1.0))
        if old is not None:
            dx, mag = dx + f64(f32(dxb)) * old, mag + np.abs(f64(f32(dxb)) * old)
        p.add_out("dx", x.shape, old, Q("map", dx, mag), shift=sh.get("dx", 0))
    if route != "none":
        p.add_out("dbeta", (F,), None, Q("exact" if c.family == "exact" else "sum", db, np.abs(dm).sum(0), rows + 2))
    if route in ("both", "misaligned"):
        p.add_out("dgamma", (F,), None, Q("sum", dg, (np.abs(dm) * xhm).sum(0), rows + 6), shift=1 if route == "misaligned" else 0)


def drive_bwd(p, E, B):
    c = p.case
    s, nfl = B.scratch()
    B.rcs.append(E("batchnorm_bwd", B.I("x"), B.I("dy"), B.I("gamma"), B.I("beta"), B.I("mean"), B.I("invstd"), B.O("dx"), B.O("dgamma"), B.O("dbeta"),
                   c.rows, c.F, p.info["relu"], p.info["dx_beta"], s, nfl))


def build_sync(c, p, rng):
    """The three sync phases over shards (rows = their sum), the host adding between them: one avsr_batchnorm_fwd_ex(bessel = 0) on the
    whole map.  opt wrong_total: nothing (the twin's fault uses it)."""
    shards, F, relu, eps, mom = c.o("shards"), c.F, c.o("relu", 0), 1e-3, 0.99
    rows = sum(shards)
    assert rows == c.rows
    x = draw_map(rng, rows, F, c.family)
    g, b = draw_affine(rng, F)
    if relu:
        x, b = clear_kink(rng, x, g, b, f64(f32(eps)), c.family)
    m, v = stats64(x)
    if c.family == "exact":
        _assert_exact_sums(x, None, m)
    e = f64(f32(eps))
    y, ymag = _fwd_q(p, x, g, b, m, v, e, relu)
    (qm, am), (qi, ai) = _vec_stats_q(p, x, m, v, e)
    mm, mv = (0.2 * rng.standard_normal(F)).astype(f32), rng.uniform(0.5, 2.0, F).astype(f32)
    p.add_in("gamma", g), p.add_in("beta", b)
    p.info.update(eps=eps, momentum=mom, relu=relu)
    p.scratch_floats = scratch_floats_of(c)
    p.rc = _plan("sync_sum", max(shards), F, p.scratch_floats)["err"]
    ex = c.family == "exact"
    r0 = 0
    for j, n in enumerate(shards):
        xs = x[r0:r0 + n]
        x64 = xs.astype(f64)
        p.add_in("x%d" % j, xs)
        p.add_out("sum%d" % j, (F,), None, Q("exact" if ex else "sum", x64.sum(0), np.abs(x64).sum(0), n + 2))
        p.add_out("mean%d" % j, (F,), None, Q("exact" if ex else "vec", qm, am))
        # the centred squares move by 2 |x - m| dm under a mean that is off by dm <= T_VEC * mean |x|
        p.add_out("sq%d" % j, (F,), None, Q("exact" if ex else "sum", ((x64 - m) ** 2).sum(0), ((np.abs(x64) + np.maximum(am, np.abs(m))) ** 2).sum(0), n + 4,
                                            slack=2.0 * T_VEC * am * np.abs(x64 - m).sum(0)))
        p.add_out("invstd%d" % j, (F,), None, Q("vec", qi, ai))
        _moving(p, "moving_mean%d" % j, mm, m, am, mom)
        _moving(p, "moving_var%d" % j, mv, v, v, mom)
        p.add_out("y%d" % j, xs.shape, None, Q("map", y[r0:r0 + n], ymag[r0:r0 + n], zero_exact=bool(relu)))
        r0 += n
    # the all-reduced operands are made on the host between the phases
    p.add_out("sum_global", (F,), None, Q("exact" if ex else "sum", x.astype(f64).sum(0), np.abs(x.astype(f64)).sum(0), rows + 4))
    p.add_out("sq_global", (F,), None, Q("exact" if ex else "sum", ((x.astype(f64) - m) ** 2).sum(0),
                                         ((np.abs(x.astype(f64)) + np.maximum(am, np.abs(m))) ** 2).sum(0), rows + 6,
                                         slack=2.0 * T_VEC * am * np.abs(x.astype(f64) - m).sum(0)))
    p.add_out("total", (1,), None, Q("exact", np.array([float(rows)]), None))
    if p.rc:                                             # the two phases that take a scratch refuse; nothing is written
        for name in p.q:
            p.q[name] = Q("untouched")


def drive_sync(p, E, B):
    c, i = p.case, p.info
    shards, F = c.o("shards"), c.F
    s, nfl = B.scratch()
    for j, n in enumerate(shards):
        B.rcs.append(E("batchnorm_sync_sum", B.I("x%d" % j), n, F, B.O("sum%d" % j), s, nfl))
    if p.rc:
        for j, n in enumerate(shards):
            B.rcs.append(E("batchnorm_sync_sqsum", B.I("x%d" % j), n, F, B.I("gamma"), B.I("beta"), B.O("mean%d" % j), B.O("sq%d" % j), s, nfl))
        return
    E.host_add(B.O("sum_global"), [B.O("sum%d" % j) for j in range(len(shards))])
    E.host_set(B.O("total"), float(sum(shards)))
    for j, n in enumerate(shards):
        B.rcs.append(E("batchnorm_sync_sqsum", B.I("x%d" % j), n, F, B.O("sum_global"), B.O("total"), B.O("mean%d" % j), B.O("sq%d" % j), s, nfl))
    E.host_add(B.O("sq_global"), [B.O("sq%d" % j) for j in range(len(shards))])
    for j, n in enumerate(shards):
        B.rcs.append(E("batchnorm_sync_apply", B.I("x%d" % j), B.O("y%d" % j), n, F, B.I("gamma"), B.I("beta"), B.O("moving_mean%d" % j),
                       B.O("moving_var%d" % j), B.O("mean%d" % j), B.O("sq_global"), B.O("total"), B.O("invstd%d" % j), i["eps"], i["momentum"], i["relu"]))


def build_moments(c, p, rng):
    """avsr_batchnorm_sync_moments: fp64 sum x | sum x^2."""
    x = draw_map(rng, c.rows, c.F, c.family)
    x64 = x.astype(f64)
    if c.family == "exact":
        _assert_exact_sums(x)
    p.add_in("x", x)
    p.scratch_floats = scratch_floats_of(c)
    p.rc = _plan("sync_moments", c.rows, c.F, p.scratch_floats)["err"]
    want = np.concatenate([x64.sum(0), (x64 * x64).sum(0)])
    q = Q("untouched") if p.rc else Q("exact" if c.family == "exact" else "sum64", want, np.concatenate([np.abs(x64).sum(0), (x64 * x64).sum(0)]), c.rows + 3)
    p.add_out("out64", (2 * c.F,), None, q, dtype=f64)


def drive_moments(p, E, B):
    s, nfl = B.scratch()
    B.rcs.append(E("batchnorm_sync_moments", B.I("x"), p.case.rows, p.case.F, B.O("out64"), s, nfl))


def partial_rows(a, b, nparts):
    """[nparts][2C] fp32 rows of the column sums of maps a | b split into nparts runs of rows (empty runs give zero rows)."""
    C = a.shape[1]
    rows = np.zeros((nparts, 2 * C), f32)
    for j, idx in enumerate(np.array_split(np.arange(a.shape[0]), nparts)):
        if idx.size:
            rows[j, :C] = a[idx].sum(0, dtype=f32)
            rows[j, C:] = b[idx].sum(0, dtype=f32)
    return rows


def build_finalize(c, p, rng):
    """avsr_bn_finalize (bessel = 1) / avsr_conv3d_bn_finalize (bessel = 0) on fixture-made rows of a [count][C] map in nparts runs; then
    avsr_bn_partials_f64 and (bessel = 1) avsr_bn_finalize_f64 with the count appended on the host: bit-equal outputs.
    opts: nparts, bessel, affine (scale / shift wanted), moving ("both" | "none" | "one"), momentum, negvar (channel 2 crafted)."""
    count, C, nparts, bessel = c.rows, c.F, c.o("nparts", 3), c.o("bessel", 1)
    eps, mom, affine, moving = 1e-5, c.o("momentum", 0.98), c.o("affine", True), c.o("moving", "both")
    x = draw_map(rng, count, C, c.family)
    part = partial_rows(x, x * x, nparts)
    if c.o("negvar"):                                  # sums no map can give: s2/count - m^2 = -9e-3 at mean 3
        part[:, 2], part[:, C + 2] = 0.0, 0.0
        part[0, 2], part[0, C + 2] = f32(3.0 * count), f32(9.0 * count * (1.0 - 1e-3))
    g, b = draw_affine(rng, C)
    mm, mv = (0.2 * rng.standard_normal(C)).astype(f32), rng.uniform(0.5, 2.0, C).astype(f32)
    p.add_in("part", part, tail=2 * C)
    p.add_in("gamma", g), p.add_in("beta", b)
    p.info.update(eps=eps, momentum=mom, bessel=bessel, nparts=nparts, moving=moving, affine=affine, f64pair=bool(bessel) and moving != "one")
    p.rc = ARG if moving == "one" else 0
    e = f64(f32(eps))
    s, s2 = part[:, :C].astype(f64).sum(0), part[:, C:].astype(f64).sum(0)
    sa = np.abs(part[:, :C].astype(f64)).sum(0)
    m = s / count
    v = np.maximum(s2 / count - m * m, 0.0)
    is_ = 1.0 / np.sqrt(v + e)
    am, vmag = sa / count, np.where(s2 / count - m * m < 0.0, 0.0, s2 / count + m * m)      # a clamped variance is exactly zero
    imag = is_ + 0.5 * is_ ** 3 * vmag
    ex = c.family == "exact"
    if ex:
        assert sa.max() < LIMIT and s2.max() < LIMIT and np.array_equal(m, np.rint(m))
    names = []

    def outs(sfx):
        if p.rc:
            for n in ("mean", "invstd") + ("scale", "shift") * affine:
                p.add_out(n + sfx, (C,), None, Q("untouched"))
            p.add_out("mov_mean" + sfx, (C,), mm, Q("untouched"))
            return
        same = (lambda n: n) if sfx else (lambda n: None)
        p.add_out("mean" + sfx, (C,), None, Q("exact" if ex else "vec", m, am, same_as=same("mean")))
        p.add_out("invstd" + sfx, (C,), None, Q("vec", is_, imag, same_as=same("invstd")))
        if affine:
            sc, scm = g * is_, np.abs(g) * imag
            p.add_out("scale" + sfx, (C,), None, Q("vec", sc, scm, same_as=same("scale")))
            p.add_out("shift" + sfx, (C,), None, Q("vec", b - m * sc, np.abs(b.astype(f64)) + am * np.abs(sc) + np.abs(m) * scm, same_as=same("shift")))
        if moving == "both":
            fac = count / (count - 1.0 if count > 1 else 1.0) if bessel else 1.0
            _moving(p, "mov_mean" + sfx, mm, m, am, mom)
            _moving(p, "mov_var" + sfx, mv, v * fac, vmag * fac, mom)
            p.q["mov_mean" + sfx].same_as, p.q["mov_var" + sfx].same_as = same("mov_mean"), same("mov_var")

    outs("")
    if not p.rc:
        p.add_out("sums64", (2 * C + 1,), None, Q("exact" if ex else "sum64", np.concatenate([s, s2, [float(count)]]),
                                                 np.concatenate([sa, s2, [float(count)]]), nparts + 2), dtype=f64)
        if p.info["f64pair"]:
            outs("_f64")


def drive_finalize(p, E, B):
    c, i = p.case, p.info
    C = c.F
    one = i["moving"] == "one"
    aff = i["affine"]
    args = lambda sfx: (B.O("mean" + sfx), B.O("invstd" + sfx), B.O("mov_mean" + sfx), None if one else B.O("mov_var" + sfx), B.I("gamma") if aff else None,
                        B.I("beta") if aff else None, B.O("scale" + sfx), B.O("shift" + sfx))
    B.rcs.append(E("bn_finalize" if i["bessel"] else "conv3d_bn_finalize", B.I("part"), i["nparts"], C, c.rows, i["eps"], i["momentum"], *args("")))
    if p.rc:
        return
    B.rcs.append(E("bn_partials_f64", B.I("part"), i["nparts"], C, B.O("sums64")))
    E.host_set(B.O("sums64")[2 * C:], float(c.rows))
    if i["f64pair"]:
        B.rcs.append(E("bn_finalize_f64", B.O("sums64"), C, i["eps"], i["momentum"], *args("_f64")))


def build_eval_affine(c, p, rng):
    C, eps = c.F, 1e-5
    g, b = draw_affine(rng, C)
    mm, mv = (0.5 * rng.standard_normal(C)).astype(f32), rng.uniform(0.0, 2.0, C).astype(f32)
    mv[0] = 0.0
    for n, v in (("gamma", g), ("beta", b), ("mov_mean", mm), ("mov_var", mv)):
        p.add_in(n, v)
    is_ = 1.0 / np.sqrt(mv.astype(f64) + f64(f32(eps)))
    sc = g * is_
    p.info.update(eps=eps)
    p.add_out("scale", (C,), None, Q("vec", sc, np.abs(sc)))
    p.add_out("shift", (C,), None, Q("vec", b - mm * sc, np.abs(b.astype(f64)) + 2 * np.abs(mm * sc)))


def drive_eval_affine(p, E, B):
    B.rcs.append(E("bn_eval_affine", B.I("gamma"), B.I("beta"), B.I("mov_mean"), B.I("mov_var"), p.info["eps"], B.O("scale"), B.O("shift"), p.case.F))


def build_stage1(c, p, rng):
    """avsr_bn_bwd_stage1.  mask: lazy (scale*x + shift > 0) | y (the written map > 0); alias: dz over dy."""
    rows, C, mask, alias = c.rows, c.F, c.o("mask", "lazy"), c.o("alias", False)
    ex = c.family == "exact"
    ok = C > 0 and C % 4 == 0 and C <= 1024
    x = draw_map(rng, rows, C, c.family)
    dy = draw_grad(rng, rows, C, c.family)
    if mask == "lazy":
        if ex:
            sc = rng.choice(np.array([1.0, 2.0, -1.0], f32), C)
            sh = (rng.integers(-2, 3, C) + 0.5).astype(f32)
        else:
            sc, sh = draw_affine(rng, C)
            for _ in range(50):
                pre = x.astype(f64) * sc + sh
                bad = np.abs(pre) < KINK * (np.abs(pre - sh) + np.abs(sh))
                if not bad.any():
                    break
                x[bad] = (x[bad] + rng.standard_normal(int(bad.sum())) * 0.5).astype(f32)
            assert not bad.any()
        keep = x.astype(f64) * sc + sh > 0
        p.add_in("scale", sc), p.add_in("shift", sh)
    else:
        y = np.maximum(rng.standard_normal((rows, C)), 0.0).astype(f32)     # a written ReLU output: exact zeros
        keep = y > 0
        p.add_in("y", y)
    p.add_in("x", x), p.add_in("dy", dy)
    p.rc = 0 if ok else ARG
    p.info.update(mask=mask)
    if p.rc:
        p.add_out("dz", x.shape, None, Q("untouched"))
        p.add_out("part", (STATS_ROWS * 2 * C,), np.full(STATS_ROWS * 2 * C, SENTINEL, np.uint32).view(f32), Q("untouched"))
        return
    dz = dy.astype(f64) * keep
    if ex:
        _assert_exact_sums(x, dy)
    if alias:
        p.alias["dz"] = "dy"
    p.add_out("dz", x.shape, dy if alias else None, Q("exact", dz, None))
    want = np.concatenate([dz.sum(0), (dz * x).sum(0)])
    pl = _plan("bwd_stage1", rows, C)
    p.info.update(nparts=pl["blocks"])
    p.add_out("part", (STATS_ROWS * 2 * C,), np.full(STATS_ROWS * 2 * C, SENTINEL, np.uint32).view(f32),
              Q("rows", want, np.concatenate([np.abs(dz).sum(0), np.abs(dz * x).sum(0)]), pl["rows_per_block"] + pl["blocks"] + 3))


def drive_stage1(p, E, B):
    c = p.case
    n = ctypes.c_int32(-7)
    lazy = p.info["mask"] == "lazy"
    B.rcs.append(E("bn_bwd_stage1", B.I("dy"), B.I("x"), B.I("scale") if lazy else None, B.I("shift") if lazy else None, None if lazy else B.I("y"),
                   B.O("dz"), c.rows, c.F, B.O("part"), n))
    B.ints["nparts"] = n.value


def _bwd_rows(c, rng, count, C, nparts):
    x = draw_map(rng, count, C, c.family)
    dz = draw_grad(rng, count, C, c.family) * (rng.random((count, C)) < 0.6)
    return x, dz.astype(f32), partial_rows(dz.astype(f32), (dz * x).astype(f32), nparts)


def _bwd_final64(C, sl, sxl, s, sx, sla, sxla, sa, sxa, count, m32, is32, g, old, gb):
    """bwd_finalize_channel in fp64 with the magnitudes of each output's terms."""
    m, is_, g = m32.astype(f64), is32.astype(f64), g.astype(f64)
    gb64 = f64(f32(gb))
    o = 0.0 if old is None else gb64 * old.astype(f64)
    dbeta, dbm = o + sl, np.abs(o) + sla
    dgamma, dgm = o + is_ * (sxl - m * sl), np.abs(o) + is_ * (sxla + np.abs(m) * sla)
    a, b = s / count, is_ * (sx - m * s) / count
    bm = is_ * (sxa + np.abs(m) * sa) / count
    k = np.concatenate([g * is_, -g * is_ * is_ * b, -g * is_ * a + g * is_ * is_ * b * m])
    km = np.concatenate([np.abs(g * is_), np.abs(g) * is_ * is_ * bm, np.abs(g) * is_ * sa / count + np.abs(g) * is_ * is_ * bm * np.abs(m)])
    return dgamma, dgm, dbeta, dbm, k, km


def build_bwd_finalize(c, p, rng):
    """avsr_bn_bwd_finalize on fixture-made rows, then avsr_bn_partials_f64 + avsr_bn_bwd_finalize_f64 (local == global): bit-equal.
    shards = (n0, n1): the fp64 form alone with local != global -- dgamma / dbeta of shard 0, k of the whole batch.
    opts: nparts, grad_beta, grads (dgamma / dbeta given)."""
    count, C, nparts, gb, grads, shards = c.rows, c.F, c.o("nparts", 3), c.o("grad_beta", 0.0), c.o("grads", True), c.o("shards")
    x, dz, part = _bwd_rows(c, rng, count, C, nparts)
    g, _ = draw_affine(rng, C)
    m32, is32 = _given_stats(x, 1e-5)
    old = None if gb == 0.0 else rng.standard_normal(C).astype(f32)
    for n, v in (("gamma", g), ("mean", m32), ("invstd", is32)):
        p.add_in(n, v)
    p.info.update(nparts=nparts, grad_beta=gb, grads=grads, shards=shards)
    col = lambda rows_: (rows_[:, :C].astype(f64).sum(0), rows_[:, C:].astype(f64).sum(0), np.abs(rows_[:, :C].astype(f64)).sum(0), np.abs(rows_[:, C:].astype(f64)).sum(0))

    def outs(sfx, loc, glo, same):
        dg, dgm, db, dbm, k, km = _bwd_final64(C, loc[0], loc[1], glo[0], glo[1], loc[2], loc[3], glo[2], glo[3], count, m32, is32, g, old, gb)
        sm = (lambda n: n) if same else (lambda n: None)
        if grads:
            p.add_out("dgamma" + sfx, (C,), old, Q("vec", dg, dgm, same_as=sm("dgamma")))
            p.add_out("dbeta" + sfx, (C,), old, Q("vec", db, dbm, same_as=sm("dbeta")))
        p.add_out("k" + sfx, (3 * C,), None, Q("vec", k, km, same_as=sm("k")))

    if shards:
        assert sum(shards) == count
        p0 = partial_rows(dz[:shards[0]], (dz * x)[:shards[0]].astype(f32), nparts)
        p1 = partial_rows(dz[shards[0]:], (dz * x)[shards[0]:].astype(f32), nparts)
        p.add_in("part", p0, tail=2 * C), p.add_in("part1", p1, tail=2 * C)
        l0, l1 = col(p0), col(p1)
        glo = tuple(a + b for a, b in zip(l0, l1))
        for j, l in enumerate((l0, l1)):
            p.add_out("local%d" % j, (2 * C,), None, Q("sum64", np.concatenate(l[:2]), np.concatenate(l[2:]), nparts + 2), dtype=f64)
        p.add_out("global", (2 * C + 1,), None, Q("sum64", np.concatenate([glo[0], glo[1], [float(count)]]), np.concatenate([glo[2], glo[3], [float(count)]]),
                                                  2 * nparts + 4), dtype=f64)
        outs("_f64", l0, glo, False)
        return
    p.add_in("part", part, tail=2 * C)
    loc = col(part)
    outs("", loc, loc, False)
    ex = c.family == "exact"
    if ex:
        assert loc[2].max() < LIMIT and loc[3].max() < LIMIT
    p.add_out("global", (2 * C + 1,), None, Q("exact" if ex else "sum64", np.concatenate([loc[0], loc[1], [float(count)]]),
                                              np.concatenate([loc[2], loc[3], [float(count)]]), nparts + 2), dtype=f64)
    outs("_f64", loc, loc, True)


def drive_bwd_finalize(p, E, B):
    c, i = p.case, p.info
    C = c.F
    g = i["grads"]
    tail = lambda sfx: (C, B.I("mean"), B.I("invstd"), B.I("gamma"), B.O("dgamma" + sfx) if g else None, B.O("dbeta" + sfx) if g else None, i["grad_beta"],
                        B.O("k" + sfx))
    if i["shards"]:
        B.rcs.append(E("bn_partials_f64", B.I("part"), i["nparts"], C, B.O("local0")))
        B.rcs.append(E("bn_partials_f64", B.I("part1"), i["nparts"], C, B.O("local1")))
        E.host_add(B.O("global")[:2 * C], [B.O("local0"), B.O("local1")])
        E.host_set(B.O("global")[2 * C:], float(c.rows))
        B.rcs.append(E("bn_bwd_finalize_f64", B.O("local0"), B.O("global"), *tail("_f64")))
        return
    B.rcs.append(E("bn_bwd_finalize", B.I("part"), i["nparts"], C, c.rows, *tail("")[1:]))
    B.rcs.append(E("bn_partials_f64", B.I("part"), i["nparts"], C, B.O("global")))
    E.host_set(B.O("global")[2 * C:], float(c.rows))
    B.rcs.append(E("bn_bwd_finalize_f64", B.O("global"), B.O("global"), *tail("_f64")))


def build_bwd_apply(c, p, rng):
    """avsr_bn_bwd_apply: dx = beta*dx + k1*dz + k2*x + k3."""
    rows, C, beta = c.rows, c.F, c.o("beta", 0.0)
    x, dz = draw_map(rng, rows, C, c.family), draw_grad(rng, rows, C, c.family)
    k = rng.standard_normal(3 * C).astype(f32)
    old = None if beta == 0.0 else rng.standard_normal((rows, C)).astype(f32)
    p.add_in("dz", dz), p.add_in("x", x), p.add_in("k", k)
    p.rc = ARG if C % 4 else 0
    p.info.update(beta=beta)
    if p.rc:
        p.add_out("dx", x.shape, old, Q("untouched"))
        return
    k64 = k.astype(f64)
    t = (k64[:C] * dz, k64[C:2 * C] * x, np.broadcast_to(k64[2 * C:], x.shape)) + (() if old is None else (f64(f32(beta)) * old,))
    p.add_out("dx", x.shape, old, Q("map", sum(t), sum(np.abs(a) for a in t)))


def drive_bwd_apply(p, E, B):
    B.rcs.append(E("bn_bwd_apply", B.I("dz"), B.I("x"), B.I("k"), B.O("dx"), p.case.rows, p.case.F, p.info["beta"]))


def build_instnorm(c, p, rng):
    """avsr_instnorm_fwd then avsr_instnorm_bwd on its mean / invstd (rows = T, opt B); alias: dx over dy."""
    T, F, Bn, eps = c.rows, c.F, c.o("B", 1), 1e-6
    x = np.stack([draw_map(rng, T, F, c.family) for _ in range(Bn)])
    dy = np.stack([draw_grad(rng, T, F, c.family) for _ in range(Bn)])
    g, b = draw_affine(rng, F)
    p.add_in("x", x), p.add_in("dy", dy), p.add_in("gamma", g), p.add_in("beta", b)
    p.info.update(eps=eps, B=Bn)
    e = f64(f32(eps))
    x64 = x.astype(f64)
    m = x64.mean(1)
    v = ((x64 - m[:, None]) ** 2).mean(1)
    is_ = 1.0 / np.sqrt(v + e)
    am = np.abs(x64).mean(1)
    ex = c.family == "exact"
    if ex:
        for i in range(Bn):
            _assert_exact_sums(x[i], dy[i], m[i])
    p.add_out("mean", (Bn, F), None, Q("exact" if ex else "vec", m, am))
    p.add_out("invstd", (Bn, F), None, Q("vec", is_, is_ + 0.5 * is_ ** 3 * v))
    gi = g.astype(f64) * is_
    xm = np.abs(x64) + np.maximum(am, np.abs(m))[:, None]
    p.add_out("y", x.shape, None, Q("map", (x64 - m[:, None]) * gi[:, None] + b, xm * np.abs(gi)[:, None] * (1.0 + 0.5 * (is_ * is_ * v)[:, None]) + np.abs(b.astype(f64))))
    xt = torch.tensor(x64, requires_grad=True)
    mt = xt.mean(1, keepdim=True)
    vt = ((xt - mt) ** 2).mean(1, keepdim=True)
    gt, bt = torch.tensor(g.astype(f64), requires_grad=True), torch.tensor(b.astype(f64), requires_grad=True)
    ((xt - mt) / torch.sqrt(vt + e) * gt + bt).mul(torch.tensor(dy.astype(f64))).sum().backward()
    d64 = dy.astype(f64)
    xh = (x64 - m[:, None]) * is_[:, None]
    xhm = xm * is_[:, None]
    p.add_out("dbeta_part", (Bn, F), None, Q("exact" if ex else "sum", d64.sum(1), np.abs(d64).sum(1), T + 2))
    p.add_out("dgamma_part", (Bn, F), None, Q("sum", (d64 * xh).sum(1), (np.abs(d64) * xhm).sum(1), T + 6))
    assert np.allclose(gt.grad.numpy(), (d64 * xh).sum((0, 1))) and np.allclose(bt.grad.numpy(), d64.sum((0, 1)))
    mag = np.abs(gi)[:, None] * (np.abs(d64) + (np.abs(d64).sum(1)[:, None] + np.abs(xh) * (np.abs(d64) * xhm).sum(1)[:, None]) / T) * (1.0 + xhm / np.maximum(np.abs(xh), 1.0))
    if c.o("alias"):
        p.alias["dx"] = "dy"
    p.add_out("dx", x.shape, dy if c.o("alias") else None, Q("map", xt.grad.numpy(), mag))


def drive_instnorm(p, E, B):
    c, i = p.case, p.info
    B.rcs.append(E("instnorm_fwd", B.I("x"), B.O("y"), i["B"], c.rows, c.F, B.I("gamma"), B.I("beta"), B.O("mean"), B.O("invstd"), i["eps"]))
    B.rcs.append(E("instnorm_bwd", B.I("x"), B.I("dy"), B.I("gamma"), B.O("mean"), B.O("invstd"), B.O("dx"), B.O("dgamma_part"), B.O("dbeta_part"),
                   i["B"], c.rows, c.F))


BUILDERS = {"fwd": (build_fwd, drive_fwd), "apply": (build_apply, drive_apply), "bwd": (build_bwd, drive_bwd), "sync": (build_sync, drive_sync),
            "moments": (build_moments, drive_moments), "finalize": (build_finalize, drive_finalize), "eval_affine": (build_eval_affine, drive_eval_affine),
            "stage1": (build_stage1, drive_stage1), "bwd_finalize": (build_bwd_finalize, drive_bwd_finalize), "bwd_apply": (build_bwd_apply, drive_bwd_apply),
            "instnorm": (build_instnorm, drive_instnorm)}
_CACHE = {}


def build(c, noise=True):
    """The problem of a case (cached: the reference is computed once and shared; nothing mutates it)."""
    if c in _CACHE:
        return _CACHE[c]
    p = Problem(c)
    BUILDERS[c.op][0](c, p, _rng(c))
    if noise:
        tw = run(p, Twin())
        for name, q in p.q.items():
            if q.kind in ("vec", "map"):
                q.noise = np.abs(_view(p, tw, name).astype(f64) - q.want)
                q.noise = np.where(np.isfinite(q.noise), q.noise, 0.0)
        if len(_CACHE) < 64 or sum(v.size for v in p.inp.values()) < (1 << 16):
            _CACHE[c] = p
    return p


def run(p, E, to_dev=None, to_host=None):
    B = Bufs(p, to_dev, to_host)
    BUILDERS[p.case.op][1](p, E, B)
    E.sync()
    return B.result()


def _view(p, res, name):
    shape, _, dt = p.out[name]
    if name in p.alias:
        a = BAND + p.shift[p.alias[name]]
        return res["in"][p.alias[name]][a:a + int(np.prod(shape))].reshape(shape)
    a = BAND + p.shift[name]
    return res["out"][name][a:a + int(np.prod(shape))].reshape(shape)


# ---- the checker -----------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == f64 else np.uint32)


def _first(badmask):
    return tuple(int(t) for t in np.argwhere(badmask)[0])


def check(p, res):
    """Judge what a run left behind.  Returns {output: (worst engine error, noise there, bound there, err / bound)} of the judged numbers."""
    c = p.case
    for rc in res["rcs"]:
        if rc != p.rc:
            raise NormMismatch("return code %d where %d is due (%s)" % (rc, p.rc, res["rcs"]))
    # inputs bit-unchanged (an aliased destination is judged as an output below)
    for name, v in p.inp.items():
        ref = _poisoned(v, p.shift[name], p.tail[name])
        got = res["in"][name]
        keep = np.ones(ref.size, bool)
        if name in p.alias.values():
            a = BAND + p.shift[name]
            keep[a:a + v.size] = False
        bad = keep & (_bits(ref) != _bits(got))
        if bad.any():
            raise NormMismatch("input %s: %d float(s) were written, first at %+d floats from its start" % (name, int(bad.sum()), int(np.flatnonzero(bad)[0]) - BAND))
    if "scratch_band" in res:
        bad = np.flatnonzero(_bits(res["scratch_band"]) != SENTINEL)
        if bad.size:
            raise NormMismatch("scratch: %d float(s) of the band behind it were written, first %d floats past its end" % (bad.size, int(bad[0])))
    report = {}
    for name, (shape, old, dt) in p.out.items():
        q = p.q[name]
        n = int(np.prod(shape))
        got = _view(p, res, name)
        if name not in p.alias:
            buf = res["out"][name]
            a = BAND + p.shift[name]
            keep = np.ones(buf.size, bool)
            keep[a:a + n] = False
            sent = np.uint64(SENTINEL) << np.uint64(32) | np.uint64(SENTINEL) if dt == f64 else SENTINEL
            bad = keep & (_bits(buf) != sent)
            if bad.any():
                raise NormMismatch("%s: %d float(s) of the bands around it were written, first at %+d floats from its start"
                                   % (name, int(bad.sum()), int(np.flatnonzero(bad)[0]) - a))
        if q.kind == "untouched":
            before = _guarded(shape, old, p.shift[name], dt)[BAND + p.shift[name]:BAND + p.shift[name] + n]
            if not np.array_equal(_bits(before), _bits(got.reshape(-1))):
                raise NormMismatch("%s: written by a call that %s" % (name, "was refused" if p.rc else "must leave it alone"))
            continue
        if q.kind == "rows":                               # the stage-1 partial rows: n of them, the rest untouched, summed in fp64
            nparts, C2 = res["ints"]["nparts"], 2 * c.F
            if nparts != p.info["nparts"]:
                raise NormMismatch("%s: %d partial rows reported where the plan says %d" % (name, nparts, p.info["nparts"]))
            flat = got.reshape(-1)
            if (_bits(flat[nparts * C2:]) != SENTINEL).any():
                raise NormMismatch("%s: a row beyond the %d reported ones was written" % (name, nparts))
            rows = flat[:nparts * C2].reshape(nparts, C2).astype(f64)
            if not np.isfinite(rows).all():
                raise NormMismatch("%s: row %d of %d was not written" % (name, _first(~np.isfinite(rows))[0], nparts))
            got = rows.sum(0)
            kind = "exact" if c.family == "exact" else "sum"
        else:
            kind = q.kind
        g64 = np.asarray(got, f64).reshape(np.shape(q.want))
        if kind == "exact":
            if not np.array_equal(g64, q.want):
                i = _first(~(g64 == q.want))
                raise NormMismatch("%s: %d element(s) differ from the exact result, first at %s: got %r, want %r" % (name, int((~(g64 == q.want)).sum()), i, g64[i], q.want[i]))
            report[name] = (0.0, 0.0, 0.0, 0.0)
        else:
            err = np.abs(g64 - q.want)
            if kind == "sum":
                bound, noise = gamma_n(q.n) * q.mag + q.slack, np.zeros_like(q.mag)
            elif kind == "sum64":
                bound, noise = gamma_n(q.n, 2.0 ** -53) * q.mag, np.zeros_like(q.mag)
            else:
                noise = q.noise if q.noise is not None else np.zeros_like(q.mag)
                bound = np.maximum((T_VEC if kind == "vec" else T_MAP) * q.mag, 8.0 * noise)
            ok = err <= bound                              # False for NaN
            if not ok.all():
                i = _first(~ok)
                raise NormMismatch("%s: %d element(s) outside the %s bound, first at %s: got %r, want %r, err %.3g, bound %.3g"
                                   % (name, int((~ok).sum()), kind, i, g64[i], q.want[i], err[i], bound[i]))
            if q.zero_exact and (g64[q.want == 0.0] != 0.0).any():
                raise NormMismatch("%s: not exactly zero under the ReLU where the reference is" % name)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, err / bound, 0.0)
            j = _first(ratio == ratio.max()) if ratio.size else ()
            report[name] = (float(err[j]), float(noise[j]), float(bound[j]), float(ratio[j])) if ratio.size else (0.0, 0.0, 0.0, 0.0)
        if q.same_as:
            other = _view(p, res, q.same_as)
            if not np.array_equal(_bits(other.reshape(-1)), _bits(np.asarray(got).reshape(-1))):
                raise NormMismatch("%s: not bit-equal to %s (one copy of the merge and of the tail was promised)" % (name, q.same_as))
    return report


def normq_lines(c, report):
    return ["NORMQ %s %-14s engine error %.3e  noise %.3e  bound %.3e  ratio %.3f" % ((case_id(c), n) + v) for n, v in sorted(report.items())]


def same_bytes(a, b):
    """Two runs of one case left identical bytes everywhere (no atomics)."""
    for grp in ("in", "out"):
        for n in a[grp]:
            if not np.array_equal(_bits(a[grp][n]), _bits(b[grp][n])):
                raise NormMismatch("%s: two identical calls left different bytes" % n)
    assert a["rcs"] == b["rcs"] and a["ints"] == b["ints"]


# ---- the engines -----------------------------------------------------------------------------------------------------------------------------
class GpuEngine:
    """The library's C entry points on device tensors; returns their codes."""

    def __init__(self, torch_, ops):
        self.t, self.ops = torch_, ops

    def __call__(self, name, *args):
        conv = lambda a: a.data_ptr() if self.t.is_tensor(a) else (ctypes.byref(a) if isinstance(a, ctypes.c_int32) else a)
        return getattr(self.ops._L(), "avsr_" + name)(*[conv(a) for a in args], self.ops._s())

    def host_add(self, dst, srcs):
        """An all-reduce: the ranks' vectors added on the host in their own precision."""
        self.t.cuda.synchronize()
        acc = srcs[0].cpu().numpy().copy()
        for s in srcs[1:]:
            acc = acc + s.cpu().numpy()
        dst.copy_(self.t.from_numpy(acc))

    def host_set(self, dst, value):
        dst.fill_(value)

    def sync(self):
        self.t.cuda.synchronize()


def _s32(a, axis=0):
    return a.sum(axis, dtype=f32)


def round_bf16(v):
    m, e = np.frexp(np.asarray(v, f64))
    return np.ldexp(np.round(m * 256.0) / 256.0, e).astype(f32)


class Twin:
    """The same formulas in numpy float32 (fp64 where the kernels hold fp64), honest -- or with one named fault (test_norm_check_cpu.py)."""

    def __init__(self, fault=None):
        self.fault = fault

    def __call__(self, name, *args):
        return getattr(self, name)(*args)

    def sync(self):
        pass

    def host_add(self, dst, srcs):
        acc = srcs[0].copy()
        for s in srcs[1:]:
            acc = acc + s
        dst[:] = acc

    def host_set(self, dst, value):
        dst[:] = value

    # -- row-walking forms --
    def _x(self, x, rows, F):
        x = x.reshape(rows, F)
        return round_bf16(x) if self.fault == "bf16_operand" else x

    def _colsum(self, t):
        """Column sums of the terms t [rows][F] as the partial-sum kernels take them: fp32 over runs of 64 rows, the runs merged in fp64."""
        rows, F = t.shape
        s = np.add.reduceat(t, np.arange(0, rows, 64), axis=0, dtype=f32).astype(f64).sum(0)
        if self.fault == "row_missing":
            s = s - t[rows - 1]
        if self.fault == "row_twice":
            s = s + t[0]
        if self.fault == "subgroup_last_row":
            assert F == 80 and rows > 61
            s = s - t[61]                                # block 0, sub-group 1 of G = 3: rows 1, 4, .., 61
        if self.fault == "base_tail":
            assert F == 260
            s[256:] = 0.0                                 # the four columns of the second pass
        return s

    def _stats(self, x, rows, eps, total=None):
        n = f64(rows if total is None else total)
        m = (self._colsum(x) / n).astype(f32)
        d = x - m
        var = (self._colsum(d * d) / n).astype(f32)
        return m, var, f32(1.0) / np.sqrt(var + f32(eps))

    def _mov(self, mm, mv, m, var, momentum):
        mom = f32(momentum)
        mm[:] = mom * mm + (f32(1.0) - mom) * m
        mv[:] = mom * mv + (f32(1.0) - mom) * var

    def batchnorm_fwd(self, x, y, rows, F, g, b, mm, mv, sm, si, training, s, nfl):
        return self.batchnorm_fwd_ex(x, y, rows, F, g, b, mm, mv, sm, si, training, 1e-3, 0.99, 0, 0, s, nfl)

    def batchnorm_fwd_ex(self, x, y, rows, F, g, b, mm, mv, sm, si, training, eps, momentum, relu, bessel, s, nfl):
        rc = _plan("fwd", rows, F, nfl)["err"]
        if rc or (mm is None) != (mv is None) or (not training and mm is None):
            if self.fault == "refused_writes":
                y[0] = 0.0
            return rc or ARG
        x = self._x(x, rows, F)
        if training:
            m, var, is_ = self._stats(x, rows, eps)
            if sm is not None:
                sm[:] = m
            if si is not None:
                si[:] = is_
            if mm is not None:
                if self.fault == "biased_for_bessel":
                    bessel = 0
                if self.fault == "bessel_for_biased":
                    bessel = 1
                self._mov(mm, mv, m, var * (f32(rows) / f32(max(1, rows - 1))) if bessel else var, momentum)
        else:
            m, is_ = mm.copy(), f32(1.0) / np.sqrt(mv + f32(eps))
        self._apply(x, y, m, is_, g, b, relu)
        if self.fault == "band_float":
            y.base[BAND + y.size] = 0.0
        return 0

    def _apply(self, x, y, m, is_, g, b, relu):
        v = (x - m) * (g * is_) + b
        y[:] = (np.maximum(v, f32(0)) if relu else v).reshape(-1)

    def batchnorm_apply(self, x, y, rows, F, g, b, m, is_, relu):
        if F % 4 or rows <= 0:
            return ARG
        self._apply(self._x(x, rows, F), y, m, is_, g, b, relu)
        return 0

    def batchnorm_xhat(self, x, m, is_, xhat, rows, F):
        xhat[:] = ((self._x(x, rows, F) - m) * is_).reshape(-1)
        return 0

    def batchnorm_bwd(self, x, dy, g, b, m, is_, dx, dgamma, dbeta, rows, F, relu, dx_beta, s, nfl):
        if _plan("bwd", rows, F, nfl)["err"]:
            if self.fault == "refused_writes" and dx is not None:
                dx[0] = 0.0
            return ARG
        x, d = self._x(x, rows, F), dy.reshape(rows, F).copy()
        xh = (x - m) * is_
        if relu:
            ga = np.abs(g) if self.fault == "neg_gamma_mask" else g
            pre = xh * ga + (f32(0) if self.fault == "beta_ignored" else b)
            d[~(pre > 0)] = 0.0
        s1, s2 = self._colsum(d).astype(f32), self._colsum(d * xh).astype(f32)
        if dx is not None:
            v = g * is_ * (d - (s1 + xh * s2) * (f32(1.0) / f32(rows)))
            if dx_beta != 0.0 or self.fault == "dx_beta_at_0":
                v = v + f32(dx_beta) * dx.reshape(rows, F)
            dx[:] = v.reshape(-1)
        if self.fault == "dgamma_dbeta_swapped":
            s1, s2 = s2, s1
        if dbeta is not None:
            dbeta[:] = s1
        if dgamma is not None:
            dgamma[:] = s2
        return 0

    def batchnorm_sync_sum(self, x, rows, F, out, s, nfl):
        if _plan("sync_sum", rows, F, nfl)["err"]:
            return ARG
        out[:] = self._colsum(self._x(x, rows, F))
        return 0

    def batchnorm_sync_sqsum(self, x, rows, F, sum_global, total, mean_out, sq_out, s, nfl):
        if _plan("sync_sqsum", rows, F, nfl)["err"]:
            return ARG
        n = f64(rows) if self.fault == "rows_for_global" else f64(int(total[0]))
        mean_out[:] = sum_global / n
        d = self._x(x, rows, F) - mean_out
        sq_out[:] = self._colsum(d * d)
        return 0

    def batchnorm_sync_apply(self, x, y, rows, F, g, b, mm, mv, mean, sq_global, total, invstd_out, eps, momentum, relu):
        if F % 4:
            return ARG
        n = f64(rows) if self.fault == "rows_for_global" else f64(int(total[0]))
        var = (sq_global / n).astype(f32)
        invstd_out[:] = f32(1.0) / np.sqrt(var + f32(eps))
        if mm is not None:
            self._mov(mm, mv, mean, var, momentum)
        self._apply(self._x(x, rows, F), y, mean, invstd_out, g, b, relu)
        return 0

    def batchnorm_sync_moments(self, x, rows, F, out64, s, nfl):
        if _plan("sync_moments", rows, F, nfl)["err"]:
            return ARG
        x = self._x(x, rows, F).astype(f64)
        t = np.concatenate([x, x * x], 1)
        out64[:] = t.sum(0) - (t[rows - 1] if self.fault == "row_missing" else 0.0) + (t[0] if self.fault == "row_twice" else 0.0)
        return 0

    # -- partial-row forms --
    def _merge(self, part, nparts, C, dtype=f64):
        if self.fault == "part_beyond":
            nparts += 1
        rows = part.base[BAND:BAND + nparts * 2 * C].reshape(nparts, 2 * C).astype(dtype)
        return rows[:, :C].sum(0, dtype=dtype), rows[:, C:].sum(0, dtype=dtype)

    def _final(self, s, s2, count, eps, momentum, bessel, mean, invstd, mm, mv, g, b, scale, shift):
        T = s.dtype.type
        m = s / T(count)
        var = s2 / T(count) - m * m
        if self.fault != "neg_var_nan":
            var = np.maximum(var, T(0))
        with np.errstate(invalid="ignore"):
            is_ = f32(1.0) / np.sqrt(var.astype(f32) + f32(eps))
        mean[:], invstd[:] = m, is_
        if scale is not None:
            sc = g * is_
            scale[:], shift[:] = sc, b - m.astype(f32) * sc
        if mm is not None:
            if self.fault == "biased_for_bessel":
                bessel = 0
            if self.fault == "bessel_for_biased":
                bessel = 1
            v = var * (T(count) / T(count - 1 if count > 1 else 1)) if bessel else var
            self._mov(mm, mv, m.astype(f32), v.astype(f32), momentum)      # (float)(var * count / (count - 1)), as the kernel

    def bn_finalize(self, part, nparts, C, count, eps, momentum, mean, invstd, mm, mv, g, b, scale, shift, bessel=1):
        if (mm is None) != (mv is None):
            if self.fault == "refused_writes":
                mean[0] = 0.0
            return ARG
        self._final(*self._merge(part, nparts, C), count, eps, momentum, bessel, mean, invstd, mm, mv, g, b, scale, shift)
        return 0

    def conv3d_bn_finalize(self, part, nparts, C, count, eps, momentum, mean, invstd, mm, mv, g, b, scale, shift):
        return self.bn_finalize(part, nparts, C, count, eps, momentum, mean, invstd, mm, mv, g, b, scale, shift, bessel=0)

    def bn_partials_f64(self, part, nparts, C, out64):
        s, s2 = self._merge(part, nparts, C)
        out64[:C], out64[C:2 * C] = s, s2
        return 0

    def bn_finalize_f64(self, sums, C, eps, momentum, mean, invstd, mm, mv, g, b, scale, shift):
        self._final(sums[:C].copy(), sums[C:2 * C].copy(), int(sums[2 * C]), eps, momentum, 1, mean, invstd, mm, mv, g, b, scale, shift)
        return 0

    def bn_eval_affine(self, g, b, mm, mv, eps, scale, shift, C):
        sc = g * (f32(1.0) / np.sqrt(mv + f32(eps)))
        scale[:], shift[:] = sc, b - mm * sc
        return 0

    def bn_bwd_stage1(self, dy, x, scale, shift, y, dz, rows, C, part, nparts):
        pl = _plan("bwd_stage1", rows, C)
        if pl["err"]:
            if self.fault == "refused_writes":
                dz[0] = 0.0
            return ARG
        x, d = x.reshape(rows, C), dy.reshape(rows, C)
        keep = (x * scale + shift > 0) if scale is not None else (y.reshape(rows, C) > 0)
        v = np.where(keep, d, f32(0))
        n, per = pl["blocks"], pl["rows_per_block"]
        for j in range(n):
            r = slice(j * per, min(rows, (j + 1) * per))
            part[j * 2 * C:j * 2 * C + C] = _s32(v[r])
            part[j * 2 * C + C:(j + 1) * 2 * C] = _s32(v[r] * x[r])
        if self.fault == "row_missing":
            part[:C] -= v[0]
        dz[:] = v.reshape(-1)
        nparts.value = n
        return 0

    def _bwd_final(self, C, sl, sxl, s, sx, count, mean, invstd, g, dgamma, dbeta, grad_beta, k):
        n = f64(count)
        gb = f32(grad_beta)
        mean, invstd, g = mean.astype(f64), invstd.astype(f64), g.astype(f64)
        if self.fault == "dgamma_dbeta_swapped":
            dgamma, dbeta = dbeta, dgamma
        if dbeta is not None:
            dbeta[:] = (gb * dbeta if grad_beta != 0.0 else f32(0)) + sl.astype(f32)
        if dgamma is not None:
            dgamma[:] = (gb * dgamma if grad_beta != 0.0 else f32(0)) + (invstd * (sxl - mean * sl)).astype(f32)
        a, b = s / n, invstd * (sx - mean * s) / n
        k2 = -g * invstd * invstd * b
        k[:C], k[C:2 * C], k[2 * C:] = g * invstd, (-k2 if self.fault == "k2_sign" else k2), -g * invstd * a + g * invstd * invstd * b * mean

    def bn_bwd_finalize(self, part, nparts, C, count, mean, invstd, g, dgamma, dbeta, grad_beta, k):
        s, sx = self._merge(part, nparts, C)
        self._bwd_final(C, s, sx, s, sx, count, mean, invstd, g, dgamma, dbeta, grad_beta, k)
        return 0

    def bn_bwd_finalize_f64(self, local, glob, C, mean, invstd, g, dgamma, dbeta, grad_beta, k):
        L, G = local.copy(), glob.copy()
        if self.fault == "local_for_global":
            G = np.concatenate([L, G[2 * C:]])
        self._bwd_final(C, L[:C], L[C:2 * C], G[:C], G[C:2 * C], int(glob[2 * C]), mean, invstd, g, dgamma, dbeta, grad_beta, k)
        return 0

    def bn_bwd_apply(self, dz, x, k, dx, rows, C, beta):
        if C % 4:
            if self.fault == "refused_writes":
                dx[0] = 0.0
            return ARG
        v = k[:C] * dz.reshape(rows, C) + k[C:2 * C] * x.reshape(rows, C) + k[2 * C:]
        if beta != 0.0 or self.fault == "dx_beta_at_0":
            v = v + f32(beta) * dx.reshape(rows, C)
        dx[:] = v.reshape(-1)
        return 0

    # -- instance norm --
    def instnorm_fwd(self, x, y, Bn, T, F, g, b, mean, invstd, eps):
        x = x.reshape(Bn, T, F)
        m = _s32(x, 1) / f32(T)
        if self.fault == "row_missing":
            m = (_s32(x, 1) - x[:, T - 1]) / f32(T)
        d = x - m[:, None]
        is_ = f32(1.0) / np.sqrt(_s32(d * d, 1) / f32(T) + f32(eps))
        mean[:], invstd[:] = m.reshape(-1), is_.reshape(-1)
        y[:] = (d * (g * is_)[:, None] + b).reshape(-1)
        return 0

    def instnorm_bwd(self, x, dy, g, mean, invstd, dx, dgp, dbp, Bn, T, F):
        x, d = x.reshape(Bn, T, F), dy.reshape(Bn, T, F)
        m, is_ = mean.reshape(Bn, 1, F), invstd.reshape(Bn, 1, F)
        xh = (x - m) * is_
        s1, s2 = _s32(d, 1), _s32(d * xh, 1)
        v = (g * is_) * (d - (s1 / f32(T))[:, None] - xh * (s2 / f32(T))[:, None])
        dgp[:], dbp[:] = s2.reshape(-1), s1.reshape(-1)
        dx[:] = v.reshape(-1)
        return 0


# ---- the kernels, by name, and which of them a case launches --------------------------------------------------------------------------------
KERNELS = sorted(["bn_partial_sum_kernel", "bn_mean_kernel", "bn_partial_sq_kernel", "bn_var_kernel", "bn_apply_kernel", "bn_xhat_kernel",
                  "bn_bwd_partial_kernel", "bn_bwd_apply_kernel", "bn_bwd_partial4_kernel", "bn_bwd_apply4_kernel", "bn_moments_partial_kernel",
                  "bn_moments_final_kernel", "bn_finalize_kernel<true>", "bn_finalize_kernel<false>", "bn_eval_affine_kernel", "bn_bwd_stage1_kernel",
                  "bn_bwd_finalize_kernel", "bn_bwd_coef_apply_kernel", "bn_partials_f64_kernel", "bn_finalize_f64_kernel", "bn_bwd_finalize_f64_kernel",
                  "instnorm_fwd_kernel", "instnorm_bwd_kernel"])


def kernels_of(p):
    """The kernels the calls of a built case launch, by the plan (none where the call is refused)."""
    c = p.case
    if p.rc:
        return set()
    if c.op == "fwd":
        return {"bn_apply_kernel"} | ({"bn_partial_sum_kernel", "bn_mean_kernel", "bn_partial_sq_kernel", "bn_var_kernel"} if p.info["training"] else set())
    if c.op == "apply":
        return {"bn_xhat_kernel"} if c.o("xhat") else {"bn_apply_kernel"}
    if c.op == "bwd":
        pl = plan_of(c)
        v = "4" if pl["vec"] else ""
        return {"bn_bwd_partial%s_kernel" % v} | ({"bn_bwd_apply%s_kernel" % v} if pl["apply_grid"] else set())
    if c.op == "sync":
        return {"bn_partial_sum_kernel", "bn_mean_kernel", "bn_partial_sq_kernel", "bn_var_kernel", "bn_apply_kernel"}
    if c.op == "moments":
        return {"bn_moments_partial_kernel", "bn_moments_final_kernel"}
    if c.op == "finalize":
        return {"bn_finalize_kernel<%s>" % ("true" if p.info["bessel"] else "false"), "bn_partials_f64_kernel"} | ({"bn_finalize_f64_kernel"} if p.info["f64pair"] else set())
    if c.op == "bwd_finalize":
        return {"bn_partials_f64_kernel", "bn_bwd_finalize_f64_kernel"} | (set() if p.info["shards"] else {"bn_bwd_finalize_kernel"})
    return {"eval_affine": {"bn_eval_affine_kernel"}, "stage1": {"bn_bwd_stage1_kernel"}, "bwd_apply": {"bn_bwd_coef_apply_kernel"},
            "instnorm": {"instnorm_fwd_kernel", "instnorm_bwd_kernel"}}[c.op]


# ---- the case table: the smallest shapes at which each form can go wrong ------------------------------------------------------------------------
def _table():
    T = []
    add = T.append
    fams = ("gauss", "offset", "const", "exact")
    # row-walking forward: every width class on every row count, the knobs rotating
    i = 0
    for F in (4, 12, 80, 128, 132, 256, 260):
        for rows in (1, 63, 64, 65, 197):
            i += 1
            add(case("fwd", rows, F, fams[i % 4], relu=i % 2, bessel=(i // 2) % 2, save=i % 3 != 0, moving=i % 5 != 0,
                     plan=(("G", 256 // F if F < 256 else 1), ("blocks", -(-rows // 64)), ("rows_per_block", 64))))
        add(case("fwd", 197, F, "exact", relu=1))
        add(case("fwd", 65, F, "gauss", training=0, relu=F % 8 == 4, save=F == 80))
        add(case("fwd", 65, F, "gauss", door="plain"))
    add(case("fwd", 131073, 4, "exact", plan=(("rows_per_block", 65), ("blocks", 2017), ("G", 64))))
    add(case("fwd", 131073, 4, "gauss", relu=1, plan=(("rows_per_block", 65),)))
    for F in (80, 260):
        add(case("fwd", 1000, F, "gauss", scratch=("rows", 3), plan=(("blocks", 3), ("rows_per_block", 334))))
        add(case("fwd", 1000, F, "exact", scratch=("rows", 3), plan=(("blocks", 3),)))
        add(case("fwd", 1000, F, "gauss", scratch="short", plan=(("err", ARG),)))
        add(case("fwd", 197, F, "gauss", scratch=("rows", 1), plan=(("blocks", 1), ("rows_per_block", 197))))
    for n in (1, 2, 5):                                  # momentum 0: the moving variance IS the variance the door feeds it
        for bessel in (0, 1):
            add(case("fwd", n, 8, "gauss", momentum=0.0, bessel=bessel))
    add(case("fwd", 5, 8, "gauss", momentum=0.0, door="plain"))
    add(case("fwd", 64, 6, "gauss", plan=(("err", ARG),)))            # F % 4
    for F in (6, 80, 260):
        add(case("apply", 65, F, "gauss", xhat=True))
    add(case("apply", 65, 80, "const", xhat=True))
    add(case("apply", 65, 80, "exact", xhat=True))
    add(case("apply", 197, 132, "exact", relu=1))
    for F in (4, 80, 260):
        add(case("apply", 197, F, "const" if F >= 8 else "gauss", relu=F != 80))
    add(case("apply", 5000, 1024, "gauss", relu=1))                     # past the 4096-block cap of the flat grid
    add(case("apply", 65, 6, "gauss"))                                  # refused
    # row-walking backward
    i = 0
    routes = ("both", "none", "one", "misaligned")
    for F in (12, 80, 256, 260):
        for rows in (1, 65, 4095):
            i += 1
            add(case("bwd", rows, F, fams[i % 4], relu=i % 2, dx_beta=(0.0, 1.0, 0.5)[i % 3], route=routes[i % 4],
                     plan=(("vec", 0), ("direct", int(routes[i % 4] == "both")), ("G", 256 // F if F < 256 else 1))))
        add(case("bwd", 65, F, "exact", relu=1, plan=(("vec", 0), ("direct", 1))))
    for F in (4, 64, 1024):
        for j, fam in enumerate(("gauss", "exact", "const" if F >= 8 else "offset")):
            add(case("bwd", 4096, F, fam, relu=j % 2, dx_beta=(0.0, 1.0, 0.5)[j], route=routes[j],
                     plan=(("vec", 1), ("direct", int(j == 0)), ("rows_per_block", 0), ("blocks", min(1024, 4096 * F // 1024)),
                           ("apply_grid", min(4096, 4096 * F // 1024)))))
    add(case("bwd", 4096, 64, "gauss", relu=1, route="misaligned", dx_beta=1.0, plan=(("vec", 1), ("direct", 0))))
    add(case("bwd", 4096, 12, "gauss", relu=1, plan=(("vec", 0), ("direct", 1), ("blocks", 64))))           # F does not divide 1024
    add(case("bwd", 4096, 12, "exact", route="none", plan=(("vec", 0), ("direct", 0))))
    add(case("bwd", 4096, 64, "gauss", relu=1, misalign="x", plan=(("vec", 0), ("direct", 1))))           # scalar kernels at rows >= 4096
    add(case("bwd", 4096, 64, "exact", misalign="dy", dx_beta=1.0, plan=(("vec", 0),)))
    add(case("bwd", 4096, 64, "gauss", scratch=("rows", 5), relu=1, plan=(("vec", 1), ("blocks", 5))))     # vb capped by the scratch
    add(case("bwd", 4096, 64, "exact", scratch=("rows", 1), route="none", plan=(("vec", 1), ("blocks", 1))))
    add(case("bwd", 1000, 80, "gauss", scratch=("rows", 3), relu=1, route="none", plan=(("vec", 0), ("blocks", 3), ("rows_per_block", 334))))
    add(case("bwd", 1000, 80, "gauss", scratch="short", plan=(("err", ARG),)))
    add(case("bwd", 4096, 64, "gauss", scratch="short", plan=(("err", ARG),)))
    add(case("bwd", 65, 6, "gauss", relu=1, dx_beta=1.0, plan=(("vec", 0), ("G", 42))))                    # no F % 4 rule in the scalar kernels
    add(case("bwd", 65, 80, "gauss", dx=False, plan=(("apply_grid", 0), ("direct", 1))))
    add(case("bwd", 4096, 64, "gauss", dx=False, relu=1, route="one", plan=(("apply_grid", 0), ("vec", 1), ("direct", 0))))
    add(case("bwd", 65, 80, "exact", dx=False, route="one", relu=1, plan=(("apply_grid", 0), ("vec", 0), ("direct", 0))))
    add(case("bwd", 4096, 64, "exact", dx=False, plan=(("apply_grid", 0), ("vec", 1), ("direct", 1))))
    add(case("bwd", 131073, 4, "exact", route="none", misalign="dy", plan=(("rows_per_block", 65), ("vec", 0))))
    # sync forms
    for F in (4, 80, 260):
        for fam in ("gauss", "exact", "const" if F >= 8 else "offset"):
            add(case("sync", 128, F, fam, shards=(37, 91), relu=int(fam == "gauss")))
    add(case("sync", 1000, 80, "gauss", shards=(1, 999), scratch=("rows", 3), plan=(("blocks", 1),)))
    add(case("sync", 1000, 80, "gauss", shards=(600, 400), scratch="short", plan=(("err", ARG),)))
    for F in (6, 80, 260):
        for fam in ("gauss", "exact"):
            add(case("moments", 256, F, fam, scratch=("rows", 1), plan=(("blocks", 1), ("rows_per_block", 256))))
            add(case("moments", 197, F, fam, plan=(("blocks", 4),)))
    add(case("moments", 256, 80, "offset", scratch=("rows", 2), plan=(("blocks", 2),)))
    add(case("moments", 256, 80, "gauss", scratch="short", plan=(("err", ARG),)))
    # partial-row forms
    i = 0
    for C in (4, 12, 20, 64, 132):
        for nparts in (1, 63, 64, 65, 512):
            i += 1
            add(case("finalize", (4099, 5, 2, 1)[i % 4], C, fams[i % 3], nparts=nparts, bessel=i % 2, affine=i % 3 != 0, moving=("both", "none")[i % 5 == 0]))
        add(case("finalize", 4099, C, "exact", nparts=65, bessel=1))
        add(case("finalize", 197, C, "offset", nparts=64, bessel=0, negvar=C >= 4))
    for count in (1, 2, 5, 4099):
        for bessel in (0, 1):
            add(case("finalize", count, 12, "gauss", nparts=3, bessel=bessel, momentum=0.0))
    add(case("finalize", 197, 12, "gauss", nparts=3, bessel=1, negvar=True))
    add(case("finalize", 197, 12, "gauss", nparts=3, bessel=0, moving="one"))             # refused
    add(case("finalize", 197, 12, "gauss", nparts=3, bessel=1, moving="one"))
    add(case("fwd", 65, 8, "gauss", moving="one"))
    for C in (4, 68):
        add(case("eval_affine", 1, C))
    i = 0
    for C in (4, 12, 80, 1024):
        RL = 256 // (C // 4)
        for rows in (1, 8 * RL - 1, 8 * RL, 8 * RL + 1, 512 * 8 * RL + 1):        # the last: rows per block grow past 8 * RL
            i += 1
            per = max(8 * RL, -(-rows // 512))
            add(case("stage1", rows, C, ("exact", "gauss")[i % 2], mask=("lazy", "y")[(i // 2) % 2], alias=i % 3 == 0,
                     plan=(("G", RL), ("rows_per_block", per), ("blocks", -(-rows // per)))))
    add(case("stage1", 512 * 8 * 12 + 100, 80, "exact", mask="lazy", plan=(("rows_per_block", 97), ("blocks", 508))))
    add(case("stage1", 9, 1028, "gauss", plan=(("err", ARG),)))
    add(case("stage1", 9, 6, "gauss", plan=(("err", ARG),)))
    for C in (4, 20, 132):
        for nparts in (1, 65, 512):
            add(case("bwd_finalize", 197, C, "gauss" if nparts != 65 else "offset", nparts=nparts, grad_beta=float(nparts == 65), grads=nparts != 512))
        add(case("bwd_finalize", 128, C, "gauss", nparts=3, shards=(37, 91), grad_beta=1.0))
        add(case("bwd_finalize", 128, C, "exact", nparts=3, grad_beta=0.0))
    for beta in (0.0, 1.0, 0.5):
        add(case("bwd_apply", 5, 12, "gauss", beta=beta, plan=(("apply_grid", 1),)))
        add(case("bwd_apply", 4099, 12, "gauss", beta=beta, plan=(("apply_grid", 7),)))       # seven grid-stride passes of seven blocks
    add(case("bwd_apply", 65, 12, "exact", beta=1.0, plan=(("apply_grid", 1),)))
    add(case("bwd_apply", 5, 6, "gauss", plan=(("err", ARG),)))
    # instance norm
    i = 0
    for Bn in (1, 3):
        for T_ in (1, 3, 4, 5, 9):
            for F in (4, 39, 64, 68, 132):
                i += 1
                add(case("instnorm", T_, F, fams[i % 4], B=Bn, alias=i % 2 == 0))
    return T


CASES = _table()


def measure(cases=None):
    """The fp32 twin's worst err / mag per kind over the table: what T_VEC and T_MAP are 8 x of."""
    worst = {"vec": 0.0, "map": 0.0}
    for c in cases or CASES:
        p = build(c)
        for q in p.q.values():
            if q.kind in worst and q.noise is not None:
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = np.where(q.mag > 0, q.noise / q.mag, 0.0)
                worst[q.kind] = max(worst[q.kind], float(r.max()) if r.size else 0.0)
    return worst

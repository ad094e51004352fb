"""Inputs, fp64 reference and checker for the conformance suite of the lip-CNN convolutions (csrc/conv_mfma.hip, conv_wgrad.hip,
conv_direct.hip, conv.hip), TensorFlow SAME geometry on NHWC maps:

    fwd         y  = conv(xin, w) + bias + res'            xin = relu(x*sc + sh) under the BN-ReLU loader, res' = res or relu(res*rsc + rsh)
                stats[j] = (sum y | sum y^2) over the frames of workgroup j, per destination channel
    bwd_data    dx = conv_transpose(dy, w) + beta*old      old = acc, or what dx held
                bnb: dz = dx * [bn_x*sc + sh > 0] is written instead, stats[j] = (sum dz | sum dz*bn_x)
    bwd_weight  dw = sum xin (x) dy + beta*dw,  db = sum dy + beta*db
                fold: dy = k1*dz + k2*y + k3 per destination channel, evaluated in the fetch (fold == 2: also stored as dx_out)

A `Case` holds every knob of one call; `build(case)` makes the operand and output buffers (numpy fp32, bands included), and the fp64
expectation (torch fp64 conv2d with autograd for the gradients); `check(problem, outputs)` judges what a kernel left in the buffers;
`run(case, torch, ops)` drives the library.

Poison.  Every operand sits at offset BAND (a multiple of 4 floats: the kernels use 16-byte loads) of a buffer whose other floats are NaN:
one stray element in an accumulator shows.  Every output sits between bands of SENTINEL, compared bit for bit afterwards; its own floats
are NaN where the call must not read them (beta == 0).  The statistics buffer is SENTINEL throughout: after the call rows [0, n) must be
finite and everything beyond untouched.  The weight gradient's scratch is followed by a SENTINEL band too.

Families.
  exact   operands non-zero integers of magnitude <= 3 (<= 2, 1 where the sums are long), scales +-1 / 2, shifts, bias, k3, old values
          small integers (even where beta == 0.5): for every output element the sum of the absolute values of its terms is below 2^24 --
          asserted from the reference --, so every partial sum in any order is an integer fp32 holds and the result is compared with
          np.array_equal.  A statistics row sums the frames of one workgroup; the checker adds the n rows in fp64, compares with the exact
          total and asserts ceil(N / n) * (max over frames and channels of sum |term|) < 2^24.
  mant_s  the source operand (x; dy for the data gradient) holds odd integers with 12 significant bits, the other operand |v| <= 3
  mant_o  the other way round (w; dy for the weight gradient).  Same 2^24 condition; no statistics.  A path that rounds an operand to
          bf16 or to 11 bits changes the answer.
  gauss   standard normal; per element |err| <= gamma_n * sum |terms|, gamma_n = n u / (1 - n u), u = 2^-24, n = roundings on the longest path:
            data path      taps*Cs + 4 (tap-group launches, at most) + 3 (bias, residual / mask map, beta*old) + 2 (an fma loader)
            weight grad    N*Ho*Wo + min(N, 1024) (partial rows) + 2 (+ 3 under fold: the two fmas of the fetch), column sums alike
            statistics     the rows' elements carry their own bound; adding m of them costs gamma_(m+2) * sum |element| more
          only where the depth (taps*Cs, N*Ho*Wo) is at most GAUSS_DEPTH_MAX: the bound grows as depth^2, a reduced-precision operand's
          error as sqrt(depth); tests/test_conv_check_cpu.py verifies that an operand rounded to 11 bits is still rejected at the cap.
          The ReLU masks (loader, residual, bnb) are taken exactly: the sign of the fp32 fma is the sign of the exact value.

numpy and CPU torch only; `run` takes the torch and ops modules of the caller."""
import dataclasses
import typing

import numpy as np
import torch

U = 2.0 ** -24
SENTINEL = np.uint32(0x7FEDBEEF)      # a NaN with a payload: nothing computes it
BAND = 256                            # floats of poison before and after every operand and output
GAUSS_DEPTH_MAX = 256
STATS_ROWS = 512                      # the statistics buffers hold 512 partial rows (include/avsr_hip.h)
LIMIT = float(1 << 24)


class ConvMismatch(AssertionError):
    pass


@dataclasses.dataclass(frozen=True)
class Case:
    op: str                           # fwd | bwd_data | bwd_weight
    N: int
    H: int
    W: int
    Ci: int
    Co: int
    k: int = 3
    stride: int = 1
    door: str = "desc"                # desc | direct | im2col
    bn: bool = False                  # BN-ReLU loader on x (fwd, bwd_weight)
    res: str = "none"                 # none | plain | lazy (fwd)
    stats: bool = False               # fwd
    bias: bool = False                # fwd
    beta: float = 0.0                 # bwd_data, bwd_weight
    acc: bool = False                 # bwd_data: beta multiplies a separate map
    bnb: bool = False                 # bwd_data: batch-norm-backward epilogue
    fold: int = 0                     # bwd_weight: 1 = dy evaluated in the fetch, 2 = and stored
    dbias: bool = False               # bwd_weight
    scratch_slabs: typing.Optional[int] = None      # bwd_weight: scratch of this many slabs of the first launch (None = ample)
    deferred: bool = False            # bwd_weight inside slab_defer_begin / _end
    family: str = "exact"
    seed: int = 0

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


def same(n, k, s):
    """TF SAME: (outputs, pad before)."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2


def geometry(c):
    Ho, pt = same(c.H, c.k, c.stride)
    Wo, pl = same(c.W, c.k, c.stride)
    return Ho, Wo, pt, pl


def conv64(x, w, b, s):
    """x [N,H,W,C] float64, w [k,k,Ci,Co]: TF conv2d(padding='SAME')."""
    k = w.shape[0]
    _, pt = same(x.shape[1], k, s)
    _, pl = same(x.shape[2], k, s)
    Ho, Wo = -(-x.shape[1] // s), -(-x.shape[2] // s)
    pb, pr = max((Ho - 1) * s + k - x.shape[1], 0) - pt, max((Wo - 1) * s + k - x.shape[2], 0) - pl
    xt = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return torch.nn.functional.conv2d(xt, w.permute(3, 2, 0, 1), b, stride=s).permute(0, 2, 3, 1)


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def conv_data_grad(dy, w, xshape, s):
    x = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
    (conv64(x, _t(w), None, s) * _t(dy)).sum().backward()
    return x.grad.numpy()


def conv_weight_grad(xin, dy, k, s):
    w = torch.zeros((k, k, xin.shape[3], dy.shape[3]), dtype=torch.float64, requires_grad=True)
    (conv64(_t(xin), w, None, s) * _t(dy)).sum().backward()
    return w.grad.numpy()


def gamma(n):
    return n * U / (1.0 - n * U)


def _ints(rng, amax, shape):
    return (rng.integers(1, amax + 1, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float32)


def _mant(rng, shape):
    return ((2 * rng.integers(1 << 10, 1 << 11, size=shape) + 1) * rng.choice([-1, 1], size=shape)).astype(np.float32)   # odd, 12 bits


def _small(rng, amax, shape, even=False):
    v = rng.integers(-amax, amax + 1, size=shape)
    return (2 * v if even else v).astype(np.float32)


def _scales(rng, n):
    return rng.choice(np.array([1.0, 2.0, -1.0, 1.0], np.float32), size=n)


class Problem:
    pass


def _poisoned(v):
    buf = np.full(v.size + 2 * BAND, np.nan, np.float32)
    buf[BAND:BAND + v.size] = v.reshape(-1)
    return buf


def _guarded(shape, old):
    n = int(np.prod(shape))
    buf = np.full(n + 2 * BAND, SENTINEL, np.uint32).view(np.float32)
    buf[BAND:BAND + n] = np.nan if old is None else old.reshape(-1)
    return buf


def _amax(c, Ho, Wo):
    """Largest operand magnitude of the exact family (3, 2, 1) whose ESTIMATED longest sum stays well inside 2^24 (build asserts the real ones)."""
    Cs = c.Co if c.op == "bwd_data" else c.Ci
    depth = c.k * c.k * Cs
    for a in (3, 2, 1):
        m2 = {3: 14.0 / 3, 2: 2.5, 1: 1.0}[a]           # mean square of a non-zero integer in [-a, a]
        sh, sw = (Ho, Wo) if c.op == "bwd_data" else (c.H, c.W)
        frames = max(-(-c.N // STATS_ROWS), min(c.N, 16, max(1, 16128 // ((sh + 2) * (sw + 2) * ((Cs + 3) & ~3)))))
        if c.op == "bwd_weight":
            dymax = a if not c.fold else 4 * a + 3
            worst = c.N * Ho * Wo * (2 * a + 3 if c.bn else a) * dymax
        elif c.stats or c.bnb:
            px = Ho * Wo if c.op == "fwd" else c.H * c.W
            worst = 2.0 * frames * px * (depth * m2 * m2 * (5 if c.bn else 1) + 40) * (3 * a if c.bnb else 1)
        else:
            worst = depth * a * a * 8
        if worst < LIMIT / 2:
            return a
    return 1


def build(case):
    c = case
    assert c.op in ("fwd", "bwd_data", "bwd_weight") and c.door in ("desc", "direct", "im2col")
    assert c.family in ("exact", "mant_s", "mant_o", "gauss") and c.res in ("none", "plain", "lazy") and c.fold in (0, 1, 2)
    assert c.op == "fwd" or (c.res == "none" and not c.stats and not c.bias)
    assert c.op == "bwd_data" or (not c.acc and not c.bnb)
    assert c.op == "bwd_weight" or (not c.fold and not c.dbias and c.scratch_slabs is None and not c.deferred)
    assert c.op != "fwd" or c.beta == 0.0
    assert not c.acc or c.beta != 0.0
    Ho, Wo, pt, pl = geometry(c)
    N, H, W, Ci, Co, k, s = c.N, c.H, c.W, c.Ci, c.Co, c.k, c.stride
    rng = np.random.default_rng([c.seed, N, H, W, Ci, Co, k, s, {"fwd": 0, "bwd_data": 1, "bwd_weight": 2}[c.op]])
    exact = c.family != "gauss"
    p = Problem()
    p.case, p.Ho, p.Wo, p.pt, p.pl = c, Ho, Wo, pt, pl
    xs, ys, ws = (N, H, W, Ci), (N, Ho, Wo, Co), (k, k, Ci, Co)
    depth = k * k * (Co if c.op == "bwd_data" else Ci) if c.op != "bwd_weight" else N * Ho * Wo
    p.depth = depth
    if c.family == "gauss":
        assert depth <= GAUSS_DEPTH_MAX, "the gauss family only guards accumulation precision at small depth"
        draw = lambda shape: rng.standard_normal(shape).astype(np.float32)
        src = oth = draw
        small = lambda shape, even=False: rng.standard_normal(shape).astype(np.float32)
        scales = lambda n: rng.uniform(0.5, 1.5, n).astype(np.float32) * rng.choice(np.array([1, 1, 1, -1], np.float32), size=n)
    else:
        assert c.beta in (0.0, 1.0, 2.0, 0.5)
        a = _amax(c, Ho, Wo) if c.family == "exact" else 3
        p.amax = a
        src = (lambda shape: _mant(rng, shape)) if c.family == "mant_s" else (lambda shape: _ints(rng, a, shape))
        oth = (lambda shape: _mant(rng, shape)) if c.family == "mant_o" else (lambda shape: _ints(rng, a, shape))
        small = lambda shape, even=False: _small(rng, 3, shape, even)
        scales = lambda n: _scales(rng, n)
        assert c.family == "exact" or not (c.stats or c.bnb or c.fold or c.bn), "the mantissa families keep to the plain product"
    v = {}                                               # operand values, fp32
    old = {}                                             # what the outputs hold before the call (None: NaN, must not be read)
    exp, mag, nr = {}, {}, {}
    even = c.beta == 0.5
    f64 = lambda a_: np.asarray(a_, np.float64)
    if c.op == "fwd":
        v["x"], v["w"] = src(xs), oth(ws)
        if c.bias:
            v["bias"] = small(Co)
        if c.bn:
            v["bn_sc"], v["bn_sh"] = scales(Ci), small(Ci)
        xin = np.maximum(f64(v["x"]) * v["bn_sc"] + v["bn_sh"], 0.0) if c.bn else f64(v["x"])
        y = conv64(_t(xin), _t(v["w"]), _t(v["bias"]) if c.bias else None, s).numpy()
        m = conv64(_t(np.abs(xin)), _t(np.abs(v["w"])), _t(np.abs(v["bias"])) if c.bias else None, s).numpy()
        if c.res != "none":
            v["res"] = small(ys) if exact else rng.standard_normal(ys).astype(np.float32)
            r = f64(v["res"])
            if c.res == "lazy":
                v["res_sc"], v["res_sh"] = scales(Co), small(Co)
                r = np.maximum(r * v["res_sc"] + v["res_sh"], 0.0)
            y, m = y + r, m + np.abs(r)
        old["y"] = None
        exp["y"], mag["y"], nr["y"] = y, m, depth + 9
        if c.stats:
            p.stat_C = Co
            p.stat_terms = (np.abs(y), y * y)
            p.stat_bound = (gamma(nr["y"]) * m, None)
    elif c.op == "bwd_data":
        v["dy"], v["w"] = src(ys), oth(ws)
        dx = conv_data_grad(v["dy"], v["w"], xs, s)
        m = conv_data_grad(np.abs(v["dy"]), np.abs(v["w"]), xs, s)
        if c.beta != 0.0:
            o = small(xs, even)
            if c.acc:
                v["acc"], old["dx"] = o, None
            else:
                old["dx"] = o
            dx, m = dx + c.beta * f64(o), m + np.abs(c.beta * f64(o))
        else:
            old["dx"] = None
        nr["dx"] = depth + 9
        if c.bnb:
            v["bn_x"], v["bnb_sc"], v["bnb_sh"] = (small(xs) if exact else rng.standard_normal(xs).astype(np.float32)), scales(Ci), small(Ci)
            mask = f64(v["bn_x"]) * v["bnb_sc"] + v["bnb_sh"] > 0
            dx, m = dx * mask, m * mask
            p.stat_C = Ci
            p.stat_terms = (np.abs(dx), np.abs(dx * f64(v["bn_x"])))
            p.stat_bound = (gamma(nr["dx"]) * m, gamma(nr["dx"] + 1) * m * np.abs(f64(v["bn_x"])))
            p.stat_exp = (dx.sum((0, 1, 2)), (dx * f64(v["bn_x"])).sum((0, 1, 2)))
        exp["dx"], mag["dx"] = dx, m
    else:
        v["x"] = src(xs)
        if c.bn:
            v["bn_sc"], v["bn_sh"] = scales(Ci), small(Ci)
        xin = np.maximum(f64(v["x"]) * v["bn_sc"] + v["bn_sh"], 0.0) if c.bn else f64(v["x"])
        nr["dw"] = nr["db"] = depth + min(N, 1024) + 2 + (3 if c.fold else 0) + (2 if c.beta else 0)
        if c.fold:
            v["dz"], v["y"] = oth(ys), oth(ys)
            v["fk"] = np.concatenate([scales(Co), scales(Co), small(Co)])
            k1, k2, k3 = f64(v["fk"][:Co]), f64(v["fk"][Co:2 * Co]), f64(v["fk"][2 * Co:])
            dy = k1 * f64(v["dz"]) + k2 * f64(v["y"]) + k3
            dym = np.abs(k1 * f64(v["dz"])) + np.abs(k2 * f64(v["y"])) + np.abs(k3)
            if c.fold == 2:
                old["dx_out"] = None
                exp["dx_out"], mag["dx_out"], nr["dx_out"] = dy, dym, 3
        else:
            v["dy"] = oth(ys)
            dy = dym = f64(v["dy"])
            dym = np.abs(dym)
        dw, m = conv_weight_grad(xin, dy, k, s), conv_weight_grad(np.abs(xin), dym, k, s)
        db, mb = dy.sum((0, 1, 2)), dym.sum((0, 1, 2))
        if c.beta != 0.0:
            old["dw"], old["db"] = small(ws, even), small(Co, even)
            dw, m = dw + c.beta * f64(old["dw"]), m + np.abs(c.beta * f64(old["dw"]))
            db, mb = db + c.beta * f64(old["db"]), mb + np.abs(c.beta * f64(old["db"]))
        else:
            old["dw"] = old["db"] = None
        exp["dw"], mag["dw"] = dw, m
        if c.dbias:
            exp["db"], mag["db"] = db, mb
        else:
            old.pop("db")
    if c.family != "gauss":
        # the 2^24 condition, from the reference: every element's terms sum (in absolute value) to an integer fp32 holds, in quanta of
        # `q` (beta == 0.5 halves even integers: still integers)
        for name in exp:
            assert float(mag[name].max()) < LIMIT, "%s: the %s family would round (sum |terms| up to %g)" % (name, c.family, mag[name].max())
            assert np.array_equal(exp[name], np.rint(exp[name])), "%s: the expectation is not integral" % name
    if c.op == "fwd" and c.stats:
        p.stat_exp = (exp["y"].sum((0, 1, 2)), (exp["y"] ** 2).sum((0, 1, 2)))
    p.val, p.exp, p.mag, p.nr = v, exp, mag, nr
    p.inputs = {name: _poisoned(a_) for name, a_ in v.items()}
    p.shapes = {name: tuple(np.shape(exp[name])) for name in exp}
    p.outputs = {name: _guarded(p.shapes[name], old[name]) for name in exp}
    p.old = old
    if c.stats or c.bnb:
        p.outputs["stats"] = np.full(STATS_ROWS * 2 * p.stat_C + 2 * BAND, SENTINEL, np.uint32).view(np.float32)
    return p


def operand(p, name):
    """The operand's fp32 values (the view a kernel is given), or None."""
    return p.val.get(name)


LABELS = {"y": "(frame, row, column, channel)", "dx": "(frame, row, column, channel)", "dx_out": "(frame, row, column, channel)",
          "dw": "(tap row, tap column, ci, co)", "db": "(co)"}


def _judge(name, exact, got, want, mag, n):
    got = got.astype(np.float64)
    if exact:
        if not np.array_equal(got, want):
            bad = np.argwhere(~(got == want))
            i = tuple(int(t) for t in bad[0])
            raise ConvMismatch("%s: %d element(s) differ from the exact result, first at %s = %s: got %r, want %r"
                               % (name, len(bad), LABELS.get(name, "index"), i, got[i], want[i]))
        return 0.0
    err = np.abs(got - want)
    bound = gamma(n) * mag
    ok = err <= bound                  # False for NaN
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(int(t) for t in bad[0])
        raise ConvMismatch("%s: %d element(s) outside the fp32 bound (n = %d), first at %s = %s: err %.3g, bound %.3g, err / bound %.3g"
                           % (name, len(bad), n, LABELS.get(name, "index"), i, err[i], bound[i], err[i] / bound[i] if bound[i] else np.inf))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


def _bands_intact(name, buf, lo, hi):
    bits = np.ascontiguousarray(buf).view(np.uint32)
    keep = np.ones(bits.size, bool)
    keep[lo:hi] = False
    bad = np.flatnonzero(keep & (bits != SENTINEL))
    if bad.size:
        raise ConvMismatch("%s: %d float(s) outside the call's output were written, first at %+d floats from its start"
                           % (name, bad.size, int(bad[0]) - lo))


def check(p, out):
    """Judge the buffers a kernel left behind (out: name -> the whole buffer, bands included; "n": the statistics rows it reported;
    "scratch_band": the band behind the scratch).  Returns the worst err / bound ratio (0.0 in the exact families)."""
    c = p.case
    exact = c.family != "gauss"
    worst = 0.0
    for name, want in p.exp.items():
        buf = np.asarray(out[name], np.float32).reshape(-1)
        assert buf.size == p.outputs[name].size
        _bands_intact(name, buf, BAND, BAND + want.size)
        got = buf[BAND:BAND + want.size].reshape(want.shape)
        worst = max(worst, _judge(name, exact, got, want, p.mag[name], p.nr[name]))
    if "scratch_band" in out:
        _bands_intact("scratch", np.asarray(out["scratch_band"], np.float32).reshape(-1), 0, 0)
    if "stats" in p.outputs:
        n, C2 = int(out["n"]), 2 * p.stat_C
        if not 0 < n <= min(STATS_ROWS, c.N):
            raise ConvMismatch("statistics: %d partial rows reported for %d frames" % (n, c.N))
        buf = np.asarray(out["stats"], np.float32).reshape(-1)
        _bands_intact("stats", buf, BAND, BAND + n * C2)
        rows = buf[BAND:BAND + n * C2].reshape(n, C2).astype(np.float64)
        if not np.isfinite(rows).all():
            r = int(np.argwhere(~np.isfinite(rows))[0][0])
            raise ConvMismatch("statistics: row %d of %d was not written" % (r, n))
        got = rows.sum(0)
        per_frame = [t.sum((1, 2)) for t in p.stat_terms]            # [N, C]
        for j, nm in enumerate(("first sums", "second sums")):
            g, w = got[j * p.stat_C:(j + 1) * p.stat_C], p.stat_exp[j]
            if exact:
                assert -(-c.N // n) * float(per_frame[j].max()) < LIMIT, \
                    "statistics %s: the case was built wrongly, a row of %d frames would round (%g per frame)" % (nm, -(-c.N // n), per_frame[j].max())
                if not np.array_equal(g, w):
                    ch = int(np.argwhere(g != w)[0][0])
                    raise ConvMismatch("statistics %s: channel %d: got %r, want %r (off by %r)" % (nm, ch, g[ch], w[ch], g[ch] - w[ch]))
            else:
                tot = p.stat_terms[j].sum((0, 1, 2))
                if j == 0 or c.bnb:
                    eb = p.stat_bound[j].sum((0, 1, 2))
                else:                                                # y^2 from an inexact y
                    b = p.stat_bound[0]
                    eb = (2 * p.stat_terms[0] * b + b * b).sum((0, 1, 2)) + gamma(2) * tot
                count = -(-c.N // n) * p.stat_terms[j].shape[1] * p.stat_terms[j].shape[2]
                bound = eb + gamma(count + 2) * tot
                err = np.abs(g - w)
                if not (err <= bound).all():
                    ch = int(np.argwhere(~(err <= bound))[0][0])
                    raise ConvMismatch("statistics %s: channel %d: err %.3g, bound %.3g" % (nm, ch, err[ch], bound[ch]))
                worst = max(worst, float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0).max()))
    return worst


# ---- driving the library (the torch and ops modules are the caller's) ----------------------------------------------------------------
PLAN_OP = {"fwd": "fwd", "bwd_data": "bwd_data", "bwd_weight": "bwd_weight"}


def plan_flags(c):
    """The flags of ops.conv_plan for this case's call."""
    f = []
    if c.op == "fwd":
        f += ["bias"] * c.bias + ["res"] * (c.res != "none") + ["stats"] * c.stats
    elif c.op == "bwd_data":
        f += ["beta"] * (c.beta != 0) + ["acc"] * c.acc + ["bnb"] * c.bnb
    else:
        f += ["beta"] * (c.beta != 0) + ["dbias"] * c.dbias + ["fold"] * (c.fold > 0) + ["fold_dx"] * (c.fold == 2)
    return f


def desc(c, ops, bn=None):
    Ho, Wo, pt, pl = geometry(c)
    d = ops.conv_desc(c.N, c.H, c.W, c.Ci, c.Co, c.k, c.stride, pt if c.k == 3 else 0, pl if c.k == 3 else 0, Ho, Wo, bn=bn)
    if bn is None and c.bn:
        d.bn_scale = d.bn_shift = 64                    # any non-NULL address: the plan query dereferences nothing
    return d


def plan(c, ops, scratch_floats=1 << 40):
    """The launches of this case's descriptor call (ops.conv_plan); with scratch_slabs, on the scratch `run` would pass."""
    d = desc(c, ops)
    launches = ops.conv_plan(d, c.op, plan_flags(c), scratch_floats)
    if c.op == "bwd_weight" and c.scratch_slabs is not None:
        launches = ops.conv_plan(d, c.op, plan_flags(c), scratch_floats_of(c, launches))
    return launches


def scratch_floats_of(c, ample_launches):
    if c.scratch_slabs is None:
        slab = max(12 * c.Ci * 16 + 16, c.k * c.k * c.Ci * c.Co + c.Co)
        return min(c.N, 1024) * slab * (2 if c.deferred else 1)
    return c.scratch_slabs * max(L["slab"] for L in ample_launches)


def run(case, torch_, ops, problem=None):
    """Build the case (or take `problem`), run it through the library and return (problem, outputs) for `check`."""
    c = case
    p = problem if problem is not None else build(c)
    Ho, Wo, pt, pl = p.Ho, p.Wo, p.pt, p.pl
    N, H, W, Ci, Co, k, s = c.N, c.H, c.W, c.Ci, c.Co, c.k, c.stride
    dev = {name: torch_.from_numpy(b.copy()).cuda() for name, b in p.inputs.items()}
    outb = {name: torch_.from_numpy(b.copy()).cuda() for name, b in p.outputs.items()}
    I = lambda name: dev[name][BAND:BAND + p.val[name].size] if name in dev else None
    O = lambda name: outb[name][BAND:BAND + int(np.prod(p.shapes[name]))] if name in p.shapes else None
    res = {}
    if c.door == "desc":
        d = desc(c, ops, bn=(I("bn_sc"), I("bn_sh")) if c.bn else None)
        stats = outb["stats"][BAND:BAND + STATS_ROWS * 2 * p.stat_C] if "stats" in outb else None
        if c.op == "fwd":
            n = ops.conv_fwd(d, I("x"), I("w"), I("bias"), O("y"), I("res"), (I("res_sc"), I("res_sh")) if c.res == "lazy" else None, stats)
            res["n"] = n
        elif c.op == "bwd_data":
            if c.acc or c.bnb:
                res["n"] = ops.conv_bwd_data_bn(d, I("dy"), I("w"), O("dx"), beta=c.beta, acc=I("acc"), bn_x=I("bn_x"),
                                                bn=(I("bnb_sc"), I("bnb_sh")) if c.bnb else None, stats=stats)
            else:
                ops.conv_bwd_data(d, I("dy"), I("w"), O("dx"), beta=c.beta)
        else:
            ample = ops.conv_plan(desc(c, ops), c.op, plan_flags(c))
            nfl = scratch_floats_of(c, ample)
            sbuf = torch_.from_numpy(np.full(nfl + BAND, SENTINEL, np.uint32).view(np.float32)).cuda()
            scratch = sbuf[:nfl]
            if c.deferred:
                ops.slab_defer_begin()
            try:
                if c.fold:
                    ops.conv_bwd_weight_bn(d, I("x"), I("dz"), I("y"), I("fk"), O("dw"), O("db"), scratch, beta=c.beta, dx_out=O("dx_out"))
                else:
                    ops.conv_bwd_weight(d, I("x"), I("dy"), O("dw"), O("db"), scratch, beta=c.beta)
            finally:
                if c.deferred:
                    ops.slab_defer_end()
            torch_.cuda.synchronize()
            res["scratch_band"] = sbuf[nfl:].cpu().numpy()
    elif c.door == "direct":
        assert k == 3 and not (c.bn or c.res != "none" or c.stats or c.acc or c.bnb or c.fold or c.dbias)
        if c.op == "fwd":
            ops.conv3x3(I("x"), I("w"), I("bias"), O("y"), N, H, W, Ci, Co, s, pt, pl, Ho, Wo)
        elif c.op == "bwd_data" and s == 1:
            ops.conv3x3(I("dy"), I("w"), None, O("dx"), N, Ho, Wo, Co, Ci, 1, 1, 1, H, W, flip=1, beta=c.beta)
        elif c.op == "bwd_data":
            ops.conv3x3_bwd_data_s2(I("dy"), I("w"), O("dx"), N, H, W, Ci, Co, pt, pl, Ho, Wo, beta=c.beta)
        else:
            nfl = 1 << 20
            sbuf = torch_.from_numpy(np.full(nfl + BAND, SENTINEL, np.uint32).view(np.float32)).cuda()
            ops.conv3x3_bwd_weight(I("x"), I("dy"), O("dw"), N, H, W, Ci, Co, s, pt, pl, Ho, Wo, sbuf[:nfl], beta=c.beta)
            torch_.cuda.synchronize()
            res["scratch_band"] = sbuf[nfl:].cpu().numpy()
    else:
        assert not (c.bn or c.res != "none" or c.stats or c.acc or c.bnb or c.fold or c.dbias)
        rows, K = N * Ho * Wo, k * k * Ci
        nan = lambda n: torch_.full((n,), float("nan"), device="cuda")
        if c.op == "fwd":
            col = nan(rows * K)
            ops.im2col(I("x"), col, N, H, W, Ci, k, k, s, pt, pl, Ho, Wo)
            ops.gemm(ops.mat(col, K), ops.mat(I("w"), Co), ops.mat(O("y"), Co), rows, Co, K, bias=I("bias"), splitk=1)
        elif c.op == "bwd_data":
            dcol = nan(rows * K)
            ops.gemm(ops.mat(I("dy"), Co), ops.mat(I("w"), Co), ops.mat(dcol, K), rows, K, Co, trans_b=1, splitk=1)
            ops.col2im(dcol, O("dx"), N, H, W, Ci, k, k, s, pt, pl, Ho, Wo, beta=c.beta)
        else:
            col = nan(rows * K)
            ops.im2col(I("x"), col, N, H, W, Ci, k, k, s, pt, pl, Ho, Wo)
            ops.gemm(ops.mat(col, K), ops.mat(I("dy"), Co), ops.mat(O("dw"), Co), K, Co, rows, trans_a=1, beta=c.beta, splitk=1)
    torch_.cuda.synchronize()
    for name, b in outb.items():
        res[name] = b.cpu().numpy()
    return p, res


# ---- the kernels' instantiations, as avsr_conv_plan reports them -----------------------------------------------------------------------
def inst_name(L):
    """The template instantiation of one avsr_conv_launch record, as the launch code spells it."""
    b = lambda x: "true" if x else "false"
    if L["kernel"] == 0:
        return "conv_gen_kernel<%d,%s,%d>" % (L["m"], b(L["ch4"]), L["ep"])
    if L["kernel"] == 1:
        return "conv_q4_kernel<%d,%d,%s,%d>" % (L["m"], L["ntc"], b(L["ch4"]), L["ep"])
    return "conv_wgrad_kernel<%d,%d,%s,%s,%d>" % (L["m"], L["ntc"], b(L["ch4"]), b(L["rs"]), L["fold"])


# every instantiation cg_launch, cg_launch_q4 and conv_bwd_weight_impl name
NAMED = sorted(set(
    ["conv_gen_kernel<5,false,0>"] + ["conv_gen_kernel<%d,true,%d>" % (m, e) for m in (2, 6, 9, 18, 20) for e in range(4)]
    + ["conv_q4_kernel<9,1,false,0>"] + ["conv_q4_kernel<9,2,true,%d>" % e for e in range(4)]
    + ["conv_wgrad_kernel<3,1,false,false,%d>" % f for f in range(3)] + ["conv_wgrad_kernel<6,1,true,false,%d>" % f for f in range(3)]
    + ["conv_wgrad_kernel<%d,%d,true,false,0>" % (m, n) for m in (5, 9, 18) for n in (1, 2)]
    + ["conv_wgrad_kernel<%d,4,true,false,0>" % m for m in (5, 9)] + ["conv_wgrad_kernel<%d,4,true,true,0>" % m for m in (5, 9)]
    + ["conv_wgrad_kernel<5,4,true,true,%d>" % f for f in (1, 2)] + ["conv_wgrad_kernel<5,1,true,false,%d>" % f for f in (1, 2)]
    + ["conv_wgrad_kernel<9,2,true,false,%d>" % f for f in (1, 2)]))


# ---- sweeping the dispatch (no GPU): tools/conv_plan_sweep.py writes profiles/conv_plan_sweep.txt with it, test_conv_check_cpu.py re-checks it ----
SWEEP_CI = (1, 2, 3, 4, 8, 12, 16, 20, 32, 48, 64)
SWEEP_CO = tuple(range(4, 65, 4))
SWEEP_N = (1, 3, 600, 4800)
SWEEP_SMALL = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 18, 35, 36, 40)
PLAN_BITS = {"bias": 1, "res": 2, "stats": 4, "beta": 8, "acc": 16, "bnb": 32, "fold": 64, "fold_dx": 128, "dbias": 256}
# every flag combination the API accepts, per op; and one set per EP / FOLD value
SWEEP_ALL_FLAGS = {0: [a + b + c for a in (0, 1) for b in (0, 2) for c in (0, 4)], 1: [a + b + c for a in (0, 8) for b in (0, 16) for c in (0, 32)],
                   2: [b + d + f for b in (0, 8) for d in (0, 256) for f in (0, 64, 192)]}
SWEEP_KEY_FLAGS = {0: [0, 2], 1: [0, 8, 32, 8 + 16 + 32], 2: [0, 64, 192 + 256 + 8]}


def plan_sweep(args):
    """avsr_conv_plan over every descriptor of one Ci: args = (Ci, hw values, Co values, N values, all_flags_everywhere).
    Returns ({instantiation: (size, witness)}, planned calls, disagreements of the *_supported queries with the plan)."""
    import ctypes as C
    import itertools
    from avsr_tf1_amd import _lib
    Ci, hw, cos, ns, everywhere = args
    lib = _lib.load()
    out = (_lib.ConvLaunch * 16)()
    fields = [f for f, _ in _lib.ConvLaunch._fields_]
    found, calls, disagree = {}, 0, []
    small = set(SWEEP_SMALL)

    def note(n, wit):
        for i in range(min(n, 16)):
            name = inst_name({f: getattr(out[i], f) for f in fields})
            size = (wit[3] * wit[4] * wit[5] * (wit[6] + wit[7]), wit)
            if name not in found or size < found[name]:
                found[name] = size

    for H, W, Co, k, s in itertools.product(hw, hw, cos, (1, 3), (1, 2)):
        Ho, pt = same(H, k, s)
        Wo, pl = same(W, k, s)
        full = everywhere or (H in small and W in small)
        for N in ns:
            for bn in (0, 1):
                d = _lib.ConvDesc(N, H, W, Ci, Co, k, s, pt if k == 3 else 0, pl if k == 3 else 0, Ho, Wo, 0, 64 if bn else None, 64 if bn else None)
                ok = {}
                for op in (0, 1, 2):
                    for fl in (SWEEP_ALL_FLAGS if full and N == 3 else SWEEP_KEY_FLAGS)[op]:
                        n = lib.avsr_conv_plan(C.byref(d), op, fl, 1 << 40, out, 16)
                        calls += 1
                        ok[op, fl] = n > 0
                        if n <= 0:
                            continue
                        note(n, (op, fl, bn, N, H, W, Ci, Co, k, s, 0))
                        if op == 2:
                            slab = max(out[i].slab for i in range(n))
                            n1 = lib.avsr_conv_plan(C.byref(d), op, fl, slab, out, 16)
                            calls += 1
                            if n1 > 0:
                                note(n1, (op, fl, bn, N, H, W, Ci, Co, k, s, 1))
                # the three queries answer what the plan answers (they run the same dry paths with these operands)
                want = (ok[0, 0] and (Ci < 4 or ok[1, 8]) and ok[2, 0], Ci >= 4 and ok[1, 8 + 16 + 32], ok[2, 64])
                got = (bool(lib.avsr_conv_supported(C.byref(d))), bool(lib.avsr_conv_bwd_data_bn_supported(C.byref(d))),
                       bool(lib.avsr_conv_bwd_weight_bn_supported(C.byref(d))))
                for q, (w_, g_) in enumerate(zip(want, got)):
                    if bool(w_) != g_:
                        disagree.append((q, bn, N, H, W, Ci, Co, k, s, bool(w_), g_))
    return found, calls, disagree


def merge_sweeps(parts):
    found, calls, disagree = {}, 0, []
    for f, n, dis in parts:
        calls += n
        disagree += dis
        for name, v in f.items():
            if name not in found or v < found[name]:
                found[name] = v
    return found, calls, disagree


def witness_line(name, wit):
    op, fl, bn, N, H, W, Ci, Co, k, s, slab = wit
    flags = "+".join(n for n, b in PLAN_BITS.items() if fl & b) or "-"
    return "%-40s op=%s flags=%s bn=%d N=%d H=%d W=%d Ci=%d Co=%d k=%d stride=%d scratch=%s" % (
        name, ("fwd", "bwd_data", "bwd_weight")[op], flags, bn, N, H, W, Ci, Co, k, s, "one_slab" if slab else "ample")


def parse_sweep_file(path):
    """(reachable: [(instantiation, witness dict)], named but unreachable: [instantiation]) of profiles/conv_plan_sweep.txt."""
    reach, unreach = [], []
    for line in open(path):
        t = line.split()
        if not t or t[0].startswith("#") or t[0] in ("reachable", "named_unreachable"):
            continue
        if len(t) == 1:
            unreach.append(t[0])
        else:
            reach.append((t[0], dict(kv.split("=", 1) for kv in t[1:])))
    return reach, unreach

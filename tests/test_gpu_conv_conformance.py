"""Conformance of the lip-CNN convolutions on the GPU: every case goes through tests/ref_conv.py -- poisoned operands, sentinel-guarded
outputs compared bit for bit, exact integer arithmetic with np.array_equal (families exact / mant_*), a derived fp32 bound on Gaussian
inputs (family gauss) -- and through the library's three doors (descriptor API, direct 3x3 kernels, im2col + GEMM).

The case table CASES is data: tests/test_conv_check_cpu.py plans every case with avsr_conv_plan (no GPU) and fails unless each reachable
kernel instantiation is run by an exact case and each regime below (grid cap, passes, scratch-limited grids, ...) is present according
to the plan.  Shapes are the smallest that reach a form; the only large cases are those that need more than 512 workgroups."""
import numpy as np
import pytest

import ref_conv as R
from ref_conv import Case

# (Ci, Co, k, stride): one per form of the kernels
FORMS = {
    "q4_8ch": (8, 8, 3, 1), "q4_3ch": (3, 8, 3, 1), "pair_16to8": (16, 8, 3, 1), "plain_1tile": (8, 16, 3, 1), "s2_4class": (8, 16, 3, 2),
    "s2_4class_16": (16, 32, 3, 2), "s2_per_class": (32, 64, 3, 2), "shortcut_8to16": (8, 16, 1, 2), "shortcut_16to32": (16, 32, 1, 2),
    "shortcut_4to4": (4, 4, 1, 2), "shortcut_64": (64, 64, 1, 2), "plain_2tiles": (32, 32, 3, 1), "tap_groups_64": (64, 64, 3, 1),
    "ci1": (1, 8, 3, 1), "ci2": (2, 4, 3, 1), "ci12to20": (12, 20, 3, 1), "ci20to12": (20, 12, 3, 1), "ci12to12": (12, 12, 3, 1), "ci20to20": (20, 20, 3, 2), "k1s1": (4, 4, 1, 1), "pair_52": (8, 52, 3, 1),
}
# H > W, H < W, 1 x W, H x 1, 1 x 1, the mixed pads at stride 2 (H odd beside W even and the reverse), odd widths beside the pixel-pair
# form, odd heights / widths under the four-class form (partial cells in the last row, the last column and the corner)
GEOMETRIES = [(5, 8), (8, 5), (1, 6), (6, 1), (1, 1), (7, 6), (6, 7), (7, 7), (9, 13)]
BETAS = (0.0, 1.0, 2.0, 0.5)


def _table():
    T = []
    add = lambda group, c: T.append((group, c))
    # ---- every form on every geometry, all three operations, the optional operands rotating ----
    i = 0
    for form, (Ci, Co, k, s) in FORMS.items():
        for (H, W) in GEOMETRIES:
            i += 1
            N = 5 if Ci < 4 else 3                      # frames of 9x13x3, 5x6x1, 5x5x2 floats then start at every alignment mod 4
            src_ok = Ci % 4 == 0
            add("forms", Case("fwd", N, H, W, Ci, Co, k, s, bias=i % 2 == 0, stats=i % 3 != 0, bn=src_ok and i % 4 == 1,
                              res=("none", "plain", "lazy")[i % 3] if src_ok else "none"))
            if src_ok:
                beta = BETAS[i % 4] if not (k == 1 and s == 2) else 1.0     # (no tap reaches three of the four pixel classes)
                add("forms", Case("bwd_data", N, H, W, Ci, Co, k, s, beta=beta))
            add("forms", Case("bwd_weight", N, H, W, Ci, Co, k, s, dbias=i % 2 == 1, beta=float(i % 2), bn=src_ok and i % 3 == 0))
    for Ci, Co in ((3, 8), (1, 8), (2, 4)):             # frame sizes that are no multiple of 4 floats
        for (H, W) in ((9, 13), (5, 6), (5, 5)):
            add("small_ci", Case("fwd", 6, H, W, Ci, Co, bias=True, stats=True))
            add("small_ci", Case("bwd_weight", 6, H, W, Ci, Co, dbias=True))
            add("small_ci", Case("bwd_weight", 6, H, W, Ci, Co, fold=1, beta=1.0))
    # ---- epilogues: every EP of every data-path form that can take it ----
    for form in ("q4_8ch", "pair_16to8", "plain_1tile", "plain_2tiles", "tap_groups_64", "k1s1", "pair_52", "ci12to20", "ci20to12"):
        Ci, Co, k, s = FORMS[form]
        for (H, W) in ((5, 6), (6, 5)):
            for res in ("plain", "lazy"):
                add("epilogues", Case("fwd", 4, H, W, Ci, Co, k, s, res=res, bias=True, stats=True, bn=res == "lazy"))
            add("epilogues", Case("fwd", 4, H, W, Ci, Co, k, s, stats=True))
            add("epilogues", Case("fwd", 4, H, W, Ci, Co, k, s, bias=True))
            for beta in BETAS:
                add("epilogues", Case("bwd_data", 4, H, W, Ci, Co, k, s, beta=beta))
                add("epilogues", Case("bwd_data", 4, H, W, Ci, Co, k, s, beta=beta, bnb=True))
                if beta:
                    add("epilogues", Case("bwd_data", 4, H, W, Ci, Co, k, s, beta=beta, acc=True))
                    add("epilogues", Case("bwd_data", 4, H, W, Ci, Co, k, s, beta=beta, acc=True, bnb=True))
    for form in ("s2_4class", "s2_4class_16"):           # the four-class stride-2 data gradient takes acc / bnb too
        Ci, Co, k, s = FORMS[form]
        for (H, W) in ((7, 6), (6, 7), (7, 7), (6, 6)):
            add("epilogues", Case("bwd_data", 4, H, W, Ci, Co, k, s, beta=0.5, acc=True, bnb=True))
            add("epilogues", Case("bwd_data", 4, H, W, Ci, Co, k, s, bnb=True))
            add("epilogues", Case("fwd", 4, H, W, Ci, Co, k, s, res="lazy", stats=True, bn=True))
    # ---- weight gradient: fold on each fold form, tap groups, the loader, deferred reductions ----
    for Ci, Co, k, s in ((8, 8, 3, 1), (3, 8, 3, 1), (8, 16, 3, 2), (4, 4, 1, 2), (4, 20, 1, 1), (16, 32, 3, 2), (20, 52, 3, 1), (32, 64, 3, 2),
                         (8, 8, 3, 2), (1, 8, 3, 1)):
        for (H, W) in ((5, 6), (6, 5), (7, 7)):
            for fold in (1, 2):
                add("wgrad", Case("bwd_weight", 4, H, W, Ci, Co, k, s, fold=fold, dbias=fold == 2, beta=float(fold - 1), bn=Ci % 4 == 0 and fold == 1))
    for Ci, Co in ((64, 16), (64, 32), (64, 64), (48, 52), (32, 64), (12, 52), (20, 4), (20, 20), (12, 4), (12, 20), (4, 52)):
        for k in (1, 3):
            add("wgrad", Case("bwd_weight", 4, 5, 6, Ci, Co, k, dbias=True))
            add("wgrad", Case("bwd_weight", 4, 6, 5, Ci, Co, k, beta=1.0, bn=True))
            add("wgrad", Case("bwd_weight", 4, 5, 6, Ci, Co, k, dbias=True, deferred=True))
    # ---- grid cap and passes (the plan decides; test_conv_check_cpu.py proves the regimes are here) ----
    for c in (Case("fwd", 515, 36, 36, 8, 8, bias=True, stats=True, res="plain"), Case("fwd", 515, 36, 36, 3, 8, bias=True, stats=True),
              Case("fwd", 515, 36, 36, 8, 16, stride=2, stats=True, bn=True), Case("bwd_data", 515, 36, 36, 8, 16, stride=2, beta=1.0, bnb=True),
              Case("bwd_data", 515, 36, 36, 8, 8, beta=0.5, acc=True),
              Case("fwd", 9192, 3, 3, 8, 16, stride=2, stats=True, bias=True), Case("bwd_data", 9192, 3, 3, 8, 16, stride=2, bnb=True),
              Case("fwd", 9192, 3, 4, 16, 8, stats=True), Case("fwd", 7, 5, 5, 16, 16, stats=True), Case("fwd", 3, 3, 3, 8, 16, stats=True),
              Case("bwd_weight", 9000, 2, 2, 8, 16, dbias=True), Case("bwd_weight", 4800, 2, 2, 16, 32, dbias=True, beta=1.0),
              Case("bwd_weight", 4800, 3, 4, 8, 8, dbias=True), Case("bwd_weight", 800, 36, 36, 8, 8, dbias=True),
              Case("bwd_weight", 515, 36, 36, 8, 8, dbias=True, fold=2),
              Case("bwd_weight", 5, 5, 6, 8, 16, scratch_slabs=1, dbias=True), Case("bwd_weight", 5, 5, 6, 8, 16, scratch_slabs=2, dbias=True),
              Case("bwd_weight", 5, 6, 6, 8, 8, scratch_slabs=2), Case("bwd_weight", 5, 5, 6, 64, 16, scratch_slabs=2, dbias=True),
              Case("bwd_weight", 7, 5, 6, 64, 64, scratch_slabs=1, dbias=True)):
        add("grid", c)
    # ---- a reduced-precision operand would show: 12-bit mantissas on the shortcuts (depth 4 .. 64) and on 3x3 with 8 channels ----
    for Ci, Co, k, s in ((4, 4, 1, 2), (8, 16, 1, 2), (16, 32, 1, 2), (64, 64, 1, 2), (8, 8, 3, 1), (8, 16, 3, 2), (16, 8, 3, 1), (3, 8, 3, 1)):
        for fam in ("mant_s", "mant_o"):
            add("mant", Case("fwd", 3, 6, 7, Ci, Co, k, s, family=fam, bias=True))
            if Ci % 4 == 0:
                add("mant", Case("bwd_data", 3, 6, 7, Ci, Co, k, s, family=fam, beta=1.0))
            add("mant", Case("bwd_weight", 3, 6, 7, Ci, Co, k, s, family=fam, dbias=True))
    # ---- Gaussian operands against the fp32 bound, where the depth cap allows ----
    for form, (Ci, Co, k, s) in FORMS.items():
        for (H, W) in ((5, 8), (7, 6)):
            src_ok = Ci % 4 == 0
            if k * k * Ci <= R.GAUSS_DEPTH_MAX:
                add("gauss", Case("fwd", 3, H, W, Ci, Co, k, s, family="gauss", bias=True, stats=True, bn=src_ok, res="lazy" if src_ok else "none"))
            if src_ok and k * k * Co <= R.GAUSS_DEPTH_MAX:
                add("gauss", Case("bwd_data", 3, H, W, Ci, Co, k, s, family="gauss", beta=1.0 if k == 1 and s == 2 else 0.5, acc=not (k == 1 and s == 2) and Ci <= 16,
                                  bnb=not (k == 1 and s == 2) and Ci <= 16))
            add("gauss", Case("bwd_weight", 3, H, W, Ci, Co, k, s, family="gauss", dbias=True, beta=1.0, bn=src_ok))
    for Ci, Co, k, s in ((8, 8, 3, 1), (8, 16, 3, 2), (4, 4, 1, 2), (32, 64, 3, 2)):
        add("gauss", Case("bwd_weight", 3, 5, 8, Ci, Co, k, s, family="gauss", fold=2, dbias=True))
    # ---- the lower tiers on the same non-square / mixed-pad / small-Ci maps ----
    for Ci, Co in ((3, 8), (1, 8), (2, 4), (8, 8), (8, 16), (16, 32), (4, 4), (32, 32)):
        for (H, W) in GEOMETRIES:
            for s in (1, 2):
                for j, op in enumerate(("fwd", "bwd_data", "bwd_weight")):
                    if op == "bwd_data" and Ci % 4:
                        continue
                    add("direct", Case(op, 5, H, W, Ci, Co, 3, s, door="direct", bias=op == "fwd", beta=(1.0, 0.0, 2.0)[j] if op != "fwd" else 0.0))
    for Ci, Co, k, s in ((3, 8, 3, 1), (1, 8, 3, 2), (2, 4, 3, 1), (8, 16, 3, 2), (16, 32, 1, 2), (32, 64, 3, 2), (64, 64, 3, 1)):
        for (H, W) in GEOMETRIES:
            for op in ("fwd", "bwd_data", "bwd_weight"):
                add("im2col", Case(op, 5, H, W, Ci, Co, k, s, door="im2col", bias=op == "fwd", beta=1.0 if op == "bwd_weight" else 0.0))
    return T


def admissible(c, ops):
    """Does the door of this case take it?  (The descriptor API by its plan, the direct kernels by conv3x3_supported.)"""
    from avsr_tf1_amd._lib import AvsrError
    if c.door == "desc":
        try:
            return len(R.plan(c, ops)) > 0
        except AvsrError:
            return False
    if c.door == "direct":
        Ho, Wo, _, _ = R.geometry(c)
        return bool(ops.conv3x3_supported(c.Ci, c.Co, c.H, c.W))
    return True


def cases():
    from avsr_tf1_amd import ops
    seen, out = set(), []
    for group, c in _table():
        if c in seen or not admissible(c, ops):
            continue
        seen.add(c)
        out.append((group, c))
    return out


CASES = cases()


def case_id(gc):
    g, c = gc
    d = {f.name: getattr(c, f.name) for f in R.dataclasses.fields(c)}
    opts = [k if v is True else "%s=%s" % (k, v) for k, v in d.items()
            if k not in ("op", "N", "H", "W", "Ci", "Co", "k", "stride", "door", "family", "seed") and v not in (False, None, 0, 0.0, "none")]
    return "%s-%s-%s-%dx%dx%d-%dto%d-k%ds%d-%s%s" % (g, c.door, c.op, c.N, c.H, c.W, c.Ci, c.Co, c.k, c.stride, c.family, "".join("-" + o for o in opts))


pytestmark = pytest.mark.gpu
WORST = {}


@pytest.mark.parametrize("gc", CASES, ids=case_id)
def test_conformance(gc):
    import torch
    from avsr_tf1_amd import ops
    _, c = gc
    p, out = R.run(c, torch, ops)
    ratio = R.check(p, out)
    if c.family == "gauss":
        WORST[c.op] = max(WORST.get(c.op, 0.0), ratio)
        print("gauss err / bound: %s %.3f (worst so far %.3f)" % (c.op, ratio, WORST[c.op]))


DETERMINISM = [Case("fwd", 7, 7, 6, 8, 16, stride=2, family="gauss", bias=True, stats=True, res="lazy", bn=True),         # conv_gen_kernel
               Case("bwd_data", 7, 9, 13, 8, 8, family="gauss", beta=0.5, acc=True, bnb=True),                           # conv_q4_kernel
               Case("bwd_data", 7, 7, 5, 8, 16, stride=2, family="gauss", bnb=True),                                      # four classes
               Case("bwd_weight", 5, 6, 8, 8, 8, family="gauss", dbias=True, fold=2),                                    # conv_wgrad_kernel, pairs
               Case("bwd_weight", 8, 5, 6, 64, 64, family="gauss", dbias=True, beta=1.0)]                                # row split


@pytest.mark.parametrize("c", DETERMINISM, ids=lambda c: case_id(("twice", c)))
def test_two_runs_leave_identical_bytes(c):
    """No atomics anywhere: the same call into fresh buffers gives the same bytes, statistics rows included."""
    import torch
    from avsr_tf1_amd import ops
    p = R.build(c)
    _, a = R.run(c, torch, ops, problem=p)
    _, b = R.run(c, torch, ops, problem=p)
    R.check(p, a)
    assert a.keys() == b.keys()
    for name in a:
        if name != "n":
            assert np.array_equal(np.asarray(a[name]).view(np.uint32), np.asarray(b[name]).view(np.uint32)), name
    assert a.get("n") == b.get("n")


# ---- refusals: the error code, and the sentinel outputs intact -----------------------------------------------------------------------------
ARG, UNSUP = -1, -3


class Bufs:
    """Device buffers of one descriptor call, every output filled with SENTINEL."""

    def __init__(self, torch, N=3, H=5, W=6, Ci=8, Co=8):
        s = lambda n: torch.from_numpy(np.full(n, R.SENTINEL, np.uint32).view(np.float32)).cuda()
        z = lambda n: torch.ones(n, device="cuda")
        big = 8 * 8 * 8 * 64                               # no descriptor of these tests is larger: a call that is NOT refused stays in bounds
        assert N * H * W * max(Ci, Co) <= big
        self.x, self.w, self.dy = z(big), z(9 * 64 * 64), z(big)
        self.vec = z(3 * 64)
        self.outs = {n: s(big) for n in ("y", "dx", "dx_out")}
        self.outs.update(dw=s(9 * 64 * 64), db=s(64), stats=s(512 * 2 * 64), scratch=s(1 << 19))

    def intact(self, torch):
        torch.cuda.synchronize()
        return all(bool((t.cpu().numpy().view(np.uint32) == R.SENTINEL).all()) for t in self.outs.values())


def _raw(ops, torch, B, d, which, **kw):
    """The C entry point's return code for call `which` on the buffers B, any operand replaceable by None through kw."""
    import ctypes as C
    L, s, f = ops._L(), ops._s(), ops.fptr
    a = dict(x=B.x, w=B.w, dy=B.dy, y=B.outs["y"], dx=B.outs["dx"], dw=B.outs["dw"], db=B.outs["db"], scratch=B.outs["scratch"], bias=None,
             res=None, stats=None, acc=None, bn_x=None, bn_sc=None, bn_sh=None, nparts=True, beta=1.0, dz=B.dy, fy=B.dy, fk=B.vec, dx_out=None,
             scratch_floats=None)
    a.update(kw)
    n = C.c_int32(0)
    npp = C.byref(n) if a["nparts"] else None
    nfl = a["scratch_floats"] if a["scratch_floats"] is not None else (a["scratch"].numel() if a["scratch"] is not None else 0)
    if which == "fwd":
        return L.avsr_conv_fwd(C.byref(d), f(a["x"]), f(a["w"]), f(a["bias"]), f(a["res"]), None, None, f(a["y"]), f(a["stats"]), npp, s)
    if which == "bwd_data":
        return L.avsr_conv_bwd_data(C.byref(d), f(a["dy"]), f(a["w"]), f(a["dx"]), float(a["beta"]), s)
    if which == "bwd_data_bn":
        return L.avsr_conv_bwd_data_bn(C.byref(d), f(a["dy"]), f(a["w"]), f(a["dx"]), float(a["beta"]), f(a["acc"]), f(a["bn_x"]), f(a["bn_sc"]),
                                       f(a["bn_sh"]), f(a["stats"]), npp, s)
    if which == "bwd_weight":
        return L.avsr_conv_bwd_weight(C.byref(d), f(a["x"]), f(a["dy"]), f(a["dw"]), f(a["db"]), float(a["beta"]), f(a["scratch"]), nfl, s)
    return L.avsr_conv_bwd_weight_bn(C.byref(d), f(a["x"]), f(a["dz"]), f(a["fy"]), f(a["fk"]), f(a["dx_out"]), f(a["dw"]), f(a["db"]),
                                     float(a["beta"]), f(a["scratch"]), nfl, s)


DOORS = ("fwd", "bwd_data", "bwd_data_bn", "bwd_weight", "bwd_weight_bn")


def _desc(ops, N=3, H=5, W=6, Ci=8, Co=8, k=3, s=1, **over):
    d = R.desc(Case("fwd", N, H, W, Ci, Co, k, s), ops)
    for key, val in over.items():
        setattr(d, key, val)
    return d


BAD_DESC = {"k=2": dict(k=2), "k=5": dict(k=5), "stride=3": dict(stride=3), "stride=0": dict(stride=0), "Co%4": dict(Co=6), "Ci=5": dict(Ci=5),
            "Ci=6": dict(Ci=6), "Ci=7": dict(Ci=7), "Co>64": dict(Co=68), "Co=0": dict(Co=0), "Ci=0": dict(Ci=0), "pad_t=2": dict(pad_t=2),
            "pad_t=-1": dict(pad_t=-1), "pad_l=2": dict(pad_l=2), "pad_l=-1": dict(pad_l=-1), "N=0": dict(N=0), "N=-1": dict(N=-1)}


@pytest.mark.parametrize("clause", list(BAD_DESC) + ["k=1 with pad_t", "k=1 with pad_l"])
def test_every_clause_of_the_descriptor_check_refuses_every_door(clause):
    import torch
    from avsr_tf1_amd import ops
    if clause.startswith("k=1"):
        d = _desc(ops, k=1, s=2, **{clause.split()[-1]: 1})
    else:
        d = _desc(ops, **BAD_DESC[clause])
    B = Bufs(torch)
    assert not ops.conv_supported(d) and not ops.conv_bwd_data_bn_supported(d) and not ops.conv_bwd_weight_bn_supported(d)
    for door in DOORS:
        assert _raw(ops, torch, B, d, door) == ARG, door
    assert B.intact(torch)


@pytest.mark.parametrize("door,missing", [("fwd", "x"), ("fwd", "w"), ("fwd", "y"), ("bwd_data", "dy"), ("bwd_data", "w"), ("bwd_data", "dx"),
                                          ("bwd_data_bn", "dy"), ("bwd_data_bn", "w"), ("bwd_data_bn", "dx"), ("bwd_weight", "x"), ("bwd_weight", "dy"),
                                          ("bwd_weight", "dw"), ("bwd_weight", "scratch"), ("bwd_weight_bn", "x"), ("bwd_weight_bn", "dz"),
                                          ("bwd_weight_bn", "fy"), ("bwd_weight_bn", "fk"), ("bwd_weight_bn", "dw"), ("bwd_weight_bn", "scratch")])
def test_a_missing_operand_is_an_argument_error(door, missing):
    import torch
    from avsr_tf1_amd import ops
    B = Bufs(torch)
    assert _raw(ops, torch, B, _desc(ops), door, **{missing: None}) == ARG
    assert B.intact(torch)


@pytest.mark.parametrize("missing", ["bn_sc", "bn_sh", "stats", "nparts"])
def test_the_batchnorm_backward_epilogue_needs_all_its_operands(missing):
    import torch
    from avsr_tf1_amd import ops
    B = Bufs(torch)
    full = dict(bn_x=B.x, bn_sc=B.vec, bn_sh=B.vec, stats=B.outs["stats"], nparts=True)
    full[missing] = None
    assert _raw(ops, torch, B, _desc(ops), "bwd_data_bn", **full) == ARG
    assert B.intact(torch)


def test_calls_the_kernels_cannot_serve_are_refused_before_any_launch():
    import torch
    from avsr_tf1_amd import ops
    B = Bufs(torch)
    bnb = dict(bn_x=B.x, bn_sc=B.vec, bn_sh=B.vec, stats=B.outs["stats"])
    # a 1x1 / stride-2 data gradient with beta == 0 (or any beta but 1): no tap reaches three of the four pixel classes
    for beta in (0.0, 2.0, 0.5):
        assert _raw(ops, torch, B, _desc(ops, Ci=8, Co=16, k=1, s=2), "bwd_data", beta=beta) == UNSUP
        assert _raw(ops, torch, B, _desc(ops, H=6, W=1, Ci=8, Co=16, k=1, s=2), "bwd_data", beta=beta) == UNSUP
    # acc or bnb where the data gradient is one launch per pixel class (stride 2, more than 16 channels; 1x1 / stride 2)
    for d in (_desc(ops, H=7, W=6, Ci=32, Co=64, s=2), _desc(ops, Ci=8, Co=16, k=1, s=2)):
        assert not ops.conv_bwd_data_bn_supported(d)
        assert _raw(ops, torch, B, d, "bwd_data_bn", acc=B.x) == UNSUP
        assert _raw(ops, torch, B, d, "bwd_data_bn", **bnb) == UNSUP
    # fold on a layer whose weight gradient needs two launches, and on a form without a fold instantiation
    for d in (_desc(ops, Ci=64, Co=16), _desc(ops, Ci=64, Co=32), _desc(ops, Ci=12, Co=4)):
        assert not ops.conv_bwd_weight_bn_supported(d)
        assert _raw(ops, torch, B, d, "bwd_weight_bn") == UNSUP
        assert _raw(ops, torch, B, d, "bwd_weight_bn", dx_out=B.outs["dx_out"]) == UNSUP
    # a 3-channel source with an epilogue operand; no data gradient towards fewer than 4 channels
    for d in (_desc(ops, Ci=3, Co=8), _desc(ops, Ci=3, Co=16), _desc(ops, Ci=1, Co=8)):
        assert _raw(ops, torch, B, d, "fwd", res=B.x) == UNSUP
        assert _raw(ops, torch, B, d, "bwd_data") == UNSUP
    # the BN-ReLU loader on a source of fewer than 4 channels (it would be ignored)
    for which in ("fwd", "bwd_weight"):
        assert _raw(ops, torch, B, _desc(ops, Ci=3, Co=8, bn_scale=ops.fptr(B.vec), bn_shift=ops.fptr(B.vec)), which) == UNSUP
    # 48 destination channels: three column tiles have no weight-gradient form
    assert _raw(ops, torch, B, _desc(ops, Ci=8, Co=48), "bwd_weight") == UNSUP
    assert B.intact(torch)


@pytest.mark.parametrize("c", [Case("bwd_weight", 5, 5, 6, 8, 16, dbias=True), Case("bwd_weight", 5, 6, 6, 8, 8, dbias=True),
                               Case("bwd_weight", 5, 5, 6, 64, 16, dbias=True)], ids=lambda c: case_id(("slab", c)))
def test_scratch_one_float_short_of_a_slab_is_an_argument_error(c):
    import torch
    from avsr_tf1_amd import ops
    B = Bufs(torch, N=c.N)
    d = R.desc(c, ops)
    slab = R.plan(c, ops)[0]["slab"]
    assert _raw(ops, torch, B, d, "bwd_weight", scratch_floats=slab - 1) == ARG
    assert B.intact(torch)


@pytest.fixture
def mfma_off():
    from avsr_tf1_amd import ops
    ops.conv_set_mfma(0)
    try:
        yield
    finally:
        ops.conv_set_mfma(1)


def test_every_door_is_unsupported_with_the_mfma_tier_switched_off(mfma_off):
    import torch
    from avsr_tf1_amd import ops
    from avsr_tf1_amd._lib import AvsrError
    B, d = Bufs(torch), _desc(ops)
    assert not ops.conv_supported(d) and not ops.conv_bwd_data_bn_supported(d) and not ops.conv_bwd_weight_bn_supported(d)
    for door in DOORS:
        assert _raw(ops, torch, B, d, door) == UNSUP, door
    with pytest.raises(AvsrError, match="-3"):
        ops.conv_plan(d, "fwd")
    assert B.intact(torch)


def test_the_switch_is_restored():
    from avsr_tf1_amd import ops
    assert ops.conv_supported(_desc(ops))


def test_report_the_worst_gauss_ratio_per_operation():
    """(Runs last in the file: prints what the commit message quotes; the bound itself is asserted case by case above.)"""
    print("worst gauss err / bound per op:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(0.0 <= v <= 1.0 for v in WORST.values())

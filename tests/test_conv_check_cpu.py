"""The convolution conformance checker (tests/ref_conv.py) judged on the CPU, and the dispatch of the descriptor API (avsr_conv_plan)
swept without a GPU.

Part 1: the "kernel" is numpy fp32 -- im2col with a shuffled depth order, shuffled partial rows.  The checker must accept this honest
result in every family and reject each named fault, one test per fault.
Part 2: the reachability sweep of avsr_conv_plan (profiles/conv_plan_sweep.txt), the coverage of tests/test_gpu_conv_conformance.py's
case table over it, and the agreement of the *_supported queries with the plan."""
import itertools
import os

import numpy as np
import pytest

import ref_conv as R
from ref_conv import BAND, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def round_bits(v, bits):
    """v rounded to `bits` significant bits (bf16: 8)."""
    m, e = np.frexp(np.asarray(v, f64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e).astype(f32)


def im2col32(x, k, s, pt, pl, Ho, Wo, fill=None):
    N, H, W, C = x.shape
    xp = np.zeros((N, max((Ho - 1) * s + k, pt + H), max((Wo - 1) * s + k, pl + W), C), f32)
    if fill is not None:
        xp[:] = fill
    xp[:, pt:pt + H, pl:pl + W] = x
    cols = np.empty((N, Ho, Wo, k, k, C), f32)
    for i in range(k):
        for j in range(k):
            cols[:, :, :, i, j] = xp[:, i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s]
    return cols


def simulate(p, fault=None, groups=3):
    """What an honest fp32 kernel leaves in the problem's buffers -- or one with the named fault."""
    c, v = p.case, p.val
    N, H, W, Ci, Co, k, s = c.N, c.H, c.W, c.Ci, c.Co, c.k, c.stride
    Ho, Wo, pt, pl = p.Ho, p.Wo, p.pt, p.pl
    rng = np.random.default_rng(5)
    out = {name: b.copy() for name, b in p.outputs.items()}

    def put(name, arr):
        out[name][BAND:BAND + arr.size] = arr.reshape(-1).astype(f32)

    def rounded(a):
        return round_bits(a, 8) if fault == "bf16" else (round_bits(a, 11) if fault == "bits11" else a)

    if fault == "swap_pads":
        assert pt != pl
        pt, pl = pl, pt
    w2 = None
    if "w" in v:
        w = v["w"]
        if fault == "w_transposed":
            assert Ci == Co
            w = np.ascontiguousarray(w.transpose(0, 1, 3, 2))
        w2 = w.reshape(k * k * Ci, Co)
    groups = max(1, min(groups, N))
    frames = np.array_split(np.arange(N), groups)

    def loaded(x):
        """The source map as staged (BN-ReLU loader) and the value of its halo."""
        if fault == "hw_index":
            assert H != W
            x = np.ascontiguousarray(x.reshape(N, W, H, Ci).transpose(0, 2, 1, 3))       # the row pitch taken from the other dimension
        if not c.bn:
            return x, None
        sc, sh = v["bn_sc"], v["bn_sh"]
        xin = np.maximum(x * sc + sh, f32(0))
        return xin, (np.maximum(sh, f32(0)) if fault == "halo" else None)

    def stat_rows(first, second):
        """[groups][2C] partial rows of two [N, ., ., C] maps, each row summed in fp32."""
        C = first.shape[3]
        rows = np.empty((groups, 2 * C), f32)
        for g, fr in enumerate(frames):
            rows[g, :C] = first[fr].reshape(-1, C).sum(0, dtype=f32)
            rows[g, C:] = second[fr].reshape(-1, C).sum(0, dtype=f32)
        return rows

    def put_stats(rows, yv):
        C = rows.shape[1] // 2
        nz = np.argwhere(yv != 0)[-1]
        val = yv[tuple(nz)]
        if fault == "sumsq_missing":
            rows[groups - 1, C + nz[3]] -= val * val
        if fault == "sum_twice":
            rows[groups - 1, nz[3]] += val
        buf = out["stats"]
        buf[BAND:BAND + rows.size] = rows.reshape(-1)
        if fault == "row_unwritten":
            assert groups >= 2
            buf[BAND + rows.shape[1]:BAND + 2 * rows.shape[1]] = p.outputs["stats"][BAND + rows.shape[1]:BAND + 2 * rows.shape[1]]
        out["n"] = groups

    if c.op == "fwd":
        xin, fill = loaded(rounded(v["x"]))
        cols = im2col32(xin, k, s, pt, pl, Ho, Wo, fill)
        if fault == "tap_dropped":
            cols[0, 0, 0, k - 1, k - 1, :] = 0
        perm = rng.permutation(k * k * Ci)
        y = cols.reshape(-1, k * k * Ci)[:, perm] @ w2[perm]
        y = y.reshape(N, Ho, Wo, Co)
        if c.bias:
            y = y + v["bias"]
        if c.res == "plain":
            y = y + v["res"]
        elif c.res == "lazy":
            y = y + np.maximum(v["res"] * v["res_sc"] + v["res_sh"], f32(0))
        if fault == "beta0_reads":
            y = y + f32(0) * out["y"][BAND:BAND + y.size].reshape(y.shape)
        put("y", y)
        if fault == "pair_overrun":
            assert W % 2 == 1
            out["y"][BAND + y.size:BAND + y.size + Co] = y[N - 1, Ho - 1, Wo - 1]
        if c.stats:
            put_stats(stat_rows(y, y * y), y)
    elif c.op == "bwd_data":
        dy = rounded(v["dy"])
        perm = rng.permutation(Co)
        dcol = (dy.reshape(-1, Co)[:, perm] @ np.ascontiguousarray(w2.T)[perm]).reshape(N, Ho, Wo, k, k, Ci)
        dxp = np.zeros((N, max((Ho - 1) * s + k, pt + H), max((Wo - 1) * s + k, pl + W), Ci), f32)
        for t in rng.permutation(k * k):
            i, j = divmod(int(t), k)
            dxp[:, i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s] += dcol[:, :, :, i, j]
        dx = dxp[:, pt:pt + H, pl:pl + W].copy()
        if c.beta != 0:
            o = v["acc"] if c.acc else p.old["dx"]
            dx = dx + f32(c.beta) * o
        elif fault == "beta0_reads":
            dx = dx + f32(0) * out["dx"][BAND:BAND + dx.size].reshape(dx.shape)
        if c.bnb:
            mask = v["bn_x"].astype(f64) * v["bnb_sc"] + v["bnb_sh"] > 0           # the fma's sign is the exact value's
            dx = np.where(mask, dx, f32(0))
        if fault == "cell_next_frame":
            assert H % 2 == 1 and N >= 2 and s == 2
            dx[1, 0, 0, :] = dx[0, H - 1, 0, :] + f32(1)                            # row H of frame 0 is row 0 of frame 1
        put("dx", dx)
        if fault == "guard_write":
            out["dx"][BAND - 1] = f32(0)
        if c.bnb:
            put_stats(stat_rows(dx, dx * v["bn_x"]), dx)
    else:
        xin, fill = loaded(rounded(v["x"]))
        cols = im2col32(xin, k, s, pt, pl, Ho, Wo, fill).reshape(N, Ho * Wo, k * k * Ci)
        if c.fold:
            k1, k2, k3 = v["fk"][:Co], v["fk"][Co:2 * Co], v["fk"][2 * Co:]
            dy = k1 * v["dz"] + (k2 * v["y"] + k3)
            if c.fold == 2:
                put("dx_out", dy)
                if fault == "dx_out_missing":
                    out["dx_out"][BAND + dy.size - 1] = p.outputs["dx_out"][BAND + dy.size - 1]
        else:
            dy = v["dy"]
        parts = [np.einsum("npk,npc->kc", cols[fr], dy[fr].reshape(len(fr), Ho * Wo, Co).astype(f32), dtype=f32) for fr in frames]
        dw = np.zeros((k * k * Ci, Co), f32)
        for g in rng.permutation(groups):
            dw = dw + parts[g]
        db = dy.reshape(-1, Co).sum(0, dtype=f32)
        if fault == "db_parity":
            db = 2 * dy[:, :, 1::2, :].reshape(-1, Co).sum(0, dtype=f32)
        if c.beta != 0:
            dw, db = dw + f32(c.beta) * p.old["dw"].reshape(dw.shape), db + f32(c.beta) * p.old["db"]
        elif fault == "beta0_reads":
            dw = dw + f32(0) * out["dw"][BAND:BAND + dw.size].reshape(dw.shape)
        put("dw", dw)
        if c.dbias:
            put("db", db)
        out["scratch_band"] = np.full(BAND, R.SENTINEL, np.uint32).view(f32)
        if fault == "guard_write":
            out["scratch_band"][0] = f32(1)
    return out


ACCEPT = [
    Case("fwd", 5, 7, 9, 8, 8, bias=True, stats=True),
    Case("fwd", 4, 9, 6, 8, 16, stride=2, bn=True, res="lazy", stats=True, bias=True),
    Case("fwd", 3, 9, 13, 3, 8, bias=True),
    Case("fwd", 3, 5, 6, 1, 8), Case("fwd", 3, 5, 5, 2, 4),
    Case("fwd", 3, 6, 5, 16, 32, k=1, stride=2, res="plain"),
    Case("bwd_data", 4, 7, 6, 8, 16, stride=2, beta=0.5), Case("bwd_data", 3, 5, 8, 8, 8, beta=2.0, acc=True, bnb=True),
    Case("bwd_data", 3, 5, 4, 16, 16, bnb=True), Case("bwd_data", 3, 6, 7, 8, 16, k=1, stride=2, beta=1.0),
    Case("bwd_weight", 5, 7, 6, 8, 8, dbias=True), Case("bwd_weight", 4, 9, 6, 8, 16, stride=2, bn=True, beta=1.0, dbias=True),
    Case("bwd_weight", 4, 5, 6, 8, 16, fold=2, dbias=True), Case("bwd_weight", 2, 9, 13, 3, 8, fold=1),
]


@pytest.mark.parametrize("family", ["exact", "mant_s", "mant_o", "gauss"])
@pytest.mark.parametrize("case", ACCEPT, ids=lambda c: "%s-%dx%dx%d-%d-%d-k%ds%d" % (c.op, c.N, c.H, c.W, c.Ci, c.Co, c.k, c.stride))
def test_checker_accepts_an_honest_fp32_result(case, family):
    if family.startswith("mant"):
        if case.stats or case.bnb or case.fold or case.bn:
            case = case.replace(stats=False, bnb=False, fold=0, bn=False)
    p = R.build(case.replace(family=family))
    ratio = R.check(p, simulate(p))
    assert ratio == 0.0 if family != "gauss" else 0.0 <= ratio <= 1.0


def rejects(case, fault, match=None, **kw):
    p = R.build(case)
    R.check(p, simulate(p, **kw))                       # the honest result passes ...
    with pytest.raises(R.ConvMismatch, match=match):    # ... the faulty one does not
        R.check(p, simulate(p, fault, **kw))


FWD = Case("fwd", 4, 7, 10, 8, 8, bias=True, stats=True)
MIXED = Case("fwd", 3, 7, 10, 8, 16, stride=2)          # H odd, W even: pad_t = 1, pad_l = 0


def test_rejects_a_tap_dropped_at_one_border_pixel():
    rejects(FWD, "tap_dropped", match=r"y: \d+ element.*\(0, 0, 0, 0\)")


def test_rejects_pad_t_and_pad_l_swapped():
    p = R.build(MIXED)
    assert (p.pt, p.pl) == (1, 0)
    rejects(MIXED, "swap_pads")
    rejects(Case("bwd_data", 3, 7, 10, 8, 16, stride=2), "swap_pads")
    rejects(Case("bwd_weight", 3, 10, 7, 8, 16, stride=2), "swap_pads")


def test_rejects_h_and_w_swapped_in_one_index():
    rejects(FWD, "hw_index")
    rejects(Case("bwd_weight", 3, 6, 5, 8, 8), "hw_index")


def test_rejects_weights_read_transposed():
    rejects(Case("fwd", 3, 5, 6, 8, 8), "w_transposed")
    rejects(Case("bwd_data", 3, 5, 6, 16, 16), "w_transposed")


def test_rejects_a_halo_that_is_not_zero_under_the_loader():
    c = Case("fwd", 3, 5, 6, 8, 8, bn=True)
    assert (R.build(c).val["bn_sh"] > 0).any()
    rejects(c, "halo")
    rejects(Case("bwd_weight", 3, 5, 6, 8, 16, bn=True), "halo")
    rejects(c.replace(family="gauss"), "halo")


def test_rejects_one_pixel_missing_from_the_sum_of_squares():
    rejects(FWD, "sumsq_missing", match="second sums")
    rejects(FWD.replace(N=40, H=12, W=12), "sumsq_missing", match="second sums")


def test_rejects_one_pixel_counted_twice_in_the_sum():
    rejects(FWD, "sum_twice", match="first sums")
    rejects(Case("bwd_data", 4, 6, 7, 8, 8, bnb=True), "sum_twice", match="first sums")


def test_rejects_a_statistics_row_left_unwritten():
    rejects(FWD, "row_unwritten", match="row 1 of 3 was not written")


def test_rejects_beta_zero_reading_the_old_destination():
    for c in (Case("fwd", 3, 5, 6, 8, 8), Case("bwd_data", 3, 5, 6, 8, 8), Case("bwd_weight", 3, 5, 6, 8, 8)):
        rejects(c, "beta0_reads")
        rejects(c.replace(family="gauss"), "beta0_reads")


def test_rejects_one_float_written_into_a_guard_band():
    rejects(Case("bwd_data", 3, 5, 6, 8, 8), "guard_write", match="outside the call's output.*-1 floats")
    rejects(Case("bwd_weight", 3, 5, 6, 8, 8), "guard_write", match="scratch")


def test_rejects_the_last_pixel_of_an_odd_width_pair_written_one_column_too_far():
    rejects(Case("fwd", 3, 6, 7, 16, 8), "pair_overrun", match=r"y: 8 float\(s\) outside")


def test_rejects_a_partial_cell_written_into_the_next_frame():
    rejects(Case("bwd_data", 3, 7, 6, 8, 16, stride=2), "cell_next_frame", match=r"\(1, 0, 0, 0\)")


def test_rejects_the_bias_gradient_of_the_wrong_parity():
    rejects(Case("bwd_weight", 3, 5, 6, 8, 8, dbias=True), "db_parity", match="db")


def test_rejects_dx_out_missing_one_element():
    c = Case("bwd_weight", 3, 5, 6, 8, 16, fold=2)
    rejects(c, "dx_out_missing", match=r"dx_out.*\(2, 4, 5, 15\)")
    rejects(c.replace(family="gauss"), "dx_out_missing")


MANT = [Case("fwd", 3, 5, 6, 8, 8, family="mant_s"), Case("fwd", 3, 6, 5, 64, 64, k=1, stride=2, family="mant_s"),
        Case("bwd_data", 3, 5, 6, 8, 8, family="mant_s"), Case("bwd_weight", 3, 5, 6, 8, 8, family="mant_s"),
        Case("fwd", 3, 6, 5, 4, 8, k=1, stride=2, family="mant_s")]


@pytest.mark.parametrize("fault", ["bf16", "bits11"])
def test_rejects_an_operand_of_reduced_precision_in_the_mantissa_family(fault):
    for c in MANT:
        rejects(c, fault)


# the deepest products the gauss family admits: GAUSS_DEPTH_MAX is a condition on the cases, justified here
DEEPEST = [Case("fwd", 3, 9, 13, 28, 8, family="gauss"), Case("bwd_data", 3, 9, 13, 8, 28, family="gauss"),
           Case("bwd_weight", 4, 8, 8, 8, 8, family="gauss"), Case("fwd", 3, 5, 6, 8, 8, family="gauss"),
           Case("fwd", 9, 6, 5, 64, 64, k=1, stride=2, family="gauss")]


def test_rejects_an_11_bit_operand_in_the_gauss_family_up_to_the_depth_cap():
    assert max(R.build(c).depth for c in DEEPEST) >= R.GAUSS_DEPTH_MAX - 4
    for c in DEEPEST:
        rejects(c, "bits11")
    with pytest.raises(AssertionError, match="small depth"):
        R.build(Case("fwd", 3, 5, 5, 32, 8, family="gauss"))


def test_exact_family_refuses_a_case_whose_sums_would_round():
    """The 2^24 condition is asserted, not assumed: a statistics row over too many frames is a failure of the case, not a skip."""
    p = R.build(Case("fwd", 40, 36, 36, 8, 8, stats=True))
    out = simulate(p, groups=1)
    with pytest.raises(AssertionError, match="built wrongly"):
        R.check(p, out)


# ---- part 2: the dispatch, swept and covered without a GPU -------------------------------------------------------------------------------
SWEEP_FILE = os.path.join(ROOT, "profiles", "conv_plan_sweep.txt")
OPS = ("fwd", "bwd_data", "bwd_weight")


def _ops():
    from avsr_tf1_amd import ops
    return ops


def test_plan_query_mirrors_the_entry_points_argument_checks():
    ops = _ops()
    from avsr_tf1_amd._lib import AvsrError
    d = R.desc(Case("fwd", 3, 5, 6, 8, 8), ops)
    assert [R.inst_name(L) for L in ops.conv_plan(d, "fwd", ["bias", "stats"])] == ["conv_q4_kernel<9,2,true,0>"]
    for op, flags in (("fwd", ["beta"]), ("bwd_data", ["bias"]), ("bwd_weight", ["res"]), ("bwd_weight", ["fold_dx"]), (3, [])):
        with pytest.raises(AvsrError, match="code -1"):
            ops.conv_plan(d, op, flags)
    with pytest.raises(AvsrError, match="code -1"):
        ops.conv_plan(d, "bwd_weight", scratch_floats=ops.conv_plan(d, "bwd_weight")[0]["slab"] - 1)
    d.k = 2
    with pytest.raises(AvsrError, match="code -1"):
        ops.conv_plan(d, "fwd")
    # the launches of a 64 -> 64 layer: 5 + 4 taps; bias and beta act on the first group, residual and statistics on the last
    d = R.desc(Case("fwd", 3, 5, 6, 64, 64), ops)
    L = ops.conv_plan(d, "fwd", ["bias", "res", "stats"])
    assert [(x["ntap"], x["ep"]) for x in L] == [(5, 0), (4, 3)] and [R.inst_name(x) for x in L] == ["conv_gen_kernel<20,true,0>", "conv_gen_kernel<18,true,3>"]
    # the weight gradient asks for the bias columns once
    L = ops.conv_plan(R.desc(Case("bwd_weight", 3, 5, 6, 64, 16), ops), "bwd_weight", ["dbias"])
    assert [x["slab"] for x in L] == [4 * 64 * 16 + 16, 4 * 64 * 16, 64 * 16] and [x["t0"] for x in L] == [0, 4, 8]


def test_every_listed_witness_reaches_its_instantiation_and_the_list_is_complete():
    """profiles/conv_plan_sweep.txt (tools/conv_plan_sweep.py: H, W in 1..40, 95 million planned calls) against the library as built."""
    ops = _ops()
    reach, unreach = R.parse_sweep_file(SWEEP_FILE)
    assert sorted([n for n, _ in reach] + unreach) == R.NAMED, "every instantiation the launch code names is listed exactly once"
    for name, w in reach:
        c = Case(w["op"], *(int(w[k]) for k in ("N", "H", "W", "Ci", "Co", "k", "stride")), bn=w["bn"] == "1")
        d = R.desc(c, ops)
        flags = [] if w["flags"] == "-" else w["flags"].split("+")
        L = ops.conv_plan(d, w["op"], flags)
        if w["scratch"] == "one_slab":
            L = ops.conv_plan(d, w["op"], flags, scratch_floats=max(x["slab"] for x in L))
        assert name in [R.inst_name(x) for x in L], (name, w)


def test_a_sweep_finds_nothing_outside_the_list_and_the_supported_queries_agree_with_the_plan():
    """A subset of the tool's sweep -- H, W in {1, 2, 5, 6, 36}, every Ci, nine Co, every flag combination, N in {3, 4800} -- must stay inside
    the reachable set on file, and avsr_conv_supported / _bwd_data_bn_supported / _bwd_weight_bn_supported must answer what the plan
    answers on every descriptor of it."""
    reach, unreach = R.parse_sweep_file(SWEEP_FILE)
    parts = [R.plan_sweep((ci, (1, 2, 5, 6, 36), (4, 8, 12, 16, 20, 32, 48, 52, 64), (3, 4800), True)) for ci in R.SWEEP_CI]
    found, calls, disagree = R.merge_sweeps(parts)
    assert calls > 500000
    assert not disagree, disagree[:5]
    assert not set(found) - {n for n, _ in reach}, sorted(set(found) - {n for n, _ in reach})
    assert not set(found) & set(unreach)


def _want_pad(CsL, SB):
    """cg_launch's bank-spreading rule: floats added to a staged pixel (0 = none wanted)."""
    for p in range(4):
        if (SB * (CsL // 4 + p)) % 4 == 2:
            return 4 * p
    return 0


def _data_regimes(c, Ls):
    """Names of the regimes of section 'grid cap and passes' (and the forms) one planned data-path case is in."""
    out = set()
    Cs, Cd = (c.Ci, c.Co) if c.op == "fwd" else (c.Co, c.Ci)
    CsL = (Cs + 3) & ~3
    for L in Ls:
        kern = "q4_%dch" % Cs if L["kernel"] == 1 else "gen_nsp%d" % L["nsp"]
        out.add("form " + kern)
        out.add("column tiles %d" % ((L["nsp"] * Cd + 15) // 16) if L["kernel"] == 0 else "form " + kern)
        F, grid, N = L["F"], L["grid"], c.N
        cnt = -(-N // grid)
        npass = -(-cnt // F)
        fp = -(-cnt // npass)
        if F == 1 and grid == 512 and 512 < N < 1024:
            out.add("round robin above 512 frames, %s %s" % (kern, c.op))
        if F > 1 and grid == 512 and N > 512 * F and npass >= 2 and (cnt % fp or (N % grid and (cnt - 1) % fp)):
            out.add("even shares in passes, last pass shorter, %s" % c.op)
        if grid > 1 and N % grid:
            out.add("N no multiple of the grid")
        if N < F:
            out.add("fewer frames than a pass holds")
        if L["kernel"] == 0 and Cs % 4 == 0:
            SB = 2 if L["nsp"] == 2 else (1 if L["nsp"] == 4 or c.op == "bwd_data" else c.stride)
            want = _want_pad(CsL, SB)
            if want and L["CsP"] == CsL + want:
                out.add("padded CsP")
            if want and L["CsP"] == CsL:
                out.add("unpadded CsP")
    if len(Ls) == 2 and [L["ntap"] for L in Ls] == [5, 4] and Cs == 64:
        out.add("tap groups 5 + 4 on a 64-channel source, %s" % c.op)
    if c.op == "bwd_data" and c.stride == 2 and c.k == 3:
        out.add("four classes in one launch" if len(Ls) == 1 and Ls[0]["nsp"] == 4 else "one launch per class")
    if c.k == 1 and c.stride == 2:
        out.add("1x1/2 shortcut %s" % c.op)
    return out


def _wgrad_regimes(c, Ls):
    out = set()
    for L in Ls:
        units = -(-c.N // L["F"])
        if c.scratch_slabs is None and L["grid"] < units and L["grid"] % 256 == 0:
            out.add("weight gradient at its 256 x wpc cap (%s)" % ("slab > 2048" if L["slab"] > 2048 else "slab <= 2048"))
        if c.scratch_slabs == 1 and L["grid"] == 1 and c.N > L["F"]:
            out.add("one slab: one workgroup walks everything")
        if c.scratch_slabs == 2 and L["grid"] == 2 and c.N == 5 and L["F"] == 1:
            out.add("two slabs, N = 5, F = 1: 3 and 2 passes")
        out.add("pixel-pair weight gradient" if L["nsp"] == 2 else "general weight gradient")
        if L["rs"]:
            out.add("row-split weight gradient")
    if len(Ls) > 1:
        out.add("weight gradient in %s tap groups" % ("deferred" if c.deferred else "immediate"))
        if c.dbias:
            assert [L["slab"] - L["ntap"] * c.Ci * c.Co for L in Ls] == [c.Co] + [0] * (len(Ls) - 1)
            out.add("bias columns on the first tap group only")
    if c.fold:
        out.add("fold %d" % c.fold)
    if c.k == 1 and c.stride == 2:
        out.add("1x1/2 shortcut bwd_weight")
    return out


REQUIRED = (
    ["round robin above 512 frames, %s" % s for s in ("q4_8ch fwd", "q4_3ch fwd", "gen_nsp1 fwd", "gen_nsp4 bwd_data", "q4_8ch bwd_data")]
    + ["even shares in passes, last pass shorter, fwd", "even shares in passes, last pass shorter, bwd_data", "N no multiple of the grid",
       "fewer frames than a pass holds", "padded CsP", "unpadded CsP", "tap groups 5 + 4 on a 64-channel source, fwd",
       "tap groups 5 + 4 on a 64-channel source, bwd_data", "four classes in one launch", "one launch per class", "1x1/2 shortcut fwd",
       "1x1/2 shortcut bwd_data", "1x1/2 shortcut bwd_weight", "form q4_8ch", "form q4_3ch", "form gen_nsp1", "form gen_nsp2", "form gen_nsp4",
       "column tiles 1", "column tiles 2", "column tiles 4",
       "weight gradient at its 256 x wpc cap (slab > 2048)", "weight gradient at its 256 x wpc cap (slab <= 2048)",
       "one slab: one workgroup walks everything", "two slabs, N = 5, F = 1: 3 and 2 passes", "pixel-pair weight gradient",
       "general weight gradient", "row-split weight gradient", "weight gradient in immediate tap groups", "weight gradient in deferred tap groups",
       "bias columns on the first tap group only", "fold 1", "fold 2"])


def test_the_gpu_case_table_covers_every_reachable_instantiation_and_every_regime():
    """tests/test_gpu_conv_conformance.py's table, planned case by case: every reachable instantiation is run by an exact case (and its
    every EP / FOLD value with it), and each regime is present according to the plan's grid, F and N -- not according to a comment."""
    ops = _ops()
    import test_gpu_conv_conformance as T
    reach, _ = R.parse_sweep_file(SWEEP_FILE)
    ran, regimes, doors = set(), set(), set()
    for group, c in T.CASES:
        doors.add((c.door, c.op, c.H > c.W, c.H < c.W))
        if c.door != "desc":
            continue
        Ls = R.plan(c, ops)
        assert Ls, c
        if c.family == "exact":
            ran.update(R.inst_name(L) for L in Ls)
            regimes |= _data_regimes(c, Ls) if c.op != "bwd_weight" else _wgrad_regimes(c, Ls)
    missing = sorted({n for n, _ in reach} - ran)
    assert not missing, "reachable instantiations no exact case runs: %s" % missing
    absent = [r for r in REQUIRED if r not in regimes]
    assert not absent, "regimes the case table does not reach according to the plan: %s" % absent
    for door in ("desc", "direct", "im2col"):
        for op in OPS:
            assert (door, op, True, False) in doors and (door, op, False, True) in doors, (door, op)
    # mixed pads, both ways round, at every door
    for door in ("desc", "direct", "im2col"):
        pads = {(R.geometry(c)[2], R.geometry(c)[3]) for _, c in T.CASES if c.door == door and c.k == 3 and c.stride == 2}
        assert {(1, 0), (0, 1)} <= pads, (door, pads)
    # frames of the 1-, 2- and 3-channel sources start at every alignment mod 4
    for Ci in (1, 2, 3):
        assert any(c.Ci == Ci and c.door == "desc" and (c.H * c.W * Ci) % 4 and {(n * c.H * c.W * Ci) % 4 for n in range(c.N)} == {0, 1, 2, 3}
                   or (c.Ci == Ci and (c.H * c.W * Ci) % 4 == 2 and c.N >= 2) for _, c in T.CASES), Ci
    assert len({c for _, c in T.CASES}) == len(T.CASES)

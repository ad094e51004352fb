"""The normalisation conformance checker (tests/ref_norm.py) judged on the CPU, and avsr_batchnorm_plan queried without a GPU.

(a) the checker accepts the honest fp32 twin on every case of the table, in every family;
(b) the fixture conditions hold for every case (integer means and the 2^24 sums of the exact family, nothing in the ReLU kink band, the
    noise caps, the zero and the constant column of the const family);
(c) the checker rejects each named fault, one test per fault, injected into the otherwise honest twin (remove the fault and the twin is
    the one (a) accepts: the test fails);
(d) avsr_batchnorm_plan mirrors the entry points' argument checks and names the form of every row of the table, and the table reaches
    every kernel of csrc/batchnorm.hip and both instance-norm kernels."""
import os
import re

import numpy as np
import pytest

import ref_norm as R
from ref_norm import ARG, CASES, Twin, case, case_id, f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def twin_run(c, fault=None):
    p = R.build(c)
    return p, R.run(p, Twin(fault))


def _maps(p):
    """(x, rows) of every row-walked operand of the case."""
    xs = [v for n, v in p.inp.items() if re.fullmatch(r"x\d*", n) and v.ndim >= 2]
    if p.case.op == "sync":                              # the shards of ONE map
        xs = [np.concatenate(xs)]
    return [(v, v.shape[-2]) for v in xs]


# ---- (a) + (b): one build per case serves both -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_the_fixture_holds_and_the_checker_accepts_the_twin(c):
    p, res = twin_run(c)
    R.check(p, res)
    # (b) noise never is the licence: 8 * noise <= 10 * T * mag, and no noise at all where a quantity has no terms
    for name, q in p.q.items():
        if q.kind in ("vec", "map"):
            T = R.T_VEC if q.kind == "vec" else R.T_MAP
            assert (8.0 * q.noise <= 10.0 * T * q.mag).all(), (name, float((q.noise / np.where(q.mag > 0, q.mag, 1.0)).max()))
    if c.family == "exact":
        for x, rows in _maps(p):
            x = x.astype(f64)
            s = x.sum(-2)
            assert np.array_equal(s / rows, np.rint(s / rows)) and np.abs(x).max() <= 3
            assert np.abs(x).sum(-2).max() < R.LIMIT and (x * x).sum(-2).max() < R.LIMIT
            if "dy" in p.inp:
                dy = p.inp["dy"].astype(f64)
                assert np.abs(dy).sum(-2).max() < R.LIMIT and np.abs(dy * x).sum(-2).max() < R.LIMIT
    if c.family == "const" and c.F >= 8 and c.op not in ("finalize", "bwd_finalize"):     # (their maps end in the fixture's partial rows)
        xs = [v for v, _ in _maps(p)]
        assert xs
        for x in xs:
            x = x.reshape(-1, c.F) if c.op != "instnorm" else x
            assert not x[..., 0].any() and (x[..., 1] == x[..., :1, 1]).all() and x[..., 1].all()
    if c.op in ("fwd", "apply", "bwd", "sync") and p.info.get("relu") and not p.rc and p.info.get("training", 1):
        x = np.concatenate([v for v, _ in _maps(p)]).astype(f64)
        m, v = R.stats64(x)
        eps = f64(np.float32(p.info.get("eps", 1e-5)))
        gx = p.inp["gamma"].astype(f64) * (x - m) / np.sqrt(v + eps)
        b = p.inp["beta"].astype(f64)
        assert not (np.abs(gx + b) < R.KINK * (np.abs(gx) + np.abs(b))).any()


def test_the_tolerances_are_eight_times_the_twin():
    w = R.measure()
    print("twin worst err / mag:", w, "T_VEC %.3g T_MAP %.3g" % (R.T_VEC, R.T_MAP))
    assert 8.0 * w["vec"] <= R.T_VEC <= 16.0 * w["vec"] and 8.0 * w["map"] <= R.T_MAP <= 16.0 * w["map"]
    assert R.T_VEC < 5e-5 / 10 and R.OFFSET_RATIO == 8.0


def test_the_table_has_every_family_and_door():
    ops = {c.op for c in CASES}
    assert ops == set(R.BUILDERS)
    for op in ops - {"eval_affine"}:
        assert {c.family for c in CASES if c.op == op} >= {"gauss", "exact"}, op
    for op in ("fwd", "bwd", "sync", "finalize", "instnorm"):
        assert {c.family for c in CASES if c.op == op} >= {"offset", "const"}, op
    # momentum 0 at n in {2, 5} through each finaliser: the moving variance is the variance the door feeds it
    for op, key in (("fwd", "bessel"), ("finalize", "bessel")):
        for n in (2, 5):
            assert {c.o(key) for c in CASES if c.op == op and c.rows == n and c.o("momentum") == 0.0} >= {0, 1}, (op, n)
    assert any(c.op == "fwd" and c.o("door") == "plain" and c.o("momentum") == 0.0 for c in CASES)


# ---- (c) the faults ----------------------------------------------------------------------------------------------------------------------------
def rejects(c, fault, match):
    p, res = twin_run(c)
    R.check(p, res)                                      # the honest twin passes on this very case
    p, res = twin_run(c, fault)
    with pytest.raises(R.NormMismatch, match=match):
        R.check(p, res)


SYNC_EXACT = case("sync", 128, 80, "exact", shards=(37, 91), relu=0)
SYNC_GAUSS = case("sync", 128, 80, "gauss", shards=(37, 91), relu=1)
BWD_RELU = case("bwd", 65, 80, "gauss", relu=1)


def test_one_row_missing_from_a_sum_is_a_whole_number_error():
    rejects(SYNC_EXACT, "row_missing", r"sum0: \d+ element\(s\) differ from the exact result")
    rejects(case("moments", 197, 80, "exact"), "row_missing", r"out64: .* differ from the exact result")
    rejects(case("stage1", 97, 80, "exact", mask="lazy"), "row_missing", r"part: .* differ from the exact result")
    rejects(case("instnorm", 9, 39, "exact", B=3), "row_missing", r"mean: .* differ from the exact result")


def test_one_row_counted_twice_is_a_whole_number_error():
    rejects(SYNC_EXACT, "row_twice", r"sum0: \d+ element\(s\) differ from the exact result")
    rejects(case("moments", 197, 80, "exact"), "row_twice", r"out64: .* differ from the exact result")


def test_a_subgroups_last_row_dropped_at_width_80():
    rejects(case("fwd", 197, 80, "exact", relu=1), "subgroup_last_row", r"save_mean: .* differ from the exact result")
    rejects(case("bwd", 65, 80, "exact", relu=1, dx=False), "subgroup_last_row", r"dbeta: .* differ from the exact result")


def test_the_tail_of_the_second_base_pass_dropped_at_width_260():
    rejects(case("fwd", 197, 260, "exact", relu=1), "base_tail", r"save_(mean|invstd): .* first at \(25[6-9],\)")
    rejects(case("bwd", 65, 260, "exact", relu=1, dx=False), "base_tail", r"dbeta: .* first at \(25[6-9],\)")


@pytest.mark.parametrize("count", [5, 4099])
@pytest.mark.parametrize("fault,bessel", [("biased_for_bessel", 1), ("bessel_for_biased", 0)])
def test_the_wrong_variance_in_the_moving_average(fault, bessel, count):
    rejects(case("finalize", count, 12, "gauss", nparts=3, bessel=bessel), fault, r"mov_var: \d+ element\(s\) outside the vec bound")
    rejects(case("fwd", count, 12, "gauss", bessel=bessel), fault, r"moving_var: \d+ element\(s\) outside the vec bound")


def test_the_divisor_rows_where_the_global_count_is_due():
    rejects(SYNC_GAUSS, "rows_for_global", r"mean0: \d+ element\(s\) outside the vec bound")


def test_beta_ignored_in_the_backward_mask():
    rejects(BWD_RELU, "beta_ignored", r"(dx|dbeta): \d+ element\(s\) outside")


def test_a_negative_gammas_mask_taken_as_positive():
    rejects(BWD_RELU, "neg_gamma_mask", r"(dx|dbeta): \d+ element\(s\) outside")


def test_dx_beta_applied_at_zero_reads_the_nan_destination():
    rejects(BWD_RELU, "dx_beta_at_0", r"dx: \d+ element\(s\) outside the map bound.*got \S*nan")
    rejects(case("bwd_apply", 5, 12, "gauss", beta=0.0), "dx_beta_at_0", r"dx: \d+ element\(s\) outside the map bound.*got \S*nan")


def test_dgamma_and_dbeta_swapped():
    rejects(BWD_RELU, "dgamma_dbeta_swapped", r"d(beta|gamma): \d+ element\(s\) outside the sum bound")
    rejects(case("bwd_finalize", 197, 20, "gauss", nparts=3), "dgamma_dbeta_swapped", r"d(beta|gamma): \d+ element\(s\) outside the vec bound")


def test_k2_with_the_wrong_sign():
    rejects(case("bwd_finalize", 197, 20, "gauss", nparts=3), "k2_sign", r"k: \d+ element\(s\) outside the vec bound, first at \(2\d,\)")


def test_the_local_sums_where_the_global_ones_are_due():
    rejects(case("bwd_finalize", 128, 20, "gauss", nparts=3, shards=(37, 91), grad_beta=1.0), "local_for_global", r"k_f64: \d+ element\(s\) outside the vec bound")


def test_a_negative_variance_let_through_as_nan():
    rejects(case("finalize", 197, 12, "gauss", nparts=3, bessel=1, negvar=True), "neg_var_nan", r"invstd: 1 element\(s\) outside the vec bound, first at \(2,\): got \S*nan")


def test_a_partial_row_beyond_nparts_read():
    rejects(case("finalize", 197, 12, "gauss", nparts=3, bessel=1), "part_beyond", r"mean: \d+ element\(s\) outside the vec bound.*got \S*nan")
    rejects(case("bwd_finalize", 197, 20, "gauss", nparts=3), "part_beyond", r"d(beta|gamma): \d+ element\(s\) outside the vec bound.*got \S*nan")


def test_a_float_in_a_band():
    rejects(case("fwd", 65, 80, "gauss"), "band_float", r"y: 1 float\(s\) of the bands around it were written, first at \+5200 floats")


def test_an_output_written_by_a_refused_call():
    rejects(case("fwd", 1000, 80, "gauss", scratch="short"), "refused_writes", r"y: written by a call that was refused")
    rejects(case("bwd", 1000, 80, "gauss", scratch="short"), "refused_writes", r"dx: written by a call that was refused")
    rejects(case("stage1", 9, 1028, "gauss"), "refused_writes", r"dz: written by a call that was refused")
    rejects(case("finalize", 197, 12, "gauss", nparts=3, bessel=0, moving="one"), "refused_writes", r"mean: written by a call that was refused")
    rejects(case("bwd_apply", 5, 6, "gauss"), "refused_writes", r"dx: written by a call that was refused")


def test_an_operand_rounded_to_bf16():
    rejects(case("fwd", 65, 80, "gauss"), "bf16_operand", r"(save_mean|save_invstd|y): \d+ element\(s\) outside")
    rejects(BWD_RELU, "bf16_operand", r"(dx|dbeta|dgamma): \d+ element\(s\) outside")
    rejects(SYNC_EXACT.replace(family="gauss"), "bf16_operand", r"(sum0|mean0): \d+ element\(s\) outside")


def test_a_wrong_return_code_and_a_written_input_are_seen():
    p, res = twin_run(case("fwd", 65, 80, "gauss"))
    res["rcs"] = [ARG]
    with pytest.raises(R.NormMismatch, match="return code -1 where 0 is due"):
        R.check(p, res)
    p, res = twin_run(case("fwd", 65, 80, "gauss"))
    res["in"]["x"] = res["in"]["x"].copy()
    res["in"]["x"][R.BAND + 7] = 0.0
    with pytest.raises(R.NormMismatch, match=r"input x: 1 float\(s\) were written, first at \+7"):
        R.check(p, res)
    p, res = twin_run(case("fwd", 65, 80, "gauss"))
    other = {k: (dict(v) if isinstance(v, dict) else v) for k, v in res.items()}
    other["out"]["y"] = res["out"]["y"].copy()
    other["out"]["y"][R.BAND + 3] += np.float32(1e-6)
    with pytest.raises(R.NormMismatch, match="two identical calls left different bytes"):
        R.same_bytes(res, other)
    R.same_bytes(res, res)


# ---- (d) the plan --------------------------------------------------------------------------------------------------------------------------------
def test_the_plan_names_the_form_of_every_row():
    n = 0
    for c in CASES:
        pl = R.plan_of(c)
        p = R.build(c)
        if pl is None:
            assert c.o("plan") is None
            continue
        assert pl["err"] == R.plan_err_of(p), case_id(c)
        for k, v in c.o("plan", ()):
            n += 1
            assert pl[k] == v, (case_id(c), k, pl[k], v, pl)
    assert n > 250
    forms = {(pl["vec"], pl["direct"], bool(pl["apply_grid"])) for pl in (R.plan_of(c) for c in CASES if c.op == "bwd") if not pl["err"]}
    assert forms == {(v, d, a) for v in (0, 1) for d in (0, 1) for a in (False, True)}
    fwd = [R.plan_of(c) for c in CASES if c.op == "fwd"]
    assert {pl["G"] for pl in fwd if not pl["err"]} >= {64, 21, 3, 2, 1} and any(pl["rows_per_block"] == 65 for pl in fwd)


PLAN_OPS = ("fwd", "bwd", "sync_sum", "sync_sqsum", "sync_moments", "bwd_stage1", "bwd_apply")


def test_the_plan_mirrors_the_argument_checks():
    plan = R._plan
    for op in PLAN_OPS:
        assert plan(op, 64, 8)["err"] == 0, op
        for rows, F in ((0, 8), (-1, 8), (64, 0), (64, -4)):
            assert plan(op, rows, F) == dict(blocks=0, rows_per_block=0, G=0, vec=0, direct=0, apply_grid=0, err=ARG), (op, rows, F)
        assert plan(op, 64, 6)["err"] == (0 if op in ("bwd", "sync_moments") else ARG), op      # the F % 4 rule, where there is one
    assert plan("bwd_stage1", 64, 1024)["err"] == 0 and plan("bwd_stage1", 64, 1028)["err"] == ARG
    assert plan("bwd_apply", 64, 1028)["err"] == 0
    assert plan("fwd", 1 << 31, 8)["err"] == ARG and plan("bwd_apply", 1 << 31, 8)["err"] == 0          # int32 rows but for the 64-bit doors
    from avsr_tf1_amd import ops
    with pytest.raises(KeyError):
        ops.batchnorm_plan("nothing", 64, 8)
    assert ops.batchnorm_plan(7, 64, 8)["err"] == ARG and ops.batchnorm_plan(-1, 64, 8)["err"] == ARG
    # scratch minima: one partial row and what lies behind it works at any row count; one float less is refused
    for op, unit in (("fwd", 3), ("bwd", 4), ("sync_sum", 1), ("sync_sqsum", 1), ("sync_moments", 4)):
        for rows in (1, 64, 1000, 131073):
            for F in (4, 80, 260):
                ok, short = plan(op, rows, F, unit * F, ("aligned",)), plan(op, rows, F, unit * F - 1, ("aligned",))
                assert ok["err"] == 0 and ok["blocks"] == 1 and (ok["rows_per_block"] in (rows, 0)) or (rows < 64 and ok["rows_per_block"] == 64), (op, rows, F, ok)
                assert short["err"] == ARG, (op, rows, F)
        assert plan(op, 64, 8, 0)["err"] == ARG and plan(op, 64, 8, -5)["err"] == ARG
    # avsr_batchnorm_bwd: the float4 kernels need 4096 rows, a width that divides 1024 and aligned operands; the flags are reported as given
    assert plan("bwd", 4096, 64, 1 << 40, ("aligned",))["vec"] == 1 and plan("bwd", 4095, 64, 1 << 40, ("aligned",))["vec"] == 0
    assert plan("bwd", 4096, 64)["vec"] == 0 and plan("bwd", 4096, 12, 1 << 40, ("aligned",))["vec"] == 0
    assert plan("bwd", 8192, 2048, 1 << 40, ("aligned",))["vec"] == 0 and plan("bwd", 8192, 2, 1 << 40, ("aligned",))["vec"] == 0
    assert plan("bwd", 64, 8, 1 << 40, ("direct",))["direct"] == 1 and plan("bwd", 64, 8)["direct"] == 0
    assert plan("bwd", 64, 8, 1 << 40, ("dx",))["apply_grid"] == 2 and plan("bwd", 64, 8)["apply_grid"] == 0
    # grids and their caps
    assert plan("fwd", 131072, 8)["blocks"] == 2048 and plan("fwd", 131072, 8)["rows_per_block"] == 64
    assert plan("fwd", 8192, 1024)["apply_grid"] == 4096 and plan("bwd", 8192, 1024, 1 << 40, ("aligned", "dx"))["apply_grid"] == 4096
    assert plan("bwd", 8192, 1024, 1 << 40, ("aligned",))["blocks"] == 1024 and plan("bwd", 8192, 1024, 1 << 40, ("dx",))["apply_grid"] == 8192
    assert plan("sync_moments", 1 << 20, 8)["blocks"] == 1024 and plan("bwd_stage1", 1 << 20, 8)["blocks"] == 512
    assert plan("bwd_apply", 1 << 22, 8)["apply_grid"] == 2048 and plan("bwd_apply", 1, 4)["apply_grid"] == 1


def test_the_table_reaches_every_kernel():
    reached = set()
    for c in CASES:
        reached |= R.kernels_of(R.build(c))
    assert sorted(reached) == R.KERNELS
    # and KERNELS is every kernel of the two sources, by name
    src = open(os.path.join(ROOT, "avsr-tf1_amd", "csrc", "batchnorm.hip")).read()
    names = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)", src))
    conv = open(os.path.join(ROOT, "avsr-tf1_amd", "csrc", "conv.hip")).read()
    names |= {n for n in re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)", conv) if n.startswith("instnorm")}
    assert names == {k.split("<")[0] for k in R.KERNELS}
    # every exported normalisation entry point is driven by some builder
    header = open(os.path.join(ROOT, "include", "avsr_hip.h")).read()
    entries = set(re.findall(r"\bint (avsr_(?:batchnorm_\w+|bn_\w+|conv3d_bn_finalize|instnorm_\w+))\(", header)) - {"avsr_batchnorm_plan"}
    driven = set(re.findall(r'E\("(\w+)"', open(os.path.join(ROOT, "tests", "ref_norm.py")).read()))
    driven |= set(re.findall(r'"(bn_finalize|conv3d_bn_finalize)"', open(os.path.join(ROOT, "tests", "ref_norm.py")).read()))
    assert entries == {"avsr_" + d for d in driven}, entries ^ {"avsr_" + d for d in driven}
    assert len(entries) == 20                               # the 18 of csrc/batchnorm.hip (the plan query aside) and the two of the instance norm

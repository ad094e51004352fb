"""Conformance of the normalisations on the GPU: every entry point of csrc/batchnorm.hip and the instance norm of csrc/conv.hip, one test
per case of tests/ref_norm.py's table.  Each test asserts the plan (avsr_batchnorm_plan) against the row before any number, runs the call
-- or the short chain of calls -- twice into fresh poisoned buffers, hands the first run to the checker (fp64 reference, exact integer
sums, per-channel and per-element bounds, bands, inputs, refusals) and compares the second run with it bit for bit.  The NORMQ lines
record engine error, noise and bound per quantity.

tests/test_norm_check_cpu.py proves on the CPU that the checker rejects the faults such kernels can have, and that the table reaches
every kernel and every form the plan can name."""
import numpy as np
import pytest

import ref_norm as R

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_conformance(c):
    import torch
    from avsr_tf1_amd import ops
    p = R.build(c)
    pl = R.plan_of(c)
    if pl is not None:
        assert pl["err"] == R.plan_err_of(p)
        for k, v in c.o("plan", ()):
            assert pl[k] == v, (k, pl)
    to_dev = lambda a: torch.from_numpy(a.copy()).cuda()
    to_host = lambda t: t.cpu().numpy()
    E = R.GpuEngine(torch, ops)
    first = R.run(p, E, to_dev, to_host)
    second = R.run(p, E, to_dev, to_host)
    report = R.check(p, first)
    R.same_bytes(first, second)
    for line in R.normq_lines(c, report):
        print(line)
    for name, v in report.items():
        key = (c.op, name.rstrip("0123456789"))
        WORST[key] = max(WORST.get(key, 0.0), v[3])


def test_report_the_worst_ratio_per_quantity():
    """(Runs last in the file: prints what the commit message quotes; the bounds themselves are asserted case by case above.)"""
    for (op, name), v in sorted(WORST.items()):
        print("NORMQ worst %-12s %-14s err / bound %.3f" % (op, name, v))
    assert all(0.0 <= v <= 1.0 for v in WORST.values())
    assert not np.isnan(list(WORST.values())).any()

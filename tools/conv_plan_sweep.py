"""Which kernel instantiations can the convolutions' descriptor API reach?  python tools/conv_plan_sweep.py [--quick] [-j N] > profiles/conv_plan_sweep.txt

Runs avsr_conv_plan (the library's own dispatch on its dry path; no GPU) over
  H, W in 1..40, Ci in {1,2,3,4,8,12,16,20,32,48,64}, Co in {4,8,...,64}, k in {1,3}, stride in {1,2}, N in {1,3,600,4800},
  with and without the BN-ReLU loader, ample and one-slab scratch,
and prints every reachable instantiation with one smallest witness, then the instantiations the launch code names and nothing reaches.
Every flag combination the API accepts is swept at N = 3 on the geometries with H, W in SWEEP_SMALL (the instantiation does not depend on
N, and the flags only select EP / FOLD); the remaining geometries and frame counts are swept with one flag set per EP / FOLD value.
About 95 million planned calls, a minute and a half on eight cores.  tests/test_conv_check_cpu.py re-plans every witness and sweeps a subset, so the
file cannot go stale unnoticed; the sweep itself lives in tests/ref_conv.py (plan_sweep)."""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_conv as R                                                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="H, W in SWEEP_SMALL only, every flag combination")
    ap.add_argument("-j", type=int, default=min(8, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    hw = R.SWEEP_SMALL if a.quick else tuple(range(1, 41))
    jobs = [(ci, hw, R.SWEEP_CO, R.SWEEP_N, a.quick) for ci in R.SWEEP_CI]
    if a.j > 1:
        with multiprocessing.Pool(a.j) as pool:
            parts = pool.map(R.plan_sweep, jobs)
    else:
        parts = [R.plan_sweep(j) for j in jobs]
    found, calls, disagree = R.merge_sweeps(parts)
    print("# avsr_conv_plan over H, W in %s; Ci in %s; Co in 4..64 step 4; k in {1,3}; stride in {1,2}; N in %s;" % (
        "SWEEP_SMALL" if a.quick else "1..40", list(R.SWEEP_CI), list(R.SWEEP_N)))
    print("# BN-ReLU loader off / on; ample and one-slab scratch; %d planned calls; %d disagreements of the *_supported queries with the plan." % (
        calls, len(disagree)))
    print("# Written by tools/conv_plan_sweep.py.")
    print("reachable %d" % len(found))
    for name in sorted(found):
        print(R.witness_line(name, found[name][1]))
    missing = [n for n in R.NAMED if n not in found]
    print("named_unreachable %d" % len(missing))
    for name in missing:
        print(name)
    for dis in disagree[:20]:
        print("# DISAGREE (query, bn, N, H, W, Ci, Co, k, stride, plan, query's answer):", dis, file=sys.stderr)
    extra = sorted(set(found) - set(R.NAMED))
    assert not extra, extra
    assert not disagree


if __name__ == "__main__":
    main()

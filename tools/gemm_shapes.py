"""Time avsr_gemm on free-standing shapes: python tools/gemm_shapes.py "M,N,K,ta,tb[,splitk]" ...   (fp32 MFMA peak 157.3 TF)

Every layout that is timed is also checked with the conformance suite's checker (tests/ref_gemm.py): Gaussian inputs against the fp32
dot-product bound up to K = GAUSS_KMAX, beyond that small integers whose fp32 result is exact -- so a timing run of a new kernel also
says whether the kernel is right.  Shapes whose fp64 reference would be too large are timed on random inputs and reported unchecked."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from avsr_tf1_amd import ops                                        # noqa: E402
import ref_gemm as R                                                # noqa: E402


def main():
    ws = torch.empty(64 << 20, device="cuda")
    ops.set_gemm_workspace(ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for spec in sys.argv[1:]:
        v = [int(x) for x in spec.split(",")]
        M, N, K, ta, tb = v[:5]
        sk = v[5] if len(v) > 5 else ops.auto_splitk(M, N, K)
        while sk > 1 and sk * M * N > ws.numel():
            sk //= 2
        family = "gauss" if K <= R.GAUSS_KMAX else "exact"
        checkable = M * N * K <= 1 << 33 and (family == "gauss" or K * R.EXACT_INT ** 2 < 1 << 24)
        if checkable:
            p = R.build(R.Case(M, N, K, ta=ta, tb=tb, splitk=sk, family=family))
            t = R.to_device(p, torch)
            go = lambda: R.issue(p, t, ops, ws)                     # noqa: E731
        else:
            A = torch.randn((K, M) if ta else (M, K), device="cuda")
            B = torch.randn((N, K) if tb else (K, N), device="cuda")
            Cm = torch.zeros(M, N, device="cuda")
            a, b, c = ops.mat(A, A.shape[1]), ops.mat(B, B.shape[1]), ops.mat(Cm, N)
            go = lambda: ops.gemm(a, b, c, M, N, K, trans_a=ta, trans_b=tb, splitk=sk, workspace=ws)      # noqa: E731
        for rep in range(2):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(10):
                go()
            e1.record()
            torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 100.0
        print("M=%-6d N=%-6d K=%-6d ta=%d tb=%d splitk=%-5s class=%-2s %8.1f us %7.1f TF" %
              (M, N, K, ta, tb, sk, R.layout_class(R.Case(M, N, K, ta=ta, tb=tb)), us, 2.0 * M * N * K / us * 1e-6))
        if not checkable:
            print("      not checked: the reference of this shape is out of the checker's range")
            continue
        try:
            ratio = R.check(p, *R.fetch(t))
            print("      %s" % ("exact (integer inputs, bit for bit)" if family == "exact" else "within the fp32 bound, worst err/bound %.3f" % ratio))
        except R.GemmMismatch as e:
            print("      WRONG: %s" % e)


if __name__ == "__main__":
    main()

"""Fisher information of the hyper-parameters from a kept factor (tgp_gp_fisher / tgp_gp_fisher_sum, seam S2j) against the
solve that keeps the factor, on one MI355X.

    python tools/fisher_bench.py [--sizes 4096,16384] [--reps R] [--out profiles/fisher_bench.txt]

For n = 4096 and 16 384 and three kernels -- AnisotropicRBF, AnisotropicVonKarman and their two-term sum -- the time of
``ops.gp_fisher`` and its ratio to ``ops.gp_solve(keep=True)`` of the same run.  The forecast it is held against: about
8 T n^3 flops (two substitutions of n rows per derivative matrix, 4 T matrices), at the covariance route's 65 TF 0.55 s for one
kernel at n = 16 384 and about 10 ms at n = 4096.

Device times are the library's own ([1] factorisation of tgp_gp_solve, [3] device compute of tgp_gp_fisher); wall times include
the host boundary.  Best of --reps after one warm-up.  A record, not a pass condition.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam               # noqa: E402


def _specs():
    iL = headline_invlam()
    arbf = ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=iL[0, 0], b=iL[0, 1], c=iL[1, 1])
    avk = ops.KernelSpec(_lib.TGP_AVK, amp=1.0, a=iL[0, 0], b=iL[0, 1], c=iL[1, 1])
    half = [ops.KernelSpec(s.kind, amp=0.5, a=s.a, b=s.b, c=s.c) for s in (avk, arbf)]
    return (("AnisotropicRBF", arbf, 1), ("AnisotropicVonKarman", avk, 1), ("AVK + ARBF", ops.KernelSumSpec(half), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = _lib.get_ctx()
    say("%-22s %6s  %12s %12s  %12s %12s  %9s %9s  %8s  %s" % ("kernel", "n", "solve wall", "chol dev", "fisher wall", "fisher dev",
                                                              "wall x", "dev x", "TF (8Tn^3)", "forecast"))
    for n in [int(s) for s in args.sizes.split(",")]:
        X, y, ye, _ = star_field(n, 1, seed=5)
        y = y - y.mean()
        for name, spec, T in _specs():
            solve_wall = chol_dev = None
            fac = None
            for _ in range(args.reps + 1):
                if fac is not None:
                    fac.free(keep_memory=True)
                t0 = time.perf_counter()
                fac = ops.gp_solve(spec, X, y, ye, keep=True)[3]
                wall = (time.perf_counter() - t0) * 1e3
                dev = _lib.timings(ctx)[1]
                solve_wall = wall if solve_wall is None or wall < solve_wall else solve_wall
                chol_dev = dev if chol_dev is None or dev < chol_dev else chol_dev
            fisher_wall = fisher_dev = None
            for r in range(args.reps + 1):
                t0 = time.perf_counter()
                ops.gp_fisher(spec, fac, X)
                wall = (time.perf_counter() - t0) * 1e3
                dev = _lib.timings(ctx)[3]
                if r > 0:
                    fisher_wall = wall if fisher_wall is None or wall < fisher_wall else fisher_wall
                    fisher_dev = dev if fisher_dev is None or dev < fisher_dev else fisher_dev
            fac.free()
            flops = 8.0 * T * float(n) ** 3
            forecast_ms = flops / 65e12 * 1e3
            say("%-22s %6d  %9.2f ms %9.2f ms  %9.2f ms %9.2f ms  %8.1fx %8.1fx  %8.1f  %.1f ms at 65 TF: %s"
                % (name, n, solve_wall, chol_dev, fisher_wall, fisher_dev, fisher_wall / solve_wall, fisher_dev / chol_dev,
                   flops / (fisher_dev * 1e-3) / 1e12, forecast_ms, "met" if fisher_dev <= forecast_ms else "missed"))
    if args.out:
        dn = os.path.dirname(args.out)
        if dn:
            os.makedirs(dn, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

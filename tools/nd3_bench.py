#!/usr/bin/env python3
"""Device times of the 3-D entries beside their 2-D namesakes on the same data with the third column dropped, in the same run:
the packed K build, the fused predict (M = 262 144) and predict_var of 4096 points, for AnisotropicRBF and AnisotropicVonKarman
at N = 16 384 and 65 536.  Times are the library's own event timings (tgp_last_timings: [0] K build, [3] predict / variance), the
smallest of --reps calls after one warm-up call.  Writes profiles/nd3_bench.txt (or --out).

    python tools/nd3_bench.py [--sizes 16384,65536] [--m 262144] [--reps 3] [--out profiles/nd3_bench.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from treegp_amd import _lib, ops  # noqa: E402

INVLAM3 = np.array([[400.0, 80.0, 30.0], [80.0, 500.0, -40.0], [30.0, -40.0, 300.0]])


def specs(kind):
    m = INVLAM3
    s3 = ops.KernelSpec3(kind, amp=1.0, m=(m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]))
    s2 = ops.KernelSpec(kind, amp=1.0, a=m[0, 0], b=m[0, 1], c=m[1, 1])
    return s2, s3


def best(fn, slot, reps, ctx):
    fn()
    times = []
    for _ in range(reps):
        fn()
        times.append(_lib.timings(ctx)[slot])
    return min(times)


def kbuild_time(spec, X, reps, ctx, lib):
    n = len(X)
    Np = lib.tgp_padded_n(n)
    dX = ops.DeviceBuffer.from_array(ctx, np.ascontiguousarray(X))
    dA = ops.DeviceBuffer(ctx, lib.tgp_panel_elems(Np) * 8)
    entry = lib.tgp_d_kbuild_lower3 if isinstance(spec, ops.KernelSpec3) else lib.tgp_d_kbuild_lower
    c = spec.to_c()
    t = best(lambda: _lib.check(ctx, entry(ctx, C.byref(c), dX.ptr, n, None, dA.ptr), "kbuild"), 0, reps, ctx)
    dX.free()
    dA.free()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,65536")
    ap.add_argument("--m", type=int, default=262144)
    ap.add_argument("--mvar", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nd3_bench.txt"))
    args = ap.parse_args()
    ctx, lib = _lib.get_ctx(), _lib.load_library()
    rng = np.random.default_rng(0)
    lines = ["# tools/nd3_bench.py: device ms, smallest of %d calls after a warm-up; 2-D = the same data with the third column dropped"
             % args.reps, "# kind  N  what  ms_2d  ms_3d  ratio_3d_over_2d"]
    for n in [int(v) for v in args.sizes.split(",")]:
        side = np.sqrt(n / 1500.0)                                      # the star density of the headline workload
        X3 = rng.uniform(0.0, side, (n, 3))
        X3[:, 2] *= 0.2
        Xs3 = rng.uniform(0.0, side, (args.m, 3))
        Xs3[:, 2] *= 0.2
        alpha = rng.standard_normal(n)
        y = rng.standard_normal(n)
        for name, kind in (("AnisotropicRBF", _lib.TGP_ARBF), ("AnisotropicVonKarman", _lib.TGP_AVK)):
            s2, s3 = specs(kind)
            rows = []
            rows.append(("kbuild", kbuild_time(s2, X3[:, :2], args.reps, ctx, lib), kbuild_time(s3, X3, args.reps, ctx, lib)))
            rows.append(("predict M=%d" % args.m,
                         best(lambda: ops.gp_predict(s2, X3[:, :2], alpha, Xs3[:, :2], ctx=ctx), 3, args.reps, ctx),
                         best(lambda: ops.gp_predict(s3, X3, alpha, Xs3, ctx=ctx), 3, args.reps, ctx)))
            tv = []
            for spec, X, Xs in ((s2, X3[:, :2], Xs3[:args.mvar, :2]), (s3, X3, Xs3[:args.mvar])):
                factor = ops.gp_solve(spec, X, y, 0.3 * np.ones(n), keep=True, want_alpha=False, ctx=ctx)[3]
                tv.append(best(lambda: ops.gp_predict_var(spec, factor, X, Xs, ctx=ctx), 3, max(1, args.reps - 1), ctx))
                factor.free()
            rows.append(("predict_var m=%d" % args.mvar, tv[0], tv[1]))
            for what, t2, t3 in rows:
                lines.append("%-22s %6d  %-20s %10.3f %10.3f  %.3f" % (name, n, what, t2, t3, t3 / t2))
                print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

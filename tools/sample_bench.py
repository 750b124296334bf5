"""Realisations (seam S3d): the product Y = L Z of tgp_factor_lmul, and a whole gaussian_random_field call.

    python tools/sample_bench.py [--sizes 8192,32768,65536] [--nrhs 1,4,16] [--reps R] [--json out.json]

  1. tgp_factor_lmul on a kept factor at every N and nrhs: device time (timings[11], best of R after a warm-up) and the
     effective rate against the bytes of L it streams, tgp_panel_elems(Np) * 8 per group of 8 right-hand sides
  2. gaussian_random_field at the largest N, 4 samples: wall time of the call (K build + Cholesky + product + transfers)

The pass is HBM-bound: the goal is the >= 4.5 TB/s the dependency-chained triangular sweeps reach on the same data.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import treegp_amd as tg                                                      # noqa: E402
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam               # noqa: E402

GROUP = 8                       # right-hand sides per read of L (LMUL_R in csrc/lmul.hip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,32768,65536")
    ap.add_argument("--nrhs", default="1,4,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    iL = headline_invlam()
    spec = ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=iL[0, 0], b=iL[0, 1], c=iL[1, 1])
    lib = _lib.load_library()
    ctx = _lib.get_ctx()
    rows = []
    sizes = [int(s) for s in a.sizes.split(",")]
    for n in sizes:
        X, _, ye, _ = star_field(n, 1, seed=5)
        fac = ops.gp_solve(spec, X, np.zeros(n), ye, keep=True, want_alpha=False)[3]
        Np = int(lib.tgp_padded_n(n))
        lbytes = 8.0 * lib.tgp_panel_elems(Np)
        for nrhs in [int(v) for v in a.nrhs.split(",")]:
            Z = np.random.default_rng(nrhs).standard_normal((nrhs, n))
            ops.factor_lmul(fac, Z)
            best, wall = None, None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ops.factor_lmul(fac, Z)
                w = (time.perf_counter() - t0) * 1e3
                d = _lib.timings(ctx)[11]
                if best is None or d < best:
                    best, wall = d, w
            groups = (nrhs + GROUP - 1) // GROUP
            r = dict(what="factor_lmul", N=n, nrhs=nrhs, device_ms=round(best, 3), wall_ms=round(wall, 3),
                     L_GB=round(lbytes / 1e9, 3), groups=groups, TBps=round(groups * lbytes / (best * 1e-3) / 1e12, 3))
            rows.append(r)
            print("factor_lmul  N=%6d nrhs=%3d  device %8.3f ms  wall %8.3f ms  L %.2f GB x %d  %.2f TB/s"
                  % (n, nrhs, best, wall, r["L_GB"], groups, r["TBps"]), flush=True)
        fac.free()
    n = max(sizes)
    X, _, ye, _ = star_field(n, 1, seed=6)
    kernel = tg.eval_kernel("1.0**2 * AnisotropicRBF(invLam=array(%r))" % (iL.tolist(),))
    tg.gaussian_random_field(kernel, X, n_samples=4, y_err=ye)
    t0 = time.perf_counter()
    out = tg.gaussian_random_field(kernel, X, n_samples=4, y_err=ye)
    wall = (time.perf_counter() - t0) * 1e3
    tm = _lib.timings(ctx)
    r = dict(what="gaussian_random_field", N=n, n_samples=4, wall_ms=round(wall, 1), kbuild_ms=round(tm[0], 2),
             chol_ms=round(tm[1], 2), lmul_ms=round(tm[11], 3), finite=bool(np.isfinite(out).all()))
    rows.append(r)
    print("gaussian_random_field N=%d 4 samples: wall %.1f ms (K build %.2f, Cholesky %.2f, L Z %.3f ms)"
          % (n, wall, tm[0], tm[1], tm[11]), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

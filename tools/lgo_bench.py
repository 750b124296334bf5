"""Diagonal blocks of K^-1 from a kept factor (tgp_factor_inv_blocks, seam S3h: what leave-group-out cross-validation needs)
against the diagonal alone (tgp_factor_inv_diag, seam S3e) on the same factor in the same run, and predict_lgo against the
loop of refits it replaces.

    python tools/lgo_bench.py [--reps R] [--refits K] [--sizes 8192,16384,32768] [--out profiles/lgo_bench.txt]

  1. N = 8192, 16 384, 32 768, groups of 128 contiguous rows: device time ([3]) of tgp_factor_inv_diag and of
     tgp_factor_inv_blocks on one factor, their ratio, and the factorisation's ([1] of tgp_gp_solve) for scale
  2. GPInterpolation.predict_lgo, wall time of the whole call on a fresh object (factorisation included), for
       rows128   groups of 128 contiguous rows (the kept factor as it is)
       folds10   10 random folds (kfold_labels; the permuted route, blocks of N / 10 rows solved on the device)
       grid16    a 16 x 16 spatial grid (spatial_block_labels; the permuted route)
     against the refit loop: for a group, solve the other points again and predict the group (ops.gp_solve + ops.gp_predict).
     --refits K groups are refitted and timed (the first K), and the loop's time is their mean times the number of groups:
     an extrapolation, marked as such.  The refits' predictions check predict_lgo's (max_abs_diff).

Device times are the library's own; wall times include the host boundary.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import treegp_amd as tg                                                     # noqa: E402
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam               # noqa: E402

LINES = []


def say(line):
    LINES.append(line)
    print(line, flush=True)


def _time(fn, reps):
    """best of `reps` after one warm-up: (wall ms, device ms, transfer ms, result)"""
    out = fn()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        tm = _lib.timings(_lib.get_ctx())
        if best is None or tm[3] < best[1]:
            best = (wall, tm[3], tm[9])
    return best + (out,)


def device_rows(spec, n, reps):
    X, y, ye, _ = star_field(n, 1, seed=5)
    chol_ms = None
    for i in range(2):                                                      # the second factorisation finds everything warm
        fac = ops.gp_solve(spec, X, y - y.mean(), ye, keep=True, want_alpha=False)[3]
        chol_ms = _lib.timings(_lib.get_ctx())[1]
        if i == 0:
            fac.free(keep_memory=True)
    starts = np.arange(0, n + 1, 128)
    wall_d, dev_d, d2h_d, d = _time(lambda: ops.factor_inv_diag(fac), reps)
    wall_b, dev_b, d2h_b, blocks = _time(lambda: ops.factor_inv_blocks(fac, starts), reps)
    fac.free()
    diff = np.max(np.abs(np.concatenate([np.diag(b) for b in blocks]) - d) / d)
    say("factorisation           N=%6d  device %9.2f ms" % (n, chol_ms))
    say("inv_diag                N=%6d  device %9.2f ms  d2h %7.2f ms  wall %9.2f ms" % (n, dev_d, d2h_d, wall_d))
    say("inv_blocks g=128        N=%6d  device %9.2f ms  d2h %7.2f ms  wall %9.2f ms  vs_inv_diag=%.3fx  "
        "diag_max_rel_diff=%.2e" % (n, dev_b, d2h_b, wall_b, dev_b / dev_d, diff))
    return dev_b / dev_d


def lgo_rows(kernel, spec, n, refits):
    X, y, ye, _ = star_field(n, 1, seed=5)
    cases = (("rows128", np.arange(n) // 128),
             ("folds10", tg.kfold_labels(n, 10)),
             ("grid16", tg.spatial_block_labels(X, 16, 16)))
    for what, labels in cases:
        gp = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=True)
        gp.initialize(X, y, y_err=ye)
        t0 = time.perf_counter()
        y_lgo = gp.predict_lgo(labels)
        wall = (time.perf_counter() - t0) * 1e3
        del gp
        names = np.unique(labels)
        r = y - y.mean()
        t_refit, worst = 0.0, 0.0
        for lab in names[:refits]:
            G = labels == lab
            t0 = time.perf_counter()
            alpha = ops.gp_solve(spec, X[~G], r[~G], ye[~G])[0]
            pred = ops.gp_predict(spec, X[~G], alpha, X[G]) + y.mean()
            t_refit += (time.perf_counter() - t0) * 1e3
            worst = max(worst, np.max(np.abs(pred - y_lgo[G])))
        k = min(refits, len(names))
        loop = t_refit / k * len(names)
        say("predict_lgo %-10s  N=%6d  groups %4d (largest %5d)  wall %10.2f ms  refit loop %12.2f ms "
            "(extrapolated from %d refits)  speedup=%.1fx  max_abs_diff=%.2e"
            % (what, n, len(names), np.bincount(np.unique(labels, return_inverse=True)[1]).max(), wall, loop, k, loop / wall, worst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--refits", type=int, default=3)
    ap.add_argument("--sizes", default="8192,16384,32768")
    ap.add_argument("--out", default=os.path.join("profiles", "lgo_bench.txt"))
    args = ap.parse_args()
    iL = headline_invlam()
    spec = ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=iL[0, 0], b=iL[0, 1], c=iL[1, 1])
    kernel = "1.0**2 * AnisotropicRBF(invLam=array([[%r, %r], [%r, %r]]))" % tuple(float(v) for v in iL.ravel())
    sizes = [int(s) for s in args.sizes.split(",")]
    say("# tools/lgo_bench.py --reps %d --refits %d --sizes %s" % (args.reps, args.refits, args.sizes))
    ratios = {n: device_rows(spec, n, args.reps) for n in sizes}
    for n in sizes:
        lgo_rows(kernel, spec, n, args.refits)
    n = max(sizes)
    say("# forecast: inv_blocks <= 1.25x inv_diag at N = 32 768 with groups of 128; measured at N = %d: %.3fx -> %s"
        % (n, ratios[n], "met" if ratios[n] <= 1.25 else "MISSED"))
    dn = os.path.dirname(args.out)
    if dn:
        os.makedirs(dn, exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

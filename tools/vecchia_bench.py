"""Local conditionals (tgp_gp_local_cond, seam S3v; ops.gp_local_cond) measured on one GPU in one run.

    python tools/vecchia_bench.py [--reps R] [--skip-large] [--skip-fit] [--out profiles/vecchia_bench.txt]

(a) headline star field, N = 65 536 and N = 1 048 576, k = 32 / 64 / 128: one PRIOR (Vecchia likelihood) and one LOO call -- the
    phases the library times and the wall time -- beside ``tgp_gp_predict_local`` with Xs = X on the same data in the same run,
    and beside the dense ``log_likelihood`` at 65 536; a call on given lists (what a fit's evaluation costs) as well;
(b) N = 16 384, same field: (log L_local - log L_dense) / n for k = 16 ... 128, for the random ordering and for sorting by x
    (approximation quality: a property of the method, reported and not asserted);
(c) one ``optimizer="local-likelihood"`` fit at N = 65 536, and one beside the dense fit at a size where both run.
Each timed call is warmed up once; times are the median (min .. max) of ``reps`` calls.  Nothing here is a pass criterion.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import treegp_amd as tg                                                     # noqa: E402
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam               # noqa: E402

FORECAST = {   # whole call, ms, written into DESIGN.md before the first measurement
    (65536, "loo", 64): 10.0, (65536, "prior", 64): 15.0, (1048576, "loo", 64): 150.0, (1048576, "prior", 64): 250.0,
}


def headline_kernel():
    iL = headline_invlam()
    a, b, c = float(iL[0, 0]), float(iL[0, 1]), float(iL[1, 1])
    spec = ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=a, b=b, c=c)
    text = "1.0**2 * AnisotropicRBF(invLam=array([[%r, %r], [%r, %r]]))" % (a, b, b, c)
    return spec, text


def med(ts):
    return "%8.2f ms (%.2f .. %.2f)" % (float(np.median(ts)), min(ts), max(ts))


def timed(fn, reps):
    """wall and the library's slots [0], [2], [3] of reps calls after one warm-up; the last result"""
    ctx = _lib.get_ctx()
    rows = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        t = _lib.timings(ctx)
        if r:
            rows.append((dt, t[0], t[2], t[3]))
    return [list(c) for c in zip(*rows)], out


def loglik(sums, n):
    return -0.5 * sums[1] - 0.5 * sums[0] - 0.5 * n * np.log(2.0 * np.pi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecchia_bench.txt"))
    args = ap.parse_args()
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    spec, text = headline_kernel()
    lines = ["# tools/vecchia_bench.py --reps %d : median (min .. max) of %d calls after one warm-up; one GPU, one run" % (args.reps, args.reps),
             "# %s" % lib.tgp_version().decode(), "# kernel %s" % text]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # (b) approximation quality first (the smallest case)
    n = 16384
    X, y, y_err, _ = star_field(n, 1, seed=3)
    resid = y - y.mean()
    _, logdet, chi2, _ = ops.gp_solve(spec, X, resid, y_err, want_alpha=False)
    ll_dense = -0.5 * chi2 - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
    say("## (b) quality, N = %d: dense log L = %.3f (%.5f per point); (log L_local - log L_dense) / n" % (n, ll_dense, ll_dense / n))
    by_x = np.empty(n, dtype=np.int32)
    by_x[np.argsort(X[:, 0], kind="stable")] = np.arange(n, dtype=np.int32)
    for k in (16, 32, 64, 128):
        row = []
        for rank in (ops.vecchia_rank(n, 0), ops.vecchia_rank(n, 1), by_x):
            _, _, sums = ops.gp_local_cond(spec, X, resid, y_err, k=k, mode="prior", rank=rank)
            row.append((loglik(sums, n) - ll_dense) / n)
        _, _, sums = ops.gp_local_cond(spec, X, resid, y_err, k=k, mode="loo")
        say("k = %3d   random (seed 0) %+.3e   random (seed 1) %+.3e   sorted by x %+.3e   [LOO score per point %.5f]"
            % (k, row[0], row[1], row[2], loglik(sums, n) / n))

    # (a) timings
    sizes = [65536] + ([] if args.skip_large else [1 << 20])
    for n in sizes:
        X, y, y_err, _ = star_field(n, 1, seed=3 if n == 65536 else 5)
        resid = y - y.mean()
        rank = ops.vecchia_rank(n, 0)
        reps = args.reps if n == 65536 else max(1, args.reps - 1)
        say("## (a) headline star field, N = %d" % n)
        if n == 65536:
            from treegp_amd.log_likelihood import log_likelihood
            gp_kernel = tg.GPInterpolation(kernel=text, optimizer="none").kernel_template
            dense = []
            obj = log_likelihood(X, resid, y_err)
            for r in range(3):
                t0 = time.perf_counter()
                ll_d = obj.log_likelihood(gp_kernel)
                dense.append((time.perf_counter() - t0) * 1e3)
            say("dense log_likelihood (wall): first %.1f ms, then %.1f and %.1f ms; log L = %.3f" % (dense[0], dense[1], dense[2], ll_d))
            lib.tgp_release_caches(ctx)
        for k in (32, 64, 128):
            (wall, grid, search, solve), out = timed(lambda: ops.gp_local_cond(spec, X, resid, y_err, k=k, mode="prior", rank=rank,
                                                                               return_neighbors=True), reps)
            nbr = out[3]
            say("k = %3d PRIOR        host+upload %s   search %s   solve+sums %s   whole call %s   log L = %.3f"
                % (k, med(grid), med(search), med(solve), med(wall), loglik(out[2], n)))
            f = FORECAST.get((n, "prior", k))
            if f:
                say("          forecast %.0f ms whole call: %s" % (f, "met" if np.median(wall) <= f else "missed by %.2fx" % (np.median(wall) / f)))
            (wall_g, grid_g, _, solve_g), out_g = timed(lambda: ops.gp_local_cond(spec, X, resid, y_err, k=k, neighbors=nbr), reps)
            say("k = %3d given lists  host+upload %s   solve+sums %s   whole call %s   (upload share %.0f %%; sums %s)"
                % (k, med(grid_g), med(solve_g), med(wall_g), 100.0 * np.median(grid_g) / np.median(wall_g),
                   "same bits" if out_g[2].tobytes() == out[2].tobytes() else "DIFFERENT BITS"))
            (wall, grid, search, solve), out = timed(lambda: ops.gp_local_cond(spec, X, resid, y_err, k=k, mode="loo"), reps)
            say("k = %3d LOO          host+upload %s   search %s   solve+sums %s   whole call %s   score = %.3f"
                % (k, med(grid), med(search), med(solve), med(wall), loglik(out[2], n)))
            f = FORECAST.get((n, "loo", k))
            if f:
                say("          forecast %.0f ms whole call: %s" % (f, "met" if np.median(wall) <= f else "missed by %.2fx" % (np.median(wall) / f)))
            (wall, grid, search, solve), _ = timed(lambda: ops.gp_predict_local(spec, X, resid, y_err, X, k=k, return_var=True), reps)
            say("k = %3d predict_local(Xs = X)  grid %s   search %s   solve %s   whole call %s"
                % (k, med(grid), med(search), med(solve), med(wall)))

    # (c) fits
    if not args.skip_fit:
        start = "0.7**2 * AnisotropicRBF(invLam=array([[60., 0.], [0., 60.]]))"
        for n, both in ((8192, True), (65536, False)):
            X, y, y_err, _ = star_field(n, 1, seed=3)
            gp = tg.GPInterpolation(kernel=start, optimizer="local-likelihood", normalize=True, local_k=64)
            gp.initialize(X, y, y_err=y_err)
            t0 = time.perf_counter()
            gp.solve()
            dt = time.perf_counter() - t0
            say("## (c) local-likelihood fit, N = %d, k = 64: %.2f s, local log L = %.3f, kernel %s"
                % (n, dt, gp._optimizer._logL, " ".join(repr(gp.kernel).split())))
            if both:
                say("    dense log L at the local optimum %.3f" % gp.return_log_likelihood())
                gd = tg.GPInterpolation(kernel=start, optimizer="log-likelihood", normalize=True)
                gd.initialize(X, y, y_err=y_err)
                t0 = time.perf_counter()
                gd.solve()
                dt = time.perf_counter() - t0
                say("    dense fit: %.2f s, log L = %.3f, kernel %s; theta local - dense = %s"
                    % (dt, gd._optimizer._logL, " ".join(repr(gd.kernel).split()), np.array2string(gp.kernel.theta - gd.kernel.theta, precision=4)))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

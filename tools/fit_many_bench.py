"""Maximum-likelihood fits of many small GPs at once (treegp_amd.solve_many, seam S2f) against a loop over the objects, same box,
same process, same run.

    python tools/fit_many_bench.py [--cases 600x64,1024x64,2048x32,4096x16] [--reps 5] [--out profiles/fit_many_bench.txt]

For every (N, B): B GPInterpolation objects "1.0**2 * AnisotropicRBF(invLam=...)" (ntheta = 4) with optimizer="log-likelihood",
each on its own synthetic star field (treegp_amd.synthetic.star_field, differing seeds) and started from its own scaling of
the headline kernel.
  auto      treegp_amd.solve_many(gps): every L-BFGS-B iteration of all B fits is one ops.gp_solve_grad_batch call
  fd        treegp_amd.solve_many(gps, gradient="fd"): SciPy's forward differences, the 5 points of all B fits in one
            ops.gp_solve_batch call per iteration (the reference's iterates)
  loop      for gp in gps: gp.solve() -- the only route before solve_many, unchanged by it: the yardstick
Every object is initialised again before each repetition, outside the timed region; a timed region ends when the fitted kernels
are back on the host (every device call synchronises).  One warm-up, then the median of --reps (at least 5) repetitions.
The last two columns are gradient evaluations per second without an optimiser around them: one ops.gp_solve_grad_batch call for
all B problems against a loop of ops.gp_solve_grad_resident over B resident problems; [3] of the batched call's timings (inverse
and reduction) and the sum of its other phases are listed with them.  Rows are appended to --out as they are measured.

Goal (a forecast from the README's figures, not a measurement: 36 600 batched solves/s at N = 1024 with B = 64 against 6 200
from four contexts, and a gradient costing about three factorisations' flops where finite differences cost five solves): auto
several-fold the loop at N <= 1024 -- taken as >= 3x -- with a shrinking margin towards N = 4096, where it should still not be
slower than the loop (>= 1x).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import treegp_amd as treegp                                                 # noqa: E402
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam              # noqa: E402

GOALS = {600: 3.0, 1024: 3.0, 2048: 1.0, 4096: 1.0}


def objects(n, count, seed):
    rng = np.random.default_rng(seed)
    iL = headline_invlam()
    gps, data = [], []
    for i in range(count):
        X, y, ye, _ = star_field(n, 1, seed=seed + i)
        kern = "1.0**2 * AnisotropicRBF(invLam=array(%r))" % ((rng.uniform(0.7, 1.4) * iL).tolist(),)
        gps.append(treegp.GPInterpolation(kernel=kern, optimizer="log-likelihood", normalize=True))
        data.append((X, y, ye))
    return gps, data


def median_of(reps, reset, fn):
    reset()
    fn()
    times = []
    for _ in range(reps):
        reset()
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="600x64,1024x64,2048x32,4096x16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "fit_many_bench.txt"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5 (the columns are medians)")
    ctx = _lib.get_ctx()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    say("# tools/fit_many_bench.py --cases %s --reps %d   (GPU_MAX_HW_QUEUES=%s)" % (a.cases, a.reps, os.environ.get("GPU_MAX_HW_QUEUES")))
    say("# fits/s: median of %d after one warm-up [min .. max of the repetitions' times in s]; grad/s: gradient evaluations per second" % a.reps)
    for case in a.cases.split(","):
        n, B = [int(v) for v in case.split("x")]
        gps, data = objects(n, B, 1000 * n + B)

        def reset():
            for gp, (X, y, ye) in zip(gps, data):
                gp.initialize(X, y, y_err=ye)

        def loop():
            for gp in gps:
                gp.solve()
        res = {}
        for name, fn in (("auto", lambda: treegp.solve_many(gps)), ("fd", lambda: treegp.solve_many(gps, gradient="fd")), ("loop", loop)):
            res[name] = median_of(a.reps, reset, fn)
            res[name + "_logL"] = float(np.mean([gp._optimizer._logL for gp in gps]))
        # gradient evaluations alone, at the start kernels
        reset()
        specs = [treegp.kernel_to_spec(gp.kernel) for gp in gps]
        Xs, ys, es = [gp._X for gp in gps], [gp._residual() for gp in gps], [gp._y_err for gp in gps]
        t_gb = median_of(a.reps, lambda: None, lambda: ops.gp_solve_grad_batch(specs, Xs, ys, es))[0]
        tm = _lib.timings(ctx)
        resident = [ops.ResidentProblem(X, y, e) for X, y, e in zip(Xs, ys, es)]
        try:
            t_gl = median_of(a.reps, lambda: None, lambda: [ops.gp_solve_grad_resident(s, p) for s, p in zip(specs, resident)])[0]
        finally:
            for p in resident:
                p.close()
        speed = res["loop"][0] / res["auto"][0]
        goal = GOALS.get(n)
        verdict = "" if goal is None else "  goal >= %.0fx: %s" % (goal, "met" if speed >= goal else "missed")
        say("N = %4d  B = %2d  fits/s  auto %8.2f [%.3f .. %.3f]  fd %8.2f [%.3f .. %.3f]  loop %8.2f [%.3f .. %.3f]  auto/loop %5.2fx  "
            "fd/loop %5.2fx%s" % (n, B, B / res["auto"][0], res["auto"][1], res["auto"][2], B / res["fd"][0], res["fd"][1], res["fd"][2],
                                 B / res["loop"][0], res["loop"][1], res["loop"][2], speed, res["loop"][0] / res["fd"][0], verdict))
        say("                   mean log L  auto %.6f  fd %.6f  loop %.6f" % (res["auto_logL"], res["fd_logL"], res["loop_logL"]))
        say("                   grad/s  batched %9.1f  loop of gp_solve_grad_resident %9.1f  %5.2fx   device ms per batched call: "
            "K + Cholesky + sweeps %.2f, inverse + reduction %.2f" % (B / t_gb, B / t_gl, t_gl / t_gb, tm[0] + tm[1] + tm[2], tm[3]))
        del gps, data
    out.close()


if __name__ == "__main__":
    main()

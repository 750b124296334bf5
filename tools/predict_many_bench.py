"""Error bars for many small GPs (seam S3f, tgp_gp_posterior_batch) against a loop over the objects, same box, same run.

    python tools/predict_many_bench.py [--sizes 256,1024,2048,4096] [--batches 16,64] [--reps R] [--json out.json]

For every N (= M, the query points per object) and B objects, each a GPInterpolation with its own star field, values, errors
and anisotropic Gaussian kernel:
  loop      [gp.predict(X, return_var=True) for gp, X in ...]: per object one factorisation (kept), the mean and the S3c
            variance (or the S3b covariance)
  batched   treegp_amd.predict_many(gps, Xs, return_var=True): one batched factorisation and substitution for all objects,
            then each object's mean from the batch's alpha
each timed from objects without a cached solution (dropped before every repetition, outside the timed region), best of R
after a warm-up, for return_var and return_cov.  The device phases come from one direct ops.gp_posterior_batch call on the
same data (timings [0] K build, [1] Cholesky, [2] sweeps, [3] posterior compute, [9] result transfer).  Goals (forecasts
from the batched solve's rates, not measurements): variance >= 4x at N = M = 1024, B = 64 and >= 2x at N = M = 4096, B = 16.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import treegp_amd as treegp                                                 # noqa: E402
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam              # noqa: E402


def objects(n, count, seed):
    rng = np.random.default_rng(seed)
    ell = 1.0 / np.sqrt(np.diag(headline_invlam()))          # the headline field's correlation lengths
    gps, Xs = [], []
    for i in range(count):
        X, y, ye, Xq = star_field(n, n, seed=seed + i)
        s = rng.uniform(0.8, 1.25)
        amp = rng.uniform(0.5, 2.0)
        kern = "%r**2 * AnisotropicRBF(scale_length=[%r, %r])" % (float(np.sqrt(amp)), float(s * ell[0]), float(s * ell[1]))
        gp = treegp.GPInterpolation(kernel=kern, optimizer="none", normalize=True)
        gp.initialize(X, y, y_err=ye)
        gps.append(gp)
        Xs.append(Xq)
    return gps, Xs


def best_of(reps, reset, fn):
    reset()
    fn()
    best = None
    for _ in range(reps):
        reset()
        t0 = time.perf_counter()
        fn()
        t = time.perf_counter() - t0
        best = t if best is None or t < best else best
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2048,4096")
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = _lib.get_ctx()
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        for B in [int(s) for s in a.batches.split(",")]:
            gps, Xs = objects(n, B, 1000 * n + B)

            def reset():
                for gp in gps:
                    gp._drop_solution()
            for what in ("var", "cov"):
                kw = {"return_" + what: True}
                t_loop = best_of(a.reps, reset, lambda: [gp.predict(X, **kw) for gp, X in zip(gps, Xs)])
                t_batch = best_of(a.reps, reset, lambda: treegp.predict_many(gps, Xs, **kw))
                specs = [treegp.kernel_to_spec(gp.kernel) for gp in gps]
                ops.gp_posterior_batch(specs, [gp._X for gp in gps], [gp._residual() for gp in gps], [gp._y_err for gp in gps],
                                       Xs, what=what)
                tm = _lib.timings(ctx)
                row = dict(n=n, m=n, batch=B, what=what, loop_s=t_loop, batched_s=t_batch, speedup=t_loop / t_batch,
                           phases_ms=dict(kbuild=tm[0], cholesky=tm[1], sweeps=tm[2], posterior=tm[3], transfer=tm[9]))
                rows.append(row)
                print("N = M = %5d  B = %3d  %s  loop %9.2f ms  batched %9.2f ms  %5.2fx   device: K %.2f chol %.2f sweeps %.2f "
                      "posterior %.2f transfer %.2f ms" % (n, B, what, 1e3 * t_loop, 1e3 * t_batch, t_loop / t_batch, tm[0], tm[1],
                                                           tm[2], tm[3], tm[9]), flush=True)
            del gps, Xs
    goals = []
    for (n, B, goal) in ((1024, 64, 4.0), (4096, 16, 2.0)):
        r = [x for x in rows if x["n"] == n and x["batch"] == B and x["what"] == "var"]
        if r:
            goals.append(dict(n=n, batch=B, goal=goal, speedup=r[0]["speedup"], met=r[0]["speedup"] >= goal))
            print("goal variance N = M = %d, B = %d: %.2fx against %.1fx -- %s" % (n, B, r[0]["speedup"], goal,
                                                                                 "met" if r[0]["speedup"] >= goal else "missed"))
    out = dict(tool="predict_many_bench", hw_queues=os.environ.get("GPU_MAX_HW_QUEUES"), reps=a.reps, rows=rows, goals=goals)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

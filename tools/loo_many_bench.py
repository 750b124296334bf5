"""Leave-one-out for many small GPs (seam S2g, tgp_gp_loo_batch) against a loop over the objects, same box, same run.

    python tools/loo_many_bench.py [--cases 256:64,1024:64,2048:64,4096:16] [--reps R] [--out profiles/loo_many_bench]

For every N and B objects, each a GPInterpolation with its own star field, values, errors and kernel (anisotropic Gaussian,
then von Karman):
  loop      [gp.predict_loo(return_var=True) for gp in gps]: per object one factorisation (kept) and the chunked S3e
            substitution of its factor
  batched   treegp_amd.predict_loo_many(gps, return_var=True): one batched factorisation, substitution and row norms for all
            objects, the leave-one-out quantities on the host
each timed from objects without a cached solution or kept factor (dropped before every repetition, outside the timed region),
best of R after a warm-up.  The device phases come from one direct ops.gp_loo_batch call on the same data (timings [0] K
build, [1] Cholesky, [2] sweeps, [3] substitution and norms).  No rate is fixed in advance; the anchors printed at the end are
the batched variance's measured ratios against its loop (predict_many_bench: 6.6x at N = M = 1024, B = 64 and 1.6x at
N = M = 4096, B = 16), a route with about three times the substitution work per problem.  Writes <out>.txt and <out>.json.
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

ANCHORS = {(1024, 64): 6.6, (4096, 16): 1.6}       # batched variance against its loop (README, predict_many_bench)


def objects(n, count, seed, kind):
    rng = np.random.default_rng(seed)
    ell = 1.0 / np.sqrt(np.diag(headline_invlam()))          # the headline field's correlation lengths
    gps = []
    for i in range(count):
        X, y, ye, _ = star_field(n, 1, seed=seed + i)
        s = rng.uniform(0.8, 1.25)
        amp = rng.uniform(0.5, 2.0)
        if kind == "gauss":
            kern = "%r**2 * AnisotropicRBF(scale_length=[%r, %r])" % (float(np.sqrt(amp)), float(s * ell[0]), float(s * ell[1]))
        else:
            kern = "%r**2 * VonKarman(length_scale=%r)" % (float(np.sqrt(amp)), float(4.0 * s * np.sqrt(ell[0] * ell[1])))
        gp = treegp.GPInterpolation(kernel=kern, optimizer="none", normalize=True)
        gp.initialize(X, y, y_err=ye)
        gps.append(gp)
    return gps


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
    ap.add_argument("--cases", default="256:64,1024:64,2048:64,4096:16", help="N:B pairs")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "loo_many_bench"))
    a = ap.parse_args()
    ctx = _lib.get_ctx()
    rows, lines = [], []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for case in a.cases.split(","):
        n, B = [int(v) for v in case.split(":")]
        for kind in ("gauss", "vk"):
            gps = objects(n, B, 1000 * n + B, kind)

            def reset():
                for gp in gps:
                    gp._drop_solution()
            t_loop = best_of(a.reps, reset, lambda: [gp.predict_loo(return_var=True) for gp in gps])
            t_batch = best_of(a.reps, reset, lambda: treegp.predict_loo_many(gps, return_var=True))
            reset()
            worst = max(np.abs(u[1] - v[1]).max() / np.abs(v[1]).max()
                        for u, v in zip(treegp.predict_loo_many(gps[:2], return_var=True),
                                        [gp.predict_loo(return_var=True) for gp in objects(n, 2, 1000 * n + B, kind)]))
            specs = [treegp.kernel_to_spec(gp.kernel) for gp in gps]
            ops.gp_loo_batch(specs, [gp._X for gp in gps], [gp._residual() for gp in gps], [gp._y_err for gp in gps])
            tm = _lib.timings(ctx)
            rows.append(dict(n=n, batch=B, kernel=kind, loop_s=t_loop, batched_s=t_batch, speedup=t_loop / t_batch,
                             var_rel_diff=worst, phases_ms=dict(kbuild=tm[0], cholesky=tm[1], sweeps=tm[2], substitution=tm[3])))
            say("N = %5d  B = %3d  %-5s  loop %9.2f ms  batched %9.2f ms  %5.2fx   device: K %.2f chol %.2f sweeps %.2f "
                "substitution + norms %.2f ms   var_loo agrees to %.1e"
                % (n, B, kind, 1e3 * t_loop, 1e3 * t_batch, t_loop / t_batch, tm[0], tm[1], tm[2], tm[3], worst))
            del gps
    anchors = []
    for (n, B), ratio in sorted(ANCHORS.items()):
        for r in rows:
            if r["n"] == n and r["batch"] == B:
                anchors.append(dict(n=n, batch=B, kernel=r["kernel"], anchor=ratio, speedup=r["speedup"], reached=r["speedup"] >= ratio))
                say("anchor (batched variance against its loop) N = %d, B = %d: %.1fx; leave-one-out %s %.2fx -- %s"
                    % (n, B, ratio, r["kernel"], r["speedup"], "reached" if r["speedup"] >= ratio else "short of it"))
    out = dict(tool="loo_many_bench", hw_queues=os.environ.get("GPU_MAX_HW_QUEUES"), reps=a.reps, rows=rows, anchors=anchors)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(a.out + ".json", "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

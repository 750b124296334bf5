"""Many small GPs at once (seam S2e, tgp_gp_solve_batch) against the ways the same solves ran before, same box, same run.

    python tools/batch_bench.py [--sizes 256,1024,2048,4096] [--batches 1,8,16,64,256] [--reps R] [--json out.json]

For every N, likelihood-only solves (K build + Cholesky + logdet + y.alpha, want_alpha=False: what one evaluation of the
maximum-likelihood fit needs) of B problems with their own coordinates, values, errors and kernel parameters:
  batched      ops.gp_solve_batch over the B problems: B / wall time of the call (best of R after a warm-up)
  single       ops.gp_solve one problem after the other on one context: 1 / wall time per solve (best of R)
  4 contexts   four host threads, each with a context of its own (one stream, as log_likelihood._contexts sets them up),
               each solving problems one after the other: solves / wall time of 64 solves (best of R)
and the last two again on device-resident data (`_res`: ops.ResidentProblem + tgp_d_gp_solve, what the maximum-likelihood
fit does and what bench.py's `likelihood_evaluations_per_sec_4_contexts` measures; the four contexts each have a problem
of their own), plus the device phases of the batched call (timings [0] K build, [1] Cholesky, [2] sweeps and logdet).
Rates are solves per second; the batched call takes host arrays.  Goal (a forecast, not a measurement): >= 4x the
four-context rate at N = 1024 and 2048 with B = 64, >= 1.5x at N = 4096 with B = 16 -- the last lines report it against
both four-context legs.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam               # noqa: E402


def problems(n, count, seed):
    """`count` problems of order n: star fields of their own, anisotropic Gaussian kernels with perturbed parameters"""
    iL = headline_invlam()
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        X, y, ye, _ = star_field(n, 1, seed=seed + i)
        s = rng.uniform(0.8, 1.25)
        out.append((ops.KernelSpec(_lib.TGP_ARBF, amp=rng.uniform(0.5, 2.0), a=s * iL[0, 0], b=s * iL[0, 1], c=s * iL[1, 1]),
                    X, y - y.mean(), ye))
    return out


def best_of(reps, fn):
    fn()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t = time.perf_counter() - t0
        best = t if best is None or t < best else best
    return best


def four_contexts(probs, total, reps):
    lib = _lib.load_library()
    ctxs = []
    for _ in range(4):
        c = _lib.new_ctx(0)
        lib.tgp_set_lookahead(c, 0)
        ctxs.append(c)

    def once():
        def work(t):
            for i in range(t, total, 4):
                p = probs[i % len(probs)]
                ops.gp_solve(p[0], p[1], p[2], p[3], want_alpha=False, ctx=ctxs[t])
        th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    t = best_of(reps, once)
    # the same on device-resident data: each context solves a problem of its own, uploaded once
    res = [ops.ResidentProblem(p[1], p[2], p[3]) for p in probs[:4]]

    def once_res():
        def work(t):
            for _ in range(t, total, 4):
                ops.gp_solve_resident(probs[t][0], res[t], ctx=ctxs[t])
        th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    t_res = best_of(reps, once_res)
    for r in res:
        r.close()
    for c in ctxs:
        lib.tgp_destroy(c)
    return total / t, total / t_res


def single_resident(p, reps, count=16):
    r = ops.ResidentProblem(p[1], p[2], p[3])

    def loop():
        for _ in range(count):
            ops.gp_solve_resident(p[0], r)
    t = best_of(reps, loop)
    r.close()
    return count / t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2048,4096")
    ap.add_argument("--batches", default="1,8,16,64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = _lib.get_ctx()
    # the hardware queues HIP opens per process decide how far four contexts overlap (the loader asks for 8 unless the
    # environment names a number): part of the baseline, so it is printed with it
    print("# GPU_MAX_HW_QUEUES=%s" % os.environ.get("GPU_MAX_HW_QUEUES", "(unset)"), flush=True)
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        batches = [int(b) for b in a.batches.split(",")]
        probs = problems(n, max(batches), 1000 * n)
        p0 = probs[0]
        single = 1.0 / best_of(a.reps, lambda: ops.gp_solve(p0[0], p0[1], p0[2], p0[3], want_alpha=False))
        single_res = single_resident(p0, a.reps)
        four, four_res = four_contexts(probs, 64, a.reps)
        print("N=%5d  single %9.1f /s   4 contexts %9.1f /s   resident data: single %9.1f /s   4 contexts %9.1f /s"
              % (n, single, four, single_res, four_res), flush=True)
        for B in batches:
            sub = probs[:B]
            args = ([p[0] for p in sub], [p[1] for p in sub], [p[2] for p in sub], [p[3] for p in sub])
            res = {}

            def call():
                res["out"] = ops.gp_solve_batch(*args, want_alpha=False)
            t = best_of(a.reps, call)
            assert (res["out"][3] == 0).all()
            tm = _lib.timings(ctx)
            r = dict(N=n, B=B, batched_per_s=round(B / t, 1), wall_ms=round(t * 1e3, 3), kbuild_ms=round(tm[0], 3),
                     chol_ms=round(tm[1], 3), sweeps_ms=round(tm[2], 3), single_per_s=round(single, 1),
                     four_ctx_per_s=round(four, 1), x_four=round(B / t / four, 2), x_single=round(B / t / single, 2),
                     single_res_per_s=round(single_res, 1), four_ctx_res_per_s=round(four_res, 1),
                     x_four_res=round(B / t / four_res, 2), x_single_res=round(B / t / single_res, 2))
            rows.append(r)
            print("N=%5d B=%4d  batched %9.1f /s (%8.3f ms: K %7.3f, Cholesky %8.3f, sweeps %7.3f)  x%.2f of 4 contexts (x%.2f resident), "
                  "x%.2f of single (x%.2f resident)"
                  % (n, B, r["batched_per_s"], r["wall_ms"], r["kbuild_ms"], r["chol_ms"], r["sweeps_ms"], r["x_four"],
                     r["x_four_res"], r["x_single"], r["x_single_res"]), flush=True)
    goals = []
    for n, B, want in ((1024, 64, 4.0), (2048, 64, 4.0), (4096, 16, 1.5)):
        r = [r for r in rows if r["N"] == n and r["B"] == B]
        if not r:
            continue
        r = r[0]
        g = dict(goal="N=%d B=%d >= %.1fx four contexts" % (n, B, want), x_host=r["x_four"], met_host=r["x_four"] >= want,
                 x_resident=r["x_four_res"], met_resident=r["x_four_res"] >= want)
        goals.append(g)
        print("goal %-36s  host-array contexts x%.2f %s   resident contexts x%.2f %s"
              % (g["goal"], g["x_host"], "met" if g["met_host"] else "MISSED", g["x_resident"],
                 "met" if g["met_resident"] else "MISSED"), flush=True)
    rows.append(dict(goals=goals))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

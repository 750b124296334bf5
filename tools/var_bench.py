"""Posterior variance (tgp_gp_predict_var, seam S3c) against the posterior covariance (tgp_gp_predict_cov) on the same kept
factor, and the variance alone at query sets the covariance cannot take.

    python tools/var_bench.py [--big] [--reps R] [--json out.json]

  1. N = 32 768, M = 4096 (the covariance shape of the README): covariance and variance on one factor
  2. the variance alone at N = 8192, M = 32 768 and M = 131 072
  3. --big: N = 65 536, M = 262 144 (the bench's query set; the covariance refuses M > 65 535)
  4. a sweep of the chunk rows Mc through TGP_VAR_CHUNK (4096 / 8192 / 16384 / 32768) at N = 32 768, M = 32 768 and at
     N = 8192, M = 131 072

Flops: M N^2 for the substitution Bt <- HT L^-T (both), 2 M^2 N more for the covariance's Bt Bt^T.  Device times are the
library's own ([3] device compute, [9] result transfer); wall times include the host boundary.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam               # noqa: E402


def _spec():
    iL = headline_invlam()
    return ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=iL[0, 0], b=iL[0, 1], c=iL[1, 1])


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


def _row(rows, what, n, m, wall, dev, d2h, flops, extra=None):
    r = dict(what=what, N=n, M=m, wall_ms=round(wall, 3), device_ms=round(dev, 3), d2h_ms=round(d2h, 3),
             us_per_point=round(1e3 * dev / m, 4), tflops=round(flops / (dev * 1e-3) / 1e12, 2))
    if extra:
        r.update(extra)
    rows.append(r)
    print("%-22s N=%6d M=%7d  device %9.2f ms  d2h %7.2f ms  wall %9.2f ms  %8.4f us/point  %6.2f TF/s%s"
          % (what, n, m, dev, d2h, wall, r["us_per_point"], r["tflops"],
             "" if not extra else "  " + " ".join("%s=%s" % kv for kv in extra.items())), flush=True)


def _factor(spec, n, m, seed=5):
    X, y, ye, Xs = star_field(n, m, seed=seed)
    fac = ops.gp_solve(spec, X, y - y.mean(), ye, keep=True, want_alpha=False)[3]
    return X, Xs, fac


def _with_chunk(rows_env, fn):
    old = os.environ.get("TGP_VAR_CHUNK")
    if rows_env is None:
        os.environ.pop("TGP_VAR_CHUNK", None)
    else:
        os.environ["TGP_VAR_CHUNK"] = str(rows_env)
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("TGP_VAR_CHUNK", None)
        else:
            os.environ["TGP_VAR_CHUNK"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true", help="also N = 65 536, M = 262 144")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    spec = _spec()
    rows = []

    n, m = 32768, 4096
    X, Xs, fac = _factor(spec, n, m)
    wall, dev, d2h, cov = _time(lambda: ops.gp_predict_cov(spec, fac, X, Xs), args.reps)
    _row(rows, "cov", n, m, wall, dev, d2h, m * n * n + 2.0 * m * m * n)
    wall, dev, d2h, var = _time(lambda: ops.gp_predict_var(spec, fac, X, Xs), args.reps)
    _row(rows, "var", n, m, wall, dev, d2h, m * float(n) * n,
         dict(max_abs_diff_vs_diag_cov="%.2e" % np.abs(var - np.diag(cov)).max()))
    del cov
    fac.free()

    for n, m in ((8192, 32768), (8192, 131072)):
        X, Xs, fac = _factor(spec, n, m)
        wall, dev, d2h, var = _time(lambda: ops.gp_predict_var(spec, fac, X, Xs), args.reps)
        _row(rows, "var", n, m, wall, dev, d2h, m * float(n) * n, dict(min_var="%.3e" % var.min()))
        fac.free()

    if not args.no_sweep:
        for n, m in ((32768, 32768), (8192, 131072)):
            X, Xs, fac = _factor(spec, n, m)
            ref = None
            for mc in (4096, 8192, 16384, 32768):
                wall, dev, d2h, var = _with_chunk(mc, lambda: _time(lambda: ops.gp_predict_var(spec, fac, X, Xs), args.reps))
                same = ref is None or np.array_equal(var, ref)
                ref = var if ref is None else ref
                _row(rows, "var Mc=%d" % mc, n, m, wall, dev, d2h, m * float(n) * n, dict(same_bits=same))
            fac.free()

    if args.big:
        n, m = 65536, 262144
        X, Xs, fac = _factor(spec, n, m)
        wall, dev, d2h, var = _time(lambda: ops.gp_predict_var(spec, fac, X, Xs), 1)
        _row(rows, "var (big)", n, m, wall, dev, d2h, m * float(n) * n, dict(min_var="%.3e" % var.min()))
        fac.free()

    if args.json:
        d = os.path.dirname(args.json)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

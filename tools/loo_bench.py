"""diag(K^-1) from a kept factor (tgp_factor_inv_diag, seam S3e: what leave-one-out cross-validation needs) against the
factorisation of the same N, and against the route it replaces: identity rows fed to tgp_gp_predict_var_dense.

    python tools/loo_bench.py [--big] [--reps R] [--no-sweep] [--json out.json]

  1. N = 8192, 16 384, 32 768 (--big: 65 536): the factorisation's device time ([1] of tgp_gp_solve) and
     tgp_factor_inv_diag's ([3]) on the same factor, with the effective rate N^3 / 3 / time
  2. N <= 16 384: the same diagonal as -var of identity rows through tgp_gp_predict_var_dense (N^3 flops of substitution,
     an N x N identity uploaded from the host inside its device interval)
  3. a sweep of the chunk rows through TGP_INVDIAG_CHUNK (4096 / 8192 / 16 384) at N = 32 768

Device times are the library's own ([3] device compute, [9] result transfer); wall times include the host boundary.
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


def _row(rows, what, n, wall, dev, d2h, extra=None):
    flops = float(n) ** 3 / 3.0
    r = dict(what=what, N=n, wall_ms=round(wall, 3), device_ms=round(dev, 3), d2h_ms=round(d2h, 3),
             tflops_n3_over_3=round(flops / (dev * 1e-3) / 1e12, 2))
    if extra:
        r.update(extra)
    rows.append(r)
    print("%-24s N=%6d  device %9.2f ms  d2h %7.2f ms  wall %9.2f ms  %6.2f TF/s (N^3/3)%s"
          % (what, n, dev, d2h, wall, r["tflops_n3_over_3"],
             "" if not extra else "  " + " ".join("%s=%s" % kv for kv in extra.items())), flush=True)


def _factor(spec, n, reps, seed=5):
    """the kept factor and the best device time of its factorisation ([1] of tgp_gp_solve) over `reps` solves"""
    X, y, ye, _ = star_field(n, 1, seed=seed)
    best, fac = None, None
    for _ in range(reps + 1):
        if fac is not None:
            fac.free(keep_memory=True)
        fac = ops.gp_solve(spec, X, y - y.mean(), ye, keep=True, want_alpha=False)[3]
        tm = _lib.timings(_lib.get_ctx())
        best = tm[1] if best is None or tm[1] < best else best
    return fac, best


def _with_chunk(rows_env, fn):
    old = os.environ.get("TGP_INVDIAG_CHUNK")
    if rows_env is None:
        os.environ.pop("TGP_INVDIAG_CHUNK", None)
    else:
        os.environ["TGP_INVDIAG_CHUNK"] = str(rows_env)
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("TGP_INVDIAG_CHUNK", None)
        else:
            os.environ["TGP_INVDIAG_CHUNK"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true", help="also N = 65 536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    spec = _spec()
    rows = []

    sizes = (8192, 16384, 32768) + ((65536,) if args.big else ())
    for n in sizes:
        fac, chol_ms = _factor(spec, n, args.reps)
        _row(rows, "factorisation", n, float("nan"), chol_ms, 0.0)
        wall, dev, d2h, d = _time(lambda: ops.factor_inv_diag(fac), args.reps)
        _row(rows, "inv_diag", n, wall, dev, d2h, dict(vs_factorisation="%.2fx" % (dev / chol_ms)))
        if n <= 16384:
            E, z = np.eye(n), np.zeros(n)
            wall_b, dev_b, d2h_b, v = _time(lambda: ops.gp_predict_var_dense(fac, E, z), args.reps)
            del E
            _row(rows, "identity via var_dense", n, wall_b, dev_b, d2h_b,
                 dict(speedup_inv_diag="%.2fx" % (dev_b / dev), max_rel_diff="%.2e" % np.max(np.abs(-v - d) / d)))
        fac.free()

    if not args.no_sweep:
        n = 32768
        fac, _ = _factor(spec, n, 0)
        ref = None
        for rc in (4096, 8192, 16384):
            wall, dev, d2h, d = _with_chunk(rc, lambda: _time(lambda: ops.factor_inv_diag(fac), args.reps))
            same = ref is None or np.array_equal(d, ref)
            ref = d if ref is None else ref
            _row(rows, "inv_diag R=%d" % rc, n, wall, dev, d2h, dict(same_bits=same))
        fac.free()

    if args.json:
        dn = os.path.dirname(args.json)
        if dn:
            os.makedirs(dn, exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

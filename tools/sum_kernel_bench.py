"""Sums of parametrised kernels on the device (include/tgp.h seams S1s / S2s) against what they replace, same box, same
process, same run.

    python tools/sum_kernel_bench.py [--kbuild 16384,65536] [--api 8192x32768] [--api-big 65536x262144] [--lik 4096]
                                     [--reps 5] [--out profiles/sum_kernel_bench.txt]

  K build      tgp_d_kbuild_lower_sum (device time, timings[0]) for a two-term ARBF + ARBF and AVK + ARBF sum against the SUM of
               the single-kernel tgp_d_kbuild_lower times of its terms.  Forecast: at most that sum (one store per element where
               term-by-term accumulation would store, read and store again), 10 % allowed for box-to-box scatter and the separate
               launches; two Gaussian terms are ~2 x 26 FMA-equivalents per element against the ~32 that hide under the store
               stream (kernel_eval.h), so their arithmetic may show.
  end to end   GPInterpolation.initialize + predict with Sum A on the device route and on the dense route (kernels.device_spec
               patched to raise: the kernel object evaluates itself term by term, the host adds, K and HT cross PCIe), and the
               device route alone at --api-big, where the dense route cannot hold HT.  No threshold.
  likelihood   one likelihood evaluation and one exact-gradient evaluation of Sum A in units of one ops.gp_solve of the sum.

One warm-up, then the median of --reps repetitions (end to end: one warm-up, one timed run).  Rows go to --out as measured.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import treegp_amd as treegp                                                 # noqa: E402
from treegp_amd import _lib, kernels, ops                                   # noqa: E402

ARBF1 = "0.5**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))"
ARBF2 = "0.7**2 * AnisotropicRBF(invLam=array([[300., -40.], [-40., 200.]]))"
AVK = "0.3**2 * AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]]))"
SUM_A = AVK + " + " + ARBF1
KBUILD_SUMS = [("ARBF + ARBF", ARBF1 + " + " + ARBF2), ("AVK + ARBF", SUM_A)]


def problem(n, m, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    y = np.sin(6 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.05 * rng.standard_normal(n)
    return X, y, 0.05 * rng.uniform(0.8, 1.2, n), rng.uniform(0, 1, (m, 2))


def median_of(reps, fn):
    fn()
    out = []
    for _ in range(reps):
        out.append(fn())
    return float(np.median(out))


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kbuild", default="16384,65536")
    ap.add_argument("--api", default="8192x32768")
    ap.add_argument("--api-big", default="65536x262144")
    ap.add_argument("--lik", default="4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "sum_kernel_bench.txt"))
    a = ap.parse_args()
    ctx = _lib.get_ctx()
    lib = _lib.load_library()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    say("# tools/sum_kernel_bench.py --kbuild %s --api %s --api-big %s --lik %s --reps %d" % (a.kbuild, a.api, a.api_big, a.lik, a.reps))
    say("# device times: median of %d after one warm-up" % a.reps)

    for n in [int(v) for v in a.kbuild.split(",") if v]:
        X, _, e, _ = problem(n, 1, n)
        Np = int(lib.tgp_padded_n(n))
        dX, de = ops.DeviceBuffer.from_array(ctx, X), ops.DeviceBuffer.from_array(ctx, e)
        dA = ops.DeviceBuffer(ctx, int(lib.tgp_panel_elems(Np)) * 8)

        def build(spec):
            entry = lib.tgp_d_kbuild_lower_sum if isinstance(spec, ops.KernelSumSpec) else lib.tgp_d_kbuild_lower
            _lib.check(ctx, entry(ctx, C.byref(spec.to_c()), dX.ptr, n, de.ptr, dA.ptr), "kbuild")
            return _lib.timings(ctx)[0]
        for name, kern in KBUILD_SUMS:
            spec = kernels.kernel_to_sum_spec(treegp.eval_kernel(kern))
            t_terms = [median_of(a.reps, lambda t=t: build(t)) for t in spec.terms]
            t_sum = median_of(a.reps, lambda: build(spec))
            ratio = t_sum / sum(t_terms)
            say("kbuild   N = %6d  %-12s fused %8.3f ms   terms %s = %8.3f ms   fused / sum of terms %.3f   %s"
                % (n, name, t_sum, " + ".join("%.3f" % t for t in t_terms), sum(t_terms), ratio,
                   "forecast met (<= 1.10)" if ratio <= 1.10 else "FORECAST MISSED (> 1.10): the fused build is arithmetic-bound"))
        for b in (dX, de, dA):
            b.free()

    def api_run(n, m, dense):
        X, y, e, Xs = problem(n, m, 3 * n)
        real = kernels.device_spec

        def closed(kernel, **kw):
            raise NotImplementedError("dense route forced")
        if dense:
            kernels.device_spec = closed
        try:
            def go():
                gp = treegp.GPInterpolation(kernel=SUM_A, optimizer="none", normalize=True)
                gp.initialize(X, y, y_err=e)
                return gp.predict(Xs)
            go()
            res = {}
            t = wall(lambda: res.setdefault("y", go()))
        finally:
            kernels.device_spec = real
        return t, res["y"]

    for case in [c for c in a.api.split(",") if c]:
        n, m = [int(v) for v in case.split("x")]
        t_dev, y_dev = api_run(n, m, False)
        t_dense, y_dense = api_run(n, m, True)
        say("api      N = %6d  M = %6d  Sum A  initialize + predict: device route %8.3f s   dense route %8.3f s   dense / device "
            "%.2fx   (max |difference| %.2e of max |y|)" % (n, m, t_dev, t_dense, t_dense / t_dev,
                                                           np.abs(y_dev - y_dense).max() / np.abs(y_dense).max()))
    for case in [c for c in a.api_big.split(",") if c]:
        n, m = [int(v) for v in case.split("x")]
        t_dev, _ = api_run(n, m, False)
        say("api      N = %6d  M = %6d  Sum A  initialize + predict: device route %8.3f s   (the dense route would need a %.0f GB "
            "host matrix and a %.0f GB HT)" % (n, m, t_dev, 8e-9 * n * n, 8e-9 * n * m))

    for n in [int(v) for v in a.lik.split(",") if v]:
        X, y, e, _ = problem(n, 1, 5 * n)
        kernel = treegp.eval_kernel(SUM_A)
        spec = kernels.kernel_to_sum_spec(kernel)
        like = treegp.log_likelihood(X, y, e)
        t_solve = median_of(a.reps, lambda: wall(lambda: ops.gp_solve(spec, X, y, e)))
        t_lik = median_of(a.reps, lambda: wall(lambda: like.log_likelihood(kernel)))
        t_grad = median_of(a.reps, lambda: wall(lambda: like.log_likelihood_gradient(kernel, any_kind=True)))
        say("lik      N = %6d  Sum A  one solve %8.2f ms   one likelihood evaluation %8.2f ms = %.2f solves   one exact-gradient "
            "evaluation (%d thetas) %8.2f ms = %.2f solves" % (n, t_solve * 1e3, t_lik * 1e3, t_lik / t_solve, len(kernel.theta),
                                                             t_grad * 1e3, t_grad / t_solve))
    out.close()


if __name__ == "__main__":
    main()

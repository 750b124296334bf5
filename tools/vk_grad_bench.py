"""The exact likelihood gradient of the von Karman kernels (include/tgp.h seam S2h) against the finite-difference route it
replaces, same box, same process, same run.

    python tools/vk_grad_bench.py [--batched 1024x64,2048x64] [--single 4096,16384] [--fits 1024x16] [--fit-single 4096]
                                  [--reps 5] [--out profiles/vk_grad_bench.txt]

For VonKarman (theta = log amp, log ell: ntheta = 2) and AnisotropicVonKarman in 2-D (ntheta = 4), each under a ConstantKernel:

  evaluation, batched   one ops.gp_solve_grad_batch_any call for B problems of order N (value and exact gradient of all of them)
                        against one ops.gp_solve_batch(want_alpha=False) call for the (ntheta + 1) B problems SciPy's forward
                        differences need: what solve_many(gradient="analytic-vk") and solve_many(gradient="fd") issue per iteration
  evaluation, single    one ops.gp_solve_grad_resident_any call against ntheta + 1 ops.gp_solve_resident calls one after the other
                        on ONE context (a fit's own finite differences run them on ntheta + 1 contexts side by side: the whole-fit
                        rows below time that)
  pair pass             timings[3] (inverse and reduction) of the von Karman call beside the same call with the Gaussian kernel of
                        the same invLam at the same n: the difference is what f and w cost over exp
  fits                  solve_many(gps, gradient=...) for B objects and GPInterpolation.solve() under TGP_ML_GRADIENT=... for one:
                        wall time, likelihood-evaluation rounds, final log L, "fd" against "analytic-vk"

One warm-up, then the median of --reps repetitions; fits are timed once after one warm-up fit of the first mode.  Rows are
appended to --out as they are measured.  Forecast from the operation count (not a measurement): the pair pass a few per cent of an
evaluation from N ~ 2048 up; one exact evaluation ~ 3 factorisations' worth for every kind, so about 5/3 over finite differences
for the anisotropic kernel and parity for the isotropic one; anything beyond that from fewer iterations.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import treegp_amd as treegp                                                 # noqa: E402
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.kernels import kernel_to_spec                               # noqa: E402

KERNELS = [("VonKarman", "0.7**2 * VonKarman(length_scale=0.25)", "0.7**2 * RBF(0.25)"),
           ("AnisotropicVonKarman", "0.7**2 * AnisotropicVonKarman(invLam=array([[20., -4.], [-4., 12.]]))",
            "0.7**2 * AnisotropicRBF(invLam=array([[20., -4.], [-4., 12.]]))")]
FD_STEP = 1e-8


def problem(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    y = np.sin(6 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.05 * rng.standard_normal(n)
    return X, y, 0.05 * rng.uniform(0.8, 1.2, n)


def median_of(reps, fn):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def fd_specs(kernel):
    """the ntheta + 1 kernels of one forward-difference gradient"""
    theta = kernel.theta
    out = [kernel_to_spec(kernel)]
    for i in range(len(theta)):
        shifted = np.array(theta, dtype=float)
        shifted[i] += FD_STEP
        out.append(kernel_to_spec(kernel.clone_with_theta(shifted)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batched", default="1024x64,2048x64")
    ap.add_argument("--single", default="4096,16384")
    ap.add_argument("--fits", default="1024x16")
    ap.add_argument("--fit-single", default="4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "vk_grad_bench.txt"))
    a = ap.parse_args()
    ctx = _lib.get_ctx()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    say("# tools/vk_grad_bench.py --batched %s --single %s --fits %s --fit-single %s --reps %d   (GPU_MAX_HW_QUEUES=%s)"
        % (a.batched, a.single, a.fits, a.fit_single, a.reps, os.environ.get("GPU_MAX_HW_QUEUES")))
    say("# times: median of %d after one warm-up; fd = the ntheta + 1 evaluations of one forward-difference gradient" % a.reps)

    for case in [c for c in a.batched.split(",") if c]:
        n, B = [int(v) for v in case.split("x")]
        data = [problem(n, 100 * n + b) for b in range(B)]
        Xs, ys, es = [d[0] for d in data], [d[1] for d in data], [d[2] for d in data]
        for name, kern, gauss in KERNELS:
            k = treegp.eval_kernel(kern)
            pts = fd_specs(k)
            nt = len(pts) - 1
            t_exact = median_of(a.reps, lambda: ops.gp_solve_grad_batch_any([pts[0]] * B, Xs, ys, es))
            tm = _lib.timings(ctx)
            gspec = kernel_to_spec(treegp.eval_kernel(gauss))
            median_of(a.reps, lambda: ops.gp_solve_grad_batch_any([gspec] * B, Xs, ys, es))
            tg = _lib.timings(ctx)
            many = [s for _ in range(B) for s in pts]
            rep = lambda v: [x for x in v for _ in range(nt + 1)]            # noqa: E731
            Xr, yr, er = rep(Xs), rep(ys), rep(es)
            t_fd = median_of(a.reps, lambda: ops.gp_solve_batch(many, Xr, yr, er, want_alpha=False))
            say("batched  N = %5d  B = %3d  %-20s ntheta = %d  exact %8.2f ms  fd (%d B solves) %8.2f ms  fd/exact %5.2fx   "
                "device ms of the exact call: K + Cholesky + sweeps %.2f, inverse + pair pass %.2f (Gaussian kernel, same n: %.2f)"
                % (n, B, name, nt, t_exact * 1e3, nt + 1, t_fd * 1e3, t_fd / t_exact, tm[0] + tm[1] + tm[2], tm[3], tg[3]))

    for n in [int(v) for v in a.single.split(",") if v]:
        X, y, e = problem(n, 7 * n)
        prob = ops.ResidentProblem(X, y, e)
        try:
            for name, kern, gauss in KERNELS:
                pts = fd_specs(treegp.eval_kernel(kern))
                nt = len(pts) - 1
                t_exact = median_of(a.reps, lambda: ops.gp_solve_grad_resident_any(pts[0], prob))
                tm = _lib.timings(ctx)
                gspec = kernel_to_spec(treegp.eval_kernel(gauss))
                median_of(a.reps, lambda: ops.gp_solve_grad_resident_any(gspec, prob))
                tg = _lib.timings(ctx)
                t_one = median_of(a.reps, lambda: ops.gp_solve_resident(pts[0], prob))
                t_fd = median_of(a.reps, lambda: [ops.gp_solve_resident(s, prob) for s in pts])
                say("single   N = %5d           %-20s ntheta = %d  exact %8.2f ms  one solve %8.2f ms  fd (%d solves, one context) "
                    "%8.2f ms  fd/exact %5.2fx  exact/solve %5.2fx   inverse + pair pass %.2f ms (Gaussian kernel, same n: %.2f ms)"
                    % (n, name, nt, t_exact * 1e3, t_one * 1e3, nt + 1, t_fd * 1e3, t_fd / t_exact, t_exact / t_one, tm[3], tg[3]))
        finally:
            prob.close()

    rounds = {"n": 0}
    real_any, real_solve = ops.gp_solve_grad_batch_any, ops.gp_solve_batch

    def count(fn):
        def wrapped(*args, **kw):
            rounds["n"] += 1
            return fn(*args, **kw)
        return wrapped
    for case in [c for c in a.fits.split(",") if c]:
        n, B = [int(v) for v in case.split("x")]
        data = [problem(n, 300 * n + b) for b in range(B)]
        for name, kern, _ in KERNELS:
            def make():
                gps = [treegp.GPInterpolation(kernel=kern, optimizer="log-likelihood", normalize=True) for _ in range(B)]
                for gp, (X, y, e) in zip(gps, data):
                    gp.initialize(X, y, y_err=e)
                return gps
            treegp.solve_many(make()[:2], gradient="fd")                      # warm-up
            row = []
            ops.gp_solve_grad_batch_any, ops.gp_solve_batch = count(real_any), count(real_solve)
            try:
                for mode in ("fd", "analytic-vk"):
                    gps = make()
                    rounds["n"] = 0
                    t0 = time.perf_counter()
                    treegp.solve_many(gps, gradient=mode)
                    dt = time.perf_counter() - t0
                    row.append((mode, dt, rounds["n"] - 1, float(np.mean([gp._optimizer._logL for gp in gps]))))
            finally:
                ops.gp_solve_grad_batch_any, ops.gp_solve_batch = real_any, real_solve
            say("fits     N = %5d  B = %3d  %-20s " % (n, B, name)
                + "   ".join("%s: %.3f s, %d rounds, mean log L %.6f" % r for r in row) + "   fd/analytic-vk %5.2fx" % (row[0][1] / row[1][1]))

    for n in [int(v) for v in a.fit_single.split(",") if v]:
        X, y, e = problem(n, 900 * n)
        for name, kern, _ in KERNELS:
            row = []
            for mode in ("fd", "analytic-vk"):
                os.environ["TGP_ML_GRADIENT"] = mode
                gp = treegp.GPInterpolation(kernel=kern, optimizer="log-likelihood", normalize=True)
                gp.initialize(X, y, y_err=e)
                if not row:
                    gp.solve()                                                # warm-up
                    gp.initialize(X, y, y_err=e)
                t0 = time.perf_counter()
                gp.solve()
                row.append((mode, time.perf_counter() - t0, float(gp._optimizer._logL)))
            os.environ.pop("TGP_ML_GRADIENT", None)
            say("fit      N = %5d           %-20s " % (n, name) + "   ".join("%s: %.3f s, log L %.6f" % r for r in row)
                + "   fd/analytic-vk %5.2fx" % (row[0][1] / row[1][1]))
    out.close()


if __name__ == "__main__":
    main()

"""Sums of kernels through the batched routes (seam S2i of include/tgp.h) against the routes the same objects took before, same
box, same process.

    python tools/sum_batch_bench.py [--shapes 64x256,64x1024,64x2048,16x4096] [--reps R] [--fit-objects 16] [--out file.txt]

Kernels: "avk+arbf" (0.3**2 * AnisotropicVonKarman + 0.5**2 * AnisotropicRBF, an atmospheric term plus a long-range optical one)
and "arbf+arbf" (two Gaussian terms: the launch list whose kernels carry no Bessel evaluator).  Every problem has a star field
of its own and perturbed parameters.  The C entries are called on arrays padded once, after a warm-up; the figure is the median
of R calls.

(a) cost of the sum: tgp_gp_solve_batch_sum (likelihood only: alpha = NULL) against tgp_gp_solve_batch of the first term alone
    on the same data, wall time and K-build phase (timings[0]) of each, and the K-build phase of the second term alone: the
    sum's build against the sum of its terms' one-term batched builds.
(b) what users gain: evaluations per second of the batched sum against the loop of single ops.gp_solve calls of the same
    KernelSumSpec on one context (the route of these objects before the batch took sums).
(c) the fit: one solve_many of --fit-objects avk+arbf objects at N = 1024 against the loop of their own solve(), with finite
    differences (the default) and with the exact gradient (gradient="analytic-vk" / TGP_ML_GRADIENT=analytic-vk).
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import treegp_amd as tg                                                      # noqa: E402
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field                                 # noqa: E402

AVK = dict(amp=0.09, a=40.0, b=-9.0, c=25.0)
ARBF = dict(amp=0.25, a=30.0, b=4.0, c=20.0)
ARBF2 = dict(amp=0.49, a=300.0, b=40.0, c=200.0)
KERNELS = {"avk+arbf": ((_lib.TGP_AVK, AVK), (_lib.TGP_ARBF, ARBF)), "arbf+arbf": ((_lib.TGP_ARBF, ARBF2), (_lib.TGP_ARBF, ARBF))}
FIT_KERNEL = ("0.3**2 * AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]])) + "
              "0.5**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))")


def problems(which, n, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        X, y, ye, _ = star_field(n, 1, seed=seed + i)
        terms = []
        for kind, kw in KERNELS[which]:
            s = rng.uniform(0.8, 1.25)
            terms.append(ops.KernelSpec(kind, amp=kw["amp"] * rng.uniform(0.8, 1.25), a=s * kw["a"], b=s * kw["b"], c=s * kw["c"]))
        out.append((ops.KernelSumSpec(terms), X, y - y.mean(), ye))
    return out


def median_of(reps, fn):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


class Batch(object):
    """the padded arrays of one batch, made once"""

    def __init__(self, probs):
        self.nb = len(probs)
        self.ns, self.nmax, self.X, self.y, self.e = ops.pad_batch([p[1] for p in probs], [p[2] for p in probs], [p[3] for p in probs])
        self.sums = (_lib.TgpKernelSum * self.nb)(*[p[0].to_c() for p in probs])
        self.term = [(_lib.TgpKernel * self.nb)(*[p[0].terms[t].to_c() for p in probs]) for t in range(2)]
        self.logdet, self.chi2, self.info = np.empty(self.nb), np.empty(self.nb), np.zeros(self.nb, dtype=np.int32)

    def call(self, lib, ctx, name, ks):
        p = _lib.ptr
        rc = getattr(lib, name)(ctx, self.nb, ks, p(self.ns), self.nmax, p(self.X), p(self.y), p(self.e), None, p(self.logdet),
                                p(self.chi2), p(self.info))
        _lib.check(ctx, rc, name)
        assert not self.info.any(), (name, self.info)


def cost_and_gain(say, lib, ctx, shapes, reps):
    for which in KERNELS:
        for B, n in shapes:
            probs = problems(which, n, B, 1000 * n)
            bt = Batch(probs)
            row = {}
            for tag, name, ks in (("sum", "tgp_gp_solve_batch_sum", bt.sums),
                                  ("term0", "tgp_gp_solve_batch", C.cast(bt.term[0], C.c_void_p)),
                                  ("term1", "tgp_gp_solve_batch", C.cast(bt.term[1], C.c_void_p))):
                t = median_of(reps, lambda: bt.call(lib, ctx, name, ks))
                row[tag] = (t, _lib.timings(ctx)[0])
            (ts, ks_), (t0, k0), (_, k1) = row["sum"], row["term0"], row["term1"]
            say("(a) %-9s B=%3d N=%5d  sum %8.3f ms (K build %7.3f)  first term alone %8.3f ms (K build %7.3f)  second term's K build "
                "%7.3f  | whole call x%.3f, K build x%.3f of the first term's, x%.3f of both terms' builds"
                % (which, B, n, ts * 1e3, ks_, t0 * 1e3, k0, k1, ts / t0, ks_ / k0, ks_ / (k0 + k1)))
            loop = median_of(reps, lambda: [ops.gp_solve(p[0], p[1], p[2], p[3], want_alpha=False) for p in probs[:min(B, 16)]])
            single = min(B, 16) / loop
            say("(b) %-9s B=%3d N=%5d  batched sum %9.1f evaluations/s   loop of single gp_solve %9.1f /s   x%.2f"
                % (which, B, n, B / ts, single, B / ts / single))


def fit_objects(count, n):
    gps = []
    for b in range(count):
        X, y, ye, _ = star_field(n, 1, seed=7000 + b)
        gp = tg.GPInterpolation(kernel=FIT_KERNEL, optimizer="log-likelihood", normalize=True)
        gp.initialize(X, y, y_err=ye)
        gps.append(gp)
    return gps


def fits(say, count, n):
    for route, env in (("auto", None), ("analytic-vk", "analytic-vk")):
        old = os.environ.get("TGP_ML_GRADIENT")
        if env is None:
            os.environ.pop("TGP_ML_GRADIENT", None)
        else:
            os.environ["TGP_ML_GRADIENT"] = env
        try:
            own = fit_objects(count, n)
            t0 = time.perf_counter()
            for gp in own:
                gp.solve()
            t_loop = time.perf_counter() - t0
        finally:
            if old is None:
                os.environ.pop("TGP_ML_GRADIENT", None)
            else:
                os.environ["TGP_ML_GRADIENT"] = old
        many = fit_objects(count, n)
        t0 = time.perf_counter()
        tg.solve_many(many, gradient=route)
        t_many = time.perf_counter() - t0
        worst = max((o._optimizer._logL - m._optimizer._logL) / abs(o._optimizer._logL) for o, m in zip(own, many))
        say("(c) %-11s B=%3d N=%5d  solve_many %8.2f s   loop of solve() %8.2f s   x%.2f   (log L of solve_many at worst %.1e "
            "relative below its own solve()'s)" % (route, count, n, t_many, t_loop, t_loop / t_many, max(worst, 0.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x256,64x1024,64x2048,16x4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-objects", type=int, default=16)
    ap.add_argument("--fit-n", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if a.out:                                        # written as it goes: a run cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    say("# tools/sum_batch_bench.py --shapes %s --reps %d --fit-objects %d --fit-n %d   (median of the repetitions after a warm-up; "
        "GPU_MAX_HW_QUEUES=%s)" % (a.shapes, a.reps, a.fit_objects, a.fit_n, os.environ.get("GPU_MAX_HW_QUEUES", "(unset)")))
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    cost_and_gain(say, lib, ctx, shapes, a.reps)
    if a.fit_objects > 0:
        fits(say, a.fit_objects, a.fit_n)


if __name__ == "__main__":
    main()

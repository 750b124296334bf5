"""The gradient of the predicted mean (tgp_d_gp_predict_grad, seam S3g) against the fused predict (tgp_d_gp_predict) it shares
its decomposition with: same data, same run, the two calls alternating.

    python tools/predict_grad_bench.py [--reps R] [--out profiles/predict_grad_bench.txt]

Sizes N = 65 536 / M = 262 144 and N = 8192 / M = 32 768; kernel forms: Gaussian (the headline invLam, fast path), VonKarman,
AnisotropicVonKarman.  Times are the library's own device interval (timings[3]: HIP events around the launches of one call,
transfers excluded, data resident); each call is warmed up once, then `reps` rounds alternate predict / gradient and the
median and the spread (min .. max) of each are reported with the pair rate N M / time and the ratio predict / gradient of the
medians.  Nothing here is a pass criterion.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam               # noqa: E402

SIZES = ((65536, 262144), (8192, 32768))


def specs():
    iL = headline_invlam()
    a, b, c = iL[0, 0], iL[0, 1], iL[1, 1]
    # von Karman lengths of the order of the Gaussian's: most pairs inside the cutoff, all branches of the Bessel code in use
    return (("gauss", ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=a, b=b, c=c)),
            ("vk", ops.KernelSpec(_lib.TGP_VK, amp=1.0, ell=1.0 / np.sqrt(0.5 * (a + c)))),
            ("avk", ops.KernelSpec(_lib.TGP_AVK, amp=1.0, a=a, b=b, c=c)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "predict_grad_bench.txt"))
    args = ap.parse_args()
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    lines = ["# tools/predict_grad_bench.py --reps %d : device ms (timings[3]), median (min .. max) of %d alternating rounds"
             % (args.reps, args.reps), "# %s" % lib.tgp_version().decode()]
    for n, m in SIZES:
        X, y, _, Xs = star_field(n, m, seed=3)
        alpha = np.random.default_rng(1).standard_normal(n) / n
        bufs = [ops.DeviceBuffer.from_array(ctx, a) for a in (X, alpha, Xs)] + [ops.DeviceBuffer(ctx, m * 8), ops.DeviceBuffer(ctx, m * 16)]
        dX, da, dXs, dys, dgs = [b.ptr for b in bufs]
        for name, spec in specs():
            k = C.byref(spec.to_c())

            def predict():
                _lib.check(ctx, lib.tgp_d_gp_predict(ctx, k, dX, n, da, dXs, m, dys), "tgp_d_gp_predict")
                return _lib.timings(ctx)[3]

            def grad():
                _lib.check(ctx, lib.tgp_d_gp_predict_grad(ctx, k, dX, n, da, dXs, m, dgs), "tgp_d_gp_predict_grad")
                return _lib.timings(ctx)[3]
            predict(), grad()
            tp, tg = [], []
            for _ in range(args.reps):
                tp.append(predict())
                tg.append(grad())
            mp_, mg = float(np.median(tp)), float(np.median(tg))
            g = bufs[4].to_array((m, 2))
            assert np.all(np.isfinite(g)) and np.any(g != 0.0)
            line = ("N=%6d M=%6d %-5s  predict %8.3f ms (%.3f .. %.3f) %.3e pairs/s   gradient %8.3f ms (%.3f .. %.3f) %.3e pairs/s"
                    "   predict / gradient = %.3f" % (n, m, name, mp_, min(tp), max(tp), n * m / (mp_ * 1e-3), mg, min(tg), max(tg),
                                                      n * m / (mg * 1e-3), mp_ / mg))
            print(line, flush=True)
            lines.append(line)
        for b in bufs:
            b.free()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

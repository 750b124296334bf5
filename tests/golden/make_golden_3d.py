#!/usr/bin/env python3
"""Generate tests/golden/g15_3d.npz by running the REFERENCE itself on 3-D coordinates.

Run in the build container only (needs /root/reference; the import recipe is make_golden.py's):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_3d.py

The reference's kernels take coordinates of any dimension (kernels.py hands pdist / cdist whatever invLam it is given, VonKarman
and scikit-learn's RBF use Euclidean distances) and GPInterpolation never looks at the number of columns outside the 2-point
correlation optimisers and the mean-function table.  Contents (inputs + the reference's outputs, nothing else):

  X (300, 3), y, y_err = 0.01, Xs (70, 3)                       fixed seed, normalize=True, optimizer="none"
  per kernel tag in arbf / avk / rbf / vk:
    <tag>_kernel      the kernel string
    <tag>_self        K(X[:96])            <tag>_cross   K(Xs, X[:96])
    <tag>_alpha       gp._alpha            <tag>_y_pred  predict(Xs)       <tag>_cov64  predict(Xs, return_cov=True)[1][:64, :64]
    <tag>_thetas      three thetas         <tag>_logL    return_log_likelihood at each of them
  fit_*               one 120-point optimizer="log-likelihood" fit (RBF with three length scales): data, start kernel, the
                      fitted theta and its log-likelihood
"""
import os

import numpy as np

from make_golden import load_reference

OUT = os.path.dirname(os.path.abspath(__file__))

INVLAM = "array([[30., 4., -3.], [4., 20., 5.], [-3., 5., 12.]])"
KERNELS = (
    ("arbf", "0.8**2 * AnisotropicRBF(invLam=%s)" % INVLAM),
    ("avk", "0.8**2 * AnisotropicVonKarman(invLam=%s)" % INVLAM),
    ("rbf", "0.8**2 * RBF([0.2, 0.3, 0.5])"),
    ("vk", "0.8**2 * VonKarman(length_scale=0.4)"),
)


def field(X):
    return (np.sin(3.0 * X[:, 0]) + np.cos(2.0 * X[:, 1]) * (0.5 + X[:, 2]) + 0.3 * np.sin(5.0 * X[:, 0] * X[:, 2] + X[:, 1]))


def main():
    tg = load_reference()
    GP = tg.GPInterpolation
    rng = np.random.default_rng(1503)
    n, m = 300, 70
    X = rng.uniform(0.0, 1.0, (n, 3))
    Xs = rng.uniform(0.0, 1.0, (m, 3))
    Xs[:3] = X[:3]                                   # coincident query points
    y_err = 0.01 * np.ones(n)
    y = field(X) + y_err * rng.standard_normal(n)
    out = dict(X=X, y=y, y_err=y_err, Xs=Xs)
    for tag, kern in KERNELS:
        k = tg.eval_kernel(kern)
        gp = GP(kernel=kern, optimizer="none", normalize=True)
        gp.initialize(X, y, y_err=y_err)
        y_pred, cov = gp.predict(Xs, return_cov=True)
        theta0 = np.array(gp.kernel.theta, dtype=float)
        thetas = np.stack([theta0, theta0 + 0.1, theta0 - 0.07 * np.arange(1, len(theta0) + 1) / len(theta0)])
        out.update({tag + "_kernel": kern, tag + "_self": k(X[:96]), tag + "_cross": k(Xs, Y=X[:96]),
                    tag + "_alpha": np.ravel(gp._alpha), tag + "_y_pred": y_pred, tag + "_cov64": cov[:64, :64],
                    tag + "_thetas": thetas, tag + "_logL": np.array([gp.return_log_likelihood(theta=t) for t in thetas])})
        print(tag, "cond(K + 1e-4 I) = %.3g" % np.linalg.cond(k(X) + 1e-4 * np.eye(n)))
    # one maximum-likelihood fit: 120 points in [0, 2]^3 drawn from a known kernel
    rng = np.random.default_rng(1504)
    Xf = rng.uniform(0.0, 2.0, (120, 3))
    ktrue = tg.eval_kernel("1.0**2 * RBF([0.35, 0.5, 0.8])")
    yf = rng.multivariate_normal(np.zeros(120), ktrue(Xf)) + 0.05 * rng.standard_normal(120)
    k0 = "0.7**2 * RBF([0.5, 0.5, 0.5])"
    gp = GP(kernel=k0, optimizer="log-likelihood", normalize=True)
    gp.initialize(Xf, yf, y_err=0.05 * np.ones(120))
    gp.solve()
    out.update(fit_X=Xf, fit_y=yf, fit_y_err=0.05 * np.ones(120), fit_kernel0=k0, fit_theta=np.array(gp.kernel.theta),
               fit_logL=gp._optimizer._logL, fit_theta_true=np.array(ktrue.theta))
    print("fit theta", gp.kernel.theta, "true", ktrue.theta, "logL", gp._optimizer._logL)
    np.savez(os.path.join(OUT, "g15_3d.npz"), **out)


if __name__ == "__main__":
    main()

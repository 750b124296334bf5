#!/usr/bin/env python3
"""Generate tests/golden/g16_fisher.npz from the REFERENCE's own kernel derivatives.

Needs the reference project (the import recipe is make_golden.py's):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fisher.py

The reference has no Fisher information; it has ``kernel(X, eval_gradient=True)`` for AnisotropicRBF (kernels.py:128-150) and
scikit-learn's for ConstantKernel and RBF.  From those (n, n, ntheta) derivative matrices NumPy forms

    F_theta[i][j] = 1/2 tr(C dK/dtheta_i C dK/dtheta_j),    C = (K + diag(y_err^2))^-1

on input set A of tests/_vk_loglik_grad_refs.py at n = 200.  The reference is evaluated BEFORE anything of this package is
imported: its eval_kernel collects every loaded Kernel subclass and would pick up this package's classes.  Contents (data only):

  X (200, 2), y_err (200,)
  per kernel tag in arbf / rbf:   <tag>_kernel  the kernel string,   <tag>_F  F_theta (ntheta, ntheta)
"""
import os
import sys

import numpy as np

from make_golden import load_reference

OUT = os.path.dirname(os.path.abspath(__file__))
KERNELS = (
    ("arbf", "0.7**2 * AnisotropicRBF(invLam=array([[40., -9.], [-9., 25.]]))"),
    ("rbf", "0.7**2 * RBF(0.2)"),
)


def data_a(n):
    """input set A of tests/_vk_loglik_grad_refs.py, restated so that nothing of this package is imported here"""
    rng = np.random.default_rng(100 + n)
    X = rng.uniform(0, 1, (n, 2))
    rng.standard_normal(n)                              # (y: drawn to keep the stream in step, not used)
    y_err = 0.1 * rng.uniform(0.8, 1.2, n)
    return X, y_err


def fisher_theta(k, X, y_err):
    K, dK = k(X, eval_gradient=True)
    C = np.linalg.inv(K + np.diag(y_err ** 2))
    CD = [C.dot(dK[:, :, i]) for i in range(dK.shape[2])]
    return np.array([[0.5 * np.sum(a * b.T) for b in CD] for a in CD])


def main():
    tg = load_reference()
    assert "treegp_amd" not in sys.modules
    X, y_err = data_a(200)
    out = dict(X=X, y_err=y_err)
    for tag, kern in KERNELS:
        k = tg.eval_kernel(kern)
        F = fisher_theta(k, X, y_err)
        out[tag + "_kernel"] = kern
        out[tag + "_F"] = F
        print(tag, "theta", k.theta, "F diag", np.diag(F), "asymmetry %.2e" % np.abs(F - F.T).max())
    np.savez(os.path.join(OUT, "g16_fisher.npz"), **out)


if __name__ == "__main__":
    main()

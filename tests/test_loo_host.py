"""CPU-only checks of leave-one-out cross-validation (seam S3e, tgp_factor_inv_diag): the C-ABI surface, the argument checks
that run before any device work, and the host formulas of treegp_amd.loo against brute force (delete the point, solve)."""
import os
import re

import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib, ops
from treegp_amd.loo import loo_quantities

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inv_diag_entry_point_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tgp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tgp_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()
    assert "tgp_factor_inv_diag" in declared
    assert "tgp_factor_inv_diag" in _lib.SIGNATURES
    assert hasattr(lib, "tgp_factor_inv_diag"), "libtgp.so does not export tgp_factor_inv_diag"
    restype, argtypes = _lib.SIGNATURES["tgp_factor_inv_diag"]
    assert len(argtypes) == 3                                   # (ctx, factor, d)


def test_arguments_are_refused_before_device_work():
    with pytest.raises(ValueError, match="kept factor"):
        ops.factor_inv_diag(None)
    freed = ops.Factor(None, None, 10)                          # a handle whose memory is gone
    with pytest.raises(ValueError, match="kept factor"):
        ops.factor_inv_diag(freed)
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (16, 2))
    gp = tg.GPInterpolation(kernel="1.0**2 * RBF(0.3)", optimizer="none")
    gp.initialize(X, np.sin(X[:, 0]))
    with pytest.raises(ValueError, match="n_fields, 16"):
        gp.predict_fields_loo(np.zeros((3, 15)))
    assert gp._alpha is None and gp._factor is None
    with pytest.raises(ValueError, match="same shape"):
        loo_quantities(np.zeros(4), np.zeros(5), np.ones(4), np.zeros(4))


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K0 = 1.3 * np.exp(-0.5 * d2 / 0.25 ** 2)                    # latent covariance
    sigma = rng.uniform(0.05, 0.3, n)
    return rng, K0, sigma


def _brute(K0, sigma, r, i):
    keep = np.delete(np.arange(len(r)), i)
    Km = K0[np.ix_(keep, keep)] + np.diag(sigma[keep] ** 2)
    k = K0[i, keep]
    w = np.linalg.solve(Km, k)
    mu = w.dot(r[keep])
    v = K0[i, i] - k.dot(w)
    s = v + sigma[i] ** 2
    logp = -0.5 * np.log(2 * np.pi * s) - 0.5 * (r[i] - mu) ** 2 / s
    return mu, s, v, logp


@pytest.mark.parametrize("n", [2, 7, 40])
def test_loo_formulas_against_deleting_the_point(n):
    rng, K0, sigma = _spd(n, 10 + n)
    K = K0 + np.diag(sigma ** 2)
    r = rng.standard_normal(n)
    alpha = np.linalg.solve(K, r)
    d = np.diag(np.linalg.inv(K))
    mu, s, v, logp = loo_quantities(r, alpha, d, sigma)
    for i in range(n):
        ref = _brute(K0, sigma, r, i)
        for got, want in zip((mu[i], s[i], v[i], logp[i]), ref):
            assert abs(got - want) <= 1e-12 * max(abs(want), 1.0), (i, got, want)


def test_loo_formulas_on_a_stack_of_residuals():
    rng, K0, sigma = _spd(25, 4)
    K = K0 + np.diag(sigma ** 2)
    R = rng.standard_normal((3, 25))
    A = np.linalg.solve(K, R.T).T
    d = np.diag(np.linalg.inv(K))
    mu, s, v, logp = loo_quantities(R, A, d, sigma)
    assert mu.shape == logp.shape == (3, 25) and s.shape == v.shape == (25,)     # the variances do not depend on the field
    for f in range(3):
        mu1, s1, v1, logp1 = loo_quantities(R[f], A[f], d, sigma)
        assert np.array_equal(mu[f], mu1) and np.array_equal(logp[f], logp1)
        assert np.array_equal(s, s1) and np.array_equal(v, v1)

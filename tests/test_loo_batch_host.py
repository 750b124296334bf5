"""CPU-only checks of predict_loo_many / loo_log_predictive_many (seam S2g): the device calls are replaced by NumPy stand-ins,
so these tests check routing, order, caching, values against the single-object methods and the error paths, not the kernels."""
import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib, ops
from treegp_amd import gp_interp


def spec_matrix(spec, X):
    X = _lib.as_xy(X)
    d = X[:, None, :] - X[None, :, :]
    q = spec.a * d[..., 0] ** 2 + 2 * spec.b * d[..., 0] * d[..., 1] + spec.c * d[..., 1] ** 2
    return spec.amp * np.exp(-0.5 * q)


def host_solve(K, y, y_err):
    """(alpha, L) of K + diag(y_err^2); numpy.linalg.LinAlgError when it is not positive definite"""
    K = np.array(K, dtype=np.float64)
    K[np.diag_indices(len(K))] += np.asarray(y_err, dtype=np.float64) ** 2
    L = np.linalg.cholesky(K)
    return np.linalg.solve(L.T, np.linalg.solve(L, y)), L


def host_inv_diag(L):
    B = np.linalg.solve(L, np.eye(len(L)))
    return (B * B).sum(axis=0)


class HostFactor(object):
    def __init__(self, L):
        self.L, self.freed = L, False

    def free(self, keep_memory=False):
        self.freed = True


BAD_LENGTH = 2.5          # a kernel with this RBF length scale fails its factorisation in the stand-ins (info > 0)


@pytest.fixture
def fake(monkeypatch):
    """single and batched routes on the host; the kernel marked by BAD_LENGTH gets a negative amp: not positive definite"""
    rec = {"loo": [], "singles": [], "dense": []}

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["singles"].append(len(X))
        alpha, L = host_solve(spec_matrix(spec, X), y, y_err)
        return alpha, 0.0, 0.0, (HostFactor(L) if keep else None)

    def gp_solve_dense(K, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["dense"].append(len(K))
        alpha, L = host_solve(K, y, y_err)
        return alpha, 0.0, 0.0, (HostFactor(L) if keep else None)

    def gp_loo_batch(specs, Xs, ys, y_errs=None, ctx=None):
        rec["loo"].append([len(X) for X in Xs])
        alphas, ds, info = [], [], []
        for s, X, y, e in zip(specs, Xs, ys, y_errs):
            if s.amp < 0:
                alphas.append(np.full(len(X), np.nan)), ds.append(np.full(len(X), np.nan)), info.append(1)
                continue
            alpha, L = host_solve(spec_matrix(s, X), y, e)
            alphas.append(alpha), ds.append(host_inv_diag(L)), info.append(0)
        return alphas, ds, np.zeros(len(specs)), np.zeros(len(specs)), np.array(info)

    def other_batch(*a, **k):
        raise AssertionError("the leave-one-out route calls gp_loo_batch alone")

    real_spec = gp_interp.kernel_to_spec

    def spec_of(k):
        s = real_spec(k)
        if abs(s.a - 1.0 / BAD_LENGTH ** 2) < 1e-12:
            s.amp = -1.0
        return s

    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(gp_interp, "kernel_to_spec", spec_of)
    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_solve_dense", gp_solve_dense)
    monkeypatch.setattr(ops, "gp_loo_batch", gp_loo_batch)
    monkeypatch.setattr(ops, "gp_solve_batch", other_batch)
    monkeypatch.setattr(ops, "gp_posterior_batch", other_batch)
    monkeypatch.setattr(ops, "gp_solve_grad_batch", other_batch)
    monkeypatch.setattr(ops, "factor_inv_diag", lambda f, ctx=None: host_inv_diag(f.L))
    return rec


def make_gp(n, seed, kernel="1.0**2 * RBF(1.5)", normalize=True, white_noise=0.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, 2))
    gp = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=normalize, white_noise=white_noise)
    gp.initialize(X, np.sin(X[:, 0]) + 0.4 + 0.1 * rng.standard_normal(n), y_err=rng.uniform(0.1, 0.2, n))
    return gp


TREE = "RBF(1.0) + WhiteKernel(0.01)"


def test_routing_order_and_caching(fake, monkeypatch):
    """a, b, cached: batched, in list order; big: n > 4096; tree: a kernel tree outside kernel_to_spec; dist: the multi-GPU
    route; kept: a kept factor of its own data.  Those four go through their own predict_loo."""
    a, b, big = make_gp(30, 1), make_gp(40, 2), make_gp(ops.BATCH_NMAX + 1, 3)
    tree = make_gp(25, 4, kernel=TREE)
    cached = make_gp(20, 5)
    cached._alpha = np.zeros(20)
    dist = make_gp(15, 6)
    dist.backend = "dist"
    monkeypatch.setattr(dist, "predict_loo", lambda return_var=False: "dist-loo")
    kept = make_gp(35, 7)
    kept_ref = kept.predict_loo(return_var=True)
    kept_factor, kept_alpha, cached_alpha = kept._factor, kept._alpha, cached._alpha
    assert kept_factor is not None
    fake["singles"].clear()
    gps = [a, big, tree, b, cached, dist, kept]
    out = tg.predict_loo_many(gps, return_var=True)
    assert fake["loo"] == [[30, 40, 20]]
    assert fake["singles"] == [ops.BATCH_NMAX + 1] and fake["dense"] == [25]
    assert out[5] == "dist-loo"
    assert cached._alpha is cached_alpha and kept._factor is kept_factor and kept._alpha is kept_alpha
    assert not kept_factor.freed
    for g in (a, b, cached):
        assert g._alpha is not None and g._factor is None
    assert big._factor is not None and tree._factor is not None          # what their own predict_loo leaves
    for i, g in enumerate(gps):
        if i == 5:
            continue
        y, v = out[i]
        assert y.shape == v.shape == (len(g._X),), i
    np.testing.assert_allclose(out[6][0], kept_ref[0], rtol=0, atol=0)
    np.testing.assert_allclose(out[6][1], kept_ref[1], rtol=0, atol=0)
    # the cached (zero) alpha is the one used: mu = r - 0 / d
    np.testing.assert_allclose(out[4][0], cached._y, rtol=1e-13)
    # without return_var: the same y_loo, a plain list of arrays
    plain = tg.predict_loo_many([a, b])
    assert fake["loo"][-1] == [30, 40]
    for p, i in zip(plain, (0, 3)):
        assert isinstance(p, np.ndarray)
        np.testing.assert_allclose(p, out[i][0], rtol=1e-13)


@pytest.mark.parametrize("normalize,white_noise", [(True, 0.0), (False, 0.0), (True, 0.05), (False, 0.05)])
def test_values_equal_predict_loo_of_fresh_copies(fake, normalize, white_noise):
    def fresh():
        return [make_gp(n, s, kernel=k, normalize=normalize, white_noise=white_noise)
                for n, s, k in ((30, 1, "1.0**2 * RBF(1.5)"), (25, 4, TREE), (41, 2, "0.7**2 * RBF(0.8)"), (1, 9, "1.0**2 * RBF(1.5)"))]
    got = tg.predict_loo_many(fresh(), return_var=True)
    assert fake["loo"] == [[30, 41, 1]] and fake["singles"] == []
    for (y, v), ref in zip(got, fresh()):
        ry, rv = ref.predict_loo(return_var=True)
        np.testing.assert_allclose(y, ry, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(v, rv, rtol=1e-12, atol=1e-13)
    scores = tg.loo_log_predictive_many(fresh())
    assert scores.dtype == np.float64 and scores.shape == (4,)
    for s, ref in zip(scores, fresh()):
        np.testing.assert_allclose(s, ref.return_loo_log_predictive(), rtol=1e-12)


def test_failed_factorisation_names_the_object_and_caches_nothing(fake):
    a, b, c = make_gp(30, 1), make_gp(40, 2), make_gp(20, 3, kernel="1.0**2 * RBF(%r)" % BAD_LENGTH)
    with pytest.raises(np.linalg.LinAlgError, match="GP 2"):
        tg.predict_loo_many([a, b, c], return_var=True)
    assert a._alpha is None and b._alpha is None and c._alpha is None
    scores = tg.loo_log_predictive_many([a, b, c])
    assert scores[2] == -np.inf and np.all(np.isfinite(scores[:2]))
    assert fake["loo"] == [[30, 40, 20]] * 2 and fake["singles"] == []
    for g in (a, b, c):
        assert g._alpha is None and g._factor is None


def test_thetas_are_cloned_into_a_copy_of_the_kernel(fake):
    a, b, tree = make_gp(30, 1), make_gp(40, 2), make_gp(25, 4, kernel=TREE)
    kept = make_gp(35, 7)
    kept.predict_loo()
    kept_factor, kept_alpha = kept._factor, kept._alpha
    gps = [a, tree, b, kept]
    before = [g.kernel.theta.copy() for g in gps]
    thetas = [a.kernel.theta + 0.1, tree.kernel.theta - 0.2, None, kept.kernel.theta + 0.3]
    fake["singles"].clear()
    got = tg.loo_log_predictive_many(gps, thetas)
    assert fake["loo"] == [[30, 40, 35]] and fake["singles"] == [] and fake["dense"] == [25]     # a kept factor excludes nobody here
    for g, th0 in zip(gps, before):
        assert np.array_equal(g.kernel.theta, th0)
        assert g._factor is (kept_factor if g is kept else None) and g._alpha is (kept_alpha if g is kept else None)
    for s, g, th in zip(got, gps, thetas):
        np.testing.assert_allclose(s, g.return_loo_log_predictive(th), rtol=1e-12)
    assert got[0] != tg.loo_log_predictive_many([a])[0]
    np.testing.assert_allclose(tg.loo_log_predictive_many(gps, [None] * 4), [g.return_loo_log_predictive() for g in gps], rtol=1e-12)


def test_list_lengths_are_refused_before_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "get_ctx", no_device)
    monkeypatch.setattr(_lib, "load_library", no_device)
    a = make_gp(10, 1)
    with pytest.raises(ValueError, match="thetas"):
        tg.loo_log_predictive_many([a], [None, None])
    with pytest.raises(ValueError):
        tg.loo_log_predictive_many([a, a], [None])
    one = ([ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(3)])
    with pytest.raises(ValueError):
        ops.gp_loo_batch([ops.KernelSpec(0)] * 2, one[1], one[2])
    with pytest.raises(ValueError):
        ops.gp_loo_batch(one[0], one[1], [np.ones(4)])
    with pytest.raises(ValueError):
        ops.gp_loo_batch(one[0], one[1], one[2], [np.ones(3)] * 2)
    with pytest.raises(ValueError):
        ops.gp_loo_batch(one[0], [np.ones((ops.BATCH_NMAX + 1, 2))], [np.ones(ops.BATCH_NMAX + 1)])
    with pytest.raises(ValueError):
        ops.gp_loo_batch(one[0], [np.ones((3, 3))], one[2])
    assert a._alpha is None

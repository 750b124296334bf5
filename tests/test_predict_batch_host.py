"""CPU-only checks of predict_many(..., return_var / return_cov) (seam S3f): the device calls are replaced by NumPy stand-ins,
so these tests check routing, order, caching, shapes and the error paths, not the kernels."""
import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib, ops
from treegp_amd import gp_interp


def spec_matrix(spec, X, Y=None):
    X = _lib.as_xy(X)
    Y = X if Y is None else _lib.as_xy(Y)
    d = X[:, None, :] - Y[None, :, :]
    q = spec.a * d[..., 0] ** 2 + 2 * spec.b * d[..., 0] * d[..., 1] + spec.c * d[..., 1] ** 2
    return spec.amp * np.exp(-0.5 * q)


def host_factor(spec, X, y_err):
    K = spec_matrix(spec, X)
    K[np.diag_indices(len(K))] += np.asarray(y_err) ** 2
    return np.linalg.cholesky(K)


def host_posterior(spec, L, X, Xq, what):
    B = np.linalg.solve(L, spec_matrix(spec, X, Xq)).T
    return spec.amp - (B * B).sum(axis=1) if what == "var" else spec_matrix(spec, Xq) - B.dot(B.T)


class HostFactor(object):
    def __init__(self, L):
        self.L, self.freed = L, False

    def free(self, keep_memory=False):
        self.freed = True


@pytest.fixture
def fake(monkeypatch):
    """single and batched routes on the host; a kernel whose amp is negative fails its factorisation (info > 0)"""
    rec = {"posterior": [], "solve_batch": 0, "singles": []}

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["singles"].append(len(X))
        L = host_factor(spec, X, y_err)
        alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
        return alpha, 0.0, 0.0, (HostFactor(L) if keep else None)

    def gp_solve_batch(*a, **k):
        rec["solve_batch"] += 1
        raise AssertionError("the posterior route does not call gp_solve_batch")

    def gp_posterior_batch(specs, Xs, ys, y_errs, Xqs, what="var", want_alpha=True, ctx=None):
        rec["posterior"].append((what, [len(X) for X in Xs], [len(X) for X in Xqs]))
        alphas, uncs, info = [], [], []
        for s, X, y, e, Xq in zip(specs, Xs, ys, y_errs, Xqs):
            if s.amp < 0:
                alphas.append(np.full(len(X), np.nan)), uncs.append(np.full(len(Xq), np.nan)), info.append(1)
                continue
            L = host_factor(s, X, e)
            alphas.append(np.linalg.solve(L.T, np.linalg.solve(L, y)))
            uncs.append(host_posterior(s, L, X, Xq, what))
            info.append(0)
        return alphas, uncs, np.zeros(len(specs)), np.zeros(len(specs)), np.array(info)

    def gp_predict(spec, X1, alpha, X2, ctx=None):
        return spec_matrix(spec, X2, X1).dot(alpha)

    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_solve_batch", gp_solve_batch)
    monkeypatch.setattr(ops, "gp_posterior_batch", gp_posterior_batch)
    monkeypatch.setattr(ops, "gp_predict", gp_predict)
    monkeypatch.setattr(ops, "gp_predict_var", lambda spec, f, X1, X2, ctx=None: host_posterior(spec, f.L, X1, X2, "var"))
    monkeypatch.setattr(ops, "gp_predict_cov", lambda spec, f, X1, X2, ctx=None: host_posterior(spec, f.L, X1, X2, "cov"))
    return rec


def make_gp(n, seed, kernel="1.0**2 * RBF(1.5)"):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, 2))
    gp = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=True)
    gp.initialize(X, np.sin(X[:, 0]) + 0.1 * rng.standard_normal(n), y_err=rng.uniform(0.1, 0.2, n))
    return gp


def objects(monkeypatch):
    """a, b: batched; big: n > 4096; tree: dense route; cached: a cached alpha (batched); dist: the multi-GPU route; kept: a
    kept factor of its own data; far: more query points than the covariance takes"""
    a, b, big = make_gp(30, 1), make_gp(40, 2), make_gp(ops.BATCH_NMAX + 1, 3)
    tree = make_gp(25, 4, kernel="RBF(1.0) + WhiteKernel(0.01)")
    monkeypatch.setattr(tree, "_return_gp_predict_dense",
                        lambda y, X1, X2, k, e, c, v=False: (np.full(len(X2), 7.0), np.ones((len(X2),) * (2 if c else 1))))
    cached = make_gp(20, 5)
    cached._alpha = np.zeros(20)
    dist = make_gp(15, 6)
    dist.backend = "dist"
    monkeypatch.setattr(dist, "predict", lambda X, **kw: "dist-predict")
    kept = make_gp(35, 7)
    far = make_gp(25, 8)
    gps = [a, big, tree, b, cached, dist, kept, far]
    Xq = [np.full((k, 2), 0.5) for k in (3, 4, 5, 6, 7, 8, 9, 10)]
    Xq[7] = np.full((ops.POSTERIOR_MMAX["cov"] + 1, 1), 0.25)
    return gps, Xq


@pytest.mark.parametrize("what", ["var", "cov"])
def test_routing_order_caching_and_shapes(fake, monkeypatch, what):
    gps, Xq = objects(monkeypatch)
    a, big, tree, b, cached, dist, kept, far = gps
    kw = {"return_" + what: True}
    kept.predict(Xq[6], **kw)
    kept_factor, cached_alpha = kept._factor, cached._alpha
    assert kept_factor is not None
    fake["singles"].clear()
    out = tg.predict_many(gps, Xq, **kw)
    batched = [a, b, cached] + ([far] if what == "var" else [])
    assert fake["posterior"] == [(what, [len(g._X) for g in batched], [len(Xq[gps.index(g)]) for g in batched])]
    assert fake["solve_batch"] == 0
    assert fake["singles"] == [ops.BATCH_NMAX + 1] + ([25] if what == "cov" else [])      # big (and far) solve by themselves
    assert out[5] == "dist-predict"
    assert cached._alpha is cached_alpha and kept._factor is kept_factor
    for g in batched:
        assert g._alpha is not None and g._factor is None
    for i, (g, X) in enumerate(zip(gps, Xq)):
        if i == 5:
            continue
        y, u = out[i]
        m = len(X)
        assert y.shape == (m,) and u.shape == ((m,) if what == "var" else (m, m)), i
    np.testing.assert_allclose(out[2][0], 7.0 + tree._mean)
    np.testing.assert_allclose(out[4][0], cached._mean)                       # the cached (zero) alpha: the mean alone
    for g, i in ((a, 0), (b, 3), (cached, 4)):
        spec = tg.kernel_to_spec(g.kernel)
        L = host_factor(spec, g._X, g._y_err)
        np.testing.assert_allclose(out[i][1], host_posterior(spec, L, g._X, Xq[i], what), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(out[i][0], g.predict(Xq[i]), rtol=0, atol=0)


def test_both_flags_and_list_lengths_are_refused_before_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "get_ctx", no_device)
    monkeypatch.setattr(_lib, "load_library", no_device)
    a = make_gp(10, 1)
    with pytest.raises(ValueError, match="return_cov and return_var"):
        tg.predict_many([a], [np.zeros((2, 2))], return_cov=True, return_var=True)
    with pytest.raises(ValueError):
        tg.predict_many([a], [np.zeros((2, 2)), np.zeros((2, 2))], return_var=True)
    with pytest.raises(ValueError):
        ops.gp_posterior_batch([ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(3)], None, [np.ones((4097, 2))], what="cov")
    with pytest.raises(ValueError):
        ops.gp_posterior_batch([ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(3)], None, [np.ones((0, 2))])
    with pytest.raises(ValueError):
        ops.gp_posterior_batch([ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(3)], None, [np.ones((2, 2))], what="std")
    with pytest.raises(ValueError):
        ops.gp_posterior_batch([ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(3)], None, [np.ones((2, 2))] * 2)
    assert a._alpha is None


@pytest.mark.parametrize("what", ["var", "cov"])
def test_failed_factorisation_names_the_object_and_caches_nothing(fake, monkeypatch, what):
    a, b, c = make_gp(30, 1), make_gp(40, 2), make_gp(20, 3)
    real_spec = gp_interp.kernel_to_spec

    def spec_of(k):
        s = real_spec(k)
        if k is c.kernel:
            s.amp = -1.0
        return s
    monkeypatch.setattr(gp_interp, "kernel_to_spec", spec_of)
    with pytest.raises(np.linalg.LinAlgError, match="GP 2"):
        tg.predict_many([a, b, c], [np.zeros((2, 2))] * 3, **{"return_" + what: True})
    assert a._alpha is None and b._alpha is None and c._alpha is None


def test_default_call_never_touches_the_posterior_entry(fake, monkeypatch):
    def no_posterior(*a, **k):
        raise AssertionError("the default call reached gp_posterior_batch")
    monkeypatch.setattr(ops, "gp_posterior_batch", no_posterior)
    calls = []

    def gp_solve_batch(specs, Xs, ys, y_errs=None, want_alpha=True, ctx=None):
        calls.append(len(specs))
        return [np.zeros(len(X)) for X in Xs], np.zeros(len(specs)), np.zeros(len(specs)), np.zeros(len(specs), dtype=int)
    monkeypatch.setattr(ops, "gp_solve_batch", gp_solve_batch)
    a, b = make_gp(30, 1), make_gp(40, 2)
    out = tg.predict_many([a, b], [np.zeros((2, 2)), np.zeros((3, 2))])
    assert calls == [2] and out[0].shape == (2,) and out[1].shape == (3,)

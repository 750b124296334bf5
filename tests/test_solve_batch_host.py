"""CPU-only checks of the batched-solve layer (ops.gp_solve_batch's padding, log_likelihood_many, predict_many): the device
calls are replaced by NumPy stand-ins, so these tests check routing, order, padding and the error paths, not the kernels."""
import sys

import numpy as np
import pytest

import treegp_amd as tg
import treegp_amd.log_likelihood  # noqa: F401
from treegp_amd import _lib, ops
from treegp_amd import gp_interp
ll_mod = sys.modules["treegp_amd.log_likelihood"]          # (the package name is shadowed by the class, as in the reference)


def spec_matrix(spec, X):
    X = _lib.as_xy(X)
    d = X[:, None, :] - X[None, :, :]
    q = spec.a * d[..., 0] ** 2 + 2 * spec.b * d[..., 0] * d[..., 1] + spec.c * d[..., 1] ** 2
    return spec.amp * np.exp(-0.5 * q)


def host_solve(spec, X, y, y_err):
    K = spec_matrix(spec, X)
    if y_err is not None:
        K[np.diag_indices(len(K))] += np.asarray(y_err) ** 2
    L = np.linalg.cholesky(K)
    z = np.linalg.solve(L, y)
    return np.linalg.solve(L.T, z), 2.0 * np.log(np.diag(L)).sum(), z.dot(z)


@pytest.fixture
def fake(monkeypatch):
    """ops.gp_solve / gp_solve_batch on the host; the batch records what it was given, a kernel whose amp is negative
    fails its factorisation (info > 0)"""
    rec = {"batches": [], "singles": []}

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["singles"].append(len(X))
        if spec.amp < 0:
            raise np.linalg.LinAlgError("1-th leading minor of the array is not positive definite")
        a, ld, c = host_solve(spec, X, y, y_err)
        return (a if want_alpha else None), ld, c, None

    def gp_solve_dense(K, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["singles"].append(len(K))
        K = np.array(K, dtype=float)
        if y_err is not None:
            K[np.diag_indices(len(K))] += np.asarray(y_err) ** 2
        L = np.linalg.cholesky(K)
        z = np.linalg.solve(L, y)
        return None, 2.0 * np.log(np.diag(L)).sum(), z.dot(z), None

    def gp_solve_batch(specs, Xs, ys, y_errs=None, want_alpha=True, ctx=None):
        ns, nmax, Xb, yb, eb = ops.pad_batch(Xs, ys, y_errs)
        rec["batches"].append([s.amp for s in specs])
        alphas, lds, cs, info = [], [], [], []
        for b, s in enumerate(specs):
            n = int(ns[b])
            if s.amp < 0:
                alphas.append(np.full(n, np.nan)), lds.append(np.nan), cs.append(np.nan), info.append(1)
                continue
            a, ld, c = host_solve(s, Xb[b, :n], yb[b, :n], None if eb is None else eb[b, :n])
            alphas.append(a), lds.append(ld), cs.append(c), info.append(0)
        return (alphas if want_alpha else None), np.array(lds), np.array(cs), np.array(info)

    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_solve_dense", gp_solve_dense)
    monkeypatch.setattr(ops, "gp_solve_batch", gp_solve_batch)
    return rec


def rbf(scale):
    return tg.eval_kernel("1.0**2 * RBF(%r)" % scale)


def data(n, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, 2))
    return X, np.sin(X[:, 0]) + 0.1 * rng.standard_normal(n), rng.uniform(0.1, 0.2, n)


def test_padding_and_shape_errors():
    ns, nmax, Xb, yb, eb = ops.pad_batch([np.arange(3.0), np.ones((2, 2))], [np.ones(3), [2.0, 3.0]], [np.ones(3), np.ones(2)])
    assert list(ns) == [3, 2] and nmax == 3
    assert np.array_equal(Xb[0], [[0, 0], [1, 0], [2, 0]])            # 1-D coordinates: zero second column
    assert np.array_equal(Xb[1], [[1, 1], [1, 1], [0, 0]]) and np.array_equal(yb[1], [2, 3, 0]) and eb[1, 2] == 0
    bad = [
        ([np.ones((3, 2))], [np.ones(4)], None),                        # y length
        ([np.ones((3, 2))], [np.ones((3, 1))], None),                   # y not 1-D
        ([np.ones((3, 3))], [np.ones(3)], None),                        # 3-D coordinates
        ([np.ones((3, 2))], [np.ones(3), np.ones(3)], None),            # list lengths
        ([np.ones((3, 2))], [np.ones(3)], [np.ones(2)]),                # y_err length
        ([np.ones((0, 2))], [np.ones(0)], None),                        # empty problem
        ([], [], None),
    ]
    for Xs, ys, es in bad:
        with pytest.raises(ValueError):
            ops.pad_batch(Xs, ys, es)


def test_gp_solve_batch_rejects_bad_shapes_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "get_ctx", no_device)
    monkeypatch.setattr(_lib, "load_library", no_device)
    with pytest.raises(ValueError):
        ops.gp_solve_batch([ops.KernelSpec(0), ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(3)])
    with pytest.raises(ValueError):
        ops.gp_solve_batch([ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(2)])
    with pytest.raises(ValueError):
        ops.gp_solve_batch([ops.KernelSpec(0)], [np.ones((4097, 2))], [np.ones(4097)])


def test_log_likelihood_many_routes_and_keeps_order(fake, monkeypatch):
    X, y, e = data(50)
    like = tg.log_likelihood(X, y, e)
    sum_tree = tg.eval_kernel("RBF(2.0) + WhiteKernel(0.1)")          # no spec: its own log_likelihood, in place
    kernels = [rbf(1.0), sum_tree, rbf(2.0), rbf(3.0), rbf(0.5)]
    real_spec = ll_mod.kernel_to_spec

    def spec_of(k):
        s = real_spec(k)
        if k is kernels[3]:
            s.amp = -1.0                  # kernel 3's factorisation fails (the stand-ins' convention)
        return s
    monkeypatch.setattr(ll_mod, "kernel_to_spec", spec_of)
    out = like.log_likelihood_many(kernels)
    assert len(fake["batches"]) == 1 and len(fake["batches"][0]) == 4     # the four spec kernels in one call, in order
    assert out[3] == -np.inf
    for i in (0, 2, 4):
        a, ld, c = host_solve(real_spec(kernels[i]), X, y, e)
        np.testing.assert_allclose(out[i], -0.5 * c - 25 * np.log(2 * np.pi) - 0.5 * ld, rtol=1e-12)
    assert fake["singles"] == [50]                                        # the kernel tree, by itself
    np.testing.assert_allclose(out[1], like.log_likelihood(sum_tree), rtol=1e-12)
    assert like.log_likelihood(kernels[3]) == out[3]                         # the same semantics one by one


def test_log_likelihood_many_large_and_distributed_go_one_by_one(fake, monkeypatch):
    X, y, e = data(ops.BATCH_NMAX + 1)
    like = tg.log_likelihood(X, y, e)
    calls = []
    monkeypatch.setattr(like, "log_likelihood", lambda k: calls.append(k) or 1.0)
    ks = [rbf(1.0), rbf(2.0)]
    assert list(like.log_likelihood_many(ks)) == [1.0, 1.0] and calls == ks and not fake["batches"]
    X, y, e = data(20)
    like = tg.log_likelihood(X, y, e)
    like.distributed = True
    calls.clear()
    monkeypatch.setattr(like, "log_likelihood", lambda k: calls.append(k) or 2.0)
    assert list(like.log_likelihood_many(ks)) == [2.0, 2.0] and calls == ks and not fake["batches"]


def make_gp(n, seed, kernel="1.0**2 * RBF(1.5)"):
    X, y, e = data(n, seed)
    gp = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=True)
    gp.initialize(X, y, y_err=e)
    return gp


def test_predict_many_routes_caches_and_predicts_in_order(fake, monkeypatch):
    predicted = []

    def gp_predict(spec, X1, alpha, X2, ctx=None):
        predicted.append(len(X2))
        return (spec_matrix(spec, np.vstack([_lib.as_xy(X2), _lib.as_xy(X1)]))[:len(X2), len(X2):]).dot(alpha)
    monkeypatch.setattr(ops, "gp_predict", gp_predict)
    a, b, big = make_gp(30, 1), make_gp(40, 2), make_gp(ops.BATCH_NMAX + 1, 3)
    tree = make_gp(25, 4, kernel="RBF(1.0) + WhiteKernel(0.01)")
    cached = make_gp(20, 5)
    cached._alpha = np.zeros(20)
    dist = make_gp(15, 6)
    dist.backend = "dist"
    monkeypatch.setattr(dist, "predict", lambda X: "dist-predict")
    monkeypatch.setattr(tree, "_return_gp_predict_dense", lambda y, X1, X2, k, e, c, v=False: (np.full(len(X2), 7.0), None))
    Xq = [np.ones((k, 2)) * 0.5 for k in (3, 4, 5, 6, 7, 8)]
    out = tg.predict_many([a, big, tree, b, cached, dist], Xq)
    assert len(fake["batches"]) == 1 and len(fake["batches"][0]) == 2       # a and b only
    assert fake["singles"] == [ops.BATCH_NMAX + 1]                          # big solves in its own predict
    assert out[5] == "dist-predict"
    np.testing.assert_allclose(out[2], 7.0 + tree._mean)
    np.testing.assert_allclose(out[4], cached._mean)                         # zero alpha: the mean alone
    for gp, X, o in ((a, Xq[0], out[0]), (b, Xq[3], out[3])):
        alpha = host_solve(ops.KernelSpec(0, 1.0, 1 / 1.5 ** 2, 0.0, 1 / 1.5 ** 2), gp._X, gp._residual(), gp._y_err)[0]
        np.testing.assert_allclose(gp._alpha, alpha, rtol=1e-12)
        np.testing.assert_allclose(o, gp_predict(tg.kernel_to_spec(gp.kernel), gp._X, alpha, X) + gp._mean, rtol=1e-12)
    # a later predict reuses the cached alpha: no solve
    before = (len(fake["batches"]), len(fake["singles"]))
    a.predict(Xq[0])
    assert (len(fake["batches"]), len(fake["singles"])) == before


def test_predict_many_failed_factorisation_names_the_object(fake, monkeypatch):
    a, b = make_gp(30, 1), make_gp(40, 2)
    real_spec = gp_interp.kernel_to_spec

    def spec_of(k):
        s = real_spec(k)
        if k is b.kernel:
            s.amp = -1.0
        return s
    monkeypatch.setattr(gp_interp, "kernel_to_spec", spec_of)
    with pytest.raises(np.linalg.LinAlgError, match="GP 1"):
        tg.predict_many([a, b], [np.zeros((2, 2)), np.zeros((2, 2))])
    assert a._alpha is None and b._alpha is None
    with pytest.raises(ValueError):
        tg.predict_many([a, b], [np.zeros((2, 2))])


def test_log_likelihood_many_device_errors_of_the_batch(fake, monkeypatch):
    """A run-time device error of the batched call (rc -2) warns and every kernel is evaluated by itself; an argument error
    (rc -1), or any error under TGP_ML_STRICT=1, raises -- as for a single evaluation."""
    X, y, e = data(30)
    like = tg.log_likelihood(X, y, e)
    ks = [rbf(1.0), rbf(2.0)]

    def failing(rc):
        def gp_solve_batch(*a, **k):
            err = _lib.TgpError("tgp_gp_solve_batch failed (%d)" % rc)
            err.rc = rc
            raise err
        return gp_solve_batch
    monkeypatch.setattr(ops, "gp_solve_batch", failing(-2))
    monkeypatch.delenv("TGP_ML_STRICT", raising=False)
    with pytest.warns(RuntimeWarning, match="one by one"):
        out = like.log_likelihood_many(ks)
    assert fake["singles"] == [30, 30]
    np.testing.assert_allclose(out, [like.log_likelihood(k) for k in ks], rtol=1e-12)
    monkeypatch.setenv("TGP_ML_STRICT", "1")
    with pytest.raises(_lib.TgpError):
        like.log_likelihood_many(ks)
    monkeypatch.delenv("TGP_ML_STRICT")
    monkeypatch.setattr(ops, "gp_solve_batch", failing(-1))
    with pytest.raises(_lib.TgpError):
        like.log_likelihood_many(ks)

"""CPU-only checks of the sampling layer (treegp_amd.sampling, GPInterpolation.sample_y): the device calls are replaced by
NumPy stand-ins, so these tests check shapes, the normal stream, the jitter and the error paths, not the kernel."""
import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib, ops, sampling


class FakeFactor(object):
    def __init__(self, L):
        self.L, self.n, self.freed = L, len(L), False

    def free(self, keep_memory=False):
        self.freed = True


@pytest.fixture
def fake(monkeypatch):
    """ops.gp_solve / gp_solve_dense / factor_lmul on the host: the solves record what they were given and keep
    cholesky(K + diag(y_err^2)); factor_lmul returns (L Z^T)^T"""
    rec = {"factors": []}

    def spec_matrix(spec, X):
        X = _lib.as_xy(X)
        d = X[:, None, :] - X[None, :, :]
        q = spec.a * d[..., 0] ** 2 + 2 * spec.b * d[..., 0] * d[..., 1] + spec.c * d[..., 1] ** 2
        return spec.amp * np.exp(-0.5 * q)

    def factorise(K, y_err, keep, want_alpha):
        assert keep and not want_alpha
        K = np.array(K, dtype=float)
        if y_err is not None:
            K[np.diag_indices(len(K))] += np.asarray(y_err) ** 2
        try:
            L = np.linalg.cholesky(K)
        except np.linalg.LinAlgError:
            raise np.linalg.LinAlgError("1-th leading minor of the array is not positive definite")
        f = FakeFactor(L)
        rec["factors"].append(f)
        return None, 0.0, 0.0, f

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["spec"], rec["y_err"], rec["ctx"] = spec, None if y_err is None else np.array(y_err), ctx
        return factorise(spec_matrix(spec, X), y_err, keep, want_alpha)

    def gp_solve_dense(K, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["K"], rec["dense_y_err"], rec["ctx"] = np.array(K), y_err, ctx
        return factorise(K, y_err, keep, want_alpha)

    def factor_lmul(factor, Z, ctx=None):
        Z = np.atleast_2d(Z)
        assert Z.shape[1] == factor.n
        return np.stack([factor.L.dot(z) for z in Z])           # row by row, as the device computes them

    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_solve_dense", gp_solve_dense)
    monkeypatch.setattr(ops, "factor_lmul", factor_lmul)
    return rec


def points(n, d=2, seed=1):
    return np.random.default_rng(seed).uniform(0, 1, (n, d))


def test_shapes_and_normal_stream_parametrised(fake):
    X = points(30)
    K = "1.5**2 * AnisotropicRBF(invLam=array([[20.0, 4.0], [4.0, 12.0]]))"
    y5 = tg.gaussian_random_field(K, X, n_samples=5, random_state=11)
    assert y5.shape == (30, 5)
    assert all(f.freed for f in fake["factors"])
    assert fake["ctx"] == "ctx"                       # one GPU: the caller's own context, never the multi-GPU route
    y1 = tg.gaussian_random_field(K, X, n_samples=1, random_state=11)
    assert y1.shape == (30, 1)
    np.testing.assert_array_equal(y1[:, 0], y5[:, 0])
    L = fake["factors"][-1].L
    z = np.random.default_rng(11).standard_normal((5, 30))
    np.testing.assert_allclose(y5, L.dot(z.T), rtol=0, atol=1e-13)
    assert not np.array_equal(y5[:, 0], tg.gaussian_random_field(K, X, n_samples=1, random_state=12)[:, 0])


def test_jitter_parametrised_kernel(fake):
    X = points(20)
    e = np.linspace(0.01, 0.1, 20)
    tg.gaussian_random_field("2.0**2 * RBF(0.4)", X, y_err=e, nugget=1e-6)
    # amp = 4: the noise handed to the device is y_err^2 + 1e-6 * 4 in quadrature
    np.testing.assert_allclose(fake["y_err"] ** 2, e ** 2 + 4e-6, rtol=1e-13)
    tg.gaussian_random_field("2.0**2 * RBF(0.4)", X, nugget=0.0)
    np.testing.assert_array_equal(fake["y_err"], np.zeros(20))


def test_jitter_kernel_tree(fake):
    X = points(25)
    kernel = tg.eval_kernel("1.0**2 * RBF(0.3) + WhiteKernel(1e-3)")
    e = np.full(25, 0.05)
    out = tg.gaussian_random_field(kernel, X, n_samples=3, random_state=4, y_err=e, nugget=1e-4)
    assert out.shape == (25, 3)
    K0 = kernel(X)
    jitter = 1e-4 * np.max(kernel.diag(X))                 # 1e-4 * (1 + 1e-3)
    assert jitter == pytest.approx(1e-4 * 1.001, rel=1e-12)
    np.testing.assert_allclose(np.diag(fake["K"]), np.diag(K0) + e ** 2 + jitter, rtol=1e-14)
    off = ~np.eye(25, dtype=bool)
    np.testing.assert_array_equal(fake["K"][off], K0[off])
    z = np.random.default_rng(4).standard_normal((3, 25))
    np.testing.assert_allclose(out, np.linalg.cholesky(fake["K"]).dot(z.T), rtol=0, atol=1e-13)


def test_one_dimensional_points(fake):
    x = np.linspace(0, 1, 12)
    out = tg.gaussian_random_field("RBF(0.2)", x, n_samples=2)
    assert out.shape == (12, 2)


def test_argument_errors(fake):
    X = points(10)
    with pytest.raises(ValueError, match="n_samples"):
        tg.gaussian_random_field("RBF(0.3)", X, n_samples=0)
    with pytest.raises(ValueError, match="nugget"):
        tg.gaussian_random_field("RBF(0.3)", X, nugget=-1e-10)
    with pytest.raises(ValueError, match="columns"):
        tg.gaussian_random_field("AnisotropicRBF(invLam=array([[4.0, 0.0], [0.0, 4.0]]))", points(10, 3))
    with pytest.raises(ValueError, match="columns"):
        tg.gaussian_random_field("AnisotropicRBF(invLam=array([[4.0]]))", X)
    with pytest.raises(ValueError, match="y_err"):
        tg.gaussian_random_field("RBF(0.3)", X, y_err=np.ones(3))
    assert not fake["factors"]                                 # refused before any factorisation


def test_not_positive_definite_names_nugget(fake):
    X = np.zeros((4, 2))                                        # four identical points: K is all ones, rank one (parametrised and kernel-tree routes)
    for kernel in ("1.0**2 * RBF(0.3)", "RBF(0.3) ** 1.0"):
        with pytest.raises(np.linalg.LinAlgError, match="nugget"):
            tg.gaussian_random_field(kernel, X, nugget=0.0)
        assert tg.gaussian_random_field(kernel, X).shape == (4, 1)       # the default nugget makes it definite


def make_gp(monkeypatch, y_star, cov, kernel="1.0**2 * RBF(0.3)"):
    gp = tg.GPInterpolation(kernel=kernel, optimizer="none")
    gp.kernel = gp.kernel_template
    calls = []

    def predict(X, return_cov=False, return_var=False):
        calls.append((len(X), return_cov, return_var))
        return y_star, cov
    monkeypatch.setattr(gp, "predict", predict)
    return gp, calls


def test_sample_y_shapes_stream_and_jitter(fake, monkeypatch):
    m = 15
    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m))
    cov = G.dot(G.T) / m
    y_star = rng.standard_normal(m)
    gp, calls = make_gp(monkeypatch, y_star, cov)
    X = points(m)
    s5 = gp.sample_y(X, n_samples=5, random_state=3, nugget=1e-8)
    s1 = gp.sample_y(X, random_state=3, nugget=1e-8)
    assert s5.shape == (m, 5) and s1.shape == (m, 1)
    np.testing.assert_array_equal(s1[:, 0], s5[:, 0])
    assert calls == [(m, True, False)] * 2
    np.testing.assert_allclose(np.diag(fake["K"]), np.diag(cov) + 1e-8, rtol=1e-14)      # amp = 1
    assert fake["dense_y_err"] is None and fake["ctx"] == "ctx"
    z = np.random.default_rng(3).standard_normal((5, m))
    np.testing.assert_allclose(s5, y_star[:, None] + np.linalg.cholesky(fake["K"]).dot(z.T), rtol=0, atol=1e-13)
    assert all(f.freed for f in fake["factors"])


def test_sample_y_kernel_tree_jitter(fake, monkeypatch):
    m = 6
    gp, _ = make_gp(monkeypatch, np.zeros(m), np.eye(m), kernel="0.5**2 * RBF(0.3) + WhiteKernel(0.25)")
    gp.sample_y(points(m), nugget=1e-3)
    np.testing.assert_allclose(np.diag(fake["K"]), 1.0 + 1e-3 * 0.5, rtol=1e-14)        # max diag k = 0.25 + 0.25


def test_sample_y_errors(fake, monkeypatch):
    gp, calls = make_gp(monkeypatch, np.zeros(3), -np.eye(3))
    with pytest.raises(np.linalg.LinAlgError, match="nugget"):
        gp.sample_y(points(3), nugget=0.0)
    with pytest.raises(ValueError, match="nugget"):
        gp.sample_y(points(3), nugget=-1.0)
    with pytest.raises(ValueError, match="n_samples"):
        gp.sample_y(points(3), n_samples=0)
    gp2, calls2 = make_gp(monkeypatch, np.zeros(3), np.eye(3),
                          kernel="AnisotropicRBF(invLam=array([[4.0, 0.0], [0.0, 4.0]]))")
    with pytest.raises(ValueError, match="columns"):
        gp2.sample_y(points(3, 1))
    assert len(calls) == 1 and not calls2                      # argument errors come before predict

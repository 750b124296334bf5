"""GPU tests of realisations (seam S3d): tgp_factor_lmul (Y = L Z with the packed factor, csrc/lmul.hip), the prior
sampler treegp_amd.gaussian_random_field and the posterior sampler GPInterpolation.sample_y.  The product is checked
against the factor unpacked to the host (so that the test is about the product, not the Cholesky), for determinism and
for independence of a column from its batch; the samplers against NumPy's Cholesky with the same normals and by their
statistics."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 8                          # right-hand sides per group of the kernel (LMUL_R in csrc/lmul.hip)


def _rbf_factor(n, seed=0, ell=0.3, amp=1.3):
    from treegp_amd import _lib, ops
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    e = rng.uniform(0.1, 0.3, n)
    spec = ops.KernelSpec(_lib.TGP_RBF, amp=amp, a=1.0 / ell ** 2, b=0.0, c=1.0 / ell ** 2)
    f = ops.gp_solve(spec, X, np.zeros(n), e, keep=True, want_alpha=False)[3]
    return spec, X, e, f


def _unpack(f):
    from treegp_amd import _lib
    lib = _lib.load_library()
    ctx = f._ctx
    dA, dW, Np = C.c_void_p(), C.c_void_p(), C.c_int64()
    _lib.check(ctx, lib.tgp_factor_device(ctx, f._h, C.byref(dA), C.byref(dW), C.byref(Np)), "tgp_factor_device")
    L = np.empty((f.n, f.n))
    _lib.check(ctx, lib.tgp_d_unpack_lower(ctx, dA, Np.value, f.n, _lib.ptr(L)), "tgp_d_unpack_lower")
    return L


@pytest.mark.parametrize("n", [1, 2, 63, 255, 256, 257, 513, 2049, 4097, 16640])
def test_lmul_against_unpacked_factor(n):
    from treegp_amd import ops
    _, _, _, f = _rbf_factor(n, seed=n)
    L = _unpack(f)
    absL = np.abs(L)
    rng = np.random.default_rng(7 + n)
    for nrhs in (1, 3, R, R + 1, 2 * R + 3):
        Z = rng.standard_normal((nrhs, n))
        Y = ops.factor_lmul(f, Z)
        assert Y.shape == (nrhs, n)
        ref = Z.dot(L.T)
        bound = 1e-12 * np.abs(Z).dot(absL.T)
        bad = np.abs(Y - ref) > bound
        assert not bad.any(), "n=%d nrhs=%d: %d entries off, worst %.3g x bound" % (
            n, nrhs, bad.sum(), (np.abs(Y - ref) / np.maximum(bound, 1e-300)).max())
    f.free()


@pytest.mark.parametrize("n", [300, 9000])
def test_lmul_deterministic_and_batch_independent(n):
    from treegp_amd import _lib, ops
    _, _, _, f = _rbf_factor(n, seed=3)
    Z = np.random.default_rng(5).standard_normal((2 * R + 3, n))
    Y1 = ops.factor_lmul(f, Z)
    assert _lib.timings(f._ctx)[11] > 0.0
    Y2 = ops.factor_lmul(f, Z)
    np.testing.assert_array_equal(Y1, Y2)
    for v in (0, 1, R - 1, R, 2 * R + 2):
        np.testing.assert_array_equal(ops.factor_lmul(f, Z[v])[0], Y1[v])
    np.testing.assert_array_equal(ops.factor_lmul(f, Z[3:R + 4]), Y1[3:R + 4])
    f.free()


def _kernel_case(tag, n):
    import treegp_amd as tg
    rng = np.random.default_rng(11)
    if tag == "arbf":
        return tg.eval_kernel("1.2**2 * AnisotropicRBF(invLam=array([[30.0, 4.0], [4.0, 20.0]]))"), rng.uniform(0, 1, (n, 2))
    if tag == "vk":
        return tg.eval_kernel("0.8**2 * VonKarman(length_scale=0.3)"), rng.uniform(0, 1, (n, 2))
    if tag == "1d":
        return tg.eval_kernel("0.9**2 * RBF(0.2)"), rng.uniform(0, 1, (n, 1))
    return tg.eval_kernel("1.0**2 * RBF(0.3) + WhiteKernel(1e-3)"), rng.uniform(0, 1, (n, 2))


@pytest.mark.parametrize("tag", ["arbf", "vk", "1d", "tree"])
@pytest.mark.parametrize("n", [37, 700, 2000])
def test_gaussian_random_field_matches_numpy_cholesky(tag, n):
    import treegp_amd as tg
    kernel, X = _kernel_case(tag, n)
    e = np.random.default_rng(n).uniform(0.1, 0.3, n)
    nugget = 1e-10
    out = tg.gaussian_random_field(kernel, X, n_samples=3, random_state=n, y_err=e, nugget=nugget)
    assert out.shape == (n, 3)
    jitter = nugget * np.max(kernel.diag(X))
    K = kernel(X) + np.diag(e ** 2) + jitter * np.eye(n)
    z = np.random.default_rng(n).standard_normal((3, n))
    ref = np.linalg.cholesky(K).dot(z.T)
    assert np.abs(out - ref).max() <= 1e-10 * np.abs(ref).max()
    one = tg.gaussian_random_field(kernel, X, n_samples=1, random_state=n, y_err=e, nugget=nugget)
    np.testing.assert_array_equal(one[:, 0], out[:, 0])


@pytest.mark.parametrize("tag", ["arbf", "vk", "1d", "tree"])
def test_gaussian_random_field_statistics(tag):
    import treegp_amd as tg
    n, S = 40, 40000
    kernel, X = _kernel_case(tag, n)
    out = tg.gaussian_random_field(kernel, X, n_samples=S, random_state=2)
    K = kernel(X) + 1e-10 * np.max(kernel.diag(X)) * np.eye(n)
    cov = out.dot(out.T) / S
    se = np.sqrt((np.outer(np.diag(K), np.diag(K)) + K ** 2) / S)
    assert (np.abs(cov - K) <= 6 * se).all(), np.abs((cov - K) / se).max()
    assert (np.abs(out.mean(axis=1)) <= 6 * np.sqrt(np.diag(K) / S)).all()


def test_full_size_quadratic_form():
    """y = L z at N = 32 768 (multi-tile segments of lmul.hip, big-step sweeps of the solve): y . (K + D)^-1 y = |z|^2"""
    from treegp_amd import ops
    n = 32768
    _, _, _, f = _rbf_factor(n, seed=9, ell=0.05)
    Z = np.random.default_rng(1).standard_normal((4, n))
    Y = ops.factor_lmul(f, Z)
    Xs = ops.factor_solve(f, Y)
    f.free()
    q = np.einsum("ij,ij->i", Y, Xs)
    zz = np.einsum("ij,ij->i", Z, Z)
    np.testing.assert_allclose(q, zz, rtol=1e-8)


def _gp(kernel, n=300, seed=4, y_err=None, mean=3.0):
    import treegp_amd as tg
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    y = mean + np.sin(4 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.1 * rng.standard_normal(n)
    e = rng.uniform(0.1, 0.2, n) if y_err is None else np.full(n, y_err)
    gp = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=True)
    gp.initialize(X, y, e)
    return gp, X


def _grid(nx=5, ny=4):
    g = np.meshgrid(np.linspace(0.1, 0.9, nx), np.linspace(0.12, 0.88, ny))
    return np.column_stack([g[0].ravel(), g[1].ravel()])


@pytest.mark.parametrize("kernel", ["1.1**2 * AnisotropicRBF(invLam=array([[25.0, 3.0], [3.0, 15.0]]))",
                                    "1.0**2 * RBF(0.3) + WhiteKernel(1e-3)"])
def test_sample_y_matches_numpy_cholesky(kernel):
    gp, _ = _gp(kernel)
    Xs = _grid()
    m = len(Xs)
    out = gp.sample_y(Xs, n_samples=6, random_state=5)
    assert out.shape == (m, 6)
    y_star, cov = gp.predict(Xs, return_cov=True)
    assert abs(np.mean(y_star)) > 1.0                        # the mean (normalize=True) is part of every realisation
    jitter = 1e-10 * np.max(gp.kernel.diag(Xs))
    z = np.random.default_rng(5).standard_normal((6, m))
    dev = np.linalg.cholesky(cov + jitter * np.eye(m)).dot(z.T)
    got = out - y_star[:, None]
    assert np.abs(got - dev).max() <= 1e-10 * np.abs(dev).max()
    np.testing.assert_array_equal(gp.sample_y(Xs, random_state=5)[:, 0], out[:, 0])


def test_sample_y_statistics_and_state():
    gp, X = _gp("1.1**2 * AnisotropicRBF(invLam=array([[25.0, 3.0], [3.0, 15.0]]))")
    Xs = _grid()
    before = gp.predict(X[:50])
    y_star, cov = gp.predict(Xs, return_cov=True)
    S = 20000
    out = gp.sample_y(Xs, n_samples=S, random_state=8)
    sd = np.sqrt(np.diag(cov))
    assert (np.abs(out.mean(axis=1) - y_star) <= 6 * sd / np.sqrt(S)).all()
    d = out - y_star[:, None]
    c = d.dot(d.T) / S
    se = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / S)
    assert (np.abs(c - cov) <= 6 * se).all(), np.abs((c - cov) / se).max()
    np.testing.assert_array_equal(gp.predict(X[:50]), before)


def test_errors():
    import treegp_amd as tg
    gp, X = _gp("1.0**2 * RBF(0.3)")
    Xs = _grid(3, 1)
    y_star = gp.predict(Xs)
    gp_bad, _ = _gp("1.0**2 * RBF(0.3)")
    indefinite = np.diag([1.0, -0.5, 1.0])                    # smallest eigenvalue -0.5: no rounding decides this
    gp_bad.predict = lambda X, return_cov=False, return_var=False: (y_star, indefinite)
    with pytest.raises(np.linalg.LinAlgError, match="nugget"):
        gp_bad.sample_y(Xs, nugget=0.0)
    with pytest.raises(np.linalg.LinAlgError, match="nugget"):
        tg.gaussian_random_field("-1.0 * RBF(0.3)", X[:20], nugget=0.0)                 # K = -k: negative definite
    with pytest.raises(np.linalg.LinAlgError, match="nugget"):
        tg.gaussian_random_field(tg.eval_kernel("-1.0 * RBF(0.3)") + tg.eval_kernel("WhiteKernel(1e-3)"), X[:20],
                                 nugget=0.0)
    with pytest.raises(ValueError, match="nugget"):
        gp.sample_y(Xs, nugget=-1e-12)
    with pytest.raises(ValueError, match="nugget"):
        tg.gaussian_random_field("RBF(0.3)", X, nugget=-1.0)
    # query points on nearly noiseless training points: the posterior covariance there is ~1e-10 and below, with rounding
    # errors of the same order; the default nugget carries it
    quiet, Xq = _gp("1.0**2 * RBF(0.3)", n=400, y_err=1e-5)
    out = quiet.sample_y(Xq[:60], n_samples=4)
    assert out.shape == (60, 4) and np.isfinite(out).all()
    np.testing.assert_allclose(out.mean(axis=1), quiet.predict(Xq[:60]), atol=1e-3)

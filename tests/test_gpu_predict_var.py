"""GPU tests of the posterior variance (seam S3c, tgp_gp_predict_var[_dense]): the diagonal of the posterior covariance
without the (m, m) matrix, for any number of query points.  The reference's callers take np.diag(y_cov)
(tests/test_gp_interp.py:51-52 there); here that diagonal is checked against the oracle, the device covariance, a host
float64 computation beyond the covariance's size limit, and through GPInterpolation."""
import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

pytestmark = pytest.mark.gpu

KINDS = {
    "rbf": ("gauss", dict(amp=1.3, a=1.0 / 0.2 ** 2, b=0.0, c=1.0 / 0.2 ** 2)),
    "arbf": ("gauss", dict(amp=1.3, a=30.0, b=4.0, c=20.0)),
    "vk": ("vk", dict(amp=0.8, ell=0.3)),
    "avk": ("avk", dict(amp=0.8, a=12.0, b=2.0, c=9.0)),
}


def _spec(tag):
    from treegp_amd import _lib, ops
    kind, kw = KINDS[tag]
    code = {"rbf": _lib.TGP_RBF, "arbf": _lib.TGP_ARBF, "vk": _lib.TGP_VK, "avk": _lib.TGP_AVK}[tag]
    return ops.KernelSpec(code, **kw), kind, kw


def _problem(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    y = rng.standard_normal(n)
    e = rng.uniform(0.05, 0.2, n)
    return rng, X, y, e


@pytest.mark.parametrize("n", [1, 129, 257, 1025, 3000])
@pytest.mark.parametrize("tag", ["rbf", "arbf", "vk", "avk"])
def test_variance_against_oracle_diagonal(tag, n):
    from oracle import gp_oracle as O
    from treegp_amd import ops
    spec, kind, kw = _spec(tag)
    rng, X, y, e = _problem(n, 1000 + n)
    fac = ops.gp_solve(spec, X, y, e, keep=True)[3]
    K = O.kernel_matrix(kind, X, **kw)
    for m in (1, 5, 130, 1000):
        Xs = rng.uniform(0, 1, (m, 2))
        var = ops.gp_predict_var(spec, fac, X, Xs)
        assert var.shape == (m,)
        ref = np.diag(O.gp_predict_cov(K, e, O.kernel_matrix(kind, Xs, X, **kw), O.kernel_matrix(kind, Xs, **kw)))
        np.testing.assert_allclose(var, ref, rtol=0, atol=1e-10 * spec.amp)
    fac.free()


def test_variance_agrees_with_device_covariance():
    from treegp_amd import ops
    spec, _, _ = _spec("arbf")
    rng, X, y, e = _problem(2048, 5)
    Xs = rng.uniform(0, 1, (1500, 2))
    fac = ops.gp_solve(spec, X, y, e, keep=True)[3]
    var = ops.gp_predict_var(spec, fac, X, Xs)
    cov = ops.gp_predict_cov(spec, fac, X, Xs)
    np.testing.assert_allclose(var, np.diag(cov), rtol=0, atol=1e-12 * spec.amp)
    fac.free()


def test_variance_does_not_depend_on_the_chunk(monkeypatch):
    from treegp_amd import ops
    spec, _, _ = _spec("avk")
    rng, X, y, e = _problem(1500, 6)
    Xs = rng.uniform(0, 1, (3000, 2))
    fac = ops.gp_solve(spec, X, y, e, keep=True)[3]
    monkeypatch.delenv("TGP_VAR_CHUNK", raising=False)
    v_default = ops.gp_predict_var(spec, fac, X, Xs)
    monkeypatch.setenv("TGP_VAR_CHUNK", "256")                # 12 chunks
    v_256 = ops.gp_predict_var(spec, fac, X, Xs)
    monkeypatch.setenv("TGP_VAR_CHUNK", "1000")               # rounded up to 1024: three chunks, the last one short
    v_1024 = ops.gp_predict_var(spec, fac, X, Xs)
    assert np.array_equal(v_256, v_default)
    assert np.array_equal(v_1024, v_default)
    fac.free()


def test_variance_beyond_the_covariance_limit():
    """m = 70 000 query points: the covariance refuses more than 65 535 (and would need 39 GB); the variance does not."""
    from oracle import gp_oracle as O
    from treegp_amd import ops
    spec, kind, kw = _spec("arbf")
    rng, X, y, e = _problem(600, 7)
    Xs = rng.uniform(-0.2, 1.2, (70000, 2))
    fac = ops.gp_solve(spec, X, y, e, keep=True)[3]
    var = ops.gp_predict_var(spec, fac, X, Xs)
    fac.free()
    L = cholesky(O.kernel_matrix(kind, X, **kw) + np.diag(e ** 2), lower=True)
    ref = np.empty(len(Xs))
    for c0 in range(0, len(Xs), 8192):
        V = solve_triangular(L, O.kernel_matrix(kind, Xs[c0:c0 + 8192], X, **kw).T, lower=True)
        ref[c0:c0 + 8192] = spec.amp - np.einsum("ij,ij->j", V, V)
    np.testing.assert_allclose(var, ref, rtol=0, atol=1e-10 * spec.amp)


@pytest.mark.parametrize("kernel, amp", [("1.0**2 * RBF(0.1) + WhiteKernel(1e-4)", 1.0),
                                         ("0.7**2 * Matern(length_scale=0.3, nu=1.5)", 0.49)])
def test_dense_route_variance(kernel, amp):
    import treegp_amd as treegp
    rng, X, y, e = _problem(700, 8)
    Xs = rng.uniform(0, 1, (900, 2))
    with pytest.raises(NotImplementedError):                  # the caller-evaluated route (tgp_gp_predict_var_dense)
        treegp.kernel_to_spec(treegp.eval_kernel(kernel))
    gp = treegp.GPInterpolation(kernel=kernel, optimizer="none", normalize=True)
    gp.initialize(X, np.sin(6 * X[:, 0]) + 0.1 * y, y_err=e)
    y_plain = gp.predict(Xs)
    y_var, var = gp.predict(Xs, return_var=True)
    y_cov, cov = gp.predict(Xs, return_cov=True)
    assert np.array_equal(y_var, y_plain) and np.array_equal(y_cov, y_plain)
    np.testing.assert_allclose(var, np.diag(cov), rtol=0, atol=1e-12 * amp)


# ---------------------------------------------------------------- through the API --------------
def _grf(kernel_skl, noise, npoints, seed=42):
    """1-D Gaussian random field drawn as the reference's tests/treegp_test_helper.py:47-104 draws it"""
    np.random.seed(seed)
    x = np.random.uniform(-10, 10, npoints).reshape((npoints, 1))
    y = np.random.multivariate_normal(np.zeros(npoints), kernel_skl(x))
    if noise is not None:
        y += np.random.normal(scale=noise, size=npoints)
        return x, y, np.ones_like(y) * noise
    return x, y, None


def test_check_interp_pattern_with_variance():
    """the reference's _check_interp (tests/test_gp_interp.py:48-69 there) with np.sqrt(var) for np.sqrt(np.diag(cov))"""
    import treegp_amd as treegp
    npoints = 40
    for ker in ["RBF", "VonKarman"]:
        for noise, white_noise, sigma, ell in ((None, 1e-5, 1.0, 2.0), (0.1, 0.0, 2.0, 2.0)):
            kernel = "%f**2 * %s(%f)" % (sigma, ker, ell)
            x, y, y_err = _grf(treegp.eval_kernel(kernel), noise, npoints)
            new_x = np.linspace(np.max(x) + 6.0 * ell, np.max(x) + 7.0 * ell, npoints).reshape((npoints, 1))
            gp = treegp.GPInterpolation(kernel=kernel, optimizer="none", white_noise=white_noise)
            gp.initialize(x, y, y_err=y_err)
            y_predict, y_var = gp.predict(x, return_var=True)
            y_std = np.sqrt(y_var)
            pull = y - y_predict
            if noise is not None:
                pull /= np.sqrt(y_err ** 2 + y_std ** 2)
            else:
                np.testing.assert_allclose(y, y_predict, atol=3.0 * white_noise)
                np.testing.assert_allclose(np.zeros_like(y_std), y_std, atol=3.0 * white_noise)
            np.testing.assert_allclose(0.0, np.mean(pull), atol=3.0 * np.std(pull) / np.sqrt(npoints))
            assert np.std(pull) <= 1.0
            gp = treegp.GPInterpolation(kernel=kernel, optimizer="none", normalize=False, white_noise=white_noise)
            gp.initialize(x, y, y_err=y_err)
            y_predict, y_var = gp.predict(new_x, return_var=True)
            np.testing.assert_allclose(np.zeros_like(y_predict), y_predict, atol=1e-5)
            np.testing.assert_allclose(sigma * np.ones(npoints), np.sqrt(y_var), atol=1e-5)


def _headline_gp(n, m, seed=11, **kw):
    import treegp_amd as treegp
    from treegp_amd.synthetic import star_field, headline_kernel_string
    X, y, y_err, Xs = star_field(n, m, seed=seed)
    gp = treegp.GPInterpolation(kernel=headline_kernel_string(), optimizer="none", **kw)
    gp.initialize(X, y, y_err=y_err)
    return gp, X, y, y_err, Xs


def test_values_bit_identical_and_variance_matches_covariance():
    gp, X, y, y_err, Xs = _headline_gp(1300, 700)
    y0 = gp.predict(Xs)
    y1, var = gp.predict(Xs, return_var=True)
    assert np.array_equal(y1, y0)
    assert var.shape == (len(Xs),)
    _, cov = gp.predict(Xs, return_cov=True)
    np.testing.assert_allclose(var, np.diag(cov), rtol=0, atol=1e-12)
    gp2, *_ = _headline_gp(1300, 700)
    y2, _ = gp2.predict(Xs, return_var=True)                  # alpha computed by the variance call itself
    assert np.array_equal(y2, y0)


@pytest.mark.parametrize("first", ["cov", "var"])
def test_variance_and_covariance_share_the_kept_factor(monkeypatch, first):
    from treegp_amd import ops
    calls = []
    real = ops.gp_solve

    def counting(*a, **k):
        calls.append(k.get("keep"))
        return real(*a, **k)

    monkeypatch.setattr(ops, "gp_solve", counting)
    gp, X, y, y_err, Xs = _headline_gp(900, 400)
    second = "var" if first == "cov" else "cov"
    out1 = gp.predict(Xs, **{"return_" + first: True})[1]
    assert len(calls) == 1
    out2 = gp.predict(Xs[::-1], **{"return_" + second: True})[1]
    assert len(calls) == 1, "the second kept-factor call factorised again"
    var = out1 if first == "var" else out2[::-1]
    cov = out1 if first == "cov" else out2[::-1, ::-1]
    np.testing.assert_allclose(var, np.diag(cov), rtol=0, atol=1e-12)
    gp.predict(Xs, return_var=True)
    assert len(calls) == 1
    gp.initialize(X, y, y_err=1.5 * y_err)                    # other errors: a new factor
    gp.predict(Xs, return_var=True)
    assert len(calls) == 2


def test_normalize_and_mean_function_leave_variance_unchanged(tmp_path):
    from treegp_amd.fits_io import write_bintable_row
    gp_a, X, y, y_err, Xs = _headline_gp(1100, 500, normalize=False)
    v_a = gp_a.predict(Xs, return_var=True)[1]
    gp_b, *_ = _headline_gp(1100, 500, normalize=True)
    v_b = gp_b.predict(Xs, return_var=True)[1]
    rng = np.random.default_rng(4)
    X0 = rng.uniform(0, 1, (400, 2))
    fits = str(tmp_path / "mean.fits")
    write_bintable_row(fits, {"COORDS0": X0, "PARAMS0": 0.3 + np.cos(3 * X0[:, 0])})
    gp_c, *_ = _headline_gp(1100, 500, normalize=True, average_fits=fits)
    y_c, v_c = gp_c.predict(Xs, return_var=True)
    assert np.array_equal(y_c, gp_c.predict(Xs))
    np.testing.assert_allclose(v_b, v_a, rtol=0, atol=1e-12)
    np.testing.assert_allclose(v_c, v_a, rtol=0, atol=1e-12)

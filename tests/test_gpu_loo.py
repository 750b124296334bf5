"""GPU tests of leave-one-out cross-validation (seam S3e, tgp_factor_inv_diag, and GPInterpolation.predict_loo /
return_loo_log_predictive / predict_fields_loo): diag(K^-1) against the oracle's inverse, chunk independence, an independent
device path at N = 32 768, and the LOO predictions against deleting each point and solving again."""
import copy

import numpy as np
import pytest

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
def test_inv_diag_against_oracle_inverse(tag, n):
    from oracle import gp_oracle as O
    from treegp_amd import ops
    spec, kind, kw = _spec(tag)
    rng, X, y, e = _problem(n, 2000 + n)
    fac = ops.gp_solve(spec, X, y, e, keep=True)[3]
    d = ops.factor_inv_diag(fac)
    assert d.shape == (n,)
    ref = np.diag(np.linalg.inv(O.kernel_matrix(kind, X, **kw) + np.diag(e ** 2)))
    np.testing.assert_allclose(d, ref, rtol=1e-9, atol=0)
    fac.free()


def test_inv_diag_does_not_depend_on_the_chunk(monkeypatch):
    from treegp_amd import ops
    spec, _, _ = _spec("avk")
    rng, X, y, e = _problem(5000, 11)                          # several chunks of 1024, n not a multiple of 256
    fac = ops.gp_solve(spec, X, y, e, keep=True)[3]
    monkeypatch.delenv("TGP_INVDIAG_CHUNK", raising=False)
    monkeypatch.delenv("TGP_COV_BIG", raising=False)
    d_default = ops.factor_inv_diag(fac)
    monkeypatch.setenv("TGP_INVDIAG_CHUNK", "1024")
    d_1024 = ops.factor_inv_diag(fac)
    monkeypatch.setenv("TGP_INVDIAG_CHUNK", "1000")            # rounded up to the step
    d_1000 = ops.factor_inv_diag(fac)
    assert np.array_equal(d_1024, d_default)
    assert np.array_equal(d_1000, d_default)
    monkeypatch.delenv("TGP_INVDIAG_CHUNK")
    monkeypatch.setenv("TGP_COV_BIG", "0")                     # the 128-block substitution (chunks on a 256 grid)
    d_128 = ops.factor_inv_diag(fac)
    monkeypatch.setenv("TGP_INVDIAG_CHUNK", "768")
    d_128c = ops.factor_inv_diag(fac)
    np.testing.assert_allclose(d_128, d_default, rtol=1e-12, atol=0)
    assert np.array_equal(d_128c, d_128)
    fac.free()


def test_inv_diag_at_32768_against_identity_rows_through_the_variance():
    from treegp_amd import ops
    spec, _, _ = _spec("rbf")
    n = 32768
    rng, X, y, e = _problem(n, 12)
    fac = ops.gp_solve(spec, X, y, e, keep=True)[3]
    d = ops.factor_inv_diag(fac)
    assert d.shape == (n,) and np.all(d > 0)
    idx = {0, 1, 1023, 1024, n - 1}
    for b in range(4096, n, 4096):                             # every chunk boundary of the default and of 4096-row chunks
        idx.update((b - 1, b))
    idx = sorted(idx)
    rest = np.setdiff1d(np.arange(n), idx)
    idx = np.sort(np.concatenate([idx, rng.choice(rest, 64 - len(idx), replace=False)]))
    E = np.zeros((len(idx), n))
    E[np.arange(len(idx)), idx] = 1.0
    ref = -ops.gp_predict_var_dense(fac, E, np.zeros(len(idx)))
    np.testing.assert_allclose(d[idx], ref, rtol=1e-10, atol=0)
    fac.free()


def _oracle_kernel(gp):
    """(K0 (n, n) latent covariance, k(x_i, x_i)) evaluated independently of the device: the oracle for the kinds the device
    describes, scikit-learn's own host evaluation for the dense route"""
    from oracle import gp_oracle as O
    from treegp_amd import _lib
    from treegp_amd.kernels import kernel_to_spec
    try:
        spec = kernel_to_spec(gp.kernel)
    except NotImplementedError:
        return gp.kernel(gp._X), 1.0
    kind = {_lib.TGP_RBF: "gauss", _lib.TGP_ARBF: "gauss", _lib.TGP_VK: "vk", _lib.TGP_AVK: "avk"}[spec.kind]
    return O.kernel_matrix(kind, gp._X, amp=spec.amp, a=spec.a, b=spec.b, c=spec.c, ell=spec.ell), spec.amp


def _brute_loo(gp, idx):
    """point i removed, the residual problem solved again with _mean and the mean function held fixed:
    (y_loo, latent var, noisy var) at the indices"""
    K0, _ = _oracle_kernel(gp)
    r = gp._y - gp._mean - gp._spatial_average
    s2 = np.asarray(gp._y_err) ** 2
    out = []
    for i in idx:
        keep = np.delete(np.arange(len(r)), i)
        w = np.linalg.solve(K0[np.ix_(keep, keep)] + np.diag(s2[keep]), K0[i, keep])
        v = K0[i, i] - K0[i, keep].dot(w)
        out.append((w.dot(r[keep]) + gp._mean + gp._spatial_average[i], v, v + s2[i]))
    return np.array(out).T


def _gp(kernel, n, seed, normalize=True, white_noise=0.0):
    import treegp_amd as tg
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    y = np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.3 + 0.05 * rng.standard_normal(n)
    e = rng.uniform(0.02, 0.1, n)
    gp = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=normalize, white_noise=white_noise)
    gp.initialize(X, y, y_err=e)
    return gp, rng


@pytest.mark.parametrize("kernel,normalize", [
    ("1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))", False),
    ("1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))", True),
    ("0.8**2 * VonKarman(length_scale=0.4)", True),
    ("1.0**2 * RBF(0.3) + WhiteKernel(1e-3)", True),
    ("0.7**2 * Matern(length_scale=0.3, nu=1.5)", False),
])
def test_predict_loo_against_deleting_each_point(kernel, normalize):
    gp, rng = _gp(kernel, 700, 21, normalize=normalize)
    y_loo, var_loo = gp.predict_loo(return_var=True)
    assert y_loo.shape == var_loo.shape == (700,)
    idx = np.concatenate([[0, 699], rng.choice(np.arange(1, 699), 6, replace=False)])
    ref_y, ref_v, _ = _brute_loo(gp, idx)
    _, amp = _oracle_kernel(gp)
    np.testing.assert_allclose(y_loo[idx], ref_y, rtol=0, atol=1e-9 * amp)
    np.testing.assert_allclose(var_loo[idx], ref_v, rtol=0, atol=1e-9 * amp)
    assert np.array_equal(gp.predict_loo(), y_loo)


def test_predict_loo_of_one_point_is_the_prior():
    import treegp_amd as tg
    gp = tg.GPInterpolation(kernel="1.7**2 * RBF(0.3)", optimizer="none", normalize=False)
    gp.initialize(np.array([[0.3, 0.4]]), np.array([2.5]), y_err=np.array([0.1]))
    y_loo, var_loo = gp.predict_loo(return_var=True)
    amp = 1.7 ** 2
    np.testing.assert_allclose(y_loo, [gp._mean + gp._spatial_average[0]], rtol=0, atol=1e-12 * 2.5)
    np.testing.assert_allclose(var_loo, [amp], rtol=1e-12)


def test_loo_log_predictive_against_brute_force():
    gp, _ = _gp("1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))", 200, 31)
    idx = np.arange(200)
    ref_y, _, ref_s = _brute_loo(gp, idx)
    ref = np.sum(-0.5 * np.log(2 * np.pi * ref_s) - 0.5 * (gp._y - ref_y) ** 2 / ref_s)
    alpha0, factor0 = gp._alpha, gp._factor
    got = gp.return_loo_log_predictive()
    np.testing.assert_allclose(got, ref, rtol=1e-10)
    assert gp._alpha is alpha0 and gp._factor is factor0          # its own temporary factor
    # theta= is the value of the cloned kernel
    theta = gp.kernel.theta + 0.1
    got_theta = gp.return_loo_log_predictive(theta=theta)
    gp2 = copy.deepcopy(gp)
    gp2.kernel = gp.kernel.clone_with_theta(theta)
    np.testing.assert_allclose(got_theta, gp2.return_loo_log_predictive(), rtol=1e-12)
    assert got_theta != got
    # a kernel whose matrix is not positive definite scores -inf, as the likelihood does
    import treegp_amd as tg
    gp3 = tg.GPInterpolation(kernel="1.0**2 * AnisotropicRBF(scale_length=[50., 50.])", optimizer="none", normalize=False)
    gp3.initialize(gp._X, gp._y, y_err=np.zeros(200))
    assert gp3.return_log_likelihood() == -np.inf
    assert gp3.return_loo_log_predictive() == -np.inf


@pytest.mark.parametrize("kernel", ["1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))",
                                    "1.0**2 * RBF(0.3) + WhiteKernel(1e-3)"])
def test_predict_fields_loo_against_separate_objects(kernel):
    import treegp_amd as tg
    gp, rng = _gp(kernel, 600, 41)
    Y = np.stack([gp._y, 2.0 * gp._y - 1.0, rng.standard_normal(600)])
    got = gp.predict_fields_loo(Y)
    assert got.shape == (3, 600)
    assert gp._alpha is None and gp._factor is None
    for f in range(3):
        one = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=True)
        one.initialize(gp._X, Y[f], y_err=gp._y_err)
        np.testing.assert_allclose(got[f], one.predict_loo(), rtol=0, atol=1e-12 * max(1.0, np.abs(Y[f]).max()))


@pytest.mark.parametrize("kernel", ["1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))",
                                    "1.0**2 * RBF(0.3) + WhiteKernel(1e-3)"])
def test_predict_loo_and_predict_var_share_the_kept_factor(kernel):
    gp, rng = _gp(kernel, 500, 51)
    gp.predict_loo()
    factor = gp._factor
    assert factor is not None
    Xs = rng.uniform(0, 1, (40, 2))
    gp.predict(Xs, return_var=True)
    assert gp._factor is factor
    gp2, _ = _gp(kernel, 500, 51)
    gp2.predict(Xs, return_var=True)
    factor2 = gp2._factor
    gp2.predict_loo(return_var=True)
    assert gp2._factor is factor2

"""CPU-only checks of the kernel sums (include/tgp.h, seams S1s / S2s): kernels.kernel_to_sum_spec / device_spec /
sum_spec_jacobian, the routing of GPInterpolation and log_likelihood with the device calls replaced by NumPy stand-ins, and the
per-term likelihood gradient against central differences of a host log-likelihood."""
import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib, kernels, ops

import _ksum_refs as S


# ---- 1. kernel_to_sum_spec ---------------------------------------------------------------------------------------------------
def test_sum_spec_term_order_and_amplitudes_of_nested_sums():
    spec = kernels.kernel_to_sum_spec(tg.eval_kernel(S.SUM_B))
    assert isinstance(spec, ops.KernelSumSpec)
    assert [t.kind for t in spec.terms] == [_lib.TGP_AVK, _lib.TGP_ARBF, _lib.TGP_VK, _lib.TGP_RBF]
    np.testing.assert_allclose([t.amp for t in spec.terms], [0.09, 0.25, 0.04, 0.49], rtol=1e-15)
    assert (spec.terms[0].a, spec.terms[0].b, spec.terms[0].c) == (40.0, -9.0, 25.0)
    assert (spec.terms[1].a, spec.terms[1].b, spec.terms[1].c) == (30.0, 4.0, 20.0)
    assert spec.terms[2].ell == 0.4
    np.testing.assert_allclose([spec.terms[3].a, spec.terms[3].c], [100.0, 100.0], rtol=1e-14)
    assert spec.amp == ((0.3 ** 2 + 0.5 ** 2) + 0.2 ** 2) + 0.7 ** 2
    # scikit-learn's own order, k1 before k2, however the sum is nested
    right = tg.eval_kernel("1.0**2 * RBF(1.0) + (2.0**2 * RBF(2.0) + 3.0**2 * VonKarman(length_scale=3.0))")
    assert [t.amp for t in kernels.kernel_to_sum_spec(right).terms] == [1.0, 4.0, 9.0]
    c = spec.to_c()
    assert c.nterms == 4 and c.term[2].kind == _lib.TGP_VK and c.term[3].amp == spec.terms[3].amp
    assert kernels.device_spec(tg.eval_kernel(S.SUM_A)).terms[1].kind == _lib.TGP_ARBF
    assert isinstance(kernels.device_spec(tg.eval_kernel("2.0**2 * RBF(0.5)")), ops.KernelSpec)


@pytest.mark.parametrize("kern", ["RBF(1.0) + WhiteKernel(0.01)",
                                  "1.0**2 * RBF(1.0) + 0.5**2 * RBF(2.0) + WhiteKernel(0.01)",
                                  "2.0**2 * (RBF(1.0) + RBF(2.0))",
                                  "RBF(1.0) + RBF(2.0) + RBF(3.0) + RBF(4.0) + RBF(5.0)",
                                  "RBF(1.0) + Matern(length_scale=1.0, nu=1.5)",
                                  "RBF(1.0) + RBF(1.0) * RBF(2.0)",
                                  "2.0**2 * RBF(1.0)"])
def test_sum_spec_rejects_everything_else(kern):
    k = tg.eval_kernel(kern)
    with pytest.raises(NotImplementedError):
        kernels.kernel_to_sum_spec(k)
    if kern != "2.0**2 * RBF(1.0)":                      # (a single kernel: device_spec describes it, as a KernelSpec)
        with pytest.raises(NotImplementedError):
            kernels.device_spec(k)


@pytest.mark.parametrize("kern", [S.SUM_A, S.SUM_B, "RBF(1.0) + RBF(2.0)"])
def test_kernel_to_spec_still_raises_for_every_sum(kern):
    with pytest.raises(NotImplementedError):
        tg.kernel_to_spec(tg.eval_kernel(kern))


def test_the_c_abi_declares_every_sum_entry_with_its_namesakes_prototype():
    pairs = {"tgp_kernel_matrix_sum": "tgp_kernel_matrix", "tgp_d_kbuild_lower_sum": "tgp_d_kbuild_lower",
             "tgp_gp_solve_sum": "tgp_gp_solve", "tgp_gp_predict_sum": "tgp_gp_predict",
             "tgp_gp_predict_grad_sum": "tgp_gp_predict_grad", "tgp_gp_predict_cov_sum": "tgp_gp_predict_cov",
             "tgp_gp_predict_var_sum": "tgp_gp_predict_var", "tgp_gp_loglik_grad_sum": "tgp_gp_loglik_grad_any"}
    for new, old in pairs.items():
        res, args = _lib.SIGNATURES[new]
        ores, oargs = _lib.SIGNATURES[old]
        assert res is ores and len(args) == len(oargs)
        for a, o in zip(args, oargs):
            assert a is o or (a._type_ is _lib.TgpKernelSum and o._type_ is _lib.TgpKernel)
    assert _lib.TGP_SUM_MAX == 4
    import ctypes
    assert ctypes.sizeof(_lib.TgpKernelSum) == 8 + 4 * ctypes.sizeof(_lib.TgpKernel)


# ---- 2. sum_spec_jacobian ----------------------------------------------------------------------------------------------------
def test_sum_jacobian_block_structure():
    k = tg.eval_kernel(S.SUM_B)
    J = kernels.sum_spec_jacobian(k)
    leaves = [k.k1.k1.k1, k.k1.k1.k2, k.k1.k2, k.k2]
    assert J.shape == (len(k.theta), 16) and len(k.theta) == 4 + 4 + 2 + 2
    row = 0
    for t, leaf in enumerate(leaves):
        b = kernels.spec_jacobian(leaf, von_karman=True)
        np.testing.assert_array_equal(J[row:row + len(b), 4 * t:4 * t + 4], b)
        rest = np.delete(J[row:row + len(b)], np.s_[4 * t:4 * t + 4], axis=1)
        assert not rest.any()
        row += len(b)
    assert row == len(k.theta)
    with pytest.raises(NotImplementedError):
        kernels.sum_spec_jacobian(tg.eval_kernel("RBF(1.0) + WhiteKernel(0.1)"))
    with pytest.raises(NotImplementedError):
        kernels.sum_spec_jacobian(tg.eval_kernel("2.0**2 * RBF(1.0)"))


def test_sum_jacobian_drops_the_rows_of_fixed_hyperparameters():
    k = tg.eval_kernel("ConstantKernel(0.09, constant_value_bounds='fixed') * AnisotropicVonKarman(invLam=array([[40., -9.], "
                       "[-9., 25.]])) + 0.5**2 * RBF(0.1, length_scale_bounds='fixed')")
    J = kernels.sum_spec_jacobian(k)
    assert J.shape == (len(k.theta), 8) and len(k.theta) == 3 + 1
    assert not J[:3, 0].any() and not J[:3, 4:].any()            # the AVK's three thetas: a, b, c of term 0 only
    np.testing.assert_array_equal(J[3], [0, 0, 0, 0, 1.0, 0, 0, 0])   # log amp of term 1; its length scale is fixed


@pytest.mark.parametrize("kern", [S.SUM_A, S.SUM_B])
def test_sum_jacobian_equals_central_differences_of_the_specs_numbers(kern):
    """d (log amp_t, a_t, b_t, c_t) / d theta_k by central differences (step 1e-6: truncation ~1e-12 relative, rounding
    ~1e-16 / 1e-6 of numbers up to 100) against the analytic rows, to 1e-7 of the largest entry"""
    k = tg.eval_kernel(kern)
    J = kernels.sum_spec_jacobian(k)
    h = 1e-6
    for i in range(len(k.theta)):
        up, dn = np.array(k.theta), np.array(k.theta)
        up[i] += h
        dn[i] -= h
        num = (S.spec_numbers(kernels.kernel_to_sum_spec(k.clone_with_theta(up)))
               - S.spec_numbers(kernels.kernel_to_sum_spec(k.clone_with_theta(dn)))) / (2 * h)
        np.testing.assert_allclose(J[i], num, rtol=0, atol=1e-7 * max(np.abs(J).max(), 1.0))


# ---- 3. routing --------------------------------------------------------------------------------------------------------------
class HostFactor(object):
    def __init__(self, Kinv):
        self.Kinv = Kinv

    def free(self, keep_memory=False):
        pass


def matrix_of(spec, X, Y=None):
    return S.sum_matrix(spec, X, Y) if isinstance(spec, ops.KernelSumSpec) else S.spec_matrix(spec, X, Y)


@pytest.fixture
def fake(monkeypatch):
    rec = {"solve": [], "dense": [], "predict": [], "grad": [], "grad_sum": []}

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["solve"].append(spec)
        alpha, ld, c, Kinv = S.host_solve(matrix_of(spec, X), y, np.zeros(len(y)) if y_err is None else y_err)
        return alpha, ld, c, (HostFactor(Kinv) if keep else None)

    def gp_solve_dense(K, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["dense"].append(len(K))
        alpha, ld, c, Kinv = S.host_solve(K, y, np.zeros(len(y)) if y_err is None else y_err)
        return alpha, ld, c, (HostFactor(Kinv) if keep else None)

    def gp_predict(spec, X, alpha, Xs, ctx=None):
        rec["predict"].append(spec)
        return matrix_of(spec, Xs, X).dot(alpha)

    def gp_predict_grad(spec, X, alpha, Xs, ctx=None):
        rec["grad"].append(spec)
        return np.zeros((len(Xs), 2))

    def gp_loglik_grad_sum(spec, factor, X, alpha, ctx=None):
        rec["grad_sum"].append(spec)
        return S.host_grad_rows(spec, X, alpha, factor.Kinv)

    def no_resident(*a, **k):
        raise AssertionError("a sum has no resident solve")

    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_solve_dense", gp_solve_dense)
    monkeypatch.setattr(ops, "gp_predict", gp_predict)
    monkeypatch.setattr(ops, "gp_predict_grad", gp_predict_grad)
    monkeypatch.setattr(ops, "gp_loglik_grad_sum", gp_loglik_grad_sum)
    monkeypatch.setattr(ops, "gp_solve_resident", no_resident)
    monkeypatch.setattr(ops, "kernel_matrix", lambda spec, X, Y=None, ctx=None: matrix_of(spec, X, Y))
    monkeypatch.setattr(ops, "_dist_engine", lambda n, ctx: None)
    return rec


def make_gp(kern, n=40):
    X, y, e, _ = S.data(n, 7)
    gp = tg.GPInterpolation(kernel=kern, optimizer="none", normalize=True)
    gp.initialize(np.array(X), np.array(y), y_err=np.array(e))
    return gp


def test_a_sum_of_parametrised_kernels_never_takes_the_dense_route(fake):
    gp = make_gp(S.SUM_A)
    Xs = S.data(40, 7)[3]
    yp = gp.predict(Xs)
    assert not fake["dense"] and len(fake["solve"]) == 1 and len(fake["predict"]) == 1
    assert isinstance(fake["solve"][0], ops.KernelSumSpec) and isinstance(fake["predict"][0], ops.KernelSumSpec)
    assert [t.kind for t in fake["solve"][0].terms] == [_lib.TGP_AVK, _lib.TGP_ARBF]
    K = gp.kernel(gp._X)                                     # the kernel object's own evaluation (ops.kernel_matrix per leaf)
    alpha = S.host_solve(K, gp._residual(), gp._y_err)[0]
    np.testing.assert_allclose(yp, gp.kernel(Xs, Y=gp._X).dot(alpha) + gp._mean, rtol=1e-10)
    g = gp.predict_gradient(Xs)
    assert g.shape == (7, 2) and isinstance(fake["grad"][0], ops.KernelSumSpec) and not fake["dense"]
    assert isinstance(gp.return_log_likelihood(), float) and not fake["dense"]
    assert isinstance(fake["solve"][-1], ops.KernelSumSpec)


def test_white_kernel_trees_keep_the_dense_route(fake):
    gp = make_gp("RBF(1.0) + WhiteKernel(0.01)")
    gp.predict(S.data(40, 7)[3])
    assert fake["dense"] == [40] and not fake["solve"] and not fake["predict"]
    with pytest.raises(NotImplementedError, match="WhiteKernel"):
        gp.predict_gradient(S.data(40, 7)[3])


def test_sums_keep_the_dense_route_while_the_multi_gpu_engine_is_active(fake, monkeypatch):
    monkeypatch.setattr(ops, "_dist_engine", lambda n, ctx: object())
    gp = make_gp(S.SUM_A)
    gp.predict(S.data(40, 7)[3])
    assert fake["dense"] == [40] and not fake["solve"] and not fake["predict"]
    like = tg.log_likelihood(gp._X, gp._residual(), gp._y_err)
    assert like.distributed
    like.log_likelihood(gp.kernel)
    assert fake["dense"] == [40, 40] and not fake["solve"]


def test_factor_fingerprint_hashes_every_term():
    X, _, e, _ = S.data(40, 7)
    base = kernels.kernel_to_sum_spec(tg.eval_kernel(S.SUM_A))
    other = kernels.kernel_to_sum_spec(tg.eval_kernel(S.SUM_A.replace("[4., 20.]", "[4., 21.]")))
    assert base.terms[0].__repr__() == other.terms[0].__repr__() and base.terms[1].c != other.terms[1].c
    fp = tg.GPInterpolation._factor_fingerprint
    assert fp(base, X, e) == fp(kernels.kernel_to_sum_spec(tg.eval_kernel(S.SUM_A)), X, e)
    assert fp(base, X, e) != fp(other, X, e)
    assert fp(base, X, e) != fp(base.terms[0], X, e)
    single = ops.KernelSpec(_lib.TGP_ARBF, amp=1.3, a=30.0, b=4.0, c=20.0)
    assert fp(single, X, e) == fp(ops.KernelSpec(_lib.TGP_ARBF, amp=1.3, a=30.0, b=4.0, c=20.0), X, e)


def test_the_kept_factor_follows_the_second_terms_parameters(fake, monkeypatch):
    gp = make_gp(S.SUM_A)
    Xs = S.data(40, 7)[3]
    monkeypatch.setattr(ops, "gp_predict_var", lambda spec, factor, X, Xq, ctx=None: np.zeros(len(Xq)))
    gp.predict(Xs, return_var=True)
    f0 = gp._factor
    gp.predict(Xs, return_var=True)
    assert gp._factor is f0 and len(fake["solve"]) == 1
    theta = np.array(gp.kernel.theta)
    theta[-1] += 0.1                                         # a parameter of the SECOND term only
    gp.kernel = gp.kernel.clone_with_theta(theta)
    gp.predict(Xs, return_var=True)
    assert gp._factor is not f0 and len(fake["solve"]) == 2


# ---- 4. the exact gradient ---------------------------------------------------------------------------------------------------
def test_sum_gradient_equals_central_differences_of_the_host_likelihood(fake, monkeypatch):
    """log_likelihood_gradient(any_kind=True) of an AVK + ARBF sum at n = 120, the device calls replaced by the dense host
    formulas (per-term pair sums against the SUM's K^-1, mapped through sum_spec_jacobian), against central differences of the
    host log L in theta.  Step 1e-5: rounding ~2 eps |log L| / h = 2e-16 * 3e2 / 1e-5 = 6e-9 absolute, truncation h^2 |f'''| / 6
    below that; the bound is 1e-8 of the largest component (44 here: 4.4e-7 absolute; measured 9e-10)."""
    n = 120
    X, y, e, _ = S.data(n, 7)
    k = tg.eval_kernel(S.SUM_A)
    like = tg.log_likelihood(np.array(X), np.array(y), np.array(e))
    ll, grad = like.log_likelihood_gradient(k, any_kind=True)
    assert len(fake["grad_sum"]) == 1 and not fake["dense"] and grad.shape == (len(k.theta),)

    def host_ll(theta):
        spec = kernels.kernel_to_sum_spec(k.clone_with_theta(theta))
        _, ld, c, _ = S.host_solve(S.sum_matrix(spec, X), y, e)
        return -0.5 * c - 0.5 * n * np.log(2 * np.pi) - 0.5 * ld
    assert ll == pytest.approx(host_ll(np.array(k.theta)), rel=1e-13)
    h = 1e-5
    fd = np.zeros(len(k.theta))
    for i in range(len(k.theta)):
        up, dn = np.array(k.theta), np.array(k.theta)
        up[i] += h
        dn[i] -= h
        fd[i] = (host_ll(up) - host_ll(dn)) / (2 * h)
    np.testing.assert_allclose(grad, fd, rtol=0, atol=1e-8 * np.abs(fd).max())
    # without any_kind the sum has no analytic gradient, as today
    with pytest.raises(NotImplementedError):
        like.log_likelihood_gradient(k)


def test_exact_gradient_is_used_for_sums_under_analytic_vk_only(fake, monkeypatch):
    X, y, e, _ = S.data(60, 7)
    k = tg.eval_kernel(S.SUM_A)
    for mode, want in (("auto", False), ("fd", False), ("analytic-vk", True)):
        monkeypatch.setenv("TGP_ML_GRADIENT", mode)
        like = tg.log_likelihood(np.array(X), np.array(y), np.array(e))
        assert like._use_exact_gradient(k) is want, mode
    monkeypatch.setenv("TGP_ML_GRADIENT", "analytic")
    with pytest.raises(NotImplementedError):
        tg.log_likelihood(np.array(X), np.array(y), np.array(e))._use_exact_gradient(k)
    monkeypatch.setenv("TGP_ML_GRADIENT", "analytic-vk")
    with pytest.raises(NotImplementedError):
        tg.log_likelihood(np.array(X), np.array(y), np.array(e))._use_exact_gradient(tg.eval_kernel("RBF(1.0) + WhiteKernel(0.1)"))


def test_ops_sum_spec_limits():
    t = ops.KernelSpec(_lib.TGP_RBF)
    assert len(ops.KernelSumSpec([t]).terms) == 1
    for bad in ([], [t] * 5):
        with pytest.raises(ValueError):
            ops.KernelSumSpec(bad)

"""CPU-only checks of the exact likelihood gradient of the von Karman kernels (include/tgp.h, seam S2h): the formulas of the
dense reference against central differences of its own log L, spec_jacobian(kernel, von_karman=True), the C ABI's surface, and
the routing of TGP_ML_GRADIENT=analytic-vk and solve_many(gradient="analytic-vk") against NumPy stand-ins that evaluate the true
von Karman K and dK."""
import os
import re
import sys

import numpy as np
import pytest
from scipy import optimize

import treegp_amd as tg
import treegp_amd.fit_many  # noqa: F401
from treegp_amd import _lib, ops
from treegp_amd.kernels import kernel_to_spec, spec_jacobian

import _vk_loglik_grad_refs as R

fit_many = sys.modules["treegp_amd.fit_many"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the formulas ---------------------------------------------------------------------------------------------------------------
def central(fun, p):
    h = 1e-5 * max(abs(p), 1.0)
    return (fun(p + h) - fun(p - h)) / (2.0 * h)


def test_reference_gradient_equals_central_differences_of_its_own_likelihood():
    """d log L / d (log amp, a, b, c) for a sheared AnisotropicVonKarman and d log L / d log ell for VonKarman through the new
    spec_jacobian row: the four sums against central differences of the same dense log L, 1e-8 relative"""
    n = 129
    X, y, y_err = R.data_a(n)
    amp, (a, b, c) = R.AMP, (40.0, -9.0, 25.0)
    _, _, ref, _ = R.solve_grad(R.TGP_AVK, X, y, y_err, amp, a, b, c)
    fd = [central(lambda t: R.log_likelihood(R.TGP_AVK, X, y, y_err, np.exp(t), a, b, c), np.log(amp)),
          central(lambda t: R.log_likelihood(R.TGP_AVK, X, y, y_err, amp, t, b, c), a),
          central(lambda t: R.log_likelihood(R.TGP_AVK, X, y, y_err, amp, a, t, c), b),
          central(lambda t: R.log_likelihood(R.TGP_AVK, X, y, y_err, amp, a, b, t), c)]
    np.testing.assert_allclose(ref, fd, rtol=1e-8, atol=0)
    ell = 0.3
    k = tg.eval_kernel("0.7**2 * VonKarman(length_scale=0.3)")
    _, _, g4, _ = R.solve_grad(R.TGP_VK, X, y, y_err, amp, ell=ell)
    grad = spec_jacobian(k, von_karman=True).dot(g4)                       # theta = (log amp, log ell)
    fd = [central(lambda t: R.log_likelihood(R.TGP_VK, X, y, y_err, np.exp(t), ell=ell), np.log(amp)),
          central(lambda t: R.log_likelihood(R.TGP_VK, X, y, y_err, amp, ell=np.exp(t)), np.log(ell))]
    np.testing.assert_allclose(grad, fd, rtol=1e-8, atol=0)


def test_reference_counts_coincident_points_without_a_slope_and_nothing_beyond_the_cutoff():
    f, w = R.profile(np.array([0.0, 1e-3, 0.5, R.K56_XMAX / (2 * np.pi) * 1.0001, 1e3]))
    assert f[0] == 1.0 and w[0] == 0.0
    assert 0 < f[2] < f[1] < 1 and w[1] > w[2] > 0
    assert f[3] == 0.0 and w[3] == 0.0 and f[4] == 0.0 and w[4] == 0.0
    h = 1e-6                                                              # w = -f' / u
    fp = (R.profile(np.array([0.5 + h]))[0][0] - R.profile(np.array([0.5 - h]))[0][0]) / (2 * h)
    assert -fp / 0.5 == pytest.approx(w[2], rel=1e-8)


# ---- 2. spec_jacobian --------------------------------------------------------------------------------------------------------------
def spec4(kernel):
    s = kernel_to_spec(kernel)
    a, b, c = R.abc(s.kind, s.a, s.b, s.c, s.ell)
    return np.array([np.log(s.amp), a, b, c])


@pytest.mark.parametrize("kern,fixed", [
    ("0.7**2 * VonKarman(length_scale=0.3)", False),
    ("0.7**2 * AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]]))", False),
    ("1.3**2 * AnisotropicVonKarman(scale_length=[0.2])", False),
    ("AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]])) * 1.1**2", False),
    ("0.7**2 * AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]]))", True),
    ("0.7**2 * VonKarman(length_scale=0.3)", True),
])
def test_spec_jacobian_with_von_karman_against_finite_differences(kern, fixed):
    k = tg.eval_kernel(kern)
    if fixed:
        const = k.k1 if hasattr(k.k1, "constant_value") else k.k2
        const.constant_value_bounds = "fixed"
        assert spec_jacobian(const, von_karman=True).shape == (0, 4)
    theta = k.theta.copy()
    jac = spec_jacobian(k, von_karman=True)
    assert jac.shape == (len(theta), 4)
    for i in range(len(theta)):
        h = 1e-6
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd = (spec4(k.clone_with_theta(tp)) - spec4(k.clone_with_theta(tm))) / (2 * h)
        np.testing.assert_allclose(jac[i], fd, rtol=1e-7, atol=1e-7 * max(np.abs(fd).max(), 1.0))
    with pytest.raises(NotImplementedError):
        spec_jacobian(k)
    with pytest.raises(TypeError):
        spec_jacobian(k, True)                                              # keyword only


def test_spec_jacobian_keeps_its_old_answers():
    g = tg.eval_kernel("0.7**2 * AnisotropicRBF(invLam=array([[40., -9.], [-9., 25.]]))")
    assert np.array_equal(spec_jacobian(g), spec_jacobian(g, von_karman=True))
    r = tg.eval_kernel("0.7**2 * RBF(0.3)")
    assert np.array_equal(spec_jacobian(r), spec_jacobian(r, von_karman=True))
    with pytest.raises(NotImplementedError):
        spec_jacobian(tg.eval_kernel("1.0 * VonKarman(length_scale=[0.3, 0.2])"), von_karman=True)
    with pytest.raises(NotImplementedError):
        spec_jacobian(tg.eval_kernel("1.0 * Matern(length_scale=0.3, nu=1.5)"), von_karman=True)
    fixed = tg.eval_kernel("1.0 * VonKarman(length_scale=0.3)")
    fixed.k2.length_scale_bounds = "fixed"
    assert spec_jacobian(fixed.k2, von_karman=True).shape == (0, 4)


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------------
PAIRS = [("tgp_gp_loglik_grad_any", "tgp_gp_loglik_grad"), ("tgp_d_gp_solve_grad_any", "tgp_d_gp_solve_grad"),
         ("tgp_gp_solve_grad_batch_any", "tgp_gp_solve_grad_batch")]


def test_the_three_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "tgp.h")).read()
    for new, old in PAIRS:
        decl = {}
        for name in (new, old):
            m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
            assert m, name
            decl[name] = len(m.group(1).split(","))
        assert decl[new] == decl[old]
        assert _lib.SIGNATURES[new][0] is _lib.SIGNATURES[old][0]
        assert _lib.SIGNATURES[new][1] == _lib.SIGNATURES[old][1] and len(_lib.SIGNATURES[new][1]) == decl[new]
    assert "S2h" in header and "kernels.py:278-288" in header               # a seam of its own, with what the reference lacks
    lib = _lib.load_library()                                               # (loading binds every signature; no device needed)
    for new, _ in PAIRS:
        fn = getattr(lib, new)
        assert fn.argtypes == _lib.SIGNATURES[new][1]


# ---- 4. mode selection and routing -------------------------------------------------------------------------------------------------
def test_analytic_vk_mode_takes_all_four_kinds(monkeypatch):
    mod = sys.modules["treegp_amd.log_likelihood"]
    small = np.zeros((100, 2))
    kinds = ["1.0**2 * RBF(0.3)", "1.0**2 * AnisotropicRBF(scale_length=[0.3, 0.2])", "1.0**2 * VonKarman(length_scale=0.3)",
             "1.0**2 * AnisotropicVonKarman(scale_length=[0.3, 0.2])"]
    monkeypatch.setenv("TGP_ML_GRADIENT", "analytic-vk")
    ll = mod.log_likelihood(small, None, None)
    assert ll.gradient == "analytic-vk"
    for kern in kinds:
        assert ll._use_exact_gradient(tg.eval_kernel(kern)) is True
    with pytest.raises(NotImplementedError, match="analytic-vk"):
        ll._use_exact_gradient(tg.eval_kernel("1.0**2 * Matern(length_scale=0.3, nu=1.5)"))
    with pytest.raises(NotImplementedError, match="analytic-vk"):
        ll._use_exact_gradient(tg.eval_kernel("1.0**2 * VonKarman(length_scale=[0.3, 0.2])"))
    monkeypatch.setenv("TGP_ML_GRADIENT", "analytic")                       # the old mode keeps refusing them
    with pytest.raises(NotImplementedError, match="no analytic derivative"):
        mod.log_likelihood(small, None, None)._use_exact_gradient(tg.eval_kernel(kinds[2]))


def test_log_likelihood_gradient_any_kind_uses_the_new_entries(monkeypatch):
    mod = sys.modules["treegp_amd.log_likelihood"]
    X, y, y_err = R.data_a(40)
    seen = []

    class Factor(object):
        def free(self, keep_memory=False):
            seen.append("free")

    def gp_solve(spec, X_, y_, e_, keep=False, ctx=None, **kw):
        ld, chi2, _, _ = R.spec_solve_grad(spec, X_, y_, e_)
        return "alpha", ld, chi2, Factor()

    def gp_loglik_grad_any(spec, factor, X_, alpha, ctx=None):
        seen.append("any")
        return R.spec_solve_grad(spec, X_, y, y_err)[2]

    def old(*a, **k):
        raise AssertionError("the Gaussian-only entry was called")
    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_loglik_grad_any", gp_loglik_grad_any)
    monkeypatch.setattr(ops, "gp_loglik_grad", old)
    monkeypatch.setattr(ops, "gp_solve_grad_resident", old)
    ll = mod.log_likelihood(X, y, y_err)
    ll.distributed = False
    for kern, kind in (("0.7**2 * VonKarman(length_scale=0.3)", R.TGP_VK),
                       ("0.7**2 * AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]]))", R.TGP_AVK)):
        k = tg.eval_kernel(kern)
        value, grad = ll.log_likelihood_gradient(k, any_kind=True)
        s = kernel_to_spec(k)
        assert value == pytest.approx(R.log_likelihood(kind, X, y, y_err, s.amp, s.a, s.b, s.c, s.ell), rel=1e-12)
        theta = k.theta.copy()
        for i in range(len(theta)):
            def at(t, i=i):
                th = theta.copy()
                th[i] = t
                s2 = kernel_to_spec(k.clone_with_theta(th))
                return R.log_likelihood(kind, X, y, y_err, s2.amp, s2.a, s2.b, s2.c, s2.ell)
            assert grad[i] == pytest.approx(central(at, theta[i]), rel=1e-7, abs=1e-7)
    assert seen == ["any", "free", "any", "free"]
    with pytest.raises(NotImplementedError):                                # without the keyword: as before
        ll.log_likelihood_gradient(tg.eval_kernel("0.7**2 * VonKarman(length_scale=0.3)"))


@pytest.fixture
def fake(monkeypatch):
    """ops.gp_solve_grad_batch_any / gp_solve_batch on the host with the true von Karman K and dK (_vk_loglik_grad_refs); both
    record the kinds of every call; the Gaussian-only batch entry must not be reached"""
    rec = {"any": [], "solve": []}

    def batch(specs, Xs, ys, y_errs):
        ns, nmax, Xb, yb, eb = ops.pad_batch(Xs, ys, y_errs)
        lds, cs, gs, info = [], [], [], []
        for b, s in enumerate(specs):
            n = int(ns[b])
            try:
                ld, c, g4, _ = R.spec_solve_grad(s, Xb[b, :n], yb[b, :n], eb[b, :n])
                lds.append(ld), cs.append(c), gs.append(g4), info.append(0)
            except np.linalg.LinAlgError:
                lds.append(np.nan), cs.append(np.nan), gs.append(np.full(4, np.nan)), info.append(1)
        return np.array(lds), np.array(cs), np.array(gs), np.array(info)

    def gp_solve_grad_batch_any(specs, Xs, ys, y_errs=None, ctx=None):
        rec["any"].append([s.kind for s in specs])
        return batch(specs, Xs, ys, y_errs)

    def gp_solve_batch(specs, Xs, ys, y_errs=None, want_alpha=True, ctx=None):
        assert not want_alpha
        rec["solve"].append([s.kind for s in specs])
        ld, c, _, info = batch(specs, Xs, ys, y_errs)
        return None, ld, c, info

    def never(*a, **k):
        raise AssertionError("not on the analytic-vk route")
    monkeypatch.setattr(_lib, "get_ctx", never)
    monkeypatch.setattr(ops, "gp_solve", never)
    monkeypatch.setattr(ops, "gp_solve_grad_batch", never)
    monkeypatch.setattr(ops, "gp_solve_grad_batch_any", gp_solve_grad_batch_any)
    monkeypatch.setattr(ops, "gp_solve_batch", gp_solve_batch)
    return rec


def make_gp(n, seed, kernel):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 4, (n, 2))
    y = np.sin(X[:, 0]) * np.cos(0.7 * X[:, 1]) + 0.1 * rng.standard_normal(n)
    gp = tg.GPInterpolation(kernel=kernel, optimizer="log-likelihood", normalize=True)
    gp.initialize(X, y, y_err=rng.uniform(0.1, 0.2, n))
    return gp


THREE = [(26, "0.7**2 * VonKarman(length_scale=1.5)"), (31, "0.8**2 * RBF(0.7)"),
         (22, "0.9**2 * AnisotropicVonKarman(invLam=array([[1.5, 0.2], [0.2, 0.9]]))")]


def three():
    return [make_gp(n, 20 + i, k) for i, (n, k) in enumerate(THREE)]


def fit_alone(gp):
    """the same optimiser by itself against the same reference: the thetas it asks for, in order"""
    work = gp.kernel.clone_with_theta(gp.kernel.theta)
    asked = []

    def fun(theta):
        asked.append(np.array(theta))
        work.theta = theta
        ld, c, g4, _ = R.spec_solve_grad(kernel_to_spec(work), gp._X, gp._residual(), gp._y_err)
        ll = -0.5 * c - 0.5 * len(gp._X) * np.log(2 * np.pi) - 0.5 * ld
        return -ll, -spec_jacobian(work, von_karman=True).dot(g4)
    best = optimize.minimize(fun, gp.kernel.theta, jac=True, method="L-BFGS-B")["x"]
    return asked, best


def test_solve_many_analytic_vk_sends_every_kind_through_the_any_batch(fake, monkeypatch):
    gps = three()
    alone = [fit_alone(gp) for gp in three()]
    asked = {}
    real = fit_many._evaluate

    def evaluate(requests):
        for slot, (fit, theta) in requests.items():
            asked.setdefault(fit.index, []).append(np.array(theta))
        return real(requests)
    monkeypatch.setattr(fit_many, "_evaluate", evaluate)
    l0 = [fit_many._log_likelihoods([fit_many._Fit(0, gp, "fd")], [kernel_to_spec(gp.kernel)])[0] for gp in three()]
    fake["solve"].clear()
    tg.solve_many(gps, gradient="analytic-vk")
    counts = [len(a) for a, _ in alone]
    for i, gp in enumerate(gps):                                            # each object's iterates are those of its fit alone
        assert len(asked[i]) == counts[i]
        assert np.array_equal(np.array(asked[i]), np.array(alone[i][0])), "object %d" % i
        assert np.array_equal(gp.kernel.theta, gp.kernel.clone_with_theta(alone[i][1]).theta)
        assert gp._optimizer._logL > l0[i]
    # one _any call per rendezvous holding every live object, whatever its kind; the fits never go through gp_solve_batch (its one
    # call is the final log L of the three fitted kernels, as for every other route)
    assert len(fake["any"]) == max(counts) and sum(len(c) for c in fake["any"]) == sum(counts)
    assert fake["any"][0] == [_lib.TGP_VK, _lib.TGP_RBF, _lib.TGP_AVK]
    assert fake["solve"] == [[_lib.TGP_VK, _lib.TGP_RBF, _lib.TGP_AVK]]


def test_solve_many_keeps_its_other_modes(fake):
    vk = make_gp(20, 1, "0.7**2 * VonKarman(length_scale=1.5)")
    with pytest.raises(ValueError):
        tg.solve_many([vk], gradient="analytic_vk")
    with pytest.raises(NotImplementedError, match="GP 0"):
        tg.solve_many([vk], gradient="analytic")
    tg.solve_many([vk], gradient="auto")                                    # von Karman: the batched finite differences
    assert not fake["any"] and [len(c) for c in fake["solve"][:-1]] == [3] * (len(fake["solve"]) - 1)


def test_gp_solve_grad_batch_any_rejects_bad_shapes_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "get_ctx", no_device)
    monkeypatch.setattr(_lib, "load_library", no_device)
    with pytest.raises(ValueError):
        ops.gp_solve_grad_batch_any([ops.KernelSpec(2), ops.KernelSpec(3)], [np.ones((3, 2))], [np.ones(3)])
    with pytest.raises(ValueError):
        ops.gp_solve_grad_batch_any([ops.KernelSpec(2)], [np.ones((4097, 2))], [np.ones(4097)])

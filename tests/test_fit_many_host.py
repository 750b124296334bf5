"""CPU-only checks of the lockstep fits (treegp_amd.solve_many) and of ops.gp_solve_grad_batch's host side: the device calls are
replaced by NumPy stand-ins, so these tests check the rendezvous, routing, order, padding and the error paths, not the kernels."""
import ctypes
import sys
import threading

import numpy as np
import pytest
from scipy import optimize

import treegp_amd as tg
import treegp_amd.fit_many  # noqa: F401
from treegp_amd import _lib, ops
from treegp_amd.kernels import kernel_to_spec, spec_jacobian

fit_many = sys.modules["treegp_amd.fit_many"]


def spec_matrix(spec, X):
    X = _lib.as_xy(X)
    d = X[:, None, :] - X[None, :, :]
    a, b, c = (spec.ell ** -2, 0.0, spec.ell ** -2) if spec.kind == _lib.TGP_VK else (spec.a, spec.b, spec.c)   # (a Gaussian stands in)
    q = a * d[..., 0] ** 2 + 2 * b * d[..., 0] * d[..., 1] + c * d[..., 1] ** 2
    return spec.amp * np.exp(-0.5 * q), d


def host_solve_grad(spec, X, y, y_err):
    """(logdet, chi2, d logL / d (log amp, a, b, c)) in the convention of tgp_gp_loglik_grad"""
    K, d = spec_matrix(spec, X)
    Kn = K + np.diag(np.asarray(y_err, dtype=float) ** 2)
    L = np.linalg.cholesky(Kn)
    z = np.linalg.solve(L, y)
    alpha = np.linalg.solve(L.T, z)
    M = np.outer(alpha, alpha) - np.linalg.inv(Kn)
    dx, dy = d[..., 0], d[..., 1]
    g4 = np.array([0.5 * np.sum(M * K), -0.25 * np.sum(M * K * dx * dx), -0.5 * np.sum(M * K * dx * dy),
                   -0.25 * np.sum(M * K * dy * dy)])
    return 2.0 * np.log(np.diag(L)).sum(), z.dot(z), g4


@pytest.fixture
def fake(monkeypatch):
    """ops.gp_solve_grad_batch / gp_solve_batch on the host; both record the size of every call, a kernel whose amp is negative
    fails its factorisation (info > 0)"""
    rec = {"grad": [], "solve": []}

    def batch(specs, Xs, ys, y_errs):
        ns, nmax, Xb, yb, eb = ops.pad_batch(Xs, ys, y_errs)
        lds, cs, gs, info = [], [], [], []
        for b, s in enumerate(specs):
            n = int(ns[b])
            if s.amp < 0:
                lds.append(np.nan), cs.append(np.nan), gs.append(np.full(4, np.nan)), info.append(1)
                continue
            ld, c, g4 = host_solve_grad(s, Xb[b, :n], yb[b, :n], eb[b, :n])
            lds.append(ld), cs.append(c), gs.append(g4), info.append(0)
        return np.array(lds), np.array(cs), np.array(gs), np.array(info)

    def gp_solve_grad_batch(specs, Xs, ys, y_errs=None, ctx=None):
        rec["grad"].append(len(specs))
        return batch(specs, Xs, ys, y_errs)

    def gp_solve_batch(specs, Xs, ys, y_errs=None, want_alpha=True, ctx=None):
        assert not want_alpha
        rec["solve"].append(len(specs))
        ld, c, _, info = batch(specs, Xs, ys, y_errs)
        return None, ld, c, info

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "get_ctx", no_device)
    monkeypatch.setattr(ops, "gp_solve", no_device)
    monkeypatch.setattr(ops, "gp_solve_grad_batch", gp_solve_grad_batch)
    monkeypatch.setattr(ops, "gp_solve_batch", gp_solve_batch)
    return rec


def make_gp(n, seed, kernel, optimizer="log-likelihood", backend=None):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 4, (n, 2))
    y = np.sin(X[:, 0]) * np.cos(0.7 * X[:, 1]) + 0.1 * rng.standard_normal(n)
    gp = tg.GPInterpolation(kernel=kernel, optimizer=optimizer, normalize=True, backend=backend)
    gp.initialize(X, y, y_err=rng.uniform(0.1, 0.2, n))
    return gp


FIVE = [(24, "0.8**2 * RBF(0.7)"), (37, "1.2**2 * AnisotropicRBF(invLam=array([[1.5, 0.2], [0.2, 0.9]]))"), (18, "0.5**2 * RBF(1.6)"),
        (45, "1.0**2 * AnisotropicRBF(invLam=array([[0.6, 0.], [0., 2.0]]))"), (31, "1.5**2 * RBF(0.4)")]


def five():
    return [make_gp(n, 10 + i, k) for i, (n, k) in enumerate(FIVE)]


def fit_alone(gp):
    """the same optimiser by itself against the same stand-in: the thetas it asks for, in order"""
    work = gp.kernel.clone_with_theta(gp.kernel.theta)
    asked = []

    def fun(theta):
        asked.append(np.array(theta))
        work.theta = theta
        ld, c, g4 = host_solve_grad(kernel_to_spec(work), gp._X, gp._residual(), gp._y_err)
        ll = -0.5 * c - 0.5 * len(gp._X) * np.log(2 * np.pi) - 0.5 * ld
        return -ll, -spec_jacobian(work).dot(g4)
    best = optimize.minimize(fun, gp.kernel.theta, jac=True, method="L-BFGS-B")["x"]
    return asked, best


def record_requests(monkeypatch):
    asked, sizes = {}, []
    real = fit_many._evaluate

    def evaluate(requests):
        sizes.append(len(requests))
        for slot, (fit, theta) in requests.items():
            asked.setdefault(fit.index, []).append(np.array(theta))
        return real(requests)
    monkeypatch.setattr(fit_many, "_evaluate", evaluate)
    return asked, sizes


def test_lockstep_equals_sequential_and_one_call_per_rendezvous(fake, monkeypatch):
    gps = five()
    alone = [fit_alone(gp) for gp in five()]
    starts = [gp.kernel.theta.copy() for gp in gps]
    asked, sizes = record_requests(monkeypatch)
    tg.solve_many(gps)
    counts = [len(a) for a, _ in alone]
    assert len(set(counts)) > 1                                     # the objects do not all stop together
    for i, gp in enumerate(gps):
        assert len(asked[i]) == counts[i]
        assert np.array_equal(np.array(asked[i]), np.array(alone[i][0])), "object %d" % i
        assert np.array_equal(gp.kernel.theta, gp.kernel.clone_with_theta(alone[i][1]).theta)    # (theta goes through exp and log)
        # the state its own solve() leaves
        assert len(gp._init_theta) == 1 and np.array_equal(gp._init_theta[0], starts[i])
        assert gp._alpha is None and gp._factor is None
        assert np.array_equal(gp._optimizer._kernel.theta, gp.kernel.theta) and gp._optimizer._kernel is not gp.kernel
        ld, c, _ = host_solve_grad(kernel_to_spec(gp.kernel), gp._X, gp._residual(), gp._y_err)
        assert gp._optimizer._logL == pytest.approx(-0.5 * c - 0.5 * len(gp._X) * np.log(2 * np.pi) - 0.5 * ld, rel=1e-13)
    # one batched gradient call per rendezvous: as many as the longest fit needs, not the sum; objects drop out, none comes back
    assert len(fake["grad"]) == max(counts) == len(sizes)
    assert fake["grad"] == sizes and sum(fake["grad"]) == sum(counts)
    assert all(a >= b for a, b in zip(fake["grad"], fake["grad"][1:])) and fake["grad"][0] == 5
    assert fake["solve"] == [5]                                       # the final log L of all five, one call


def run_with_limit(fn, seconds=30):
    box = {}

    def target():
        try:
            box["out"] = fn()
        except BaseException as ex:                                 # noqa: B902
            box["err"] = ex
    t = threading.Thread(target=target, daemon=True)
    t.start()
    t.join(seconds)
    assert not t.is_alive(), "solve_many did not return within %d s" % seconds
    return box


def optimiser_threads():
    return [t for t in threading.enumerate() if t.name.startswith("solve_many-")]


def test_an_error_in_an_evaluation_releases_everyone(fake, monkeypatch):
    gps = five()
    before = [gp.kernel.theta.copy() for gp in gps]
    real = ops.gp_solve_grad_batch
    calls = []

    def third_call_fails(*a, **k):
        calls.append(1)
        if len(calls) == 3:
            raise _lib.TgpError("tgp_gp_solve_grad_batch failed (-2): stand-in")
        return real(*a, **k)
    monkeypatch.setattr(ops, "gp_solve_grad_batch", third_call_fails)
    box = run_with_limit(lambda: tg.solve_many(gps))
    assert isinstance(box.get("err"), _lib.TgpError) and "stand-in" in str(box["err"])
    assert not optimiser_threads()
    for gp, theta in zip(gps, before):                               # nothing half-fitted is left behind
        assert np.array_equal(gp.kernel.theta, theta) and not hasattr(gp, "_optimizer")


def test_an_error_in_an_optimiser_thread_releases_everyone(fake, monkeypatch):
    gps = five()
    real = optimize.minimize
    target = gps[2].kernel.theta.copy()

    def minimize(fun, x0, **kw):
        seen = []

        def wrapped(theta):
            seen.append(1)
            if np.array_equal(x0, target) and len(seen) == 3:
                raise KeyError("raised inside one object's objective")
            return fun(theta)
        return real(wrapped, x0, **kw)
    monkeypatch.setattr(fit_many.optimize, "minimize", minimize)
    box = run_with_limit(lambda: tg.solve_many(gps))
    assert isinstance(box.get("err"), KeyError)
    assert not optimiser_threads()


def test_routing(fake, monkeypatch):
    own = []
    monkeypatch.setattr(tg.GPInterpolation, "solve", lambda self: own.append(self))
    big = make_gp(ops.BATCH_NMAX + 1, 1, "1.0**2 * RBF(1.0)")
    dist = make_gp(20, 2, "1.0**2 * RBF(1.0)", backend="dist")
    tree = make_gp(20, 3, "RBF(1.0) + WhiteKernel(0.01)")
    pcf = make_gp(20, 4, "1.0**2 * RBF(1.0)", optimizer="two-pcf")
    aniso = make_gp(20, 5, "1.0**2 * AnisotropicRBF(invLam=array([[1., 0.], [0., 1.]]))", optimizer="anisotropic")
    none = make_gp(20, 6, "1.0**2 * RBF(1.0)", optimizer="none")
    a, b = make_gp(22, 7, "1.0**2 * RBF(1.0)"), make_gp(26, 8, "0.7**2 * VonKarman(length_scale=1.5)")
    tg.solve_many([big, a, dist, tree, pcf, b, aniso, none])
    assert own == [big, dist, tree, pcf, aniso, none]                   # their own solve(), in list order
    assert fake["grad"] and set(fake["grad"]) == {1}                    # a: the batched gradient
    assert set(fake["solve"][:-1]) == {3} and fake["solve"][-1] == 2    # b: ntheta + 1 points per rendezvous; then both log L
    for gp, fresh in ((a, make_gp(22, 7, "1.0**2 * RBF(1.0)")), (b, make_gp(26, 8, "0.7**2 * VonKarman(length_scale=1.5)"))):
        start = fit_many._log_likelihoods([fit_many._Fit(0, fresh, "fd")], [kernel_to_spec(fresh.kernel)])[0]
        assert gp._optimizer._logL > start and not np.array_equal(gp.kernel.theta, fresh.kernel.theta)


def test_gradient_argument(fake):
    vk = make_gp(20, 1, "0.7**2 * VonKarman(length_scale=1.5)")
    a = make_gp(25, 2, "1.0**2 * RBF(1.0)")
    with pytest.raises(NotImplementedError, match="GP 1"):
        tg.solve_many([a, vk], gradient="analytic")
    assert not fake["grad"] and not fake["solve"] and not hasattr(a, "_optimizer")
    with pytest.raises(ValueError):
        tg.solve_many([a], gradient="exact")
    tg.solve_many([a, vk], gradient="fd")
    assert not fake["grad"]
    assert fake["solve"][0] == 3 + 3 and fake["solve"][-1] == 2         # (ntheta + 1) points of both objects in one call
    a2 = make_gp(25, 2, "1.0**2 * RBF(1.0)")
    tg.solve_many([a2], gradient="analytic")
    assert fake["grad"]
    np.testing.assert_allclose(a2.kernel.theta, a.kernel.theta, atol=1e-3)    # both routes reach the optimum


def test_failed_factorisation_and_non_finite_values_reject_the_point(fake):
    a, b = make_gp(20, 1, "1.0**2 * RBF(1.0)"), make_gp(22, 2, "1.0**2 * RBF(1.0)")
    fits = [fit_many._Fit(0, a, "analytic"), fit_many._Fit(1, b, "fd")]
    for f in fits:
        real = f.spec_at

        def spec_at(theta, real=real):
            s, jac = real(theta)
            s.amp = -1.0                                                # the stand-ins' convention: info > 0
            return s, jac
        f.spec_at = spec_at
    out = fit_many._evaluate({0: (fits[0], a.kernel.theta), 1: (fits[1], b.kernel.theta)})
    assert out[0][0] == np.inf and np.array_equal(out[0][1], np.zeros(2))
    assert out[1][0] == np.inf and out[1][1].shape == (2,)


class FakeLib(object):
    """records what tgp_gp_solve_grad_batch is given and fills its outputs"""

    def __init__(self):
        self.seen = None

    def tgp_gp_solve_grad_batch(self, ctx, nb, ks, ns, nmax, X, y, yerr, logdet, ydota, grad, info):
        def arr(p, count, ctype=ctypes.c_double):
            return np.ctypeslib.as_array((ctype * count).from_address(p.value))
        self.seen = dict(ctx=ctx, nb=nb, nmax=nmax, ns=arr(ns, nb, ctypes.c_int64).copy(), X=arr(X, nb * nmax * 2).copy(),
                         y=arr(y, nb * nmax).copy(), yerr=None if yerr is None else arr(yerr, nb * nmax).copy(),
                         amps=[k.amp for k in ctypes.cast(ks, ctypes.POINTER(_lib.TgpKernel))[:nb]])
        arr(logdet, nb)[:] = np.arange(nb)
        arr(ydota, nb)[:] = 10 + np.arange(nb)
        arr(grad, nb * 4)[:] = np.arange(nb * 4)
        arr(info, nb, ctypes.c_int32)[:] = [0, 7][:nb]
        return 0


def test_gp_solve_grad_batch_pads_and_returns(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    specs = [ops.KernelSpec(0, 2.0), ops.KernelSpec(1, 3.0)]
    ld, c, g4, info = ops.gp_solve_grad_batch(specs, [np.arange(3.0), np.ones((2, 2))], [np.ones(3), [2.0, 3.0]],
                                              [np.full(3, 0.5), np.full(2, 0.25)])
    s = lib.seen
    assert s["nb"] == 2 and s["nmax"] == 3 and list(s["ns"]) == [3, 2] and s["amps"] == [2.0, 3.0]
    assert np.array_equal(s["X"].reshape(2, 3, 2), [[[0, 0], [1, 0], [2, 0]], [[1, 1], [1, 1], [0, 0]]])
    assert np.array_equal(s["y"].reshape(2, 3), [[1, 1, 1], [2, 3, 0]]) and np.array_equal(s["yerr"].reshape(2, 3), [[.5, .5, .5], [.25, .25, 0]])
    assert np.array_equal(ld, [0, 1]) and np.array_equal(c, [10, 11]) and np.array_equal(g4, np.arange(8.0).reshape(2, 4))
    assert info.dtype == np.int64 and list(info) == [0, 7]
    ops.gp_solve_grad_batch(specs[:1], [np.ones((3, 2))], [np.ones(3)])
    assert lib.seen["yerr"] is None


def test_gp_solve_grad_batch_rejects_bad_shapes_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "get_ctx", no_device)
    monkeypatch.setattr(_lib, "load_library", no_device)
    with pytest.raises(ValueError):
        ops.gp_solve_grad_batch([ops.KernelSpec(0), ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(3)])
    with pytest.raises(ValueError):
        ops.gp_solve_grad_batch([ops.KernelSpec(0)], [np.ones((3, 2))], [np.ones(2)])
    with pytest.raises(ValueError):
        ops.gp_solve_grad_batch([ops.KernelSpec(0)], [np.ones((4097, 2))], [np.ones(4097)])

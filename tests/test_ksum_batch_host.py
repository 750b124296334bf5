"""CPU-only checks of the batched routes for sums of kernels (include/tgp.h, seam S2i): the C-ABI's prototypes, which objects
``_batch_spec`` lets into a batch, the routing of predict_many / predict_loo_many / log_likelihood_many / solve_many and of
``ops.gp_solve_batch`` itself with the device calls replaced by NumPy stand-ins, and the chain rule of the exact route."""
import ctypes
import sys

import numpy as np
import pytest

import _ksum_refs as S
import treegp_amd as tg
import treegp_amd.fit_many  # noqa: F401
from treegp_amd import _lib, gp_interp, kernels, ops

fit_many = sys.modules["treegp_amd.fit_many"]

TREE = "RBF(1.0) + WhiteKernel(0.01)"
FIVE = "RBF(1.0) + RBF(2.0) + RBF(3.0) + RBF(4.0) + RBF(5.0)"
SINGLE = "0.5**2 * RBF(0.2)"


# ---- 1. the C-ABI --------------------------------------------------------------------------------------------------------------
def test_the_c_abi_declares_every_batched_sum_entry_with_its_namesakes_prototype():
    pairs = {"tgp_gp_solve_batch_sum": "tgp_gp_solve_batch", "tgp_gp_posterior_batch_sum": "tgp_gp_posterior_batch",
             "tgp_gp_loo_batch_sum": "tgp_gp_loo_batch", "tgp_gp_solve_grad_batch_sum": "tgp_gp_solve_grad_batch_any"}
    for new, old in pairs.items():
        res, args = _lib.SIGNATURES[new]
        ores, oargs = _lib.SIGNATURES[old]
        assert res is ores and len(args) == len(oargs), new
        for i, (a, o) in enumerate(zip(args, oargs)):
            if i == 2:                                   # ks: an array of tgp_kernel_sum in place of one of tgp_kernel
                assert a._type_ is _lib.TgpKernelSum and o is ctypes.c_void_p, new
            else:
                assert a is o, (new, i)
    res, args = _lib.SIGNATURES["tgp_kbuild_batch_sum"]
    assert res is ctypes.c_int and len(args) == 8 and args[2]._type_ is _lib.TgpKernelSum and args[1] is ctypes.c_int
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "tgp.h")).read()
    for name in list(pairs) + ["tgp_kbuild_batch_sum"]:
        assert "int %s(tgp_ctx *ctx, int nb, const tgp_kernel_sum *ks, const int64_t *ns, int64_t nmax," % name in header, name


# ---- 2. which objects a batch takes --------------------------------------------------------------------------------------------
def make_gp(kern, n=40, optimizer="none", seed=7):
    X, y, e, _ = S.data(n, seed)
    gp = tg.GPInterpolation(kernel=kern, optimizer=optimizer, normalize=True)
    gp.initialize(np.array(X), np.array(y), y_err=np.array(e))
    return gp


def test_batch_spec_takes_sums_and_leaves_the_other_trees_out(monkeypatch):
    monkeypatch.setattr(ops, "_dist_engine", lambda n, ctx: None)
    spec = gp_interp._batch_spec(make_gp(S.SUM_A))
    assert isinstance(spec, ops.KernelSumSpec) and [t.kind for t in spec.terms] == [_lib.TGP_AVK, _lib.TGP_ARBF]
    assert len(gp_interp._batch_spec(make_gp(S.SUM_B)).terms) == 4
    assert isinstance(gp_interp._batch_spec(make_gp(SINGLE)), ops.KernelSpec)
    assert gp_interp._batch_spec(make_gp(TREE)) is None
    assert gp_interp._batch_spec(make_gp(FIVE)) is None
    # the exclusions stay: the multi-GPU route and the size
    dist = make_gp(S.SUM_A)
    dist.backend = "dist"
    assert gp_interp._batch_spec(dist) is None
    monkeypatch.setattr(ops, "_dist_engine", lambda n, ctx: object())
    assert gp_interp._batch_spec(make_gp(S.SUM_A)) is None


# ---- 3. routing, the device calls replaced by NumPy stand-ins ------------------------------------------------------------------
def matrix_of(spec, X, Y=None):
    return S.sum_matrix(spec, X, Y) if isinstance(spec, ops.KernelSumSpec) else S.spec_matrix(spec, X, Y)


def as_sum(spec):
    return spec if isinstance(spec, ops.KernelSumSpec) else ops.KernelSumSpec([spec])


@pytest.fixture
def fake(monkeypatch):
    """the batched ops calls on the host, each recording the specs it is handed; the single-problem solve of a device kernel
    is an error (the objects under test must be in the batch), the dense one records its size"""
    rec = {"solve_batch": [], "loo_batch": [], "posterior_batch": [], "grad_batch_sum": [], "dense": []}

    def solved(specs, Xs, ys, y_errs):
        return [S.host_solve(matrix_of(s, X), y, e) for s, X, y, e in zip(specs, Xs, ys, y_errs)]

    def gp_solve_batch(specs, Xs, ys, y_errs=None, want_alpha=True, ctx=None):
        rec["solve_batch"].append(list(specs))
        out = solved(specs, Xs, ys, y_errs)
        return ([o[0] for o in out] if want_alpha else None, np.array([o[1] for o in out]), np.array([o[2] for o in out]),
                np.zeros(len(out), dtype=np.int64))

    def gp_loo_batch(specs, Xs, ys, y_errs=None, ctx=None):
        rec["loo_batch"].append(list(specs))
        out = solved(specs, Xs, ys, y_errs)
        return ([o[0] for o in out], [np.diag(o[3]).copy() for o in out], np.array([o[1] for o in out]),
                np.array([o[2] for o in out]), np.zeros(len(out), dtype=np.int64))

    def gp_posterior_batch(specs, Xs, ys, y_errs, Xqs, what="var", want_alpha=True, ctx=None):
        rec["posterior_batch"].append(list(specs))
        out = solved(specs, Xs, ys, y_errs)
        uncs = []
        for s, X, Xq, o in zip(specs, Xs, Xqs, out):
            H = matrix_of(s, Xq, X)
            cov = matrix_of(s, Xq) - H.dot(o[3]).dot(H.T)
            uncs.append(cov if what == "cov" else np.diag(cov).copy())
        return [o[0] for o in out], uncs, np.zeros(len(out)), np.zeros(len(out)), np.zeros(len(out), dtype=np.int64)

    def gp_solve_grad_batch_sum(specs, Xs, ys, y_errs=None, ctx=None):
        rec["grad_batch_sum"].append(list(specs))
        out = solved(specs, Xs, ys, y_errs)
        rows = [S.host_grad_rows(as_sum(s), X, o[0], o[3]) for s, X, o in zip(specs, Xs, out)]
        return np.array([o[1] for o in out]), np.array([o[2] for o in out]), rows, np.zeros(len(out), dtype=np.int64)

    def gp_solve_dense(K, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["dense"].append(len(K))
        alpha, ld, c, _ = S.host_solve(K, y, np.zeros(len(y)) if y_err is None else y_err)
        return alpha, ld, c, None

    def no_single(*a, **k):
        raise AssertionError("an object the batch takes went through its own single-problem call")

    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(ops, "_dist_engine", lambda n, ctx: None)
    monkeypatch.setattr(ops, "gp_solve", no_single)
    monkeypatch.setattr(ops, "gp_solve_resident", no_single)
    monkeypatch.setattr(ops, "gp_solve_batch", gp_solve_batch)
    monkeypatch.setattr(ops, "gp_loo_batch", gp_loo_batch)
    monkeypatch.setattr(ops, "gp_posterior_batch", gp_posterior_batch)
    monkeypatch.setattr(ops, "gp_solve_grad_batch_sum", gp_solve_grad_batch_sum)
    monkeypatch.setattr(ops, "gp_solve_dense", gp_solve_dense)
    monkeypatch.setattr(ops, "gp_predict", lambda spec, X, alpha, Xs, ctx=None: matrix_of(spec, Xs, X).dot(alpha))
    monkeypatch.setattr(ops, "kernel_matrix", lambda spec, X, Y=None, ctx=None: matrix_of(spec, X, Y))
    return rec


def trio():
    """a sum, a single kernel and a tree with a WhiteKernel (the non-batchable object)"""
    return [make_gp(S.SUM_A, 40), make_gp(TREE, 25), make_gp(SINGLE, 30), make_gp(S.SUM_B, 35)]


def kinds_of(specs):
    return ["sum%d" % len(s.terms) if isinstance(s, ops.KernelSumSpec) else "single" for s in specs]


@pytest.mark.parametrize("what", [None, "var", "cov"])
def test_predict_many_sends_sums_into_the_batch_and_the_tree_to_its_own_predict(fake, monkeypatch, what):
    gps = trio()
    own = []
    monkeypatch.setattr(gps[1], "predict", lambda X, **kw: own.append(kw) or "tree")
    Xq = [S.data(40, 7)[3][:m] for m in (3, 4, 5, 7)]
    kw = {} if what is None else {"return_" + what: True}
    out = tg.predict_many(gps, Xq, **kw)
    called = fake["solve_batch"] if what is None else fake["posterior_batch"]
    assert len(called) == 1 and kinds_of(called[0]) == ["sum2", "single", "sum4"]
    assert not (fake["posterior_batch"] if what is None else fake["solve_batch"]) and not fake["dense"]
    assert out[1] == "tree" and len(own) == 1
    for i in (0, 2, 3):
        gp = gps[i]
        spec = gp_interp._batch_spec(gp)
        alpha, _, _, Kinv = S.host_solve(matrix_of(spec, gp._X), gp._residual(), gp._y_err)
        y = out[i] if what is None else out[i][0]
        np.testing.assert_allclose(y, matrix_of(spec, Xq[i], gp._X).dot(alpha) + gp._mean, rtol=1e-12)
        if what is not None:
            H = matrix_of(spec, Xq[i], gp._X)
            cov = matrix_of(spec, Xq[i]) - H.dot(Kinv).dot(H.T)
            np.testing.assert_allclose(out[i][1], cov if what == "cov" else np.diag(cov), rtol=0, atol=1e-12 * spec.amp)


def test_predict_loo_many_sends_sums_into_the_batch_and_the_tree_to_its_own_method(fake, monkeypatch):
    gps = trio()
    monkeypatch.setattr(gps[1], "predict_loo", lambda return_var=False: "tree")
    monkeypatch.setattr(gps[1], "return_loo_log_predictive", lambda theta=None: -7.0)
    out = tg.predict_loo_many(gps, return_var=True)
    assert len(fake["loo_batch"]) == 1 and kinds_of(fake["loo_batch"][0]) == ["sum2", "single", "sum4"]
    assert out[1] == "tree" and all(out[i][0].shape == out[i][1].shape == (len(gps[i]._X),) for i in (0, 2, 3))
    scores = tg.loo_log_predictive_many(trio()[:1] + [gps[1]] + trio()[2:])
    assert len(fake["loo_batch"]) == 2 and kinds_of(fake["loo_batch"][1]) == ["sum2", "single", "sum4"]
    assert scores[1] == -7.0 and np.all(np.isfinite(scores))


def test_log_likelihood_many_sends_sums_into_the_batched_solve(fake):
    X, y, e, _ = S.data(40, 7)
    like = tg.log_likelihood(np.array(X), np.array(y), np.array(e))
    ks = [tg.eval_kernel(k) for k in (S.SUM_A, TREE, SINGLE, S.SUM_B, FIVE)]
    got = like.log_likelihood_many(ks)
    assert len(fake["solve_batch"]) == 1 and kinds_of(fake["solve_batch"][0]) == ["sum2", "single", "sum4"]
    assert fake["dense"] == [40, 40]                                     # the tree and the five-term sum: their own evaluation
    for i, k in enumerate(ks):
        _, ld, c, _ = S.host_solve(k(np.array(X)) if i in (1, 4) else matrix_of(kernels.device_spec(k), X), y, e)
        np.testing.assert_allclose(got[i], -0.5 * c - 20 * np.log(2 * np.pi) - 0.5 * ld, rtol=1e-12)


def fit_trio():
    return [make_gp(S.SUM_A, 30, optimizer="log-likelihood"), make_gp(TREE, 25, optimizer="log-likelihood"),
            make_gp(S.SUM_A, 36, optimizer="log-likelihood", seed=9)]


def test_solve_many_fits_sums_in_the_batch_by_finite_differences_by_default(fake, monkeypatch):
    own = []
    monkeypatch.setattr(tg.GPInterpolation, "solve", lambda self: own.append(self))
    gps = fit_trio()
    start = [gp.kernel.theta.copy() for gp in gps]
    tg.solve_many(gps)
    assert own == [gps[1]]                                               # the tree: its own solve()
    assert not fake["grad_batch_sum"] and fake["solve_batch"]
    assert all(set(kinds_of(specs)) == {"sum2"} for specs in fake["solve_batch"])
    ntheta = len(start[0])
    assert ntheta == 8 and len(fake["solve_batch"][0]) == 2 * (ntheta + 1)   # ntheta + 1 points of both objects in one call
    assert len(fake["solve_batch"][-1]) == 2                             # the log L of both fitted kernels
    for i in (0, 2):
        assert isinstance(gps[i]._optimizer._logL, float) and not np.array_equal(gps[i].kernel.theta, start[i])
        l0 = fit_many._log_likelihoods([fit_many._Fit(0, fit_trio()[i], "fd")], [gp_interp._batch_spec(fit_trio()[i])])[0]
        assert gps[i]._optimizer._logL > l0


def test_solve_many_takes_the_exact_route_of_the_sums_on_request(fake, monkeypatch):
    own = []
    monkeypatch.setattr(tg.GPInterpolation, "solve", lambda self: own.append(self))
    gps, ref = fit_trio(), fit_trio()
    tg.solve_many(gps, gradient="analytic-vk")
    assert own == [gps[1]] and fake["grad_batch_sum"]
    assert all(set(kinds_of(specs)) == {"sum2"} for specs in fake["grad_batch_sum"])
    assert len(fake["solve_batch"]) == 1 and len(fake["solve_batch"][0]) == 2      # only the log L of the fitted kernels
    fake["solve_batch"].clear()
    tg.solve_many(ref)                                                   # finite differences end no higher (test_gpu_fit_many.py)
    for i in (0, 2):
        lref = ref[i]._optimizer._logL
        assert gps[i]._optimizer._logL >= lref - 1e-6 * abs(lref), (i, gps[i]._optimizer._logL, lref)
    with pytest.raises(NotImplementedError, match="GP 0"):
        tg.solve_many(fit_trio(), gradient="analytic")                   # (Gaussian single kernels only, as before)


# ---- 4. ops.gp_solve_batch picks its entry -------------------------------------------------------------------------------------
class FakeLib(object):
    """records which entry is called and what kernels it is given; fills the outputs"""

    def __init__(self):
        self.calls = []

    def _solve(self, name, ctype, ctx, nb, ks, ns, nmax, X, y, yerr, alpha, logdet, ydota, info):
        def arr(p, count, ct=ctypes.c_double):
            return np.ctypeslib.as_array((ct * count).from_address(p.value))
        k = ctypes.cast(ks, ctypes.POINTER(ctype))
        if ctype is _lib.TgpKernelSum:
            seen = [[(k[b].term[t].kind, k[b].term[t].amp) for t in range(k[b].nterms)] for b in range(nb)]
        else:
            seen = [[(k[b].kind, k[b].amp)] for b in range(nb)]
        self.calls.append((name, seen))
        arr(logdet, nb)[:] = np.arange(nb)
        arr(ydota, nb)[:] = 10 + np.arange(nb)
        arr(info, nb, ctypes.c_int32)[:] = 0
        return 0

    def tgp_gp_solve_batch(self, *a):
        return self._solve("tgp_gp_solve_batch", _lib.TgpKernel, *a)

    def tgp_gp_solve_batch_sum(self, *a):
        return self._solve("tgp_gp_solve_batch_sum", _lib.TgpKernelSum, *a)


def test_gp_solve_batch_calls_the_old_entry_without_sums_and_the_sum_entry_with_wrapped_kernels(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    a, b = ops.KernelSpec(_lib.TGP_RBF, amp=2.0), ops.KernelSpec(_lib.TGP_VK, amp=3.0)
    s = ops.KernelSumSpec([ops.KernelSpec(_lib.TGP_AVK, amp=0.25), ops.KernelSpec(_lib.TGP_ARBF, amp=0.5)])
    Xs, ys = [np.ones((3, 2)), np.ones((2, 2)), np.ones((4, 2))], [np.ones(3), np.ones(2), np.ones(4)]
    _, ld, c, info = ops.gp_solve_batch([a, b], Xs[:2], ys[:2], want_alpha=False)
    assert lib.calls == [("tgp_gp_solve_batch", [[(_lib.TGP_RBF, 2.0)], [(_lib.TGP_VK, 3.0)]])]
    assert np.array_equal(ld, [0, 1]) and np.array_equal(c, [10, 11]) and info.dtype == np.int64
    ops.gp_solve_batch([a, s, b], Xs, ys, want_alpha=False)
    assert lib.calls[1] == ("tgp_gp_solve_batch_sum", [[(_lib.TGP_RBF, 2.0)], [(_lib.TGP_AVK, 0.25), (_lib.TGP_ARBF, 0.5)],
                                                      [(_lib.TGP_VK, 3.0)]])
    ops.gp_solve_batch([ops.KernelSumSpec([a])], Xs[:1], ys[:1], want_alpha=False)       # a sum of one term is still a sum
    assert lib.calls[2] == ("tgp_gp_solve_batch_sum", [[(_lib.TGP_RBF, 2.0)]])


# ---- 5. the chain rule of the exact route --------------------------------------------------------------------------------------
def test_sum_jacobian_times_the_batched_rows_equals_central_differences_of_the_host_likelihood():
    """what solve_many(gradient="analytic-vk") hands L-BFGS-B for Sum A at n = 60: ``sum_spec_jacobian`` times the flattened
    (nterms, 4) rows (the dense host formulas stand in for ops.gp_solve_grad_batch_sum), against central differences of the
    host log L in theta.  Step 1e-5: rounding ~2 eps |log L| / h = 2e-16 * 1e2 / 1e-5 = 2e-9 absolute, truncation
    h^2 |f'''| / 6 below that; the bound is 1e-8 of the largest component, as in test_ksum_host.py."""
    n = 60
    X, y, e, _ = S.data(n, 7)
    k = tg.eval_kernel(S.SUM_A)

    def host_ll(theta):
        spec = kernels.kernel_to_sum_spec(k.clone_with_theta(theta))
        _, ld, c, _ = S.host_solve(S.sum_matrix(spec, X), y, e)
        return -0.5 * c - 0.5 * n * np.log(2 * np.pi) - 0.5 * ld
    fit = fit_many._Fit(0, make_gp(S.SUM_A, n, optimizer="log-likelihood"), "analytic-vk")
    theta0 = np.array(k.theta)
    spec, jac = fit.spec_at(theta0)
    assert isinstance(spec, ops.KernelSumSpec) and jac.shape == (len(theta0), 8)
    alpha, _, _, Kinv = S.host_solve(S.sum_matrix(spec, X), y, e)
    rows = S.host_grad_rows(spec, X, alpha, Kinv)
    assert rows.shape == (2, 4)
    grad = jac.dot(np.ravel(rows))
    h = 1e-5
    fd = np.zeros(len(theta0))
    for i in range(len(theta0)):
        up, dn = theta0.copy(), theta0.copy()
        up[i] += h
        dn[i] -= h
        fd[i] = (host_ll(up) - host_ll(dn)) / (2 * h)
    np.testing.assert_allclose(grad, fd, rtol=0, atol=1e-8 * np.abs(fd).max())
    assert fit_many._Fit(0, make_gp(S.SUM_A, n, optimizer="log-likelihood"), "fd").spec_at(theta0)[1] is None

"""GPU tests of the kernel sums (include/tgp.h, seams S1s / S2s).  The stored values (K build, kernel matrix) are compared bit for
bit with the fp64 sum, in term order, of what the single-kernel entries write for each term -- those values are held to mpmath
by test_gpu_kernel_values.py, so bit equality is the whole accuracy statement and needs no tolerance.  Solve, posterior,
likelihood gradient and the API are held to the project's usual tolerances (test_gpu_dense_multi.py, test_gpu_vk_loglik_grad.py).
On the CPU oracle cond(K + diag(y_err^2)) is 6.9e3 for the first three terms of Sum B at n = 513 and 4.9e4 for g10's sum2."""
import ctypes as C

import numpy as np
import pytest

import _ksum_refs as S
from _history_helpers import Ctx, raw, rejected_nan

pytestmark = pytest.mark.gpu


def mods():
    import treegp_amd as tg
    from treegp_amd import _lib, kernels, ops
    return tg, _lib, kernels, ops


def sumspec(kern):
    tg, _, kernels, _ = mods()
    return kernels.kernel_to_sum_spec(tg.eval_kernel(kern))


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(raw(a), raw(b))


def assert_same_bits(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero(raw(a) != raw(b))[0]
    assert len(bad) == 0, "%s: %d of %d values differ, first at %d: %r vs %r" % (what, len(bad), a.size, bad[0],
                                                                               a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]])


def in_term_order(arrays):
    out = np.array(arrays[0], dtype=np.float64)
    for a in arrays[1:]:
        out = out + a
    return out


# ---- 1. the packed K build ---------------------------------------------------------------------------------------------------
def kbuild_packed(ctxh, spec, X, e):
    """(packed panels with NaN where nothing is written, unpacked lower triangle) of the K build of a KernelSpec / KernelSumSpec"""
    _, _lib, _, ops = mods()
    lib = _lib.load_library()
    n = len(X)
    Np = int(lib.tgp_padded_n(n))
    elems = int(lib.tgp_panel_elems(Np))
    dX = ops.DeviceBuffer.from_array(ctxh, X)
    de = ops.DeviceBuffer.from_array(ctxh, e) if e is not None else None
    dA = ops.DeviceBuffer.from_array(ctxh, np.full(elems, np.nan))
    entry = lib.tgp_d_kbuild_lower_sum if isinstance(spec, ops.KernelSumSpec) else lib.tgp_d_kbuild_lower
    _lib.check(ctxh, entry(ctxh, C.byref(spec.to_c()), dX.ptr, n, de.ptr if de else None, dA.ptr), "kbuild")
    K = np.empty((n, n))
    _lib.check(ctxh, lib.tgp_d_unpack_lower(ctxh, dA.ptr, Np, n, K.ctypes.data_as(C.c_void_p)), "unpack")
    packed = dA.to_array((elems,))
    for b in (dX, de, dA):
        if b is not None:
            b.free()
    return packed, K


def packed_indices(n):
    """global (row, column) of every element of the packed layout of padded order Np (include/tgp.h, factor storage)"""
    Np = (n + 255) // 256 * 256
    rows, cols = [], []
    for p in range(Np // 256):
        i, j = np.meshgrid(np.arange(256 * p, Np), np.arange(256 * p, 256 * p + 256), indexing="ij")
        rows.append(i.reshape(-1))
        cols.append(j.reshape(-1))
    return np.concatenate(rows), np.concatenate(cols)


@pytest.mark.parametrize("with_yerr", [True, False])
@pytest.mark.parametrize("kern", [S.SUM_A, S.SUM_B], ids=["A", "B"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_kbuild_sum_is_the_sum_of_the_single_kernel_builds_bit_for_bit(n, kern, with_yerr):
    _, _lib, _, ops = mods()
    ctxh = _lib.get_ctx()
    X, _, e, _ = S.data(n)
    spec = sumspec(kern)
    packed, K = kbuild_packed(ctxh, spec, X, e if with_yerr else None)
    terms = [kbuild_packed(ctxh, t, X, None) for t in spec.terms]
    want = in_term_order([k for _, k in terms])
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    assert_same_bits(K[low], want[low], "strict lower triangle")
    assert not K[np.triu(np.ones((n, n), dtype=bool), 1)].any()
    # the diagonal: fl(sum of the amplitudes) + yerr^2 to 2 ulp (the device may fuse the square into the add)
    d = spec.amp + (e * e if with_yerr else 0.0) * np.ones(n)
    assert np.all(np.abs(np.diag(K) - d) <= 2 * np.spacing(d)), np.abs(np.diag(K) - d).max()
    if not with_yerr:
        assert_same_bits(np.diag(K), np.full(n, spec.amp), "diagonal without noise")
    # padded rows and columns, and what is never written, are the namesake's
    I, J = packed_indices(n)
    pad = (I >= n) | (J >= n)
    assert_same_bits(packed[pad], terms[0][0][pad], "padding")
    unwritten = np.isnan(terms[0][0])
    assert np.array_equal(np.isnan(packed), unwritten), "the sum build writes other elements than the single-kernel build"


# ---- 2. the dense kernel matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", [S.SUM_A, S.SUM_B], ids=["A", "B"])
def test_kernel_matrix_sum_is_the_host_sum_of_the_terms_bit_for_bit(kern):
    _, _, _, ops = mods()
    X, _, _, Xs = S.data(257)
    spec = sumspec(kern)
    K = ops.kernel_matrix(spec, X)
    assert_same_bits(K, in_term_order([ops.kernel_matrix(t, X) for t in spec.terms]), "self")
    assert_same_bits(np.diag(K), np.full(257, spec.amp), "self diagonal")
    for m in (1, 257):
        H = ops.kernel_matrix(spec, X, Xs[:m])
        assert H.shape == (257, m)
        assert_same_bits(H, in_term_order([ops.kernel_matrix(t, X, Xs[:m]) for t in spec.terms]), "cross m=%d" % m)
    # and it is the kernel, not only a consistent sum: the host's own evaluation (scipy's Bessel functions)
    np.testing.assert_allclose(K, S.sum_matrix(spec, X), rtol=0, atol=1e-12 * spec.amp)


# ---- 3. one term -------------------------------------------------------------------------------------------------------------
def every_entry(ctxh, spec, X, y, e, Xs, alpha_in):
    """[(name, value)] of every entry that takes a kernel (KernelSpec: the single-kernel entries, KernelSumSpec: the _sum ones)"""
    _, _, _, ops = mods()
    out = [("kernel_matrix.self", ops.kernel_matrix(spec, X, ctx=ctxh)),
           ("kernel_matrix.cross", ops.kernel_matrix(spec, X, Xs, ctx=ctxh)),
           ("kbuild", kbuild_packed(ctxh, spec, X, e)[1])]
    alpha, logdet, ydota, fac = ops.gp_solve(spec, X, y, e, keep=True, ctx=ctxh)
    try:
        out += [("alpha", alpha), ("logdet", logdet), ("ydota", ydota)]
        _, ld2, yd2, _ = ops.gp_solve(spec, X, y, e, want_alpha=False, ctx=ctxh)
        out += [("logdet.noalpha", ld2), ("ydota.noalpha", yd2)]
        out.append(("predict", ops.gp_predict(spec, X, alpha_in, Xs, ctx=ctxh)))
        out.append(("predict_grad", ops.gp_predict_grad(spec, X, alpha_in, Xs, ctx=ctxh)))
        out.append(("cov", ops.gp_predict_cov(spec, fac, X, Xs, ctx=ctxh)))
        out.append(("var", ops.gp_predict_var(spec, fac, X, Xs, ctx=ctxh)))
        if isinstance(spec, ops.KernelSumSpec):
            out.append(("loglik_grad", ops.gp_loglik_grad_sum(spec, fac, X, alpha, ctx=ctxh)))
        else:
            out.append(("loglik_grad", ops.gp_loglik_grad_any(spec, fac, X, alpha, ctx=ctxh).reshape(1, 4)))
    finally:
        fac.free()
    return out


@pytest.mark.parametrize("which", [1, 0], ids=["arbf", "avk"])
def test_one_term_is_the_single_kernel_entry_bit_for_bit(which):
    _, _lib, _, ops = mods()
    X, y, e, Xs = S.data(300)
    term = sumspec(S.SUM_A).terms[which]
    a_in = np.random.default_rng(3).standard_normal(300)
    with Ctx() as c:
        one = every_entry(c.h, ops.KernelSumSpec([term]), X, y, e, Xs, a_in)
    with Ctx() as c:
        ref = every_entry(c.h, term, X, y, e, Xs, a_in)
    assert [k for k, _ in one] == [k for k, _ in ref]
    for (k, a), (_, b) in zip(one, ref):
        assert_same_bits(a, b, k)


# ---- 4. the mean and its gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", [S.SUM_A, S.SUM_B], ids=["A", "B"])
@pytest.mark.parametrize("m", [1, 257])
def test_predict_sum_is_the_sum_of_the_terms_predictions_bit_for_bit(m, kern):
    _, _, _, ops = mods()
    X, y, e, Xs = S.data(513)
    Xs = Xs[:m]
    spec = sumspec(kern)
    alpha = np.random.default_rng(5).standard_normal(513)
    yp = ops.gp_predict(spec, X, alpha, Xs)
    gp = ops.gp_predict_grad(spec, X, alpha, Xs)
    assert yp.shape == (m,) and gp.shape == (m, 2)
    assert_same_bits(yp, in_term_order([ops.gp_predict(t, X, alpha, Xs) for t in spec.terms]), "predict")
    assert_same_bits(gp, in_term_order([ops.gp_predict_grad(t, X, alpha, Xs) for t in spec.terms]), "predict_grad")
    assert_same_bits(ops.gp_predict(spec, X, alpha, Xs), yp, "predict, second run")
    assert_same_bits(ops.gp_predict_grad(spec, X, alpha, Xs), gp, "predict_grad, second run")
    ref = S.sum_matrix(spec, Xs, X).dot(alpha)
    np.testing.assert_allclose(yp, ref, rtol=0, atol=1e-10 * max(np.abs(ref).max(), 1.0))


# ---- 5. the solve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 513])
def test_solve_sum_against_the_dense_route(n):
    _, _, _, ops = mods()
    X, y, e, _ = S.data(n)
    spec = sumspec(S.SUM_B)
    K = in_term_order([ops.kernel_matrix(t, X) for t in spec.terms])
    a0, ld0, yd0, _ = ops.gp_solve_dense(K, y, e)
    a1, ld1, yd1, _ = ops.gp_solve(spec, X, y, e)
    print("n=%d alpha err %.3e of max, logdet rel %.3e, ydota rel %.3e"
          % (n, np.abs(a1 - a0).max() / np.abs(a0).max(), abs(ld1 / ld0 - 1), abs(yd1 / yd0 - 1)))
    np.testing.assert_allclose(a1, a0, rtol=0, atol=1e-9 * np.abs(a0).max())
    np.testing.assert_allclose([ld1, yd1], [ld0, yd0], rtol=1e-11)
    _, ld2, yd2, _ = ops.gp_solve(spec, X, y, e, want_alpha=False)
    np.testing.assert_allclose([ld2, yd2], [ld0, yd0], rtol=1e-11)
    # and against the host's own evaluation and LAPACK
    ah, ldh, ydh, _ = S.host_solve(S.sum_matrix(spec, X), y, e)
    np.testing.assert_allclose(a1, ah, rtol=0, atol=1e-9 * np.abs(ah).max())
    np.testing.assert_allclose([ld1, yd1], [ldh, ydh], rtol=1e-11)


# ---- 6. the posterior --------------------------------------------------------------------------------------------------------
def test_posterior_of_a_sum_against_the_dense_entries_on_the_same_factor():
    _, _, _, ops = mods()
    X, y, e, Xs = S.data(513)
    spec = sumspec(S.SUM_B)
    _, _, _, fac = ops.gp_solve(spec, X, y, e, keep=True)
    try:
        HT = ops.kernel_matrix(spec, Xs, X)
        Kss = ops.kernel_matrix(spec, Xs)
        cov = ops.gp_predict_cov(spec, fac, X, Xs)
        var = ops.gp_predict_var(spec, fac, X, Xs)
        cov_d = ops.gp_predict_cov_dense(fac, HT, Kss)
        var_d = ops.gp_predict_var_dense(fac, HT, np.diag(Kss).copy())
    finally:
        fac.free()
    print("cov err %.3e, var err %.3e, var - diag(cov) %.3e (units of sum amp)"
          % (np.abs(cov - cov_d).max() / spec.amp, np.abs(var - var_d).max() / spec.amp, np.abs(var - np.diag(cov)).max() / spec.amp))
    np.testing.assert_allclose(cov, cov_d, rtol=0, atol=1e-9 * spec.amp)
    np.testing.assert_allclose(var, var_d, rtol=0, atol=1e-9 * spec.amp)
    np.testing.assert_allclose(var, np.diag(cov), rtol=0, atol=1e-13 * spec.amp)


# ---- 7. the likelihood gradient ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 513])
def test_loglik_grad_sum_rows_are_the_terms_and_match_the_dense_reference(n):
    _, _, _, ops = mods()
    X, y, e, _ = S.data(n)
    spec = sumspec(S.SUM_B)
    alpha, _, _, fac = ops.gp_solve(spec, X, y, e, keep=True)
    try:
        g = ops.gp_loglik_grad_sum(spec, fac, X, alpha)
        rows = [ops.gp_loglik_grad_any(t, fac, X, alpha) for t in spec.terms]
    finally:
        fac.free()
    assert g.shape == (4, 4)
    for t in range(4):
        assert_same_bits(g[t], rows[t], "row %d" % t)
    ah, _, _, Kinv = S.host_solve(S.sum_matrix(spec, X), y, e)
    ref = S.host_grad_rows(spec, X, ah, Kinv)
    print("n=%d worst |g - ref| / max(|ref|, 1) = %.3e" % (n, (np.abs(g - ref) / np.maximum(np.abs(ref), 1.0)).max()))
    np.testing.assert_allclose(g, ref, rtol=1e-8, atol=1e-8 * max(np.abs(ref).max(), 1.0))


# ---- 8. the API --------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_golden_sum2_on_the_device_route(golden, monkeypatch):
    """g10's sum2 = 0.7**2 * RBF(0.1) + 0.5**2 * AnisotropicRBF(scale_length=[0.4, 0.25]) against the values the reference
    produced, at test_gpu_dense_multi.py's tolerances, with the dense route closed"""
    tg, _, _, ops = mods()

    def closed(*a, **k):
        raise AssertionError("a sum of parametrised kernels took the dense route")
    monkeypatch.setattr(ops, "gp_solve_dense", closed)
    g = golden("g10_sklearn_kernels.npz")
    gp = tg.GPInterpolation(kernel=str(g["sum2_kernel"]), optimizer="none", normalize=True, white_noise=0.0)
    gp.initialize(g["X"], g["y"], y_err=g["y_err"])
    yp, cov = gp.predict(g["Xs"][:128], return_cov=True)
    ref = g["sum2_y_pred"]
    assert _rel(yp, ref[:128]) < 1e-10
    assert _rel(gp.predict(g["Xs"]), ref) < 1e-10
    np.testing.assert_allclose(gp._alpha, g["sum2_alpha"], rtol=0, atol=1e-9 * np.abs(g["sum2_alpha"]).max())
    np.testing.assert_allclose(cov, g["sum2_cov128"], rtol=0, atol=1e-9 * np.abs(g["sum2_cov128"]).max())
    np.testing.assert_allclose(gp.return_log_likelihood(), float(g["sum2_logL"]), rtol=1e-11)
    var = gp.predict(g["Xs"][:128], return_var=True)[1]
    np.testing.assert_allclose(var, np.diag(g["sum2_cov128"]), rtol=0, atol=1e-9 * np.abs(g["sum2_cov128"]).max())


def make_gp(kern, n, **kw):
    tg = mods()[0]
    X, y, e, _ = S.data(n)
    gp = tg.GPInterpolation(kernel=kern, optimizer=kw.pop("optimizer", "none"), normalize=True, **kw)
    gp.initialize(np.array(X), np.array(y), y_err=np.array(e))
    return gp


def test_predict_gradient_of_a_sum_equals_central_differences_of_predict():
    """Sum A at 40 points kept 1e-3 away from every star (the von Karman term has a cusp on each): central differences of
    predict with step 1e-5, to 1e-6 of the field's amplitude"""
    gp = make_gp(S.SUM_A, 300)
    rng = np.random.default_rng(11)
    pts = []
    while len(pts) < 40:
        p = rng.uniform(0.05, 0.95, 2)
        if np.sqrt(((gp._X - p) ** 2).sum(axis=1)).min() >= 1e-3:
            pts.append(p)
    Xq = np.array(pts)
    g = gp.predict_gradient(Xq)
    assert g.shape == (40, 2)
    h = 1e-5
    fd = np.empty((40, 2))
    for c in range(2):
        step = np.zeros(2)
        step[c] = h
        fd[:, c] = (gp.predict(Xq + step) - gp.predict(Xq - step)) / (2 * h)
    amplitude = np.abs(gp.predict(gp._X) - gp._mean).max()
    print("predict_gradient: worst error %.3e of the amplitude %.3e" % (np.abs(g - fd).max() / amplitude, amplitude))
    np.testing.assert_allclose(g, fd, rtol=0, atol=1e-6 * amplitude)


def test_loo_lgo_and_sampling_of_a_sum_equal_the_dense_route(monkeypatch):
    tg, _, kernels, _ = mods()
    n = 300
    labels = tg.kfold_labels(n, 5)
    Xq = S.data(n)[3][:50]

    def everything(gp):
        y_loo, v_loo = gp.predict_loo(return_var=True)
        y_lgo, v_lgo = gp.predict_lgo(labels, return_var=True)
        return [("loo", y_loo), ("loo var", v_loo), ("lgo", y_lgo), ("lgo var", v_lgo),
                ("sample_y", gp.sample_y(Xq, n_samples=3, random_state=4))]
    device = everything(make_gp(S.SUM_A, n))

    def closed(kernel, **kw):
        raise NotImplementedError("dense route forced")
    monkeypatch.setattr(kernels, "device_spec", closed)
    dense = everything(make_gp(S.SUM_A, n))
    for (k, a), (_, b) in zip(device, dense):
        print("%s: device vs dense %.3e of max" % (k, np.abs(a - b).max() / np.abs(b).max()))
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9 * np.abs(b).max(), err_msg=k)


def test_exact_gradient_fit_of_a_sum_reaches_the_finite_difference_fit(monkeypatch):
    """one maximum-likelihood fit of Sum A at n = 300 with TGP_ML_GRADIENT=analytic-vk against the default (finite-difference)
    fit from the same start: the same log L to 1e-6 relative"""
    tg = mods()[0]
    n = 300
    X = np.array(S.data(n)[0])
    e = np.array(S.data(n)[2])
    y = tg.gaussian_random_field(S.SUM_A, X, n_samples=1, random_state=2, y_err=e)[:, 0]
    logl = {}
    for mode in ("auto", "analytic-vk"):
        monkeypatch.setenv("TGP_ML_GRADIENT", mode)
        gp = tg.GPInterpolation(kernel=S.SUM_A, optimizer="log-likelihood", normalize=False)
        gp.initialize(X, y, y_err=e)
        gp.solve()
        logl[mode] = gp.return_log_likelihood()
    print("fit of Sum A: log L finite differences %.10f, exact gradient %.10f" % (logl["auto"], logl["analytic-vk"]))
    assert logl["analytic-vk"] == pytest.approx(logl["auto"], rel=1e-6)


# ---- 9. history, 10. rejections ----------------------------------------------------------------------------------------------
_FRESH = {}


def history_inputs():
    X, y, e, Xs = S.data(300)
    return X, y, e, Xs, np.random.default_rng(9).standard_normal(300)


def fresh_reference():
    """every _sum entry with Sum B at n = 300 as the first calls on a new context; computed once, shared, left unchanged"""
    if "ref" not in _FRESH:
        with Ctx() as c:
            _FRESH["ref"] = every_entry(c.h, sumspec(S.SUM_B), *history_inputs())
    return _FRESH["ref"]


def assert_fresh_bits(got, what):
    ref = fresh_reference()
    assert [k for k, _ in got] == [k for k, _ in ref]
    for (k, a), (_, b) in zip(got, ref):
        assert_same_bits(a, b, what + ": " + k)


def test_sum_entries_do_not_depend_on_what_the_context_did_before():
    _, _lib, _, ops = mods()
    spec = sumspec(S.SUM_B)
    Xl, yl, el, _ = S.data(700)
    big = ops.KernelSpec(_lib.TGP_ARBF, amp=1.3e4, a=60.0, b=8.0, c=45.0)
    with Ctx() as c:
        fac = ops.gp_solve(big, Xl + 7.0, yl * 1e8, el * 1e2, keep=True, ctx=c.h)[3]       # a larger, louder single-kernel solve
        ops.gp_predict_var(big, fac, Xl + 7.0, Xl[:300] + 7.0, ctx=c.h)
        ops.gp_loglik_grad_any(big, fac, Xl + 7.0, yl * 1e8, ctx=c.h)
        fac.free(keep_memory=True)
        rejected_nan(c, 700)                                                               # rejected: not positive definite
        assert_fresh_bits(every_entry(c.h, spec, *history_inputs()), "after a larger and a rejected solve")
        _lib.check(c.h, c.lib.tgp_release_caches(c.h), "tgp_release_caches")
        assert_fresh_bits(every_entry(c.h, spec, *history_inputs()), "after tgp_release_caches")


def raw_sum_calls(c, csum, fac, X, y, e, Xs, alpha):
    """return code and message of every _sum entry called with the ctypes sum `csum`"""
    _, _lib, _, ops = mods()
    lib = c.lib
    n, m = len(X), len(Xs)
    k = C.byref(csum)
    p = _lib.ptr
    dX = ops.DeviceBuffer.from_array(c.h, X)
    dA = ops.DeviceBuffer(c.h, int(lib.tgp_panel_elems(lib.tgp_padded_n(n))) * 8)
    out, ld, yd, h = np.empty(max(n * n, m * m, 16)), C.c_double(), C.c_double(), C.c_void_p()
    calls = {
        "tgp_kernel_matrix_sum": lambda: lib.tgp_kernel_matrix_sum(c.h, k, p(X), n, None, 0, p(out)),
        "tgp_d_kbuild_lower_sum": lambda: lib.tgp_d_kbuild_lower_sum(c.h, k, dX.ptr, n, None, dA.ptr),
        "tgp_gp_solve_sum": lambda: lib.tgp_gp_solve_sum(c.h, k, p(X), n, p(y), p(e), p(out), C.byref(ld), C.byref(yd), C.byref(h)),
        "tgp_gp_predict_sum": lambda: lib.tgp_gp_predict_sum(c.h, k, p(X), n, p(alpha), p(Xs), m, p(out)),
        "tgp_gp_predict_grad_sum": lambda: lib.tgp_gp_predict_grad_sum(c.h, k, p(X), n, p(alpha), p(Xs), m, p(out)),
        "tgp_gp_predict_cov_sum": lambda: lib.tgp_gp_predict_cov_sum(c.h, fac._h, k, p(X), n, p(Xs), m, p(out)),
        "tgp_gp_predict_var_sum": lambda: lib.tgp_gp_predict_var_sum(c.h, fac._h, k, p(X), n, p(Xs), m, p(out)),
        "tgp_gp_loglik_grad_sum": lambda: lib.tgp_gp_loglik_grad_sum(c.h, fac._h, k, p(X), n, p(alpha), p(out)),
    }
    res = {}
    for name, fn in calls.items():
        rc = fn()
        res[name] = (rc, (lib.tgp_last_error(c.h) or b"").decode())
    assert not h.value, "a rejected solve kept a factor"
    dX.free()
    dA.free()
    return res


def test_bad_sums_are_rejected_by_name_and_leave_the_context_as_new():
    _, _lib, _, ops = mods()
    X, y, e, Xs, alpha = [np.ascontiguousarray(a, dtype=np.float64) for a in history_inputs()]
    good = sumspec(S.SUM_B)
    with Ctx() as c:
        fac = c.track(ops.gp_solve(good, X, y, e, keep=True, ctx=c.h)[3])
        cases = []
        for nterms in (0, 5):
            bad = good.to_c()
            bad.nterms = nterms
            cases.append(("nterms=%d" % nterms, bad))
        bad = good.to_c()
        bad.term[2].kind = 99
        cases.append(("unknown kind in term 2", bad))
        for what, bad in cases:
            for name, (rc, msg) in raw_sum_calls(c, bad, fac, X, y, e, Xs, alpha).items():
                assert rc == -1, (what, name, rc, msg)
                assert name in msg, (what, name, msg)
        fac.free()
        c.facs.remove(fac)
        assert_fresh_bits(every_entry(c.h, good, X, y, e, Xs, alpha), "after the rejected calls")

"""GPU tests of the 3-D entries (include/tgp.h, "S1, S2, S3 in three dimensions"): kernel values pair by pair on every route that
evaluates a kernel against 40-digit references, the shapes where tiling can go wrong, the API against the reference project's
own results (tests/golden/g15_3d.npz) and against long-double restatements, independence from earlier calls.  References and
bounds: tests/_nd3_refs.py (nothing there calls the library); tests/test_nd3_host.py checks without a GPU that the inputs used
here reach every branch they claim."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import treegp_amd as tg
from treegp_amd import _lib, ops

import _nd3_refs as R
from _nd3_refs import LD, U53

pytestmark = pytest.mark.gpu

KINDS = {"arbf": _lib.TGP_ARBF, "rbf": _lib.TGP_RBF, "avk": _lib.TGP_AVK, "vk": _lib.TGP_VK}
STRINGS = {
    "arbf": "0.8**2 * AnisotropicRBF(invLam=array([[30., 4., -3.], [4., 20., 5.], [-3., 5., 12.]]))",
    "avk": "0.8**2 * AnisotropicVonKarman(invLam=array([[30., 4., -3.], [4., 20., 5.], [-3., 5., 12.]]))",
    "rbf": "0.8**2 * RBF([0.2, 0.3, 0.5])",
    "vk": "0.8**2 * VonKarman(length_scale=0.4)",
}
HALF_TINY = np.ldexp(LD(1.0), -1075)


def make_spec(kernel):
    kind, amp, M, ell = kernel
    if kind == "vk":
        return ops.KernelSpec3(KINDS[kind], amp=amp, ell=ell)
    return ops.KernelSpec3(KINDS[kind], amp=amp, m=(M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]))


def kbuild_raw(spec, X, yerr=None):
    """(the whole packed array, Np, the unpacked (n, n) lower triangle) of tgp_d_kbuild_lower3"""
    ctx, lib = _lib.get_ctx(), _lib.load_library()
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = len(X)
    Np = lib.tgp_padded_n(n)
    ne = lib.tgp_panel_elems(Np)
    dX = ops.DeviceBuffer.from_array(ctx, X)
    de = ops.DeviceBuffer.from_array(ctx, np.zeros(n) if yerr is None else np.ascontiguousarray(yerr, dtype=np.float64))
    dA = ops.DeviceBuffer.from_array(ctx, np.full(ne, np.nan))           # what the build does not write stays NaN
    _lib.check(ctx, lib.tgp_d_kbuild_lower3(ctx, C.byref(spec.to_c()), dX.ptr, n, de.ptr, dA.ptr), "tgp_d_kbuild_lower3")
    K = np.empty((n, n))
    _lib.check(ctx, lib.tgp_d_unpack_lower(ctx, dA.ptr, Np, n, K.ctypes.data_as(C.c_void_p)), "tgp_d_unpack_lower")
    A = dA.to_array((ne,))
    for buf in (dX, de, dA):
        buf.free()
    return A, Np, K


def within(dev, ref, bound, what):
    dev = np.asarray(dev, float)
    err = np.abs(LD(dev) - ref)
    ratio = np.where(np.isfinite(dev), err / bound, np.inf).astype(float)
    i = int(np.argmax(ratio))
    print("%s: max error / bound %.3f at %d (dev %r ref %r)" % (what, ratio.flat[i], i, dev.flat[i], float(ref.flat[i])))
    assert ratio.flat[i] <= 1.0, what


_REFS = {}


def value_case(tag):
    """(kernel, P, c, ref, aux, half_T) of the pair-by-pair inputs, computed once per kernel"""
    if tag not in _REFS:
        kernel = R.KERNELS[tag]
        P, c = R.value_queries(tag), R.VALUE_CENTER
        ref, aux = R.kernel_matrix_mp(kernel, P, c[None, :])
        M = kernel[2] if kernel[2] is not None else np.eye(3) / kernel[3] ** 2
        _REFS[tag] = (kernel, P, c, ref[:, 0], aux[:, 0], R.term_magnitude(M, P, c[None, :])[:, 0])
    return _REFS[tag]


def far_factor(spec):
    """a kept factor of one training point so far from everything that every cross value is exactly 0: predict_cov3 then
    returns the self block of its cross panels"""
    Xfar = np.array([[1.0e7, -2.0e7, 3.0e7]])
    return Xfar, ops.gp_solve(spec, Xfar, np.zeros(1), np.array([0.1]), keep=True)[3]


# ---------------------------------------------------------------------------------------------------------
# values, pair by pair
@pytest.mark.parametrize("tag", ["arbf", "rbf", "avk", "vk"])
def test_values_pair_by_pair_on_every_route(tag):
    kernel, P, c, ref, aux, half_T = value_case(tag)
    amp = kernel[1]
    spec = make_spec(kernel)
    gauss = tag in ("arbf", "rbf")
    p = 257                                                              # where the centre sits among the points of the self matrices
    X = np.insert(P[1:], p, c, axis=0)                                   # (row 0 of P is the centre itself)
    others = np.delete(np.arange(len(X)), p)
    routes = {}
    routes["kmat_cross"] = ops.kernel_matrix(spec, P, c[None, :])[:, 0]
    K = ops.kernel_matrix(spec, X)
    assert np.all(np.diag(K) == amp) and np.array_equal(K[others, p], K[p, others])
    routes["kmat_self"] = np.concatenate([[K[p, p]], K[others, p]])
    _, _, Kb = kbuild_raw(spec, X)
    assert np.all(np.diag(Kb) == amp) and np.all(Kb[np.triu_indices(len(X), 1)] == 0.0)
    routes["kbuild"] = np.concatenate([[Kb[p, p]], Kb[p, :p], Kb[p + 1:, p]])
    routes["predict"] = ops.gp_predict(spec, c[None, :], np.ones(1), P)
    onehot = np.zeros(len(X))
    onehot[p] = 1.0
    finite = np.isfinite(K[:, p])                                        # (every value is finite here)
    assert finite.all()
    routes["predict_onehot"] = ops.gp_predict(spec, X, onehot, P)
    if gauss:
        zero = ref < LD(amp) * HALF_TINY
        assert zero.sum() >= 3
        bounds = {r: R.gauss_bound_direct(ref, half_T, amp, kbuild=(r == "kbuild")) for r in routes}
        bounds["predict"] = R.gauss_bound_transformed(ref, aux, R.diameter_exponent(kernel[2], np.concatenate([P, c[None, :]])))
        bounds["predict_onehot"] = bounds["predict"]
    else:
        zero = aux > R.K56_XMAX * (1 + 1e-12)
        assert zero.sum() >= 5
        q_half = (aux / (2 * np.pi)) ** 2 / 2
        ratio = np.where(q_half > 0, half_T / np.where(q_half > 0, q_half, 1.0), 1.0)
        bounds = {r: R.vk_bound(ref, amp, aux, ratio) for r in routes}
    for r, dev in routes.items():
        assert dev[0] == amp, r                                          # the coincident point: exactly amp
        within(dev, ref, bounds[r], "%s %s" % (tag, r))
        if r != "kbuild" or not gauss:                                   # (the K build's clamped exponent leaves < amp 4.5e-308)
            assert np.all(dev[zero] == 0.0), r
    # cross panels through predict_cov3 / predict_var3: the self block, with a factor whose cross values are exactly 0
    Q = P[:40]
    refQ, auxQ = R.kernel_matrix_mp(kernel, Q)
    Mq = kernel[2] if kernel[2] is not None else np.eye(3) / kernel[3] ** 2
    hT = R.term_magnitude(Mq, Q, Q)
    Xfar, factor = far_factor(spec)
    cov = ops.gp_predict_cov(spec, factor, Xfar, Q)
    var = ops.gp_predict_var(spec, factor, Xfar, Q)
    factor.free()
    assert np.all(np.diag(cov) == amp) and np.all(var == amp) and np.array_equal(cov, cov.T)
    if gauss:
        bq = R.gauss_bound_direct(refQ, hT, amp)
    else:
        qh = (auxQ / (2 * np.pi)) ** 2 / 2
        bq = R.vk_bound(refQ, amp, auxQ, np.where(qh > 0, hT / np.where(qh > 0, qh, 1.0), 1.0))
    within(cov, refQ, bq, "%s cross panels" % tag)


@pytest.mark.parametrize("name", ["rank_one", "indefinite"])
def test_fallback_invlam_takes_the_direct_form(name):
    """invLam without a Cholesky factor: the fused predict evaluates the quadratic form directly, as every other route does"""
    M = {"rank_one": R.RANK_ONE, "indefinite": R.INDEFINITE}[name]
    kernel = ("arbf", 0.7, M, None)
    spec = make_spec(kernel)
    c = R.VALUE_CENTER
    P = R.direction_points(300, 21, 1e-3, 2.5, c)
    P[0] = c
    ref, _ = R.kernel_matrix_mp(kernel, P, c[None, :])
    bound = R.gauss_bound_direct(ref[:, 0], R.term_magnitude(M, P, c[None, :])[:, 0], 0.7)
    routes = {"kmat_cross": ops.kernel_matrix(spec, P, c[None, :])[:, 0], "predict": ops.gp_predict(spec, c[None, :], np.ones(1), P)}
    X = np.insert(P[1:], 130, c, axis=0)
    Kb = kbuild_raw(spec, X)[2]
    routes["kbuild"] = np.concatenate([[Kb[130, 130]], Kb[130, :130], Kb[131:, 130]])
    for r, dev in routes.items():
        assert dev[0] == 0.7
        within(dev, ref[:, 0], R.gauss_bound_direct(ref[:, 0], R.term_magnitude(M, P, c[None, :])[:, 0], 0.7, kbuild=(r == "kbuild")),
               "%s %s" % (name, r))
    assert np.array_equal(routes["kmat_cross"], routes["predict"])       # the same direct form, the same bits


@pytest.mark.parametrize("tag", ["arbf", "avk", "vk"])
def test_nan_coordinate_stays_nan(tag):
    kernel = R.KERNELS[tag]
    spec = make_spec(kernel)
    rng = np.random.default_rng(5)
    X, Xs = rng.uniform(size=(300, 3)), rng.uniform(size=(40, 3))
    alpha = rng.standard_normal(300)
    base = ops.gp_predict(spec, X, alpha, Xs)
    Xn = Xs.copy()
    Xn[17, 2] = np.nan
    got = ops.gp_predict(spec, X, alpha, Xn)
    keep = np.arange(40) != 17
    assert np.isnan(got[17]) and np.array_equal(got[keep], base[keep])
    K = ops.kernel_matrix(spec, Xn, X)
    assert np.all(np.isnan(K[17])) and np.all(np.isfinite(K[keep]))
    Xt = X.copy()
    Xt[5, 0] = np.nan                                                    # a NaN training point reaches every query
    assert np.all(np.isnan(ops.gp_predict(spec, Xt, alpha, Xs)))
    Kb = kbuild_raw(spec, Xt)[2]
    assert np.all(np.isnan(Kb[6:, 5])) and np.all(np.isnan(Kb[5, :5])) and Kb[5, 5] == kernel[1]
    nan_spec = make_spec((kernel[0], kernel[1], kernel[2] * np.nan if kernel[2] is not None else None, np.nan))
    assert np.all(np.isnan(ops.gp_predict(nan_spec, X, alpha, Xs)))


@pytest.mark.parametrize("tag", ["arbf", "avk"])
def test_translated_far_from_the_origin(tag):
    """coordinates on a 2^-20 grid shifted by exactly representable amounts: the differences are the same numbers, so the routes
    that difference first return the same bits and the transformed predict (origin subtracted before the transform) stays
    within its bound"""
    kernel = R.KERNELS[tag]
    spec = make_spec(kernel)
    rng = np.random.default_rng(8)
    X = rng.integers(0, 2 ** 20, (200, 3)) / 2.0 ** 20
    Xs = rng.integers(0, 2 ** 20, (60, 3)) / 2.0 ** 20
    alpha = rng.standard_normal(200)
    K0 = ops.kernel_matrix(spec, Xs, X)
    y0 = ops.gp_predict(spec, X, alpha, Xs)
    ref, aux = R.kernel_matrix_mp(kernel, Xs[:12], X) if tag == "arbf" else (None, None)
    for shift in ((1024.0, 1024.0, 1024.0), (2.0 ** 20, -2.0 ** 17, 2.0 ** 10)):
        sh = np.array(shift)
        assert np.array_equal((X + sh) - sh, X) and np.array_equal((Xs + sh) - sh, Xs)
        assert np.array_equal(ops.kernel_matrix(spec, Xs + sh, X + sh), K0)
        assert np.array_equal(kbuild_raw(spec, X + sh)[2], kbuild_raw(spec, X)[2])
        y = ops.gp_predict(spec, X + sh, alpha, Xs + sh)
        if tag == "avk":
            assert np.array_equal(y, y0)
        else:
            S = R.diameter_exponent(kernel[2], np.concatenate([X, Xs]))
            vb = R.gauss_bound_transformed(ref, aux, S)
            bound = (vb * np.abs(LD(alpha))[None, :]).sum(axis=1) + R.predict_sum_bound((np.abs(ref) * np.abs(LD(alpha))).sum(axis=1), 200)
            within(y[:12], ref @ LD(alpha), bound, "arbf predict shifted by %r" % (shift,))


# ---------------------------------------------------------------------------------------------------------
# shapes
NS = (1, 127, 128, 129, 300, 513)
MS = (1, 255, 256, 257, 600)


def _pool(seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(size=(NS[-1], 3)), rng.standard_normal(NS[-1]), rng.uniform(size=(MS[-1], 3)), 0.05 + 0.1 * rng.uniform(size=NS[-1])


@pytest.mark.parametrize("n", NS)
def test_packed_lower_triangle_with_its_padding(n):
    kernel = R.KERNELS["arbf"]
    spec = make_spec(kernel)
    X, _, _, yerr = _pool()
    X, yerr = X[:n], yerr[:n]
    A, Np, K = kbuild_raw(spec, X, yerr)
    lib = _lib.load_library()
    ref = R.gauss_matrix_ld(kernel, X, X)
    hT = R.term_magnitude(kernel[2], X, X)
    low = np.tril_indices(n, -1)
    if n > 1:
        within(K[low], ref[low], R.gauss_bound_direct(ref[low], hT[low], kernel[1], kbuild=True), "kbuild n=%d" % n)
    # exactly amp + yerr_i^2: one fused multiply-add, so the correctly rounded sum (half an ulp of the exact value, which the
    # long doubles hold to 2^-64)
    exact = LD(kernel[1]) + LD(yerr) * LD(yerr)
    assert np.all(np.abs(LD(np.diag(K)) - exact) <= LD(U53) * exact * (1 + LD(2.0 ** -9)))
    # the packed array itself: element (i, j), j <= i, of panel p = j // 256 sits at panel_off(p) + (i - 256 p) 256 + j % 256
    full = np.full((Np, Np), np.nan)
    for p in range(Np // 256):
        off = lib.tgp_panel_off(p, Np)
        rows = Np - 256 * p
        full[256 * p:, 256 * p:256 * p + 256] = A[off:off + rows * 256].reshape(rows, 256)
    ii, jj = np.tril_indices(Np)
    packed = full[ii, jj]
    want = np.where(ii == jj, 1.0, 0.0)                                  # padded rows: identity; padded columns: zero
    inside = (ii < n) & (jj < n)
    want[inside] = K[ii[inside], jj[inside]]
    assert np.array_equal(packed, want)
    for kind in ("avk", "vk"):                                           # the von Karman instantiations against the dense matrix (same evaluator)
        s2 = make_spec(R.KERNELS[kind])
        Kd = ops.kernel_matrix(s2, X)
        Kv = kbuild_raw(s2, X)[2]
        assert np.array_equal(Kv[low], Kd[low]) and np.all(np.diag(Kv) == R.KERNELS[kind][1])


@pytest.mark.parametrize("n", NS)
def test_predict_shapes_against_the_long_double_sum(n):
    """ys against sum_i k_i alpha_i in long doubles within c u sum |alpha_i k_i| (+ the values' own bound), c from the
    summation order (_nd3_refs.predict_sum_bound); the von Karman kinds against the device's own dense matrix (the same
    evaluator: only the summation differs)"""
    X, alpha, Xs, _ = _pool()
    X, alpha = X[:n], alpha[:n]
    kernel = R.KERNELS["arbf"]
    spec = make_spec(kernel)
    ref = R.gauss_matrix_ld(kernel, Xs, X)
    s = np.asarray(-np.log(ref / LD(kernel[1])), dtype=float)
    S = R.diameter_exponent(kernel[2], np.concatenate([X, Xs]))
    terms = np.abs(ref) * np.abs(LD(alpha))[None, :]
    bound = (R.gauss_bound_transformed(ref, s, S) * np.abs(LD(alpha))[None, :]).sum(axis=1) + R.predict_sum_bound(terms.sum(axis=1), n)
    want = ref @ LD(alpha)
    for m in MS:
        ys = ops.gp_predict(spec, X, alpha, Xs[:m])
        assert ys.shape == (m,)
        within(ys, want[:m], bound[:m], "arbf predict n=%d m=%d" % (n, m))
        assert np.array_equal(ys, ops.gp_predict(spec, X, alpha, Xs[:m]))             # the same bits on a second call
    for kind in ("avk", "vk"):
        s2 = make_spec(R.KERNELS[kind])
        Kd = LD(ops.kernel_matrix(s2, Xs, X))
        want2 = Kd @ LD(alpha)
        b2 = R.predict_sum_bound((np.abs(Kd) * np.abs(LD(alpha))[None, :]).sum(axis=1), n) + LD(1e-300)
        for m in MS:
            within(ops.gp_predict(s2, X, alpha, Xs[:m]), want2[:m], b2[:m], "%s predict n=%d m=%d" % (kind, n, m))
    # the dense matrix at these shapes: cross against the long-double values, self symmetric with an exact diagonal
    Kc = ops.kernel_matrix(spec, Xs[:257], X)
    within(Kc, ref[:257], R.gauss_bound_direct(ref[:257], R.term_magnitude(kernel[2], Xs[:257], X), kernel[1]), "kmat n=%d" % n)
    Ks = ops.kernel_matrix(spec, X)
    assert np.array_equal(Ks, Ks.T) and np.all(np.diag(Ks) == kernel[1])


# ---------------------------------------------------------------------------------------------------------
# the API against the reference project's own results
@pytest.mark.parametrize("tag", ["arbf", "avk", "rbf", "vk"])
def test_api_parity_with_the_reference(golden, tag):
    g = golden("g15_3d.npz")
    gp = tg.GPInterpolation(kernel=str(g[tag + "_kernel"]), optimizer="none", normalize=True)
    gp.initialize(g["X"], g["y"], y_err=g["y_err"])
    Xs = g["Xs"]
    y_pred, cov = gp.predict(Xs, return_cov=True)
    np.testing.assert_allclose(gp._alpha, g[tag + "_alpha"], rtol=0, atol=1e-9 * np.abs(g[tag + "_alpha"]).max())
    np.testing.assert_allclose(y_pred, g[tag + "_y_pred"], rtol=0, atol=1e-10 * np.abs(g[tag + "_y_pred"]).max())
    np.testing.assert_allclose(gp.predict(Xs), g[tag + "_y_pred"], rtol=0, atol=1e-10 * np.abs(g[tag + "_y_pred"]).max())
    np.testing.assert_allclose(cov[:64, :64], g[tag + "_cov64"], rtol=0, atol=1e-9 * np.abs(g[tag + "_cov64"]).max())
    for theta, logl in zip(g[tag + "_thetas"], g[tag + "_logL"]):
        np.testing.assert_allclose(gp.return_log_likelihood(theta=theta), logl, rtol=1e-11)
    # kernel tables through the classes' own __call__ (scikit-learn's RBF evaluates itself on the host: the device spec there)
    k = tg.eval_kernel(str(g[tag + "_kernel"]))
    if tag == "rbf":
        spec = tg.kernels.kernel_to_spec3(k)
        Kself, Kx = ops.kernel_matrix(spec, g["X"][:96]), ops.kernel_matrix(spec, Xs, g["X"][:96])
    else:
        Kself, Kx = k(g["X"][:96]), k(Xs, Y=g["X"][:96])
    np.testing.assert_allclose(Kself, g[tag + "_self"], rtol=2e-12, atol=1e-12)
    np.testing.assert_allclose(Kx, g[tag + "_cross"], rtol=2e-12, atol=1e-12)
    # return_var is the diagonal of return_cov; cov is symmetric.  Both come from the same panels and the same substitution and
    # differ in the order of one sum of n terms each: 2 (n + 2) u amp
    y2, var = gp.predict(Xs, return_var=True)
    tol = 2 * (len(g["X"]) + 2) * U53 * 0.64
    assert np.array_equal(y2, gp.predict(Xs)) and np.abs(var - np.diag(cov)).max() <= tol
    assert np.abs(cov - cov.T).max() <= tol


def test_ml_fit_reaches_the_reference_optimum(golden):
    """the 120-point fit of g15 (the reference's L-BFGS-B with SciPy's finite differences) at the tolerances of the 2-D g11 test"""
    g = golden("g15_3d.npz")
    gp = tg.GPInterpolation(kernel=str(g["fit_kernel0"]), optimizer="log-likelihood", normalize=True)
    gp.initialize(g["fit_X"], g["fit_y"], y_err=g["fit_y_err"])
    gp.solve()
    ref_l = float(g["fit_logL"])
    assert gp._optimizer._logL >= ref_l - 1e-6 * abs(ref_l), (gp._optimizer._logL, ref_l)
    np.testing.assert_allclose(gp.kernel.theta, g["fit_theta"], atol=2e-3)
    np.testing.assert_allclose(gp.return_log_likelihood(theta=g["fit_theta"]), ref_l, rtol=1e-10)


def test_2d_statistics_raise_and_2d_specs_keep_refusing_three_columns():
    rng = np.random.default_rng(0)
    X, y = rng.uniform(size=(30, 3)), rng.standard_normal(30)
    gp = tg.GPInterpolation(kernel=STRINGS["arbf"], optimizer="two-pcf")
    gp.initialize(X, y, y_err=0.1 * np.ones(30))
    with pytest.raises(ValueError, match="2-D statistic"):
        gp.solve()
    with pytest.raises(ValueError):
        ops.gp_solve(ops.KernelSpec(_lib.TGP_ARBF), X, y, None)
    with pytest.raises(ValueError):
        ops.gp_solve(make_spec(R.KERNELS["arbf"]), X[:, :2], y, None)


def test_argument_errors_name_the_field():
    ctx, lib = _lib.get_ctx(), _lib.load_library()
    X = np.zeros((4, 3))
    out = np.empty((4, 4))
    for field, value, match in (("ndim", 2, "ndim"), ("kind", 7, "kind")):
        c = make_spec(R.KERNELS["arbf"]).to_c()
        setattr(c, field, value)
        rc = lib.tgp_kernel_matrix3(ctx, C.byref(c), X.ctypes.data_as(C.c_void_p), 4, None, 0, out.ctypes.data_as(C.c_void_p))
        assert rc == -1
        msg = lib.tgp_last_error(ctx).decode()
        assert "tgp_kernel_matrix3" in msg and match in msg
        alpha = np.zeros(4)
        rc = lib.tgp_gp_solve3(ctx, C.byref(c), X.ctypes.data_as(C.c_void_p), 4, alpha.ctypes.data_as(C.c_void_p), None,
                               alpha.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc == -1 and "tgp_gp_solve3" in lib.tgp_last_error(ctx).decode()
    assert ops.kernel_matrix(make_spec(R.KERNELS["arbf"]), X).shape == (4, 4)       # the context is usable afterwards


# ---------------------------------------------------------------------------------------------------------
# predict_gradient
@pytest.mark.parametrize("tag", ["arbf", "rbf", "avk", "vk"])
def test_predict_gradient_against_the_analytic_derivative(tag):
    """(M, 3) against sum_i alpha_i grad k in 40 digits.  Bound per component c: sum_i |alpha_i| |grad_i|_c' rel_i with
    |grad_i|_c' = amp f_i sum_b |M_cb| |d_b| (the magnitudes of the products that make (M d)_c) and rel_i the value's relative
    bound of _nd3_refs (Gaussian: (8 + 20 T/2) u; von Karman: 2e-13 + (x + 2)(10 T/q + 3) u, w having the profile's accuracy
    and slope) plus (n + 8) u for the sum and the three products and two additions of (M d)_c."""
    import mpmath as mp
    kernel = R.KERNELS[tag]
    kind, amp, M, ell = kernel
    Mm = M if M is not None else np.eye(3) / ell ** 2
    rng = np.random.default_rng(12)
    n, m = 40, 24
    X = rng.uniform(size=(n, 3)) * (0.6 if kind in ("rbf", "arbf") else 2.5)
    Xs = rng.uniform(size=(m, 3)) * (0.6 if kind in ("rbf", "arbf") else 2.5)
    Xs[:3] = X[:3]                                                       # queries on training points
    alpha = rng.standard_normal(n)
    gp = tg.GPInterpolation(kernel=STRINGS[tag], optimizer="none", normalize=False)
    gp.initialize(X, np.zeros(n), y_err=0.1 * np.ones(n))
    gp._alpha = alpha                                                    # the cached solution predict_gradient uses
    got = gp.predict_gradient(Xs)
    assert got.shape == (m, 3)
    assert np.array_equal(got, ops.gp_predict_grad(make_spec(kernel), X, alpha, Xs))
    want = np.zeros((m, 3), LD)
    bound = np.zeros((m, 3), LD)
    hT = R.term_magnitude(Mm, Xs, X)
    for q in range(m):
        for i in range(n):
            gvec = R.grad_pair_mp(kernel, Xs[q], X[i])
            d = Xs[q] - X[i]
            qf = float(d @ Mm @ d)
            if qf == 0.0:
                assert gvec == [0, 0, 0]
                continue
            if kind in ("rbf", "arbf"):
                rel = (8 + 20 * hT[q, i]) * U53
                f = float(mp.exp(-mp.mpf(qf) / 2))
            else:
                x = 2 * np.pi * np.sqrt(qf)
                rel = 2e-13 + (x + 2) * (10 * hT[q, i] / (qf / 2) + 3) * U53
                f = float(R.vk_slope_mp(mp.sqrt(mp.mpf(qf))))
            rel += (n + 8) * U53
            for cidx in range(3):
                want[q, cidx] += R._mpf_to_ld(gvec[cidx]) * LD(alpha[i])
                bound[q, cidx] += LD(abs(alpha[i]) * amp * f * float(np.abs(Mm[cidx]) @ np.abs(d)) * rel)
    within(got, want, bound + LD(1e-300), "%s predict_gradient" % tag)
    # zero slope of a field on its only star
    one = ops.gp_predict_grad(make_spec(kernel), X[:1], np.ones(1), X[:1])
    assert np.array_equal(one, np.zeros((1, 3)))


# ---------------------------------------------------------------------------------------------------------
# consistency on a 150-point object against long-double restatements
@pytest.fixture(scope="module")
def obj150():
    rng = np.random.default_rng(31)
    n = 150
    X = rng.uniform(size=(n, 3))
    y = np.sin(3 * X[:, 0]) + np.cos(2 * X[:, 1]) * (0.5 + X[:, 2]) + 0.05 * rng.standard_normal(n) + 2.0
    yerr = 0.05 + 0.02 * rng.uniform(size=n)
    Xs = rng.uniform(size=(40, 3))
    kernel = R.KERNELS["arbf"]
    return dict(X=X, y=y, yerr=yerr, Xs=Xs, kernel=kernel, ref=R.DenseGP(kernel, X, yerr))


def _gp150(o):
    gp = tg.GPInterpolation(kernel=STRINGS["arbf"], optimizer="none", normalize=True)
    gp.initialize(o["X"], o["y"], y_err=o["yerr"])
    return gp


def test_predict_fields_loo_lgo_against_long_double(obj150):
    o = obj150
    ref, amp = o["ref"], o["kernel"][1]
    gp = _gp150(o)
    mean = np.mean(o["y"])
    r = LD(o["y"]) - LD(mean)
    alpha = ref.solve(r)
    # predict_fields: two fields, each with its own mean
    Y = np.stack([o["y"], 0.5 * o["y"] ** 2 - 1.0])
    got = gp.predict_fields(Y, o["Xs"])
    for f in range(2):
        mf = np.mean(Y[f])
        want = ref.predict(ref.solve(LD(Y[f]) - LD(mf)), o["Xs"]) + LD(mf)
        assert np.abs(LD(got[f]) - want).max() <= 1e-10 * np.abs(Y[f]).max()
    # predict_loo: mu_i = r_i - alpha_i / d_i, var_i = 1 / d_i - sigma_i^2 (Rasmussen & Williams 5.4.2)
    Kinv = ref.inverse()
    d = np.diag(Kinv)
    y_loo, v_loo = gp.predict_loo(return_var=True)
    np.testing.assert_allclose(y_loo, np.asarray(r - alpha / d + LD(mean), float), rtol=0, atol=1e-9 * amp)
    np.testing.assert_allclose(v_loo, np.asarray(1 / d - LD(o["yerr"]) ** 2, float), rtol=0, atol=1e-9 * amp)
    # predict_lgo: groups of contiguous runs; mu_G = r_G - P_GG^-1 alpha_G, C_G = P_GG^-1 - diag(sigma_G^2)
    labels = np.repeat(np.arange(6), 25)
    y_lgo, v_lgo = gp.predict_lgo(labels, return_var=True)
    for gidx in range(6):
        G = np.arange(25 * gidx, 25 * gidx + 25)
        Pl = R.cholesky_ld(Kinv[np.ix_(G, G)])
        sol = R.solve_upper_ld(Pl.T, R.solve_lower_ld(Pl, alpha[G]))
        PinvL = R.solve_upper_ld(Pl.T, R.solve_lower_ld(Pl, np.eye(25, dtype=LD)))
        np.testing.assert_allclose(y_lgo[G], np.asarray(r[G] - sol + LD(mean), float), rtol=0, atol=1e-9 * amp)
        np.testing.assert_allclose(v_lgo[G], np.asarray(np.diag(PinvL) - LD(o["yerr"][G]) ** 2, float), rtol=0, atol=1e-9 * amp)


def test_sample_y_and_random_field_against_long_double(obj150):
    o = obj150
    gp = _gp150(o)
    Xs = o["Xs"]
    out = gp.sample_y(Xs, n_samples=4, random_state=5)
    assert out.shape == (40, 4)
    y_star, cov = gp.predict(Xs, return_cov=True)
    z = np.random.default_rng(5).standard_normal((4, 40))
    Ls = R.cholesky_ld(LD(cov) + LD(1e-10 * 0.64) * np.eye(40, dtype=LD))       # the same normals, the device's covariance
    dev = np.asarray(Ls @ LD(z.T), float)
    assert np.abs((out - y_star[:, None]) - dev).max() <= 1e-10 * np.abs(dev).max()
    # the posterior covariance itself against the long-double restatement, at the API tolerance
    want = o["ref"].cov(Xs)
    assert np.abs(LD(cov) - want).max() <= 1e-9 * float(np.abs(want).max())
    # a prior field on 3-D points: L z with L the factor of K + jitter
    F = tg.gaussian_random_field(STRINGS["arbf"], o["X"], n_samples=3, random_state=7, y_err=o["yerr"])
    Kp = o["ref"].K + LD(1e-10 * 0.64) * np.eye(150, dtype=LD)
    zz = np.random.default_rng(7).standard_normal((3, 150))
    wantF = np.asarray(R.cholesky_ld(Kp) @ LD(zz.T), float)
    assert F.shape == (150, 3) and np.abs(F - wantF).max() <= 1e-9 * np.abs(wantF).max()


def test_constant_third_coordinate_reproduces_the_2d_object():
    """invLam block diagonal and z constant: the 3-D object is the 2-D one (different arithmetic, the API tolerances)"""
    rng = np.random.default_rng(41)
    n, m = 200, 50
    X2, Xs2 = rng.uniform(size=(n, 2)), rng.uniform(size=(m, 2))
    y = np.sin(4 * X2[:, 0]) * X2[:, 1] + 0.02 * rng.standard_normal(n)
    yerr = 0.02 * np.ones(n)
    for cls in ("AnisotropicRBF", "AnisotropicVonKarman"):
        k2 = "0.6**2 * %s(invLam=array([[40., 6.], [6., 25.]]))" % cls
        k3 = "0.6**2 * %s(invLam=array([[40., 6., 0.], [6., 25., 0.], [0., 0., 9.]]))" % cls
        g2 = tg.GPInterpolation(kernel=k2, optimizer="none", normalize=True)
        g2.initialize(X2, y, y_err=yerr)
        g3 = tg.GPInterpolation(kernel=k3, optimizer="none", normalize=True)
        g3.initialize(np.column_stack([X2, 0.75 * np.ones(n)]), y, y_err=yerr)
        p2, c2 = g2.predict(Xs2, return_cov=True)
        p3, c3 = g3.predict(np.column_stack([Xs2, 0.75 * np.ones(m)]), return_cov=True)
        np.testing.assert_allclose(p3, p2, rtol=0, atol=1e-10 * np.abs(p2).max())
        np.testing.assert_allclose(c3, c2, rtol=0, atol=1e-9 * np.abs(c2).max())
        np.testing.assert_allclose(g3._alpha, g2._alpha, rtol=0, atol=1e-9 * np.abs(g2._alpha).max())
        grad = g3.predict_gradient(np.column_stack([Xs2, 0.75 * np.ones(m)]))
        np.testing.assert_allclose(grad[:, :2], g2.predict_gradient(Xs2), rtol=0, atol=1e-9 * np.abs(grad).max())
        assert np.all(grad[:, 2] == 0.0)                                 # no slope along the constant coordinate


# ---------------------------------------------------------------------------------------------------------
# independence from earlier calls
def test_3d_call_after_history_has_the_bits_of_a_fresh_context():
    rng = np.random.default_rng(51)
    X, y, Xs = rng.uniform(size=(300, 3)), rng.standard_normal(300), rng.uniform(size=(257, 3))
    yerr = 0.1 * np.ones(300)

    def run(ctx):
        out = []
        for tag in ("arbf", "avk"):
            spec = make_spec(R.KERNELS[tag])
            alpha, logdet, chi2, factor = ops.gp_solve(spec, X, y, yerr, keep=True, ctx=ctx)
            out += [alpha, np.array([logdet, chi2]), ops.gp_predict(spec, X, alpha, Xs, ctx=ctx),
                    ops.gp_predict_var(spec, factor, X, Xs, ctx=ctx), ops.gp_predict_grad(spec, X, alpha, Xs, ctx=ctx)]
            factor.free()
        return out

    fresh = _lib.OwnedCtx(0)
    want = run(fresh.handle)
    used = _lib.OwnedCtx(0)
    h = used.handle
    X2 = rng.uniform(size=(3000, 2))
    s2 = ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=400.0, b=80.0, c=500.0)
    a2 = ops.gp_solve(s2, X2, rng.standard_normal(3000), 0.1 * np.ones(3000), ctx=h)[0]     # a large 2-D call
    ops.gp_predict(s2, X2, a2, rng.uniform(size=(5000, 2)), ctx=h)
    with pytest.raises(np.linalg.LinAlgError):                           # a rejected solve: coincident points without noise
        ops.gp_solve(make_spec(R.KERNELS["arbf"]), np.zeros((300, 3)), y, None, ctx=h)
    _lib.check(h, _lib.load_library().tgp_release_caches(h), "tgp_release_caches")
    got = run(h)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)

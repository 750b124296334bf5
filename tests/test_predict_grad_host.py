"""CPU-only checks of the gradient of the predicted mean (seam S3g): the device function w(u) compiled for the host against
mpmath, the references of tests/_predict_grad_refs.py against mpmath's numerical derivative of the covariance formulas, the host
logic of GPInterpolation.predict_gradient with the device calls replaced by NumPy stand-ins, and the library's surface."""
import ctypes
import os
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import treegp_amd as tg
from treegp_amd import _lib, ops

import _predict_grad_refs as R
from _kernel_value_helpers import K56_XMAX, LD, _mpf_to_ld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------
# w(u)
def test_device_slope_function_on_host(tmp_path):
    """bessel_k16.h compiled with g++ against mpmath at 30 digits: relative error <= 2e-13 wherever the function is not
    exactly 0 (no absolute term: w is a normal number right up to the cutoff), exactly 0 beyond the cutoff, every branch
    populated."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s"\nextern "C" void w(const double* u, double* o, long n)'
                   '{ for (long i = 0; i < n; ++i) o[i] = vonkarman_slope(u[i]); }\n'
                   % os.path.join(ROOT, "treegp_amd", "csrc", "bessel_k16.h"))
    so = str(tmp_path / "libw.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, str(src)])
    lib = ctypes.CDLL(so)
    rng = np.random.default_rng(0)
    u = np.concatenate([10 ** rng.uniform(-9, 2.05, 20000), [2.0 ** k / (2 * np.pi) for k in range(6)],
                        [111.0, 111.08, 1e-300]])
    out = np.empty_like(u)
    lib.w(u.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(len(u)))
    x = (2 * np.pi) * u                                  # the function's own fp64 argument
    inside = x <= K56_XMAX
    edges = [0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, K56_XMAX]
    counts = [int(((x > lo) & (x <= hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]
    assert min(counts) >= 200, counts
    assert (~inside).sum() >= 2 and np.all(out[~inside] == 0.0)
    assert inside[-3] and not inside[-2]                 # 111.0 and 111.08 sit either side of the cutoff
    old = mp.mp.dps
    mp.mp.dps = 30
    try:
        ref = np.array([_mpf_to_ld(R.w_mp(mp.mpf(float(v)))) for v in u[inside]])
    finally:
        mp.mp.dps = old
    dev = out[inside]
    assert np.all(np.isfinite(dev)) and np.all(dev > 0)
    rel = np.abs(LD(dev) - ref) / ref
    i = int(np.argmax(rel))
    print("w(u): max relative error %.3e at u = %r" % (float(rel[i]), float(u[inside][i])))
    assert float(rel[i]) <= 2e-13
    nan = np.array([np.nan])
    lib.w(nan.ctypes.data_as(ctypes.c_void_p), nan.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(1))
    assert np.isnan(nan[0])


# ---------------------------------------------------------------------------------------------------------
# the references
PAIR_CASES = [
    ("rbf", dict(amp=1.3, a=4.0, b=0.0, c=4.0, ell=1.0), False),
    ("arbf", dict(amp=0.7, a=400.0, b=80.0, c=500.0, ell=1.0), False),
    ("arbf", dict(amp=1.1, a=0.25, b=0.0, c=0.0, ell=1.0), True),            # 1-D
    ("vk", dict(amp=0.49, a=1.0, b=0.0, c=1.0, ell=0.3), False),
    ("vk", dict(amp=2.0, a=1.0, b=0.0, c=1.0, ell=1.7), True),               # 1-D
    ("avk", dict(amp=0.9, a=400.0, b=80.0, c=500.0, ell=1.0), False),
]


def _pairs(kind, p, one_d, count=50, seed=3):
    """displacements whose u (von Karman) runs through the series and the six segments, q / 2 (Gaussian) up to ~300"""
    rng = np.random.default_rng(seed)
    if kind in ("vk", "avk"):
        target = np.concatenate([10 ** rng.uniform(-6, np.log10(1 / (2 * np.pi)), count - 42),
                                 np.repeat([1.5, 3.0, 6.0, 12.0, 24.0, 100.0, 600.0], 6) * rng.uniform(0.9, 1.1, 42) / (2 * np.pi)])
    else:
        target = np.sqrt(2 * 10 ** rng.uniform(-8, 2.5, count))
    th = np.zeros(count) if one_d else rng.uniform(0, 2 * np.pi, count)
    e = np.stack([np.cos(th), np.sin(th)], axis=1)
    a, b, c = (p["ell"] ** -2, 0.0, p["ell"] ** -2) if kind == "vk" else (p["a"], p["b"], p["c"])
    scale = np.sqrt(a * e[:, 0] ** 2 + 2 * b * e[:, 0] * e[:, 1] + c * e[:, 1] ** 2)
    return e * (target / scale)[:, None]


def test_reference_formulas_against_mpmath_diff():
    """Independent of the derivation: mpmath's numerical derivative of the reference's covariance formulas at 40 digits agrees
    with the closed form of pair_grad_mp to 1e-20, for all four kinds, every branch of w, a sheared invLam and 1-D; and the
    long-double terms the GPU test sums agree with the closed form to (8 + x) 2^-60 (x or q / 2: the conditioning of the
    exponential; the sum of ~25 long-double terms of the integral for K_{1/6} carries a few units of 2^-64 each): 1/128 of
    an fp64 rounding, far inside every E of the device bound."""
    old = mp.mp.dps
    mp.mp.dps = 40
    try:
        total = 0
        for kind, p, one_d in PAIR_CASES:
            D = _pairs(kind, p, one_d)
            X = np.array([[0.4, -0.2]]) if not one_d else np.array([[0.4, 0.0]])
            Xs = X + D
            D = Xs - X                                         # what the long-double route sees (exact here or not: D is the input)
            alpha = np.array([1.7])
            terms = R.grad_terms(kind, p, X, alpha, Xs)
            for j, (dx, dy) in enumerate(D.tolist()):
                dxm, dym = mp.mpf(float(Xs[j, 0])) - mp.mpf(float(X[0, 0])), mp.mpf(float(Xs[j, 1])) - mp.mpf(float(X[0, 1]))
                gx, gy = R.pair_grad_mp(kind, p, dxm, dym)
                nx = mp.diff(lambda t: R.cov_mp(kind, p, t, dym), dxm)
                ny = mp.diff(lambda t: R.cov_mp(kind, p, dxm, t), dym)
                for g, d in ((gx, nx), (gy, ny)):
                    assert abs(g - d) <= mp.mpf("1e-20") * abs(d), (kind, p, dx, dy, g, d)
                if one_d:
                    assert gy == 0 and ny == 0
                # the long-double term (alpha = 1.7) against the closed form
                cond = float(terms["x"][0, j]) if "x" in terms else float(terms["q"][0, j]) / 2
                scal = abs(1.7 * p["amp"] * float(terms["k"][0, j]))
                for c, g in enumerate((gx, gy)):
                    err = abs(terms["T"][0, j, c] - _mpf_to_ld(mp.mpf(1.7) * g))
                    tol = (8 + cond) * 2.0 ** -60 * scal * float(terms["A"][0, j, c])
                    assert float(err) <= tol, (kind, p, dx, dy, c, float(err), tol)
                total += 1
        assert total >= 300
    finally:
        mp.mp.dps = old


def test_long_double_w_against_mpmath():
    """the vectorised long-double w of the GPU test's oracle against mpmath over all its branches, to (8 + x) 2^-60"""
    rng = np.random.default_rng(8)
    u = np.concatenate([10 ** rng.uniform(-9, 2.05, 400), [1 / (2 * np.pi), 1.0000001 / (2 * np.pi), 111.0, 111.08, 1e-300]])
    got = R.w_ld(LD(u))
    old = mp.mp.dps
    mp.mp.dps = 40
    try:
        for v, g in zip(u.tolist(), got):
            x = 2 * np.pi * v
            if x > K56_XMAX:
                assert g == 0
                continue
            ref = _mpf_to_ld(R.w_mp(mp.mpf(v)))
            assert float(abs(g - ref) / ref) <= (8 + x) * 2.0 ** -60, (v, float(g), float(ref))
    finally:
        mp.mp.dps = old


# ---------------------------------------------------------------------------------------------------------
# predict_gradient, host logic
def _gauss(spec, A, B):
    A, B = _lib.as_xy(A), _lib.as_xy(B)
    d = A[:, None, :] - B[None, :, :]
    a, b, c = (spec.ell ** -2, 0.0, spec.ell ** -2) if spec.kind == _lib.TGP_VK else (spec.a, spec.b, spec.c)   # (a Gaussian stands in)
    q = a * d[..., 0] ** 2 + 2 * b * d[..., 0] * d[..., 1] + c * d[..., 1] ** 2
    M = np.array([[a, b], [b, c]])
    return spec.amp * np.exp(-0.5 * q), d @ M


@pytest.fixture
def fake(monkeypatch):
    """ops.gp_solve / gp_predict_grad / knn_mean on the host; every call is recorded"""
    rec = {"solve": [], "grad": []}

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["solve"].append(keep)
        K = _gauss(spec, X, X)[0] + np.diag(np.asarray(y_err, float) ** 2)
        return np.linalg.solve(K, y), 0.0, 0.0, None

    def gp_predict_grad(spec, X, alpha, Xs, ctx=None):
        rec["grad"].append((spec, X, alpha, Xs))
        K, Md = _gauss(spec, Xs, X)
        return -np.einsum("ji,jic->jc", K * np.asarray(alpha)[None, :], Md)

    def knn_mean(X0, y0, X, k):
        d = ((np.asarray(X)[:, None, :] - np.asarray(X0)[None, :, :]) ** 2).sum(axis=2)
        return np.asarray(y0)[np.argsort(d, axis=1)[:, :k]].mean(axis=1)

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "get_ctx", no_device)
    monkeypatch.setattr(ops, "gp_predict", no_device)
    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_predict_grad", gp_predict_grad)
    monkeypatch.setattr(ops, "knn_mean", knn_mean)
    return rec


def _data(ndim, n=40, m=17, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, ndim))
    y = np.sin(5 * X[:, 0]) + 0.05 * rng.standard_normal(n) + 3.0
    return X, y, 0.05 * np.ones(n), rng.uniform(0, 1, (m, ndim))


def test_predict_gradient_shapes_and_cache(fake):
    X, y, e, Xs = _data(2)
    gp = tg.GPInterpolation(kernel="1.0**2 * AnisotropicRBF(invLam=array([[40., 8.], [8., 50.]]))", optimizer="none")
    gp.initialize(X, y, y_err=e)
    g = gp.predict_gradient(Xs)
    assert g.shape == (17, 2) and fake["solve"] == [False]              # solved once, no factor kept
    spec, X1, alpha, X2 = fake["grad"][0]
    assert X1 is gp._X and alpha is gp._alpha and X2 is Xs and spec.kind == _lib.TGP_ARBF
    assert np.array_equal(gp.predict_gradient(Xs), g) and fake["solve"] == [False]     # the cached alpha serves the next call
    X, y, e, Xs = _data(1)
    for kernel in ("1.0**2 * AnisotropicRBF(scale_length=[0.3])", "1.0**2 * VonKarman(length_scale=0.5)"):
        gp = tg.GPInterpolation(kernel=kernel, optimizer="none")
        gp.initialize(X, y, y_err=e)
        assert gp.predict_gradient(Xs).shape == (17, 1)


def test_predict_gradient_ignores_mean_and_mean_function(fake):
    X, y, e, Xs = _data(2)
    kernel = "0.8**2 * RBF(0.3)"

    def grad(y, normalize, table=None):
        gp = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=normalize)
        if table is not None:
            gp._X0, gp._y0 = table
        gp.initialize(X, y, y_err=e)
        return gp, gp.predict_gradient(Xs)
    base = grad(y - np.mean(y), False)[1]
    assert np.array_equal(grad(y, True)[1], base)                        # the constant of normalize drops out
    rng = np.random.default_rng(5)
    X0, y0 = rng.uniform(0, 1, (60, 2)), rng.standard_normal(60)
    gp, g = grad(y - np.mean(y), False, table=(X0, y0))
    avg = gp._spatial_average
    assert np.count_nonzero(avg) > 0
    # the same residual reached without a table gives the same gradient: the (piecewise constant) mean function adds nothing
    assert np.array_equal(g, grad(y - np.mean(y) - avg, False)[1])
    assert not np.array_equal(g, base)                                   # (it does change what the GP is fitted to)


def test_predict_gradient_errors(fake):
    X, y, e, Xs = _data(2)
    gp = tg.GPInterpolation(kernel="RBF(0.5) + WhiteKernel(1e-3)", optimizer="none")
    gp.initialize(X, y, y_err=e)
    with pytest.raises(NotImplementedError, match="WhiteKernel"):
        gp.predict_gradient(Xs)
    assert fake["solve"] == [] and fake["grad"] == []
    gp = tg.GPInterpolation(kernel="RBF(0.5)", optimizer="none")
    with pytest.raises(AttributeError):
        gp.predict(Xs)
    with pytest.raises(AttributeError):
        gp.predict_gradient(Xs)


def test_library_exports_the_new_symbols():
    lib = _lib.load_library()
    for name in ("tgp_gp_predict_grad", "tgp_d_gp_predict_grad"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "tgp.h")).read()
    assert "tgp_gp_predict_grad(" in hdr and "tgp_d_gp_predict_grad(" in hdr
    assert not hasattr(tg, "gp_predict_grad") and hasattr(tg.GPInterpolation, "predict_gradient")

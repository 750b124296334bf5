"""CPU-only checks of the 3-D entries (include/tgp.h, "S1, S2, S3 in three dimensions"): the spec mapping and the struct layout
against the header, the 2-D gate left as it was, the route choice of GPInterpolation with stand-ins for the library, the
references of tests/_nd3_refs.py against the reference project's own tables (tests/golden/g15_3d.npz), and -- from the references
alone -- that the inputs of tests/test_gpu_nd3.py reach every branch they claim."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import treegp_amd as tg
from treegp_amd import _lib, gp_interp, kernels, ops

import _nd3_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVLAM_STR = "array([[30., 4., -3.], [4., 20., 5.], [-3., 5., 12.]])"
STRINGS = {
    "arbf": "0.8**2 * AnisotropicRBF(invLam=%s)" % INVLAM_STR,
    "avk": "0.8**2 * AnisotropicVonKarman(invLam=%s)" % INVLAM_STR,
    "rbf": "0.8**2 * RBF([0.2, 0.3, 0.5])",
    "vk": "0.8**2 * VonKarman(length_scale=0.4)",
}


# ---------------------------------------------------------------------------------------------------------
# spec mapping, struct layout
def test_kernel_to_spec3_maps_the_four_kernels():
    kinds = {"arbf": _lib.TGP_ARBF, "avk": _lib.TGP_AVK, "rbf": _lib.TGP_RBF, "vk": _lib.TGP_VK}
    for tag, s in STRINGS.items():
        spec = kernels.kernel_to_spec3(tg.eval_kernel(s))
        assert isinstance(spec, ops.KernelSpec3) and spec.kind == kinds[tag]
        assert spec.amp == 0.8 ** 2
        c = spec.to_c()
        assert c.ndim == 3 and c.kind == kinds[tag] and c.amp == spec.amp and tuple(c.m) == spec.m and c.ell == spec.ell
    m = kernels.kernel_to_spec3(tg.eval_kernel(STRINGS["arbf"])).m
    assert m == (30.0, 4.0, -3.0, 20.0, 5.0, 12.0)
    assert kernels.kernel_to_spec3(tg.eval_kernel(STRINGS["vk"])).ell == 0.4
    m = kernels.kernel_to_spec3(tg.eval_kernel(STRINGS["rbf"])).m
    assert m == (1 / 0.2 ** 2, 0.0, 0.0, 1 / 0.3 ** 2, 0.0, 1 / 0.5 ** 2)
    assert kernels.kernel_to_spec3(tg.eval_kernel("RBF(0.5)")).m == (4.0, 0.0, 0.0, 4.0, 0.0, 4.0)
    with pytest.raises(NotImplementedError, match="one or three"):
        kernels.kernel_to_spec3(tg.eval_kernel("RBF([0.5, 0.4])"))
    with pytest.raises(NotImplementedError):
        kernels.kernel_to_spec3(tg.eval_kernel("AnisotropicRBF(invLam=array([[4., 0.], [0., 4.]]))"))
    with pytest.raises(NotImplementedError):                                  # sums of 3-D kernels keep the dense route
        kernels.kernel_to_spec3(tg.eval_kernel(STRINGS["arbf"] + " + " + STRINGS["vk"]))
    with pytest.raises(NotImplementedError):
        kernels.device_spec(tg.eval_kernel(STRINGS["arbf"] + " + " + STRINGS["vk"]), ndim=3)
    # a non-symmetric invLam is averaged, as _invlam_spec does
    ns = np.array([[30.0, 5.0, -3.0], [3.0, 20.0, 6.0], [-3.0, 4.0, 12.0]])
    assert kernels._invlam_spec3(_lib.TGP_ARBF, ns, 2.0).m == (30.0, 4.0, -3.0, 20.0, 5.0, 12.0)
    # the dimension comes from the coordinates: device_spec(ndim=3) for the isotropic kinds
    assert isinstance(kernels.device_spec(tg.eval_kernel(STRINGS["vk"]), ndim=3), ops.KernelSpec3)
    assert isinstance(kernels.device_spec(tg.eval_kernel(STRINGS["vk"])), ops.KernelSpec)
    with pytest.raises(ValueError, match="6 numbers"):
        ops.KernelSpec3(_lib.TGP_ARBF, m=(1.0, 2.0, 3.0))


def test_the_2d_gate_is_unchanged():
    k3 = tg.eval_kernel(STRINGS["arbf"])
    with pytest.raises(NotImplementedError, match="1-D and 2-D"):
        tg.kernel_to_spec(k3)
    with pytest.raises(NotImplementedError):
        kernels.device_spec(k3)
    s = tg.kernel_to_spec(tg.eval_kernel("0.5**2 * AnisotropicRBF(invLam=array([[400., 80.], [80., 500.]]))"))
    assert isinstance(s, ops.KernelSpec) and (s.kind, s.amp, s.a, s.b, s.c) == (_lib.TGP_ARBF, 0.25, 400.0, 80.0, 500.0)
    s = tg.kernel_to_spec(tg.eval_kernel("RBF([0.5, 0.25])"))
    assert (s.kind, s.a, s.b, s.c) == (_lib.TGP_RBF, 4.0, 0.0, 16.0)
    with pytest.raises(NotImplementedError):
        tg.kernel_to_spec(tg.eval_kernel("RBF([0.2, 0.3, 0.5])"))
    with pytest.raises(ValueError):
        _lib.as_xy(np.zeros((5, 3)))
    assert ops._coords(ops.KernelSpec(_lib.TGP_ARBF), np.zeros((4, 1))).shape == (4, 2)
    with pytest.raises(ValueError):                                           # a 2-D spec given three columns
        ops._coords(ops.KernelSpec(_lib.TGP_ARBF), np.zeros((5, 3)))


def test_as_xyz():
    X = np.arange(12.0).reshape(4, 3)
    out = _lib.as_xyz(X[::-1])
    assert out.flags["C_CONTIGUOUS"] and out.dtype == np.float64 and np.array_equal(out, X[::-1])
    assert _lib.as_xyz(X.astype(np.float32)).dtype == np.float64
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((4, 4)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError):
            _lib.as_xyz(bad)
    with pytest.raises(ValueError):
        ops._coords(ops.KernelSpec3(_lib.TGP_VK), np.zeros((4, 2)))


def test_struct_layout_and_entries_match_the_header():
    text = open(os.path.join(ROOT, "include", "tgp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} tgp_kernel3;", text).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+)(?:\[(\d+)\])?;", body, flags=re.M)
    assert [(t, n, int(c or 1)) for t, n, c in fields] == [("int32_t", "kind", 1), ("int32_t", "ndim", 1), ("double", "amp", 1),
                                                           ("double", "m", 6), ("double", "ell", 1)]
    K = _lib.TgpKernel3
    assert [(K.kind.offset, K.ndim.offset, K.amp.offset, K.m.offset, K.ell.offset)] == [(0, 4, 8, 16, 64)]
    assert ctypes.sizeof(K) == 72
    declared = set(re.findall(r"^int (tgp_\w+3)\(", text, flags=re.M))
    assert declared == {"tgp_kernel_matrix3", "tgp_d_kbuild_lower3", "tgp_gp_solve3", "tgp_gp_predict3", "tgp_gp_predict_grad3",
                        "tgp_gp_predict_cov3", "tgp_gp_predict_var3"}
    for name in declared:
        two_d = _lib.SIGNATURES[name[:-1]]
        res, args = _lib.SIGNATURES[name]
        assert res == two_d[0] and len(args) == len(two_d[1])                # the namesake's prototype with a tgp_kernel3
        assert [a for a in args if a is not ctypes.POINTER(K)] == [a for a in two_d[1] if a is not ctypes.POINTER(_lib.TgpKernel)]
    lib = _lib.load_library()
    assert all(hasattr(lib, n) for n in declared)


def test_entry_dispatch_by_spec_type():
    class Lib(object):
        tgp_gp_solve = "2d"
        tgp_gp_solve3 = "3d"
        tgp_gp_solve_sum = "sum"
    assert ops._entry(Lib, "tgp_gp_solve", ops.KernelSpec3(_lib.TGP_ARBF)) == ("3d", "tgp_gp_solve3")
    assert ops._entry(Lib, "tgp_gp_solve", ops.KernelSpec(_lib.TGP_ARBF)) == ("2d", "tgp_gp_solve")
    assert ops._entry(Lib, "tgp_gp_solve", ops.KernelSumSpec([ops.KernelSpec(_lib.TGP_ARBF)])) == ("sum", "tgp_gp_solve_sum")


# ---------------------------------------------------------------------------------------------------------
# route choice with stand-ins for the library
class Calls(list):
    def names(self):
        return [c[0] for c in self]


@pytest.fixture
def fake(monkeypatch):
    calls = Calls()

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        calls.append(("gp_solve", spec, np.shape(X)))
        return (np.zeros(len(X)) if want_alpha else None), 0.0, 0.0, None

    def gp_predict(spec, X, alpha, Xs, ctx=None):
        calls.append(("gp_predict", spec, np.shape(Xs)))
        return np.zeros(len(Xs))

    def gp_predict_grad(spec, X, alpha, Xs, ctx=None):
        calls.append(("gp_predict_grad", spec, np.shape(Xs)))
        return np.zeros((len(Xs), 3 if isinstance(spec, ops.KernelSpec3) else 2))

    def gp_solve_dense(K, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        calls.append(("gp_solve_dense", None, np.shape(K)))
        return (np.zeros(len(K)) if want_alpha else None), 0.0, 0.0, None

    def kernel_matrix(spec, X, Y=None, ctx=None):
        calls.append(("kernel_matrix", spec, np.shape(X)))
        return np.eye(len(X)) if Y is None else np.zeros((len(X), len(Y)))

    def gp_solve_batch(*a, **k):
        raise AssertionError("a 3-D object must not reach the batched routes")

    for name, fn in (("gp_solve", gp_solve), ("gp_predict", gp_predict), ("gp_predict_grad", gp_predict_grad),
                     ("gp_solve_dense", gp_solve_dense), ("kernel_matrix", kernel_matrix), ("gp_solve_batch", gp_solve_batch),
                     ("gp_posterior_batch", gp_solve_batch), ("gp_loo_batch", gp_solve_batch)):
        monkeypatch.setattr(ops, name, fn)
    return calls


def _gp3(kernel=STRINGS["arbf"], n=12, **kw):
    rng = np.random.default_rng(1)
    gp = tg.GPInterpolation(kernel=kernel, optimizer=kw.pop("optimizer", "none"), **kw)
    gp.initialize(rng.uniform(size=(n, 3)), rng.standard_normal(n), y_err=0.1 * np.ones(n))
    return gp


def test_3d_objects_take_the_device_route(fake):
    for tag, s in STRINGS.items():
        del fake[:]
        gp = _gp3(s)
        out = gp.predict(np.zeros((5, 3)))
        assert out.shape == (5,)
        assert fake.names() == ["gp_solve", "gp_predict"], (tag, fake.names())
        assert all(isinstance(c[1], ops.KernelSpec3) for c in fake)
        g = gp.predict_gradient(np.zeros((5, 3)))
        assert g.shape == (5, 3) and fake.names()[-1] == "gp_predict_grad" and isinstance(fake[-1][1], ops.KernelSpec3)
        assert np.isfinite(gp.return_log_likelihood()) and fake.names()[-1] == "gp_solve"
    # a sum of 3-D kernels: the dense route, its matrices from the classes' own __call__ through ops.kernel_matrix
    del fake[:]
    gp = _gp3(STRINGS["arbf"] + " + " + STRINGS["avk"])
    gp.predict(np.zeros((5, 3)))
    assert "gp_solve_dense" in fake.names() and "gp_solve" not in fake.names()
    assert all(isinstance(c[1], ops.KernelSpec3) for c in fake if c[0] == "kernel_matrix") and "kernel_matrix" in fake.names()
    # the fingerprint of a kept factor tells 3-D kernels apart
    a = gp_interp.GPInterpolation._factor_fingerprint(ops.KernelSpec3(1, m=(1, 0, 0, 1, 0, 1)), np.zeros((2, 3)), np.zeros(2))
    b = gp_interp.GPInterpolation._factor_fingerprint(ops.KernelSpec3(1, m=(1, 0, 0.5, 1, 0, 1)), np.zeros((2, 3)), np.zeros(2))
    assert a != b


def test_2d_statistics_raise_for_3d(fake, tmp_path):
    for opt in ("two-pcf", "anisotropic"):
        gp = _gp3(optimizer=opt)
        with pytest.raises(ValueError, match="2-D statistic"):
            gp.solve()
    gp = tg.GPInterpolation(kernel=STRINGS["arbf"], optimizer="none")
    gp._X0, gp._y0 = np.ones((6, 2)), np.ones(6)                              # a mean-function table is present
    with pytest.raises(ValueError, match="2-D statistic"):
        gp.initialize(np.zeros((4, 3)), np.zeros(4))
    assert not fake


def test_batch_helpers_exclude_3d_objects(fake):
    gp3, gp2 = _gp3(), tg.GPInterpolation(kernel="0.5**2 * RBF(0.3)", optimizer="none")
    gp2.initialize(np.random.default_rng(0).uniform(size=(10, 2)), np.zeros(10), y_err=0.1 * np.ones(10))
    assert gp_interp._batch_spec(gp3) is None and gp_interp._batch_spec(gp2) is not None
    out = gp_interp.predict_many([gp3], [np.zeros((4, 3))])                   # gp_solve_batch would raise
    assert out[0].shape == (4,) and fake.names() == ["gp_solve", "gp_predict"]


def test_log_likelihood_fit_differences_for_3d(fake, monkeypatch):
    LL = sys.modules["treegp_amd.log_likelihood"]
    X = np.random.default_rng(2).uniform(size=(9, 3))
    for mode in ("auto", "analytic", "analytic-vk"):
        monkeypatch.setenv("TGP_ML_GRADIENT", mode)
        ll = LL.log_likelihood(X, np.zeros(9), 0.1 * np.ones(9))
        assert ll.three_d and not ll._use_exact_gradient(tg.eval_kernel(STRINGS["arbf"]))
        assert isinstance(ll._device_spec(tg.eval_kernel(STRINGS["vk"])), ops.KernelSpec3)
    monkeypatch.setattr(LL, "_PARALLEL_MAX_N", 4)                             # "above N = 16 384": still finite differences
    ll = LL.log_likelihood(X, np.zeros(9), 0.1 * np.ones(9))
    assert not ll.parallel_fd and not ll._use_exact_gradient(tg.eval_kernel(STRINGS["arbf"]))
    del fake[:]
    assert np.all(np.isfinite(ll.log_likelihood_many([tg.eval_kernel(STRINGS["arbf"])])))     # no batched solve
    assert fake.names() == ["gp_solve"]


def test_dense_route_under_an_active_multi_gpu_engine(fake, monkeypatch):
    class Engine(object):
        def gp_solve(self, *a, **k):
            raise AssertionError("the multi-GPU engine has no 3-D K build")
        gp_predict = gp_solve
    real = ops._dist_engine
    monkeypatch.setattr(ops, "_dist_engine", lambda n, ctx: Engine())
    gp = _gp3()
    gp.predict(np.zeros((5, 3)))
    assert "gp_solve_dense" in fake.names() and "gp_solve" not in fake.names() and "gp_predict" not in fake.names()
    assert all(isinstance(c[1], ops.KernelSpec3) for c in fake if c[0] == "kernel_matrix")
    LL = sys.modules["treegp_amd.log_likelihood"]
    ll = LL.log_likelihood(gp._X, gp._y, gp._y_err)
    assert ll.distributed
    with pytest.raises(NotImplementedError):
        ll._device_spec(gp.kernel)
    monkeypatch.setattr(ops, "_dist_engine", real)


# ---------------------------------------------------------------------------------------------------------
# the references against the reference project's own tables
def test_references_match_the_golden_tables(golden):
    g = golden("g15_3d.npz")
    X, Xs = g["X"], g["Xs"]
    for tag, kernel in R.KERNELS.items():
        assert str(g[tag + "_kernel"]) == STRINGS[tag]
        ns, nc = (96, 70) if tag in ("arbf", "rbf") else (28, 16)            # (mpmath's Bessel function: a sub-block)
        ref, _ = R.kernel_matrix_mp(kernel, X[:ns])
        np.testing.assert_allclose(ref.astype(float), g[tag + "_self"][:ns, :ns], rtol=2e-12, atol=1e-14, err_msg=tag)
        ref, _ = R.kernel_matrix_mp(kernel, Xs[:nc], X[:ns])
        np.testing.assert_allclose(ref.astype(float), g[tag + "_cross"][:nc, :ns], rtol=2e-12, atol=1e-14, err_msg=tag)
        assert np.all(np.diag(g[tag + "_self"]) == 0.8 ** 2)
    for tag in ("arbf", "rbf"):
        kernel = R.KERNELS[tag]
        np.testing.assert_allclose(R.gauss_matrix_ld(kernel, Xs, X[:96]).astype(float), g[tag + "_cross"], rtol=2e-12, atol=1e-14)
        gp = R.DenseGP(kernel, X, g["y_err"])
        mean = np.mean(g["y"])
        alpha = gp.solve(R.LD(g["y"]) - R.LD(mean))
        amax = np.abs(g[tag + "_alpha"]).max()
        np.testing.assert_allclose(alpha.astype(float), g[tag + "_alpha"], rtol=0, atol=1e-9 * amax)
        yp = (gp.predict(alpha, Xs) + R.LD(mean)).astype(float)
        np.testing.assert_allclose(yp, g[tag + "_y_pred"], rtol=0, atol=1e-10 * np.abs(g[tag + "_y_pred"]).max())
        cov = gp.cov(Xs[:64]).astype(float)
        np.testing.assert_allclose(cov, g[tag + "_cov64"], rtol=0, atol=1e-9 * np.abs(g[tag + "_cov64"]).max())
        r = R.LD(g["y"]) - R.LD(mean)
        logl = float(-0.5 * (r @ alpha) - 0.5 * len(X) * np.log(R.LD(2.0) * np.pi) - 0.5 * gp.logdet())
        np.testing.assert_allclose(logl, g[tag + "_logL"][0], rtol=1e-11)


def test_slope_reference_is_the_derivative_of_the_value():
    import mpmath as mp
    for tag, kernel in R.KERNELS.items():
        xi = np.array([0.1, 0.2, 0.3])
        for xq in (np.array([0.15, 0.1, 0.45]), np.array([0.6, -0.3, 0.2])):
            g = R.grad_pair_mp(kernel, xq, xi)
            for a in range(3):
                f = lambda t: R.value_of_d_mp(kernel, [mp.mpf(float(xq[b])) - mp.mpf(float(xi[b])) + (t if b == a else 0)
                                                       for b in range(3)])[0]
                num = mp.diff(f, 0)
                assert abs(num - g[a]) <= mp.mpf(10) ** -25 * max(abs(g[a]), 1), (tag, a)
        assert R.grad_pair_mp(kernel, xi, xi) == [0, 0, 0]                     # a pair at u == 0 contributes exactly 0


# ---------------------------------------------------------------------------------------------------------
# the GPU test's inputs reach every branch they claim (from the references alone)
def test_gauss_inputs_reach_every_residue_and_the_underflow():
    for tag in ("arbf", "rbf"):
        kernel = R.KERNELS[tag]
        P = R.value_queries(tag)
        ref, s = R.kernel_matrix_mp(kernel, P, R.VALUE_CENTER[None, :])
        ref, s = ref[:, 0], s[:, 0]
        assert s[0] == 0.0 and float(ref[0]) == kernel[1]                     # the coincident point
        assert set(R.gauss_residues(s[s > 0.5]).tolist()) == set(range(256)), tag
        assert s.min() == 0.0 and np.sort(s)[1] < 1e-7 and s.max() > 800.0
        f = ref.astype(float)
        assert ((f > 0) & (f < 2.0 ** -1022)).sum() >= 3, "subnormal values"
        assert (ref < R.LD(kernel[1]) * np.ldexp(R.LD(1.0), -1075)).sum() >= 3, "flushed values"
        # the matrix has a Cholesky factor (transformed path) and the diameter bound is finite
        np.linalg.cholesky(kernel[2])
        assert np.isfinite(R.diameter_exponent(kernel[2], P[::10]))


def test_fallback_invlams_have_no_cholesky_factor():
    for M in (R.RANK_ONE, R.INDEFINITE):
        assert np.array_equal(M, M.T)
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(M)
    # what the launcher tests (csrc/nd3.hip: cholesky3): d11 == 0 exactly for v v^T, < 0 for the indefinite matrix
    for M, cmp in ((R.RANK_ONE, lambda d: d == 0.0), (R.INDEFINITE, lambda d: d < 0.0)):
        l10 = M[0, 1] / np.sqrt(M[0, 0])
        assert M[0, 0] > 0 and cmp(M[1, 1] - l10 * l10)
    assert np.linalg.eigvalsh(R.INDEFINITE).min() < 0 < np.linalg.eigvalsh(R.INDEFINITE).max()
    assert np.linalg.matrix_rank(R.RANK_ONE) == 1


def test_von_karman_inputs_reach_every_segment_and_the_cut():
    for tag in ("avk", "vk"):
        kernel = R.KERNELS[tag]
        P = R.value_queries(tag)
        d = P - R.VALUE_CENTER
        if tag == "vk":
            x = 2 * np.pi * np.sqrt((d * d).sum(axis=1)) / kernel[3]
        else:
            x = 2 * np.pi * np.sqrt(np.einsum("ia,ab,ib->i", d, kernel[2], d))
        seg = R.vk_segment(x)
        counts = np.bincount(seg, minlength=8)
        assert counts.min() >= 5, (tag, dict(zip(R.VK_SEGMENTS, counts)))
        assert x[0] == 0.0                                                     # the coincident point
        assert float(R.pair_mp(kernel, P[0], R.VALUE_CENTER)[0]) == kernel[1]

"""CPU-only checks of local kriging (include/tgp.h, seam S3l): the entry against the header and the loaded library, the host
reference of tests/_local_refs.py against the oracle's dense predict at k = n and against its own definition, the Python layer
(``ops.gp_predict_local``, ``GPInterpolation.predict_local``) with stand-ins for the library, and the grid build of
treegp_amd/csrc/local_grid.h as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import treegp_amd as tg
from treegp_amd import _lib, ops
from oracle import gp_oracle as O

import _local_refs as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------
# the C ABI
def test_entry_matches_the_header_and_the_library():
    text = open(os.path.join(ROOT, "include", "tgp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"^int (tgp_gp_predict_local\w*)\(([^;]*)\);", code, flags=re.M | re.S))
    assert set(protos) == {"tgp_gp_predict_local"}
    args = [" ".join(a.split()) for a in protos["tgp_gp_predict_local"].split(",")]
    assert args == ["tgp_ctx *ctx", "const tgp_kernel *k", "const double *X", "int64_t n", "const double *y", "const double *yerr",
                    "const double *Xs", "int64_t m", "int kn", "double *ys", "double *var", "int32_t *nbr", "int32_t *info"]
    res, argtypes = _lib.SIGNATURES["tgp_gp_predict_local"]
    vp = ctypes.c_void_p
    assert res is ctypes.c_int
    assert argtypes == [vp, ctypes.POINTER(_lib.TgpKernel), vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp, vp, vp]
    assert "S3l" in text
    assert hasattr(_lib.load_library(), "tgp_gp_predict_local")
    assert hasattr(ops, "gp_predict_local") and hasattr(tg.GPInterpolation, "predict_local")


# ---------------------------------------------------------------------------------------------------------
# the reference
@pytest.mark.parametrize("name", ["rbf", "arbf", "vk", "avk"])
@pytest.mark.parametrize("n", [1, 5, 64, 130])
def test_reference_is_the_dense_gp_when_k_is_n(name, n):
    spec = LR.make_spec(name)
    X, y, y_err, Xs = LR.uniform_data(n, 40, seed=n)
    ys, var, nbr, info = LR.local_predict(spec, X, y, y_err, Xs, k=n)
    assert nbr.shape == (40, n) and not info.any()
    assert (np.sort(nbr, axis=1) == np.arange(n)).all()
    ys_d, var_d = LR.dense_predict(spec, X, y, y_err, Xs)
    e_y, e_v = np.abs(ys - ys_d).max() / np.abs(y).max(), np.abs(var - var_d).max() / spec.amp
    print("k = n = %d %s: |dys| %.2e of max|y|, |dvar| %.2e of amp" % (n, name, e_y, e_v))
    assert e_y <= 1e-10 and e_v <= 1e-10


def test_reference_neighbours_and_their_checks():
    spec = LR.make_spec("arbf")
    r00, r01, r11 = LR.whitening(spec)
    assert abs(r00 * r00 - spec.a) < 1e-13 * spec.a and abs(r00 * r01 - spec.b) < 1e-13 * abs(spec.b)
    assert abs(r01 * r01 + r11 * r11 - spec.c) < 1e-13 * spec.c
    X, y, y_err, Xs = LR.uniform_data(300, 50)
    D = LR.dist2(spec, X, Xs)
    d = X[None, :, :] - Xs[:, None, :]
    q = spec.a * d[..., 0] ** 2 + 2 * spec.b * d[..., 0] * d[..., 1] + spec.c * d[..., 1] ** 2
    np.testing.assert_allclose(D, q, rtol=1e-11, atol=1e-13)               # the whitened distance is the Mahalanobis one
    nbr = LR.brute_neighbors(spec, X, Xs, 17)
    LR.check_neighbor_sets(spec, X, Xs, nbr)
    wrong = np.array(nbr)
    far = np.argmax(D, axis=1)
    wrong[:, -1] = far                                                     # a nearer row is left out
    with pytest.raises(AssertionError, match="left out"):
        LR.check_neighbor_sets(spec, X, Xs, wrong)
    with pytest.raises(AssertionError, match="nearest first"):
        LR.check_neighbor_sets(spec, X, Xs, nbr[:, ::-1].copy())
    twice = np.array(nbr)
    twice[:, 1] = twice[:, 0]
    with pytest.raises(AssertionError, match="twice"):
        LR.check_neighbor_sets(spec, X, Xs, twice)
    # ties go to the lower row: a lattice, queries on its sites
    g = np.arange(6.0)
    L = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    nb = LR.brute_neighbors(LR.make_spec("rbf"), L, L[14:15], 5)
    assert nb[0, 0] == 14 and list(nb[0, 1:]) == [8, 13, 15, 20]
    with pytest.raises(np.linalg.LinAlgError):
        LR.whitening(LR.make_spec("arbf", a=1.0, b=2.0, c=1.0))


def test_reference_reports_the_failing_minor():
    spec = LR.make_spec("rbf")
    X = np.array([[0.0, 0.0], [0.1, 0.0], [0.1, 0.0], [0.3, 0.2]])
    y = np.array([1.0, 2.0, 3.0, 4.0])
    nbr = np.array([[0, 1, 2, 3], [3, 0, 1, 2]], dtype=np.int32)
    ys, var, info = LR.local_predict_ld(spec, X, y, None, np.array([[0.0, 0.1], [0.2, 0.2]]), nbr)
    assert list(info) == [3, 4] and np.isnan(ys).all() and np.isnan(var).all()
    ys, var, info = LR.local_predict_ld(spec, X, y, np.full(4, 0.1), np.array([[0.0, 0.1], [0.2, 0.2]]), nbr)
    assert not info.any() and np.isfinite(ys).all()
    # k = 1 in closed form
    ys, var, info = LR.local_predict_ld(spec, X, y, np.full(4, 0.1), np.array([[0.05, 0.0]]), np.array([[1]], dtype=np.int32))
    ks = LR.kernel_values(spec, np.array([[0.05, 0.0]]), X[1:2])[0, 0]
    assert abs(ys[0] - ks * 2.0 / (spec.amp + 0.01)) < 1e-15 and abs(var[0] - (spec.amp - ks * ks / (spec.amp + 0.01))) < 1e-15


# ---------------------------------------------------------------------------------------------------------
# ops.gp_predict_local with a stand-in for the library
class FakeLib(object):
    """answers tgp_gp_predict_local with the host reference, writing through the pointers it is given"""

    def __init__(self):
        self.calls = []

    def tgp_gp_predict_local(self, ctx, kref, X, n, y, yerr, Xs, m, kn, ys, var, nbr, info):
        k = kref._obj
        spec = ops.KernelSpec(k.kind, k.amp, k.a, k.b, k.c, k.ell)

        def arr(p, count, ctype=ctypes.c_double):
            return None if p is None else np.ctypeslib.as_array((ctype * count).from_address(p.value))
        Xa, ya, ea = arr(X, 2 * n).reshape(n, 2), arr(y, n), arr(yerr, n)
        Xsa = arr(Xs, 2 * m).reshape(m, 2)
        self.calls.append(dict(n=n, m=m, kn=kn, var=var is not None, nbr=nbr is not None, yerr=ea is not None, spec=spec))
        r_ys, r_var, r_nbr, r_info = LR.local_predict(spec, Xa, ya, ea, Xsa, kn)
        arr(ys, m)[:] = r_ys
        if var is not None:
            arr(var, m)[:] = r_var
        if nbr is not None:
            arr(nbr, m * kn, ctypes.c_int32).reshape(m, kn)[:] = r_nbr
        arr(info, m, ctypes.c_int32)[:] = r_info
        return 0

    def tgp_last_error(self, ctx):
        return b"stand-in"


@pytest.fixture
def fakelib(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    monkeypatch.setattr(_lib, "get_ctx", lambda device=None: None)
    return lib


def test_ops_plumbing_and_k_clipping(fakelib):
    spec = LR.make_spec("arbf")
    X, y, y_err, Xs = LR.uniform_data(50, 7)
    ys = ops.gp_predict_local(spec, X, y, y_err, Xs, k=8)
    assert isinstance(ys, np.ndarray) and ys.shape == (7,)
    ys2, var, nbr = ops.gp_predict_local(spec, X, y, y_err, Xs, k=8, return_var=True, return_neighbors=True)
    assert np.array_equal(ys, ys2) and var.shape == (7,) and nbr.shape == (7, 8) and nbr.dtype == np.int32
    assert fakelib.calls[0] == dict(n=50, m=7, kn=8, var=False, nbr=False, yerr=True, spec=fakelib.calls[0]["spec"])
    assert fakelib.calls[1]["var"] and fakelib.calls[1]["nbr"]
    # the default k is 64 and k is clipped to n: the exact GP
    ys3, nbr3 = ops.gp_predict_local(spec, X, y, y_err, Xs, return_neighbors=True)
    assert fakelib.calls[-1]["kn"] == 50 and nbr3.shape == (7, 50)
    ys_d, _ = LR.dense_predict(spec, X, y, y_err, Xs)
    assert np.abs(ys3 - ys_d).max() <= 1e-10 * np.abs(y).max()
    # no errors given, 1-D coordinates (zero second column), a (var,) pair alone
    ys4, var4 = ops.gp_predict_local(LR.make_spec("rbf"), X[:, 0], y, None, Xs[:, :1], k=2, return_var=True)
    assert not fakelib.calls[-1]["yerr"] and fakelib.calls[-1]["kn"] == 2 and var4.shape == (7,)
    # no queries: nothing reaches the library
    before = len(fakelib.calls)
    out = ops.gp_predict_local(spec, X, y, y_err, np.zeros((0, 2)), k=4, return_neighbors=True)
    assert out[0].shape == (0,) and out[1].shape == (0, 4) and len(fakelib.calls) == before


def test_ops_argument_errors(fakelib):
    spec = LR.make_spec("rbf")
    X, y, y_err, Xs = LR.uniform_data(20, 3)
    for k in (0, 129, -1, 2.5):
        with pytest.raises(ValueError, match="1 .. 128"):
            ops.gp_predict_local(spec, X, y, y_err, Xs, k=k)
    with pytest.raises(ValueError, match="y 19 values"):
        ops.gp_predict_local(spec, X, y[:19], y_err, Xs)
    with pytest.raises(ValueError, match="y_err 19 values"):
        ops.gp_predict_local(spec, X, y, y_err[:19], Xs)
    with pytest.raises(ValueError, match="only 1-D and 2-D"):
        ops.gp_predict_local(spec, np.zeros((20, 3)), y, y_err, Xs)
    with pytest.raises(NotImplementedError, match="sum of kernels"):
        ops.gp_predict_local(ops.KernelSumSpec([spec, spec]), X, y, y_err, Xs)
    with pytest.raises(NotImplementedError, match="3-D"):
        ops.gp_predict_local(ops.KernelSpec3(_lib.TGP_RBF), np.zeros((20, 3)), y, y_err, np.zeros((3, 3)))
    with pytest.raises(ValueError, match="KernelSpec"):
        ops.gp_predict_local("RBF(1)", X, y, y_err, Xs)
    assert fakelib.calls == []
    # an argument error of the library (-1) surfaces as TgpError with its message
    fakelib.tgp_gp_predict_local = lambda *a: -1
    with pytest.raises(_lib.TgpError, match="stand-in") as ei:
        ops.gp_predict_local(spec, X, y, y_err, Xs)
    assert ei.value.rc == -1


def test_ops_names_the_first_failed_query(fakelib):
    spec = LR.make_spec("rbf")
    X = np.array([[0.0, 0.0], [0.1, 0.0], [0.1, 0.0], [0.9, 0.9], [0.95, 0.9]])
    y = np.arange(5.0)
    Xs = np.array([[0.9, 0.92], [0.1, 0.01], [0.0, 0.02]])
    with pytest.raises(np.linalg.LinAlgError, match=r"query 1: the 2-th leading minor") as ei:
        ops.gp_predict_local(spec, X, y, None, Xs, k=2, return_var=True)
    assert list(ei.value.info) == [0, 2, 0]
    ys, var = ei.value.results
    assert np.isnan(ys[1]) and np.isnan(var[1]) and np.isfinite(ys[[0, 2]]).all()


# ---------------------------------------------------------------------------------------------------------
# GPInterpolation.predict_local with stand-ins for the device
@pytest.fixture
def fake_device(monkeypatch):
    """every ops call of predict / predict_local answered on the host; each one is recorded"""
    calls = []

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        calls.append("gp_solve")
        alpha, logdet = O.gp_solve(LR.kernel_values(spec, X), np.asarray(y, dtype=float), np.asarray(y_err, dtype=float))
        return alpha, logdet, float(np.dot(y, alpha)), None

    def gp_predict(spec, X, alpha, Xs, ctx=None):
        calls.append("gp_predict")
        return O.gp_predict(LR.kernel_values(spec, Xs, X), alpha)

    def gp_predict_local(spec, X, y, y_err, Xs, k=64, return_var=False, return_neighbors=False, ctx=None):
        calls.append(("gp_predict_local", k, LR.as_xy(X).shape, LR.as_xy(Xs).shape))
        ys, var, nbr, info = LR.local_predict(spec, LR.as_xy(X), y, y_err, LR.as_xy(Xs), k)
        out = (ys,) + ((var,) if return_var else ()) + ((nbr,) if return_neighbors else ())
        return out if len(out) > 1 else ys

    def knn_mean(X0, y0, X, k=4, ctx=None):
        calls.append("knn_mean")
        return O.knn_mean(np.asarray(X0), np.asarray(y0), LR.as_xy(X)[:, :np.shape(X0)[1]], k)

    def forbidden(*a, **k):
        raise AssertionError("predict_local performs no dense factorisation")

    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_predict", gp_predict)
    monkeypatch.setattr(ops, "gp_predict_local", gp_predict_local)
    monkeypatch.setattr(ops, "knn_mean", knn_mean)
    monkeypatch.setattr(ops, "gp_solve_dense", forbidden)
    monkeypatch.setattr(ops, "_dist_engine", lambda n, ctx: None)
    return calls


KERN = "0.8**2 * AnisotropicRBF(invLam=array([[60., -14.], [-14., 35.]]))"


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("table", [False, True])
def test_mean_and_mean_function_are_handled_as_in_predict(fake_device, normalize, table):
    X, y, y_err, Xs = LR.uniform_data(60, 25, seed=3)
    y = y + 7.5
    gp = tg.GPInterpolation(kernel=KERN, optimizer="none", normalize=normalize, white_noise=0.02)
    if table:
        rng = np.random.default_rng(1)
        gp._X0, gp._y0 = rng.uniform(size=(30, 2)), 7.0 + rng.standard_normal(30)
    gp.initialize(X, y, y_err=y_err)
    del fake_device[:]
    ys, var = gp.predict_local(Xs, k=60, return_var=True)
    assert gp._alpha is None and gp._factor is None                      # no solve, nothing cached
    assert [c for c in fake_device if c != "knn_mean"] == [("gp_predict_local", 60, (60, 2), (25, 2))]
    ref = gp.predict(Xs)
    assert np.abs(ys - ref).max() <= 2e-10 * np.abs(y).max()
    assert "gp_solve" in fake_device
    # the residual handed down is y - mean - mean function, the errors carry the white noise
    seen = {}

    def spy(spec, X_, y_, e_, Xs_, k=64, return_var=False, return_neighbors=False, ctx=None):
        seen.update(y=np.array(y_), e=np.array(e_), k=k)
        return np.zeros(len(Xs_))
    ops.gp_predict_local = spy
    out = gp.predict_local(Xs)
    np.testing.assert_array_equal(seen["y"], gp._y - gp._mean - gp._spatial_average)
    np.testing.assert_allclose(seen["e"], np.sqrt(y_err ** 2 + 0.02 ** 2))
    assert seen["k"] == 64
    np.testing.assert_array_equal(out, gp._mean + gp._build_average_meanify(Xs))
    if not normalize:
        assert gp._mean == 0.0


def test_object_method_shapes_clipping_and_one_dimension(fake_device):
    X, y, y_err, Xs = LR.uniform_data(40, 9, seed=5)
    gp = tg.GPInterpolation(kernel="0.8**2 * RBF(0.2)", optimizer="none")
    gp.initialize(X[:, :1], y, y_err=y_err)
    ys, nbr = gp.predict_local(Xs[:, :1], k=128, return_neighbors=True)         # k >= n: clipped, the exact GP
    assert ys.shape == (9,) and nbr.shape == (9, 40)
    assert fake_device[-1] == ("gp_predict_local", 128, (40, 2), (9, 2))       # 1-D X goes through predict's padding
    ref = gp.predict(Xs[:, :1])
    assert np.abs(ys - ref).max() <= 2e-10 * np.abs(y).max()
    ys3, var3, nbr3 = gp.predict_local(Xs[:, :1], k=5, return_var=True, return_neighbors=True)
    assert var3.shape == (9,) and nbr3.shape == (9, 5) and (var3 > 0).all()
    _, var_full = gp.predict_local(Xs[:, :1], k=40, return_var=True)
    assert (var3 >= var_full - 1e-12).all()                                     # fewer stars never know more


def test_refusals_of_the_object_method(fake_device):
    X, y, y_err, Xs = LR.uniform_data(20, 4)
    for kern in ("0.7**2 * RBF(0.2) + WhiteKernel(0.01)", "0.7**2 * Matern(0.2, nu=1.5)"):
        gp = tg.GPInterpolation(kernel=kern, optimizer="none")
        gp.initialize(X, y, y_err=y_err)
        with pytest.raises(NotImplementedError, match="dense route"):
            gp.predict_local(Xs)
    gp = tg.GPInterpolation(kernel="0.3**2 * RBF(0.2) + 0.5**2 * RBF(0.7)", optimizer="none")
    gp.initialize(X, y, y_err=y_err)
    with pytest.raises(NotImplementedError, match="sum of kernels"):
        gp.predict_local(Xs)
    X3 = np.random.default_rng(2).uniform(size=(20, 3))
    gp = tg.GPInterpolation(kernel="0.8**2 * RBF([0.2, 0.3, 0.5])", optimizer="none")
    gp.initialize(X3, y, y_err=y_err)
    with pytest.raises(NotImplementedError, match="3-D"):
        gp.predict_local(X3[:4])
    assert fake_device == []


# ---------------------------------------------------------------------------------------------------------
# the grid build on the host, under sanitizers
def test_grid_build_under_sanitizers(tmp_path):
    """tests/sanitize/local_grid_driver.cpp: the plain host functions of treegp_amd/csrc/local_grid.h (whitening factor, grid plan,
    counting sort) compiled alone with AddressSanitizer + UBSan and driven with uniform, clustered, collinear, 1-D, duplicated,
    lattice, far-away, NaN and overflowing inputs in exact-size buffers."""
    # the compiler that builds the library's host side (tools/sanitize_host.sh uses it too): clang links the sanitizer runtimes
    # into the program itself
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    assert cxx is not None, "no clang++ found next to hipcc"
    exe = str(tmp_path / "local_grid_driver")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "local_grid_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "local grid ok under sanitizers" in r.stdout

"""CPU-only checks of the local conditionals (include/tgp.h, seam S3v): the entry against the header and the loaded library, the
host reference of tests/_vecchia_refs.py against the dense GP in its two exact limits (PRIOR with k = n - 1 is the dense
log-likelihood by the chain rule; LOO with k = n - 1 is the closed form from K^-1), the Python layer (``ops.gp_local_cond``,
``ops.vecchia_rank``, the ``GPInterpolation`` methods and the ``local-likelihood`` optimiser) with stand-ins for the library, and
the host checks of treegp_amd/csrc/local_grid.h as a stand-alone program under AddressSanitizer + UBSan."""
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
import _vecchia_refs as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------
# the C ABI
def test_entry_matches_the_header_and_the_library():
    text = open(os.path.join(ROOT, "include", "tgp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"^int (tgp_gp_local_cond\w*)\(([^;]*)\);", code, flags=re.M | re.S))
    assert set(protos) == {"tgp_gp_local_cond"}
    args = [" ".join(a.split()) for a in protos["tgp_gp_local_cond"].split(",")]
    assert args == ["tgp_ctx *ctx", "const tgp_kernel *k", "const double *X", "int64_t n", "const double *y", "const double *yerr",
                    "int mode", "const int32_t *rank", "int kn", "const int32_t *nbr_in", "double *mu", "double *var", "int32_t *nbr",
                    "int32_t *cnt", "int32_t *info", "double *sums"]
    assert re.search(r"^#define TGP_LOCAL_LOO 0$", code, flags=re.M) and re.search(r"^#define TGP_LOCAL_PRIOR 1$", code, flags=re.M)
    assert ops.LOCAL_MODES == {"loo": 0, "prior": 1}
    res, argtypes = _lib.SIGNATURES["tgp_gp_local_cond"]
    vp = ctypes.c_void_p
    assert res is ctypes.c_int
    assert argtypes == [vp, ctypes.POINTER(_lib.TgpKernel), vp, ctypes.c_int64, vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp,
                        vp, vp, vp, vp]
    assert "S3v" in text and text.index("S3l: local kriging") < text.index("S3v: local conditionals") < text.index("S3b: cov")
    assert hasattr(_lib.load_library(), "tgp_gp_local_cond")
    for name in ("predict_loo_local", "return_loo_log_predictive_local", "return_log_likelihood_local"):
        assert hasattr(tg.GPInterpolation, name)


# ---------------------------------------------------------------------------------------------------------
# the reference in its exact limits
@pytest.mark.parametrize("name", ["rbf", "arbf", "vk", "avk"])
def test_reference_prior_with_all_predecessors_is_the_dense_likelihood(name):
    n = 40
    spec = LR.make_spec(name)
    X, y, y_err, _ = LR.uniform_data(n, 1, seed=40)
    rank = ops.vecchia_rank(n, seed=3)
    mu, var, nbr, cnt, info = VR.cond_reference(spec, X, y, y_err, n - 1, "prior", rank)
    assert not info.any() and np.array_equal(cnt, rank)                  # every predecessor, and nothing else
    assert mu[rank == 0] == 0.0 and var[rank == 0] == spec.amp
    ll = VR.log_score_ld(y, y_err, mu, var)
    alpha, logdet = O.gp_solve(LR.kernel_values(spec, X), y, y_err)       # the oracle's dense route, float64
    chi2 = float(np.dot(y, alpha))
    ll_dense = -0.5 * chi2 - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
    # the rounding of the float64 dense route: 1e-10 of the quantity's scale, the tolerance of test_local_host.py at k = n
    scale = 0.5 * abs(chi2) + 0.5 * abs(logdet) + 0.5 * n * np.log(2.0 * np.pi)
    print("%s: chain rule - dense = %.3e of %.3e" % (name, float(ll - LD(ll_dense)), scale))
    assert abs(float(ll - LD(ll_dense))) <= 1e-10 * scale
    # and against the long-double dense factorisation of this file's own
    ll_ld, _, _ = VR.dense_loglik_ld(LR.kernel_values(spec, X), y, y_err)
    assert abs(float(ll - ll_ld)) <= 1e-10 * scale


@pytest.mark.parametrize("name", ["rbf", "avk"])
def test_reference_loo_with_all_others_is_the_closed_form(name):
    n = 40
    spec = LR.make_spec(name)
    X, y, y_err, _ = LR.uniform_data(n, 1, seed=41)
    mu, var, nbr, cnt, info = VR.cond_reference(spec, X, y, y_err, n - 1, "loo")
    assert not info.any() and (cnt == n - 1).all()
    assert ((np.sort(nbr, axis=1) == np.array([np.delete(np.arange(n), i) for i in range(n)])).all())
    mu_c, var_c = VR.loo_closed_form(LR.kernel_values(spec, X), y, y_err)
    e_m, e_v = np.abs(mu - mu_c).max() / np.abs(y).max(), np.abs(var - var_c).max() / spec.amp
    print("%s: LOO against K^-1: |dmu| %.2e of max|y|, |dvar| %.2e of amp" % (name, e_m, e_v))
    assert e_m <= 1e-10 and e_v <= 1e-10


def test_reference_lists_and_their_checks():
    spec = LR.make_spec("arbf")
    X, y, y_err, _ = LR.uniform_data(120, 1)
    rank = ops.vecchia_rank(120, seed=1)
    for mode, rk in (("loo", None), ("prior", rank)):
        nbr, cnt = VR.brute_lists(spec, X, 9, mode, rk)
        VR.check_lists(spec, X, nbr, cnt, 9, mode, rk)
        if mode == "prior":
            assert np.array_equal(cnt, np.minimum(rank, 9)) and (nbr[rank == 0] == -1).all()
            full = cnt == 9
            assert (rank[nbr[full]] < rank[full][:, None]).all()
        else:
            assert (cnt == 9).all() and (nbr != np.arange(120)[:, None]).all()
        i = int(np.flatnonzero(cnt == 9)[0])
        wrong = nbr.copy()
        wrong[i, 0] = i
        with pytest.raises(AssertionError, match="ineligible"):
            VR.check_lists(spec, X, wrong, cnt, 9, mode, rk)
        wrong = nbr.copy()
        wrong[i] = wrong[i, ::-1]
        with pytest.raises(AssertionError, match="nearest first"):
            VR.check_lists(spec, X, wrong, cnt, 9, mode, rk)
        wrong = nbr.copy()
        wrong[i, 1] = wrong[i, 0]
        with pytest.raises(AssertionError, match="twice"):
            VR.check_lists(spec, X, wrong, cnt, 9, mode, rk)
        short = cnt.copy()
        short[i] = 8
        with pytest.raises(AssertionError, match="cnt"):
            VR.check_lists(spec, X, nbr, short, 9, mode, rk)
    # a duplicate of row i at another row is its first neighbour in LOO mode; ties go to the lower row
    g = np.arange(5.0)
    L = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    L = np.vstack([L, L[12:13]])
    nbr, cnt = VR.brute_lists(LR.make_spec("rbf"), L, 5, "loo")
    assert list(nbr[12]) == [25, 7, 11, 13, 17] and list(nbr[25]) == [12, 7, 11, 13, 17]
    # n = 1: nothing is eligible
    nbr, cnt = VR.brute_lists(LR.make_spec("rbf"), L[:1], 3, "loo")
    assert cnt[0] == 0 and (nbr == -1).all()


def test_vecchia_rank_is_a_reproducible_permutation():
    for n in (1, 2, 1000):
        r = ops.vecchia_rank(n)
        assert r.dtype == np.int32 and r.shape == (n,) and np.array_equal(np.sort(r), np.arange(n))
        assert np.array_equal(r, ops.vecchia_rank(n, seed=0))
        order = np.random.default_rng(0).permutation(n)
        assert np.array_equal(r[order], np.arange(n))                   # the j-th row of the ordering has rank j
    assert not np.array_equal(ops.vecchia_rank(1000, seed=1), ops.vecchia_rank(1000, seed=2))


# ---------------------------------------------------------------------------------------------------------
# ops.gp_local_cond with a stand-in for the library
class FakeLib(object):
    """answers tgp_gp_local_cond with the host reference, writing through the pointers it is given"""

    def __init__(self):
        self.calls = []

    def tgp_gp_local_cond(self, ctx, kref, X, n, y, yerr, mode, rank, kn, nbr_in, mu, var, nbr, cnt, info, sums):
        k = kref._obj
        spec = ops.KernelSpec(k.kind, k.amp, k.a, k.b, k.c, k.ell)

        def arr(p, count, ctype=ctypes.c_double):
            return None if p is None else np.ctypeslib.as_array((ctype * count).from_address(p.value))
        Xa, ya, ea = arr(X, 2 * n).reshape(n, 2), arr(y, n), arr(yerr, n)
        ra, given = arr(rank, n, ctypes.c_int32), arr(nbr_in, n * kn, ctypes.c_int32)
        self.calls.append(dict(n=n, kn=kn, mode=mode, rank=None if ra is None else ra.copy(), given=given is not None,
                               yerr=ea is not None, outs=[p is not None for p in (mu, var, nbr, cnt, info, sums)], spec=spec))
        if given is not None:
            r_nbr = given.reshape(n, kn).copy()
            r_cnt = (r_nbr >= 0).sum(axis=1).astype(np.int32)
        else:
            r_nbr, r_cnt = VR.brute_lists(spec, Xa, kn, "loo" if mode == 0 else "prior", ra)
        r_mu, r_var, r_info = VR.cond_ld(spec, Xa, ya, ea, r_nbr, r_cnt)
        ok = r_info == 0
        t0, t1, _, _ = VR.terms_ld(ya[ok], None if ea is None else ea[ok], r_mu[ok], r_var[ok])
        for p, v, ct in ((mu, r_mu, ctypes.c_double), (var, r_var, ctypes.c_double), (cnt, r_cnt, ctypes.c_int32),
                         (info, r_info, ctypes.c_int32), (nbr, r_nbr.ravel(), ctypes.c_int32),
                         (sums, np.array([t0.sum(), t1.sum(), (~ok).sum()], dtype=np.float64), ctypes.c_double)):
            if p is not None:
                arr(p, len(v), ct)[:] = v
        return 0

    def tgp_last_error(self, ctx):
        return b"stand-in"


@pytest.fixture
def fakelib(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    monkeypatch.setattr(_lib, "get_ctx", lambda device=None: None)
    return lib


def test_ops_plumbing(fakelib):
    spec = LR.make_spec("arbf")
    X, y, y_err, _ = LR.uniform_data(50, 1)
    mu, var, sums = ops.gp_local_cond(spec, X, y, y_err, k=8)
    assert mu.shape == (50,) and var.shape == (50,) and sums.shape == (3,) and sums[2] == 0
    c = fakelib.calls[0]
    assert (c["n"], c["kn"], c["mode"], c["given"], c["yerr"]) == (50, 8, 0, False, True) and c["rank"] is None
    assert c["outs"] == [True, True, False, False, True, True]
    rank = ops.vecchia_rank(50, seed=4)
    mu2, var2, sums2, nbr, cnt = ops.gp_local_cond(spec, X, y, y_err, k=8, mode="prior", rank=rank, return_neighbors=True)
    c = fakelib.calls[1]
    assert c["mode"] == 1 and np.array_equal(c["rank"], rank) and c["outs"] == [True] * 6
    assert nbr.shape == (50, 8) and nbr.dtype == np.int32 and cnt.dtype == np.int32 and np.array_equal(cnt, np.minimum(rank, 8))
    # k is NOT clipped to n: the lists are padded; the default k is 64; int64 ranks are converted
    mu3, var3, sums3, nbr3, cnt3 = ops.gp_local_cond(spec, X, y, y_err, mode="prior", rank=rank.astype(np.int64), return_neighbors=True)
    assert fakelib.calls[-1]["kn"] == 64 and nbr3.shape == (50, 64) and np.array_equal(cnt3, rank)
    ll = -0.5 * sums3[1] - 0.5 * sums3[0] - 25.0 * np.log(2.0 * np.pi)
    ll_dense, _, _ = VR.dense_loglik_ld(LR.kernel_values(spec, X), y, y_err)
    assert abs(ll - float(ll_dense)) <= 1e-10 * (abs(sums3[0]) + abs(sums3[1]) + 50.0)
    # given lists: no mode, no rank reaches the search; the same values come back
    mu4, var4, sums4 = ops.gp_local_cond(spec, X, y, y_err, k=8, neighbors=nbr)
    assert fakelib.calls[-1]["given"] and fakelib.calls[-1]["rank"] is None
    assert np.array_equal(mu4, mu2) and np.array_equal(var4, var2) and np.array_equal(sums4, sums2)
    # no errors given, 1-D coordinates (zero second column)
    ops.gp_local_cond(LR.make_spec("rbf"), X[:, 0], y, None, k=2)
    assert not fakelib.calls[-1]["yerr"] and fakelib.calls[-1]["kn"] == 2


def test_ops_argument_errors(fakelib):
    spec = LR.make_spec("rbf")
    X, y, y_err, _ = LR.uniform_data(20, 1)
    for k in (0, 129, -1, 2.5):
        with pytest.raises(ValueError, match="1 .. 128"):
            ops.gp_local_cond(spec, X, y, y_err, k=k)
    with pytest.raises(ValueError, match="'loo' or 'prior'"):
        ops.gp_local_cond(spec, X, y, y_err, mode="vecchia")
    with pytest.raises(ValueError, match="needs rank"):
        ops.gp_local_cond(spec, X, y, y_err, mode="prior")
    with pytest.raises(ValueError, match="rank 19 values"):
        ops.gp_local_cond(spec, X, y, y_err, mode="prior", rank=np.arange(19))
    with pytest.raises(ValueError, match=r"neighbors must be \(20, 4\)"):
        ops.gp_local_cond(spec, X, y, y_err, k=4, neighbors=np.zeros((20, 5), dtype=np.int32))
    with pytest.raises(ValueError, match="y 19 values"):
        ops.gp_local_cond(spec, X, y[:19], y_err)
    with pytest.raises(ValueError, match="y_err 19 values"):
        ops.gp_local_cond(spec, X, y, y_err[:19])
    with pytest.raises(ValueError, match="only 1-D and 2-D"):
        ops.gp_local_cond(spec, np.zeros((20, 3)), y, y_err)
    with pytest.raises(NotImplementedError, match="sum of kernels"):
        ops.gp_local_cond(ops.KernelSumSpec([spec, spec]), X, y, y_err)
    with pytest.raises(NotImplementedError, match="3-D"):
        ops.gp_local_cond(ops.KernelSpec3(_lib.TGP_RBF), np.zeros((20, 3)), y, y_err)
    with pytest.raises(ValueError, match="KernelSpec"):
        ops.gp_local_cond("RBF(1)", X, y, y_err)
    assert fakelib.calls == []
    fakelib.tgp_gp_local_cond = lambda *a: -1
    with pytest.raises(_lib.TgpError, match="stand-in") as ei:
        ops.gp_local_cond(spec, X, y, y_err)
    assert ei.value.rc == -1


def test_ops_names_the_first_failed_row(fakelib):
    spec = LR.make_spec("rbf")
    X = np.array([[0.5, 0.5], [0.1, 0.0], [0.1, 0.0], [0.9, 0.9], [0.95, 0.9], [0.1, 0.01]])
    y = np.arange(6.0)
    with pytest.raises(np.linalg.LinAlgError, match=r"row 5: the 2-th leading minor") as ei:
        ops.gp_local_cond(spec, X, y, None, k=2, return_neighbors=True)
    assert list(ei.value.info) == [0, 0, 0, 0, 0, 2]
    mu, var, sums, nbr, cnt = ei.value.results
    assert np.isnan(mu[5]) and np.isnan(var[5]) and np.isfinite(mu[:5]).all() and sums[2] == 1 and list(nbr[5]) == [1, 2]


# ---------------------------------------------------------------------------------------------------------
# the object methods with stand-ins for the device
@pytest.fixture
def fake_device(monkeypatch):
    """the ops calls of predict_loo / return_log_likelihood and of the local routes answered on the host; each is recorded"""
    calls = []

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        calls.append("gp_solve")
        K = LR.kernel_values(spec, X)
        alpha, logdet = O.gp_solve(K, np.asarray(y, dtype=float), np.asarray(y_err, dtype=float))

        class Kept(object):
            Kinv = np.linalg.inv(K + np.diag(np.asarray(y_err, dtype=float) ** 2))

            def free(self, keep_memory=False):
                pass
        return alpha, logdet, float(np.dot(y, alpha)), (Kept() if keep else None)

    def factor_inv_diag(factor, ctx=None):
        calls.append("factor_inv_diag")
        return np.diag(factor.Kinv).copy()

    def gp_local_cond(spec, X, y, y_err, k=64, mode="loo", rank=None, neighbors=None, return_neighbors=False, ctx=None):
        X = LR.as_xy(X)
        calls.append(("gp_local_cond", k, mode, X.shape, None if neighbors is None else id(neighbors)))
        if neighbors is None:
            nbr, cnt = VR.brute_lists(spec, X, k, mode, rank)
        else:
            nbr, cnt = neighbors, (np.asarray(neighbors) >= 0).sum(axis=1).astype(np.int32)
        mu, var, info = VR.cond_ld(spec, X, y, y_err, nbr, cnt)
        if info.any():
            raise np.linalg.LinAlgError("row %d" % np.flatnonzero(info)[0])
        t0, t1, _, _ = VR.terms_ld(y, y_err, mu, var)
        out = (mu, var, np.array([t0.sum(), t1.sum(), 0.0], dtype=np.float64))
        return out + ((nbr, cnt) if return_neighbors else ())

    def knn_mean(X0, y0, X, k=4, ctx=None):
        calls.append("knn_mean")
        return O.knn_mean(np.asarray(X0), np.asarray(y0), LR.as_xy(X)[:, :np.shape(X0)[1]], k)

    def forbidden(*a, **k):
        raise AssertionError("the local routes perform no dense factorisation")

    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "factor_inv_diag", factor_inv_diag)
    monkeypatch.setattr(ops, "gp_local_cond", gp_local_cond)
    monkeypatch.setattr(ops, "knn_mean", knn_mean)
    monkeypatch.setattr(ops, "gp_solve_dense", forbidden)
    monkeypatch.setattr(ops, "_dist_engine", lambda n, ctx: None)
    return calls


KERN = "0.8**2 * AnisotropicRBF(invLam=array([[60., -14.], [-14., 35.]]))"


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("table", [False, True])
def test_mean_and_mean_function_are_handled_as_in_predict_loo(fake_device, normalize, table):
    X, y, y_err, _ = LR.uniform_data(60, 1, seed=3)
    y = y + 7.5
    gp = tg.GPInterpolation(kernel=KERN, optimizer="none", normalize=normalize, white_noise=0.02)
    if table:
        rng = np.random.default_rng(1)
        gp._X0, gp._y0 = rng.uniform(size=(30, 2)), 7.0 + rng.standard_normal(30)
    gp.initialize(X, y, y_err=y_err)
    del fake_device[:]
    y_loo, var = gp.predict_loo_local(k=59, return_var=True)
    assert gp._alpha is None and gp._factor is None                      # no solve, nothing cached
    assert [c[:4] for c in fake_device if c != "knn_mean"] == [("gp_local_cond", 59, "loo", (60, 2))]
    ref, ref_var = gp.predict_loo(return_var=True)                       # k >= n - 1: predict_loo
    scale = np.abs(gp._residual()).max()
    assert np.abs(y_loo - ref).max() <= 2e-10 * scale and np.abs(var - ref_var).max() <= 2e-10 * 0.64
    assert "gp_solve" in fake_device
    # the default k, the shapes with the lists, and what is handed down: y - mean - mean function, errors with the white noise
    seen = {}

    def spy(spec, X_, y_, e_, k=64, mode="loo", rank=None, neighbors=None, return_neighbors=False, ctx=None):
        seen.update(y=np.array(y_), e=np.array(e_), k=k, mode=mode)
        n = len(y_)
        return (np.zeros(n), np.ones(n), np.zeros(3)) + ((np.zeros((n, k), dtype=np.int32), np.zeros(n, dtype=np.int32)) if return_neighbors else ())
    ops.gp_local_cond = spy
    out = gp.predict_loo_local()
    np.testing.assert_array_equal(seen["y"], gp._y - gp._mean - gp._spatial_average)
    np.testing.assert_allclose(seen["e"], np.sqrt(y_err ** 2 + 0.02 ** 2))
    assert seen["k"] == 64 and seen["mode"] == "loo"
    np.testing.assert_array_equal(out, gp._mean + gp._spatial_average)
    y2, nbr2, cnt2 = gp.predict_loo_local(k=5, return_neighbors=True)
    assert nbr2.shape == (60, 5) and cnt2.shape == (60,)
    y3, v3, nbr3, cnt3 = gp.predict_loo_local(k=5, return_var=True, return_neighbors=True)
    assert v3.shape == (60,) and nbr3.shape == (60, 5)
    if not normalize:
        assert gp._mean == 0.0


def test_scores_in_their_exact_limits_and_with_theta(fake_device):
    X, y, y_err, _ = LR.uniform_data(50, 1, seed=5)
    gp = tg.GPInterpolation(kernel=KERN, optimizer="none")
    gp.initialize(X, y, y_err=y_err)
    ll = gp.return_log_likelihood_local(k=128)                            # k >= n - 1: the dense likelihood
    ll_dense = gp.return_log_likelihood()
    assert abs(ll - ll_dense) <= 1e-10 * (abs(ll_dense) + 50.0)
    loo = gp.return_loo_log_predictive_local(k=49)
    assert abs(loo - gp.return_loo_log_predictive()) <= 1e-9 * (abs(loo) + 50.0)
    # fewer neighbours: another number, and one that depends on the seed of the ordering; theta is honoured
    a, b = gp.return_log_likelihood_local(k=4), gp.return_log_likelihood_local(k=4, seed=1)
    assert a != ll and a != b and np.isfinite(a) and np.isfinite(b)
    theta = gp.kernel.theta + 0.1
    assert gp.return_log_likelihood_local(theta=theta, k=4) != a
    assert gp.return_loo_log_predictive_local(theta=theta, k=4) != gp.return_loo_log_predictive_local(k=4)
    assert np.array_equal(gp.kernel.theta, theta - 0.1)
    # a failed row is -inf, as log_likelihood's

    def failing(*a, **k):
        raise np.linalg.LinAlgError("row 3")
    ops.gp_local_cond = failing
    assert gp.return_log_likelihood_local() == -np.inf and gp.return_loo_log_predictive_local() == -np.inf


def test_local_likelihood_fit_searches_once(fake_device):
    rng = np.random.default_rng(12)
    X = rng.uniform(size=(150, 2))
    K = LR.kernel_values(LR.make_spec("rbf", amp=1.0, a=1.0 / 0.2 ** 2, c=1.0 / 0.2 ** 2), X)
    y = np.linalg.cholesky(K + 1e-10 * np.eye(150)).dot(rng.standard_normal(150)) + 0.05 * rng.standard_normal(150)
    y_err = np.full(150, 0.05)
    gp = tg.GPInterpolation(kernel="0.5**2 * RBF(0.4)", optimizer="local-likelihood", normalize=False, local_k=12, local_seed=2)
    gp.initialize(X, y, y_err=y_err)
    start = gp.return_log_likelihood_local(k=12, seed=2)
    del fake_device[:]
    gp.solve()
    cond = [c for c in fake_device if c[0] == "gp_local_cond"]
    assert cond[0][4] is None and all(c[1:3] == (12, "prior") for c in cond)           # one search ...
    assert len(cond) > 4 and len({c[4] for c in cond[1:]}) == 1 and cond[1][4] is not None   # ... then one list for every evaluation
    assert "gp_solve" not in fake_device
    assert gp._optimizer._logL > start and np.isfinite(gp._optimizer._logL)
    assert np.array_equal(gp._optimizer.rank, ops.vecchia_rank(150, seed=2))
    assert abs(np.exp(gp.kernel.theta[-1]) - 0.2) < 0.1                                 # the length the field was drawn with


def test_defaults_change_nothing_for_the_other_optimisers():
    gp = tg.GPInterpolation(kernel="RBF(1)", optimizer="none")
    assert gp.local_k == 64 and gp.local_seed == 0
    with pytest.raises(ValueError, match="local-likelihood"):
        tg.GPInterpolation(kernel="RBF(1)", optimizer="vecchia")


def test_refusals(fake_device):
    X, y, y_err, _ = LR.uniform_data(20, 1)
    methods = (lambda g: g.predict_loo_local(), lambda g: g.return_loo_log_predictive_local(), lambda g: g.return_log_likelihood_local())
    for kern in ("0.7**2 * RBF(0.2) + WhiteKernel(0.01)", "0.7**2 * Matern(0.2, nu=1.5)"):
        gp = tg.GPInterpolation(kernel=kern, optimizer="none")
        gp.initialize(X, y, y_err=y_err)
        for m in methods:
            with pytest.raises(NotImplementedError, match="dense route"):
                m(gp)
        gp.optimizer = "local-likelihood"
        with pytest.raises(NotImplementedError, match="dense route"):
            gp.solve()
    gp = tg.GPInterpolation(kernel="0.3**2 * RBF(0.2) + 0.5**2 * RBF(0.7)", optimizer="local-likelihood")
    gp.initialize(X, y, y_err=y_err)
    for m in methods + (lambda g: g.solve(),):
        with pytest.raises(NotImplementedError, match="sum of kernels"):
            m(gp)
    X3 = np.random.default_rng(2).uniform(size=(20, 3))
    gp = tg.GPInterpolation(kernel="0.8**2 * RBF([0.2, 0.3, 0.5])", optimizer="local-likelihood")
    gp.initialize(X3, y, y_err=y_err)
    for m in methods + (lambda g: g.solve(),):
        with pytest.raises(NotImplementedError, match="3-D"):
            m(gp)
    assert fake_device == []


# ---------------------------------------------------------------------------------------------------------
# the host checks, under sanitizers
def test_host_checks_under_sanitizers(tmp_path):
    """tests/sanitize/local_cond_driver.cpp: the rank check, the list check and the ranks-into-cell-order step of
    treegp_amd/csrc/local_grid.h compiled alone with AddressSanitizer + UBSan and driven in exact-size buffers."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    assert cxx is not None, "no clang++ found next to hipcc"
    exe = str(tmp_path / "local_cond_driver")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "local_cond_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "local conditionals ok under sanitizers" in r.stdout

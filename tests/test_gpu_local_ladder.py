"""The local routes (local kriging and the local conditionals: local_solve_kernel of treegp_amd/csrc/local.hip, the only
factorisation of the library that is not potrf128) up the condition ladder, cond_2(K_S) = 2.6e3 ... 8e10, against the long-double
truth of tests/_local_ladder_refs.py and beside what LAPACK achieves on the same local matrices.

test_gpu_local.py and test_gpu_vecchia.py work at cond(K_S) <= 5.2e4 and accept |dvar| <= 1e-10 amp; from rung 3 up the true
variance itself is 1e-9 ... 1e-8 amp, and the Vecchia likelihood sees the RELATIVE error of s2 = var + yerr^2.

Bounds (none of them taken from device output): every figure -- mu / max|y|, var / amp, and for the conditionals
|d log s2| and |d r^2/s2| / max r^2/s2 formed on the host in long double from the device's mu and var -- is held to
16 x max(LAPACK's figure on the same lists, 2^-53) (_local_ladder_refs.bound_u).  Values are compared ON THE LISTS THE DEVICE
RETURNED, after those lists have been checked as test_gpu_local.py and test_gpu_vecchia.py check them.  A (route, rung, figure)
that misses is named in EXCEPTIONS with twice the ratio measured on an MI355X, as in test_gpu_cond_ladder.py.  Every case prints
one LADDER line per figure (-s); LAB_NOTES.md, "Condition ladder", has the table."""
import numpy as np
import pytest

import _cond_ladder as CL
import _local_ladder_refs as R
import _local_refs as LR
import _vecchia_refs as VR
from test_local_ladder_host import COND_LOCAL, COND_SHEAR_3

pytestmark = pytest.mark.gpu

LD = np.longdouble
N = R.N

# (route, rung, figure) -> the multiple of max(LAPACK's figure, u) the route is held to instead of 16: twice the ratio measured on
# an MI355X (LAB_NOTES.md, "Condition ladder", has the figures).  No local route needs an entry: local_solve_kernel is within
# 0.2 - 11 x LAPACK on every rung and figure (median 0.9).  Every entry is the DENSE side of the patch comparison: gp_solve +
# gp_predict + gp_predict_var on 128 points is one 128-block, and its sweeps and its substitution multiply by the explicit
# inverse W of that block, whose condition number is sqrt(cond K_S): conditionally stable only, as test_gpu_cond_ladder.py says
# of every dense route.  At n = 2304 LAPACK's own error hides it; on one correlated patch, where LAPACK's v.w and amp - v.v stay
# at a few u, it shows.  A numpy model (W = L^-1 by substitution, alpha = W^T (W y), var = amp - |W k*|^2; printed by
# test_local_ladder_host.py) gives the same figures: 1.9e-12 / 2.0e-10 / 1.4e-09 / 2.0e-08 for mu and 1.1e-14 / 6.0e-14 /
# 3.6e-13 / 1.2e-12 for var on rungs 1 ... 4.  The remedy is the one the inverse slabs have on record (one residual correction
# per block, z += W (b - L z)); it changes the bits of every dense route and was not built.
EXCEPTIONS = {
    ("patch/dense", 1, "mu"): 35,       # measured 17.5 x: device 3.12e-12, LAPACK 1.79e-13
    ("patch/dense", 1, "var"): 67,      # measured 33.2 x: device 1.04e-14, LAPACK 3.12e-16
    ("patch/dense", 2, "mu"): 79,       # measured 39.1 x: device 8.81e-11, LAPACK 2.26e-12
    ("patch/dense", 2, "var"): 126,     # measured 62.6 x: device 7.28e-14, LAPACK 1.16e-15
    ("patch/dense", 3, "mu"): 204,      # measured 101.8 x: device 3.09e-09, LAPACK 3.04e-11
    ("patch/dense", 3, "var"): 350,     # measured 174.6 x: device 1.74e-13, LAPACK 9.96e-16
    ("patch/dense", 4, "mu"): 290,      # measured 144.8 x: device 1.67e-08, LAPACK 1.16e-10
    ("patch/dense", 4, "var"): 558,     # measured 278.6 x: device 5.78e-13, LAPACK 2.08e-15
}


@pytest.fixture(scope="module")
def ops():
    from treegp_amd import ops
    assert np.array_equal(ops.vecchia_rank(N, 0), R.vecchia_rank())
    return ops


def judge(route, i, cond, dev, lap):
    for what in dev:
        assert np.isfinite(dev[what]), (route, i, what)
    bad = R.judge(route, i, cond, dev, lap, EXCEPTIONS)
    assert not bad, "\n".join(bad)


# ---- local kriging at the 256 queries --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("i", CL.RUNGS)
def test_predict_local(ops, i, k):
    X, y, e = R.rung_data(i)
    Xq = CL.queries()
    ys, var, nbr = ops.gp_predict_local(R.spec(), X, y, e, Xq, k=k, return_var=True, return_neighbors=True)
    LR.check_neighbor_sets(R.spec(), X, Xq, nbr, D=R.tables()["Dq"])
    c = R.predict_case_on(i, k, nbr)
    judge("predict_local/%d" % k, i, COND_LOCAL[k][i], c.figures(ys, var), c.lapack)


# ---- the conditionals: local leave-one-out and the Vecchia terms ----------------------------------------------------------------

def cond_figures(ops, route, i, k, mode, cond, name="rbf"):
    """gp_local_cond on the brute-force lists and with the search; the four figures on the sampled rows, info and the sums"""
    X, y, e = R.rung_data(i)
    sp, rows = R.spec(name), R.sample_rows()
    rank = R.vecchia_rank() if mode == "prior" else None
    b_nbr, b_cnt = R.brute_lists(name, k, mode)
    given = ops.gp_local_cond(sp, X, y, e, k=k, neighbors=b_nbr, return_neighbors=True)      # (raises if any info is not zero)
    assert np.array_equal(given[3], b_nbr) and np.array_equal(given[4], b_cnt)
    found = ops.gp_local_cond(sp, X, y, e, k=k, mode=mode, rank=rank, return_neighbors=True)
    VR.check_lists(sp, X, found[3], found[4], k, mode, rank, D=R.tables(name)["D"])
    for tag, (mu, var, sums, nbr, cnt) in (("given", given), ("search", found)):
        assert mu.shape == (N,) and np.isfinite(mu).all() and np.isfinite(var).all()
        c = R.cond_case_on(i, k, mode, nbr[rows], cnt[rows], name)
        judge("%s/%s" % (route, tag), i, cond, c.figures(mu[rows], var[rows]), c.lapack)
        VR.check_sums(y, e, mu, var, sums, "%s/%s rung %d" % (route, tag, i))
    if mode == "prior":
        first = int(np.argmin(R.vecchia_rank()))
        assert found[4][first] == 0 and found[0][first] == 0.0 and found[1][first] == sp.amp


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("i", CL.RUNGS)
def test_local_cond(ops, i, k, mode):
    cond_figures(ops, "local_cond/%s/%d" % (mode, k), i, k, mode, COND_LOCAL[k][i])


# ---- the exact limits on a dense patch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", CL.RUNGS)
def test_exact_limit_on_a_dense_patch(ops, i):
    """The 129 ladder points nearest (0.5, 0.5), k = 128: the prior conditionals under the identity ranking are the dense
    log-likelihood, and local kriging on the first 128 points is the exact GP -- which ties the LDS factorisation to potrf128
    (gp_solve + gp_predict + gp_predict_var on the same 128 points) where both are stressed."""
    p, sp = R.patch_case(i), R.spec()
    n = R.NPATCH
    rank = np.arange(n, dtype=np.int32)
    mu, var, sums, nbr, cnt = ops.gp_local_cond(sp, p.X, p.y, p.e, k=128, mode="prior", rank=rank, return_neighbors=True)
    assert np.array_equal(cnt, rank)                                               # every predecessor
    assert all(sorted(nbr[r, :r]) == list(range(r)) for r in range(n))
    ll = -LD(0.5) * LD(sums[1]) - LD(0.5) * LD(sums[0]) - LD(0.5) * n * VR.LOG_2PI
    err = abs(float(ll - p.ll_t))
    print(CL.line("patch/loglik", i, COND_LOCAL[128][i], "logL", err, p.ll_err_lapack)
          + "   (log L %.6f, floor u |log L| = %.2e)" % (float(p.ll_t), R.U * abs(float(p.ll_t))))
    assert err <= p.ll_bound
    k = n - 1
    X, y, e = p.X[:k], p.y[:k], p.e[:k]
    ys, v_local, nbr = ops.gp_predict_local(sp, X, y, e, p.Xq, k=k, return_var=True, return_neighbors=True)
    assert (np.sort(nbr, axis=1) == np.arange(k)).all()
    alpha, _, _, fac = ops.gp_solve(sp, X, y, e, keep=True)
    try:
        yd, v_dense = ops.gp_predict(sp, X, alpha, p.Xq), ops.gp_predict_var(sp, fac, X, p.Xq)
    finally:
        fac.free()
    bad = R.judge("patch/predict_local", i, COND_LOCAL[128][i], p.figures(ys, v_local), p.lapack, EXCEPTIONS)
    bad += R.judge("patch/dense", i, COND_LOCAL[128][i], p.figures(yd, v_dense), p.lapack, EXCEPTIONS)
    assert not bad, "\n".join(bad)


# ---- a sheared kernel ------------------------------------------------------------------------------------------------------------

def test_sheared_kernel_rung_3(ops):
    """AnisotropicRBF with invLam [[60, -14], [-14, 35]] at noise 1e-4: the 128 neighbours lie within a correlation ellipse and the
    median cond_2(K_S) is 9e9 (test_local_ladder_host.py)"""
    i, k, sp = 3, 128, R.spec("shear")
    X, y, e = R.rung_data(i)
    Xq = CL.queries()
    ys, var, nbr = ops.gp_predict_local(sp, X, y, e, Xq, k=k, return_var=True, return_neighbors=True)
    LR.check_neighbor_sets(sp, X, Xq, nbr, D=R.tables("shear")["Dq"])
    c = R.predict_case_on(i, k, nbr, "shear")
    judge("shear/predict_local/%d" % k, i, COND_SHEAR_3, c.figures(ys, var), c.lapack)
    cond_figures(ops, "shear/local_cond/loo/%d" % k, i, k, "loo", COND_SHEAR_3, name="shear")


# ---- through the object ------------------------------------------------------------------------------------------------------------

def test_api_rung_3(ops):
    """GPInterpolation(normalize=True) on rung 3 with the field shifted by 3: the truth of the residual, pushed through the
    object's mean handling (the mean is added to LAPACK's answer in fp64 as it is to the device's)"""
    import treegp_amd as tg
    i, k = 3, 33
    X, y, e = R.rung_data(i)
    y3 = y + 3.0
    gp = tg.GPInterpolation(kernel="1.0**2 * RBF(0.1)", optimizer="none", normalize=True)
    gp.initialize(X, y3, y_err=e)
    mean = np.mean(y3)
    res = y3 - mean - 0.0
    assert gp._mean == mean and np.array_equal(gp._residual(), res)
    sp = gp._local_spec("test")
    assert (sp.kind, sp.amp, sp.a, sp.b, sp.c) == (R.spec().kind, 1.0, CL.KW["a"], 0.0, CL.KW["c"])
    T, rows = R.tables(), R.sample_rows()
    yscale = float(np.abs(res).max())

    def shifted(case):
        """LAPACK's figures with the mean added in fp64, and a function giving a candidate's figures against truth + mean"""
        mu_t = case.mu_t + LD(mean)
        fig = lambda mu, var: R.figures(mu, var, mu_t, case.var_t, yscale, R.AMP, None if case.y is None else case.y + LD(mean), case.e)
        return fig, fig(case.mu_l + mean, case.var_l)

    # predict_local at the 256 queries
    Xq = CL.queries()
    ys, var, nbr = gp.predict_local(Xq, k=k, return_var=True, return_neighbors=True)
    LR.check_neighbor_sets(sp, X, Xq, nbr, D=T["Dq"])
    fig, lap = shifted(R.Case("rbf", res, e, nbr, np.full(len(nbr), k, dtype=np.int32)))
    judge("api/predict_local/%d" % k, i, COND_LOCAL[k][i], fig(ys, var), lap)
    # predict_loo_local on the sampled rows
    y_loo, var, nbr, cnt = gp.predict_loo_local(k=k, return_var=True, return_neighbors=True)
    VR.check_lists(sp, X, nbr, cnt, k, "loo", D=T["D"])
    fig, lap = shifted(R.Case("rbf", res, e, nbr[rows], cnt[rows], rows=rows))
    judge("api/predict_loo_local/%d" % k, i, COND_LOCAL[k][i], fig(y_loo[rows], var[rows]), lap)
    # the Vecchia likelihood over all 2304 rows, on the lists the search returns for this call's arguments
    rank = R.vecchia_rank()
    nbr, cnt = ops.gp_local_cond(sp, X, res, e, k=k, mode="prior", rank=rank, return_neighbors=True)[3:]
    VR.check_lists(sp, X, nbr, cnt, k, "prior", rank, D=T["D"])
    every = np.arange(N)
    case = R.Case("rbf", res, e, nbr, cnt, rows=every)
    l_t, c_t, _ = R.terms(res, e, case.mu_t, case.var_t)
    ll_t = -LD(0.5) * c_t.sum() - LD(0.5) * l_t.sum() - LD(0.5) * N * VR.LOG_2PI
    s2 = case.var_l + e ** 2                                                       # LAPACK's: the terms and their sum in fp64
    ll_l = -0.5 * np.sum((res - case.mu_l) ** 2 / s2) - 0.5 * np.sum(np.log(s2)) - 0.5 * N * np.log(2.0 * np.pi)
    lap = abs(float(LD(ll_l) - ll_t))
    dev = abs(float(LD(gp.return_log_likelihood_local(k=k, seed=0)) - ll_t))
    print(CL.line("api/log_likelihood_local/%d" % k, i, COND_LOCAL[k][i], "logL", dev, lap)
          + "   (log L %.6f, floor u |log L| = %.2e)" % (float(ll_t), R.U * abs(float(ll_t))))
    assert dev <= 16.0 * max(lap, R.U * abs(float(ll_t)))


# ---- no noise at all ---------------------------------------------------------------------------------------------------------------

def _outcome(call):
    try:
        out = call()
        return out, np.zeros(len(out[0]), dtype=np.int32)
    except np.linalg.LinAlgError as ex:
        return ex.results, ex.info


@pytest.mark.parametrize("k", [33, 128])
def test_no_noise_is_reported_not_invented(ops, k):
    """y_err = None: the local matrices are worse conditioned than the whole ladder, and some are not positive definite in fp64.  A
    non-positive pivot is an ordinary return value: every row is either reported (info > 0, NaN) or answered (info = 0, finite),
    and the sums count exactly the reported rows.  Which rows LAPACK factors too is printed and not asserted: at the edge of
    definiteness two correct solvers may differ."""
    X, y, _ = R.rung_data(2)
    sp, T, zero = R.spec(), R.tables(), np.zeros(N)
    Xq = CL.queries()
    (ys, var, nbr), info = _outcome(lambda: ops.gp_predict_local(sp, X, y, None, Xq, k=k, return_var=True, return_neighbors=True))
    failed = info > 0
    assert (info >= 0).all() and (info <= k).all()
    assert np.isnan(ys[failed]).all() and np.isnan(var[failed]).all()
    assert np.isfinite(ys[~failed]).all() and np.isfinite(var[~failed]).all()
    _, _, piv = R.lapack_on_lists(R.AMP, y, zero, nbr, np.full(len(nbr), k), T["K"], T["Kq"])
    print("no noise k %d predict_local: %d of %d queries reported; LAPACK factors %d, both factor %d"
          % (k, failed.sum(), len(info), (piv > 0).sum(), (~failed & (piv > 0)).sum()))
    for mode in R.MODES:
        rank = R.vecchia_rank() if mode == "prior" else None
        (mu, var, sums, nbr, cnt), info = _outcome(
            lambda: ops.gp_local_cond(sp, X, y, None, k=k, mode=mode, rank=rank, return_neighbors=True))
        failed = info > 0
        assert (info >= 0).all() and (info <= cnt).all()
        assert np.isnan(mu[failed]).all() and np.isnan(var[failed]).all()
        assert np.isfinite(mu[~failed]).all() and np.isfinite(var[~failed]).all()
        assert sums[2] == float(failed.sum())
        rows = R.sample_rows()
        _, _, piv = R.lapack_on_lists(R.AMP, y, zero, nbr[rows], cnt[rows], T["K"], T["K"][rows])
        print("no noise k %d %s: %d of %d rows reported, %d answered with var <= 0; of the 256 sampled rows LAPACK factors %d, the "
              "device %d, both %d" % (k, mode, failed.sum(), N, (var[~failed] <= 0).sum(), (piv > 0).sum(), (~failed[rows]).sum(),
                                      (~failed[rows] & (piv > 0)).sum()))

"""The yardstick of test_gpu_local_ladder.py, pinned on the host from the references of tests/_local_ladder_refs.py alone: the
local matrices reach the condition numbers the GPU tests claim to cover, the long-double truth is valid (against mpmath at 40
digits), s2 is large enough beside LAPACK's variance error for its logarithm to be a fair figure, LAPACK factors every local
matrix, and a numpy fp64 model of local_solve_kernel's order of operations meets the bound the device is held to.  LAPACK's and the
model's figures per rung are printed (-s)."""
import numpy as np
import pytest

import _cond_ladder as CL
import _local_ladder_refs as R

# median cond_2 of the local matrices of the 256 sampled rows (leave-one-out lists), per rung, k = 32, 33, 128: measured with
# numpy's eigvalsh on the oracle's fp64 kernel values; held to a factor 2 as COND_2304 is in test_cond_ladder_host.py
COND_LOCAL = {
    32: (2.6e3, 2.6e5, 2.6e7, 2.6e9, 2.9e10),
    33: (2.7e3, 2.7e5, 2.7e7, 2.7e9, 3.0e10),
    128: (6.6e3, 6.6e5, 6.6e7, 6.6e9, 7.4e10),
}
COND_SHEAR_3 = 9.1e9            # the sheared kernel, rung 3, k = 128


def test_sampled_rows():
    rows, rank = R.sample_rows(), R.vecchia_rank()
    assert len(rows) == R.NROWS == len(set(rows)) and rows[0] == 0 and rows[-1] == R.N - 1
    assert int(np.argmin(rank)) in rows and int(np.argmax(rank)) in rows
    assert sorted(rank) == list(range(R.N))


@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("i", CL.RUNGS)
def test_local_matrices_reach_their_condition_numbers(i, k):
    med = float(np.median(R.local_cond2("rbf", i, k)))
    k_eff = COND_LOCAL[k][0] * CL.NOISES[0] ** 2 / CL.AMP          # the well-conditioned rung's cond x e^2 / amp
    print("rung %d k %3d median cond_2(K_S) %.3e (recorded %.1e; k_eff amp / e^2 = %.1e, k_eff = %.0f)"
          % (i, k, med, COND_LOCAL[k][i], k_eff * CL.AMP / CL.NOISES[i] ** 2, k_eff))
    assert COND_LOCAL[k][i] / 2 <= med <= COND_LOCAL[k][i] * 2
    assert 1.0 <= k_eff <= k and 0.5 <= med * CL.NOISES[i] ** 2 / (k_eff * CL.AMP) <= 2.0


def test_sheared_kernel_is_ill_conditioned_within_a_correlation_ellipse():
    med = float(np.median(R.local_cond2("shear", 3, 128)))
    nbr, cnt = R.brute_lists("shear", 128, "loo")
    rows = R.sample_rows()
    far = R.tables("shear")["D"][rows, nbr[rows, 127]]               # d^T invLam d of each row's farthest neighbour
    print("sheared kernel rung 3 k 128: median cond_2 %.3e, median farthest neighbour at d^T invLam d = %.3f" % (med, np.median(far)))
    assert med >= 1e9 and COND_SHEAR_3 / 2 <= med <= COND_SHEAR_3 * 2
    assert np.median(far) <= 1.0


def _mp_row(case, t, y, e, name="rbf"):
    """mu and var of row t of a conditional case by mpmath at 40 digits: kernel values, mp.cholesky and substitution"""
    import mpmath as mp
    mp.mp.dps = 40
    sp = R.spec(name)
    X = CL.points(R.N)[0]
    S = [int(r) for r in case.nbr[t, :case.cnt[t]]]
    pts = [(mp.mpf(float(X[r, 0])), mp.mpf(float(X[r, 1]))) for r in S]
    q0 = (mp.mpf(float(X[case.rows[t], 0])), mp.mpf(float(X[case.rows[t], 1])))
    a, b, c, amp = mp.mpf(sp.a), mp.mpf(sp.b), mp.mpf(sp.c), mp.mpf(sp.amp)

    def kv(p, q):
        dx, dy = p[0] - q[0], p[1] - q[1]
        return amp * mp.exp(-(a * dx * dx + 2 * b * dx * dy + c * dy * dy) / 2)
    k = len(S)
    A = mp.matrix(k, k)
    for u in range(k):
        for v in range(u):
            A[u, v] = A[v, u] = kv(pts[u], pts[v])
        A[u, u] = amp + mp.mpf(float(e[S[u]])) ** 2
    L = mp.cholesky(A)

    def forward(b):
        x = []
        for u in range(k):
            x.append((b[u] - sum(L[u, p] * x[p] for p in range(u))) / L[u, u])
        return x
    v = forward([kv(q0, p) for p in pts])
    w = forward([mp.mpf(float(y[r])) for r in S])
    return sum(v[u] * w[u] for u in range(k)), amp - sum(v[u] * v[u] for u in range(k))


def _mpf(x):
    """a long double as an mpf, exactly: its fp64 head and what is left"""
    import mpmath as mp
    head = float(x)
    return mp.mpf(head) + mp.mpf(float(x - R.LD(head)))


def test_the_truth_is_valid_against_mpmath():
    """4 rows of rung 4 at k = 128: the long-double truth lies within 1e-2 of LAPACK's error of the 40-digit answer"""
    import mpmath as mp
    case = R.cond_case(4, 128, "loo")
    _, y, e = R.rung_data(4)
    e_mu_t = e_var_t = 0.0
    for t in (0, 85, 170, 255):
        mu, var = _mp_row(case, t, y, e)
        e_mu_t = max(e_mu_t, float(abs(_mpf(case.mu_t[t]) - mu)) / case.yscale)
        e_var_t = max(e_var_t, float(abs(_mpf(case.var_t[t]) - var)) / R.AMP)
    print("rung 4 k 128: truth against mpmath |dmu| %.2e (LAPACK %.2e), |dvar| %.2e (LAPACK %.2e)"
          % (e_mu_t, case.lapack["mu"], e_var_t, case.lapack["var"]))
    assert e_mu_t <= 1e-2 * case.lapack["mu"] and e_var_t <= 1e-2 * case.lapack["var"]


def _cases(i):
    for k in R.KS:
        yield "predict/%d" % k, R.predict_case(i, k)
        for mode in R.MODES:
            yield "%s/%d" % (mode, k), R.cond_case(i, k, mode)
    if i == 3:
        yield "shear-predict/128", R.predict_case(3, 128, "shear")
        yield "shear-loo/128", R.cond_case(3, 128, "loo", "shear")


@pytest.mark.parametrize("i", CL.RUNGS)
def test_the_logarithm_is_a_fair_figure_and_the_model_meets_the_bound(i):
    """On every rung and row s2_true >= 1e3 x LAPACK's |dvar| and no pivot of LAPACK's factor is non-positive (else the inputs
    are wrong, not the device); the fp64 model of the kernel meets bound_u on every figure, so the bound is attainable.  The
    model's ratios are printed, and are no expectation of the device."""
    bad = []
    for route, c in _cases(i):
        assert (c.piv_l > 0.0).all() and np.isfinite(c.var_l).all(), route
        dvar = np.abs(np.asarray(c.var_l, dtype=R.LD) - c.var_t)
        margin = float((c.s2_true() / np.maximum(dvar, R.LD(1e-300))).min())
        print("rung %d %-18s min s2_true %.2e, smallest s2_true / LAPACK |dvar| %.2e" % (i, route, float(c.s2_true().min()), margin))
        assert margin >= 1e3, route
        mu, var, info = c.model()
        assert not info.any(), route
        bad += R.judge("model/" + route, i, COND_LOCAL[int(route.split("/")[1])][i], c.figures(mu, var), c.lapack)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("i", CL.RUNGS)
def test_dense_patch_references(i):
    p = R.patch_case(i)
    assert len(p.X) == R.NPATCH and np.hypot(*(p.Xq - 0.5).T).max() <= np.hypot(*(p.X - 0.5).T).max()
    print("rung %d patch: log L %.6f, LAPACK's error %.2e, bound %.2e; LAPACK mu %.2e var %.2e"
          % (i, float(p.ll_t), p.ll_err_lapack, p.ll_bound, p.lapack["mu"], p.lapack["var"]))
    print("   products with an explicit inverse of L (a model of the dense route on one 128-block): mu %.2e var %.2e"
          % (p.explicit_inverse["mu"], p.explicit_inverse["var"]))
    assert np.isfinite(p.ll_l) and p.ll_bound >= 16.0 * R.U * abs(float(p.ll_t))

"""GPU tests of leave-group-out cross-validation (seam S3h, tgp_factor_inv_blocks, and GPInterpolation.predict_lgo /
return_lgo_log_predictive): the diagonal blocks of K^-1 against the oracle's inverse, against the row norms of seam S3e,
independence of the chunk, the route and the other groups bit for bit, the argument errors, and the predictions against
deleting each group and solving again."""
import functools
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
from test_gpu_loo import _gp, _oracle_kernel, _problem, _spec  # noqa: E402  (the leave-one-out tests' kinds and problems)

pytestmark = pytest.mark.gpu

# the smallest shapes that reach every edge of the kernel: one point; groups of 1, 127 and 1 around a tile edge; sizes 1 and
# exactly 128, a group across a tile edge (130 .. 257), a panel edge (257 .. 300 starts one row into a panel) and the
# 1024-column step (1023 .. 1025); one group of many tiles; many groups that never line up with a tile
SHAPES = {
    "one": (1, [0, 1]),
    "tile_edge": (129, [0, 1, 128, 129]),
    "ragged": (1300, [0, 1, 2, 130, 257, 300, 1023, 1025, 1300]),
    "one_group": (3000, [0, 3000]),
    "by_127": (3000, list(range(0, 3000, 127)) + [3000]),
}


@functools.lru_cache(maxsize=None)
def _oracle_inverse(tag, n):
    """(X, y, e, inverse of the oracle's K + diag(e^2)), computed once per kind and size and never written to"""
    from oracle import gp_oracle as O
    _, kind, kw = _spec(tag)
    _, X, y, e = _problem(n, 2000 + n)
    ref = np.linalg.inv(O.kernel_matrix(kind, X, **kw) + np.diag(e ** 2))
    for a in (X, y, e, ref):
        a.setflags(write=False)
    return X, y, e, ref


def _slices(starts):
    return [slice(s, e) for s, e in zip(starts[:-1], starts[1:])]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("tag", ["rbf", "arbf", "vk", "avk"])
def test_blocks_against_oracle_inverse(tag, shape):
    from treegp_amd import ops
    n, starts = SHAPES[shape]
    X, y, e, ref = _oracle_inverse(tag, n)
    fac = ops.gp_solve(_spec(tag)[0], X, y, e, keep=True)[3]
    blocks = ops.factor_inv_blocks(fac, np.array(starts))
    fac.free()
    assert len(blocks) == len(starts) - 1
    worst = 0.0
    for g, sl in enumerate(_slices(starts)):
        B = blocks[g]
        assert B.shape == (sl.stop - sl.start,) * 2
        assert np.array_equal(B, B.T), "block %d is not symmetric bit for bit" % g
        d = np.sqrt(np.diag(ref)[sl])
        worst = max(worst, np.max(np.abs(B - ref[sl, sl]) / np.outer(d, d)))
    print("%s %s: largest |block - ref| / sqrt(ref_ii ref_jj) = %.3e" % (tag, shape, worst))
    assert worst <= 1e-9


def test_block_diagonals_agree_with_the_row_norms():
    from treegp_amd import ops
    n = 1300
    _, X, y, e = _problem(n, 77)
    fac = ops.gp_solve(_spec("avk")[0], X, y, e, keep=True)[3]
    d = ops.factor_inv_diag(fac)
    ones = ops.factor_inv_blocks(fac, np.arange(n + 1))
    assert all(b.shape == (1, 1) for b in ones)
    np.testing.assert_allclose(np.array([b[0, 0] for b in ones]), d, rtol=1e-12, atol=0)
    starts = np.array(list(range(0, n, 200)) + [n])
    by200 = ops.factor_inv_blocks(fac, starts)
    np.testing.assert_allclose(np.concatenate([np.diag(b) for b in by200]), d, rtol=1e-12, atol=0)
    fac.free()


def test_blocks_depend_neither_on_the_chunk_nor_on_the_route_nor_on_the_other_groups(monkeypatch):
    from treegp_amd import ops
    _, X, y, e = _problem(5000, 11)                            # several chunks, n not a multiple of 256
    fac = ops.gp_solve(_spec("avk")[0], X, y, e, keep=True)[3]
    # ragged groups; 1023 .. 1290 starts one row below the 1024-step, 1290 .. 2790 holds 1500 rows
    starts = np.array([0, 7, 300, 1023, 1290, 2790, 2800, 3333, 4096, 4777, 5000])
    monkeypatch.delenv("TGP_INVDIAG_CHUNK", raising=False)
    monkeypatch.delenv("TGP_COV_BIG", raising=False)
    default = ops.factor_inv_blocks(fac, starts)
    for chunk in ("2048", "3000"):
        monkeypatch.setenv("TGP_INVDIAG_CHUNK", chunk)
        got = ops.factor_inv_blocks(fac, starts)
        assert all(np.array_equal(a, b) for a, b in zip(got, default)), chunk
    # the same two blocks with their neighbours merged and split differently (smaller groups: smaller chunks as well)
    other = np.array([0, 300, 1023, 1290, 2000, 2790, 3333, 4096, 5000])
    monkeypatch.setenv("TGP_INVDIAG_CHUNK", "2048")
    got = ops.factor_inv_blocks(fac, other)
    assert np.array_equal(got[2], default[3])                   # 1023 .. 1290
    assert np.array_equal(got[6], default[7])                   # 3333 .. 4096
    monkeypatch.delenv("TGP_INVDIAG_CHUNK")
    got = ops.factor_inv_blocks(fac, other)
    assert np.array_equal(got[2], default[3]) and np.array_equal(got[6], default[7])
    # the 128-block substitution (chunks on a 256 grid)
    monkeypatch.setenv("TGP_COV_BIG", "0")
    small = ops.factor_inv_blocks(fac, starts)
    monkeypatch.setenv("TGP_INVDIAG_CHUNK", "768")
    small_c = ops.factor_inv_blocks(fac, starts)
    for a, b, c in zip(small, default, small_c):
        d = np.sqrt(np.diag(b))
        assert np.max(np.abs(a - b) / np.outer(d, d)) <= 1e-12
        assert np.array_equal(a, c)
    fac.free()


def test_argument_errors_name_the_entry_and_leave_the_factor_usable():
    from treegp_amd import ops
    from treegp_amd._lib import TgpError
    n = 4200
    _, X, y, e = _problem(n, 5)
    fac = ops.gp_solve(_spec("rbf")[0], X, y, e, keep=True)[3]
    with pytest.raises(TgpError, match=r"starts\[2\] = 100 is not above starts\[1\] = 100"):
        ops.factor_inv_blocks(fac, np.array([0, 100, 100, n]))
    with pytest.raises(TgpError, match=r"starts\[3\] = 90 is not above starts\[2\] = 200"):
        ops.factor_inv_blocks(fac, np.array([0, 100, 200, 90, n]))
    with pytest.raises(TgpError, match=r"starts\[0\] = 1 must be 0"):
        ops.factor_inv_blocks(fac, np.array([1, 100, n]))
    with pytest.raises(TgpError, match=r"starts\[3\] = 4199 must be the factor's n = 4200"):
        ops.factor_inv_blocks(fac, np.array([0, 100, 2000, n - 1]))
    with pytest.raises(TgpError, match=r"starts\[2\] = 4201 must be the factor's n = 4200"):
        ops.factor_inv_blocks(fac, np.array([0, 2000, n + 1]))
    with pytest.raises(TgpError, match=r"group 1 \(starts\[1\] = 3 to starts\[2\] = 4100\) has more than TGP_INVBLOCK_GMAX = 4096"):
        ops.factor_inv_blocks(fac, np.array([0, 3, 4100, n]))
    blocks = ops.factor_inv_blocks(fac, np.array([0, 4096, n]))                 # the largest group there is
    d = ops.factor_inv_diag(fac)
    np.testing.assert_allclose(np.concatenate([np.diag(b) for b in blocks]), d, rtol=1e-12, atol=0)
    assert np.array_equal(blocks[0], blocks[0].T)
    fac.free()


# ---- GPInterpolation ---------------------------------------------------------------------------------------------------------
def _brute_lgo(gp, groups):
    """every group of row indices removed in turn and the residual problem solved again, with _mean and the mean function held
    fixed: per group (y_lgo, latent covariance, log p(y_G | y_-G))"""
    K0, _ = _oracle_kernel(gp)
    r = gp._y - gp._mean - gp._spatial_average
    s2 = np.asarray(gp._y_err) ** 2
    out = []
    for G in groups:
        keep = np.setdiff1d(np.arange(len(r)), G)
        W = np.linalg.solve(K0[np.ix_(keep, keep)] + np.diag(s2[keep]), K0[np.ix_(keep, G)])
        mu = W.T.dot(r[keep])
        C = K0[np.ix_(G, G)] - K0[np.ix_(G, keep)].dot(W)
        S = C + np.diag(s2[G])
        res = r[G] - mu
        logp = -0.5 * len(G) * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(S)[1] - 0.5 * res.dot(np.linalg.solve(S, res))
        out.append((mu + gp._mean + gp._spatial_average[G], C, logp))
    return out


def _count_solves(monkeypatch):
    from treegp_amd import ops
    calls = []
    real, real_dense = ops.gp_solve, ops.gp_solve_dense
    monkeypatch.setattr(ops, "gp_solve", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops, "gp_solve_dense", lambda *a, **k: (calls.append(1), real_dense(*a, **k))[1])
    return calls


@pytest.mark.parametrize("kernel,normalize", [
    ("1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))", False),
    ("1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))", True),
    ("0.8**2 * VonKarman(length_scale=0.4)", True),
    ("1.0**2 * RBF(0.3) + WhiteKernel(1e-3)", True),
    ("0.7**2 * Matern(length_scale=0.3, nu=1.5)", False),
])
def test_predict_lgo_against_deleting_each_group(kernel, normalize, monkeypatch):
    import treegp_amd as tg
    gp, rng = _gp(kernel, 700, 21, normalize=normalize)
    _, amp = _oracle_kernel(gp)
    calls = _count_solves(monkeypatch)
    # contiguous labels, names in no order: the cached alpha and the kept factor
    contiguous = np.repeat([5, 2, 9, 7, 1], [1, 99, 150, 200, 250])
    # a 4 x 4 grid of patches: scattered rows, the permuted problem on a temporary factor
    patches = tg.spatial_block_labels(gp._X, 4, 4)
    assert len(np.unique(patches)) == 16
    for labels in (contiguous, patches):
        scattered = labels is patches
        if scattered:
            gp.predict_loo()                                    # something cached and kept that must stay
        alpha0, factor0, before = gp._alpha, gp._factor, len(calls)
        y_lgo, var_lgo = gp.predict_lgo(labels, return_var=True)
        assert y_lgo.shape == var_lgo.shape == (700,)
        y2, covs = gp.predict_lgo(labels, return_cov=True)
        assert np.array_equal(gp.predict_lgo(labels), y_lgo) and np.array_equal(y2, y_lgo)
        if scattered:
            assert gp._alpha is alpha0 and gp._factor is factor0
            assert len(calls) == before + 3                     # one temporary factor per call
        else:
            assert len(calls) == 1, "one factorisation serves every call with contiguous labels"
            gp.predict_loo()
            assert len(calls) == 1
        names = list(np.unique(labels))
        groups = [np.flatnonzero(labels == lab) for lab in names]
        ref = _brute_lgo(gp, groups)
        for G, (ref_y, ref_C, _) in zip(groups, ref):
            np.testing.assert_allclose(y_lgo[G], ref_y, rtol=0, atol=1e-9 * amp)
            np.testing.assert_allclose(var_lgo[G], np.diag(ref_C), rtol=0, atol=1e-9 * amp)
        assert sorted(covs) == names
        for k in (1, len(names) - 1):                           # covariances of two groups
            idx, C = covs[names[k]]
            assert np.array_equal(idx, groups[k])
            np.testing.assert_allclose(C, ref[k][1], rtol=0, atol=1e-9 * amp)
        want = sum(r[2] for r in ref)
        got = gp.return_lgo_log_predictive(labels)
        print("%s scattered=%s: log predictive %.12g, brute force %.12g" % (kernel, scattered, got, want))
        np.testing.assert_allclose(got, want, rtol=1e-9)


def test_lgo_log_predictive_leaves_the_solution_alone_and_scores_a_singular_kernel_minus_inf():
    import treegp_amd as tg
    gp, _ = _gp("1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))", 200, 31)
    labels = tg.kfold_labels(200, 5)
    gp.predict_loo()
    alpha0, factor0 = gp._alpha, gp._factor
    got = gp.return_lgo_log_predictive(labels)
    want = sum(r[2] for r in _brute_lgo(gp, [np.flatnonzero(labels == k) for k in range(5)]))
    np.testing.assert_allclose(got, want, rtol=1e-9)
    assert gp._alpha is alpha0 and gp._factor is factor0
    theta = gp.kernel.theta + 0.1
    got_theta = gp.return_lgo_log_predictive(labels, theta=theta)
    gp2, _ = _gp("1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))", 200, 31)
    gp2.kernel = gp.kernel.clone_with_theta(theta)
    np.testing.assert_allclose(got_theta, gp2.return_lgo_log_predictive(labels), rtol=1e-12)
    assert got_theta != got
    # a kernel whose matrix is not positive definite scores -inf, as the likelihood and the leave-one-out score do
    gp3 = tg.GPInterpolation(kernel="1.0**2 * AnisotropicRBF(scale_length=[50., 50.])", optimizer="none", normalize=False)
    gp3.initialize(gp._X, gp._y, y_err=np.zeros(200))
    assert gp3.return_log_likelihood() == -np.inf
    assert gp3.return_lgo_log_predictive(labels) == -np.inf
    assert gp3.return_lgo_log_predictive(np.repeat([0, 1], 100)) == -np.inf


def test_all_distinct_labels_reproduce_predict_loo():
    gp, _ = _gp("0.8**2 * VonKarman(length_scale=0.4)", 700, 61)
    y_loo, var_loo = gp.predict_loo(return_var=True)
    factor = gp._factor
    y_lgo, var_lgo = gp.predict_lgo(np.arange(700)[::-1], return_var=True)      # every label its own run of one row
    assert gp._factor is factor
    np.testing.assert_allclose(y_lgo, y_loo, rtol=1e-10, atol=0)
    np.testing.assert_allclose(var_lgo, var_loo, rtol=1e-10, atol=0)


def test_a_large_group_goes_back_to_the_device(monkeypatch):
    """blocks above the switch-over of lgo_quantities are solved on the device: both sides agree within the tolerance of the
    brute-force test"""
    from treegp_amd import loo
    gp, _ = _gp("1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))", 700, 21, normalize=True)
    _, amp = _oracle_kernel(gp)
    labels = np.repeat([0, 1, 2], [100, 450, 150])
    assert 450 > loo.LGO_HOST_GMAX
    y_dev, covs_dev = gp.predict_lgo(labels, return_cov=True)
    y_dev2, var_dev = gp.predict_lgo(labels, return_var=True)
    score_dev = gp.return_lgo_log_predictive(labels)
    monkeypatch.setattr(loo, "LGO_HOST_GMAX", 4096)
    y_host, covs_host = gp.predict_lgo(labels, return_cov=True)
    score_host = gp.return_lgo_log_predictive(labels)
    np.testing.assert_allclose(y_dev, y_host, rtol=0, atol=1e-9 * amp)
    np.testing.assert_allclose(y_dev2, y_host, rtol=0, atol=1e-9 * amp)
    np.testing.assert_allclose(covs_dev[1][1], covs_host[1][1], rtol=0, atol=1e-9 * amp)
    np.testing.assert_allclose(var_dev[100:550], np.diag(covs_host[1][1]), rtol=0, atol=1e-9 * amp)
    np.testing.assert_allclose(score_dev, score_host, rtol=1e-9)

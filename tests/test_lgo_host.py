"""CPU-only checks of leave-group-out cross-validation (seam S3h, tgp_factor_inv_blocks): the C-ABI surface, the argument
checks that run before any device work, the host formulas of treegp_amd.loo against deleting each group and solving again,
the permutation and scatter-back of predict_lgo with the device calls replaced by NumPy stand-ins, and the label helpers."""
import os
import re
import sys

import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib, gp_interp, loo, ops

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
from test_loo_batch_host import HostFactor, host_inv_diag, host_solve, spec_matrix  # noqa: E402  (the LOO stand-ins)

ROOT = os.path.dirname(TESTS)


def test_inv_blocks_entry_point_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tgp.h")).read()
    assert re.search(r"#define\s+TGP_INVBLOCK_GMAX\s+4096\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tgp_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()
    assert "tgp_factor_inv_blocks" in declared
    assert hasattr(lib, "tgp_factor_inv_blocks"), "libtgp.so does not export tgp_factor_inv_blocks"
    restype, argtypes = _lib.SIGNATURES["tgp_factor_inv_blocks"]
    assert len(argtypes) == 5                                   # (ctx, factor, starts, ngroups, blocks)
    assert ops.INVBLOCK_GMAX == 4096
    assert tg.kfold_labels is loo.kfold_labels and tg.spatial_block_labels is loo.spatial_block_labels


# ---- the formulas -----------------------------------------------------------------------------------------------------------
def _spd(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K0 = 1.3 * np.exp(-0.5 * d2 / 0.25 ** 2)                    # latent covariance
    sigma = rng.uniform(0.05, 0.3, n)
    return rng, K0, sigma


def _brute_group(K0, sigma, r, G):
    """the group deleted, the rest solved again: (mean of r_G, latent covariance, log p(r_G | r_-G))"""
    keep = np.setdiff1d(np.arange(len(r)), G)
    Km = K0[np.ix_(keep, keep)] + np.diag(sigma[keep] ** 2)
    W = np.linalg.solve(Km, K0[np.ix_(keep, G)])
    mu = W.T.dot(r[keep])
    C = K0[np.ix_(G, G)] - K0[np.ix_(G, keep)].dot(W)
    S = C + np.diag(sigma[G] ** 2)
    res = r[G] - mu
    logp = -0.5 * len(G) * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(S)[1] - 0.5 * res.dot(np.linalg.solve(S, res))
    return mu, C, logp


def _blocks(K, starts):
    P = np.linalg.inv(K)
    return [P[s:e, s:e].copy() for s, e in zip(starts[:-1], starts[1:])]


@pytest.mark.parametrize("starts", [[0, 40], [0, 1, 2, 40], [0, 7, 8, 25, 40], list(range(41))])
def test_lgo_formulas_against_deleting_the_group(starts):
    rng, K0, sigma = _spd(40, 5)
    K = K0 + np.diag(sigma ** 2)
    r = rng.standard_normal(40)
    alpha = np.linalg.solve(K, r)
    mu, v, logp, covs = loo.lgo_quantities(r, alpha, _blocks(K, starts), sigma, starts, want_cov=True)
    assert mu.shape == v.shape == (40,) and logp.shape == (len(starts) - 1,) and len(covs) == len(starts) - 1
    for g, (s, e) in enumerate(zip(starts[:-1], starts[1:])):
        G = np.arange(s, e)
        if len(G) == 40:
            ref_mu, ref_C = np.zeros(40), K0                    # nothing is left: the prior
            ref_logp = -20 * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(K)[1] - 0.5 * r.dot(alpha)
        else:
            ref_mu, ref_C, ref_logp = _brute_group(K0, sigma, r, G)
        np.testing.assert_allclose(mu[s:e], ref_mu, rtol=0, atol=1e-11)
        np.testing.assert_allclose(covs[g], ref_C, rtol=0, atol=1e-11)
        np.testing.assert_allclose(v[s:e], np.diag(ref_C), rtol=0, atol=1e-11)
        assert abs(logp[g] - ref_logp) <= 1e-11 * max(1.0, abs(ref_logp))
    # without the covariances: the same numbers
    mu2, v2, logp2, none = loo.lgo_quantities(r, alpha, _blocks(K, starts), sigma, starts)
    assert none is None
    np.testing.assert_allclose(mu2, mu, rtol=0, atol=1e-13)
    np.testing.assert_allclose(v2, v, rtol=0, atol=1e-13)
    np.testing.assert_allclose(logp2, logp, rtol=1e-13)
    if len(starts) == 41:                                       # groups of one point: leave-one-out
        lmu, _, lv, llogp = loo.loo_quantities(r, alpha, np.diag(np.linalg.inv(K)), sigma)
        np.testing.assert_allclose(mu, lmu, rtol=0, atol=1e-13)
        np.testing.assert_allclose(v, lv, rtol=0, atol=1e-13)
        np.testing.assert_allclose(logp, llogp, rtol=1e-12)


def test_lgo_quantities_refuses_mismatched_arguments():
    rng, K0, sigma = _spd(10, 1)
    K = K0 + np.diag(sigma ** 2)
    B = _blocks(K, [0, 4, 10])
    r = np.zeros(10)
    with pytest.raises(ValueError, match="same shape"):
        loo.lgo_quantities(r, np.zeros(9), B, sigma, [0, 4, 10])
    with pytest.raises(ValueError, match="starts"):
        loo.lgo_quantities(r, r, B, sigma, [0, 4, 9])
    with pytest.raises(ValueError, match="starts"):
        loo.lgo_quantities(r, r, B, sigma, [0, 4, 4, 10])
    with pytest.raises(ValueError, match="block 1"):
        loo.lgo_quantities(r, r, [B[0], B[0]], sigma, [0, 4, 10])
    with pytest.raises(np.linalg.LinAlgError):
        loo.lgo_quantities(r, r, [B[0], -B[1]], sigma, [0, 4, 10])


# ---- stand-ins for the device ------------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    rec = {"singles": [], "dense": [], "blocks": [], "solve_rhs": []}

    def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["singles"].append(len(X))
        alpha, L = host_solve(spec_matrix(spec, X), y, np.zeros(len(y)) if y_err is None else y_err)
        return alpha, 2.0 * np.sum(np.log(np.diag(L))), float(np.dot(y, alpha)), (HostFactor(L) if keep else None)

    def gp_solve_dense(K, y, y_err=None, keep=False, want_alpha=True, ctx=None):
        rec["dense"].append(len(K))
        alpha, L = host_solve(K, y, np.zeros(len(y)) if y_err is None else y_err)
        return alpha, 2.0 * np.sum(np.log(np.diag(L))), float(np.dot(y, alpha)), (HostFactor(L) if keep else None)

    def factor_inv_blocks(factor, starts, ctx=None):
        assert not factor.freed
        starts = [int(s) for s in starts]
        rec["blocks"].append(starts)
        return _blocks(factor.L.dot(factor.L.T), starts)

    def factor_solve(factor, B, ctx=None):
        rec["solve_rhs"].append(len(B))
        return np.linalg.solve(factor.L.T, np.linalg.solve(factor.L, np.asarray(B).T)).T

    monkeypatch.setattr(_lib, "get_ctx", lambda: "ctx")
    monkeypatch.setattr(ops, "gp_solve", gp_solve)
    monkeypatch.setattr(ops, "gp_solve_dense", gp_solve_dense)
    monkeypatch.setattr(ops, "factor_inv_blocks", factor_inv_blocks)
    monkeypatch.setattr(ops, "factor_inv_diag", lambda f, ctx=None: host_inv_diag(f.L))
    monkeypatch.setattr(ops, "factor_solve", factor_solve)
    return rec


def make_gp(n, seed, kernel="1.0**2 * RBF(1.5)", normalize=True):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, 2))
    gp = tg.GPInterpolation(kernel=kernel, optimizer="none", normalize=normalize)
    gp.initialize(X, np.sin(X[:, 0]) + 0.4 + 0.1 * rng.standard_normal(n), y_err=rng.uniform(0.1, 0.2, n))
    return gp


def _latent(gp):
    try:
        return spec_matrix(gp_interp.kernel_to_spec(gp.kernel), gp._X)
    except NotImplementedError:
        return gp.kernel(gp._X)


def _brute_predict_lgo(gp, labels):
    K0, r, sigma = _latent(gp), gp._residual(), np.asarray(gp._y_err)
    y, v, covs, total = np.empty(len(r)), np.empty(len(r)), {}, 0.0
    for lab in np.unique(labels):
        G = np.flatnonzero(labels == lab)
        mu, C, logp = _brute_group(K0, sigma, r, G)
        y[G], v[G], covs[lab.item()] = mu + gp._mean + gp._spatial_average[G], np.diag(C), (G, C)
        total += logp
    return y, v, covs, total


TREE = "RBF(1.0) + WhiteKernel(0.01)"


@pytest.mark.parametrize("kernel", ["1.0**2 * RBF(1.5)", TREE])
def test_contiguous_labels_use_the_cached_solution(fake, kernel):
    gp = make_gp(60, 1, kernel=kernel)
    labels = np.repeat([7, 3, 9, 4], [1, 20, 14, 25])            # contiguous runs, names neither sorted nor dense
    y, v = gp.predict_lgo(labels, return_var=True)
    count = fake["dense"] if kernel == TREE else fake["singles"]
    assert count == [60] and fake["blocks"] == [[0, 1, 21, 35, 60]]
    alpha, factor = gp._alpha, gp._factor
    assert alpha is not None and factor is not None and not factor.freed
    ref_y, ref_v, ref_covs, ref_total = _brute_predict_lgo(gp, labels)
    np.testing.assert_allclose(y, ref_y, rtol=0, atol=1e-10)
    np.testing.assert_allclose(v, ref_v, rtol=0, atol=1e-10)
    y2, covs = gp.predict_lgo(labels, return_cov=True)
    assert np.array_equal(y2, y) and np.array_equal(gp.predict_lgo(labels), y)
    assert count == [60], "the kept factor serves every later call"
    assert gp._alpha is alpha and gp._factor is factor
    assert list(covs) == [7, 3, 9, 4]                           # the groups in their order of appearance
    for lab, (idx, C) in covs.items():
        assert np.array_equal(idx, ref_covs[lab][0])
        np.testing.assert_allclose(C, ref_covs[lab][1], rtol=0, atol=1e-10)
        np.testing.assert_allclose(np.diag(C), v[idx], rtol=0, atol=1e-13)
    gp.predict_loo()
    assert count == [60] and gp._factor is factor               # predict_loo and predict_lgo share the kept factor
    np.testing.assert_allclose(gp.return_lgo_log_predictive(labels), ref_total, rtol=1e-10)
    assert count == [60, 60] and gp._alpha is alpha and gp._factor is factor       # a temporary factor of its own


@pytest.mark.parametrize("kernel", ["1.0**2 * RBF(1.5)", TREE])
def test_scattered_labels_are_permuted_and_scattered_back(fake, kernel):
    gp = make_gp(50, 2, kernel=kernel)
    rng = np.random.default_rng(8)
    labels = rng.integers(0, 6, 50) * 10 - 20                    # negative, sparse names in no order
    assert len(np.unique(labels)) == 6
    y, v = gp.predict_lgo(labels, return_var=True)
    assert gp._alpha is None and gp._factor is None              # a temporary factor: nothing cached, nothing kept
    sizes = [int(np.sum(labels == lab)) for lab in np.unique(labels)]
    assert fake["blocks"] == [list(np.concatenate([[0], np.cumsum(sizes)]))]
    ref_y, ref_v, ref_covs, ref_total = _brute_predict_lgo(gp, labels)
    np.testing.assert_allclose(y, ref_y, rtol=0, atol=1e-10)
    np.testing.assert_allclose(v, ref_v, rtol=0, atol=1e-10)
    y2, covs = gp.predict_lgo(labels, return_cov=True)
    np.testing.assert_allclose(y2, y, rtol=0, atol=1e-13)
    assert sorted(covs) == sorted(ref_covs)
    for lab, (idx, C) in covs.items():
        assert np.array_equal(idx, ref_covs[lab][0])            # the stable sort keeps a group's points in their order
        np.testing.assert_allclose(C, ref_covs[lab][1], rtol=0, atol=1e-10)
    # a kept factor and a cached alpha are left exactly as they were
    gp.predict_loo()
    alpha, factor = gp._alpha, gp._factor
    gp.predict_lgo(labels)
    assert gp._alpha is alpha and gp._factor is factor and not factor.freed
    np.testing.assert_allclose(gp.return_lgo_log_predictive(labels), ref_total, rtol=1e-10)
    assert gp._alpha is alpha and gp._factor is factor
    # theta= is the value of the cloned kernel
    theta = gp.kernel.theta + 0.1
    before = gp.kernel.theta.copy()
    got = gp.return_lgo_log_predictive(labels, theta=theta)
    assert np.array_equal(gp.kernel.theta, before) and got != ref_total
    # all-distinct labels: leave-one-out
    y_loo, v_loo = gp.predict_loo(return_var=True)
    for distinct in (np.arange(50), rng.permutation(50)):
        y1, v1 = gp.predict_lgo(distinct, return_var=True)
        np.testing.assert_allclose(y1, y_loo, rtol=0, atol=1e-11)
        np.testing.assert_allclose(v1, v_loo, rtol=0, atol=1e-11)


def test_labels_are_validated_before_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_lib, "get_ctx", no_device)
    monkeypatch.setattr(_lib, "load_library", no_device)
    gp = make_gp(12, 3)
    for bad in (np.zeros(11, dtype=int), np.zeros((12, 1), dtype=int), 3):
        with pytest.raises(ValueError, match=r"shape \(12,\)"):
            gp.predict_lgo(bad)
        with pytest.raises(ValueError, match=r"shape \(12,\)"):
            gp.return_lgo_log_predictive(bad)
    with pytest.raises(ValueError, match="at most one"):
        gp.predict_lgo(np.zeros(12, dtype=int), return_var=True, return_cov=True)
    big = make_gp(4200, 4)
    labels = np.full(4200, 5)
    labels[:50] = 17
    labels[100:150] = 17                                         # 4100 points carry the label 5, scattered around 17's
    with pytest.raises(ValueError, match=r"group 5 has 4100 points.*4096"):
        big.predict_lgo(labels)
    with pytest.raises(ValueError, match=r"group 5 has 4100 points.*4096"):
        big.return_lgo_log_predictive(labels)
    assert gp._alpha is None and big._alpha is None
    with pytest.raises(ValueError, match="kept factor"):
        ops.factor_inv_blocks(None, [0, 3])
    freed = ops.Factor(None, None, 10)
    with pytest.raises(ValueError, match="kept factor"):
        ops.factor_inv_blocks(freed, [0, 10])
    alive = ops.Factor(None, 1, 10)
    try:
        for bad in ([0], [[0, 10]], [0.0, 10.0]):
            with pytest.raises(ValueError, match="1-D integer"):
                ops.factor_inv_blocks(alive, bad)
    finally:
        alive._h = None                                          # nothing to free


def test_large_blocks_go_back_to_the_device_and_agree_with_lapack(fake, monkeypatch):
    rng, K0, sigma = _spd(90, 6)
    K = K0 + np.diag(sigma ** 2)
    r = rng.standard_normal(90)
    alpha = np.linalg.solve(K, r)
    starts = [0, 10, 50, 90]
    B = _blocks(K, starts)
    host = loo.lgo_quantities(r, alpha, B, sigma, starts, want_cov=True)
    assert fake["dense"] == [] and fake["solve_rhs"] == []
    assert 100 <= loo.LGO_HOST_GMAX <= 1000                      # the shipped switch-over: a few hundred rows
    monkeypatch.setattr(loo, "LGO_HOST_GMAX", 10)                # the two groups of 40 now take the device route
    dev = loo.lgo_quantities(r, alpha, B, sigma, starts, want_cov=True)
    assert fake["dense"] == [40, 40] and fake["solve_rhs"] == [40, 40]
    dev_var = loo.lgo_quantities(r, alpha, B, sigma, starts)
    assert fake["dense"] == [40] * 4 and fake["solve_rhs"] == [40, 40]         # identity right-hand sides only when asked for
    for h, d, d2 in zip(host[:3], dev[:3], dev_var[:3]):
        np.testing.assert_allclose(d, h, rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(d2, h, rtol=1e-10, atol=1e-11)
    for Ch, Cd in zip(host[3], dev[3]):
        np.testing.assert_allclose(Cd, Ch, rtol=0, atol=1e-11)
        assert np.array_equal(Cd, Cd.T)


# ---- label helpers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(10, 10), (103, 10), (7, 1), (4096, 3)])
def test_kfold_labels(n, k):
    lab = tg.kfold_labels(n, k)
    assert lab.shape == (n,) and lab.dtype.kind == "i"
    counts = np.bincount(lab, minlength=k)
    assert len(counts) == k and counts.sum() == n and counts.max() - counts.min() <= 1
    assert np.array_equal(lab, tg.kfold_labels(n, k, random_state=0))
    if n > 20:
        assert not np.array_equal(lab, tg.kfold_labels(n, k, random_state=1))
        assert not np.array_equal(lab, np.sort(lab))             # the folds are random, not runs of rows
    with pytest.raises(ValueError):
        tg.kfold_labels(n, n + 1)
    with pytest.raises(ValueError):
        tg.kfold_labels(n, 0)


def test_spatial_block_labels():
    rng = np.random.default_rng(2)
    X = rng.uniform(-3, 5, (500, 2))
    X[0], X[1] = [-3, -3], [5, 5]                               # the corners of the bounding box
    lab = tg.spatial_block_labels(X, 4, 3)
    assert lab.shape == (500,) and lab.min() >= 0 and lab.max() <= 11 and lab[0] == 0 and lab[1] == 11
    ix, iy = lab % 4, lab // 4
    assert np.all(np.abs((X[:, 0] + 3) / 8 * 4 - (ix + 0.5)) <= 0.5 + 1e-12)
    assert np.all(np.abs((X[:, 1] + 3) / 8 * 3 - (iy + 0.5)) <= 0.5 + 1e-12)
    # empty cells produce no label: points in two opposite corners only
    Y = np.concatenate([rng.uniform(0, 0.1, (20, 2)), rng.uniform(0.9, 1.0, (30, 2))])
    lab = tg.spatial_block_labels(Y, 4, 4)
    assert sorted(np.unique(lab)) == [0, 15] and np.sum(lab == 0) == 20
    # one dimension, one point, one cell
    assert np.array_equal(tg.spatial_block_labels(np.array([0.0, 0.49, 0.51, 1.0]), 2, 5), [0, 0, 1, 1])
    assert np.array_equal(tg.spatial_block_labels(np.array([[2.0, 3.0]]), 3, 3), [0])
    assert np.array_equal(tg.spatial_block_labels(X, 1, 1), np.zeros(500, dtype=int))
    with pytest.raises(ValueError):
        tg.spatial_block_labels(X, 0, 2)
    with pytest.raises(ValueError):
        tg.spatial_block_labels(np.zeros((4, 3)), 2, 2)

"""Host references of the local conditionals (include/tgp.h, seam S3v), built on tests/_local_refs.py: used by
test_vecchia_host.py and test_gpu_vecchia.py.  Nothing here calls the library.

  eligible neighbours   brute force: the stable sort of the whitened distances of _local_refs with the ineligible rows (the row
                        itself; or every row that is not earlier in the ordering) moved to +inf, cut at min(k, eligible rows)
  conditionals          ``_local_refs.local_predict_ld`` on those (or on given) lists with the query X[i]; rows are grouped by the
                        length of their list, an empty list gives mu = 0, var = amp
  sums                  the per-row terms and their sums in np.longdouble
  dense log L           a column Cholesky in np.longdouble
"""
import numpy as np

import _local_refs as LR

LD = np.longdouble
LOG_2PI = np.log(LD(2.0) * np.pi)


def self_dist2(spec, X):
    return LR.dist2(spec, X, X)


def eligible(n, mode, rank=None):
    """(n, n) bool: E[i, r] = row r may be in row i's list"""
    if mode == "loo":
        return ~np.eye(n, dtype=bool)
    rank = np.asarray(rank)
    return rank[None, :] < rank[:, None]


def brute_lists(spec, X, k, mode, rank=None, D=None):
    """nbr (n, k) int32 padded with -1, cnt (n) int32: the min(k, eligible) nearest eligible rows, nearest first, ties to the
    lower row"""
    D = self_dist2(spec, X) if D is None else D
    n = D.shape[0]
    E = eligible(n, mode, rank)
    order = np.argsort(np.where(E, D, np.inf), axis=1, kind="stable")
    cnt = np.minimum(E.sum(axis=1), k).astype(np.int32)
    nbr = np.full((n, k), -1, dtype=np.int32)
    take = min(k, n)
    nbr[:, :take] = order[:, :take]
    nbr[np.arange(k)[None, :] >= cnt[:, None]] = -1
    return nbr, cnt


def check_lists(spec, X, nbr, cnt, k, mode, rank=None, D=None):
    """asserts that every list is a valid nearest-eligible set: cnt = min(k, eligible rows), -1 exactly from cnt on, eligible rows
    only, all different, nearest first, the farthest member no farther than (1 + 1e-12) x the nearest eligible row left out"""
    D = self_dist2(spec, X) if D is None else D
    n = D.shape[0]
    E = eligible(n, mode, rank)
    nbr, cnt = np.asarray(nbr), np.asarray(cnt)
    assert nbr.shape == (n, k) and nbr.dtype == np.int32 and cnt.shape == (n,) and cnt.dtype == np.int32
    assert np.array_equal(cnt, np.minimum(E.sum(axis=1), k)), "cnt is not min(k, eligible rows)"
    pad = np.arange(k)[None, :] >= cnt[:, None]
    assert (nbr[pad] == -1).all() and (nbr[~pad] >= 0).all() and nbr.max(initial=-1) < n, "padding or range"
    safe = np.where(pad, 0, nbr).astype(np.int64)
    assert np.take_along_axis(E, safe, axis=1)[~pad].all(), "an ineligible row is in a list"
    srt = np.sort(np.where(pad, n + np.arange(k)[None, :], nbr), axis=1)
    assert (np.diff(srt, axis=1) > 0).all(), "a row appears twice in a list"
    dm = np.where(pad, np.inf, np.take_along_axis(D, safe, axis=1))
    assert (dm[:, 1:] >= dm[:, :-1]).all(), "a list is not nearest first"
    out = np.where(E, D, np.inf)
    rows = np.repeat(np.arange(n), k)[~pad.ravel()]
    out[rows, nbr[~pad]] = np.inf
    nearest_out = out.min(axis=1)
    last = np.where(cnt > 0, dm[np.arange(n), np.maximum(cnt - 1, 0)], -np.inf)
    assert (last <= (1.0 + 1e-12) * nearest_out).all(), "a nearer eligible row was left out"


def cond_ld(spec, X, y, y_err, nbr, cnt, K=None, rows=None):
    """mu, var (float64) and info of the conditionals ON THE GIVEN lists, long-double solves; ``rows``: only these rows (the
    outputs are then theirs, in that order)"""
    X = LR.as_xy(X)
    nbr, cnt = np.asarray(nbr), np.asarray(cnt)
    rows = np.arange(len(nbr)) if rows is None else np.asarray(rows)
    mu, var = np.zeros(len(rows)), np.full(len(rows), float(spec.amp))
    info = np.zeros(len(rows), dtype=np.int32)
    for c in np.unique(cnt[rows]):
        if c == 0:
            continue
        at = np.flatnonzero(cnt[rows] == c)
        r = rows[at]
        a, b, f = LR.local_predict_ld(spec, X, y, y_err, X[r], nbr[r, :c], K=K, Kx=None if K is None else K[r])
        mu[at], var[at], info[at] = a, b, f
    return mu, var, info


def cond_reference(spec, X, y, y_err, k, mode, rank=None):
    """the whole definition on the host: mu, var, nbr, cnt, info"""
    nbr, cnt = brute_lists(spec, X, k, mode, rank)
    mu, var, info = cond_ld(spec, X, y, y_err, nbr, cnt, K=LR.kernel_values(spec, X))
    return mu, var, nbr, cnt, info


def terms_ld(y, y_err, mu, var):
    """the per-row terms log s2_i and (y_i - mu_i)^2 / s2_i in np.longdouble, with r_i and s2_i"""
    e2 = np.zeros(len(y)) if y_err is None else np.asarray(y_err, dtype=np.float64) ** 2
    s2 = np.asarray(var, dtype=LD) + e2.astype(LD)
    r = np.asarray(y, dtype=LD) - np.asarray(mu, dtype=LD)
    return np.log(s2), r * r / s2, r, s2


def log_score_ld(y, y_err, mu, var):
    """-1/2 sum r^2 / s2 - 1/2 sum log s2 - n/2 log 2 pi in np.longdouble"""
    t0, t1, _, _ = terms_ld(y, y_err, mu, var)
    return -LD(0.5) * t1.sum() - LD(0.5) * t0.sum() - LD(0.5) * len(y) * LOG_2PI


def check_sums(y, y_err, mu, var, sums, tag=""):
    """sums against the long-double sums of the terms formed from the device's own mu and var: (log2 n + 8) 2^-53 sum |t_i| --
    the fixed tree, and the few-ulp log and the divide of each term"""
    t0, t1, _, _ = terms_ld(y, y_err, mu, var)
    n = len(y)
    for j, t in enumerate((t0, t1)):
        bound = (np.log2(n) + 8.0) * 2.0 ** -53 * float(np.abs(t).sum())
        err = abs(float(LD(sums[j]) - t.sum()))
        print("%s sums[%d]: |device - long double| = %.3e, bound %.3e" % (tag, j, err, bound))
        assert err <= bound
    assert sums[2] == 0.0


def dense_loglik_ld(K, y, y_err):
    """log L of the dense GP in np.longdouble: K float64 with diagonal amp; returns (log L, y.K^-1.y, log det)"""
    n = len(y)
    A = np.array(K, dtype=LD)
    if y_err is not None:
        A[np.arange(n), np.arange(n)] += np.asarray(y_err, dtype=LD) ** 2
    L = np.zeros_like(A)
    w = np.zeros(n, dtype=LD)
    yl = np.asarray(y, dtype=LD)
    for j in range(n):
        col = A[j:, j] - L[j:, :j].dot(L[j, :j])
        assert col[0] > 0
        L[j:, j] = col / np.sqrt(col[0])
        w[j] = (yl[j] - L[j, :j].dot(w[:j])) / L[j, j]
    chi2, logdet = (w * w).sum(), LD(2.0) * np.log(np.diag(L)).sum()
    return -LD(0.5) * chi2 - LD(0.5) * logdet - LD(0.5) * n * LOG_2PI, chi2, logdet


def loo_closed_form(K, y, y_err):
    """leave-one-out mean and latent variance from K^-1 (Rasmussen & Williams 5.4.2) in np.longdouble"""
    n = len(y)
    e2 = np.zeros(n, dtype=LD) if y_err is None else np.asarray(y_err, dtype=LD) ** 2
    A = np.array(K, dtype=LD)
    A[np.arange(n), np.arange(n)] += e2
    # Gauss-Jordan without pivoting on a positive definite matrix, in long double (np.linalg has no long-double solver)
    M = np.hstack([A, np.eye(n, dtype=LD)])
    for j in range(n):
        M[j] = M[j] / M[j, j]
        f = M[:, j].copy()
        f[j] = 0
        M -= f[:, None] * M[j][None, :]
    Ki = M[:, n:]
    d = np.diag(Ki)
    alpha = Ki.dot(np.asarray(y, dtype=LD))
    return np.asarray(y, dtype=LD) - alpha / d, LD(1.0) / d - e2

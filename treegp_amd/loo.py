"""Leave-one-out (LOO) quantities of a GP from alpha = K^-1 r and d = diag(K^-1) (Rasmussen & Williams 2006, section 5.4.2,
eqs. 5.10-5.12; not in the reference).  K = amp k(X, X) + diag(sigma^2) is the noisy covariance the library factorises, r the
residual it was solved for.  Point i left out of the other n - 1:

    mu_i = r_i - alpha_i / d_i                                 LOO mean of r_i
    s_i  = 1 / d_i                                             noisy predictive variance (of y_i)
    v_i  = 1 / d_i - sigma_i^2                                 latent predictive variance (what predict(X, return_var=True) means)
    log p(y_i | y_-i) = -1/2 log 2 pi + 1/2 log d_i - 1/2 alpha_i^2 / d_i

O(n) on the host; d comes from the device (ops.factor_inv_diag).

Further down: the same closed form for GROUPS of points left out (lgo_quantities, from the diagonal blocks of K^-1 that
ops.factor_inv_blocks computes), and the helpers that label the groups (kfold_labels, spatial_block_labels).
"""
import numpy as np

_HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def loo_quantities(r, alpha, d, sigma):
    """(mu, s, v, logp) for one residual r (n,) and its alpha (n,), or a stack of them (k, n); d and sigma (n,) are shared
    by the stack.  Nothing is clamped: v may come out slightly negative where the noise dominates, as predict's variance."""
    r, alpha = np.asarray(r, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    d, sigma = np.asarray(d, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    if r.shape != alpha.shape or r.shape[-1:] != d.shape or d.shape != sigma.shape:
        raise ValueError("loo_quantities: r and alpha must have the same shape (n,) or (k, n), d and sigma (n,)")
    s = 1.0 / d
    mu = r - alpha / d
    v = s - sigma ** 2
    logp = -_HALF_LOG_2PI + 0.5 * np.log(d) - 0.5 * alpha * alpha / d
    return mu, s, v, logp


# ---- leave-group-out: the same closed form with the diagonal BLOCKS of P = K^-1 (ops.factor_inv_blocks) --------------------------
#     mu_G = r_G - P_GG^-1 alpha_G                               prediction of r_G from the points outside G
#     S_G  = P_GG^-1                                             noisy predictive covariance (of y_G)
#     C_G  = P_GG^-1 - diag(sigma_G^2)                           latent covariance (what predict(X[G], return_cov=True) means)
#     log p(y_G | y_-G) = -g/2 log 2 pi + 1/2 log det P_GG - 1/2 alpha_G^T P_GG^-1 alpha_G
LGO_HOST_GMAX = 384      # blocks up to this many rows are solved with LAPACK on the host, larger ones on the device


def _lgo_block_host(P, a, want_cov):
    """(P^-1 a, log det P, diag(P^-1), P^-1 or None) by LAPACK's Cholesky; numpy.linalg.LinAlgError when P is not positive definite"""
    from scipy.linalg import cho_solve, solve_triangular
    L = np.linalg.cholesky(P)
    x = cho_solve((L, True), a)
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    Linv = solve_triangular(L, np.eye(len(P)), lower=True)
    if want_cov:
        S = Linv.T.dot(Linv)
        return x, logdet, np.diag(S).copy(), S
    return x, logdet, np.sum(Linv * Linv, axis=0), None


def _lgo_block_device(P, a, want_cov):
    """the same for a large block, which goes back to the device as a dense problem of its own: the solve gives P^-1 a and
    log det P, its factor the diagonal of P^-1 and, when asked for, P^-1 from identity right-hand sides"""
    from . import ops
    x, logdet, _, factor = ops.gp_solve_dense(P, a, None, keep=True)
    try:
        d = ops.factor_inv_diag(factor)
        S = None
        if want_cov:
            g = len(P)
            S = np.empty((g, g))
            for i0 in range(0, g, 512):
                E = np.zeros((min(512, g - i0), g))
                E[np.arange(len(E)), i0 + np.arange(len(E))] = 1.0
                S[i0:i0 + len(E)] = ops.factor_solve(factor, E)
            S = 0.5 * (S + S.T)
    finally:
        factor.free()
    return x, logdet, d, S


def lgo_quantities(r, alpha, blocks, sigma, starts, want_cov=False):
    """(mu (n,), v (n,), logp (ngroups,), covs) for the residual r (n,), its alpha (n,), the diagonal blocks of K^-1 of the groups
    of contiguous rows starts[g] .. starts[g+1] - 1 (a list of (g, g) arrays, ops.factor_inv_blocks) and sigma (n,): the
    leave-group-out mean of every point, its latent variance diag(C_G), every group's log predictive density and, for want_cov,
    the list of the latent covariances C_G (else None).  Nothing is clamped.  Raises numpy.linalg.LinAlgError when a block is
    not positive definite."""
    r, alpha, sigma = (np.asarray(a, dtype=np.float64) for a in (r, alpha, sigma))
    starts = np.asarray(starts, dtype=np.int64)
    n = r.shape[0] if r.ndim == 1 else -1
    if r.ndim != 1 or alpha.shape != (n,) or sigma.shape != (n,):
        raise ValueError("lgo_quantities: r, alpha and sigma must have the same shape (n,)")
    if starts.ndim != 1 or len(starts) != len(blocks) + 1 or starts[0] != 0 or starts[-1] != n or np.any(np.diff(starts) < 1):
        raise ValueError("lgo_quantities: starts must rise from 0 to n = %d in len(blocks) + 1 = %d entries" % (n, len(blocks) + 1))
    mu, v = np.empty(n), np.empty(n)
    logp = np.empty(len(blocks))
    covs = [] if want_cov else None
    for g, P in enumerate(blocks):
        s, e = int(starts[g]), int(starts[g + 1])
        P = np.asarray(P, dtype=np.float64)
        if P.shape != (e - s, e - s):
            raise ValueError("lgo_quantities: block %d must be (%d, %d), got %r" % (g, e - s, e - s, P.shape))
        solve = _lgo_block_host if e - s <= LGO_HOST_GMAX else _lgo_block_device
        x, logdet, d, S = solve(P, alpha[s:e], want_cov)
        mu[s:e] = r[s:e] - x
        v[s:e] = d - sigma[s:e] ** 2
        logp[g] = -(e - s) * _HALF_LOG_2PI + 0.5 * logdet - 0.5 * alpha[s:e].dot(x)
        if want_cov:
            C = S.copy()
            C[np.diag_indices(e - s)] -= sigma[s:e] ** 2
            covs.append(C)
    return mu, v, logp, covs


def group_runs(labels, gmax=None):
    """(perm or None, starts (ngroups + 1,), names (ngroups,)) for one label per point: perm is None when every label already
    occupies one contiguous run of rows (the groups are then taken in their order of appearance), else the stable sort by label
    that makes them contiguous.  ValueError naming the label for a group above gmax points."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or len(labels) < 1:
        raise ValueError("group labels must be a 1-D array with one entry per point, got shape %r" % (labels.shape,))
    n = len(labels)
    edges = np.flatnonzero(labels[1:] != labels[:-1]) + 1
    perm = None
    if len(edges) + 1 != len(np.unique(labels)):
        perm = np.argsort(labels, kind="stable")
        labels = labels[perm]
        edges = np.flatnonzero(labels[1:] != labels[:-1]) + 1
    starts = np.concatenate([[0], edges, [n]]).astype(np.int64)
    names = labels[starts[:-1]]
    sizes = np.diff(starts)
    if gmax is not None and sizes.max() > gmax:
        g = int(np.argmax(sizes))
        raise ValueError("group %r has %d points; a group may hold at most %d" % (names[g].item(), sizes[g], gmax))
    return perm, starts, names


def kfold_labels(n, k, random_state=0):
    """(n,) labels 0 .. k - 1 of k random folds whose sizes differ by at most one point (the folds of
    np.random.default_rng(random_state).permutation(n) dealt in turn)"""
    n, k = int(n), int(k)
    if n < 1 or k < 1 or k > n:
        raise ValueError("kfold_labels: need 1 <= k <= n, got n = %d, k = %d" % (n, k))
    labels = np.empty(n, dtype=np.int64)
    labels[np.random.default_rng(random_state).permutation(n)] = np.arange(n) % k
    return labels


def spatial_block_labels(X, nx, ny):
    """(n,) labels iy * nx + ix of the cells of an nx x ny grid over the bounding box of X (n, 1 or 2): leaving a label out
    leaves a patch of the field without stars.  Cells without a point produce no label."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    nx, ny = int(nx), int(ny)
    if X.ndim != 2 or X.shape[1] not in (1, 2) or len(X) < 1 or nx < 1 or ny < 1:
        raise ValueError("spatial_block_labels: X must be (n, 1 or 2) with n >= 1 and nx, ny >= 1")

    def cell(x, m):
        lo, hi = x.min(), x.max()
        if not hi > lo:
            return np.zeros(len(x), dtype=np.int64)
        return np.minimum((m * ((x - lo) / (hi - lo))).astype(np.int64), m - 1)

    ix = cell(X[:, 0], nx)
    iy = cell(X[:, 1], ny) if X.shape[1] == 2 else np.zeros(len(X), dtype=np.int64)
    return iy * nx + ix

"""Host references of local kriging (include/tgp.h, seam S3l): used by test_local_host.py and test_gpu_local.py.  Nothing here
calls the library.

  neighbours   brute force in float64 in the whitened metric, with the header's arithmetic: u0 = r00 x + (r01 y), u1 = r11 y,
               d2 = du0^2 + du1^2, every product and sum rounded on its own (NumPy never fuses them); ties to the lower row.
  local solve  kernel values in float64 (the oracle's, as in the other _refs files), then the factorisation, the two
               substitutions and the sums in np.longdouble: a column Cholesky written out here, run for a batch of queries at
               once, with k* and y_S carried along as two extra rows (row k of the factor of [[K, .], [k*^T, .]] is
               (L^-1 k*)^T: the forward substitution, term for term).
"""
import numpy as np

from oracle import gp_oracle as O
from treegp_amd import _lib

LD = np.longdouble
KIND_NAME = {_lib.TGP_RBF: "gauss", _lib.TGP_ARBF: "gauss", _lib.TGP_VK: "vk", _lib.TGP_AVK: "avk"}


def as_xy(X):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.shape[1] == 1:
        X = np.hstack([X, np.zeros_like(X)])
    return X


def whitening(spec):
    """(r00, r01, r11) of the upper-triangular R with R^T R = invLam; the identity for the isotropic kinds; LinAlgError when
    invLam has no Cholesky factor"""
    if spec.kind in (_lib.TGP_RBF, _lib.TGP_VK):
        return 1.0, 0.0, 1.0
    if not spec.a > 0 or not np.isfinite(spec.a):
        raise np.linalg.LinAlgError("invLam is not positive definite")
    r00 = np.sqrt(np.float64(spec.a))
    r01 = np.float64(spec.b) / r00
    s = np.float64(spec.c) - r01 * r01
    if not s > 0 or not np.isfinite(s):
        raise np.linalg.LinAlgError("invLam is not positive definite")
    return float(r00), float(r01), float(np.sqrt(s))


def whiten(spec, X):
    r00, r01, r11 = whitening(spec)
    X = as_xy(X)
    t = r01 * X[:, 1]
    return np.stack([r00 * X[:, 0] + t, r11 * X[:, 1]], axis=1)


def dist2(spec, X, Xs):
    """(m, n) squared distances in the whitened metric"""
    U, Us = whiten(spec, X), whiten(spec, Xs)
    d0 = U[None, :, 0] - Us[:, None, 0]
    d1 = U[None, :, 1] - Us[:, None, 1]
    return d0 * d0 + d1 * d1


def brute_neighbors(spec, X, Xs, k, D=None):
    """(m, min(k, n)) int32: the k nearest rows, nearest first, ties to the lower row (a stable sort of the distances)"""
    D = dist2(spec, X, Xs) if D is None else D
    k = min(int(k), D.shape[1])
    return np.argsort(D, axis=1, kind="stable")[:, :k].astype(np.int32)


def check_neighbor_sets(spec, X, Xs, nbr, D=None):
    """asserts that every row of nbr is a valid nearest set: rows of the table, all different, nearest first, and the farthest
    member no farther than (1 + 1e-12) x the nearest row left out"""
    D = dist2(spec, X, Xs) if D is None else D
    m, n = D.shape
    nbr = np.asarray(nbr)
    assert nbr.shape[0] == m and nbr.dtype == np.int32
    k = nbr.shape[1]
    assert k <= n and nbr.min() >= 0 and nbr.max() < n
    assert (np.diff(np.sort(nbr, axis=1), axis=1) > 0).all(), "a row appears twice in a neighbour list"
    dm = np.take_along_axis(D, nbr.astype(np.int64), axis=1)
    assert (np.diff(dm, axis=1) >= 0).all(), "a neighbour list is not nearest first"
    if k < n:
        out = np.array(D)
        np.put_along_axis(out, nbr.astype(np.int64), np.inf, axis=1)
        nearest_out = out.min(axis=1)
        worst = np.max(dm[:, -1] - (1.0 + 1e-12) * nearest_out)
        assert (dm[:, -1] <= (1.0 + 1e-12) * nearest_out).all(), "a nearer row was left out (by %g)" % worst


def kernel_values(spec, A, B=None):
    """amp k(A, B) in float64 from the oracle (B None: the self kernel, diagonal exactly amp)"""
    return O.kernel_matrix(KIND_NAME[spec.kind], as_xy(A), None if B is None else as_xy(B), amp=spec.amp, a=spec.a, b=spec.b,
                           c=spec.c, ell=spec.ell)


def solve_ld_batch(KS, ks, yS):
    """KS (B, k, k), ks (B, k), yS (B, k) -> ys (B), vv (B), info (B): L L^T = KS, v = L^-1 ks, w = L^-1 yS, ys = v.w, vv = v.v, all
    in np.longdouble; info = 0 or the order of the first pivot that is not positive (outputs NaN then)"""
    B, k = ks.shape
    M = np.empty((B, k + 2, k), dtype=LD)
    M[:, :k, :] = KS
    M[:, k, :] = ks
    M[:, k + 1, :] = yS
    L = np.zeros_like(M)
    info = np.zeros(B, dtype=np.int32)
    for j in range(k):
        col = M[:, j:, j] - np.einsum("bip,bp->bi", L[:, j:, :j], L[:, j, :j])
        piv = col[:, 0]
        bad = ~(piv > 0)
        info[bad & (info == 0)] = j + 1
        piv = np.where(bad, LD(1.0), piv)
        L[:, j:, j] = col / np.sqrt(piv)[:, None]
    v, w = L[:, k, :], L[:, k + 1, :]
    ys, vv = (v * w).sum(axis=1), (v * v).sum(axis=1)
    ys[info > 0] = np.nan
    vv[info > 0] = np.nan
    return ys, vv, info


def local_predict_ld(spec, X, y, y_err, Xs, nbr, K=None, Kx=None, batch=128):
    """ys, var (float64) and info of local kriging ON THE GIVEN neighbour lists nbr (m, k).  K = kernel_values(spec, X) and
    Kx = kernel_values(spec, Xs, X) may be passed in (computed once per case and shared)."""
    X, Xs = as_xy(X), as_xy(Xs)
    nbr = np.asarray(nbr, dtype=np.int64)
    m, k = nbr.shape
    y = np.asarray(y, dtype=np.float64)
    e2 = np.zeros(len(X)) if y_err is None else np.asarray(y_err, dtype=np.float64) ** 2
    ys, var, info = np.empty(m), np.empty(m), np.empty(m, dtype=np.int32)
    for s in range(0, m, batch):
        nb = nbr[s:s + batch]
        if K is not None:
            KS = K[nb[:, :, None], nb[:, None, :]]
        else:
            KS = np.stack([kernel_values(spec, X[r]) for r in nb])
        KS = np.array(KS, dtype=np.float64)
        idx = np.arange(k)
        KS[:, idx, idx] = spec.amp + e2[nb]
        if Kx is not None:
            kst = np.take_along_axis(Kx[s:s + batch], nb, axis=1)
        else:
            kst = np.stack([kernel_values(spec, Xs[s + t:s + t + 1], X[r])[0] for t, r in enumerate(nb)])
        a, vv, inf = solve_ld_batch(KS, kst, y[nb])
        ys[s:s + batch] = np.array(a, dtype=np.float64)
        var[s:s + batch] = np.array(LD(spec.amp) - vv, dtype=np.float64)
        info[s:s + batch] = inf
    return ys, var, info


def local_predict(spec, X, y, y_err, Xs, k):
    """the whole definition on the host: brute-force neighbours, then the long-double solve; returns ys, var, nbr, info"""
    nbr = brute_neighbors(spec, X, Xs, k)
    ys, var, info = local_predict_ld(spec, X, y, y_err, Xs, nbr)
    return ys, var, nbr, info


def dense_predict(spec, X, y, y_err, Xs):
    """the exact GP through the oracle's dense route: ys and the diagonal of the posterior covariance"""
    X, Xs = as_xy(X), as_xy(Xs)
    e = np.zeros(len(X)) if y_err is None else np.asarray(y_err, dtype=np.float64)
    K = kernel_values(spec, X)
    HT = kernel_values(spec, Xs, X)
    alpha, _ = O.gp_solve(K, np.asarray(y, dtype=np.float64), e)
    cov = O.gp_predict_cov(K, e, HT, kernel_values(spec, Xs))
    return O.gp_predict(HT, alpha), np.diag(cov).copy()


# ---- data shared by the host and the GPU tests ---------------------------------------------------------------------------------
AMP = 0.64
SPECS = {
    "rbf": dict(kind=_lib.TGP_RBF, amp=AMP, a=1.0 / 0.15 ** 2, b=0.0, c=1.0 / 0.15 ** 2),
    "arbf": dict(kind=_lib.TGP_ARBF, amp=AMP, a=60.0, b=-14.0, c=35.0),
    "vk": dict(kind=_lib.TGP_VK, amp=AMP, ell=0.6),
    "avk": dict(kind=_lib.TGP_AVK, amp=AMP, a=4.0, b=0.8, c=2.5),
}
NOISE2 = 2.5e-3 * AMP            # yerr^2: cond(K_S) <= k amp / yerr^2 + 1 <= 5.2e4 for k <= 128 by the trace bound


def make_spec(name, **over):
    from treegp_amd import ops
    kw = dict(SPECS[name])
    kw.update(over)
    return ops.KernelSpec(**kw)


def uniform_data(n, m, seed=11):
    """n uniform points of the unit square with a smooth field plus scatter, errors of NOISE2, m uniform queries"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, 2))
    y = np.sin(5.0 * X[:, 0]) * np.cos(3.0 * X[:, 1]) + 0.05 * rng.standard_normal(n)
    y_err = np.full(n, np.sqrt(NOISE2))
    Xs = rng.uniform(-0.02, 1.02, size=(m, 2))
    return X, y, y_err, Xs

"""Host references of the local routes up the condition ladder (test_local_ladder_host.py, test_gpu_local_ladder.py): numpy and
scipy only (mpmath in the host test of the truth's validity).  Nothing here calls the library.

The data are the ladder's (tests/_cond_ladder.py): 2304 points of the unit square, an RBF of length 0.1 and amplitude 1, five
noise levels.  A query's k nearest stars lie within about one correlation length, so the local matrices K_S reach
cond_2 = 2.6e3 ... 8e10 for k = 32 ... 128, and the true s2 = var + yerr^2 falls to 1e-9 amp on the top rung.

  truth    kernel values in np.longdouble from the fp64 coordinates (differences, then the quadratic form, then exp), the
           diagonal amp + e^2 in long double, then ``_local_refs.solve_ld_batch``.  The truth carries the TRUE kernel and not an
           fp64 rounding of it: at cond 1e10 one ulp of a kernel value moves the answer as much as LAPACK's own rounding does.
  LAPACK   scipy.linalg.cholesky + solve_triangular in fp64 on the oracle's fp64 kernel values, mu = v.w, var = amp - v.v: the
           reference project's arithmetic applied to one local matrix.
  model    a numpy fp64 model of local_solve_kernel's order of operations (treegp_amd/csrc/local.hip), without fused
           multiply-adds: the host test holds it to the bound, which is thereby attainable.
  figures  each divided by its scale, maximum over the rows: mu (max|y|), var (amp), and for the conditionals
           logs2 = |log s2 - log s2_true| and chi = |r^2/s2 - (r^2/s2)_true| / max_i (r^2/s2)_true, formed here in long double from
           a candidate's fp64 mu and var.
  bound    bound_u(lapack) = 16 x max(LAPACK's figure, 2^-53): 16 is the project's margin against a vendor solver
           (_cond_ladder.bound); the floor is one unit round-off of the scale and not that function's 1e-12, which would hide the
           variance errors these tests exist for (LAPACK's |dvar| stays at a few u amp on every rung).

Gaussian kernels only.  The solve is the same template for every kind; the von Karman profile is held to 2e-13 of its value by
test_gpu_kernel_values.py, 1e3 u, which would swamp the solver's error."""
import functools

import numpy as np
import scipy.linalg as sl

import _cond_ladder as CL
import _local_refs as LR
import _vecchia_refs as VR

LD, U, AMP = CL.LD, CL.U, CL.AMP
N = 2304
KS = (32, 33, 128)               # the 32-bucket full, one past it, the 128-bucket full
MODES = ("loo", "prior")
NROWS = 256                      # sampled training rows of the conditionals
SHEAR = dict(amp=AMP, a=60.0, b=-14.0, c=35.0)     # the sheared kernel: 128 neighbours lie within d^T invLam d <= 1 (host test)
NPATCH = 129                     # the dense patch: the ladder points nearest (0.5, 0.5)
NPATCH_Q = 64


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def bound_u(lapack_err, factor=16.0):
    return factor * max(float(lapack_err), U)


@functools.lru_cache(maxsize=None)
def spec(name="rbf"):
    from treegp_amd import _lib, ops
    if name == "rbf":
        return ops.KernelSpec(_lib.TGP_RBF, **CL.KW)
    return ops.KernelSpec(_lib.TGP_ARBF, **SHEAR)


@functools.lru_cache(maxsize=None)
def vecchia_rank(n=N, seed=0):
    """the definition of ops.vecchia_rank, restated (the GPU tests assert that the two agree)"""
    order = np.random.default_rng(seed).permutation(n)
    rank = np.empty(n, dtype=np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    return _ro(rank)[0]


@functools.lru_cache(maxsize=None)
def sample_rows():
    """the 256 sampled training rows: 0, n - 1, the rows of lowest and highest Vecchia rank, and random ones; sorted"""
    rank = vecchia_rank()
    fixed = sorted({0, N - 1, int(np.argmin(rank)), int(np.argmax(rank))})
    rest = np.random.default_rng(4).choice(np.setdiff1d(np.arange(N), fixed), NROWS - len(fixed), replace=False)
    return _ro(np.sort(np.concatenate([fixed, rest])).astype(np.int64))[0]


# ---- kernel values -------------------------------------------------------------------------------------------------------------

def kernel_ld(sp, A, B=None):
    """amp k(A, B) in long double from the fp64 coordinates; B None: the self kernel, diagonal exactly amp"""
    A = np.asarray(LR.as_xy(A), dtype=LD)
    Bv = A if B is None else np.asarray(LR.as_xy(B), dtype=LD)
    dx = A[:, None, 0] - Bv[None, :, 0]
    dy = A[:, None, 1] - Bv[None, :, 1]
    q = LD(sp.a) * dx * dx + LD(2.0) * LD(sp.b) * dx * dy + LD(sp.c) * dy * dy
    K = LD(sp.amp) * np.exp(-q / LD(2.0))
    if B is None:
        K[np.diag_indices(len(A))] = LD(sp.amp)
    return K


@functools.lru_cache(maxsize=None)
def tables(name="rbf"):
    """what every rung shares for one kernel: the whitened distances (stars, and queries to stars) and the kernel values of the
    stars and of the 256 queries, in fp64 from the oracle and in long double"""
    sp = spec(name)
    X, _ = CL.points(N)
    Xq = CL.queries()
    return dict(zip(("D", "Dq", "K", "Kq", "Kl", "Kql"), _ro(
        VR.self_dist2(sp, X), LR.dist2(sp, X, Xq), LR.kernel_values(sp, X), LR.kernel_values(sp, Xq, X),
        kernel_ld(sp, X), kernel_ld(sp, Xq, X))))


@functools.lru_cache(maxsize=None)
def brute_lists(name, k, mode):
    """(nbr (n, k), cnt (n)) of _vecchia_refs.brute_lists; the same on every rung"""
    rank = vecchia_rank() if mode == "prior" else None
    return _ro(*VR.brute_lists(spec(name), CL.points(N)[0], k, mode, rank, D=tables(name)["D"]))


@functools.lru_cache(maxsize=None)
def brute_query_lists(name, k):
    return _ro(LR.brute_neighbors(spec(name), CL.points(N)[0], CL.queries(), k, D=tables(name)["Dq"]))[0]


# ---- the three solvers on given lists --------------------------------------------------------------------------------------------

def _groups(cnt):
    for c in np.unique(cnt):
        yield int(c), np.flatnonzero(cnt == c)


def truth_on_lists(amp, y, e, nbr, cnt, Kl, Kql):
    """mu, var (long double) of each row t on its list nbr[t, :cnt[t]]: Kl (n, n) and Kql (rows, n) are long-double kernel
    values of the stars and of the rows' own points; an empty list gives 0 and amp.  Every matrix must factor."""
    m = len(nbr)
    nbr = np.asarray(nbr, dtype=np.int64)
    el2 = np.asarray(e, dtype=LD) ** 2
    mu, var = np.zeros(m, dtype=LD), np.full(m, LD(amp))
    for c, at in _groups(np.asarray(cnt)):
        if c == 0:
            continue
        for s in range(0, len(at), 128):
            t = at[s:s + 128]
            nb = nbr[t, :c]
            KS = Kl[nb[:, :, None], nb[:, None, :]]
            idx = np.arange(c)
            KS[:, idx, idx] = LD(amp) + el2[nb]
            a, vv, info = LR.solve_ld_batch(KS, np.take_along_axis(Kql[t], nb, axis=1), np.asarray(y, dtype=LD)[nb])
            assert not info.any(), "the long-double factorisation met a pivot that is not positive"
            mu[t], var[t] = a, LD(amp) - vv
    return mu, var


def lapack_on_lists(amp, y, e, nbr, cnt, K, Kq):
    """mu, var (fp64), min pivot: scipy's Cholesky in fp64 on the oracle's fp64 kernel values K (n, n), Kq (rows, n), row by row.
    A matrix LAPACK does not factor gives NaN and a pivot of 0."""
    m = len(nbr)
    e2 = np.asarray(e, dtype=np.float64) ** 2
    mu, var, piv = np.zeros(m), np.full(m, float(amp)), np.full(m, np.inf)
    for t in range(m):
        c = int(cnt[t])
        if c == 0:
            continue
        S = np.asarray(nbr[t, :c], dtype=np.int64)
        A = np.array(K[np.ix_(S, S)])
        A[np.arange(c), np.arange(c)] = amp + e2[S]
        try:
            L = sl.cholesky(A, lower=True)
        except np.linalg.LinAlgError:
            mu[t], var[t], piv[t] = np.nan, np.nan, 0.0
            continue
        v = sl.solve_triangular(L, Kq[t, S], lower=True)
        w = sl.solve_triangular(L, y[S], lower=True)
        mu[t], var[t], piv[t] = np.dot(v, w), amp - np.dot(v, v), np.diag(L).min()
    return mu, var, piv


def _lane_sum(P):
    """sum over the last axis (length <= 128) in the kernel's order: lane l adds c = l, l + 64 in turn, then a butterfly"""
    B, k = P.shape
    s = np.zeros((B, 64))
    for c0 in range(0, k, 64):
        part = P[:, c0:c0 + 64]
        s[:, :part.shape[1]] = s[:, :part.shape[1]] + part
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ off]
    return s[:, 0]


def model_on_lists(amp, y, e, nbr, cnt, K, Kq):
    """mu, var, info (fp64) by local_solve_kernel's order of operations in numpy fp64, every product and sum rounded on its own:
    right-looking, column j scaled by the rounded 1 / sqrt(d_j) on either side of every update, rows k and k + 1 carried
    along, v_c = A[k][c] / sqrt(A[c][c]) by the reciprocal again, the two sums in the lanes' order, var = amp - v.v"""
    m = len(nbr)
    nbr = np.asarray(nbr, dtype=np.int64)
    e2 = np.asarray(e, dtype=np.float64) ** 2
    mu, var, info = np.zeros(m), np.full(m, float(amp)), np.zeros(m, dtype=np.int32)
    for c, at in _groups(np.asarray(cnt)):
        if c == 0:
            continue
        nb = nbr[at, :c]
        A = np.empty((len(at), c + 2, c))
        A[:, :c, :] = K[nb[:, :, None], nb[:, None, :]]
        idx = np.arange(c)
        A[:, idx, idx] = amp + e2[nb]
        A[:, c, :] = np.take_along_axis(Kq[at], nb, axis=1)
        A[:, c + 1, :] = y[nb]
        fail = np.zeros(len(at), dtype=np.int32)
        for j in range(c):
            d = A[:, j, j]
            fail[(fail == 0) & ~(d > 0.0)] = j + 1
            inv = 1.0 / np.sqrt(np.where(d > 0.0, d, 1.0))
            li = A[:, j + 1:, j] * inv[:, None]
            lc = A[:, j + 1:c, j] * inv[:, None]
            A[:, j + 1:, j + 1:] = A[:, j + 1:, j + 1:] - li[:, :, None] * lc[:, None, :]
        dg = A[:, idx, idx]
        inv = 1.0 / np.sqrt(np.where(dg > 0.0, dg, 1.0))
        v, w = A[:, c, :] * inv, A[:, c + 1, :] * inv
        a, vv = _lane_sum(v * w), _lane_sum(v * v)
        mu[at] = np.where(fail > 0, np.nan, a)
        var[at] = np.where(fail > 0, np.nan, amp - vv)
        info[at] = fail
    return mu, var, info


# ---- figures ---------------------------------------------------------------------------------------------------------------------

def terms(y, e, mu, var):
    """log s2 and r^2 / s2 in long double, s2 = var + e^2 with e^2 formed in long double, r = y - mu"""
    s2 = np.asarray(var, dtype=LD) + np.asarray(e, dtype=LD) ** 2
    r = np.asarray(y, dtype=LD) - np.asarray(mu, dtype=LD)
    return np.log(s2), r * r / s2, s2


def figures(mu, var, mu_t, var_t, yscale, amp=AMP, y=None, e=None):
    """dict of the figures of a candidate (mu, var) against the truth; with y and e (the rows' own) logs2 and chi too"""
    f = {"mu": float(np.abs(np.asarray(mu, dtype=LD) - mu_t).max() / yscale),
         "var": float(np.abs(np.asarray(var, dtype=LD) - var_t).max() / amp)}
    if y is not None:
        l, c, _ = terms(y, e, mu, var)
        lt, ct, _ = terms(y, e, mu_t, var_t)
        f["logs2"] = float(np.abs(l - lt).max())
        f["chi"] = float(np.abs(c - ct).max() / ct.max())
    return f


class Case(object):
    """The truth and LAPACK's answer on one set of lists, and LAPACK's figures.  Nothing in it is written after construction."""

    def __init__(self, name, y, e, nbr, cnt, rows=None, amp=AMP):
        """rows None: the lists are those of the 256 queries; else of these training rows (then logs2 and chi exist)"""
        T = tables(name)
        self.nbr, self.cnt, self.rows, self.amp = np.array(nbr), np.array(cnt), rows, amp
        Kq, Kql = (T["Kq"], T["Kql"]) if rows is None else (T["K"][rows], T["Kl"][rows])
        self.y, self.e = (None, None) if rows is None else (y[rows], e[rows])
        self.yscale = float(np.abs(y).max())
        self.mu_t, self.var_t = truth_on_lists(amp, y, e, nbr, cnt, T["Kl"], Kql)
        self.mu_l, self.var_l, self.piv_l = lapack_on_lists(amp, y, e, nbr, cnt, T["K"], Kq)
        self.inputs = (y, e, T["K"], Kq)
        self.lapack = self.figures(self.mu_l, self.var_l)
        _ro(self.nbr, self.cnt, self.mu_t, self.var_t, self.mu_l, self.var_l, self.piv_l)

    def figures(self, mu, var):
        return figures(mu, var, self.mu_t, self.var_t, self.yscale, self.amp, self.y, self.e)

    def model(self):
        y, e, K, Kq = self.inputs
        return model_on_lists(self.amp, y, e, self.nbr, self.cnt, K, Kq)

    def s2_true(self):
        e = np.zeros(len(self.mu_t)) if self.e is None else self.e
        return self.var_t + np.asarray(e, dtype=LD) ** 2


def rung_data(i):
    X, y, e, _, _ = CL.rung(i, N)
    return X, y, e


@functools.lru_cache(maxsize=None)
def cond_case(i, k, mode, name="rbf"):
    """the conditionals of the 256 sampled rows on the brute-force lists"""
    _, y, e = rung_data(i)
    rows = sample_rows()
    nbr, cnt = brute_lists(name, k, mode)
    return Case(name, y, e, nbr[rows], cnt[rows], rows=rows)


@functools.lru_cache(maxsize=None)
def predict_case(i, k, name="rbf"):
    """local kriging at the 256 queries on the brute-force lists"""
    _, y, e = rung_data(i)
    nbr = brute_query_lists(name, k)
    return Case(name, y, e, nbr, np.full(len(nbr), k, dtype=np.int32))


def cond_case_on(i, k, mode, nbr_rows, cnt_rows, name="rbf"):
    """the case of the lists a device returned for the sampled rows: the cached one where they are the brute-force lists"""
    ref = cond_case(i, k, mode, name)
    if np.array_equal(ref.nbr, nbr_rows) and np.array_equal(ref.cnt, cnt_rows):
        return ref
    _, y, e = rung_data(i)
    return Case(name, y, e, nbr_rows, cnt_rows, rows=sample_rows())


def predict_case_on(i, k, nbr, name="rbf"):
    ref = predict_case(i, k, name)
    if np.array_equal(ref.nbr, nbr):
        return ref
    _, y, e = rung_data(i)
    return Case(name, y, e, nbr, np.full(len(nbr), k, dtype=np.int32))


def local_cond2(name, i, k, mode="loo"):
    """cond_2 of the 256 local matrices (fp64, oracle kernel values) of the sampled rows' brute-force lists"""
    _, _, e = rung_data(i)
    nbr, cnt = brute_lists(name, k, mode)
    K = tables(name)["K"]
    out = []
    for r in sample_rows():
        S = nbr[r, :cnt[r]].astype(np.int64)
        if len(S) == 0:
            continue
        A = np.array(K[np.ix_(S, S)])
        A[np.arange(len(S)), np.arange(len(S))] = AMP + e[S] ** 2
        out.append(CL.cond2(A))
    return np.array(out)


# ---- the dense patch -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def patch():
    """(rows (129,) of the ladder points nearest (0.5, 0.5), nearest first; Xq (64, 2) queries within the patch)"""
    X, _ = CL.points(N)
    d2 = (X[:, 0] - 0.5) ** 2 + (X[:, 1] - 0.5) ** 2
    rows = np.argsort(d2, kind="stable")[:NPATCH]
    radius = np.sqrt(d2[rows[-1]])
    rng = np.random.default_rng(6)
    rho, phi = radius * np.sqrt(rng.uniform(size=NPATCH_Q)), rng.uniform(0.0, 2.0 * np.pi, NPATCH_Q)
    Xq = np.stack([0.5 + rho * np.cos(phi), 0.5 + rho * np.sin(phi)], axis=1)
    return _ro(rows, Xq)


class PatchCase(object):
    """rung i on the dense patch: the log-likelihood of its 129 points (truth and LAPACK's), and the exact GP of the first 128 at
    the 64 patch queries (truth and LAPACK's)"""

    def __init__(self, i):
        sp = spec("rbf")
        X, y, e = rung_data(i)
        rows, Xq = patch()
        self.X, self.y, self.e, self.Xq = _ro(np.array(X[rows]), np.array(y[rows]), np.array(e[rows]), Xq)
        n = NPATCH
        Kl, K = kernel_ld(sp, self.X), LR.kernel_values(sp, self.X)
        self.ll_t = VR.dense_loglik_ld(Kl, self.y, self.e)[0]
        A = np.array(K)
        A[np.arange(n), np.arange(n)] = AMP + self.e ** 2
        L = sl.cholesky(A, lower=True)
        w = sl.solve_triangular(L, self.y, lower=True)
        self.ll_l = -0.5 * np.dot(w, w) - np.sum(np.log(np.diag(L))) - 0.5 * n * np.log(2.0 * np.pi)
        self.ll_err_lapack = abs(float(LD(self.ll_l) - self.ll_t))
        self.ll_bound = 16.0 * max(self.ll_err_lapack, U * abs(float(self.ll_t)))
        # the exact GP of the first 128 points at the patch queries
        k = n - 1
        nbr = np.tile(np.arange(k, dtype=np.int32), (NPATCH_Q, 1))
        cnt = np.full(NPATCH_Q, k, dtype=np.int32)
        self.yscale = float(np.abs(y).max())
        self.mu_t, self.var_t = truth_on_lists(AMP, self.y[:k], self.e[:k], nbr, cnt, Kl[:k, :k], kernel_ld(sp, Xq, self.X[:k]))
        mu_l, var_l, piv = lapack_on_lists(AMP, self.y[:k], self.e[:k], nbr, cnt, K[:k, :k], LR.kernel_values(sp, Xq, self.X[:k]))
        assert (piv > 0).all()
        self.lapack = self.figures(mu_l, var_l)
        # a model of the dense route on one 128-block: products with the explicit inverse W of L
        Lk = sl.cholesky(A[:k, :k], lower=True)
        W = sl.solve_triangular(Lk, np.eye(k), lower=True)
        H = LR.kernel_values(sp, Xq, self.X[:k])
        V = W @ H.T
        self.explicit_inverse = self.figures(H @ (W.T @ (W @ self.y[:k])), AMP - np.sum(V * V, axis=0))

    def figures(self, mu, var):
        return figures(mu, var, self.mu_t, self.var_t, self.yscale)


@functools.lru_cache(maxsize=None)
def patch_case(i):
    return PatchCase(i)


def judge(route, i, cond, dev, lap, exceptions=None):
    """one LADDER line per figure of ``dev`` beside ``lap``; returns the list of misses of 16 x max(LAPACK, u) (or of the entry of
    ``exceptions`` for (route, rung, figure))"""
    bad = []
    for what in sorted(dev):
        print(CL.line(route, i, cond, what, dev[what], lap[what]))
        factor = (exceptions or {}).get((route, i, what), 16.0)
        if not dev[what] <= bound_u(lap[what], factor):
            bad.append("%s rung %d %s: %.3e > %g x max(LAPACK %.3e, u)" % (route, i, what, dev[what], factor, lap[what]))
    return bad

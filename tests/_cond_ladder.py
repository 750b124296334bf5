"""Host-side references of the condition ladder (test_cond_ladder_host.py, test_gpu_cond_ladder.py): numpy and scipy only.

The ladder is one point set and one field, K = amp k(X) + noise^2 I with an RBF of length 0.1 on the unit square, at five noise
levels: cond_2(K) = 1.3e4 ... 1.5e11 at n = 2304, the range BASELINE.md (section 2) records for the reference's users.  A route
that solves with the Cholesky factor is judged against a solution of the same fp64 matrix that carries digits LAPACK's does not
(refined_solve: residuals and the running solution in 80-bit long double), and beside what LAPACK itself achieves on that
matrix for the same quantity, computed as the reference project computes it.  All residuals and dot products of the metrics
are taken in long double, so the figures are the solvers' errors and not the yardstick's."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.linalg as sl

from oracle import gp_oracle as O

U = 2.0 ** -53                                      # unit round-off of fp64
LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the ladder's reference needs an 80-bit (or wider) long double"

NOISES = (1e-1, 1e-2, 1e-3, 1e-4, 3e-5)
COND_2304 = (1.3e4, 1.3e6, 1.3e8, 1.3e10, 1.5e11)   # cond_2(K) at n = 2304, seed 1
RUNGS = tuple(range(len(NOISES)))
AMP = 1.0
ELL = 0.1
KW = dict(amp=AMP, a=1.0 / ELL ** 2, b=0.0, c=1.0 / ELL ** 2)
NQ = 256                                            # queries of the prediction error
REFINE_STEPS = 4


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def points(n, seed=1):
    """(X, clean field) shared by the five rungs of one size"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, 2))
    return _ro(X, np.sin(5.0 * X[:, 0]) * np.cos(3.0 * X[:, 1]))


@functools.lru_cache(maxsize=None)
def rung(i, n, seed=1):
    """X (n, 2), y (n,), e (n,) constant, K0 = amp k(X), K = K0 with K0[j, j] + e[j]**2 on the diagonal (the one rounding the
    device's dense route also makes).  Read-only arrays."""
    noise = NOISES[i]
    X, f = points(n, seed)
    y = f + noise * np.random.default_rng([seed, i, n]).standard_normal(n)
    e = np.full(n, noise)
    K0 = O.kernel_matrix("gauss", X, **KW)
    K = K0.copy()
    K[np.diag_indices(n)] = np.diag(K0) + e ** 2
    return _ro(X, y, e, K0, K)


@functools.lru_cache(maxsize=None)
def queries(seed=2):
    """the NQ fixed random query points of the prediction error"""
    return _ro(np.random.default_rng(seed).uniform(0.0, 1.0, (NQ, 2)))[0]


def cond2(K):
    ev = np.linalg.eigvalsh(K)
    return float(ev[-1] / ev[0])


@functools.lru_cache(maxsize=None)
def rung_cond(i, n):
    """cond_2 of a rung: computed at the small sizes, the recorded figure (test_cond_ladder_host.py holds it to a factor 2)
    at n = 2304 and the ragged size just below it"""
    return COND_2304[i] if n >= 2048 else cond2(rung(i, n)[4])


def _rows_ld(A, B, r):
    return np.einsum("ij,j...->i...", A[r:r + 128].astype(LD), B)


def matmul_ld(A, B):
    """A @ B with the products and sums in long double; A fp64 (converted a block of rows at a time), B any float type.
    numpy has no BLAS for long double: several right-hand sides go through a few threads, a block of rows each."""
    B = np.asarray(B, dtype=LD)
    starts = range(0, A.shape[0], 128)
    if B.ndim == 1 or B.shape[1] < 8:
        parts = [_rows_ld(A, B, r) for r in starts]
    else:
        with ThreadPoolExecutor(8) as ex:
            parts = list(ex.map(lambda r: _rows_ld(A, B, r), starts))
    return np.concatenate(parts, axis=0)


def refined_solve(K, B, factor=None):
    """K^-1 B for the fp64 matrix K, B (n,) or (n, k): scipy.linalg.cho_factor in fp64, then REFINE_STEPS steps of iterative
    refinement with the residual B - K x and the running solution x in long double.  Returns (x in long double, corrections):
    corrections[s] is max |dx| of step s, per column.  The solution is valid when check_refinement(corrections) passes."""
    if factor is None:
        factor = sl.cho_factor(K, lower=True)
    Bl = np.asarray(B, dtype=LD)
    x = sl.cho_solve(factor, np.asarray(B, dtype=np.float64)).astype(LD)
    corr = []
    for _ in range(REFINE_STEPS):
        r = Bl - matmul_ld(K, x)
        d = sl.cho_solve(factor, r.astype(np.float64))
        x = x + d
        corr.append(np.abs(d).max(axis=0))
    x.setflags(write=False)
    return x, np.array(corr, dtype=np.float64)


def check_refinement(corr, what=""):
    """The validity condition of a refined solution: the last correction is at most 1e-2 of the first (the first is LAPACK's
    own forward error, so the result carries two or more digits beyond LAPACK's).  A rung that misses it fails its test."""
    first, last = np.atleast_1d(corr[0]), np.atleast_1d(corr[-1])
    assert np.all(np.isfinite(corr)), what
    assert np.all(last <= 1e-2 * first), "%s: refinement stalled, corrections %s" % (what, np.asarray(corr).reshape(len(corr), -1).max(axis=1))


class Reference(object):
    """Everything the tests of one rung share: the inputs, LAPACK's factor and solution, the refined solution and the
    quantities the metrics are scaled by.  Nothing in it is written after construction."""

    def __init__(self, K, y, X=None, spec_kw=None, kind="gauss", factor=None):
        self.K, self.y, self.n, self.X = K, y, K.shape[0], X
        # (cho_factor raises LinAlgError where LAPACK cannot factor the rung)
        self.factor = sl.cho_factor(K, lower=True) if factor is None else factor
        self.alpha_lapack = sl.cho_solve(self.factor, y)
        self.alpha, self.corr = refined_solve(K, y, self.factor)
        self.normK = float(np.abs(K).sum(axis=1).max())
        self.ydota = float(np.dot(np.asarray(y, dtype=LD), self.alpha))
        if X is not None:
            self.H = O.kernel_matrix(kind, queries(), X, **(spec_kw or KW))
            self.H.setflags(write=False)
            self.pred = matmul_ld(self.H, self.alpha)
            self.pred_scale = float(np.abs(self.pred).max())
        self.lapack = self.metrics(self.alpha_lapack, float(np.dot(y, self.alpha_lapack)))

    def metrics(self, alpha, ydota=None):
        """dict of the issue's five figures for a candidate alpha (fp64): eta, pred, resid, ydota, fwd"""
        a = np.asarray(alpha, dtype=LD)
        r = np.abs(matmul_ld(self.K, a) - self.y)
        m = {
            "eta": float(r.max() / (self.normK * np.abs(a).max() + np.abs(self.y).max())),
            "resid": float(r.max() / np.abs(self.y).max()),
            "fwd": float(np.abs(a - self.alpha).max() / np.abs(self.alpha).max()),
        }
        if hasattr(self, "H"):
            m["pred"] = float(np.abs(matmul_ld(self.H, a - self.alpha)).max() / self.pred_scale)
        if ydota is not None:
            m["ydota"] = abs(float((LD(ydota) - np.dot(np.asarray(self.y, dtype=LD), self.alpha)) / self.ydota))
        return m


@functools.lru_cache(maxsize=None)
def reference(i, n, seed=1):
    X, y, e, K0, K = rung(i, n, seed)
    return Reference(K, y, X)


# ---- the posterior family: variance, covariance diagonal, diag(K^-1) and its blocks ------------------------------------------

NPOST = 64                       # queries of the variance / covariance: 32 random, 32 training points shifted by 1e-3
FIXED_ROWS = (0, 127, 128, 1023, 1024)
BLOCK = (1000, 1130)             # the block of K^-1 the tests fetch: 130 rows across the 1024 step


@functools.lru_cache(maxsize=None)
def posterior_inputs(n, seed=3):
    """(Xq (64, 2), rows (64,)): the query points and the sampled rows of K^-1 -- FIXED_ROWS, n - 1 and random ones"""
    rng = np.random.default_rng(seed)
    X, _ = points(n)
    near = X[rng.choice(n, NPOST // 2, replace=False)] + 1e-3
    Xq = np.vstack([rng.uniform(0.0, 1.0, (NPOST // 2, 2)), near])
    fixed = [r for r in FIXED_ROWS if r < n] + [n - 1]
    rest = rng.choice(np.setdiff1d(np.arange(n), fixed), NPOST - len(fixed), replace=False)
    rows = np.sort(np.concatenate([fixed, rest])).astype(np.int64)
    return _ro(Xq, rows)


class PosteriorReference(object):
    """Variance at the 64 queries, diag(K^-1) at the 64 sampled rows and the BLOCK of K^-1, from refined solves in long
    double; LAPACK's fp64 figures for the same quantities, formed as the reference project forms them."""

    def __init__(self, ref, what="", with_block=True):
        """ref: the Reference of the matrix (an oracle rung, or the device's own K of one)"""
        X, K, n = ref.X, ref.K, ref.n
        Xq, rows = posterior_inputs(n)
        self.Xq, self.rows = Xq, rows
        self.HT = O.kernel_matrix("gauss", Xq, X, **KW)                       # (64, n)
        self.Kss = O.kernel_matrix("gauss", Xq, **KW)
        self.HT.setflags(write=False)
        self.Kss.setflags(write=False)
        E = np.zeros((n, len(rows)))
        E[rows, np.arange(len(rows))] = 1.0
        Xs, corr = refined_solve(K, np.hstack([self.HT.T, E]), ref.factor)
        check_refinement(corr, "posterior " + what)
        xk, xe = Xs[:, :NPOST], Xs[:, NPOST:]
        self.var = AMP - np.einsum("ji,ij->j", self.HT.astype(LD), xk)        # amp - k*^T K^-1 k*
        self.invdiag = xe[rows, np.arange(len(rows))]
        # LAPACK, fp64: amp - |L^-1 k*|^2, Kss - V^T V, |L^-1 e_i|^2
        V = sl.solve_triangular(ref.factor[0], self.HT.T, lower=True)
        self.var_lapack = AMP - np.sum(V * V, axis=0)
        self.covdiag_lapack = np.diag(self.Kss - V.T @ V)
        Ve = sl.solve_triangular(ref.factor[0], E, lower=True)
        self.invdiag_lapack = np.sum(Ve * Ve, axis=0)
        self.err_var_lapack = float(np.abs(self.var_lapack - self.var).max() / AMP)
        self.err_covdiag_lapack = float(np.abs(self.covdiag_lapack - self.var).max() / AMP)
        self.err_invdiag_lapack = float(np.abs((self.invdiag_lapack - self.invdiag) / self.invdiag).max())
        if with_block:
            b0, b1 = BLOCK
            Eb = np.zeros((n, b1 - b0))
            Eb[np.arange(b0, b1), np.arange(b1 - b0)] = 1.0
            Xb, corr = refined_solve(K, Eb, ref.factor)
            check_refinement(corr, "block " + what)
            self.block = Xb[b0:b1]                                            # (130, 130) of K^-1
            Vb = sl.solve_triangular(ref.factor[0], Eb, lower=True)
            self.block_lapack = Vb.T @ Vb
            self.err_block_lapack = self.block_err(self.block_lapack)

    def block_err(self, Bk):
        """max relative error of the entries of a candidate block, each against its own reference value"""
        return float(np.abs((np.asarray(Bk, dtype=LD) - self.block) / self.block).max())


@functools.lru_cache(maxsize=None)
def posterior_reference(i, n, with_block=True):
    return PosteriorReference(reference(i, n), "rung %d n %d" % (i, n), with_block)


def bound(lapack_err, factor=16.0):
    """what a device figure is held to: max(16 x LAPACK's error for the same quantity on the same matrix, 1e-12 x scale).
    16 is the project's margin against a vendor solver (test_kernel_matrix_factor_residual_against_rocsolver); 1e-12 is the
    kernel-table tolerance of DESIGN.md section 5, a floor where both errors are at rounding level.  The figures of this module
    are already divided by their scale, so the floor is 1e-12."""
    return max(factor * lapack_err, 1e-12)


def line(route, i, cond, what, dev, lap):
    """one printed line per figure: the route x rung tables of LAB_NOTES.md are made of these"""
    return "LADDER %-34s rung %d cond %.1e %-8s device %.3e lapack %.3e ratio %.2f" % (
        route, i, cond, what, dev, lap, dev / lap if lap > 0 else float("inf"))

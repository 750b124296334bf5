"""Dense host references of the Fisher information in the device's parameters (include/tgp.h, seam S2j): used by
test_fisher_host.py and test_gpu_fisher.py.  Nothing here calls the library.

For term t of a kernel, p_t = (log amp, a, b, c); with (K, W, dx, dy) of ``_vk_loglik_grad_refs.kernel_and_slope`` and W's
diagonal zeroed, D_0 = K (without noise), D_1 = -1/2 W dx^2, D_2 = -W dx dy, D_3 = -1/2 W dy^2.  With L the Cholesky factor of
sum_t K_t + diag(y_err^2) and S_r = L^-1 D_r L^-T (two triangular solves), F[r][s] = 1/2 <S_r, S_s>.

Two versions: float64 through LAPACK, and np.longdouble with a column Cholesky and a substitution of its own (up to n = 600).
"""
import numpy as np
from scipy import linalg

from _vk_loglik_grad_refs import kernel_and_slope

LONGDOUBLE_NMAX = 600


def terms_of(spec):
    """the ops.KernelSpec terms of a KernelSpec or a KernelSumSpec"""
    return list(getattr(spec, "terms", [spec]))


def derivative_matrices(spec, X):
    """(Ksum, [D_0 .. D_{4T-1}]) in float64, term order"""
    Ds, Ksum = [], 0.0
    for s in terms_of(spec):
        K, W, dx, dy = kernel_and_slope(s.kind, X, s.amp, s.a, s.b, s.c, s.ell)
        W = np.array(W)
        np.fill_diagonal(W, 0.0)
        Ds += [K, -0.5 * W * dx * dx, -W * dx * dy, -0.5 * W * dy * dy]
        Ksum = Ksum + K
    return Ksum, Ds


def _noisy(Ksum, y_err, n):
    Kn = np.array(Ksum, dtype=np.float64)
    if y_err is not None:
        Kn[np.diag_indices(n)] += np.asarray(y_err, dtype=np.float64) ** 2
    return Kn


def fisher_f64(spec, X, y_err):
    """F_p (4T, 4T) through LAPACK; numpy.linalg.LinAlgError for a matrix that is not positive definite"""
    Ksum, Ds = derivative_matrices(spec, X)
    L = np.linalg.cholesky(_noisy(Ksum, y_err, len(Ksum)))
    S = []
    for D in Ds:
        Y = linalg.solve_triangular(L, D, lower=True)                    # L^-1 D
        S.append(linalg.solve_triangular(L, Y.T, lower=True))            # L^-1 (L^-1 D)^T = L^-1 D L^-T
    return np.array([[0.5 * np.sum(a * b) for b in S] for a in S])


def cholesky_ld(A):
    """column Cholesky in np.longdouble"""
    A = np.array(A, dtype=np.longdouble)
    n = len(A)
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        col = A[j:, j] - L[j:, :j].dot(L[j, :j])
        if not col[0] > 0:
            raise np.linalg.LinAlgError("%d-th leading minor is not positive definite" % (j + 1))
        L[j:, j] = col / np.sqrt(col[0])
    return L


def forward_ld(L, B):
    """L^-1 B by forward substitution in np.longdouble"""
    Y = np.array(B, dtype=np.longdouble)
    for i in range(len(L)):
        Y[i] = (Y[i] - L[i, :i].dot(Y[:i])) / L[i, i]
    return Y


def fisher_longdouble(spec, X, y_err):
    """F_p (4T, 4T) with factorisation, substitutions and sums in np.longdouble (the kernel values are float64); returned as float64"""
    n = len(X)
    if n > LONGDOUBLE_NMAX:
        raise ValueError("the long-double reference is meant for n <= %d" % LONGDOUBLE_NMAX)
    Ksum, Ds = derivative_matrices(spec, X)
    L = cholesky_ld(_noisy(Ksum, y_err, n))
    S = [forward_ld(L, forward_ld(L, D).T) for D in Ds]
    F = np.array([[np.sum(a * b) for b in S] for a in S], dtype=np.longdouble) * np.longdouble(0.5)
    return np.array(F, dtype=np.float64)


def rel_err(F, ref):
    """max |F - ref| / sqrt(ref_ii ref_jj); an entry that agrees exactly counts 0 whatever its scale (n = 1: the slopes are 0)"""
    d = np.sqrt(np.diag(ref))
    num = np.abs(np.asarray(F) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(num == 0.0, 0.0, num / np.outer(d, d))))


_CACHE = {}


def reference(tag, spec, X, y_err, longdouble):
    """the reference of a named case, computed once per (tag, n, noise, precision), shared and never changed"""
    key = (tag, len(X), y_err is not None, bool(longdouble))
    if key not in _CACHE:
        F = (fisher_longdouble if longdouble else fisher_f64)(spec, X, y_err)
        F.setflags(write=False)
        _CACHE[key] = F
    return _CACHE[key]

"""Inputs and dense NumPy references of the kernel-sum tests (include/tgp.h, seams S1s / S2s): used by test_ksum_host.py and
test_gpu_ksum.py.  Nothing here calls the library."""
import numpy as np

from _vk_loglik_grad_refs import TGP_RBF, TGP_ARBF, TGP_VK, abc, as_xy, kernel_and_slope, profile

SUM_A = ("0.3**2 * AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]])) + "
         "0.5**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))")
SUM_B = SUM_A + " + 0.2**2 * VonKarman(length_scale=0.4) + 0.7**2 * RBF(0.1)"     # four terms, every kind, the maximum count

_DATA = {}


def data(n, m=257):
    """X uniform on the unit square, y a smooth field plus noise, y_err in [0.02, 0.1], m query points; made once per (n, m)"""
    if (n, m) not in _DATA:
        rng = np.random.default_rng(4000 + 7 * n + m)
        X = rng.uniform(0, 1, (n, 2))
        y = np.sin(5 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.05 * rng.standard_normal(n)
        e = rng.uniform(0.02, 0.1, n)
        Xs = rng.uniform(0, 1, (m, 2))
        for a in (X, y, e, Xs):
            a.setflags(write=False)
        _DATA[(n, m)] = (X, y, e, Xs)
    return _DATA[(n, m)]


def spec_matrix(spec, X, Y=None):
    """amp k(X, Y) of one ops.KernelSpec on the host (scipy's Bessel functions for the von Karman kinds)"""
    X = as_xy(X)
    Y = X if Y is None else as_xy(Y)
    dx = X[:, None, 0] - Y[None, :, 0]
    dy = X[:, None, 1] - Y[None, :, 1]
    a, b, c = abc(spec.kind, spec.a, spec.b, spec.c, spec.ell)
    q = a * dx * dx + 2.0 * b * dx * dy + c * dy * dy
    if spec.kind in (TGP_RBF, TGP_ARBF):
        return spec.amp * np.exp(-0.5 * q)
    return spec.amp * profile(np.sqrt(np.maximum(q, 0.0)))[0]


def sum_matrix(sumspec, X, Y=None):
    out = spec_matrix(sumspec.terms[0], X, Y)
    for t in sumspec.terms[1:]:
        out = out + spec_matrix(t, X, Y)
    return out


def host_solve(K, y, e):
    """(alpha, logdet, y . alpha, K^-1) of K + diag(e^2)"""
    Kn = np.array(K, dtype=np.float64)
    Kn[np.diag_indices(len(Kn))] += np.asarray(e, dtype=np.float64) ** 2
    L = np.linalg.cholesky(Kn)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    Li = np.linalg.solve(L, np.eye(len(L)))
    return alpha, 2.0 * np.log(np.diag(L)).sum(), float(np.dot(y, alpha)), Li.T.dot(Li)


def host_grad_rows(sumspec, X, alpha, Kinv):
    """(nterms, 4): row t = 1/2 sum_ij (alpha_i alpha_j - [K^-1]_ij) dK_t,ij / d (log amp_t, a_t, b_t, c_t), K^-1 the SUM's"""
    M = np.outer(alpha, alpha) - Kinv
    rows = []
    for s in sumspec.terms:
        K, W, dx, dy = kernel_and_slope(s.kind, X, s.amp, s.a, s.b, s.c, s.ell)
        rows.append([(0.5 * M * K).sum(), (-0.25 * M * W * dx * dx).sum(), (-0.5 * M * W * dx * dy).sum(),
                     (-0.25 * M * W * dy * dy).sum()])
    return np.array(rows)


def spec_numbers(sumspec):
    """(log amp, a, b, c) of every term, flattened, in the convention of the likelihood gradient (VonKarman: a = c = 1 / ell^2)"""
    out = []
    for s in sumspec.terms:
        a, b, c = abc(s.kind, s.a, s.b, s.c, s.ell)
        out += [np.log(s.amp), a, b, c]
    return np.array(out)

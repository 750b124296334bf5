"""Dense NumPy reference of the likelihood gradient for all four kernel kinds (include/tgp.h, seam S2h): used by
test_vk_loglik_grad_host.py and test_gpu_vk_loglik_grad.py.  Nothing here calls the library.

With (dx, dy) = X_i - X_j, q = a dx^2 + 2 b dx dy + c dy^2, u = sqrt(q) (the isotropic von Karman kind: a = c = 1 / ell^2, b = 0),
K_ij = amp f(u), m_ij = alpha_i alpha_j - [(K + D)^-1]_ij:

    ref[0] =  1/2 sum_ij m_ij amp f(u_ij)
    ref[1] = -1/4 sum_ij m_ij amp w(u_ij) dx^2
    ref[2] = -1/2 sum_ij m_ij amp w(u_ij) dx dy
    ref[3] = -1/4 sum_ij m_ij amp w(u_ij) dy^2

f(u) = u^(5/6) K_{5/6}(2 pi u) / lim0 with f(0) = 1 is the reference's von Karman formula (treegp/kernels.py:253-262) and
w(u) = -f'(u) / u = 2 pi u^(-1/6) K_{1/6}(2 pi u) / lim0 (A&S 9.6.28), taken as 0 at u == 0, where dx = dy = 0 anyway; both from
scipy.special.kv, both 0 beyond the value's cutoff 2 pi u > K56_XMAX (they are below 1e-300 there).  For the Gaussian kinds
f = w = exp(-q / 2).  S[p] = sum_ij |term_ij| is the scale of each sum.
"""
import numpy as np
from scipy import linalg, special

K56_XMAX = 697.8738840444552
LIM0 = special.gamma(5.0 / 6.0) / (2.0 * np.pi ** (5.0 / 6.0))
TGP_RBF, TGP_ARBF, TGP_VK, TGP_AVK = 0, 1, 2, 3


def as_xy(X):
    X = np.asarray(X, dtype=float)
    if X.ndim == 1:
        X = X[:, None]
    return X if X.shape[1] == 2 else np.hstack([X, np.zeros((X.shape[0], 1))])


def profile(u):
    """(f, w) of an array u >= 0"""
    u = np.asarray(u, dtype=float)
    f, w = np.zeros(u.shape), np.zeros(u.shape)
    x = 2.0 * np.pi * u
    f[u == 0] = 1.0
    on = (u > 0) & (x <= K56_XMAX)
    f[on] = u[on] ** (5.0 / 6.0) * special.kv(5.0 / 6.0, x[on]) / LIM0
    w[on] = 2.0 * np.pi * u[on] ** (-1.0 / 6.0) * special.kv(1.0 / 6.0, x[on]) / LIM0
    return f, w


def abc(kind, a=0.0, b=0.0, c=0.0, ell=0.0):
    return (1.0 / ell ** 2, 0.0, 1.0 / ell ** 2) if kind == TGP_VK else (a, b, c)


def kernel_and_slope(kind, X, amp, a=0.0, b=0.0, c=0.0, ell=0.0):
    """(K, W, dx, dy): K_ij = amp f(u_ij), W_ij = amp w(u_ij) (the Gaussian kinds: both amp exp(-q / 2))"""
    X = as_xy(X)
    dx = X[:, None, 0] - X[None, :, 0]
    dy = X[:, None, 1] - X[None, :, 1]
    a, b, c = abc(kind, a, b, c, ell)
    q = a * dx * dx + 2.0 * b * dx * dy + c * dy * dy
    if kind in (TGP_RBF, TGP_ARBF):
        f = w = np.exp(-0.5 * q)
    else:
        f, w = profile(np.sqrt(np.maximum(q, 0.0)))
    return amp * f, amp * w, dx, dy


def solve_grad(kind, X, y, y_err, amp, a=0.0, b=0.0, c=0.0, ell=0.0):
    """(logdet, chi2, ref (4,), S (4,)) by a Cholesky solve and an explicit inverse; raises numpy.linalg.LinAlgError for a
    matrix that is not positive definite"""
    K, W, dx, dy = kernel_and_slope(kind, X, amp, a, b, c, ell)
    Kn = K + np.diag(np.asarray(y_err, dtype=float) ** 2)
    L = np.linalg.cholesky(Kn)
    z = linalg.solve_triangular(L, np.asarray(y, dtype=float), lower=True)
    alpha = linalg.solve_triangular(L.T, z, lower=False)
    Li = linalg.solve_triangular(L, np.eye(len(z)), lower=True)
    M = np.outer(alpha, alpha) - Li.T.dot(Li)
    terms = [0.5 * M * K, -0.25 * M * W * dx * dx, -0.5 * M * W * dx * dy, -0.25 * M * W * dy * dy]
    ref = np.array([t.sum() for t in terms])
    S = np.array([np.abs(t).sum() for t in terms])
    return 2.0 * np.log(np.diag(L)).sum(), z.dot(z), ref, S


def spec_solve_grad(spec, X, y, y_err):
    """the same for a treegp_amd.ops.KernelSpec"""
    return solve_grad(spec.kind, X, y, y_err, spec.amp, spec.a, spec.b, spec.c, spec.ell)


def log_likelihood(kind, X, y, y_err, amp, a=0.0, b=0.0, c=0.0, ell=0.0):
    K = kernel_and_slope(kind, X, amp, a, b, c, ell)[0]
    L = np.linalg.cholesky(K + np.diag(np.asarray(y_err, dtype=float) ** 2))
    z = linalg.solve_triangular(L, np.asarray(y, dtype=float), lower=True)
    return -0.5 * z.dot(z) - 0.5 * len(z) * np.log(2.0 * np.pi) - np.log(np.diag(L)).sum()


# ---- the inputs of the GPU tests (computed once per size, shared, never changed) -------------------------------------------------
AMP = 0.49
INVLAM = np.array([[40.0, -9.0], [-9.0, 25.0]])
SET_A = {"avk": "0.7**2 * AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]]))",
         "vk": "0.7**2 * VonKarman(length_scale=0.3)",
         "avk1d": "0.7**2 * AnisotropicVonKarman(scale_length=[0.2])"}


def data_a(n, nd=2):
    """input set A: X uniform on the unit square (or interval), y = sin 5x + 0.1 noise, y_err = 0.1 U(0.8, 1.2)"""
    rng = np.random.default_rng(100 + n)
    X = rng.uniform(0, 1, (n, nd))
    y = np.sin(5 * X[:, 0]) + 0.1 * rng.standard_normal(n)
    y_err = 0.1 * rng.uniform(0.8, 1.2, n)
    return X, y, y_err


MIN_SEP = 0.026


def data_ladder(n=300, seed=7):
    """The scale ladder's points: uniform on the unit square with a hard core of MIN_SEP between any two, the last point a copy of
    the first.  At s = 1e6 the smallest eigenvalue of invLam is 20.78e6, so every distinct pair has
    2 pi u >= 2 pi sqrt(20.78e6) MIN_SEP = 745 > K56_XMAX: the whole rung lies beyond the cutoff, which is what makes its
    slots 1 .. 3 exactly 0."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n - 1:
        p = rng.uniform(0, 1, 2)
        if all((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 >= MIN_SEP ** 2 for q in pts):
            pts.append(p)
    X = np.array(pts + [pts[0]])
    y = np.sin(5 * X[:, 0]) + 0.1 * rng.standard_normal(n)
    y[-1] = y[0] + 0.01
    y_err = 0.1 * rng.uniform(0.8, 1.2, n)
    return X, y, y_err

"""References and bounds for the gradient of the predicted mean (tgp_gp_predict_grad, seam S3g): used by
test_predict_grad_host.py and test_gpu_predict_grad.py.  Nothing here calls the library.

The quantity: gs[j] = sum_i t_ij, t_ij = alpha_i amp grad_x k(x - X_i) at x = Xs_j.  With d = Xs_j - X_i, M = invLam
(the isotropic von Karman kind: M = I / ell^2), q = d^T M d, u = sqrt(q):

    Gaussian kinds      t_ij = -alpha_i amp exp(-q / 2) M d
    von Karman kinds    t_ij = -alpha_i amp w(u) M d,   w(u) = -f'(u) / u = 2 pi u^(-1/6) K_{1/6}(2 pi u) / lim0,   0 at u == 0

(f(u) = u^(5/6) K_{5/6}(2 pi u) / lim0 and d/dx [x^nu K_nu(x)] = -x^nu K_{nu-1}(x).)  Three levels of reference:

  * mpmath: ``cov_mp`` restates the covariance formulas (treegp/kernels.py:114-126, 249-276, 355-381), ``pair_grad_mp`` the
    derivative above; the host test differentiates the former numerically (mpmath.diff) against the latter.
  * long double, vectorised: ``w_ld`` and ``grad_terms`` evaluate every pair of a call in x87 extended precision with the
    float64 inputs taken as exact; the host test checks them against mpmath.  K_{1/6} for x > 1 comes from the integral
    K_nu(x) = int_0^inf exp(-x cosh t) cosh(nu t) dt by the trapezoidal rule.  The integrand is even and analytic in the
    strip |Im t| < pi / 2, so the rule's error relative to e^-x is min over d < pi / 2 of exp(x (1 - cos d) - 2 pi d / h):
    exp(x - pi^2 / h) at the edge of the strip, exp(-2 pi^2 / (h^2 x)) at d = 2 pi / (h x) where that lies inside it; the
    step h = 0.65 / sqrt(x) for x > 38 (d = 1.57 there) and pi^2 / (x + 48) below keeps it under e^-46 = 1e-20.  For x <= 1:
    the ascending series.
  * ``grad_bound``: the tolerance of the device result, derived below from the number formats alone.
"""
import mpmath as mp
import numpy as np

from _kernel_value_helpers import K56_XMAX, LD, U53, _mpf_to_ld, diameter_exponent

KINDS = ("rbf", "arbf", "vk", "avk")
W_RTOL = 2e-13                   # the host test's criterion for w(u)


# ---------------------------------------------------------------------------------------------------------
# mpmath
def _lim0():
    nu = mp.mpf(5) / 6
    return mp.gamma(nu) / (2 * mp.pi ** nu)


def w_mp(u):
    """w(u) = 2 pi u^(-1/6) K_{1/6}(2 pi u) / lim0 for an mpf u > 0"""
    mu = mp.mpf(1) / 6
    return 2 * mp.pi * u ** (-mu) * mp.besselk(mu, 2 * mp.pi * u) / _lim0()


def form_mp(kind, p, dx, dy):
    """(a, b, c) of M as mpf and q = d^T M d"""
    if kind == "vk":
        a, b, c = 1 / mp.mpf(p["ell"]) ** 2, mp.mpf(0), 1 / mp.mpf(p["ell"]) ** 2
    else:
        a, b, c = mp.mpf(p["a"]), mp.mpf(p["b"]), mp.mpf(p["c"])
    return a, b, c, a * dx * dx + 2 * b * dx * dy + c * dy * dy


def cov_mp(kind, p, dx, dy):
    """amp k(d), the reference's formulas: exp(-q / 2); u^(5/6) K_{5/6}(2 pi u) / lim0 with u = |d| / ell (VonKarman) or
    sqrt(q) (AnisotropicVonKarman), 1 at u == 0"""
    a, b, c, q = form_mp(kind, p, dx, dy)
    amp = mp.mpf(p["amp"])
    if kind in ("rbf", "arbf"):
        return amp * mp.exp(-q / 2)
    u = mp.sqrt(dx * dx + dy * dy) / mp.mpf(p["ell"]) if kind == "vk" else mp.sqrt(q)
    if u == 0:
        return amp
    nu = mp.mpf(5) / 6
    return amp * u ** nu * mp.besselk(nu, 2 * mp.pi * u) / _lim0()


def pair_grad_mp(kind, p, dx, dy):
    """amp grad_d k(d) as two mpf: the closed form the device evaluates"""
    a, b, c, q = form_mp(kind, p, dx, dy)
    amp = mp.mpf(p["amp"])
    gx, gy = a * dx + b * dy, b * dx + c * dy
    if kind in ("rbf", "arbf"):
        s = mp.exp(-q / 2)
    else:
        u = mp.sqrt(q)
        s = w_mp(u) if u != 0 else mp.mpf(0)
    return -amp * s * gx, -amp * s * gy


# ---------------------------------------------------------------------------------------------------------
# long double
_SER = {}


def _series_constants(nser=18):
    if not _SER:
        old = mp.mp.dps
        mp.mp.dps = 40
        mu = mp.mpf(1) / 6
        lim0 = _lim0()
        _SER["a"] = [_mpf_to_ld(1 / (mp.factorial(k) * mp.rf(1 - mu, k))) for k in range(nser)]
        _SER["b"] = [_mpf_to_ld(1 / (mp.factorial(k) * mp.rf(1 + mu, k))) for k in range(nser)]
        _SER["c1"] = _mpf_to_ld(2 * mp.pi ** 2 * mp.pi ** (-mu) / (mp.gamma(1 - mu) * lim0))
        _SER["c2"] = _mpf_to_ld(2 * mp.pi ** 2 * mp.pi ** mu / (mp.gamma(1 + mu) * lim0))
        _SER["pre"] = _mpf_to_ld(2 * mp.pi / lim0)
        _SER["pi"] = _mpf_to_ld(mp.pi)
        mp.mp.dps = old
    return _SER


def w_ld(u):
    """w(u) for an array of long doubles u >= 0: 0 at u == 0 (never used there) and for 2 pi u > K56_XMAX"""
    k = _series_constants()
    u = np.asarray(u, LD)
    x = 2 * k["pi"] * u
    out = np.zeros(u.shape, LD)
    small = (u > 0) & (x <= 1)
    if small.any():
        us = u[small]
        t = (k["pi"] * us) ** 2
        sa = np.full(us.shape, k["a"][-1], LD)
        sb = np.full(us.shape, k["b"][-1], LD)
        for ca, cb in zip(k["a"][-2::-1], k["b"][-2::-1]):
            sa = sa * t + ca
            sb = sb * t + cb
        out[small] = k["c1"] / np.cbrt(us) * sa - k["c2"] * sb
    big = (x > 1) & (x <= LD(K56_XMAX))
    if big.any():
        ub, xb = u[big], x[big]
        h = np.where(xb > 38, LD(0.65) / np.sqrt(xb), k["pi"] ** 2 / (xb + 48))
        tmax = np.arccosh(1 + LD(50.0) / xb)                 # beyond it the integrand is below e^-50 of its peak
        need = np.ceil((tmax / h).astype(float)).astype(np.int64) + 1
        acc = np.full(xb.shape, LD(0.5), LD)                   # t = 0: cosh(0) / 2
        order = np.argsort(need)
        for part in np.array_split(order, 8):                  # (elements that need few nodes do not pay for the others')
            if len(part) == 0:
                continue
            xp, hp, ap = xb[part], h[part], acc[part]
            for j in range(1, int(need[part].max())):
                t = j * hp
                ap += np.exp(-2 * xp * np.sinh(t / 2) ** 2) * np.cosh(t / 6)  # exp(-x (cosh t - 1)) cosh(t / 6)
            acc[part] = ap
        out[big] = k["pre"] * np.exp(-xb) * (acc * h) / np.cbrt(np.sqrt(ub))  # 2 pi u^(-1/6) K / lim0
    return out


def _params(kind, p):
    if kind == "vk":
        e2 = LD(1.0) / (LD(p["ell"]) * LD(p["ell"]))
        return e2, LD(0.0), e2
    return LD(p["a"]), LD(p["b"]), LD(p["c"])


def grad_terms(kind, p, X, alpha, Xs):
    """t[i, j, :] for every pair of a call in long double, with the magnitudes the bound needs: dict with
    T (n, m, 2), k (n, m) = exp(-q/2) or w(u), A (n, m, 2) = (|a dx| + |b dy|, |b dx| + |c dy|), q and Qbar
    (= |dx| A_x + |dy| A_y >= q: the sum of the magnitudes of the products in q), x = 2 pi u (von Karman)."""
    X, Xs = np.asarray(X, float), np.asarray(Xs, float)
    a, b, c = _params(kind, p)
    dx = LD(Xs[None, :, 0]) - LD(X[:, None, 0])
    dy = LD(Xs[None, :, 1]) - LD(X[:, None, 1])
    gx, gy = a * dx + b * dy, b * dx + c * dy
    A = np.stack([np.abs(a * dx) + np.abs(b * dy), np.abs(b * dx) + np.abs(c * dy)], axis=2)
    q = dx * gx + dy * gy
    Qbar = np.abs(dx) * A[..., 0] + np.abs(dy) * A[..., 1]
    out = {"A": A, "q": q, "Qbar": Qbar}
    if kind in ("rbf", "arbf"):
        kv = np.exp(-q / 2)
    else:
        u = np.sqrt(np.maximum(q, 0))
        kv = w_ld(u)
        out["x"] = 2 * _series_constants()["pi"] * u
    s = -(LD(p["amp"]) * LD(np.asarray(alpha, float))[:, None]) * kv
    out["k"] = kv
    out["T"] = np.stack([s * gx, s * gy], axis=2)
    return out


# ---------------------------------------------------------------------------------------------------------
# the bound
LIN = 4.0


def pair_slack(kind, p, X, alpha, Xs, terms, fast, S=None):
    """E_ijc |t_ijc| (n, m, 2), long double: the evaluation error of one pair's contribution in units of 2^-53, so that

        |g_jc - ref_jc| <= 2^-53 sum_i (n + E_ijc) |t_ijc|

    n 2^-53 sum |t| is the worst case of a sum of n rounded terms in any order.  E_ijc has three parts.

    (1) The scalar factor, relative: E_val |t_ijc|.
        Gaussian, differences first (generic route): E_val = 8 + 16 Qbar / 2 -- the value's pair bound of
        _kernel_value_helpers.gauss_bound with the term magnitude standing in for s, as its term_magnitude does: the exponent
        q / 2 is a sum of products each rounded relative to its own size, exp turns its absolute error into a relative one;
        8 covers exp (<= 2 ulp), the products by alpha and amp and the constants.
        Gaussian fast path: E_val = 8 + 16 sqrt(s S), s = q / 2, S = the exponent across the diameter of the points of the call
        (gauss_bound; the transformed coordinates are rounded relative to sqrt(S) before the difference is taken).
        von Karman: E_val = W_RTOL 2^53 + 8 + (2 + x) (1.5 + 2.25 Qbar / q), x = 2 pi u.  W_RTOL is the host test's criterion
        for w.  The argument: q carries <= 4.5 Qbar 2^-53 (dx, dy half an ulp each, M d three, the products and the sum one),
        u = sqrt(q) half of that relatively plus one, the isotropic kind's 1 / ell half more; w turns a relative error of u
        into |d ln w / d ln u| = 1/3 + x K_{5/6}(x) / K_{1/6}(x) <= 2 + x of its own (K_{5/6} / K_{1/6} <= 1 + 1 / x).
    (2) The vector factor M d.  Its components are sums of two products that may cancel (a sheared invLam: a dx + b dy), so
        their error is relative to A_c = |a dx| + |b dy|, not to the component: LIN A_c per unit of the scalar factor, LIN = 4
        (dx, dy: 1/2 each; two products and a sum: 1.5; the reduction's multiply by -amp or by T^T, whose entries are rounded
        themselves: 1.5).  In the form above this is E |t_c| with the condition number A_c / |(M d)_c| in E; it is kept as a
        product so that a vanishing component is no division by zero.  The fast path computes M d = L v from the transformed
        difference v = L^T d: relative to sum_c' |L_cc'| |v_c'| instead.
    (3) Fast path only: v is the difference of coordinates that were transformed and ROUNDED first.  A point p carries
        <= 3 2^-53 mag(p), mag_0 = |l00 x'| + |l10 y'|, mag_1 = |l11 y'|, (x', y') = p - origin (x': 1/2, the entries of T:
        1.5, the product and the sum: 1), so v_c' carries 3 (mag_c'(X_i) + mag_c'(Xs_j)) + |v_c'| / 2, and the term
        |alpha amp k| sum_c' |L_cc'| times that.  With the training point that serves as origin mag = 0: identical points
        have v = 0 exactly.
    """
    T, kv, A, q, Qbar = terms["T"], terms["k"], terms["A"], terms["q"], terms["Qbar"]
    absT = np.abs(T)
    scal = np.abs(LD(p["amp"]) * LD(np.asarray(alpha, float))[:, None] * kv)           # |alpha amp k|
    if kind in ("rbf", "arbf") and fast:
        s = np.maximum(q / 2, 0)
        e_val = LD(8.0) + LD(16.0) * np.sqrt(s * np.maximum(LD(S), s))
    elif kind in ("rbf", "arbf"):
        e_val = LD(8.0) + LD(16.0) * Qbar / 2
    else:
        ratio = np.where(q > 0, Qbar / np.where(q > 0, q, 1), LD(1.0))
        e_val = LD(W_RTOL) / LD(U53) + LD(8.0) + (LD(2.0) + terms["x"]) * (LD(1.5) + LD(2.25) * ratio)
    out = e_val[..., None] * absT
    if not fast:
        return out + LD(LIN) * scal[..., None] * A
    a, b, c = float(p["a"]), float(p["b"]), float(p["c"])
    l00 = np.sqrt(a)
    l10 = b / l00
    l11 = np.sqrt(max(c - l10 * l10, 0.0))
    Lm = np.abs(np.array([[l00, 0.0], [l10, l11]]))            # |L|: (M d)_c = sum_c' L_cc' v_c'
    X, Xs = np.asarray(X, float), np.asarray(Xs, float)

    def mags(P):
        d = LD(P) - LD(X[0])
        return np.stack([np.abs(l00 * d[:, 0]) + np.abs(l10 * d[:, 1]), np.abs(l11 * d[:, 1])], axis=1)
    mi, mj = mags(X), mags(Xs)
    dx = LD(Xs[None, :, 0]) - LD(X[:, None, 0])
    dy = LD(Xs[None, :, 1]) - LD(X[:, None, 1])
    v = np.stack([np.abs(l00 * dx + l10 * dy), np.abs(l11 * dy)], axis=2)
    dv = 3 * (mi[:, None, :] + mj[None, :, :]) + v / 2
    mix = (LD(LIN) * v + dv) @ LD(Lm.T)                         # [..., c] = sum_c' |L_cc'| (LIN |v_c'| + dv_c')
    return out + scal[..., None] * mix


def grad_bound(n, absT_sum, slack_sum):
    """2^-53 (n sum_i |t_ijc| + sum_i E_ijc |t_ijc|) from the two sums over i"""
    return LD(U53) * (LD(float(n)) * absT_sum + slack_sum)


def call_exponent(kind, p, X, Xs):
    """S of gauss_bound for the points of one call (the fast path's only)"""
    return diameter_exponent(np.vstack([X, Xs]), float(p["a"]), float(p["b"]), float(p["c"]))


def takes_fast_path(kind, p):
    """launch_predict_grad's condition (TGP_PREDICT_GENERIC aside): a Gaussian kind whose invLam has a Cholesky factor"""
    if kind not in ("rbf", "arbf") or not p["a"] > 0:
        return False
    return p["c"] - (p["b"] / np.sqrt(p["a"])) ** 2 >= 0

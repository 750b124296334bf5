"""Leave-one-out (LOO) quantities of a GP from alpha = K^-1 r and d = diag(K^-1) (Rasmussen & Williams 2006, section 5.4.2,
eqs. 5.10-5.12; not in the reference).  K = amp k(X, X) + diag(sigma^2) is the noisy covariance the library factorises, r the
residual it was solved for.  Point i left out of the other n - 1:

    mu_i = r_i - alpha_i / d_i                                 LOO mean of r_i
    s_i  = 1 / d_i                                             noisy predictive variance (of y_i)
    v_i  = 1 / d_i - sigma_i^2                                 latent predictive variance (what predict(X, return_var=True) means)
    log p(y_i | y_-i) = -1/2 log 2 pi + 1/2 log d_i - 1/2 alpha_i^2 / d_i

O(n) on the host; d comes from the device (ops.factor_inv_diag).
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

"""Realisations of Gaussian random fields, drawn on the GPU.

The reference makes every one of its test inputs as ``np.random.multivariate_normal(np.zeros(n), kernel(x))``
(tests/treegp_test_helper.py:64-66, 95-97): an SVD of the dense n x n matrix on the host.  Here the covariance is
factorised on the device (``ops.gp_solve`` keeps the packed factor; K never leaves the device for the kernels
``kernel_to_spec`` accepts) and standard normals z become y = L z (``ops.factor_lmul``, seam S3d of include/tgp.h).

The normals come from NumPy: ``np.random.default_rng(random_state).standard_normal((n_samples, n))``, row v for
realisation v, so that every result can be reproduced from NumPy alone and one sample equals the first of five.

One GPU only: the factorisation and the product run on this process's context even when the multi-GPU route is enabled
(``treegp_amd.dist``); sampling over several GPUs is not provided.
"""
import numpy as np
from sklearn.gaussian_process.kernels import Exponentiation, KernelOperator

from . import _lib
from . import ops
from . import kernels as _kernels
from .kernels import _CholeskyParametrised, eval_kernel


def check_sampling_args(n_samples, nugget):
    if int(n_samples) != n_samples or n_samples < 1:
        raise ValueError("n_samples must be a positive integer, got %r" % (n_samples,))
    if not nugget >= 0:
        raise ValueError("nugget must be >= 0, got %r" % (nugget,))


def _kernel_ndims(kernel):
    """the coordinate dimensions the leaves of a kernel tree insist on (empty: any)"""
    if isinstance(kernel, KernelOperator):
        return _kernel_ndims(kernel.k1) | _kernel_ndims(kernel.k2)
    if isinstance(kernel, Exponentiation):
        return _kernel_ndims(kernel.kernel)
    if isinstance(kernel, _CholeskyParametrised):
        return {kernel.ndim}
    ls = getattr(kernel, "length_scale", None)
    if ls is not None and np.iterable(ls) and len(ls) > 1:
        return {len(ls)}
    return set()


def as_coords(kernel, X):
    """X as (n, d) float64; ValueError when d is not what the kernel describes"""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.ndim != 2 or len(X) < 1:
        raise ValueError("X must be (n_points, n_dims) with at least one point, got shape %s" % (X.shape,))
    want = _kernel_ndims(kernel)
    if want and want != {X.shape[1]}:
        raise ValueError("X has %d columns, the kernel %r describes %s-dimensional coordinates"
                         % (X.shape[1], kernel, "/".join(str(d) for d in sorted(want))))
    return X


def prior_diag_max(kernel, X):
    """max over X of k(x, x): amp for the parametrised kernels (the sum of the amplitudes for a sum of them),
    max(kernel.diag(X)) for any other kernel tree"""
    try:
        return _kernels.device_spec(kernel, ndim=np.shape(X)[1] if np.ndim(X) == 2 else 1).amp
    except NotImplementedError:
        return float(np.max(kernel.diag(X)))


def normals(n_samples, n, random_state):
    return np.random.default_rng(random_state).standard_normal((int(n_samples), n))


def not_positive_definite(exc, nugget):
    return np.linalg.LinAlgError("the covariance to sample from is not positive definite (%s); raise nugget (now %g, "
                                 "the jitter added to its diagonal in units of max k(x, x))" % (exc, nugget))


def lmul_dense(C, Z, nugget):
    """Z (n_samples, n) -> (L Z^T)^T with L the Cholesky factor of the host matrix C, factorised on this process's GPU"""
    ctx = _lib.get_ctx()
    try:
        factor = ops.gp_solve_dense(C, np.zeros(len(C)), None, keep=True, want_alpha=False, ctx=ctx)[3]
    except np.linalg.LinAlgError as exc:
        raise not_positive_definite(exc, nugget)
    try:
        return ops.factor_lmul(factor, Z, ctx=ctx)
    finally:
        factor.free()


def gaussian_random_field(kernel, X, n_samples=1, random_state=0, y_err=None, nugget=1e-10):
    """Realisations of a zero-mean Gaussian random field with covariance K + diag(y_err^2) + jitter I at the points X,
    K = kernel(X) and jitter = nugget * max k(x, x).  What the reference does with np.random.multivariate_normal(0, K).

    :param kernel:       kernel string (``eval_kernel``) or scikit-learn kernel object.
    :param X:            coordinates (n, 1, 2 or 3), or (n,) for 1-D.
    :param n_samples:    number of realisations.
    :param random_state: seed of ``np.random.default_rng``; realisation v is L z with z the v-th row of
                         ``default_rng(random_state).standard_normal((n_samples, n))``.
    :param y_err:        per-point noise added in quadrature (None: none).
    :param nugget:       jitter on the diagonal, relative to max k(x, x); the knob to raise when the factorisation fails.
    :returns:            (n, n_samples) array, scikit-learn's ``sample_y`` layout.

    Raises numpy.linalg.LinAlgError when the covariance is not positive definite, ValueError for n_samples < 1,
    nugget < 0 or X that does not match the kernel.  Runs on one GPU (the multi-GPU route is not used).
    """
    if isinstance(kernel, str):
        kernel = eval_kernel(kernel)
    check_sampling_args(n_samples, nugget)
    X = as_coords(kernel, X)
    n = len(X)
    e2 = np.zeros(n) if y_err is None else np.asarray(y_err, dtype=np.float64) ** 2
    if e2.shape != (n,):
        raise ValueError("y_err must have one value per point (%d), got shape %s" % (n, e2.shape))
    jitter = nugget * prior_diag_max(kernel, X)
    Z = normals(n_samples, n, random_state)
    try:
        spec = _kernels.device_spec(kernel, ndim=X.shape[1])
    except NotImplementedError:
        spec = None
    if spec is None:
        # any other scikit-learn kernel tree evaluates itself on the host; the device factorises what it returns
        K = np.array(kernel(X), dtype=np.float64)
        K[np.diag_indices(n)] += e2 + jitter
        Y = lmul_dense(K, Z, nugget)
    else:
        # K is built and factorised on the device and never leaves it
        ctx = _lib.get_ctx()
        try:
            factor = ops.gp_solve(spec, X, np.zeros(n), np.sqrt(e2 + jitter), keep=True, want_alpha=False, ctx=ctx)[3]
        except np.linalg.LinAlgError as exc:
            raise not_positive_definite(exc, nugget)
        try:
            Y = ops.factor_lmul(factor, Z, ctx=ctx)
        finally:
            factor.free()
    return np.ascontiguousarray(Y.T)

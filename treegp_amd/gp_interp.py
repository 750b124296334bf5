"""``GPInterpolation`` with treegp's constructor / initialize / solve / predict API, running the
kernel-matrix build, Cholesky solve and prediction on the GPU.

Mirrors ``treegp/gp_interp.py:15-291`` of the reference (plotting, :293-377, is out of scope).
State and cache semantics are the reference's: ``_alpha`` is computed on the first ``predict``
and invalidated by ``initialize`` (:227) and ``_fit`` (:119); ``predict`` works without
``solve``; ``normalize`` uses the mean of ``y - spatial_average`` taken before white noise is
folded in (:217-224); a mean-function table counts as present when X0 is not all zeros (:235).
"""
import copy

import numpy as np
from sklearn.neighbors import KNeighborsRegressor

from . import kernels as _kernels
from . import ops
from .fits_io import read_bintable_row
from .kernels import eval_kernel, kernel_to_spec
from .loo import group_runs, lgo_quantities, loo_quantities


def _three_d(X):
    """coordinates with three columns: the ``3`` entries of include/tgp.h (ops.KernelSpec3)"""
    return np.ndim(X) == 2 and np.shape(X)[1] == 3


class GPInterpolation(object):
    """Gaussian-process interpolation of one scalar field over 1-D / 2-D / 3-D coordinates.  3-D coordinates (position plus
    time, position plus colour) take the device route by themselves for the four parametrised kernels (``kernels.kernel_to_spec3``)
    with ``optimizer`` "none" or "log-likelihood"; the 2-point-correlation optimisers and a mean-function table are 2-D
    statistics and raise ValueError for them.

    :param kernel:        string that ``eval_kernel`` turns into a scikit-learn kernel. [default 'RBF(1)']
    :param optimizer:     "none", "two-pcf", "anisotropic", "log-likelihood" or "local-likelihood" (not in the reference:
                          L-BFGS-B on Vecchia's approximation of the likelihood, ``local_likelihood.py``; linear in n, no
                          n x n factor; 1-D / 2-D coordinates and one parametrised kernel).
    :param normalize:     subtract the mean of the data before interpolating. [default True]
    :param p0:            start point (size, g1, g2) of the anisotropic 2-pcf fit.
    :param white_noise:   extra uncorrelated noise added in quadrature to y_err. [default 0.]
    :param n_neighbors:   neighbours of the KNN interpolation of the mean function. [default 4]
    :param average_fits:  FITS table (meanify output) holding the mean function. [default None]
    :param indice_meanify: column of the mean function to use when it has several.
    :param nbins, min_sep, max_sep: binning of the 2-point correlation function.
    :param local_k, local_seed: neighbours per row and seed of the random ordering of "local-likelihood"; the other
                          optimisers do not look at them. [default 64, 0]
    :param backend:       not in the reference.  None: one GPU, unless the multi-GPU route is enabled
                          (``treegp_amd.dist.enable()`` or TGP_DIST=1 under ``torchrun``) and the problem is at least its
                          size threshold; "dist": always the multi-GPU route (row-block-cyclic Cholesky over the ranks of
                          torch.distributed, query points sharded; every rank makes the same calls with the same data and
                          gets the same results); "single": always this rank's GPU alone.
    """

    def __init__(self, kernel="RBF(1)", optimizer="two-pcf", normalize=True, p0=[3000.0, 0.0, 0.0],
                 white_noise=0.0, n_neighbors=4, average_fits=None, indice_meanify=None, nbins=20,
                 min_sep=None, max_sep=None, backend=None, local_k=64, local_seed=0):
        if backend not in (None, "dist", "single"):
            raise ValueError("backend must be None, 'dist' or 'single'. Current value: %s" % (backend,))
        self.backend = backend
        self.normalize, self.optimizer, self.white_noise = normalize, optimizer, white_noise
        self.n_neighbors, self.indice_meanify = n_neighbors, indice_meanify
        self.nbins, self.min_sep, self.max_sep = nbins, min_sep, max_sep
        self.local_k, self.local_seed = local_k, local_seed
        self.robust_fit = optimizer == "anisotropic"       # the 2-D fit of (size, g1, g2) goes with the TwoD pcf
        self.p0_robust_fit = p0

        if not isinstance(kernel, str):
            raise TypeError("kernel should be a string a list or a numpy.ndarray of string")
        self.kernel_template = eval_kernel(kernel)

        if optimizer not in ("anisotropic", "two-pcf", "log-likelihood", "local-likelihood", "none"):
            raise ValueError("Only anisotropic, two-pcf, log-likelihood, local-likelihood and none are supported for optimizer. "
                             "Current value: %s" % (optimizer))

        # mean function: the meanify table (gp_interp.py:97-107, read there with fitsio) or none yet
        self._X0 = self._y0 = None
        if average_fits is not None:
            table = read_bintable_row(average_fits)
            self._X0, self._y0 = table["COORDS0"], table["PARAMS0"]
        self._alpha = None
        self._factor = self._factor_key = None

    def _scope(self):
        """the backend choice of this object, in force for the solves made inside (treegp_amd.dist.scope)"""
        if self.backend is None:
            import contextlib
            return contextlib.nullcontext()
        from . import dist
        return dist.scope(self.backend)

    # -- hyper-parameter fit ---------------------------------------------------------------------
    def _fit(self, kernel, X, y, y_err):
        """Run the requested optimiser on the (mean-subtracted) data and return the fitted kernel; the
        cached solution is dropped either way (gp_interp.py:111-141)."""
        from .two_pcf import two_pcf
        from .log_likelihood import log_likelihood
        self._drop_solution()
        if self.optimizer in ("two-pcf", "anisotropic"):
            self._optimizer = two_pcf(X, y, y_err, self.min_sep, self.max_sep, nbins=self.nbins,
                                      anisotropic=(self.optimizer == "anisotropic"),
                                      robust_fit=self.robust_fit, p0=self.p0_robust_fit)
        elif self.optimizer == "log-likelihood":
            self._optimizer = log_likelihood(X, y, y_err)
        elif self.optimizer == "local-likelihood":
            from .local_likelihood import local_likelihood
            self._optimizer = local_likelihood(X, y, y_err, k=self.local_k, seed=self.local_seed)
        else:
            return kernel
        return self._optimizer.optimizer(kernel)

    def _drop_solution(self):
        self._alpha = None
        self._set_factor(None, None)

    def __del__(self):
        # a dropped object hands its factor's memory to the context (the next fit of this size allocates nothing: at N = 65 536
        # a hipFree + hipMalloc of 17 GB between two fits otherwise); raw ops.Factor handles free their memory by default
        try:
            self._set_factor(None, None)
        except Exception:
            pass

    def _set_factor(self, factor, key):
        if getattr(self, "_factor", None) is not None:
            self._factor.free(keep_memory=True)        # a refit of this object solves the same size next: its memory is reused
        self._factor, self._factor_key = factor, key

    def _device_spec(self, kernel, n=None):
        """The device description of ``kernel`` for the single-problem routes: ``kernel_to_spec``'s, or else a sum's
        (``kernels.device_spec``: 2 .. 4 parametrised terms, ``ops.KernelSumSpec``); NotImplementedError for every other
        tree, which takes the dense route.  The multi-GPU engine has no sum-aware K build: while it would take a problem of
        ``n`` points (this object's backend included), sums keep the dense route too."""
        with self._scope():
            multi_gpu = ops._dist_engine(len(self._X) if n is None else n, None) is not None
        if _three_d(self._X):
            # ops.KernelSpec3; the multi-GPU engine has no 3-D K build and sums of 3-D kernels no device form: the dense route,
            # where the kernel object evaluates itself through ops.kernel_matrix
            if multi_gpu:
                raise NotImplementedError("3-D coordinates keep the dense route under the multi-GPU engine")
            return _kernels.device_spec(kernel, ndim=3)
        return _kernels.device_spec(kernel, allow_sum=not multi_gpu, single=kernel_to_spec)

    @staticmethod
    def _factor_fingerprint(spec, X1, y_err):
        import hashlib
        h = hashlib.blake2b(digest_size=16)
        for term in getattr(spec, "terms", [spec]):          # a sum: every term
            if isinstance(term, ops.KernelSpec3):
                h.update(np.asarray((3.0, term.kind, term.amp, term.ell) + term.m, dtype=np.float64).tobytes())
                continue
            h.update(np.asarray([term.kind, term.amp, term.a, term.b, term.c, term.ell], dtype=np.float64).tobytes())
        for arr in (X1, y_err):
            arr = np.ascontiguousarray(arr, dtype=np.float64)
            h.update(str(arr.shape).encode())
            h.update(arr.tobytes())
        return h.digest()

    @staticmethod
    def _dense_fingerprint(kernel, X1, y_err):
        import hashlib
        h = hashlib.blake2b(digest_size=16)
        h.update(repr(kernel).encode())
        h.update(np.asarray(kernel.theta, dtype=np.float64).tobytes())
        for arr in (X1, y_err):
            arr = np.ascontiguousarray(arr, dtype=np.float64)
            h.update(str(arr.shape).encode())
            h.update(arr.tobytes())
        return h.digest()

    def _ensure_solution(self, y, X1, kernel, spec, y_err, want_factor):
        """The cached ``_alpha`` (solved for when None) and, for want_factor, a kept factor of K + diag(y_err^2) that matches
        its fingerprint.  spec: the device description of the kernel, None for the dense route (scikit-learn evaluates K).
        The reference caches only alpha (computed when it is None, whatever the arguments: gp_interp.py:179) and rebuilds
        K + diag(y_err^2) from its ARGUMENTS for every covariance request (:186-187).  The factor kept on the device therefore
        carries the fingerprint of what it was built from and is rebuilt when that differs; alpha stays the cached one."""
        if spec is not None:
            key = self._factor_fingerprint(spec, X1, y_err) if want_factor else None
            if self._alpha is None:
                self._alpha, _, _, factor = ops.gp_solve(spec, X1, y, y_err, keep=want_factor)
                self._set_factor(factor, key)
            elif want_factor and (self._factor is None or self._factor_key != key):
                factor = ops.gp_solve(spec, X1, y, y_err, keep=True)[3]
                self._set_factor(factor, key)
            return
        key = self._dense_fingerprint(kernel, X1, y_err) if want_factor else None
        need_alpha = self._alpha is None
        if need_alpha or (want_factor and (self._factor is None or self._factor_key != key)):
            alpha, _, _, factor = ops.gp_solve_dense(kernel(X1), y, y_err, keep=want_factor)
            if need_alpha:
                self._alpha = alpha
            self._set_factor(factor, key)

    # -- prediction ------------------------------------------------------------------------------
    def predict(self, X, return_cov=False, return_var=False):
        """Interpolated values (and optionally the posterior covariance) at X (n_samples, 1 or 2).
        gp_interp.py:143-166: the GP acts on y - mean - mean function; both are added back.
        Not in the reference: ``return_var=True`` returns (y, var) with var (n_samples,) = the diagonal of what
        ``return_cov=True`` returns, without forming the covariance (any number of points; not clamped at zero)."""
        if return_cov and return_var:
            raise ValueError("at most one of return_cov and return_var may be True")
        residual = self._y - self._mean - self._spatial_average
        with self._scope():
            y_star, y_unc = self.return_gp_predict(residual, self._X, X, self.kernel, y_err=self._y_err,
                                                   return_cov=return_cov, return_var=return_var)
        y_star = y_star + (self._mean + self._build_average_meanify(X))
        return (y_star, y_unc) if (return_cov or return_var) else y_star

    def return_gp_predict(self, y, X1, X2, kernel, y_err, return_cov=False, return_var=False):
        """gp_interp.py:168-194 on the GPU: fused K build + Cholesky + solve (tgp_gp_solve), fused
        cross-kernel mat-vec (tgp_gp_predict) and, for return_cov, Kss - HT K^-1 HT^T from the
        factor kept on the device (tgp_gp_predict_cov) instead of a second factorisation; for return_var
        its diagonal alone from the same kept factor (tgp_gp_predict_var)."""
        if return_cov and return_var:
            raise ValueError("at most one of return_cov and return_var may be True")
        try:
            spec = self._device_spec(kernel, len(X1))
        except NotImplementedError:
            # any other scikit-learn kernel tree (WhiteKernel, Matern, sums beyond kernels.kernel_to_sum_spec, ...): the kernel object evaluates itself on
            # the host, exactly as in the reference, and the device factorises what it returns (tgp_gp_solve_dense)
            return self._return_gp_predict_dense(y, X1, X2, kernel, y_err, return_cov, return_var)
        self._ensure_solution(y, X1, kernel, spec, y_err, want_factor=return_cov or return_var)
        y_predict = ops.gp_predict(spec, X1, self._alpha, X2)
        if return_cov:
            y_cov = ops.gp_predict_cov(spec, self._factor, X1, X2)
            return y_predict, y_cov
        if return_var:
            return y_predict, ops.gp_predict_var(spec, self._factor, X1, X2)
        return y_predict, None

    def _return_gp_predict_dense(self, y, X1, X2, kernel, y_err, return_cov, return_var=False):
        """gp_interp.py:177-192 for a kernel only scikit-learn can evaluate: HT, K and k(X2) come from ``kernel.__call__``
        on the host; factorisation, solve and the posterior covariance run on the device.  For return_var the diagonal
        of k(X2) is ``kernel.diag(X2)`` (WhiteKernel's noise included, as in diag(kernel(X2)))."""
        HT = kernel(X2, Y=X1)
        self._ensure_solution(y, X1, kernel, None, y_err, want_factor=return_cov or return_var)
        y_predict = np.dot(HT, self._alpha.reshape((len(self._alpha), 1))).T[0]
        if return_cov:
            return y_predict, ops.gp_predict_cov_dense(self._factor, HT, kernel(X2))
        if return_var:
            return y_predict, ops.gp_predict_var_dense(self._factor, HT, kernel.diag(X2))
        return y_predict, None

    def predict_gradient(self, X):
        """Spatial derivative of the interpolated field at X (n_samples, 1, 2 or 3): (n_samples, ndim), column c the derivative
        along coordinate c of the GP part of what ``predict(X)`` returns, from the kernel's analytic derivative
        (ops.gp_predict_grad) instead of differences of ``predict`` at shifted points.  Not in the reference.  The constant
        ``_mean`` of ``normalize`` drops out; a KNN mean function is piecewise constant and contributes nothing (its jumps
        between neighbourhoods are not a slope).  A von Karman field has a cusp on every star: the slope reported there is
        zero.  Uses the cached ``_alpha`` under the rules of ``predict`` (solved for on first use, no factor is kept).
        Kernels of the dense route (anything ``kernels.device_spec`` does not describe: one parametrised kernel or a sum of up
        to four) have no device form of their derivative: NotImplementedError.  Runs on one GPU whichever backend solved."""
        try:
            spec = _kernels.device_spec(self.kernel, single=kernel_to_spec, ndim=3 if _three_d(self._X) else 2)
        except NotImplementedError:
            raise NotImplementedError("predict_gradient needs a kernel with a device form (RBF, AnisotropicRBF, VonKarman, "
                                      "AnisotropicVonKarman, optionally times a constant, or a sum of up to four of those); "
                                      "got %r" % (self.kernel,))
        with self._scope():
            solve_spec = spec
            if isinstance(spec, (ops.KernelSumSpec, ops.KernelSpec3)) and ops._dist_engine(len(self._X), None) is not None:
                solve_spec = None                               # a sum or a 3-D object under the multi-GPU engine is solved on the dense route
            self._ensure_solution(self._residual(), self._X, self.kernel, solve_spec, self._y_err, want_factor=False)
        ndim = 1 if np.ndim(X) < 2 else np.shape(X)[1]
        return ops.gp_predict_grad(spec, self._X, self._alpha, X)[:, :ndim]

    def predict_local(self, X, k=64, return_var=False, return_neighbors=False):
        """Local kriging at X (n_samples, 1 or 2): every point is predicted from its ``k`` nearest stars alone -- nearest in the
        kernel's own metric -- instead of from one dense factorisation of all of them (ops.gp_predict_local, seam S3l of
        include/tgp.h).  Not in the reference.  Linear in the number of points, no n x n matrix: with the 2-point-correlation
        optimisers (which need no factorisation either) ``initialize`` -> ``solve`` -> ``predict_local`` serves catalogues of
        10^5 - 10^6 stars that ``predict`` cannot hold.  Residual, ``_mean`` and the mean function are handled exactly as in
        ``predict``: the GP acts on y - _mean - mean function and both are added back.  ``k`` in 1 .. 128, clipped to the number of
        stars; with ``k`` >= that number the result is the exact GP's.  ``return_var``: also the variance of each local problem
        (not clamped at zero; it is never below the exact GP's, which conditions on more).  ``return_neighbors``: also the
        (n_samples, min(k, n)) rows of the stars used, nearest first.  ``_alpha`` and a kept factor are neither used nor
        touched.  Raises numpy.linalg.LinAlgError naming the first point whose local matrix is not positive definite, and
        NotImplementedError for 3-D coordinates, sums of kernels and the kernels of the dense route.  Runs on one GPU whichever
        backend is set."""
        if _three_d(self._X) or _three_d(X):
            raise NotImplementedError("predict_local takes 1-D or 2-D coordinates: the neighbour search has no 3-D form")
        try:
            spec = _kernels.device_spec(self.kernel, single=kernel_to_spec)
        except NotImplementedError:
            raise NotImplementedError("predict_local needs one kernel with a device form (RBF, AnisotropicRBF, VonKarman, "
                                      "AnisotropicVonKarman, optionally times a constant); %r takes the dense route" % (self.kernel,))
        if isinstance(spec, ops.KernelSumSpec):
            raise NotImplementedError("predict_local takes one parametrised kernel: a sum of kernels has no single metric to rank "
                                      "neighbours by; got %r" % (self.kernel,))
        out = ops.gp_predict_local(spec, self._X, self._residual(), self._y_err, X, k=k, return_var=return_var,
                                   return_neighbors=return_neighbors)
        shift = self._mean + self._build_average_meanify(X)
        if return_var or return_neighbors:
            return (out[0] + shift,) + tuple(out[1:])
        return out + shift

    def sample_y(self, X, n_samples=1, random_state=0, nugget=1e-10):
        """Realisations of the posterior at X (n_points, 1 or 2): (n_points, n_samples), scikit-learn's ``sample_y``
        layout (not in the reference).  y_star + L* z with y_star, cov = ``predict(X, return_cov=True)`` (mean, meanify and
        the kept factor included), L* the Cholesky factor of cov + jitter I, jitter = nugget * max k(x, x), and z the v-th
        row of ``np.random.default_rng(random_state).standard_normal((n_samples, n_points))`` for realisation v.
        The posterior covariance comes through ``predict`` under this object's backend; its factorisation and the
        product run on one GPU (no multi-GPU sampling).  The cached solution is left as ``predict`` leaves it.
        Raises numpy.linalg.LinAlgError when cov + jitter I is not positive definite (raise ``nugget``), ValueError for
        n_samples < 1, nugget < 0 or X that does not match the kernel."""
        from . import sampling
        sampling.check_sampling_args(n_samples, nugget)
        X = sampling.as_coords(self.kernel, X)
        y_star, cov = self.predict(X, return_cov=True)
        C = np.array(cov, dtype=np.float64)
        C[np.diag_indices(len(C))] += nugget * sampling.prior_diag_max(self.kernel, X)
        Y = sampling.lmul_dense(C, sampling.normals(n_samples, len(X), random_state), nugget)
        return y_star[:, None] + Y.T

    def predict_fields(self, Y, X, y_err=None):
        """Several fields measured at the SAME positions with the same kernel and errors (one GP per PSF parameter, the Piff
        pattern of treegp/README.rst:28; with the reference each field is its own GPInterpolation, i.e. its own K build,
        cholesky and cho_solve).  Y: (n_fields, n) values at the positions given to ``initialize``; returns (n_fields, m)
        predictions at X.  One K build and one factorisation serve all fields; every field keeps its own mean
        (``normalize``) and shares the mean function table, the kernel and the errors of ``initialize``."""
        Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
        if Y.shape[1] != len(self._X):
            raise ValueError("Y must be (n_fields, %d)" % len(self._X))
        sigma = self._y_err if y_err is None else np.sqrt(np.asarray(y_err, dtype=np.float64) ** 2 + self.white_noise ** 2)
        means = np.mean(Y - self._spatial_average, axis=1) if self.normalize else np.zeros(len(Y))
        R = Y - means[:, None] - self._spatial_average[None, :]
        try:
            spec = self._device_spec(self.kernel)
        except NotImplementedError:
            spec = None
        with self._scope():
            if spec is not None:
                _, _, _, factor = ops.gp_solve(spec, self._X, R[0], sigma, keep=True, want_alpha=False)
            else:
                _, _, _, factor = ops.gp_solve_dense(self.kernel(self._X), R[0], sigma, keep=True, want_alpha=False)
            try:
                alphas = ops.factor_solve(factor, R)
            finally:
                factor.free(keep_memory=True)
            if spec is not None:
                pred = np.stack([ops.gp_predict(spec, self._X, a, X) for a in alphas])
            else:
                pred = alphas.dot(self.kernel(X, Y=self._X).T)
        return pred + means[:, None] + self._build_average_meanify(X)[None, :]

    # -- leave-one-out (not in the reference) ----------------------------------------------------
    def predict_loo(self, return_var=False):
        """Leave-one-out predictions at the positions given to ``initialize``: entry i is what ``predict(X[i:i+1],
        return_var=True)`` returns for a GP with the same kernel given the other n - 1 points, in closed form from alpha and
        diag(K^-1) (Rasmussen & Williams 5.4.2; ops.factor_inv_diag, ~n^3 / 3 flops on the device) instead of n refits.
        ``_mean`` and the mean function are held at their full-data values (R&W treat them as fixed).  Returns y_loo (n,),
        or (y_loo, var_loo) with var_loo the latent variance 1 / d_i - sigma_i^2, not clamped at zero, as ``return_var``.
        Uses the cached ``_alpha`` and the kept factor under the same rules as ``predict(..., return_var=True)``: either
        reuses what the other left; any kernel tree works (the dense route keeps a factor as well)."""
        r = self._residual()
        try:
            spec = self._device_spec(self.kernel)
        except NotImplementedError:
            spec = None
        with self._scope():
            self._ensure_solution(r, self._X, self.kernel, spec, self._y_err, want_factor=True)
            d = ops.factor_inv_diag(self._factor)
        mu, _, v, _ = loo_quantities(r, self._alpha, d, self._y_err)
        y_loo = mu + self._mean + self._spatial_average
        return (y_loo, v) if return_var else y_loo

    def return_loo_log_predictive(self, theta=None):
        """sum_i log p(y_i | y_-i) (Rasmussen & Williams eq. 5.11) for the current (or the given) hyper-parameters: a held-out
        score of the fit, comparable between optimisers.  Mirrors ``return_log_likelihood``: a temporary factor of its own,
        ``_alpha`` and the kept factor are left untouched; -inf when the factorisation fails."""
        from ._lib import TgpError
        from .log_likelihood import _rejects_theta
        kernel = copy.deepcopy(self.kernel)
        if theta is not None:
            kernel = kernel.clone_with_theta(theta)
        r = self._residual()
        try:
            spec = self._device_spec(kernel)
        except NotImplementedError:
            spec = None
        try:
            with self._scope():
                if spec is not None:
                    alpha, _, _, factor = ops.gp_solve(spec, self._X, r, self._y_err, keep=True)
                else:
                    alpha, _, _, factor = ops.gp_solve_dense(kernel(self._X), r, self._y_err, keep=True)
                try:
                    d = ops.factor_inv_diag(factor)
                finally:
                    factor.free(keep_memory=True)
            with np.errstate(invalid="ignore", divide="ignore"):
                total = float(np.sum(loo_quantities(r, alpha, d, self._y_err)[3]))
        except (np.linalg.LinAlgError, FloatingPointError, ValueError):
            total = -np.inf                    # as log_likelihood (log_likelihood.py:38-39 of the reference)
        except TgpError as ex:
            if not _rejects_theta(ex):
                raise
            total = -np.inf
        return total if np.isfinite(total) else -np.inf

    # -- local leave-one-out and Vecchia's likelihood: no n x n factor (not in the reference) -----
    def _local_spec(self, what, kernel=None):
        """the 2-D ``KernelSpec`` of the kernel for the local routes, or their refusals in the style of ``predict_local``"""
        return _kernels.local_spec(self.kernel if kernel is None else kernel, self._X, what, single=kernel_to_spec)

    def predict_loo_local(self, k=64, return_var=False, return_neighbors=False):
        """Local leave-one-out at the positions given to ``initialize``: entry i is predicted from the ``k`` nearest OTHER stars
        alone -- nearest in the kernel's own metric; a duplicate of star i at another row is a legal neighbour -- with no n x n
        factor (ops.gp_local_cond, seam S3v of include/tgp.h).  Linear in n: the held-out check of a fit on a catalogue that
        ``predict_loo`` cannot hold, and the way to see on one's own data whether ``k`` is large enough.  Residual, ``_mean`` and
        the mean function are handled as in ``predict_loo``; the variance of ``return_var`` is latent, as there, and not clamped.
        With ``k`` >= n - 1 it is ``predict_loo``.  ``return_neighbors``: also the (n, k) rows used, nearest first, padded with -1,
        and their lengths.  ``_alpha`` and a kept factor are neither used nor touched.  Raises numpy.linalg.LinAlgError naming the
        first row whose local matrix is not positive definite, NotImplementedError for 3-D coordinates, sums of kernels and the
        kernels of the dense route.  Runs on one GPU whichever backend is set."""
        spec = self._local_spec("predict_loo_local")
        out = ops.gp_local_cond(spec, self._X, self._residual(), self._y_err, k=k, mode="loo", return_neighbors=return_neighbors)
        y_loo = out[0] + self._mean + self._spatial_average
        res = (y_loo,) + ((out[1],) if return_var else ()) + (tuple(out[3:]) if return_neighbors else ())
        return res if len(res) > 1 else y_loo

    def _local_log_score(self, what, theta, k, mode, rank=None, neighbors=None):
        """-1/2 sums[1] - 1/2 sums[0] - n/2 log 2 pi of ops.gp_local_cond; -inf when a row failed (as ``log_likelihood``)"""
        from ._lib import TgpError
        from .log_likelihood import _rejects_theta
        kernel = copy.deepcopy(self.kernel)
        if theta is not None:
            kernel = kernel.clone_with_theta(theta)
        spec = self._local_spec(what, kernel)
        try:
            _, _, sums = ops.gp_local_cond(spec, self._X, self._residual(), self._y_err, k=k, mode=mode, rank=rank,
                                           neighbors=neighbors)
            total = -0.5 * sums[1] - 0.5 * sums[0] - 0.5 * len(self._X) * np.log(2.0 * np.pi)
        except (np.linalg.LinAlgError, FloatingPointError):
            total = -np.inf
        except TgpError as ex:
            # an invLam without a Cholesky factor is a rejected theta, as a K that is not positive definite is
            if "has no Cholesky factor" not in str(ex) and not _rejects_theta(ex):
                raise
            total = -np.inf
        return float(total) if np.isfinite(total) else -np.inf

    def return_loo_log_predictive_local(self, theta=None, k=64):
        """sum_i log N(y_i | mu_i, var_i + y_err_i^2) with mu_i, var_i the local leave-one-out of ``predict_loo_local`` for the
        current (or the given) hyper-parameters: ``return_loo_log_predictive`` without the dense factor, the same number when
        ``k`` >= n - 1.  A held-out score to compare two fits of a large catalogue with.  -inf when a local matrix is not positive
        definite."""
        return self._local_log_score("return_loo_log_predictive_local", theta, k, "loo")

    def return_log_likelihood_local(self, theta=None, k=64, seed=0):
        """Vecchia's approximation of the log-likelihood for the current (or the given) hyper-parameters:
        sum_i log N(y_i | mu_i, var_i + y_err_i^2), row i conditioned on its ``k`` nearest rows among those earlier in the random
        ordering ``ops.vecchia_rank(n, seed)``.  By the chain rule it is ``return_log_likelihood`` when ``k`` >= n - 1; it is
        linear in n and needs no n x n factor.  -inf when any row's local matrix is not positive definite, as ``log_likelihood``
        returns for K."""
        return self._local_log_score("return_log_likelihood_local", theta, k, "prior", rank=ops.vecchia_rank(len(self._X), seed))

    # -- error bars on the hyper-parameters (not in the reference) --------------------------------
    def return_fisher_information(self, theta=None):
        """F_theta (ntheta, ntheta), the Fisher information of the Gaussian likelihood for the current (or the given)
        hyper-parameters: F_ij = 1/2 tr(C dK/dtheta_i C dK/dtheta_j), C = (K + diag(y_err^2))^-1 (white noise included); its
        inverse is the covariance of the maximum-likelihood estimate (``return_theta_covariance``).  It does not depend on y.
        Mirrors ``return_loo_log_predictive``: a temporary factor of its own (``ops.gp_fisher`` on it, include/tgp.h seam S2j;
        about 24 factorisations' worth of flops per term), ``_alpha`` and the kept factor are left untouched.  Fixed
        hyper-parameters have no row.  numpy.linalg.LinAlgError when K is not positive definite; NotImplementedError for 3-D
        coordinates (the device has no 3-D derivative) and for kernel trees that take the dense route (WhiteKernel, Matern,
        more than four terms), which has no derivative matrices."""
        kernel = copy.deepcopy(self.kernel)
        if theta is not None:
            kernel = kernel.clone_with_theta(theta)
        if _three_d(self._X):
            raise NotImplementedError("return_fisher_information: 3-D coordinates have no derivative matrices on the device "
                                      "(only the K build, predict and covariance take (n, 3) coordinates)")
        try:
            spec = self._device_spec(kernel)
        except NotImplementedError as ex:
            raise NotImplementedError("return_fisher_information needs a kernel with a device form (RBF, AnisotropicRBF, VonKarman, "
                                      "AnisotropicVonKarman or a sum of up to four of them); this one takes the dense route, which "
                                      "has no derivative matrices: %s" % ex)
        with self._scope():
            factor = ops.gp_solve(spec, self._X, self._residual(), self._y_err, keep=True, want_alpha=False)[3]
            try:
                F_p = ops.gp_fisher(spec, factor, self._X)
            finally:
                factor.free(keep_memory=True)
        return _kernels.fisher_theta(kernel, F_p)

    def return_theta_covariance(self, theta=None):
        """The inverse of ``return_fisher_information(theta)``: the covariance of the maximum-likelihood estimate of theta
        (Cramer-Rao), e.g. ``np.sqrt(np.diag(gp.return_theta_covariance()))`` for the one-sigma errors after ``solve()``.
        Through a Cholesky factorisation: numpy.linalg.LinAlgError when F_theta is not positive definite (a hyper-parameter the
        data do not constrain).  Raises as ``return_fisher_information`` otherwise."""
        F = self.return_fisher_information(theta)
        L = np.linalg.cholesky(F)                           # LinAlgError: not positive definite
        Li = np.linalg.solve(L, np.eye(len(L)))
        return Li.T.dot(Li)

    # -- leave-group-out (not in the reference) --------------------------------------------------
    def _lgo_solve(self, kernel, perm, starts, want_cov):
        """lgo_quantities of the problem permuted by ``perm`` (the groups contiguous) from a temporary factor of its own:
        (mu, v, logp, covs) in the permuted order"""
        X, r, sigma = self._X, self._residual(), self._y_err
        if perm is not None:
            X, r, sigma = X[perm], r[perm], np.asarray(sigma)[perm]
        try:
            spec = self._device_spec(kernel)
        except NotImplementedError:
            spec = None
        with self._scope():
            if spec is not None:
                alpha, _, _, factor = ops.gp_solve(spec, X, r, sigma, keep=True)
            else:
                alpha, _, _, factor = ops.gp_solve_dense(kernel(X), r, sigma, keep=True)
            try:
                blocks = ops.factor_inv_blocks(factor, starts)
            finally:
                factor.free(keep_memory=True)
            return lgo_quantities(r, alpha, blocks, sigma, starts, want_cov=want_cov)

    def predict_lgo(self, groups, return_var=False, return_cov=False):
        """Leave-group-out predictions at the positions given to ``initialize``.  ``groups``: one integer label per training
        point, any labels (``kfold_labels``, ``spatial_block_labels``, a chip number, ...).  Entry i of y_lgo (n,) is what
        ``predict(X[i:i+1])`` returns for a GP with the same kernel given every point OUTSIDE i's group: for a spatially
        correlated field the held-out score that ``predict_loo`` flatters, since a deleted star's neighbours still carry
        almost all of its information.  Closed form from alpha and the diagonal blocks of K^-1 (Rasmussen & Williams 5.4.2
        with blocks for points; ops.factor_inv_blocks, one substitution on the device) instead of one refit per group.
        ``return_var``: also the latent variances (n,), what ``predict(X[i:i+1], return_var=True)`` gives there;
        ``return_cov``: also a dict label -> (indices, C_G) with the group's points and their latent covariance, what
        ``predict(X[indices], return_cov=True)`` gives.  At most one of the two; nothing is clamped.  ``_mean`` and the mean
        function are held at their full-data values, as in ``predict_loo``.
        When every label occupies one contiguous run of rows (catalogues concatenated chip by chip) the cached ``_alpha`` and
        the kept factor serve under ``predict_loo``'s rules.  Otherwise the problem permuted by the stable sort by label is
        solved on a temporary factor, and ``_alpha`` and the kept factor stay untouched.  Any kernel tree works.
        ValueError for labels of the wrong length or a group above 4096 points (naming the label)."""
        if return_cov and return_var:
            raise ValueError("at most one of return_cov and return_var may be True")
        n = len(self._X)
        labels = np.asarray(groups)
        if labels.shape != (n,):
            raise ValueError("groups must hold one label per training point, shape (%d,); got %r" % (n, labels.shape))
        perm, starts, names = group_runs(labels, gmax=ops.INVBLOCK_GMAX)
        if perm is None:
            r = self._residual()
            try:
                spec = self._device_spec(self.kernel)
            except NotImplementedError:
                spec = None
            with self._scope():
                self._ensure_solution(r, self._X, self.kernel, spec, self._y_err, want_factor=True)
                blocks = ops.factor_inv_blocks(self._factor, starts)
                mu, v, _, covs = lgo_quantities(r, self._alpha, blocks, self._y_err, starts, want_cov=return_cov)
            index = np.arange(n)
        else:
            mu_p, v_p, _, covs = self._lgo_solve(self.kernel, perm, starts, return_cov)
            mu, v = np.empty(n), np.empty(n)
            mu[perm], v[perm] = mu_p, v_p
            index = perm
        y_lgo = mu + self._mean + self._spatial_average
        if return_cov:
            return y_lgo, {names[g].item(): (index[starts[g]:starts[g + 1]].copy(), covs[g]) for g in range(len(names))}
        return (y_lgo, v) if return_var else y_lgo

    def return_lgo_log_predictive(self, groups, theta=None):
        """sum over the groups of log p(y_G | y_-G) for the current (or the given) hyper-parameters: the held-out score of
        ``predict_lgo``'s folds, comparable between optimisers and kernels.  Mirrors ``return_loo_log_predictive``: a
        temporary factor of its own, ``_alpha`` and the kept factor are left untouched; -inf when the factorisation fails."""
        from ._lib import TgpError
        from .log_likelihood import _rejects_theta
        n = len(self._X)
        labels = np.asarray(groups)
        if labels.shape != (n,):
            raise ValueError("groups must hold one label per training point, shape (%d,); got %r" % (n, labels.shape))
        perm, starts, _ = group_runs(labels, gmax=ops.INVBLOCK_GMAX)
        kernel = copy.deepcopy(self.kernel)
        if theta is not None:
            kernel = kernel.clone_with_theta(theta)
        try:
            with np.errstate(invalid="ignore", divide="ignore"):
                total = float(np.sum(self._lgo_solve(kernel, perm, starts, False)[2]))
        except (np.linalg.LinAlgError, FloatingPointError, ValueError):
            total = -np.inf                    # as return_loo_log_predictive
        except TgpError as ex:
            if not _rejects_theta(ex):
                raise
            total = -np.inf
        return total if np.isfinite(total) else -np.inf

    def predict_fields_loo(self, Y, y_err=None):
        """Leave-one-out predictions of several fields measured at the positions given to ``initialize`` (the
        ``predict_fields`` pattern): Y (n_fields, n) -> (n_fields, n).  One factorisation, one diag(K^-1) and one multi-
        right-hand-side solve serve all fields; every field keeps its own mean (``normalize``), held fixed as in
        ``predict_loo``, and shares the mean function, the kernel and the errors.  ``_alpha`` and the kept factor are left
        untouched."""
        Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
        if Y.ndim != 2 or Y.shape[1] != len(self._X):
            raise ValueError("Y must be (n_fields, %d)" % len(self._X))
        sigma = self._y_err if y_err is None else np.sqrt(np.asarray(y_err, dtype=np.float64) ** 2 + self.white_noise ** 2)
        means = np.mean(Y - self._spatial_average, axis=1) if self.normalize else np.zeros(len(Y))
        R = Y - means[:, None] - self._spatial_average[None, :]
        try:
            spec = self._device_spec(self.kernel)
        except NotImplementedError:
            spec = None
        with self._scope():
            if spec is not None:
                _, _, _, factor = ops.gp_solve(spec, self._X, R[0], sigma, keep=True, want_alpha=False)
            else:
                _, _, _, factor = ops.gp_solve_dense(self.kernel(self._X), R[0], sigma, keep=True, want_alpha=False)
            try:
                alphas = ops.factor_solve(factor, R)
                d = ops.factor_inv_diag(factor)
            finally:
                factor.free(keep_memory=True)
        mu = loo_quantities(R, alphas, d, sigma)[0]
        return mu + means[:, None] + self._spatial_average[None, :]

    # -- data ------------------------------------------------------------------------------------
    def initialize(self, X, y, y_err=None):
        """Take the data: coordinates (n, 1, 2 or 3), values, errors (zeros when None).  gp_interp.py:196-227:
        a fresh copy of the kernel template, white noise added to the errors in quadrature, the mean taken
        of y minus the mean function, any cached solution dropped."""
        if _three_d(X) and self._X0 is not None and np.count_nonzero(self._X0) > 0:
            raise ValueError("a mean-function table is a 2-D statistic (meanify bins the first two coordinates); it cannot be "
                             "used with 3-D coordinates, got X of shape %r" % (np.shape(X),))
        self.kernel = copy.deepcopy(self.kernel_template)
        self._X, self._y = X, y
        sigma = np.zeros_like(y) if y_err is None else y_err
        if self._X0 is None:
            # no mean-function table: an all-zero one, created once and kept across initialize() calls
            self._X0, self._y0 = np.zeros_like(X), np.zeros_like(y)
        self._spatial_average = self._build_average_meanify(X)
        if self.white_noise > 0:
            sigma = np.sqrt(sigma ** 2 + self.white_noise ** 2)
        self._y_err = sigma
        self._mean = np.mean(y - self._spatial_average) if self.normalize else 0.0
        self._drop_solution()

    def _build_average_meanify(self, X):
        """Mean function at X by K-nearest-neighbour interpolation of the meanify table, zeros when
        there is none.  gp_interp.py:229-243."""
        if np.count_nonzero(self._X0) > 0:               # "a table is present" = X0 is not all zeros
            y0 = np.asarray(self._y0)
            k = self.n_neighbors
            on_gpu = k <= 8 or k == 16
            if y0.ndim == 1 and on_gpu:
                return ops.knn_mean(self._X0, y0, X, k)                          # tgp_knn_mean
            if y0.ndim == 2 and self.indice_meanify is not None and on_gpu:
                return ops.knn_mean(self._X0, y0[:, self.indice_meanify], X, k)
            # multi-column table without a column pick / unusual k: scikit-learn, as the reference does
            table = KNeighborsRegressor(n_neighbors=k).fit(self._X0, self._y0)
            average = table.predict(X)
            return average if self.indice_meanify is None else average[:, self.indice_meanify]
        return np.zeros(len(X))

    def _residual(self):
        return self._y - self._mean - self._spatial_average

    def solve(self):
        """Fit the hyper-parameters if an optimizer was requested (gp_interp.py:245-258); the starting theta
        is kept in ``_init_theta``."""
        if _three_d(self._X) and self.optimizer in ("two-pcf", "anisotropic"):
            raise ValueError("optimizer=%r fits a 2-D statistic (the 2-point correlation function of the first two coordinates); "
                             "3-D coordinates take optimizer='log-likelihood' or 'none'" % (self.optimizer,))
        self._init_theta = [copy.deepcopy(self.kernel).theta]
        with self._scope():
            self.kernel = self._fit(self.kernel, self._X, self._residual(), self._y_err)

    def return_2pcf(self):
        """xi, xi_weight, distance, coord, mask of the measured 2-point correlation function
        (gp_interp.py:260-275)."""
        from .two_pcf import two_pcf
        measured = two_pcf(self._X, self._residual(), self._y_err, self.min_sep, self.max_sep, nbins=self.nbins,
                           anisotropic=(self.optimizer == "anisotropic"))
        return measured.return_2pcf()

    def return_log_likelihood(self, theta=None):
        """Log-likelihood of the data for the current (or the given) hyper-parameters (gp_interp.py:277-291)."""
        from .log_likelihood import log_likelihood
        kernel = copy.deepcopy(self.kernel)
        if theta is not None:
            kernel = kernel.clone_with_theta(theta)
        with self._scope():
            return log_likelihood(self._X, self._residual(), self._y_err).log_likelihood(kernel)

    def plot_fitted_kernel(self):
        raise NotImplementedError("plotting (treegp/gp_interp.py:293-377) is outside the GPU hot path")


def predict_many(gps, Xs, return_cov=False, return_var=False):
    """``[gp.predict(X) for gp, X in zip(gps, Xs)]`` with the solves of many small GPs in one batched factorisation (the
    reference's regime: one GP per PSF parameter, exposure or chip, README.rst:28).  ``gps``: initialised GPInterpolation
    objects; ``Xs``: their query points.  The objects whose kernel ``kernels.device_spec`` describes (one parametrised kernel
    or a sum of up to four), that are not on the multi-GPU route, hold at most 4096 points and have no cached solution get their alpha from one batched solve
    (ops.gp_solve_batch); it is cached in ``gp._alpha`` as ``predict`` caches it, so that a later ``gp.predict`` reuses
    it.  Every object then predicts through its own ``predict``: the others solve there as usual.  A failed
    factorisation raises numpy.linalg.LinAlgError naming the object's index (nothing is cached then).

    ``return_cov=True`` / ``return_var=True`` return a list of ``(y, cov)`` / ``(y, var)`` with what each object's
    ``gp.predict(X, return_cov=True)`` / ``return_var=True`` gives: the posterior of the objects above (a cached solution
    does not exclude them here) with at most 4096 (covariance) or 65 280 (variance) query points and no kept factor of the
    same data comes from one batched factorisation and substitution (ops.gp_posterior_batch); a cached alpha is kept, an
    object without one caches the batch's, and no kept factor is left behind.  The mean is each object's own ``predict(X)``
    from its cached alpha.  Every other object goes through its own ``predict``.  At most one flag may be True."""
    if return_cov and return_var:
        raise ValueError("at most one of return_cov and return_var may be True")
    gps, Xs = list(gps), list(Xs)
    if len(gps) != len(Xs):
        raise ValueError("predict_many: %d GPs but %d arrays of query points" % (len(gps), len(Xs)))
    if return_cov or return_var:
        return _predict_many_posterior(gps, Xs, "cov" if return_cov else "var")
    picked, specs = [], []
    for i, gp in enumerate(gps):
        if gp._alpha is not None:
            continue
        spec = _batch_spec(gp)
        if spec is None:
            continue
        picked.append(i)
        specs.append(spec)
    if picked:
        alphas, _, _, info = ops.gp_solve_batch(specs, [gps[i]._X for i in picked], [gps[i]._residual() for i in picked],
                                                [gps[i]._y_err for i in picked])
        _raise_failed(picked, info)
        for j, i in enumerate(picked):
            gps[i]._alpha = alphas[j]
            gps[i]._set_factor(None, None)        # what predict's own solve leaves: no kept factor
    return [gp.predict(X) for gp, X in zip(gps, Xs)]


def _batch_spec(gp, kernel=None):
    """the device kernel of an object the batched routes may take (``kernels.device_spec`` describes it -- ``gp.kernel``, or the
    given one: one parametrised kernel, ``ops.KernelSpec``, or a sum of up to four, ``ops.KernelSumSpec`` -- not on the multi-GPU
    route, at most 4096 points), else None"""
    if gp.backend == "dist" or len(gp._X) > ops.BATCH_NMAX or _three_d(gp._X):
        return None                               # (a 3-D object is one of the "other objects": there is no batched 3-D build)
    try:
        spec = _kernels.device_spec(gp.kernel if kernel is None else kernel, allow_sum=True, single=kernel_to_spec)
    except NotImplementedError:
        return None
    with gp._scope():
        if ops._dist_engine(len(gp._X), None) is not None:
            return None
    return spec


def _raise_failed(picked, info, who="predict_many"):
    for j, i in enumerate(picked):
        if info[j] > 0:
            raise np.linalg.LinAlgError("%s: GP %d: %d-th leading minor of the array is not positive definite"
                                        % (who, i, info[j]))


def _predict_many_posterior(gps, Xs, what):
    picked, specs = [], []
    for i, gp in enumerate(gps):
        m = len(Xs[i])
        if m < 1 or m > ops.POSTERIOR_MMAX[what]:
            continue
        spec = _batch_spec(gp)
        if spec is None:
            continue
        if gp._factor is not None and gp._factor_key == gp._factor_fingerprint(spec, gp._X, gp._y_err):
            continue                              # its own predict reuses the kept factor: no factorisation to save
        picked.append(i)
        specs.append(spec)
    uncs = {}
    if picked:
        alphas, unc, _, _, info = ops.gp_posterior_batch(specs, [gps[i]._X for i in picked],
                                                         [gps[i]._residual() for i in picked],
                                                         [gps[i]._y_err for i in picked], [Xs[i] for i in picked], what=what)
        _raise_failed(picked, info)
        for j, i in enumerate(picked):
            if gps[i]._alpha is None:
                gps[i]._alpha = alphas[j]         # a cached alpha stays, as in _ensure_solution
            gps[i]._set_factor(None, None)
            uncs[i] = unc[j]
    out = []
    for i, (gp, X) in enumerate(zip(gps, Xs)):
        if i in uncs:
            out.append((gp.predict(X), uncs[i]))
        else:
            out.append(gp.predict(X, return_cov=what == "cov", return_var=what == "var"))
    return out


def predict_loo_many(gps, return_var=False):
    """``[gp.predict_loo(return_var) for gp in gps]`` with the factorisations and diag(K^-1) of many small GPs in one batched
    call (ops.gp_loo_batch): the validation step between ``solve_many`` and ``predict_many``.  The objects the batched routes
    take (``kernels.device_spec`` describes the kernel, not on the multi-GPU route, at most 4096 points) and that hold no kept factor
    of the same data go through it, then through ``loo_quantities`` on the host exactly as ``predict_loo``; a cached alpha is
    kept, an object without one caches the batch's, and no kept factor is left behind.  Every other object goes through its own
    ``predict_loo``.  A failed factorisation raises numpy.linalg.LinAlgError naming the object's index (nothing is cached
    then)."""
    gps = list(gps)
    picked, specs = [], []
    for i, gp in enumerate(gps):
        spec = _batch_spec(gp)
        if spec is None:
            continue
        if gp._factor is not None and gp._factor_key == gp._factor_fingerprint(spec, gp._X, gp._y_err):
            continue                              # its own predict_loo reuses the kept factor: no factorisation to save
        picked.append(i)
        specs.append(spec)
    done = {}
    if picked:
        residuals = [gps[i]._residual() for i in picked]
        alphas, ds, _, _, info = ops.gp_loo_batch(specs, [gps[i]._X for i in picked], residuals,
                                                  [gps[i]._y_err for i in picked])
        _raise_failed(picked, info, "predict_loo_many")
        for j, i in enumerate(picked):
            gp = gps[i]
            if gp._alpha is None:
                gp._alpha = alphas[j]             # a cached alpha stays, as in _ensure_solution
            gp._set_factor(None, None)
            mu, _, v, _ = loo_quantities(residuals[j], gp._alpha, ds[j], gp._y_err)
            y_loo = mu + gp._mean + gp._spatial_average
            done[i] = (y_loo, v) if return_var else y_loo
    return [done[i] if i in done else gp.predict_loo(return_var=return_var) for i, gp in enumerate(gps)]


def loo_log_predictive_many(gps, thetas=None):
    """``[gp.return_loo_log_predictive(theta) for gp, theta in zip(gps, thetas)]`` as a float array, the objects the batched
    routes take in one batched call (ops.gp_loo_batch).  ``thetas``: None, or a list with None or a theta per object, cloned
    into a copy of the object's kernel.  -inf for a factorisation that fails or a sum that is not finite, as the single method;
    ``_alpha``, the kept factor and ``gp.kernel`` of every object are left untouched.  Every other object goes through its own
    ``return_loo_log_predictive``."""
    from ._lib import TgpError
    gps = list(gps)
    thetas = [None] * len(gps) if thetas is None else list(thetas)
    if len(thetas) != len(gps):
        raise ValueError("loo_log_predictive_many: %d GPs but %d thetas" % (len(gps), len(thetas)))
    out = np.full(len(gps), -np.inf)
    picked, specs = [], []
    for i, (gp, theta) in enumerate(zip(gps, thetas)):
        kernel = copy.deepcopy(gp.kernel)
        if theta is not None:
            kernel = kernel.clone_with_theta(theta)
        spec = _batch_spec(gp, kernel)
        if spec is None:
            out[i] = gp.return_loo_log_predictive(theta)
        else:
            picked.append(i)
            specs.append(spec)
    if picked:
        residuals = [gps[i]._residual() for i in picked]
        try:
            alphas, ds, _, _, info = ops.gp_loo_batch(specs, [gps[i]._X for i in picked], residuals,
                                                      [gps[i]._y_err for i in picked])
        except TgpError as ex:
            # judged as a device error of one evaluation (log_likelihood._rejects_theta): an argument error, or any error
            # under TGP_ML_STRICT=1, raises; a run-time one warns, and every object meets what its own method gives it
            from .log_likelihood import _rejects_theta
            if not _rejects_theta(ex):
                raise
            for i in picked:
                out[i] = gps[i].return_loo_log_predictive(thetas[i])
            return out
        for j, i in enumerate(picked):
            if info[j] > 0:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                total = float(np.sum(loo_quantities(residuals[j], alphas[j], ds[j], gps[i]._y_err)[3]))
            out[i] = total if np.isfinite(total) else -np.inf
    return out

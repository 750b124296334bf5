"""Maximum-likelihood hyper-parameter search; mirrors ``treegp/log_likelihood.py:7-62``.

Each likelihood evaluation is one fused GPU solve (tgp_gp_solve: K build + noise diagonal +
Cholesky + solve + logdet, K never leaves the device).  The L-BFGS-B driver stays on the host,
as in the reference, and so does its gradient: forward differences with SciPy's own step (the
reference passes no ``jac``, :57, so SciPy differentiates numerically).  The difference is that the
ntheta + 1 evaluations one gradient needs are independent solves of a small problem, which leave
most of the GPU idle one at a time: they are issued together, one context / stream per evaluation
(``parallel_fd``; 2-2.5x on a fit at N = 512 ... 8192).  Same optimiser, same formula, same iterates.
During a fit the data stay on the device (``ops.ResidentProblem``): an evaluation sends the kernel parameters and gets
two scalars back; the quadratic form is |L^-1 y|^2, with y carried through the factorisation as an extra matrix row
(no triangular sweep; the forward sweep alone when n is a multiple of 256).
"""
import copy
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from scipy import optimize

from . import _lib, ops
from . import kernels as _kernels
from ._lib import TgpError
from .kernels import kernel_to_spec, spec_jacobian

_FD_STEP = 1e-8                  # scipy.optimize.minimize(method="L-BFGS-B") default `eps` (absolute forward step)
_PARALLEL_MAX_N = 16384          # beyond this one solve fills the GPU by itself
_BATCH_CALL = 256                # log_likelihood_many: kernels per batched call (the library chunks further by device memory)
_pool_lock = threading.Lock()
_ctx_pool = []                   # extra contexts (one stream each) for concurrent evaluations, created on demand


def _contexts(count):
    with _pool_lock:
        while len(_ctx_pool) < count:
            ctx = _lib.new_ctx(int(os.environ.get("TGP_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
            _lib.load_library().tgp_set_lookahead(ctx, 0)     # side by side: one stream each (hardware queues are few)
            _ctx_pool.append(ctx)
        return _ctx_pool[:count]


def _rejects_theta(ex):
    """What a library error inside ONE likelihood evaluation means for the fit.  The reference catches everything
    (``except BaseException``, log_likelihood.py:38) so that any failure is a rejected theta and L-BFGS-B carries on.  Here a
    run-time device error (rc -2: out of device memory, a failed HIP call) is treated the same way, with a RuntimeWarning so
    that it cannot pass unnoticed; an argument error (rc -1) is a bug in the caller and always propagates.  TGP_ML_STRICT=1:
    every TgpError propagates (departures)."""
    if os.environ.get("TGP_ML_STRICT") == "1" or getattr(ex, "rc", -1) != -2:
        return False
    import warnings
    warnings.warn("likelihood evaluation failed on the device and counts as -inf (set TGP_ML_STRICT=1 to raise): %s" % ex,
                  RuntimeWarning, stacklevel=3)
    return True


class log_likelihood(object):
    """:param X: coordinates (n_samples, 1, 2 or 3)  :param y: values  :param y_err: errors."""

    def __init__(self, X, y, y_err):
        self.X, self.y, self.y_err = X, y, y_err
        self.ndata = len(X[:, 0])
        # 3-D coordinates: every evaluation is one ops.gp_solve with a KernelSpec3 (no resident data, no batched solve, no exact
        # gradient: the fit differences the likelihood at every size, as the reference does)
        self.three_d = np.ndim(X) == 2 and np.shape(X)[1] == 3
        # the multi-GPU route (treegp_amd.dist) takes every evaluation by itself: all ranks factorise one K together
        self.distributed = ops._dist_engine(self.ndata, None) is not None
        self.parallel_fd = (os.environ.get("TGP_ML_PARALLEL", "1") != "0" and self.ndata <= _PARALLEL_MAX_N
                            and not self.distributed)
        # "fd": the reference's fit (SciPy differentiates numerically, log_likelihood.py:57).  "analytic": L-BFGS-B is given
        # the exact gradient instead (log_likelihood_gradient; Gaussian kernels only) -- a different path through theta-space
        # to the same optimum.  "auto" (default): finite differences, the reference's iterates, wherever their ntheta + 1
        # evaluations run side by side (n <= 16 384); above that, where each of them is a full solve of its own, the exact
        # gradient (1.7 - 2 x a solve instead of ntheta more solves) if the kernel has one.  "analytic-vk": the exact gradient
        # for all four kinds, the von Karman ones through the derivative the reference does not have (include/tgp.h, S2h).
        self.gradient = os.environ.get("TGP_ML_GRADIENT", "auto")

    def _device_spec(self, kernel):
        """``kernel_to_spec``'s description, or else a sum's (``kernels.device_spec``) -- except on the multi-GPU route, where
        sums keep the dense route; NotImplementedError for every other tree.  3-D coordinates: ``kernel_to_spec3``'s description
        (the dense route under the multi-GPU engine, which has no 3-D K build, and for sums)"""
        if self.three_d:
            if self.distributed:
                raise NotImplementedError("3-D coordinates keep the dense route under the multi-GPU engine")
            return _kernels.device_spec(kernel, ndim=3)
        return _kernels.device_spec(kernel, allow_sum=not self.distributed, single=kernel_to_spec)

    def log_likelihood(self, kernel, ctx=None, resident=None):
        """-0.5 y.K^-1.y - (n/2) log 2 pi - 0.5 log det K; any failure (e.g. K not positive
        definite) gives -inf, as at log_likelihood.py:28-39.  `resident`: the data already on the device
        (ops.ResidentProblem, used by optimizer() for the evaluations of one fit)."""
        try:
            try:
                spec = self._device_spec(kernel)
            except NotImplementedError:
                spec = None                       # any other scikit-learn kernel tree: it evaluates itself on the host
            if spec is None:
                _, log_det, chi2, _ = ops.gp_solve_dense(kernel(self.X), self.y, self.y_err, want_alpha=False, ctx=ctx)
            elif resident is not None and not isinstance(spec, (ops.KernelSumSpec, ops.KernelSpec3)):   # (no resident variant of the sum and 3-D solves)
                log_det, chi2 = ops.gp_solve_resident(spec, resident, ctx=ctx)
            else:
                _, log_det, chi2, _ = ops.gp_solve(spec, self.X, self.y, self.y_err, want_alpha=False, ctx=ctx)
            ll = -0.5 * chi2 - (0.5 * self.ndata) * np.log(2.0 * np.pi) - 0.5 * log_det
        except (np.linalg.LinAlgError, FloatingPointError, ValueError):
            # the mathematical failures the reference turns into -inf (log_likelihood.py:38-39)
            ll = -np.inf
        except TgpError as ex:
            if not _rejects_theta(ex):
                raise
            ll = -np.inf
        if not np.isfinite(ll):
            ll = -np.inf
        return ll

    def log_likelihood_many(self, kernels):
        """One log L per kernel, each with exactly ``log_likelihood(kernel)``'s semantics (-inf for a matrix that is not
        positive definite and for the failures that method turns into -inf).  The kernels ``kernels.device_spec`` describes
        (one parametrised kernel, or a sum of up to four) go through batched solves (ops.gp_solve_batch: one launch sequence for up to _BATCH_CALL of them); other kernel trees,
        n > 4096 and the multi-GPU route take ``log_likelihood`` one kernel after the other."""
        kernels = list(kernels)
        out = np.full(len(kernels), -np.inf)
        batched = []
        for i, kernel in enumerate(kernels):
            spec = None
            if not self.distributed and self.ndata <= ops.BATCH_NMAX and not self.three_d:
                try:
                    spec = self._device_spec(kernel)
                except NotImplementedError:
                    spec = None
            if spec is None:
                out[i] = self.log_likelihood(kernel)
            else:
                batched.append((i, spec))
        const = (0.5 * self.ndata) * np.log(2.0 * np.pi)
        for c0 in range(0, len(batched), _BATCH_CALL):
            part = batched[c0:c0 + _BATCH_CALL]
            m = len(part)
            try:
                _, log_det, chi2, info = ops.gp_solve_batch([s for _, s in part], [self.X] * m, [self.y] * m,
                                                            None if self.y_err is None else [self.y_err] * m,
                                                            want_alpha=False)
            except (ValueError, TgpError) as ex:
                # a device error of the batch is judged as one of a single evaluation (_rejects_theta): an argument error, or
                # any error under TGP_ML_STRICT=1, raises; a run-time one (rc -2: e.g. the batch's memory) warns, and then
                # every kernel meets what log_likelihood would give it by itself
                if isinstance(ex, TgpError):
                    if os.environ.get("TGP_ML_STRICT") == "1" or getattr(ex, "rc", -1) != -2:
                        raise
                    import warnings
                    warnings.warn("batched likelihood evaluation failed on the device, its %d kernels are evaluated one by "
                                  "one (set TGP_ML_STRICT=1 to raise): %s" % (m, ex), RuntimeWarning, stacklevel=2)
                for i, _ in part:
                    out[i] = self.log_likelihood(kernels[i])
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                ll = -0.5 * chi2 - const - 0.5 * log_det
            for j, (i, _) in enumerate(part):
                out[i] = ll[j] if info[j] == 0 and np.isfinite(ll[j]) else -np.inf
        return out

    def log_likelihood_gradient(self, kernel, ctx=None, resident=None, any_kind=False):
        """(log L, d log L / d theta): 1/2 tr((alpha alpha^T - K^-1) dK/dtheta_k) with the kernel derivative of
        ``treegp/kernels.py:128-150``; K^-1 is formed on the device from the factor of the same solve
        (``ops.gp_loglik_grad``).  Failures give (-inf, zeros) as ``log_likelihood`` gives -inf.
        ``any_kind=True``: the von Karman kernels too, through the entries of seam S2h (``ops.gp_loglik_grad_any``) and
        ``spec_jacobian(kernel, von_karman=True)``; the same numbers for the Gaussian ones.  With ``any_kind=True`` also the sums
        of ``kernels.kernel_to_sum_spec``: a kept factor, ``ops.gp_loglik_grad_sum`` and ``kernels.sum_spec_jacobian``."""
        ntheta = len(kernel.theta)
        try:
            spec = self._device_spec(kernel) if any_kind else kernel_to_spec(kernel)
            is_sum = isinstance(spec, ops.KernelSumSpec)
            if is_sum:
                jac = _kernels.sum_spec_jacobian(kernel)
            else:
                jac = spec_jacobian(kernel, von_karman=True) if any_kind else spec_jacobian(kernel)
            if is_sum:
                alpha, log_det, chi2, factor = ops.gp_solve(spec, self.X, self.y, self.y_err, keep=True, ctx=ctx)
                try:
                    g4 = ops.gp_loglik_grad_sum(spec, factor, self.X, alpha, ctx=ctx).ravel()
                finally:
                    factor.free(keep_memory=True)
            elif resident is not None:
                solve_grad = ops.gp_solve_grad_resident_any if any_kind else ops.gp_solve_grad_resident
                log_det, chi2, g4 = solve_grad(spec, resident, ctx=ctx)
            else:
                alpha, log_det, chi2, factor = ops.gp_solve(spec, self.X, self.y, self.y_err, keep=True, ctx=ctx)
                try:
                    loglik_grad = ops.gp_loglik_grad_any if any_kind else ops.gp_loglik_grad
                    g4 = loglik_grad(spec, factor, self.X, alpha, ctx=ctx)
                finally:
                    factor.free(keep_memory=True)          # the next evaluation solves the same size on this context
            ll = -0.5 * chi2 - (0.5 * self.ndata) * np.log(2.0 * np.pi) - 0.5 * log_det
        except (np.linalg.LinAlgError, FloatingPointError, ValueError):
            return -np.inf, np.zeros(ntheta)
        except TgpError as ex:
            if not _rejects_theta(ex):
                raise
            return -np.inf, np.zeros(ntheta)
        if not np.isfinite(ll):
            return -np.inf, np.zeros(ntheta)
        return ll, jac.dot(g4)

    def fisher_information(self, kernel, ctx=None):
        """F_theta (ntheta, ntheta): the Fisher information of the Gaussian likelihood at ``kernel``'s hyper-parameters,
        F_ij = 1/2 tr(C dK/dtheta_i C dK/dtheta_j) with C = (K + diag(y_err^2))^-1; its inverse is the covariance of the
        maximum-likelihood estimate.  It does not depend on y.  One solve that keeps its factor, ``ops.gp_fisher`` on it
        (include/tgp.h, seam S2j) and ``kernels.fisher_theta`` on the host.  NotImplementedError for 3-D coordinates and for
        kernel trees without a device form; numpy.linalg.LinAlgError when K is not positive definite."""
        if self.three_d:
            raise NotImplementedError("fisher_information: the device has no derivative matrices for 3-D coordinates")
        try:
            spec = _kernels.device_spec(kernel, single=kernel_to_spec)
        except NotImplementedError as ex:
            raise NotImplementedError("fisher_information needs a kernel with a device form (RBF, AnisotropicRBF, VonKarman, "
                                      "AnisotropicVonKarman or a sum of up to four of them); WhiteKernel, Matern and longer "
                                      "sums take the dense route, which has no derivative matrices: %s" % ex)
        # y plays no part in F: the solve is only what builds and keeps the factor
        _, _, _, factor = ops.gp_solve(spec, self.X, self.y, self.y_err, keep=True, want_alpha=False, ctx=ctx)
        try:
            F_p = ops.gp_fisher(spec, factor, self.X, ctx=ctx)
        finally:
            factor.free(keep_memory=True)
        return _kernels.fisher_theta(kernel, F_p)

    def optimizer(self, kernel):
        """L-BFGS-B on -log L over theta (log_likelihood.py:43-62)."""
        template = kernel
        # X, y, y_err do not change during the fit: they go to the device once, every evaluation sends only theta
        resident = None
        if os.environ.get("TGP_ML_RESIDENT", "1") != "0" and not self.distributed and not self.three_d:
            resident = ops.ResidentProblem(self.X, self.y, self.y_err)

        def cost(theta, ctx=None, work=None):
            # `work`: a kernel object owned by this evaluation slot whose theta is set in place -- what clone_with_theta
            # does after its (much slower) clone; the host side of an evaluation is otherwise mostly that clone
            if work is None:
                work = template.clone_with_theta(theta)
            else:
                work.theta = theta
            return -self.log_likelihood(work, ctx=ctx, resident=resident)

        try:
            best = self._minimise(cost, template, resident)
        finally:
            if resident is not None:
                resident.close()
        fitted = template.clone_with_theta(best)
        self._kernel = copy.deepcopy(fitted)
        self._logL = self.log_likelihood(self._kernel)
        return fitted

    def _use_exact_gradient(self, template):
        if self.three_d:                                  # the exact gradient is 2-D: finite differences, whatever was asked for
            return False
        if self.gradient == "analytic-vk":                # the exact gradient for all four kinds (seam S2h), asked for explicitly
            try:
                if isinstance(self._device_spec(template), ops.KernelSumSpec):
                    _kernels.sum_spec_jacobian(template)
                else:
                    spec_jacobian(template, von_karman=True)
            except NotImplementedError:
                raise NotImplementedError("TGP_ML_GRADIENT=analytic-vk: %r has no analytic derivative on the device (kernel "
                                          "trees of kernel_to_spec, and sums of them, only)" % (template,))
            return True
        if self.gradient not in ("analytic", "auto"):
            return False
        try:
            spec_jacobian(template)
            gaussian = kernel_to_spec(template).kind in (_lib.TGP_RBF, _lib.TGP_ARBF)
        except NotImplementedError:
            gaussian = False
        if self.gradient == "analytic":
            if not gaussian:
                raise NotImplementedError("TGP_ML_GRADIENT=analytic: %r has no analytic derivative (Gaussian kernels only, as in "
                                          "the reference: treegp/kernels.py:128-150)" % (template,))
            return True
        # (on the multi-GPU route K^-1 would be formed by every rank on its replicated factor: not a saving there)
        return gaussian and self.ndata > _PARALLEL_MAX_N and not self.distributed and self._gradient_fits()

    def _gradient_fits(self):
        """The device gradient forms K^-1: two Np x Np buffers beside the factor, and its launches index row tiles of a
        matrix of at most 65535 rows (csrc/cov.hip: cov_plan).  Beyond either limit the fit keeps SciPy's finite differences."""
        lib = _lib.load_library()
        Np = int(lib.tgp_padded_n(self.ndata))
        if Np > 65535:
            return False
        need = 8.0 * (2.0 * Np * Np + 2.0 * float(lib.tgp_panel_elems(Np)))
        import ctypes
        free, total = ctypes.c_int64(), ctypes.c_int64()
        try:
            ctx = _lib.get_ctx()
        except RuntimeError:              # no device: nothing will run anyway, the choice is made on the size alone
            return True
        if lib.tgp_mem_info(ctx, ctypes.byref(free), ctypes.byref(total)) != 0:
            return True
        return need < 0.9 * free.value

    def _minimise(self, cost, template, resident=None):
        if self._use_exact_gradient(template):
            work = template.clone_with_theta(template.theta)

            state = {"exact": True}

            def cost_and_gradient(theta):
                work.theta = theta
                if state["exact"]:
                    try:
                        if self.gradient == "analytic-vk":
                            ll, grad = self.log_likelihood_gradient(work, resident=resident, any_kind=True)
                        else:
                            ll, grad = self.log_likelihood_gradient(work, resident=resident)
                        return -ll, -grad
                    except ops._lib.TgpError as err:
                        if self.gradient in ("analytic", "analytic-vk"):
                            raise                         # asked for explicitly: fail loudly
                        import warnings
                        warnings.warn("exact likelihood gradient unavailable (%s); continuing with finite differences" % err)
                        state["exact"] = False
                # SciPy's forward differences (the reference's scheme), one evaluation after the other
                f0 = -self.log_likelihood(work, resident=resident)
                grad = np.zeros(len(theta))
                for i in range(len(theta)):
                    shifted = np.array(theta, dtype=float)
                    shifted[i] += _FD_STEP
                    work.theta = shifted
                    grad[i] = (-self.log_likelihood(work, resident=resident) - f0) / (shifted[i] - theta[i])
                return f0, grad

            best = optimize.minimize(cost_and_gradient, template.theta, jac=True, method="L-BFGS-B")["x"]
        elif self.parallel_fd:
            ntheta = len(template.theta)
            ctxs = _contexts(ntheta + 1)
            works = [template.clone_with_theta(template.theta) for _ in range(ntheta + 1)]
            # evaluations in flight at once: all ntheta + 1 by default; TGP_ML_MAX_CONCURRENT caps it (the rest queue up)
            pool = ThreadPoolExecutor(max_workers=min(ntheta + 1, int(os.environ.get("TGP_ML_MAX_CONCURRENT", ntheta + 1))))

            def cost_and_gradient(theta):
                # SciPy's 2-point scheme for L-BFGS-B (approx_derivative, abs_step = eps): x_i + h, df / actual dx
                points = [np.array(theta, dtype=float)]
                for i in range(ntheta):
                    shifted = points[0].copy()
                    shifted[i] = points[0][i] + _FD_STEP
                    points.append(shifted)
                values = list(pool.map(cost, points, ctxs, works))
                grad = np.array([(values[i + 1] - values[0]) / (points[i + 1][i] - points[0][i]) for i in range(ntheta)])
                return values[0], grad

            try:
                best = optimize.minimize(cost_and_gradient, template.theta, jac=True, method="L-BFGS-B")["x"]
            finally:
                pool.shutdown()
        else:
            work = template.clone_with_theta(template.theta)
            best = optimize.minimize(lambda theta: cost(theta, None, work), template.theta, method="L-BFGS-B")["x"]
        return best

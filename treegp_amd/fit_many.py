"""Maximum-likelihood fits of many small GPs in lockstep: ``solve_many(gps)`` is ``for gp in gps: gp.solve()`` with one batched
device call per optimiser iteration instead of one launch chain per object and evaluation.

The reference's regime is one GP per PSF parameter, exposure or chip (README.rst:28), each fitted by its own L-BFGS-B
(treegp/log_likelihood.py:43-62, 37-82 likelihood evaluations per fit).  Here every eligible object keeps its own optimiser --
``scipy.optimize.minimize(..., jac=True, method="L-BFGS-B")`` from ``template.theta`` without bounds, exactly what
``log_likelihood._minimise`` runs -- in a thread of its own.  An objective call hands (fit, theta) to the calling thread and
blocks; when every live optimiser has either asked or finished, the caller evaluates all pending requests in one batched call
per route and releases them:

  analytic   Gaussian kernel trees with a ``spec_jacobian``: value and exact gradient of every object from
             ``ops.gp_solve_grad_batch`` (K^-1 formed on the device per problem), chain rule to theta on the host;
  analytic-vk  on request (``gradient="analytic-vk"``): every kernel ``kernel_to_spec`` describes, the von Karman kinds with
             the exact derivative of seam S2h (include/tgp.h), from ``ops.gp_solve_grad_batch_any``;
  fd         the other kernels ``kernel_to_spec`` describes (von Karman kinds), or every object with ``gradient="fd"``: SciPy's
             forward differences with ``_FD_STEP`` (log_likelihood.py's scheme, the reference's iterates), the ntheta + 1
             points of every object in one ``ops.gp_solve_batch(want_alpha=False)``.

Sums of up to four parametrised kernels (``kernels.kernel_to_sum_spec``) are eligible too: ``fd`` by default, as the single
``solve()`` differences them, and with ``gradient="analytic-vk"`` the exact route through ``ops.gp_solve_grad_batch_sum`` (K^-1
once per problem, the pair pass once per term) and ``kernels.sum_spec_jacobian``.

L-BFGS-B keeps its state in the arrays of its own call, so an object's iterates are those of a fit run alone; objects that
converge early drop out of the following calls.  All device calls are made by the calling thread.
"""
import copy
import threading

import numpy as np
from scipy import optimize

from . import _lib, ops
from .gp_interp import _batch_spec
from . import kernels as _kernels
from .kernels import kernel_to_spec, spec_jacobian
from .log_likelihood import log_likelihood, _BATCH_CALL, _FD_STEP

__all__ = ["solve_many"]


class _Abort(Exception):
    """raised inside an optimiser thread to unwind it after another thread or the evaluation has failed"""


class _Fit(object):
    """one eligible object's fit: its data, a kernel whose theta the evaluations set in place, the route of its gradient"""

    def __init__(self, index, gp, route):
        self.index, self.gp, self.route = index, gp, route
        self.template = gp.kernel
        self.work = self.template.clone_with_theta(self.template.theta)
        self.X, self.y, self.y_err = gp._X, gp._residual(), gp._y_err
        self.const = (0.5 * len(self.X)) * np.log(2.0 * np.pi)
        self.best = None

    def spec_at(self, theta):
        """(KernelSpec, d(log amp, a, b, c) / d theta or None) at theta -- for a sum (KernelSumSpec, d(log amp_t, a_t, b_t, c_t
        for every term) / d theta or None); None for a theta the kernel cannot take, which counts as a rejected point as in
        ``log_likelihood.log_likelihood``"""
        try:
            self.work.theta = theta
            spec = _device_spec(self.work)
            if isinstance(spec, ops.KernelSumSpec):
                jac = _kernels.sum_spec_jacobian(self.work) if self.route == "analytic-vk" else None
            elif self.route == "analytic-vk":
                jac = spec_jacobian(self.work, von_karman=True)
            else:
                jac = spec_jacobian(self.work) if self.route == "analytic" else None
        except (FloatingPointError, ValueError):
            return None
        return spec, jac


def _device_spec(kernel):
    """what ``_batch_spec`` found for the object: ``kernel_to_spec``'s description, or else a sum's"""
    return _kernels.device_spec(kernel, allow_sum=True, single=kernel_to_spec)


def _has_analytic_gradient(kernel):
    """the default exact route (``ops.gp_solve_grad_batch``): single Gaussian kernels; a sum keeps finite differences unless
    ``gradient="analytic-vk"`` asks for the exact route of the sums, as in the single ``solve()``"""
    try:
        spec_jacobian(kernel)
        return kernel_to_spec(kernel).kind in (_lib.TGP_RBF, _lib.TGP_ARBF)
    except NotImplementedError:
        return False


def _log_likelihoods(fits, specs):
    """log L of fits[k] with specs[k] from one batched solve; -inf for a failed factorisation or a non-finite value"""
    _, log_det, chi2, info = ops.gp_solve_batch(specs, [f.X for f in fits], [f.y for f in fits], [f.y_err for f in fits],
                                                want_alpha=False)
    with np.errstate(invalid="ignore", over="ignore"):
        ll = -0.5 * chi2 - np.array([f.const for f in fits]) - 0.5 * log_det
    return [float(ll[k]) if info[k] == 0 and np.isfinite(ll[k]) else -np.inf for k in range(len(fits))]


def _evaluate(requests):
    """{slot: (fit, theta)} -> {slot: (-log L, -d log L / d theta)}: one ``ops.gp_solve_grad_batch`` for the requests of the
    analytic route, one ``ops.gp_solve_grad_batch_any`` for those of the analytic-vk route (all four kinds;
    ``ops.gp_solve_grad_batch_sum`` when a sum is among them) and one ``ops.gp_solve_batch`` for those of the finite-difference
    route."""
    out = {}
    exact, exact_fits, exact_specs = [], [], []
    any_kind = False
    fd, fd_fits, fd_specs = [], [], []
    for slot in sorted(requests):
        fit, theta = requests[slot]
        ntheta = len(theta)
        if fit.route in ("analytic", "analytic-vk"):        # (solve_many gives every fit of a call the same exact route)
            any_kind = fit.route == "analytic-vk"
            sj = fit.spec_at(theta)
            if sj is None:
                out[slot] = (np.inf, np.zeros(ntheta))
                continue
            exact.append((slot, sj[1], ntheta))
            exact_fits.append(fit)
            exact_specs.append(sj[0])
            continue
        # SciPy's 2-point scheme for L-BFGS-B (approx_derivative, abs_step = eps): x_i + h, df / actual dx
        points = [np.array(theta, dtype=float)]
        for i in range(ntheta):
            shifted = points[0].copy()
            shifted[i] = points[0][i] + _FD_STEP
            points.append(shifted)
        specs = [fit.spec_at(p) for p in points]
        fd.append((slot, points, [s is not None for s in specs], len(fd_specs)))
        for s in specs:
            if s is not None:
                fd_fits.append(fit)
                fd_specs.append(s[0])
    if exact:
        solve_grad_batch = ops.gp_solve_grad_batch_any if any_kind else ops.gp_solve_grad_batch
        if any(isinstance(s, ops.KernelSumSpec) for s in exact_specs):
            solve_grad_batch = ops.gp_solve_grad_batch_sum          # rows (nterms_b, 4) per problem, flattened for the chain rule
        log_det, chi2, g4, info = solve_grad_batch(exact_specs, [f.X for f in exact_fits], [f.y for f in exact_fits],
                                                   [f.y_err for f in exact_fits])
        for k, (slot, jac, ntheta) in enumerate(exact):
            with np.errstate(invalid="ignore", over="ignore"):
                ll = -0.5 * chi2[k] - exact_fits[k].const - 0.5 * log_det[k]
            if info[k] != 0 or not np.isfinite(ll):
                out[slot] = (np.inf, np.zeros(ntheta))
            else:
                out[slot] = (-float(ll), -jac.dot(np.ravel(g4[k])))
    if fd:
        lls = _log_likelihoods(fd_fits, fd_specs) if fd_specs else []
        for slot, points, ok, first in fd:
            values, k = [], first
            for good in ok:
                values.append(-lls[k] if good else np.inf)
                k += int(good)
            ntheta = len(points) - 1
            with np.errstate(invalid="ignore"):
                grad = np.array([(values[i + 1] - values[0]) / (points[i + 1][i] - points[0][i]) for i in range(ntheta)])
            out[slot] = (values[0], grad)
    return out


def _lockstep(fits):
    """Run every fit's L-BFGS-B in a thread of its own; the calling thread answers their objective calls one rendezvous at a
    time through ``_evaluate``.  Returns when every optimiser has finished (``fit.best`` set).  An exception of an evaluation or
    of an optimiser thread releases every waiter and is raised here after all threads have joined."""
    cond = threading.Condition()
    pending, results = {}, {}
    state = {"live": len(fits), "error": None}

    def ask(slot, theta):
        with cond:
            if state["error"] is not None:
                raise _Abort()
            pending[slot] = (fits[slot], np.array(theta, dtype=float))
            cond.notify_all()
            while slot not in results and state["error"] is None:
                cond.wait()
            if state["error"] is not None:
                raise _Abort()
            return results.pop(slot)

    def run(slot):
        fit = fits[slot]
        try:
            fit.best = optimize.minimize(lambda theta: ask(slot, theta), fit.template.theta, jac=True, method="L-BFGS-B")["x"]
        except _Abort:
            pass
        except BaseException as ex:                        # noqa: B902  (re-raised by the calling thread)
            with cond:
                if state["error"] is None:
                    state["error"] = ex
        finally:
            with cond:
                state["live"] -= 1
                cond.notify_all()

    threads = [threading.Thread(target=run, args=(slot,), name="solve_many-%d" % slot, daemon=True) for slot in range(len(fits))]
    for t in threads:
        t.start()
    try:
        while True:
            with cond:
                while state["error"] is None and state["live"] > 0 and len(pending) < state["live"]:
                    cond.wait()
                if state["error"] is not None or state["live"] == 0:
                    break
                batch = dict(pending)
                pending.clear()
            answers = _evaluate(batch)                      # outside the lock: the waiters hold nothing
            with cond:
                results.update(answers)
                cond.notify_all()
    except BaseException as ex:
        with cond:
            if state["error"] is None:
                state["error"] = ex
    finally:
        with cond:
            if state["error"] is None and state["live"] > 0:
                state["error"] = _Abort()
            cond.notify_all()
        for t in threads:
            t.join()
    if state["error"] is not None:
        raise state["error"]


def solve_many(gps, gradient="auto"):
    """``for gp in gps: gp.solve()`` with the maximum-likelihood fits of many small GPs run in lockstep: one batched device call
    per optimiser iteration for all of them.  ``gps``: initialised GPInterpolation objects.  The objects with
    ``optimizer="log-likelihood"`` whose kernel ``kernels.device_spec`` describes (one parametrised kernel, or a sum of up to
    four: "0.3**2 * AnisotropicVonKarman(...) + 0.5**2 * AnisotropicRBF(...)"), that are not on the multi-GPU route and hold at
    most 4096 points are fitted here, at most 256 at a time; afterwards each is in the state its own ``solve()`` leaves
    (``_init_theta``, the fitted ``kernel``, ``_optimizer`` with ``_kernel`` and ``_logL``, no cached solution).  Every other
    object then goes through its own ``solve()``, in list order.

    ``gradient``: "auto" (default) gives L-BFGS-B the exact gradient for the Gaussian kernels (RBF, AnisotropicRBF) and SciPy's
    forward differences for the von Karman kinds and for sums (what the single ``solve()`` does for them); "fd" forward
    differences for every object, the reference's iterates;
    "analytic" raises NotImplementedError for an eligible object whose kernel has no analytic derivative; "analytic-vk" gives
    every eligible object, the von Karman kinds and sums included, the exact gradient (``ops.gp_solve_grad_batch_any``, or
    ``ops.gp_solve_grad_batch_sum`` when a sum is among the objects: a derivative the reference does not have), one call per
    rendezvous."""
    if gradient not in ("auto", "fd", "analytic", "analytic-vk"):
        raise ValueError("solve_many: gradient must be 'auto', 'fd', 'analytic' or 'analytic-vk', got %r" % (gradient,))
    gps = list(gps)
    fits, batched = [], set()
    for i, gp in enumerate(gps):
        if gp.optimizer != "log-likelihood" or _batch_spec(gp) is None:
            continue
        if gradient == "analytic-vk":                      # every kernel _batch_spec accepts has a derivative there
            fits.append(_Fit(i, gp, "analytic-vk"))
            batched.add(i)
            continue
        exact = _has_analytic_gradient(gp.kernel)
        if gradient == "analytic" and not exact:
            raise NotImplementedError("solve_many(gradient='analytic'): GP %d: %r has no analytic derivative (Gaussian kernels "
                                      "only, as in the reference: treegp/kernels.py:128-150)" % (i, gp.kernel))
        fits.append(_Fit(i, gp, "analytic" if exact and gradient != "fd" else "fd"))
        batched.add(i)
    for c0 in range(0, len(fits), _BATCH_CALL):
        group = fits[c0:c0 + _BATCH_CALL]
        _lockstep(group)
        fitted = [f.template.clone_with_theta(f.best) for f in group]
        logls = _log_likelihoods(group, [_device_spec(k) for k in fitted])
        for f, kernel, logl in zip(group, fitted, logls):
            gp = f.gp
            gp._init_theta = [copy.deepcopy(f.template).theta]
            gp._drop_solution()
            with gp._scope():
                gp._optimizer = log_likelihood(f.X, f.y, f.y_err)
            gp._optimizer._kernel = copy.deepcopy(kernel)
            gp._optimizer._logL = logl
            gp.kernel = kernel
    for i, gp in enumerate(gps):
        if i not in batched:
            gp.solve()

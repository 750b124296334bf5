"""Covariance functions with treegp's interface, evaluated on the GPU.

Mirrors ``treegp/kernels.py`` of the reference: ``eval_kernel`` (:17-59), ``AnisotropicRBF``
(:62-186), ``VonKarman`` (:189-301), ``AnisotropicVonKarman`` (:304-420).  The classes stay
scikit-learn ``Kernel`` objects (theta, bounds, clone_with_theta, ``amp * kernel`` products all
work as in the reference) but ``__call__`` goes to ``tgp_kernel_matrix`` (include/tgp.h, seam
S1) instead of scipy ``pdist/cdist`` + ``special.kv``.  There is no host evaluation path.

``kernel_to_spec`` turns a kernel object tree into the plain numbers the device kernels take.
"""
import numpy as np
from sklearn.gaussian_process.kernels import (ConstantKernel, Hyperparameter, Kernel, NormalizedKernelMixin,
                                              Product, RBF, StationaryKernelMixin, Sum)

from . import _lib
from . import ops


def _all_kernel_classes(cls=Kernel):
    found = []
    for sub in cls.__subclasses__():
        found.append(sub)
        found.extend(_all_kernel_classes(sub))
    return found


def eval_kernel(kernel):
    """Build a kernel object from its repr-like string, e.g. ``"0.5**2 * AnisotropicRBF(invLam=array(...))"``.

    Same contract as the reference (kernels.py:17-59): every scikit-learn ``Kernel`` subclass
    (which includes the classes of this module) and ``array`` are visible to the expression;
    a failing expression raises RuntimeError, an un-instantiated class raises TypeError.
    """
    scope = {c.__name__: c for c in _all_kernel_classes()}
    scope["array"] = np.array
    try:
        built = eval(kernel, scope)
    except Exception as exc:
        msg = "Failed to evaluate kernel string {0!r}.  Original exception: {1}".format(kernel, exc)
        raise RuntimeError(msg)
    if type(built.theta) is property:        # the expression named a class without instantiating it
        raise TypeError("String provided was not initialized properly")
    return built


class _CholeskyParametrised(StationaryKernelMixin, NormalizedKernelMixin, Kernel):
    """Shared parametrisation of the two invLam kernels (kernels.py:95-112,154-186 and
    :336-353,388-420): invLam = L L^T, theta = [log diag(L), strictly-lower L row-wise]."""

    _tgp_kind = None

    def __init__(self, invLam=None, scale_length=None, bounds=(-5, 5)):
        if scale_length is not None and invLam is not None:
            raise TypeError("Cannot set both invLam and scale_length in %s." % type(self).__name__)
        if scale_length is not None:                     # axis-aligned: invLam = diag(1 / l^2)
            invLam = np.diag(np.reciprocal(np.square(np.array(scale_length, dtype=float))))
        n = invLam.shape[0]
        self.ndim, self.ntheta = n, n * (n + 1) // 2
        self._d, self._t = np.diag_indices(n), np.tril_indices(n, -1)      # where theta lands in L
        self.set_params(invLam)
        limits = np.array(bounds)
        if limits.ndim == 1:                             # one (min, max) for every element of theta
            limits = np.tile(limits, (self.ntheta, 1))
        assert limits.shape == (self.ntheta, 2)
        self._bounds = limits

    # -- scikit-learn plumbing -------------------------------------------------------------
    @property
    def hyperparameter_cholesky_factor(self):
        return Hyperparameter("CholeskyFactor", "numeric", (1e-5, 1e5), int(self.ntheta))

    def get_params(self, deep=True):
        # only invLam: a clone therefore comes back with the default bounds (reference quirk)
        return dict(invLam=self.invLam)

    def set_params(self, invLam=None):
        """invLam -> L (lower Cholesky factor) -> theta = [log diag(L), strictly-lower L]."""
        if invLam is None:
            return
        chol = np.linalg.cholesky(invLam)
        self.invLam, self._L = invLam, chol
        self._theta = np.concatenate([np.log(chol[self._d]), chol[self._t]])

    @property
    def theta(self):
        return self._theta

    @theta.setter
    def theta(self, theta):
        """theta -> L -> invLam = L L^T (always positive definite)."""
        chol = np.zeros_like(self.invLam)
        chol[self._d] = np.exp(theta[:self.ndim])
        chol[self._t] = theta[self.ndim:]
        self._theta, self._L = theta, chol
        self.invLam = chol.dot(chol.T)

    @property
    def bounds(self):
        return self._bounds

    def __repr__(self):
        return "%s(invLam=%r)" % (type(self).__name__, self.invLam)

    # -- evaluation ------------------------------------------------------------------------
    def _spec(self):
        if self.ndim == 3:
            return _invlam_spec3(self._tgp_kind, self.invLam, 1.0)
        return _invlam_spec(self._tgp_kind, self.invLam, 1.0)

    def __call__(self, X, Y=None, eval_gradient=False):
        X = np.atleast_2d(X)
        if eval_gradient and Y is not None:
            raise ValueError("Gradient can only be evaluated when Y is None.")
        if X.shape[1] != self.ndim:
            raise ValueError("X has %d columns, kernel has ndim=%d" % (X.shape[1], self.ndim))
        K = ops.kernel_matrix(self._spec(), X, None if Y is None else np.atleast_2d(Y))
        if not eval_gradient:
            return K
        return K, self._gradient(X, K)

    def invLam_gradient(self):
        """d invLam / d theta_k, shape (ntheta, ndim, ndim): dL L^T + L dL^T with dL the single-element matrices of
        ``treegp/kernels.py:138-145`` (L_kk for the log-diagonal thetas, 1 for the strictly-lower ones)."""
        dL = np.zeros((self.ntheta, self.ndim, self.ndim))
        dL[(np.arange(self.ndim),) + self._d] = self._L[self._d]
        dL[(np.arange(self.ndim, self.ntheta),) + self._t] = 1.0
        half = np.dot(dL, self._L.T)
        return half + np.transpose(half, (0, 2, 1))

    def _gradient(self, X, K):
        raise ValueError("Gradient can not be evaluated.")          # AnisotropicVonKarman, kernels.py:383-384


class AnisotropicRBF(_CholeskyParametrised):
    """exp(-0.5 (x-x')^T invLam (x-x'))  -- treegp/kernels.py:62-186.

    :param invLam:        inverse covariance matrix (ndim x ndim, ndim in {1, 2, 3} on the GPU).
    :param scale_length:  axis-aligned scale lengths instead of invLam (exactly one of the two).
    :param bounds:        bounds on theta, (2,) or (ntheta, 2).
    """
    _tgp_kind = _lib.TGP_ARBF

    def _gradient(self, X, K):
        """dK/dtheta_k = -1/2 K dX^T (d invLam/d theta_k) dX (kernels.py:128-150), from the device's K; host arithmetic on
        (n, n) arrays, one per theta -- nothing on the fit's path asks for it (log_likelihood.py:57 passes no jac; the
        likelihood gradient has its own device entry point, ops.gp_loglik_grad)."""
        if self.hyperparameter_cholesky_factor.fixed:            # kernels.py:128-130: no free parameter, an (n, n, 0) gradient
            return np.empty((X.shape[0], X.shape[0], 0))
        d = [X[:, None, a] - X[None, :, a] for a in range(self.ndim)]
        out = np.empty(K.shape + (self.ntheta,))
        for k, g in enumerate(self.invLam_gradient()):
            q = np.zeros_like(K)
            for a in range(self.ndim):
                for b in range(self.ndim):
                    if g[a, b] != 0.0:
                        q += g[a, b] * d[a] * d[b]
            out[:, :, k] = -0.5 * K * q
        return out


class AnisotropicVonKarman(_CholeskyParametrised):
    """d^(5/6) K_{5/6}(2 pi d) / lim0 with the Mahalanobis distance d -- treegp/kernels.py:304-420."""
    _tgp_kind = _lib.TGP_AVK


class VonKarman(StationaryKernelMixin, NormalizedKernelMixin, Kernel):
    """(d/l)^(5/6) K_{5/6}(2 pi d/l) / lim0, Euclidean d -- treegp/kernels.py:189-301.

    :param length_scale:         scalar length scale (theta = log length_scale).
    :param length_scale_bounds:  bounds on length_scale.
    """

    def __init__(self, length_scale=1.0, length_scale_bounds=(1e-5, 1e5)):
        self.length_scale, self.length_scale_bounds = length_scale, length_scale_bounds

    @property
    def anisotropic(self):
        scale = self.length_scale
        return bool(np.iterable(scale) and len(scale) > 1)

    @property
    def hyperparameter_length_scale(self):
        count = len(self.length_scale) if self.anisotropic else 1
        return Hyperparameter("length_scale", "numeric", self.length_scale_bounds, count)

    def _spec(self, ndim=2):
        """the device description for coordinates of `ndim` columns (the kernel itself carries no dimension)"""
        if self.anisotropic:
            raise NotImplementedError("per-axis length scales are not defined for VonKarman distances")
        ell = float(np.ravel(self.length_scale)[0])
        if ndim == 3:
            return ops.KernelSpec3(_lib.TGP_VK, amp=1.0, ell=ell)
        return ops.KernelSpec(_lib.TGP_VK, amp=1.0, ell=ell)

    def __call__(self, X, Y=None, eval_gradient=False):
        X = np.atleast_2d(X)
        if eval_gradient and Y is not None:
            raise ValueError("Gradient can only be evaluated when Y is None.")
        K = ops.kernel_matrix(self._spec(3 if X.shape[1] == 3 else 2), X, None if Y is None else np.atleast_2d(Y))
        if not eval_gradient:
            return K
        # what the reference returns (kernels.py:278-288): K times the Euclidean distances -- not dK/d log l, reproduced as is
        if self.hyperparameter_length_scale.fixed:
            return K, np.empty((X.shape[0], X.shape[0], 0))
        diff = X[:, None, :] - X[None, :, :]
        return K, (K * np.sqrt(np.sum(diff * diff, axis=-1)))[:, :, np.newaxis]

    def __repr__(self):
        name = type(self).__name__
        if self.anisotropic:
            return "%s(length_scale=[%s])" % (name, ", ".join("%.3g" % v for v in self.length_scale))
        return "%s(length_scale=%.3g)" % (name, np.ravel(self.length_scale)[0])


# ---- kernel object -> device description ---------------------------------------------------
def _invlam_spec(kind, invLam, amp):
    invLam = np.asarray(invLam, dtype=np.float64)
    nd = invLam.shape[0]
    if nd == 1:
        return ops.KernelSpec(kind, amp=amp, a=invLam[0, 0], b=0.0, c=0.0)
    if nd == 2:
        return ops.KernelSpec(kind, amp=amp, a=invLam[0, 0], b=0.5 * (invLam[0, 1] + invLam[1, 0]), c=invLam[1, 1])
    raise NotImplementedError("the GPU kernels cover 1-D and 2-D coordinates (treegp's own scope), got ndim=%d" % nd)


def kernel_to_spec(kernel):
    """{kind, amp, a, b, c, ell} for the supported kernel trees:
    [ConstantKernel *]* one of RBF / AnisotropicRBF / VonKarman / AnisotropicVonKarman
    (what every reference test and doc string builds, e.g. tests/test_gp_interp.py:31,123).
    Anything else raises NotImplementedError -- there is no silent host fallback."""
    amp = 1.0
    node = kernel
    while isinstance(node, Product):
        if isinstance(node.k1, ConstantKernel):
            amp *= float(node.k1.constant_value)
            node = node.k2
        elif isinstance(node.k2, ConstantKernel):
            amp *= float(node.k2.constant_value)
            node = node.k1
        else:
            raise NotImplementedError("only ConstantKernel * <stationary kernel> products run on the GPU, got %r" % (kernel,))
    if isinstance(node, AnisotropicRBF):
        return _invlam_spec(_lib.TGP_ARBF, node.invLam, amp)
    if isinstance(node, AnisotropicVonKarman):
        return _invlam_spec(_lib.TGP_AVK, node.invLam, amp)
    if isinstance(node, VonKarman):
        s = node._spec()
        s.amp = amp
        return s
    if type(node) is RBF:                       # exactly RBF: scikit-learn's Matern derives from it
        ls = np.ravel(np.asarray(node.length_scale, dtype=np.float64))
        if ls.size == 1:
            inv = 1.0 / ls[0] ** 2
            return ops.KernelSpec(_lib.TGP_RBF, amp=amp, a=inv, b=0.0, c=inv)
        if ls.size == 2:
            return ops.KernelSpec(_lib.TGP_RBF, amp=amp, a=1.0 / ls[0] ** 2, b=0.0, c=1.0 / ls[1] ** 2)
        raise NotImplementedError("RBF with %d length scales" % ls.size)
    raise NotImplementedError("kernel %r is not supported by the GPU hot path" % (kernel,))


def _invlam_spec3(kind, invLam, amp):
    """``ops.KernelSpec3`` of a 3 x 3 invLam; a non-symmetric one is averaged, as ``_invlam_spec`` does"""
    invLam = np.asarray(invLam, dtype=np.float64)
    if invLam.shape != (3, 3):
        raise NotImplementedError("a 3-D kernel needs a 3 x 3 invLam, got shape %r" % (invLam.shape,))
    sym = 0.5 * (invLam + invLam.T)
    return ops.KernelSpec3(kind, amp=amp, m=(invLam[0, 0], sym[0, 1], sym[0, 2], invLam[1, 1], sym[1, 2], invLam[2, 2]))


def kernel_to_spec3(kernel):
    """``ops.KernelSpec3`` (kind, amp, m = invLam xx, xy, xz, yy, yz, zz, ell) for the trees ``kernel_to_spec`` accepts, over
    (n, 3) coordinates: [ConstantKernel *]* one of RBF (one or three length scales) / AnisotropicRBF / AnisotropicVonKarman
    (3 x 3 invLam) / VonKarman.  Anything else raises NotImplementedError -- there is no silent host fallback."""
    amp = 1.0
    node = kernel
    while isinstance(node, Product):
        if isinstance(node.k1, ConstantKernel):
            amp *= float(node.k1.constant_value)
            node = node.k2
        elif isinstance(node.k2, ConstantKernel):
            amp *= float(node.k2.constant_value)
            node = node.k1
        else:
            raise NotImplementedError("only ConstantKernel * <stationary kernel> products run on the GPU, got %r" % (kernel,))
    if isinstance(node, AnisotropicRBF):
        return _invlam_spec3(_lib.TGP_ARBF, node.invLam, amp)
    if isinstance(node, AnisotropicVonKarman):
        return _invlam_spec3(_lib.TGP_AVK, node.invLam, amp)
    if isinstance(node, VonKarman):
        s = node._spec(3)
        s.amp = amp
        return s
    if type(node) is RBF:                       # exactly RBF: scikit-learn's Matern derives from it
        ls = np.ravel(np.asarray(node.length_scale, dtype=np.float64))
        if ls.size == 1:
            ls = np.repeat(ls, 3)
        if ls.size != 3:
            raise NotImplementedError("RBF over 3-D coordinates needs one or three length scales, got %d" % ls.size)
        return ops.KernelSpec3(_lib.TGP_RBF, amp=amp, m=(1.0 / ls[0] ** 2, 0.0, 0.0, 1.0 / ls[1] ** 2, 0.0, 1.0 / ls[2] ** 2))
    raise NotImplementedError("kernel %r is not supported by the GPU hot path" % (kernel,))


def _sum_leaves(kernel):
    """the terms of a (nested) scikit-learn Sum in its own order, k1 before k2"""
    if isinstance(kernel, Sum):
        return _sum_leaves(kernel.k1) + _sum_leaves(kernel.k2)
    return [kernel]


def kernel_to_sum_spec(kernel):
    """``ops.KernelSumSpec`` for a (nested) scikit-learn ``Sum`` whose leaves, in scikit-learn's own order (k1 before k2), are
    2 .. TGP_SUM_MAX trees ``kernel_to_spec`` accepts -- e.g. "0.3**2 * AnisotropicVonKarman(...) + 0.5**2 * AnisotropicRBF(...)".
    Everything else raises NotImplementedError and keeps the dense route: any tree with a WhiteKernel or a Matern leaf, a
    constant multiplying a whole sum, more than TGP_SUM_MAX terms.  There is no silent host fallback."""
    if not isinstance(kernel, Sum):
        raise NotImplementedError("not a sum of kernels: %r" % (kernel,))
    leaves = _sum_leaves(kernel)
    if len(leaves) > _lib.TGP_SUM_MAX:
        raise NotImplementedError("sums of at most %d kernels run on the GPU, got %d terms in %r"
                                  % (_lib.TGP_SUM_MAX, len(leaves), kernel))
    return ops.KernelSumSpec([kernel_to_spec(leaf) for leaf in leaves])


def device_spec(kernel, allow_sum=True, single=None, ndim=2):
    """The device description of a kernel for the single-problem routes: ``kernel_to_spec``'s ``ops.KernelSpec``, or else
    ``kernel_to_sum_spec``'s ``ops.KernelSumSpec``; NotImplementedError for every other tree (the dense route).
    ``allow_sum=False``: sums raise too (the multi-GPU engine has no sum-aware K build: they keep the dense route there).
    ``single``: the caller's own ``kernel_to_spec`` name, so that the modules' call sites keep resolving single kernels
    through the name they import (their tests stand in for it there).
    ``ndim``: the number of columns of the coordinates (the isotropic kernels carry none).  ``ndim == 3``: ``kernel_to_spec3``'s
    ``ops.KernelSpec3``; sums of 3-D kernels raise NotImplementedError whatever ``allow_sum`` says (they keep the dense route)."""
    if ndim == 3:
        return kernel_to_spec3(kernel)
    try:
        return (single or kernel_to_spec)(kernel)
    except NotImplementedError:
        if not allow_sum:
            raise
        return kernel_to_sum_spec(kernel)


def local_spec(kernel, X, what, single=None):
    """The 2-D ``ops.KernelSpec`` of ``kernel`` for the routes of the local conditionals (``GPInterpolation.predict_loo_local``
    and its scores, ``optimizer="local-likelihood"``), or their refusals, in the style of ``predict_local``'s: NotImplementedError
    naming ``what`` for 3-D coordinates ``X``, for the kernel trees of the dense route and for sums of kernels."""
    if np.ndim(X) == 2 and np.shape(X)[1] == 3:
        raise NotImplementedError("%s takes 1-D or 2-D coordinates: the neighbour search has no 3-D form" % what)
    try:
        spec = device_spec(kernel, single=single or kernel_to_spec)
    except NotImplementedError:
        raise NotImplementedError("%s needs one kernel with a device form (RBF, AnisotropicRBF, VonKarman, "
                                  "AnisotropicVonKarman, optionally times a constant); %r takes the dense route" % (what, kernel))
    if isinstance(spec, ops.KernelSumSpec):
        raise NotImplementedError("%s takes one parametrised kernel: a sum of kernels has no single metric to rank "
                                  "neighbours by; got %r" % (what, kernel))
    return spec


def sum_spec_jacobian(kernel):
    """d(log amp_t, a_t, b_t, c_t for every term t) / d theta, shape (ntheta, 4 * nterms), for the sums ``kernel_to_sum_spec``
    accepts: block structured, the theta of a Sum being k1.theta then k2.theta, term t's rows ``spec_jacobian(term_t,
    von_karman=True)`` in columns 4 t .. 4 t + 3.  Its product with the flattened ``ops.gp_loglik_grad_sum`` is d logL / d theta."""
    if not isinstance(kernel, Sum):
        raise NotImplementedError("not a sum of kernels: %r" % (kernel,))
    blocks = [spec_jacobian(leaf, von_karman=True) for leaf in _sum_leaves(kernel)]
    out = np.zeros((sum(len(b) for b in blocks), 4 * len(blocks)))
    row = 0
    for t, b in enumerate(blocks):
        out[row:row + len(b), 4 * t:4 * t + 4] = b
        row += len(b)
    return out


def fisher_theta(kernel, F_p):
    """J F_p J^T: the Fisher information of scikit-learn's theta from ``ops.gp_fisher``'s matrix in the device's parameters
    (log amp_t, a_t, b_t, c_t per term).  J is ``spec_jacobian(kernel, von_karman=True)`` (ntheta x 4) for one parametrised
    kernel and ``sum_spec_jacobian(kernel)`` for a sum; fixed hyper-parameters have no row in J and drop out.
    NotImplementedError for the trees ``device_spec`` does not describe."""
    device_spec(kernel)                                     # the same gate as the device route (raises NotImplementedError)
    J = sum_spec_jacobian(kernel) if isinstance(kernel, Sum) else spec_jacobian(kernel, von_karman=True)
    F_p = np.asarray(F_p, dtype=np.float64)
    if F_p.shape != (J.shape[1], J.shape[1]):
        raise ValueError("fisher_theta: F_p has shape %r, the kernel needs (%d, %d)" % (F_p.shape, J.shape[1], J.shape[1]))
    return J.dot(F_p).dot(J.T)


def spec_jacobian(kernel, *, von_karman=False):
    """d(log amp, a, b, c) / d theta, shape (ntheta, 4), for the Gaussian kernel trees ``kernel_to_spec`` accepts
    (theta in scikit-learn's order: a Product's k1 first).  ``ops.gp_loglik_grad`` returns d logL / d(log amp, a, b, c);
    its product with this matrix is d logL / d theta with the kernel derivative of the reference:
    dK/dtheta_k = -1/2 K dX^T (dInvLam/dtheta_k) dX with dInvLam = dL L^T + L dL^T, dL the single-element matrices of
    ``treegp/kernels.py:138-145`` (AnisotropicRBF), and scikit-learn's own for ConstantKernel (K) and RBF.

    ``von_karman=True`` adds the von Karman classes, for the four numbers of ``ops.gp_loglik_grad_any`` (a derivative the
    reference does not have: kernels.py:278-288, 383-384): AnisotropicVonKarman has AnisotropicRBF's parametrisation and rows;
    VonKarman has a = c = l^-2, theta = log l, the row of an isotropic RBF."""
    if isinstance(kernel, Product):
        return np.vstack([spec_jacobian(kernel.k1, von_karman=von_karman), spec_jacobian(kernel.k2, von_karman=von_karman)])
    if isinstance(kernel, ConstantKernel):
        if kernel.hyperparameter_constant_value.fixed:
            return np.zeros((0, 4))
        return np.array([[1.0, 0.0, 0.0, 0.0]])
    if isinstance(kernel, AnisotropicRBF) or (von_karman and isinstance(kernel, AnisotropicVonKarman)):
        if kernel.hyperparameter_cholesky_factor.fixed:         # theta is empty then (kernels.py:128-130)
            return np.zeros((0, 4))
        nd = kernel.ndim
        rows = []
        for g in kernel.invLam_gradient():
            rows.append([0.0, g[0, 0], g[0, 1] if nd == 2 else 0.0, g[1, 1] if nd == 2 else 0.0])
        return np.array(rows).reshape(kernel.ntheta, 4)
    if type(kernel) is RBF:
        if kernel.hyperparameter_length_scale.fixed:
            return np.zeros((0, 4))
        ls = np.ravel(np.asarray(kernel.length_scale, dtype=np.float64))
        if ls.size == 1:                                    # a = c = l^-2, theta = log l
            return np.array([[0.0, -2.0 / ls[0] ** 2, 0.0, -2.0 / ls[0] ** 2]])
        if ls.size == 2:
            return np.array([[0.0, -2.0 / ls[0] ** 2, 0.0, 0.0], [0.0, 0.0, 0.0, -2.0 / ls[1] ** 2]])
    if von_karman and isinstance(kernel, VonKarman) and not kernel.anisotropic:
        if kernel.hyperparameter_length_scale.fixed:
            return np.zeros((0, 4))
        ell = float(np.ravel(kernel.length_scale)[0])
        return np.array([[0.0, -2.0 / ell ** 2, 0.0, -2.0 / ell ** 2]])
    raise NotImplementedError("no analytic derivative for %r (the reference has one for AnisotropicRBF only: "
                              "treegp/kernels.py:128-150)" % (kernel,))

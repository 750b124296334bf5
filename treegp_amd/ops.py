"""NumPy-facing wrappers of the C-ABI seams (include/tgp.h).  Every function runs on the GPU
through libtgp.so; nothing here computes on the host.

A kernel is described by ``KernelSpec`` -- the plain numbers the device needs -- which
``treegp_amd.kernels.kernel_to_spec`` derives from a scikit-learn kernel object.
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _lib
from ._lib import TgpKernel, TgpKernel3, TgpKernelSum, check, f64, ptr, as_xy, as_xyz


class KernelSpec(object):
    __slots__ = ("kind", "amp", "a", "b", "c", "ell")

    def __init__(self, kind, amp=1.0, a=1.0, b=0.0, c=1.0, ell=1.0):
        self.kind, self.amp, self.a, self.b, self.c, self.ell = int(kind), float(amp), float(a), float(b), float(c), float(ell)

    def to_c(self):
        return TgpKernel(self.kind, 0, self.amp, self.a, self.b, self.c, self.ell)

    def __repr__(self):
        return "KernelSpec(kind=%d, amp=%r, a=%r, b=%r, c=%r, ell=%r)" % (self.kind, self.amp, self.a, self.b, self.c, self.ell)


class KernelSumSpec(object):
    """A sum of 1 .. ``_lib.TGP_SUM_MAX`` parametrised kernels (a list of ``KernelSpec``, in the order the values are added):
    what ``treegp_amd.kernels.kernel_to_sum_spec`` derives from a scikit-learn ``Sum`` (2 terms or more; with one term every
    entry is its single-kernel namesake, bit for bit).  ``kernel_matrix``, ``gp_solve``,
    ``gp_predict``, ``gp_predict_grad``, ``gp_predict_cov`` and ``gp_predict_var`` take it wherever they take a ``KernelSpec``
    and go to the ``_sum`` entries of include/tgp.h (seams S1s / S2s); ``gp_loglik_grad_sum`` is its likelihood gradient.
    The batched calls ``gp_solve_batch``, ``gp_loo_batch`` and ``gp_posterior_batch`` take it among their kernels (seam S2i),
    ``gp_solve_grad_batch_sum`` is the batched likelihood gradient and ``kbuild_batch`` returns what the batched K build stores.
    The multi-GPU engine does not take sums: these calls run on this process's GPU whatever the multi-GPU settings."""
    __slots__ = ("terms",)

    def __init__(self, terms):
        self.terms = list(terms)
        if not 1 <= len(self.terms) <= _lib.TGP_SUM_MAX:
            raise ValueError("a kernel sum holds 1 .. %d terms, got %d" % (_lib.TGP_SUM_MAX, len(self.terms)))

    @property
    def amp(self):
        """k(x, x): the amplitudes added in term order, the diagonal the device writes"""
        total = self.terms[0].amp
        for t in self.terms[1:]:
            total = total + t.amp
        return total

    def to_c(self):
        c = TgpKernelSum()
        c.nterms = len(self.terms)
        for i, t in enumerate(self.terms):
            c.term[i] = t.to_c()
        return c

    def __repr__(self):
        return "KernelSumSpec(%r)" % (self.terms,)


class KernelSpec3(object):
    """One parametrised kernel over (n, 3) coordinates (tgp_kernel3 of include/tgp.h): ``m`` is the upper triangle of the
    symmetric invLam, row-wise (xx, xy, xz, yy, yz, zz); ``ell`` the length scale of the isotropic von Karman kind.
    ``treegp_amd.kernels.kernel_to_spec3`` derives it from a scikit-learn kernel object.  ``kernel_matrix``, ``gp_solve``,
    ``gp_predict``, ``gp_predict_grad`` (result (m, 3)), ``gp_predict_cov`` and ``gp_predict_var`` take it wherever they take a
    ``KernelSpec`` and go to the ``3`` entries; coordinates must then be (n, 3).  These calls run on this process's GPU whatever
    the multi-GPU settings."""
    __slots__ = ("kind", "amp", "m", "ell")

    def __init__(self, kind, amp=1.0, m=(1.0, 0.0, 0.0, 1.0, 0.0, 1.0), ell=1.0):
        m = tuple(float(v) for v in np.ravel(m))
        if len(m) != 6:
            raise ValueError("KernelSpec3.m holds invLam xx, xy, xz, yy, yz, zz: 6 numbers, got %d" % len(m))
        self.kind, self.amp, self.m, self.ell = int(kind), float(amp), m, float(ell)

    def to_c(self):
        return TgpKernel3(self.kind, 3, self.amp, (C.c_double * 6)(*self.m), self.ell)

    def __repr__(self):
        return "KernelSpec3(kind=%d, amp=%r, m=%r, ell=%r)" % (self.kind, self.amp, self.m, self.ell)


def _entry(lib, name, spec):
    """the library entry `name` for a KernelSpec, its `_sum` namesake (same arguments) for a KernelSumSpec, its `3` namesake for a
    KernelSpec3"""
    if isinstance(spec, KernelSumSpec):
        name += "_sum"
    elif isinstance(spec, KernelSpec3):
        name += "3"
    return getattr(lib, name), name


def _coords(spec, X):
    """the coordinates as the entry of `spec` takes them: (n, 3) for a KernelSpec3, ``as_xy``'s (n, 2) otherwise (so a 2-D spec
    given three columns keeps raising ValueError)"""
    return as_xyz(X) if isinstance(spec, KernelSpec3) else as_xy(X)


class Factor(object):
    """Device-resident Cholesky factor handle (tgp_factor*), freed with the object."""

    def __init__(self, ctx, handle, n, keepalive=None):
        self._ctx, self._h, self.n = ctx, handle, n
        self._keepalive = keepalive          # a borrowed handle (tgp_factor_borrow): the tensors that own its memory

    def free(self, keep_memory=False):
        """Default: the memory goes back to the device at once (tgp_factor_free) -- a dropped handle must not leave 17 GB (N =
        65 536; 69 GB at 131 072) attached to its context, where it can turn another solve's allocation -- the multi-GPU engine's
        replicated factor, on one rank only -- into an out-of-memory error.  keep_memory=True (the refit paths of
        GPInterpolation and the ML loop, which solve the same size again right away): the packed matrix stays with the context
        as the cache of its next solve of this size (tgp_factor_release), no hipFree + hipMalloc; TGP_FACTOR_FREE=1 overrides."""
        if self._h:
            lib = _lib.load_library()
            if keep_memory and os.environ.get("TGP_FACTOR_FREE") != "1":
                lib.tgp_factor_release(self._ctx, self._h)
            else:
                lib.tgp_factor_free(self._ctx, self._h)                 # (synchronises the context's stream first)
            self._h = None
        self._keepalive = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def kernel_matrix(spec, X, Y=None, ctx=None):
    """amp * k(X, Y) as an (n, m) array; Y=None gives the self kernel with an exact diagonal.
    Replaces kernel.__call__ (treegp/kernels.py:114-126, 249-276, 355-381)."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    fn, name = _entry(lib, "tgp_kernel_matrix", spec)
    X2 = _coords(spec, X)
    n = X2.shape[0]
    if Y is None:
        out = np.empty((n, n))
        rc = fn(ctx, C.byref(spec.to_c()), ptr(X2), n, None, 0, ptr(out))
    else:
        Y2 = _coords(spec, Y)
        m = Y2.shape[0]
        out = np.empty((n, m))
        rc = fn(ctx, C.byref(spec.to_c()), ptr(X2), n, ptr(Y2), m, ptr(out))
    check(ctx, rc, name)
    return out


def _dist_engine(n, ctx):
    """The multi-GPU engine this call should go through (treegp_amd.dist.enable / TGP_DIST=1 / backend="dist"), or None.
    A caller that names its own context stays on that context's GPU."""
    if ctx is not None:
        return None
    import sys
    d = sys.modules.get("treegp_amd.dist")
    if d is None:
        if os.environ.get("TGP_DIST") != "1":
            return None
        from . import dist as d
    return d.engine_for(n)


def gp_solve(spec, X, y, y_err=None, keep=False, want_alpha=True, ctx=None):
    """(alpha, logdet, y.alpha, factor|None) for K = amp k(X) + diag(y_err^2).
    Raises numpy.linalg.LinAlgError when K is not positive definite, as scipy.linalg.cholesky
    does at treegp/gp_interp.py:181."""
    eng = None if isinstance(spec, (KernelSumSpec, KernelSpec3)) else _dist_engine(len(X), ctx)
    if eng is not None:
        return eng.gp_solve(spec, X, y, y_err, keep=keep, want_alpha=want_alpha)
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    fn, name = _entry(lib, "tgp_gp_solve", spec)
    X2 = _coords(spec, X)
    n = X2.shape[0]
    y = f64(y)
    e = None if y_err is None else f64(y_err)
    alpha = np.empty(n) if want_alpha else None
    logdet, ydota = C.c_double(0.0), C.c_double(0.0)
    h = C.c_void_p()
    rc = fn(ctx, C.byref(spec.to_c()), ptr(X2), n, ptr(y), ptr(e), ptr(alpha), C.byref(logdet),
            C.byref(ydota), C.byref(h) if keep else None)
    check(ctx, rc, name)
    if rc > 0:
        raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % rc)
    return alpha, logdet.value, ydota.value, (Factor(ctx, h, n) if keep else None)


BATCH_NMAX = 4096      # tgp_gp_solve_batch: largest order of a problem (above it one solve alone fills the chip)


def pad_batch(Xs, ys, y_errs=None):
    """Lists of per-problem arrays -> (ns, nmax, X (nb, nmax, 2), y (nb, nmax), yerr (nb, nmax) or None), zero beyond n_b.
    1-D coordinates get a zero second column.  Raises ValueError on any shape mismatch."""
    Xs, ys = list(Xs), list(ys)
    nb = len(Xs)
    if nb < 1:
        raise ValueError("gp_solve_batch needs at least one problem")
    if len(ys) != nb:
        raise ValueError("gp_solve_batch: %d coordinate arrays but %d value arrays" % (nb, len(ys)))
    if y_errs is not None:
        y_errs = list(y_errs)
        if len(y_errs) != nb:
            raise ValueError("gp_solve_batch: %d coordinate arrays but %d error arrays" % (nb, len(y_errs)))
    X2s = [as_xy(X) for X in Xs]
    ns = np.array([X.shape[0] for X in X2s], dtype=np.int64)
    if np.any(ns < 1):
        raise ValueError("gp_solve_batch: every problem needs at least one point")
    nmax = int(ns.max())
    Xb = np.zeros((nb, nmax, 2))
    yb = np.zeros((nb, nmax))
    eb = None if y_errs is None else np.zeros((nb, nmax))
    for b in range(nb):
        n = int(ns[b])
        yv = np.asarray(ys[b], dtype=np.float64).reshape(-1) if np.ndim(ys[b]) <= 1 else None
        if yv is None or yv.shape[0] != n:
            raise ValueError("gp_solve_batch: problem %d has %d points but y of shape %r" % (b, n, np.shape(ys[b])))
        Xb[b, :n] = X2s[b]
        yb[b, :n] = yv
        if eb is not None:
            ev = np.asarray(y_errs[b], dtype=np.float64)
            if ev.ndim != 1 or ev.shape[0] != n:
                raise ValueError("gp_solve_batch: problem %d has %d points but y_err of shape %r" % (b, n, ev.shape))
            eb[b, :n] = ev
    return ns, nmax, Xb, yb, eb


def _batch_kernels(lib, name, specs):
    """(entry, its name, the ctypes array of the kernels) of a batched call: the entry `name` with an array of tgp_kernel when
    no spec is a ``KernelSumSpec`` -- the call of before sums existed -- else its `_sum` namesake (seam S2i of include/tgp.h)
    with an array of tgp_kernel_sum, every ``KernelSpec`` wrapped as a sum of one term"""
    nb = len(specs)
    if not any(isinstance(s, KernelSumSpec) for s in specs):
        ks = (TgpKernel * nb)(*[s.to_c() for s in specs])
        return getattr(lib, name), name, C.cast(ks, C.c_void_p), ks
    ks = (TgpKernelSum * nb)(*[(s if isinstance(s, KernelSumSpec) else KernelSumSpec([s])).to_c() for s in specs])
    return getattr(lib, name + "_sum"), name + "_sum", ks, ks


def gp_solve_batch(specs, Xs, ys, y_errs=None, want_alpha=True, ctx=None):
    """gp_solve for many independent small problems in one launch sequence (tgp_gp_solve_batch): problem b has kernel
    specs[b], coordinates Xs[b] (n_b, 1 or 2), values ys[b] (n_b,) and errors y_errs[b] (or none at all), n_b <= 4096.
    Returns (alphas: list of (n_b,) arrays or None, logdets (nb,), chi2 = y.alpha (nb,), info (nb,) int): info[b] > 0 is
    the order of the failing leading minor of problem b, whose other outputs are then meaningless.  Each problem's result
    does not depend on the others in the call.  ``specs`` may hold ``KernelSumSpec`` entries among the ``KernelSpec`` ones:
    the call then goes to tgp_gp_solve_batch_sum; ``gp_loo_batch`` and ``gp_posterior_batch`` take them the same way."""
    specs = list(specs)
    ns, nmax, Xb, yb, eb = pad_batch(Xs, ys, y_errs)
    nb = len(ns)
    if len(specs) != nb:
        raise ValueError("gp_solve_batch: %d kernels for %d problems" % (len(specs), nb))
    if nmax > BATCH_NMAX:
        raise ValueError("gp_solve_batch: problems of order up to %d, got %d (use gp_solve)" % (BATCH_NMAX, nmax))
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    fn, name, ks, _keep = _batch_kernels(lib, "tgp_gp_solve_batch", specs)
    alpha = np.empty((nb, nmax)) if want_alpha else None
    logdet = np.empty(nb)
    chi2 = np.empty(nb)
    info = np.zeros(nb, dtype=np.int32)
    rc = fn(ctx, nb, ks, ptr(ns), nmax, ptr(Xb), ptr(yb), ptr(eb), ptr(alpha), ptr(logdet), ptr(chi2), ptr(info))
    check(ctx, rc, name)
    alphas = [alpha[b, :int(ns[b])].copy() for b in range(nb)] if want_alpha else None
    return alphas, logdet, chi2, info.astype(np.int64)


def gp_solve_grad_batch(specs, Xs, ys, y_errs=None, ctx=None):
    """One evaluation of many gradient-driven fits in one launch sequence (tgp_gp_solve_grad_batch): gp_solve_batch plus, from
    each problem's factor and alpha in the same call, d logL / d (log amp, a, b, c) as ``gp_loglik_grad`` gives it for one
    problem.  Arguments as gp_solve_batch; Gaussian kernels only.  Returns (logdets (nb,), chi2 = y.alpha (nb,), g4 (nb, 4),
    info (nb,) int): logdets and chi2 are bit for bit gp_solve_batch's, info[b] > 0 marks a problem whose other outputs are
    meaningless, and each problem's result does not depend on the others in the call."""
    specs = list(specs)
    ns, nmax, Xb, yb, eb = pad_batch(Xs, ys, y_errs)
    nb = len(ns)
    if len(specs) != nb:
        raise ValueError("gp_solve_grad_batch: %d kernels for %d problems" % (len(specs), nb))
    if nmax > BATCH_NMAX:
        raise ValueError("gp_solve_grad_batch: problems of order up to %d, got %d (use gp_solve and gp_loglik_grad)"
                         % (BATCH_NMAX, nmax))
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    ks = (TgpKernel * nb)(*[s.to_c() for s in specs])
    logdet = np.empty(nb)
    chi2 = np.empty(nb)
    g4 = np.empty((nb, 4))
    info = np.zeros(nb, dtype=np.int32)
    rc = lib.tgp_gp_solve_grad_batch(ctx, nb, C.cast(ks, C.c_void_p), ptr(ns), nmax, ptr(Xb), ptr(yb), ptr(eb), ptr(logdet),
                                     ptr(chi2), ptr(g4), ptr(info))
    check(ctx, rc, "tgp_gp_solve_grad_batch")
    return logdet, chi2, g4, info.astype(np.int64)


def gp_solve_grad_batch_any(specs, Xs, ys, y_errs=None, ctx=None):
    """``gp_solve_grad_batch`` for all four kernel kinds, mixed freely within the call (tgp_gp_solve_grad_batch_any, seam S2h of
    include/tgp.h): for the von Karman kinds the exact derivative the reference does not have.  Same arguments and returns; for
    the Gaussian kinds the same bits."""
    specs = list(specs)
    ns, nmax, Xb, yb, eb = pad_batch(Xs, ys, y_errs)
    nb = len(ns)
    if len(specs) != nb:
        raise ValueError("gp_solve_grad_batch_any: %d kernels for %d problems" % (len(specs), nb))
    if nmax > BATCH_NMAX:
        raise ValueError("gp_solve_grad_batch_any: problems of order up to %d, got %d (use gp_solve and gp_loglik_grad_any)"
                         % (BATCH_NMAX, nmax))
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    ks = (TgpKernel * nb)(*[s.to_c() for s in specs])
    logdet = np.empty(nb)
    chi2 = np.empty(nb)
    g4 = np.empty((nb, 4))
    info = np.zeros(nb, dtype=np.int32)
    rc = lib.tgp_gp_solve_grad_batch_any(ctx, nb, C.cast(ks, C.c_void_p), ptr(ns), nmax, ptr(Xb), ptr(yb), ptr(eb), ptr(logdet),
                                         ptr(chi2), ptr(g4), ptr(info))
    check(ctx, rc, "tgp_gp_solve_grad_batch_any")
    return logdet, chi2, g4, info.astype(np.int64)


def _as_sum(spec):
    return spec if isinstance(spec, KernelSumSpec) else KernelSumSpec([spec])


def gp_solve_grad_batch_sum(specs, Xs, ys, y_errs=None, ctx=None):
    """``gp_solve_grad_batch_any`` for sums of kernels (tgp_gp_solve_grad_batch_sum, seam S2i of include/tgp.h): ``specs`` holds
    ``KernelSumSpec`` entries (a ``KernelSpec`` counts as a sum of one term), term counts and kinds mixed freely.  K^-1 is formed
    once per problem and the pair pass runs once per term.  Returns (logdets (nb,), chi2 (nb,), grads, info (nb,) int) with
    ``grads[b]`` of shape (nterms_b, 4): row t is d logL / d (log amp_t, a_t, b_t, c_t), what ``gp_loglik_grad_sum`` gives for
    one problem; ``kernels.sum_spec_jacobian`` takes its flattened rows to theta."""
    specs = [_as_sum(s) for s in specs]
    ns, nmax, Xb, yb, eb = pad_batch(Xs, ys, y_errs)
    nb = len(ns)
    if len(specs) != nb:
        raise ValueError("gp_solve_grad_batch_sum: %d kernels for %d problems" % (len(specs), nb))
    if nmax > BATCH_NMAX:
        raise ValueError("gp_solve_grad_batch_sum: problems of order up to %d, got %d (use gp_solve and gp_loglik_grad_sum)"
                         % (BATCH_NMAX, nmax))
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    ks = (TgpKernelSum * nb)(*[s.to_c() for s in specs])
    logdet = np.empty(nb)
    chi2 = np.empty(nb)
    g = np.empty((nb, _lib.TGP_SUM_MAX, 4))
    info = np.zeros(nb, dtype=np.int32)
    rc = lib.tgp_gp_solve_grad_batch_sum(ctx, nb, ks, ptr(ns), nmax, ptr(Xb), ptr(yb), ptr(eb), ptr(logdet), ptr(chi2), ptr(g),
                                         ptr(info))
    check(ctx, rc, "tgp_gp_solve_grad_batch_sum")
    return logdet, chi2, [g[b, :len(specs[b].terms)].copy() for b in range(nb)], info.astype(np.int64)


def kbuild_batch(specs, Xs, y_errs=None, ctx=None):
    """What the batched K build stores (tgp_kbuild_batch_sum, the building block of seam S2i): for every problem the lower
    triangle with its diagonal of K_b + diag(y_err_b^2) as an (n_b, n_b) array, exactly 0 above the diagonal.  ``specs``:
    ``KernelSpec`` or ``KernelSumSpec`` entries; no factorisation runs.  The batched counterpart of the single build's
    tgp_d_kbuild_lower + tgp_d_unpack_lower: it makes the stored values testable pair by pair."""
    specs = [_as_sum(s) for s in specs]
    Xs = list(Xs)
    ns, nmax, Xb, _, eb = pad_batch(Xs, [np.zeros(len(X)) for X in Xs], y_errs)
    nb = len(ns)
    if len(specs) != nb:
        raise ValueError("kbuild_batch: %d kernels for %d problems" % (len(specs), nb))
    if nmax > BATCH_NMAX:
        raise ValueError("kbuild_batch: problems of order up to %d, got %d" % (BATCH_NMAX, nmax))
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    ks = (TgpKernelSum * nb)(*[s.to_c() for s in specs])
    K = np.empty((nb, nmax, nmax))
    rc = lib.tgp_kbuild_batch_sum(ctx, nb, ks, ptr(ns), nmax, ptr(Xb), ptr(eb), ptr(K))
    check(ctx, rc, "tgp_kbuild_batch_sum")
    return [K[b, :int(ns[b]), :int(ns[b])].copy() for b in range(nb)]


def gp_loo_batch(specs, Xs, ys, y_errs=None, ctx=None):
    """gp_solve_batch plus, from each problem's factor in the same call, d_b = diag((K_b + diag(y_err_b^2))^-1)
    (tgp_gp_loo_batch): with alpha, all that the leave-one-out quantities of a GP need (treegp_amd.loo).  Arguments as
    gp_solve_batch; every kernel kind.  Returns (alphas, invdiags: lists of (n_b,) arrays, logdets (nb,), chi2 = y.alpha (nb,),
    info (nb,) int): alphas, logdets, chi2 and info are bit for bit gp_solve_batch's, info[b] > 0 marks a problem whose other
    outputs are meaningless, and each problem's result does not depend on the others in the call."""
    specs = list(specs)
    ns, nmax, Xb, yb, eb = pad_batch(Xs, ys, y_errs)
    nb = len(ns)
    if len(specs) != nb:
        raise ValueError("gp_loo_batch: %d kernels for %d problems" % (len(specs), nb))
    if nmax > BATCH_NMAX:
        raise ValueError("gp_loo_batch: problems of order up to %d, got %d (use gp_solve and factor_inv_diag)"
                         % (BATCH_NMAX, nmax))
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    fn, name, ks, _keep = _batch_kernels(lib, "tgp_gp_loo_batch", specs)
    alpha = np.empty((nb, nmax))
    invdiag = np.empty((nb, nmax))
    logdet = np.empty(nb)
    chi2 = np.empty(nb)
    info = np.zeros(nb, dtype=np.int32)
    rc = fn(ctx, nb, ks, ptr(ns), nmax, ptr(Xb), ptr(yb), ptr(eb), ptr(alpha), ptr(invdiag), ptr(logdet), ptr(chi2), ptr(info))
    check(ctx, rc, name)
    alphas = [alpha[b, :int(ns[b])].copy() for b in range(nb)]
    invdiags = [invdiag[b, :int(ns[b])].copy() for b in range(nb)]
    return alphas, invdiags, logdet, chi2, info.astype(np.int64)


POSTERIOR_MMAX = {"var": 65280, "cov": 4096}    # tgp_gp_posterior_batch: query points per problem (the row grids of S3b / S3c)


def gp_posterior_batch(specs, Xs, ys, y_errs, Xqs, what="var", want_alpha=True, ctx=None):
    """gp_solve_batch plus, from each problem's factor in the same call, the posterior at its query points Xqs[b] (m_b, 1 or 2)
    (tgp_gp_posterior_batch): what="var" gives the variance (m_b,) as gp_predict_var, what="cov" the covariance (m_b, m_b) as
    gp_predict_cov.  Returns (alphas or None, uncs, logdets, chi2, info); alphas, logdets, chi2 and info are bit for bit what
    gp_solve_batch returns for the same batch, and a problem with info[b] > 0 has meaningless outputs."""
    if what not in POSTERIOR_MMAX:
        raise ValueError("gp_posterior_batch: what must be 'var' or 'cov', got %r" % (what,))
    specs = list(specs)
    ns, nmax, Xb, yb, eb = pad_batch(Xs, ys, y_errs)
    nb = len(ns)
    if len(specs) != nb:
        raise ValueError("gp_posterior_batch: %d kernels for %d problems" % (len(specs), nb))
    if nmax > BATCH_NMAX:
        raise ValueError("gp_posterior_batch: problems of order up to %d, got %d (use gp_solve)" % (BATCH_NMAX, nmax))
    Xqs = list(Xqs)
    if len(Xqs) != nb:
        raise ValueError("gp_posterior_batch: %d problems but %d arrays of query points" % (nb, len(Xqs)))
    Xq2 = [as_xy(X) for X in Xqs]
    ms = np.array([X.shape[0] for X in Xq2], dtype=np.int64)
    if np.any(ms < 1):
        raise ValueError("gp_posterior_batch: every problem needs at least one query point")
    mmax = int(ms.max())
    if mmax > POSTERIOR_MMAX[what]:
        raise ValueError("gp_posterior_batch: what=%r takes up to %d query points per problem, got %d"
                         % (what, POSTERIOR_MMAX[what], mmax))
    Xqb = np.zeros((nb, mmax, 2))
    for b in range(nb):
        Xqb[b, :ms[b]] = Xq2[b]
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    fn, name, ks, _keep = _batch_kernels(lib, "tgp_gp_posterior_batch", specs)
    alpha = np.empty((nb, nmax)) if want_alpha else None
    unc = np.empty((nb, mmax, mmax) if what == "cov" else (nb, mmax))
    logdet = np.empty(nb)
    chi2 = np.empty(nb)
    info = np.zeros(nb, dtype=np.int32)
    rc = fn(ctx, nb, ks, ptr(ns), nmax, ptr(Xb), ptr(yb), ptr(eb), ptr(ms), mmax, ptr(Xqb), 2 if what == "cov" else 1, ptr(alpha),
            ptr(unc), ptr(logdet), ptr(chi2), ptr(info))
    check(ctx, rc, name)
    alphas = [alpha[b, :int(ns[b])].copy() for b in range(nb)] if want_alpha else None
    # a problem with mmax points gets a view of the batch's array (no second copy of up to 128 MiB per covariance), the
    # others a compact copy of their block
    if what == "cov":
        uncs = [unc[b] if ms[b] == mmax else unc[b, :ms[b], :ms[b]].copy() for b in range(nb)]
    else:
        uncs = [unc[b] if ms[b] == mmax else unc[b, :ms[b]].copy() for b in range(nb)]
    return alphas, uncs, logdet, chi2, info.astype(np.int64)


def gp_solve_dense(K, y, y_err=None, keep=False, want_alpha=True, ctx=None):
    """gp_solve for a kernel matrix evaluated by the caller (any scikit-learn kernel tree): K (n, n), lower triangle
    read; y_err^2 is added to the diagonal on the device (tgp_gp_solve_dense)."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    K = f64(K)
    n = K.shape[0]
    if K.shape != (n, n):
        raise ValueError("K must be square")
    y = f64(y)
    e = None if y_err is None else f64(y_err)
    alpha = np.empty(n) if want_alpha else None
    logdet, ydota = C.c_double(0.0), C.c_double(0.0)
    h = C.c_void_p()
    rc = lib.tgp_gp_solve_dense(ctx, ptr(K), n, ptr(y), ptr(e), ptr(alpha), C.byref(logdet), C.byref(ydota),
                                C.byref(h) if keep else None)
    check(ctx, rc, "tgp_gp_solve_dense")
    if rc > 0:
        raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % rc)
    return alpha, logdet.value, ydota.value, (Factor(ctx, h, n) if keep else None)


def factor_solve(factor, B, ctx=None):
    """(K + D)^-1 applied to every row of B (nrhs, n) with a kept factor (tgp_factor_solve): the factor is read once per
    sweep for up to 4 right-hand sides."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    B = np.atleast_2d(f64(B))
    if B.shape[1] != factor.n:
        raise ValueError("B must be (nrhs, %d)" % factor.n)
    out = np.empty_like(B)
    check(ctx, lib.tgp_factor_solve(ctx, factor._h, ptr(B), B.shape[0], ptr(out)), "tgp_factor_solve")
    return out


def factor_lmul(factor, Z, ctx=None):
    """L applied to every row of Z (nrhs, n) with a kept factor, L the lower Cholesky factor of K + D (tgp_factor_lmul):
    rows of standard normals become realisations of N(0, K + D).  The factor is read once per group of 8 rows; row v of
    the result does not depend on the other rows of Z."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    Z = np.atleast_2d(f64(Z))
    if Z.ndim != 2 or Z.shape[1] != factor.n:
        raise ValueError("Z must be (nrhs, %d)" % factor.n)
    out = np.empty_like(Z)
    check(ctx, lib.tgp_factor_lmul(ctx, factor._h, ptr(Z), Z.shape[0], ptr(out)), "tgp_factor_lmul")
    return out


def factor_inv_diag(factor, ctx=None):
    """diag((K + D)^-1) (n,) from a kept factor (tgp_factor_inv_diag): |L^-1 e_i|^2 for every i, identity rows substituted on
    the device in chunks (~n^3 / 3 flops, no n x n buffer on either side).  With alpha = (K + D)^-1 r it gives every point's
    leave-one-out prediction (treegp_amd.loo.loo_quantities)."""
    if factor is None or not factor._h:
        raise ValueError("factor_inv_diag needs a kept factor (gp_solve(..., keep=True)) that has not been freed")
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    d = np.empty(factor.n)
    check(ctx, lib.tgp_factor_inv_diag(ctx, factor._h, ptr(d)), "tgp_factor_inv_diag")
    return d


INVBLOCK_GMAX = 4096   # tgp_factor_inv_blocks: most rows of one group (TGP_INVBLOCK_GMAX)


def factor_inv_blocks(factor, starts, ctx=None):
    """The diagonal blocks of (K + D)^-1 from a kept factor (tgp_factor_inv_blocks): group g is rows starts[g] .. starts[g+1] - 1,
    starts (ngroups + 1,) integers.  Returns a list of (g, g) arrays, each symmetric bit for bit.  With alpha = (K + D)^-1 r they
    give every group's prediction from the points outside it (treegp_amd.loo.lgo_quantities).  The factor and the shape of
    ``starts`` are checked here (ValueError); its values -- increasing from 0 to n, no group above 4096 rows -- by the library
    before anything runs on the device (TgpError naming the entry)."""
    if factor is None or not factor._h:
        raise ValueError("factor_inv_blocks needs a kept factor (gp_solve(..., keep=True)) that has not been freed")
    s = np.asarray(starts)
    if s.ndim != 1 or s.shape[0] < 2 or s.dtype.kind not in "iu":
        raise ValueError("factor_inv_blocks: starts must be a 1-D integer array of ngroups + 1 >= 2 entries, got %s %r"
                         % (s.dtype, s.shape))
    s = np.ascontiguousarray(s, dtype=np.int64)
    sizes = np.diff(s)
    # values the library will refuse get no buffer sized by them
    valid = s[0] == 0 and s[-1] == factor.n and np.all(sizes > 0) and np.all(sizes <= INVBLOCK_GMAX)
    flat = np.empty(int(np.sum(sizes * sizes)) if valid else 1)
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    check(ctx, lib.tgp_factor_inv_blocks(ctx, factor._h, ptr(s), len(s) - 1, ptr(flat)), "tgp_factor_inv_blocks")
    if not valid:
        raise ValueError("factor_inv_blocks: the library accepted starts that this wrapper holds invalid")
    offs = np.concatenate([[0], np.cumsum(sizes * sizes)])
    return [flat[offs[g]:offs[g + 1]].reshape(int(sizes[g]), int(sizes[g])) for g in range(len(sizes))]


def gp_predict_cov_dense(factor, HT, Kss, ctx=None):
    """Kss - HT (K + D)^-1 HT^T for caller-evaluated HT = kernel(X2, Y=X1) (m, n) and Kss = kernel(X2) (m, m)."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    HT, Kss = f64(HT), f64(Kss)
    m = HT.shape[0]
    if HT.shape != (m, factor.n) or Kss.shape != (m, m):
        raise ValueError("HT must be (m, n) and Kss (m, m)")
    cov = np.empty((m, m))
    check(ctx, lib.tgp_gp_predict_cov_dense(ctx, factor._h, ptr(HT), ptr(Kss), m, ptr(cov)), "tgp_gp_predict_cov_dense")
    return cov


def gp_predict_var_dense(factor, HT, kss, ctx=None):
    """diag(Kss - HT (K + D)^-1 HT^T) for caller-evaluated HT = kernel(X2, Y=X1) (m, n) and kss = kernel.diag(X2) (m),
    without forming the (m, m) covariance (tgp_gp_predict_var_dense)."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    HT, kss = f64(HT), f64(kss)
    m = HT.shape[0]
    if HT.shape != (m, factor.n) or kss.shape != (m,):
        raise ValueError("HT must be (m, n) and kss (m,)")
    var = np.empty(m)
    check(ctx, lib.tgp_gp_predict_var_dense(ctx, factor._h, ptr(HT), ptr(kss), m, ptr(var)), "tgp_gp_predict_var_dense")
    return var


class ResidentProblem(object):
    """X, y, y_err of one GP problem kept on the device (``tgp_dev_alloc`` / ``tgp_h2d``) for a series of solves
    that differ only in the kernel -- the likelihood evaluations of a maximum-likelihood fit.  Uploading the three
    arrays costs ~90 us per call at the host boundary, as much as the whole solve at N = 256.  The buffers are plain
    device memory: any context of the same device may use them.  ``close()`` frees them."""

    def __init__(self, X, y, y_err=None, ctx=None):
        self._ctx = ctx or _lib.get_ctx()
        self._lib = _lib.load_library()
        X2 = as_xy(X)
        self.n = X2.shape[0]
        self._bufs = []
        self.d_X = self._upload(X2)
        self.d_y = self._upload(f64(y))
        self.d_e = None if y_err is None else self._upload(f64(y_err))

    def _upload(self, a):
        d = C.c_void_p()
        check(self._ctx, self._lib.tgp_dev_alloc(self._ctx, a.nbytes, C.byref(d)), "tgp_dev_alloc")
        self._bufs.append(d)
        check(self._ctx, self._lib.tgp_h2d(self._ctx, d, ptr(a), a.nbytes), "tgp_h2d")
        return d

    def close(self):
        for d in self._bufs:
            self._lib.tgp_dev_free(self._ctx, d)
        self._bufs = []

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


def gp_solve_resident(spec, problem, ctx=None):
    """(logdet, y.K^-1.y) for a ResidentProblem: ``tgp_d_gp_solve`` without alpha, nothing but the kernel parameters
    crosses the host boundary.  Raises numpy.linalg.LinAlgError like gp_solve."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    logdet, ydota = C.c_double(0.0), C.c_double(0.0)
    rc = lib.tgp_d_gp_solve(ctx, C.byref(spec.to_c()), problem.d_X, problem.n, problem.d_y, problem.d_e, None,
                            C.byref(logdet), C.byref(ydota), None)
    check(ctx, rc, "tgp_d_gp_solve")
    if rc > 0:
        raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % rc)
    return logdet.value, ydota.value


def gp_solve_grad_resident(spec, problem, ctx=None):
    """(logdet, y.K^-1.y, d logL / d (log amp, a, b, c)) for a ResidentProblem in one call (``tgp_d_gp_solve_grad``):
    one evaluation of a gradient-driven maximum-likelihood fit.  Gaussian kernels only."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    logdet, ydota = C.c_double(0.0), C.c_double(0.0)
    grad = np.empty(4)
    rc = lib.tgp_d_gp_solve_grad(ctx, C.byref(spec.to_c()), problem.d_X, problem.n, problem.d_y, problem.d_e,
                                 C.byref(logdet), C.byref(ydota), ptr(grad))
    check(ctx, rc, "tgp_d_gp_solve_grad")
    if rc > 0:
        raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % rc)
    return logdet.value, ydota.value, grad


def gp_solve_grad_resident_any(spec, problem, ctx=None):
    """``gp_solve_grad_resident`` for all four kernel kinds (``tgp_d_gp_solve_grad_any``, seam S2h)."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    logdet, ydota = C.c_double(0.0), C.c_double(0.0)
    grad = np.empty(4)
    rc = lib.tgp_d_gp_solve_grad_any(ctx, C.byref(spec.to_c()), problem.d_X, problem.n, problem.d_y, problem.d_e,
                                     C.byref(logdet), C.byref(ydota), ptr(grad))
    check(ctx, rc, "tgp_d_gp_solve_grad_any")
    if rc > 0:
        raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % rc)
    return logdet.value, ydota.value, grad


def gp_predict(spec, X, alpha, Xs, ctx=None):
    """ys = k(Xs, X) @ alpha without materialising the cross kernel (gp_interp.py:177,183)."""
    eng = None if isinstance(spec, (KernelSumSpec, KernelSpec3)) else _dist_engine(len(X), ctx)
    if eng is not None:
        return eng.gp_predict(spec, X, alpha, Xs)
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    X2, Xs2 = _coords(spec, X), _coords(spec, Xs)
    alpha = f64(alpha)
    ys = np.empty(Xs2.shape[0])
    fn, name = _entry(lib, "tgp_gp_predict", spec)
    rc = fn(ctx, C.byref(spec.to_c()), ptr(X2), X2.shape[0], ptr(alpha), ptr(Xs2), Xs2.shape[0], ptr(ys))
    check(ctx, rc, name)
    return ys


def gp_predict_grad(spec, X, alpha, Xs, ctx=None):
    """(m, 2): the derivative with respect to the query point of what ``gp_predict`` returns, d/dXs [k(Xs, X) @ alpha], from the
    kernel's analytic derivative (tgp_gp_predict_grad, seam S3g of include/tgp.h).  A training point at zero distance from a
    query contributes no slope; 1-D coordinates give a zero second column.  Runs on this process's GPU whatever the multi-GPU
    settings: the sum is one pass over the pairs, as ``gp_predict``'s."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    X2, Xs2 = _coords(spec, X), _coords(spec, Xs)
    alpha = f64(alpha)
    gs = np.empty((Xs2.shape[0], Xs2.shape[1]))            # (m, 2); (m, 3) for a KernelSpec3
    fn, name = _entry(lib, "tgp_gp_predict_grad", spec)
    rc = fn(ctx, C.byref(spec.to_c()), ptr(X2), X2.shape[0], ptr(alpha), ptr(Xs2), Xs2.shape[0], ptr(gs))
    check(ctx, rc, name)
    return gs


LOCAL_KMAX = 128


def gp_predict_local(spec, X, y, y_err, Xs, k=64, return_var=False, return_neighbors=False, ctx=None):
    """Local kriging (tgp_gp_predict_local, seam S3l of include/tgp.h): each query is conditioned on its ``k`` nearest training
    points alone -- nearest in the kernel's own metric, ties to the lower row -- and gets the GP mean ``ys`` (and, for
    ``return_var``, the variance ``amp - v.v``, not clamped) of that small problem.  No n x n matrix exists; the cost is linear
    in the number of queries.  ``y`` is the residual the GP acts on, ``y_err`` its errors or None.  ``k`` in 1 .. 128 is
    clipped to the number of training points (the result is then the exact GP's).  Returns ``ys``, then ``var`` if asked for,
    then for ``return_neighbors`` the (m, min(k, n)) int32 rows of each query's neighbours, nearest first.  A query whose local
    matrix is not positive definite raises numpy.linalg.LinAlgError naming the first one; the error carries ``info``
    (per query: 0, or the order of the failing minor) and the outputs (NaN for failed queries) as ``.info`` and ``.results``.
    ``spec`` is a 2-D ``KernelSpec``: a ``KernelSumSpec`` or a ``KernelSpec3`` raises NotImplementedError.  Runs on this
    process's GPU whatever the multi-GPU settings."""
    if isinstance(spec, KernelSumSpec):
        raise NotImplementedError("gp_predict_local takes one parametrised kernel: a sum of kernels (KernelSumSpec) has no single "
                                  "metric to rank neighbours by")
    if isinstance(spec, KernelSpec3):
        raise NotImplementedError("gp_predict_local takes 2-D coordinates: the bucket grid has no 3-D form (KernelSpec3)")
    if not isinstance(spec, KernelSpec):
        raise ValueError("gp_predict_local: spec must be a KernelSpec, got %r" % (type(spec).__name__,))
    if int(k) != k or not 1 <= int(k) <= LOCAL_KMAX:
        raise ValueError("gp_predict_local: k must be an integer in 1 .. %d, got %r" % (LOCAL_KMAX, k))
    X2, Xs2 = as_xy(X), as_xy(Xs)
    n, m = X2.shape[0], Xs2.shape[0]
    y = f64(y).ravel()
    if n < 1 or y.shape[0] != n:
        raise ValueError("gp_predict_local: X holds %d points and y %d values" % (n, y.shape[0]))
    e = None
    if y_err is not None:
        e = f64(y_err).ravel()
        if e.shape[0] != n:
            raise ValueError("gp_predict_local: X holds %d points and y_err %d values" % (n, e.shape[0]))
    kn = min(int(k), n)
    ys, var = np.empty(m), (np.empty(m) if return_var else None)
    nbr = np.empty((m, kn), dtype=np.int32) if return_neighbors else None
    info = np.zeros(m, dtype=np.int32)
    if m > 0:
        ctx = ctx or _lib.get_ctx()
        lib = _lib.load_library()
        rc = lib.tgp_gp_predict_local(ctx, C.byref(spec.to_c()), ptr(X2), n, ptr(y), ptr(e), ptr(Xs2), m, kn, ptr(ys), ptr(var),
                                      ptr(nbr), ptr(info))
        check(ctx, rc, "tgp_gp_predict_local")
    out = (ys,) + ((var,) if return_var else ()) + ((nbr,) if return_neighbors else ())
    bad = np.flatnonzero(info > 0)
    if len(bad):
        err = np.linalg.LinAlgError("gp_predict_local: query %d: the %d-th leading minor of its local matrix (k = %d) is not "
                                    "positive definite (%d of %d queries failed)" % (bad[0], info[bad[0]], kn, len(bad), m))
        err.info, err.results = info, out
        raise err
    return out if len(out) > 1 else ys


LOCAL_MODES = {"loo": 0, "prior": 1}       # TGP_LOCAL_LOO, TGP_LOCAL_PRIOR


def vecchia_rank(n, seed=0):
    """The rank array (int32, a permutation of 0 .. n - 1) of the ordering ``np.random.default_rng(seed).permutation(n)``: row
    ``permutation[j]`` has rank j.  The default ordering of the Vecchia likelihood (``gp_local_cond(mode="prior")``): the literature
    on Vecchia orderings reports a random ordering close to max-min ordering and clearly better than sorting by a coordinate."""
    order = np.random.default_rng(seed).permutation(int(n))
    rank = np.empty(int(n), dtype=np.int32)
    rank[order] = np.arange(int(n), dtype=np.int32)
    return rank


def gp_local_cond(spec, X, y, y_err, k=64, mode="loo", rank=None, neighbors=None, return_neighbors=False, ctx=None):
    """Local conditionals (tgp_gp_local_cond, seam S3v of include/tgp.h): every TRAINING row i gets the mean ``mu[i]`` and the latent
    variance ``var[i]`` (``amp - v.v``, not clamped) of the GP conditioned on its ``k`` nearest eligible rows alone, by the search and
    the solve of ``gp_predict_local``.  ``mode="loo"``: every other row is eligible (local leave-one-out).  ``mode="prior"``: the
    rows of lower ``rank`` (an int permutation of 0 .. n - 1, required; ``vecchia_rank`` makes one), and
    ``-0.5 sums[1] - 0.5 sums[0] - n/2 log 2 pi`` is Vecchia's approximation of the log-likelihood, the exact one when ``k`` reaches
    all predecessors.  ``neighbors``: (n, k) int32 lists with -1 padding at the end only, used instead of a search (``mode`` and
    ``rank`` are then not consulted): a fit finds them once and keeps them, so that its objective is smooth in theta.
    ``y`` is the residual the GP acts on, ``y_err`` its errors or None.  ``k`` in 1 .. 128 is not clipped: lists are padded with -1.
    Returns ``(mu, var, sums)`` -- sums = [sum log s2_i, sum (y_i - mu_i)^2 / s2_i over the rows that did not fail, number of failed
    rows], s2_i = var_i + y_err_i^2, reduced on the device in a fixed order -- then for ``return_neighbors`` ``(nbr, cnt)``: the
    (n, k) lists, nearest first, and their lengths.  A row whose local matrix is not positive definite raises
    numpy.linalg.LinAlgError naming the first one; the error carries ``.info`` and ``.results`` (the outputs, NaN for failed rows).
    ``spec`` is a 2-D ``KernelSpec``: a ``KernelSumSpec`` or a ``KernelSpec3`` raises NotImplementedError.  Runs on this process's
    GPU whatever the multi-GPU settings."""
    if isinstance(spec, KernelSumSpec):
        raise NotImplementedError("gp_local_cond takes one parametrised kernel: a sum of kernels (KernelSumSpec) has no single "
                                  "metric to rank neighbours by")
    if isinstance(spec, KernelSpec3):
        raise NotImplementedError("gp_local_cond takes 2-D coordinates: the bucket grid has no 3-D form (KernelSpec3)")
    if not isinstance(spec, KernelSpec):
        raise ValueError("gp_local_cond: spec must be a KernelSpec, got %r" % (type(spec).__name__,))
    if int(k) != k or not 1 <= int(k) <= LOCAL_KMAX:
        raise ValueError("gp_local_cond: k must be an integer in 1 .. %d, got %r" % (LOCAL_KMAX, k))
    if mode not in LOCAL_MODES:
        raise ValueError("gp_local_cond: mode must be 'loo' or 'prior', got %r" % (mode,))
    X2 = as_xy(X)
    n, kn = X2.shape[0], int(k)
    y = f64(y).ravel()
    if n < 1 or y.shape[0] != n:
        raise ValueError("gp_local_cond: X holds %d points and y %d values" % (n, y.shape[0]))
    e = None
    if y_err is not None:
        e = f64(y_err).ravel()
        if e.shape[0] != n:
            raise ValueError("gp_local_cond: X holds %d points and y_err %d values" % (n, e.shape[0]))
    nbr_in = r32 = None
    if neighbors is not None:
        nbr_in = np.ascontiguousarray(neighbors, dtype=np.int32)
        if nbr_in.shape != (n, kn):
            raise ValueError("gp_local_cond: neighbors must be (%d, %d), got %r" % (n, kn, nbr_in.shape))
    elif mode == "prior":
        if rank is None:
            raise ValueError("gp_local_cond: mode='prior' needs rank, a permutation of 0 .. n - 1 (ops.vecchia_rank)")
        r32 = np.ascontiguousarray(rank, dtype=np.int32).ravel()
        if r32.shape[0] != n:
            raise ValueError("gp_local_cond: X holds %d points and rank %d values" % (n, r32.shape[0]))
    mu, var, sums = np.empty(n), np.empty(n), np.zeros(3)
    nbr = np.empty((n, kn), dtype=np.int32) if return_neighbors else None
    cnt = np.empty(n, dtype=np.int32) if return_neighbors else None
    info = np.zeros(n, dtype=np.int32)
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    rc = lib.tgp_gp_local_cond(ctx, C.byref(spec.to_c()), ptr(X2), n, ptr(y), ptr(e), LOCAL_MODES[mode], ptr(r32), kn, ptr(nbr_in),
                               ptr(mu), ptr(var), ptr(nbr), ptr(cnt), ptr(info), ptr(sums))
    check(ctx, rc, "tgp_gp_local_cond")
    out = (mu, var, sums) + ((nbr, cnt) if return_neighbors else ())
    bad = np.flatnonzero(info > 0)
    if len(bad):
        err = np.linalg.LinAlgError("gp_local_cond: row %d: the %d-th leading minor of its local matrix (k = %d) is not positive "
                                    "definite (%d of %d rows failed)" % (bad[0], info[bad[0]], kn, len(bad), n))
        err.info, err.results = info, out
        raise err
    return out


def gp_predict_cov(spec, factor, X, Xs, ctx=None):
    """Posterior covariance k(Xs,Xs) - HT K^-1 HT^T (gp_interp.py:184-192) from a kept factor."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    X2, Xs2 = _coords(spec, X), _coords(spec, Xs)
    m = Xs2.shape[0]
    cov = np.empty((m, m))
    fn, name = _entry(lib, "tgp_gp_predict_cov", spec)
    rc = fn(ctx, factor._h, C.byref(spec.to_c()), ptr(X2), X2.shape[0], ptr(Xs2), m, ptr(cov))
    check(ctx, rc, name)
    return cov


def gp_predict_var(spec, factor, X, Xs, ctx=None):
    """Posterior variance diag(k(Xs,Xs) - HT K^-1 HT^T) from a kept factor, for any number of query points: the (m, m)
    covariance is never formed (tgp_gp_predict_var; the reference's callers take np.diag of gp_interp.py:184-192)."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    X2, Xs2 = _coords(spec, X), _coords(spec, Xs)
    m = Xs2.shape[0]
    var = np.empty(m)
    fn, name = _entry(lib, "tgp_gp_predict_var", spec)
    rc = fn(ctx, factor._h, C.byref(spec.to_c()), ptr(X2), X2.shape[0], ptr(Xs2), m, ptr(var))
    check(ctx, rc, name)
    return var


def gp_loglik_grad(spec, factor, X, alpha, ctx=None):
    """1/2 sum_ij (alpha_i alpha_j - [K^-1]_ij) dK_ij/dp for p = (log amp, a, b, c), from the factor and alpha of one
    ``gp_solve(..., keep=True)`` (include/tgp.h, seam S2d).  Gaussian kernels only; ``kernels.spec_jacobian`` maps the four
    numbers to d logL / d theta."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    X2 = as_xy(X)
    alpha = f64(alpha)
    grad = np.empty(4)
    rc = lib.tgp_gp_loglik_grad(ctx, factor._h, C.byref(spec.to_c()), ptr(X2), X2.shape[0], ptr(alpha), ptr(grad))
    check(ctx, rc, "tgp_gp_loglik_grad")
    return grad


def gp_loglik_grad_any(spec, factor, X, alpha, ctx=None):
    """``gp_loglik_grad`` for all four kernel kinds (``tgp_gp_loglik_grad_any``, seam S2h): for the von Karman kinds the sums
    with the profile f in slot 0 and w = -f'/u in slots 1 .. 3; ``kernels.spec_jacobian(kernel, von_karman=True)`` maps the four
    numbers to d logL / d theta.  The same bits as ``gp_loglik_grad`` for the Gaussian kinds."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    X2 = as_xy(X)
    alpha = f64(alpha)
    grad = np.empty(4)
    rc = lib.tgp_gp_loglik_grad_any(ctx, factor._h, C.byref(spec.to_c()), ptr(X2), X2.shape[0], ptr(alpha), ptr(grad))
    check(ctx, rc, "tgp_gp_loglik_grad_any")
    return grad


def gp_loglik_grad_sum(sumspec, factor, X, alpha, ctx=None):
    """(nterms, 4): row t is ``gp_loglik_grad_any`` of term t -- d log L / d (log amp_t, a_t, b_t, c_t) -- from the factor and
    alpha of one ``gp_solve(sumspec, ..., keep=True)`` (``tgp_gp_loglik_grad_sum``, seam S2s): K^-1 is formed once, the pair
    pass runs once per term.  ``kernels.sum_spec_jacobian`` maps the flattened numbers to d logL / d theta."""
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    X2 = as_xy(X)
    alpha = f64(alpha)
    grad = np.empty((len(sumspec.terms), 4))
    rc = lib.tgp_gp_loglik_grad_sum(ctx, factor._h, C.byref(sumspec.to_c()), ptr(X2), X2.shape[0], ptr(alpha), ptr(grad))
    check(ctx, rc, "tgp_gp_loglik_grad_sum")
    return grad


def gp_fisher(spec, factor, X, ctx=None):
    """Fisher information of the Gaussian likelihood in the device's own parameters, (4 T, 4 T) for the T terms of ``spec`` (a
    ``KernelSpec``: T = 1; a ``KernelSumSpec``): F[r][s] = 1/2 tr(C D_r C D_s) with C = (K + diag(y_err^2))^-1 and
    D_{4 t + k} = dK / d(log amp_t, a_t, b_t, c_t)[k], from the factor of one ``gp_solve(spec, ..., keep=True)`` of the same X,
    kernel and y_err (``tgp_gp_fisher`` / ``tgp_gp_fisher_sum``, seam S2j).  ``kernels.fisher_theta`` maps it to scikit-learn's
    theta.  Bitwise symmetric; the factor is only read.  There is no 3-D derivative on the device: ValueError for a
    ``KernelSpec3``, and for a factor that was freed.  Runs on this process's GPU whatever the multi-GPU settings."""
    if isinstance(spec, KernelSpec3):
        raise ValueError("gp_fisher: the device has no derivative matrices for 3-D coordinates (KernelSpec3)")
    if not isinstance(spec, (KernelSpec, KernelSumSpec)):
        raise ValueError("gp_fisher: spec must be a KernelSpec or a KernelSumSpec, got %r" % (type(spec).__name__,))
    if factor is None or not getattr(factor, "_h", None):
        raise ValueError("gp_fisher: the factor was freed (keep one with gp_solve(..., keep=True))")
    ctx = ctx or factor._ctx
    lib = _lib.load_library()
    X2 = as_xy(X)
    nterms = len(spec.terms) if isinstance(spec, KernelSumSpec) else 1
    F = np.empty((4 * nterms, 4 * nterms))
    fn, name = _entry(lib, "tgp_gp_fisher", spec)
    rc = fn(ctx, factor._h, C.byref(spec.to_c()), ptr(X2), X2.shape[0], ptr(F))
    check(ctx, rc, name)
    return F


# ---- pair binning across ranks: i-tiles / bootstrap resamples dealt to the ranks ------
_pair = threading.local()                  # per thread: the tests run virtual ranks as threads


def _pair_comm():
    return getattr(_pair, "comm", None)


def set_pair_comm(comm):
    """Shard every following kk_twod / kk_log / kk_twod_bootstrap call over the ranks of ``comm``
    (an object with rank, size, all_reduce_sum(tensor), e.g. treegp_amd.dist.TorchComm); None
    switches back to single-GPU.  Every rank must make the same calls with the same data."""
    _pair.comm = comm if (comm is not None and comm.size > 1) else None


def kk_partial(bin_type, x, y, k, w, min_sep, max_sep, nbins, part, nparts, ctx=None):
    """Raw accumulators (3, nbins^2) [TwoD, bin_type 0] or (5, nbins) [Log, 1] of one shard."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    x, y, k = f64(x), f64(y), f64(k)
    w = None if w is None else f64(w)
    acc = np.zeros((3, nbins * nbins) if bin_type == 0 else (5, nbins))
    rc = lib.tgp_kk_partial(ctx, int(bin_type), ptr(x), ptr(y), ptr(k), ptr(w), len(x), float(min_sep),
                            float(max_sep), int(nbins), int(part), int(nparts), ptr(acc))
    check(ctx, rc, "tgp_kk_partial")
    return acc


def _kk_sharded(bin_type, x, y, k, w, min_sep, max_sep, nbins, ctx, comm):
    import torch
    acc = kk_partial(bin_type, x, y, k, w, min_sep, max_sep, nbins, comm.rank, comm.size, ctx)
    t = torch.from_numpy(acc)
    dev = getattr(comm, "device", None)
    if dev is not None:
        t = t.to(dev)
    comm.all_reduce_sum(t)                               # <= 5 nbins^2 doubles
    acc = t.cpu().numpy()
    ww = acc[1]
    nz = ww != 0.0
    safe = np.where(nz, ww, 1.0)
    xi = np.where(nz, acc[0] / safe, 0.0)
    if bin_type == 0:
        return xi, ww, acc[2]
    return xi, ww, np.where(nz, acc[2] / safe, 0.0), np.where(nz, acc[3] / safe, 0.0), acc[4]


def kk_twod(x, y, k, w, min_sep, max_sep, nbins, ctx=None):
    if _pair_comm() is not None:
        return _kk_sharded(0, x, y, k, w, min_sep, max_sep, nbins, ctx, _pair_comm())
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    x, y, k = f64(x), f64(y), f64(k)
    w = None if w is None else f64(w)
    nb2 = nbins * nbins
    xi, wt, npairs = np.empty(nb2), np.empty(nb2), np.empty(nb2)
    rc = lib.tgp_kk_twod(ctx, ptr(x), ptr(y), ptr(k), ptr(w), len(x), float(min_sep), float(max_sep), int(nbins),
                         ptr(xi), ptr(wt), ptr(npairs))
    check(ctx, rc, "tgp_kk_twod")
    return xi, wt, npairs


def kk_log(x, y, k, w, min_sep, max_sep, nbins, ctx=None):
    if _pair_comm() is not None:
        return _kk_sharded(1, x, y, k, w, min_sep, max_sep, nbins, ctx, _pair_comm())
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    x, y, k = f64(x), f64(y), f64(k)
    w = None if w is None else f64(w)
    out = [np.empty(nbins) for _ in range(5)]
    rc = lib.tgp_kk_log(ctx, ptr(x), ptr(y), ptr(k), ptr(w), len(x), float(min_sep), float(max_sep), int(nbins),
                        *[ptr(o) for o in out])
    check(ctx, rc, "tgp_kk_log")
    return tuple(out)       # xi, weight, meanr, meanlogr, npairs


def kk_twod_bootstrap(x, y, yv, y_err, idx, min_sep, max_sep, nbins, ctx=None):
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    x, y, yv = f64(x), f64(y), f64(yv)
    e = None if y_err is None else f64(y_err)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    n_boot, n = idx.shape
    assert n == len(x)
    comm = _pair_comm()
    if comm is not None:
        # whole resamples per rank (rows rank, rank + size, ...), then one sum puts the rows together
        import torch
        mine = idx[comm.rank::comm.size]
        full = np.zeros((n_boot, nbins * nbins))
        if len(mine):
            full[comm.rank::comm.size] = _kk_twod_bootstrap_local(ctx, lib, x, y, yv, e, mine, min_sep, max_sep, nbins)
        t = torch.from_numpy(full)
        dev = getattr(comm, "device", None)
        if dev is not None:
            t = t.to(dev)
        comm.all_reduce_sum(t)
        return t.cpu().numpy()
    return _kk_twod_bootstrap_local(ctx, lib, x, y, yv, e, idx, min_sep, max_sep, nbins)


def _kk_twod_bootstrap_local(ctx, lib, x, y, yv, e, idx, min_sep, max_sep, nbins):
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    n_boot, n = idx.shape
    out = np.empty((n_boot, nbins * nbins))
    rc = lib.tgp_kk_twod_bootstrap(ctx, ptr(x), ptr(y), ptr(yv), ptr(e), n, ptr(idx), n_boot, float(min_sep),
                                   float(max_sep), int(nbins), ptr(out))
    check(ctx, rc, "tgp_kk_twod_bootstrap")
    return out


def vcorr_sums(x, y, dx, dy, edges, ctx=None):
    """Raw per-bin sums (7, nbins) of the vector pair correlation over all pairs (utils.py:36-72)."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    x, y, dx, dy, edges = f64(x), f64(y), f64(dx), f64(dy), f64(edges)
    nbins = len(edges) - 1
    acc = np.zeros((7, nbins))
    rc = lib.tgp_vcorr(ctx, ptr(x), ptr(y), ptr(dx), ptr(dy), len(x), ptr(edges), nbins, ptr(acc))
    check(ctx, rc, "tgp_vcorr")
    return acc


def knn_mean(X0, y0, X, k=4, ctx=None):
    """Uniform mean of the k nearest table rows for every row of X (gp_interp.py:236-238)."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    X02, X2 = as_xy(X0), as_xy(X)
    y0 = f64(y0)
    out = np.empty(X2.shape[0])
    rc = lib.tgp_knn_mean(ctx, ptr(X02), ptr(y0), X02.shape[0], ptr(X2), X2.shape[0], int(k), ptr(out))
    check(ctx, rc, "tgp_knn_mean")
    return out


_STATS = {"mean": 0, "median": 1, "weighted": 2}


def binned_stat_2d(u, v, values, u_edges, v_edges, statistic="mean", err=None, ctx=None):
    """scipy.stats.binned_statistic_2d(u, v, values, bins=[u_edges, v_edges], statistic) on the GPU
    (meanify.py:76-107).  Returns average, wrms, count, each (len(u_edges)-1, len(v_edges)-1)."""
    ctx = ctx or _lib.get_ctx()
    lib = _lib.load_library()
    u, v, values = f64(u), f64(v), f64(values)
    ue, ve = f64(u_edges), f64(v_edges)
    e = None if err is None else f64(err)
    if statistic not in _STATS:
        raise ValueError("statistic must be one of %s" % sorted(_STATS))
    if statistic == "weighted" and e is None:
        raise ValueError("the weighted statistic needs errors")
    shape = (len(ue) - 1, len(ve) - 1)
    avg, wrms, cnt = np.empty(shape), np.empty(shape), np.empty(shape)
    rc = lib.tgp_binned_stat_2d(ctx, ptr(u), ptr(v), ptr(values), ptr(e), len(u), ptr(ue), len(ue), ptr(ve), len(ve),
                                _STATS[statistic], ptr(avg), ptr(wrms), ptr(cnt))
    check(ctx, rc, "tgp_binned_stat_2d")
    return avg, wrms, cnt


# ---- device-resident tier ---------------------------------------------------------------------
class DeviceBuffer(object):
    def __init__(self, ctx, nbytes):
        self._ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        check(ctx, _lib.load_library().tgp_dev_alloc(ctx, self.nbytes, C.byref(p)), "tgp_dev_alloc")
        self.ptr = p

    @classmethod
    def from_array(cls, ctx, a):
        a = np.ascontiguousarray(a)
        buf = cls(ctx, a.nbytes)
        check(ctx, _lib.load_library().tgp_h2d(ctx, buf.ptr, ptr(a), a.nbytes), "tgp_h2d")
        return buf

    def to_array(self, shape, dtype=np.float64):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(self._ctx, _lib.load_library().tgp_d2h(self._ctx, ptr(out), self.ptr, out.nbytes), "tgp_d2h")
        return out

    def free(self):
        if self.ptr:
            _lib.load_library().tgp_dev_free(self._ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

"""Change of units: every device route must return the same bits, shifted in the exponent, for data rescaled by powers of two.

Almost everything the library does is homogeneous: kernels multiply by amp at the end, the factorisation uses products, FMAs
and reciprocal square roots with Newton steps, the posterior transforms are sqrt, quotients and differences of products.  A
rescaling of the values by 2^p (amp by 4^p), of the data alone by 2^r, or of the coordinates by 2^q (invLam by 4^-q, ell by
2^q) is exact in binary, so each output must be ``np.ldexp(unscaled, shift)`` bit for bit, the shift read from the dimension
table of tests/_units_helpers.py.  No reference is needed; what breaks it is an absolute epsilon, clamp, threshold or jitter, a
seed taken through a narrower type, a constant with a physical dimension.  tests/test_units_host.py asserts on the CPU that
none of the scaled inputs or kernel values comes near the subnormal range, where bit-homogeneity would legitimately end.

The unscaled and the scaled call run in this process on the same context.  Outputs that go through a logarithm (logdet, the
Vecchia and leave-one-out log scores, return_log_likelihood, sum log s2) move by an exact multiple of ln 2 and are held to
``_units_helpers.log_tolerance``.

Pair statistics.  The pair counts of kk_twod and knn_mean are held to equal bits.  xi and the weights of kk_twod and
kk_twod_bootstrap (both paths, TGP_BOOT_LISTS) are sums of fp64 atomics whose order of addition is not fixed: two calls at one
scale already differ in the last bits (measured: 69 of 121 xi pixels, 915 of 968 bootstrap values), so across scales they are
held to the shifted long-double value of the unit-scale catalogue within its shifted error bound (tests/_pair_stat_refs.py,
derived from u = 2^-53; both scale exactly).  kk_log and vcorr_sums bin in ln r, which is not exactly homogeneous, and are held
to equal pair counts per bin on a catalogue whose long-double reference has no pair within 1e-9 bin widths of an edge at any
scale (asserted in test_units_host.py).

Left out, with the reason:
  binned_stat_2d          rounds its bin coordinates with np.around to decimals, the reference's own behaviour: not homogeneous
  the fits                (log_likelihood, local_likelihood, two_pcf optimisers, solve_many, gp_solve_resident and its gradient
                          forms, which exist only to serve them): L-BFGS-B on log theta is not bit-homogeneous and
                          length_scale_bounds=(1e-5, 1e5) is a documented limit in units
  gp_solve_grad_batch,    the Gaussian-only namesakes of gp_solve_grad_batch_any / the sum form of it: the same device bodies
  gp_solve_grad_batch_sum
  kbuild_batch            read by the batched routes, whose outputs are held here
  kk_partial and the      the multi-GPU building blocks need several ranks (tests/test_gpu_dist*.py)
  dist engine
"""
import ctypes as C
import os

import numpy as np
import pytest

import _units_helpers as H
from _units_helpers import Units

pytestmark = pytest.mark.gpu

_lib = ops = None


@pytest.fixture(scope="module", autouse=True)
def _modules():
    global _lib, ops
    from treegp_amd import _lib as L, ops as O_
    _lib, ops = L, O_
    _lib.load_library()
    yield


def ids(units):
    return [repr(u) for u in units]


def spec2(kind, units, **kw):
    return ops.KernelSpec(getattr(_lib, "TGP_" + kind), **units.kw(kw))


def spec_of(name, units, amp=H.AMP):
    """the kernels of the file in the given units: rbf, arbf, vk, avk, sum (AVK + ARBF), arbf3, vk3"""
    if name == "rbf":
        return spec2("RBF", units, amp=amp, a=400.0, b=0.0, c=400.0)
    if name == "arbf":
        return spec2("ARBF", units, amp=amp, **H.INVLAM)
    if name == "vk":
        return spec2("VK", units, amp=amp, ell=H.ELL)
    if name == "avk":
        return spec2("AVK", units, amp=amp, a=120.0, b=30.0, c=150.0)
    if name == "sum":
        return ops.KernelSumSpec([spec2("AVK", units, amp=0.5 * amp, a=120.0, b=30.0, c=150.0),
                                  spec2("ARBF", units, amp=0.75 * amp, **H.INVLAM)])
    if name == "arbf3":
        return ops.KernelSpec3(_lib.TGP_ARBF, **units.kw(dict(amp=amp, m=H.M3)))
    if name == "vk3":
        return ops.KernelSpec3(_lib.TGP_VK, **units.kw(dict(amp=amp, ell=H.ELL)))
    raise ValueError(name)


_BASE = {}


def base(key, fn):
    """the unit-scale outputs of a route, computed once per module run and left unchanged"""
    if key not in _BASE:
        _BASE[key] = fn(H.UNIT)
    return _BASE[key]


def check(key, fn, units):
    H.assert_homogeneous(fn(units), base(key, fn), units, "%s" % (key,))


# ---- 1: values ------------------------------------------------------------------------------------------------------------

def kbuild_raw(spec, X, yerr):
    """the unpacked (n, n) lower triangle of the packed K build (tgp_d_kbuild_lower / _sum / 3), diagonal with y_err^2"""
    ctx, lib = _lib.get_ctx(), _lib.load_library()
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = len(X)
    Np = lib.tgp_padded_n(n)
    ne = lib.tgp_panel_elems(Np)
    name = "tgp_d_kbuild_lower" + ("_sum" if isinstance(spec, ops.KernelSumSpec) else "3" if isinstance(spec, ops.KernelSpec3)
                                   else "")
    dX = ops.DeviceBuffer.from_array(ctx, X)
    de = ops.DeviceBuffer.from_array(ctx, np.ascontiguousarray(yerr, dtype=np.float64))
    dA = ops.DeviceBuffer.from_array(ctx, np.full(ne, np.nan))
    try:
        _lib.check(ctx, getattr(lib, name)(ctx, C.byref(spec.to_c()), dX.ptr, n, de.ptr, dA.ptr), name)
        K = np.empty((n, n))
        _lib.check(ctx, lib.tgp_d_unpack_lower(ctx, dA.ptr, Np, n, K.ctypes.data_as(C.c_void_p)), "tgp_d_unpack_lower")
    finally:
        for buf in (dX, de, dA):
            buf.free()
    return np.tril(K)


VALUE_KERNELS = ("rbf", "arbf", "vk", "avk", "sum", "arbf3", "vk3")


def run_values(kname, n, units):
    P = H.inputs(n, ndim=3 if kname.endswith("3") else 2).at(units)
    spec = spec_of(kname, units)
    return [("kernel_matrix self", "K", ops.kernel_matrix(spec, P.X)),
            ("kernel_matrix cross", "K", ops.kernel_matrix(spec, P.Xq, P.X)),
            ("kernel_matrix cross m=1", "K", ops.kernel_matrix(spec, P.Xq[:1], P.X)),
            ("packed K build", "K", kbuild_raw(spec, P.X, P.e))]


@pytest.mark.parametrize("units", H.NO_Y, ids=ids(H.NO_Y))
@pytest.mark.parametrize("n", [300, 1025])
@pytest.mark.parametrize("kname", VALUE_KERNELS)
def test_values(kname, n, units):
    """kernel_matrix (self and cross) and the packed K build: Y^2 for all four kinds, a sum and both 3-D kinds"""
    check(("values", kname, n), lambda u: run_values(kname, n, u), units)


# ---- 2: factor and solves -------------------------------------------------------------------------------------------------

def kept_factor(fac):
    """(lower triangle of L over rows < n, inverted diagonal blocks restricted to rows < n) of a kept factor, copied out through
    tgp_factor_device.  The padding rows (identity, or the augmented right-hand side) carry no unit and are left out."""
    ctx, lib = fac._ctx, _lib.load_library()
    dA, dW, Np = C.c_void_p(), C.c_void_p(), C.c_int64()
    _lib.check(ctx, lib.tgp_factor_device(ctx, fac._h, C.byref(dA), C.byref(dW), C.byref(Np)), "tgp_factor_device")
    Np, n = Np.value, fac.n
    ne = lib.tgp_panel_elems(Np)
    A = np.empty(ne)
    _lib.check(ctx, lib.tgp_d2h(ctx, A.ctypes.data_as(C.c_void_p), dA, A.nbytes), "tgp_d2h")
    W = np.empty((Np // 128, 128, 128))
    _lib.check(ctx, lib.tgp_d2h(ctx, W.ctypes.data_as(C.c_void_p), dW, W.nbytes), "tgp_d2h")
    L = np.zeros((n, n))
    for p in range((n + 255) // 256):
        off, m = lib.tgp_panel_off(p, Np), Np - 256 * p
        blk = A[off:off + m * 256].reshape(m, 256)
        r1, c1 = n - 256 * p, min(256, n - 256 * p)
        L[256 * p:, 256 * p:256 * p + c1] = blk[:r1, :c1]
    L = np.tril(L)
    Wn = []
    for j in range((n + 127) // 128):
        k = min(128, n - 128 * j)
        Wn.append(np.tril(W[j, :k, :k]).reshape(-1))
    return L, np.concatenate(Wn)


def run_solve(n, units, kname="arbf"):
    P = H.inputs(n).at(units)
    spec = spec_of(kname, units)
    alpha, logdet, ydota, fac = ops.gp_solve(spec, P.X, P.y, P.e, keep=True)
    try:
        L, W = kept_factor(fac)
        out = [("alpha", "alpha", alpha), ("ydota", "ydota", ydota), ("logdet", None, logdet), ("L", "L", L), ("W", "W", W),
               ("factor_solve", "factor_solve", ops.factor_solve(fac, P.B)),
               ("factor_lmul", "factor_lmul", ops.factor_lmul(fac, P.Z)),
               ("factor_inv_diag", "inv_diag", ops.factor_inv_diag(fac)),
               ("factor_inv_blocks", "inv_blocks",
                np.concatenate([b.reshape(-1) for b in ops.factor_inv_blocks(fac, H.inv_block_starts(n))]))]
        for m in H.QUERY_M:
            out += [("gp_predict_cov[%d]" % m, "cov", ops.gp_predict_cov(spec, fac, P.X, P.Xq[:m])),
                    ("gp_predict_var[%d]" % m, "var", ops.gp_predict_var(spec, fac, P.X, P.Xq[:m]))]
    finally:
        fac.free()
    a2, ld2, yd2, _ = ops.gp_solve(spec, P.X, P.y, P.e)
    out += [("alpha (no keep)", "alpha", a2), ("ydota (no keep)", "ydota", yd2), ("logdet (no keep)", None, ld2)]
    for m in H.QUERY_M:
        out += [("gp_predict[%d]" % m, "predict", ops.gp_predict(spec, P.X, alpha, P.Xq[:m])),
                ("gp_predict_grad[%d]" % m, "predict_grad", ops.gp_predict_grad(spec, P.X, alpha, P.Xq[:m]))]
    return out


def check_logdet(scaled, unscaled, n, units, names=("logdet", "logdet (no keep)")):
    ds, du = {k: v for k, _, v in scaled}, {k: v for k, _, v in unscaled}
    for k in names:
        H.assert_log_shift(ds[k], du[k], n, 2 * units.p, "%s n=%d under %r" % (k, n, units))


@pytest.mark.parametrize("units", H.WITH_Y, ids=ids(H.WITH_Y))
@pytest.mark.parametrize("n", H.DENSE_N)
def test_solve_factor_and_posterior(n, units):
    """gp_solve with and without a kept factor, the packed factor and its inverted blocks, factor_solve (5 right-hand sides),
    factor_lmul, factor_inv_diag, factor_inv_blocks (groups crossing row 1024), gp_predict, gp_predict_grad, gp_predict_cov,
    gp_predict_var.  n = 300: one pair of panels, the augmented-row solve; 2300: mode 2 with a queued bulk step, the big-step
    sweeps and the big covariance substitution, the augmented row; 2304 = Np: no padding row, the separate forward sweep."""
    fn = lambda u: run_solve(n, u)
    got, ref = fn(units), base(("solve", n), fn)
    check_logdet(got, ref, n, units)
    H.assert_homogeneous(got, ref, units, "gp_solve n=%d" % n)


@pytest.mark.parametrize("units", H.NO_Y, ids=ids(H.NO_Y))
@pytest.mark.parametrize("kname", ["vk", "sum", "arbf3"])
def test_solve_other_kernels(kname, units):
    """the same route for a von Karman kernel, a sum and 3-D coordinates, n = 300"""
    def fn(u):
        P = H.inputs(300, ndim=3 if kname.endswith("3") else 2).at(u)
        spec = spec_of(kname, u)
        alpha, logdet, ydota, fac = ops.gp_solve(spec, P.X, P.y, P.e, keep=True)
        try:
            out = [("alpha", "alpha", alpha), ("ydota", "ydota", ydota), ("logdet", None, logdet),
                   ("gp_predict_cov", "cov", ops.gp_predict_cov(spec, fac, P.X, P.Xq)),
                   ("gp_predict_var", "var", ops.gp_predict_var(spec, fac, P.X, P.Xq))]
        finally:
            fac.free()
        return out + [("gp_predict", "predict", ops.gp_predict(spec, P.X, alpha, P.Xq)),
                      ("gp_predict_grad", "predict_grad", ops.gp_predict_grad(spec, P.X, alpha, P.Xq))]
    got, ref = fn(units), base(("solve-other", kname), fn)
    check_logdet(got, ref, 300, units, names=("logdet",))
    H.assert_homogeneous(got, ref, units, "gp_solve %s" % kname)


def host_kernel(P, units, Y=None, X=None):
    """amp exp(-q / 2) on the host in the given units (exactly homogeneous: q is the same number at every scale)"""
    from oracle import gp_oracle as O
    kw = units.kw(dict(amp=H.AMP, **H.INVLAM))
    return O.kernel_matrix("gauss", P.X if X is None else X, Y, **kw)


def run_dense(n, units):
    P = H.inputs(n).at(units)
    K = host_kernel(P, units)
    alpha, logdet, ydota, fac = ops.gp_solve_dense(K, P.y, P.e, keep=True)
    out = [("alpha", "alpha", alpha), ("ydota", "ydota", ydota), ("logdet", None, logdet)]
    try:
        L, W = kept_factor(fac)
        out += [("L", "L", L), ("W", "W", W)]
        for m in H.QUERY_M:
            HT = host_kernel(P, units, Y=P.X, X=P.Xq[:m])
            Kss = host_kernel(P, units, X=P.Xq[:m])
            out += [("gp_predict_cov_dense[%d]" % m, "cov", ops.gp_predict_cov_dense(fac, HT, Kss)),
                    ("gp_predict_var_dense[%d]" % m, "var", ops.gp_predict_var_dense(fac, HT, np.diag(Kss).copy()))]
    finally:
        fac.free()
    return out


@pytest.mark.parametrize("units", H.WITH_Y, ids=ids(H.WITH_Y))
@pytest.mark.parametrize("n", H.DENSE_N)
def test_dense_solve_and_posterior(n, units):
    """gp_solve_dense, gp_predict_cov_dense, gp_predict_var_dense on a caller-evaluated K"""
    fn = lambda u: run_dense(n, u)
    got, ref = fn(units), base(("dense", n), fn)
    check_logdet(got, ref, n, units, names=("logdet",))
    H.assert_homogeneous(got, ref, units, "gp_solve_dense n=%d" % n)


# ---- 4: likelihood gradient and Fisher ------------------------------------------------------------------------------------

G4 = ("grad_logamp", "grad_abc", "grad_abc", "grad_abc")


def run_grad(n, units):
    P = H.inputs(n).at(units)
    out = []
    for kname in ("arbf", "vk", "avk", "sum"):
        spec = spec_of(kname, units)
        alpha, _, _, fac = ops.gp_solve(spec, P.X, P.y, P.e, keep=True)
        try:
            if kname == "arbf":
                g = ops.gp_loglik_grad(spec, fac, P.X, alpha)
                out += [("gp_loglik_grad[%d]" % i, G4[i], g[i]) for i in range(4)]
            if kname == "sum":
                g = ops.gp_loglik_grad_sum(spec, fac, P.X, alpha)
                out += [("gp_loglik_grad_sum[%d,%d]" % (t, i), G4[i], g[t, i]) for t in range(2) for i in range(4)]
            else:
                g = ops.gp_loglik_grad_any(spec, fac, P.X, alpha)
                out += [("gp_loglik_grad_any %s[%d]" % (kname, i), G4[i], g[i]) for i in range(4)]
        finally:
            fac.free()
    return out


@pytest.mark.parametrize("units", H.NO_Y, ids=ids(H.NO_Y))
@pytest.mark.parametrize("n", [300, 2300])
def test_loglik_grad(n, units):
    """gp_loglik_grad, gp_loglik_grad_any (Gaussian, vk, avk), gp_loglik_grad_sum: d / d log amp has no unit, d / d (a, b, c)
    has X^2 (for the isotropic von Karman kind slot 1 is the derivative with respect to a = 1 / ell^2).  Not homogeneous in y
    alone (alpha alpha^T - K^-1), so S_y does not apply."""
    check(("grad", n), lambda u: run_grad(n, u), units)


def run_fisher(units):
    P = H.inputs(H.FISHER_N).at(units)
    out = []
    for kname, nt in (("arbf", 1), ("avk", 1), ("sum", 2)):
        spec = spec_of(kname, units)
        fac = ops.gp_solve(spec, P.X, P.y, P.e, keep=True, want_alpha=False)[3]
        try:
            out.append(("gp_fisher " + kname, H.fisher_shift(units, nt), ops.gp_fisher(spec, fac, P.X)))
        finally:
            fac.free()
    return out


@pytest.mark.parametrize("units", H.NO_Y, ids=ids(H.NO_Y))
def test_fisher(units):
    """gp_fisher for one kernel and a two-term sum: entry (r, s) has the product of the dimensions of d / d theta_r, d / d theta_s"""
    got = run_fisher(units)
    ref = [(k, H.fisher_shift(units, 2 if k.endswith("sum") else 1), v) for k, _, v in base("fisher", run_fisher)]
    failures = []
    for (k, sh, a), (_, _, b) in zip(got, ref):
        rep = H.diff_report(a, b, sh)
        if rep:
            failures.append("%s: %s" % (k, rep))
    assert not failures, "gp_fisher under %r is not bit-homogeneous:\n  %s" % (units, "\n  ".join(failures))


# ---- 5: batched -----------------------------------------------------------------------------------------------------------

BATCH_KERNELS = ("arbf", "vk", "avk", "rbf", "arbf")


def run_batch(units_list):
    Ps = [H.inputs(n, seed=7 + b).at(u) for b, (n, u) in enumerate(zip(H.BATCH_NS, units_list))]
    specs = [spec_of(k, u) for k, u in zip(BATCH_KERNELS, units_list)]
    Xs, ys, es = [p.X for p in Ps], [p.y for p in Ps], [p.e for p in Ps]
    Xq = [p.Xq[:m] for p, m in zip(Ps, H.BATCH_MS)]
    out = [[] for _ in Ps]

    def put(tag, lists, arrays):
        for b in range(len(Ps)):
            for nm, dim, l in lists:
                out[b].append(("%s.%s" % (tag, nm), dim, l[b]))
            for nm, dim, a in arrays:
                if dim == "g4":
                    out[b] += [("%s.g4[%d]" % (tag, i), G4[i], a[b][i]) for i in range(4)]
                else:
                    out[b].append(("%s.%s" % (tag, nm), dim, a[b]))

    al, ld, c2, info = ops.gp_solve_batch(specs, Xs, ys, es)
    put("solve", [("alpha", "alpha", al)], [("logdet", None, ld), ("chi2", "ydota", c2), ("info", "int", info)])
    ld, c2, g4, info = ops.gp_solve_grad_batch_any(specs, Xs, ys, es)
    put("grad", [], [("logdet", None, ld), ("chi2", "ydota", c2), ("g4", "g4", g4), ("info", "int", info)])
    al, dg, ld, c2, info = ops.gp_loo_batch(specs, Xs, ys, es)
    put("loo", [("alpha", "alpha", al), ("invdiag", "inv_diag", dg)],
        [("logdet", None, ld), ("chi2", "ydota", c2), ("info", "int", info)])
    for what in ("var", "cov"):
        al, un, ld, c2, info = ops.gp_posterior_batch(specs, Xs, ys, es, Xq, what=what)
        put(what, [("alpha", "alpha", al), ("unc", what, un)], [("logdet", None, ld), ("chi2", "ydota", c2), ("info", "int", info)])
    return out


BATCH_UNITS = [("S_a per problem", [Units(p=p) for p in H.BATCH_P])] + \
              [(repr(u), [u] * len(H.BATCH_NS)) for u in H.S_Y + H.S_X + (H.COMBINED,)]


@pytest.mark.parametrize("case", BATCH_UNITS, ids=[c[0] for c in BATCH_UNITS])
def test_batched_routes(case):
    """gp_solve_batch, gp_solve_grad_batch_any, gp_loo_batch, gp_posterior_batch (var and cov) on one ragged mixed batch,
    ns = [1, 130, 256, 1000, 1025], under S_a with a different p per problem, S_y, S_x and the combined case"""
    _, units_list = case
    got = run_batch(units_list)
    ref = base("batch", lambda u: run_batch([u] * len(H.BATCH_NS)))
    failures = []
    for b, (g, r, u) in enumerate(zip(got, ref, units_list)):
        if u.r:       # the gradient is not homogeneous in y alone
            g = [(k, None if k.startswith("grad.g4") else d, v) for k, d, v in g]
            r = [(k, None if k.startswith("grad.g4") else d, v) for k, d, v in r]
        dg, dr = {k: v for k, _, v in g}, {k: v for k, _, v in r}
        for tag in ("solve", "grad", "loo", "var", "cov"):
            H.assert_log_shift(dg[tag + ".logdet"], dr[tag + ".logdet"], H.BATCH_NS[b], 2 * u.p, "batch %s.logdet[%d]" % (tag, b))
        try:
            H.assert_homogeneous(g, r, u, "problem %d (n = %d, %s)" % (b, H.BATCH_NS[b], BATCH_KERNELS[b]))
        except AssertionError as exc:
            failures.append(str(exc))
    assert not failures, "\n".join(failures)


# ---- 6: local -------------------------------------------------------------------------------------------------------------

def run_local(kname, k, units):
    P = H.inputs(H.LOCAL_N, seed=2).at(units)
    spec = spec_of(kname, units)
    Xq = P.Xq[:H.LOCAL_M]
    ys, var, nbr = ops.gp_predict_local(spec, P.X, P.y, P.e, Xq, k=k, return_var=True, return_neighbors=True)
    out = [("predict_local mean", "local_mean", ys), ("predict_local var", "local_var", var), ("predict_local nbr", "int", nbr)]
    rank = ops.vecchia_rank(P.n, seed=0)
    for mode in ("loo", "prior"):
        mu, v, sums, nb, cnt = ops.gp_local_cond(spec, P.X, P.y, P.e, k=k, mode=mode, rank=rank if mode == "prior" else None,
                                                 return_neighbors=True)
        out += [("local_cond %s mean" % mode, "local_mean", mu), ("local_cond %s var" % mode, "local_var", v),
                ("local_cond %s sum log s2" % mode, None, sums[0]), ("local_cond %s sum r2/s2" % mode, "chi2_sum", sums[1]),
                ("local_cond %s failed" % mode, "int", int(sums[2])),
                ("local_cond %s nbr" % mode, "int", nb), ("local_cond %s cnt" % mode, "int", cnt)]
    return out


@pytest.mark.parametrize("units", H.WITH_Y, ids=ids(H.WITH_Y))
@pytest.mark.parametrize("k", [32, 128])
@pytest.mark.parametrize("kname", ["arbf", "vk"])
def test_local_routes(kname, k, units):
    """gp_predict_local and gp_local_cond in both modes, N = 3000, M = 257: means Y, variances Y^2, identical neighbour lists,
    counts and info, the sum of r^2 / s^2 without unit, the sum of log s2 moved by n p ln 4"""
    fn = lambda u: run_local(kname, k, u)
    got, ref = fn(units), base(("local", kname, k), fn)
    dg, dr = {kk: v for kk, _, v in got}, {kk: v for kk, _, v in ref}
    for mode in ("loo", "prior"):
        H.assert_log_shift(dg["local_cond %s sum log s2" % mode], dr["local_cond %s sum log s2" % mode], H.LOCAL_N, 2 * units.p,
                           "local_cond %s sum log s2 under %r" % (mode, units))
    H.assert_homogeneous(got, ref, units, "local %s k=%d" % (kname, k))


# ---- 7: pair statistics ---------------------------------------------------------------------------------------------------

PAIR_UNITS = H.S_A + H.S_X + (H.COMBINED,)


def _boot(lists, *args):
    old = os.environ.get("TGP_BOOT_LISTS")
    try:
        if lists:
            os.environ.pop("TGP_BOOT_LISTS", None)
        else:
            os.environ["TGP_BOOT_LISTS"] = "0"
        return ops.kk_twod_bootstrap(*args)
    finally:
        os.environ.pop("TGP_BOOT_LISTS", None)
        if old is not None:
            os.environ["TGP_BOOT_LISTS"] = old


_PAIR_REFS = {}


def pair_refs():
    """long-double values and error bounds of the unit-scale sums (tests/_pair_stat_refs.py), made once"""
    if not _PAIR_REFS:
        import _pair_stat_refs as R
        from oracle import gp_oracle as O
        c, t = H.pair_catalogue(), H.PAIR_TWOD
        for tag, w in (("", None), (" weighted", c["w"])):
            ref = R.ref_kk_twod(c["x"], c["y"], c["k"], w, t["min_sep"], t["max_sep"], t["nbins"])
            bnd = R.kk_bounds(ref, log=False)
            _PAIR_REFS["kk_twod%s xi" % tag] = (ref["xi"], bnd["xi"])
            _PAIR_REFS["kk_twod%s weight" % tag] = (ref["weight"], bnd["weight"])
        idx = O.bootstrap_indices(len(c["x"]), H.PAIR_NBOOT)
        ref = R.ref_kk_bootstrap(c["x"], c["y"], c["k"], c["err"], idx, t["min_sep"], t["max_sep"], t["nbins"], chunk=2)
        for lists in (1, 0):
            _PAIR_REFS["kk_twod_bootstrap lists=%d" % lists] = (ref["xi"], ref["bound"])
    return _PAIR_REFS


def run_pairs(units):
    """(exact, sums): outputs whose bits are fixed, and the sums accumulated with fp64 atomics in no fixed order"""
    from oracle import gp_oracle as O
    c = H.pair_catalogue()
    x, y, k, err = units.x(c["x"]), units.x(c["y"]), units.val(c["k"]), units.val(c["err"])
    t = H.PAIR_TWOD
    mn, mx, nb = units.sep(t["min_sep"]), units.sep(t["max_sep"]), t["nbins"]
    exact, sums = [], []
    for tag, w in (("", None), (" weighted", c["w"])):
        xi, wt, npairs = ops.kk_twod(x, y, k, w, mn, mx, nb)
        sums += [("kk_twod%s xi" % tag, "xi", xi), ("kk_twod%s weight" % tag, "weight", wt)]
        exact.append(("kk_twod%s npairs" % tag, "int", npairs))
    idx = O.bootstrap_indices(len(x), H.PAIR_NBOOT)
    for lists in (1, 0):
        sums.append(("kk_twod_bootstrap lists=%d" % lists, "xi", _boot(lists, x, y, k, err, idx, mn, mx, nb)))
    Xq = units.x(H.inputs(300).Xq)
    for kk in (1, 4, 16):
        exact.append(("knn_mean k=%d" % kk, "knn_mean", ops.knn_mean(np.column_stack([x, y]), k, Xq, kk)))
    lg = H.PAIR_LOG
    res = ops.kk_log(x, y, k, c["w"], units.sep(lg["min_sep"]), units.sep(lg["max_sep"]), lg["nbins"])
    exact.append(("kk_log npairs", "int", res[4]))
    acc = ops.vcorr_sums(x, y, units.val(c["dx"]), units.val(c["dy"]), H.pair_log_edges(units))
    exact.append(("vcorr_sums counts", "int", acc[0]))
    return exact, sums


def check_pair_sums(sums, units):
    refs = pair_refs()
    for name, dim, got in sums:
        ref, bound = refs[name]
        worst = H.assert_shifted_within(got, ref, bound, units.shift(dim), "%s under %r" % (name, units))
        print("UNITS %-28s %-22r error / bound %.3f" % (name, units, worst))


@pytest.mark.parametrize("units", (H.UNIT,) + PAIR_UNITS, ids=ids((H.UNIT,) + PAIR_UNITS))
def test_pair_statistics(units):
    """Pair counts of kk_twod, kk_log and vcorr_sums and the k-nearest-neighbour means (Y): equal bits.  xi (Y^2) and the weights
    of kk_twod, and kk_twod_bootstrap on both paths, are sums of fp64 atomics whose order the device does not fix: they do not
    repeat their own bits at one scale (LAB_NOTES.md "Change of units" records it), so they are held at every scale to
    the shifted long-double value of the unit-scale catalogue within its shifted error bound (tests/_pair_stat_refs.py: the
    bound test_gpu_pair_regimes.py uses, derived from u = 2^-53).  An absolute epsilon in the binning moves pair counts; an
    absolute threshold or constant on the values misses the bound by orders of magnitude at amp ~ 1e-15."""
    exact, sums = run_pairs(units)
    H.assert_homogeneous(exact, base("pairs", run_pairs)[0], units, "pair statistics")
    check_pair_sums(sums, units)


def test_pair_outputs_with_fixed_bits_repeat_themselves():
    """the premise of the bit comparison: at one scale, a second call on the same context gives the same bits"""
    H.assert_homogeneous(run_pairs(H.UNIT)[0], base("pairs", run_pairs)[0], H.UNIT, "pair statistics, same call twice")


# ---- 8: API ---------------------------------------------------------------------------------------------------------------

def _kernel_string(units, amp=H.AMP):
    a, b, c = (float(units.invlam(H.INVLAM[k])) for k in "abc")
    return "%r * AnisotropicRBF(invLam=array([[%r, %r], [%r, %r]]))" % (units.amp(amp), a, b, b, c)


def _gp(units, n=300, seed=0, white=0.03125):
    import treegp_amd
    P = H.inputs(n, seed=seed).at(units)
    y = P.y + units.y(np.float64(4.0))                       # the mean left in
    gp = treegp_amd.GPInterpolation(kernel=_kernel_string(units), optimizer="none", normalize=True,
                                    white_noise=float(units.val(white)))
    gp.initialize(P.X, y, y_err=P.e)
    gp.solve()
    return gp, P, y


def run_api(units):
    import treegp_amd
    gp, P, y = _gp(units)
    n = P.n
    out = [("predict", "predict", gp.predict(P.Xq))]
    yv, var = gp.predict(P.Xq, return_var=True)
    yc, cov = gp.predict(P.Xq[:130], return_cov=True)
    out += [("predict var.y", "predict", yv), ("predict var", "var", var), ("predict cov.y", "predict", yc),
            ("predict cov", "cov", cov), ("predict_gradient", "predict_grad", gp.predict_gradient(P.Xq))]
    yl, vl = gp.predict_loo(return_var=True)
    out += [("predict_loo", "predict", yl), ("predict_loo var", "var", vl)]
    groups = (np.arange(n) * 7) % 5
    yg, vg = gp.predict_lgo(groups, return_var=True)
    out += [("predict_lgo", "predict", yg), ("predict_lgo var", "var", vg)]
    Y = np.stack([y, units.y(np.cos(11.0 * H.inputs(n).X[:, 1]))])
    out.append(("predict_fields", "predict", gp.predict_fields(Y, P.Xq)))
    out.append(("sample_y", "field", gp.sample_y(P.Xq[:64], n_samples=3, random_state=5)))
    ypl, vpl, nbr = gp.predict_local(P.Xq, k=32, return_var=True, return_neighbors=True)
    out += [("predict_local", "predict", ypl), ("predict_local var", "var", vpl), ("predict_local nbr", "int", nbr)]
    out.append(("gaussian_random_field", "field",
                treegp_amd.gaussian_random_field(_kernel_string(units), P.X, n_samples=2, random_state=3, y_err=P.e)))
    out.append(("return_log_likelihood", None, gp.return_log_likelihood()))
    return out


def test_api_combined_units():
    """one GPInterpolation (optimizer="none", normalize=True, white_noise set, the mean left in the data) under S_a(-25) * S_x(+12):
    predict (mean, return_var, return_cov), predict_gradient, predict_loo, predict_lgo, predict_fields, sample_y with the same
    random_state (its jitter is nugget * max k, hence homogeneous), predict_local, gaussian_random_field; -2 return_log_likelihood
    moves by logdet's n 2p ln 2 and is held to the tolerance of a sum of n logarithms"""
    units = H.COMBINED
    got, ref = run_api(units), base("api", run_api)
    ll_s, ll_u = [v for k, _, v in got if k == "return_log_likelihood"][0], [v for k, _, v in ref if k == "return_log_likelihood"][0]
    # log L = -chi2 / 2 - n / 2 log 2 pi - logdet / 2: only logdet moves, by n * 2p * ln 2
    H.assert_log_shift(-2.0 * ll_s, -2.0 * ll_u, 300, 2 * units.p, "return_log_likelihood")
    H.assert_homogeneous(got, ref, units, "GPInterpolation")


def test_predict_many_in_different_units():
    """predict_many on two objects in different units: each result has the bits of the object's own unit-scale result"""
    import treegp_amd
    us = (Units(p=-25), Units(p=10, q=12))
    for kw in (dict(), dict(return_var=True), dict(return_cov=True)):
        gps = [_gp(u, n=200 + 57 * i, seed=3 + i) for i, u in enumerate(us)]
        ref = [_gp(H.UNIT, n=200 + 57 * i, seed=3 + i) for i in range(2)]
        got = treegp_amd.predict_many([g[0] for g in gps], [g[1].Xq[:130] for g in gps], **kw)
        want = treegp_amd.predict_many([g[0] for g in ref], [g[1].Xq[:130] for g in ref], **kw)
        for i, u in enumerate(us):
            g, w = (got[i], want[i]) if kw else ((got[i],), (want[i],))
            dims = ("predict", "cov" if "return_cov" in kw else "var")
            H.assert_homogeneous([("predict_many[%d].%d" % (i, j), dims[j], v) for j, v in enumerate(g)],
                                 [("predict_many[%d].%d" % (i, j), dims[j], v) for j, v in enumerate(w)], u, "predict_many %r" % (kw,))

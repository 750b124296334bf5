"""Pair-by-pair values of the device covariance functions against mpmath (used by test_gpu_kernel_values.py).

The entry points of the library only return sums of kernel values, except for a one-hot ``alpha``:
``gp_predict(spec, X, e_j, Xs)[q] = amp k(Xs_q, X_j)``, every other term being ``value * 0.0``.  This module
builds the point sets, the mpmath references and the bounds, and drives every route that computes a
covariance value on the device (packed K build, dense kernel matrix, fused predict).  The switches of the
fused predict (TGP_PREDICT_EXP / TGP_PREDICT_GENERIC / TGP_PREDICT_WGS) are read once per process, so the
same sweeps also run as a script in a fresh process:

    python tests/_kernel_value_helpers.py gauss      # one JSON line of measured maxima

The reference is mpmath only (never oracle/, never the library): exp(-q/2) with q formed in mpmath from the
fp64 coordinates by differencing first, and u^(5/6) K_{5/6}(2 pi u) / (Gamma(5/6) / (2 pi^(5/6))).
"""
import ctypes as C
import hashlib
import json
import os
import sys

import mpmath as mp
import numpy as np

mp.mp.dps = 40

LD = np.longdouble
assert np.finfo(LD).nmant >= 63 and np.finfo(LD).minexp <= -16000, "the references are carried as x87 long doubles"

U53 = 2.0 ** -53
TINY = 2.0 ** -1074            # smallest subnormal
MIN_NORMAL = 2.0 ** -1022
HALF_TINY = np.ldexp(LD(1.0), -1075)     # (not an fp64 number) below it the correctly rounded result is 0
K56_XMAX = 697.8738840444552   # bessel_k56.h
README_INVLAM = (400.0, 80.0, 500.0)       # a, b, c of [[400, 80], [80, 500]]


# ---------------------------------------------------------------------------------------------------------
# references
def _mpf_to_ld(v):
    """mpf -> long double to its full 64 bits, also far below the fp64 range"""
    if v == 0:
        return LD(0.0)
    man, e = mp.frexp(v)                      # v = man 2^e, 0.5 <= |man| < 1
    hi = float(man)
    lo = float(man - hi)
    return np.ldexp(LD(hi) + LD(lo), int(e))


def gauss_ref(Xq, xt, a, b, c, amp=1.0):
    """(ref, s): amp exp(-q/2) as long doubles and s = q/2 as fp64, q = a dx^2 + 2 b dx dy + c dy^2 in mpmath from the
    fp64 numbers, the difference taken first (treegp/kernels.py:114-126)"""
    a, b, c, amp = mp.mpf(a), mp.mpf(b), mp.mpf(c), mp.mpf(amp)
    x0, y0 = mp.mpf(float(xt[0])), mp.mpf(float(xt[1]))
    ref = np.empty(len(Xq), LD)
    s = np.empty(len(Xq))
    for i, (x, y) in enumerate(np.asarray(Xq, float).tolist()):
        dx, dy = mp.mpf(x) - x0, mp.mpf(y) - y0
        h = (a * dx * dx + 2 * b * dx * dy + c * dy * dy) / 2
        s[i] = float(h)
        ref[i] = _mpf_to_ld(amp * mp.exp(-h))
    return ref, s


def gauss_residues(s):
    """round(256 log2(e) s) mod 256: the entry of the 256-entry table of 2^(j/256) that the pair reads"""
    k = np.rint(LD(s) * (LD(256.0) / np.log(LD(2.0))))
    return (k % 256).astype(np.int64)


def vk_unit_mp(u):
    """u^(5/6) K_{5/6}(2 pi u) / lim0, 1 at u == 0 (treegp/kernels.py:249-276); u an mpf"""
    if u == 0:
        return mp.mpf(1)
    nu = mp.mpf(5) / 6
    lim0 = mp.gamma(nu) / (2 * mp.pi ** nu)
    return u ** nu * mp.besselk(nu, 2 * mp.pi * u) / lim0


def vk_ref_from_u(u):
    """(ref long double, 2 pi u as fp64) for fp64 arguments u taken as exact"""
    ref = np.empty(len(u), LD)
    x = np.empty(len(u))
    for i, v in enumerate(np.asarray(u, float).tolist()):
        m = mp.mpf(v)
        ref[i] = _mpf_to_ld(vk_unit_mp(m))
        x[i] = float(2 * mp.pi * m)
    return ref, x


def vk_ref_offaxis(Xq, xt, kind, amp, a=None, b=None, c=None, ell=None):
    """(ref, 2 pi u) with u formed in mpmath from the fp64 coordinates by differencing first"""
    x0, y0 = mp.mpf(float(xt[0])), mp.mpf(float(xt[1]))
    ref = np.empty(len(Xq), LD)
    xs = np.empty(len(Xq))
    for i, (x, y) in enumerate(np.asarray(Xq, float).tolist()):
        dx, dy = mp.mpf(x) - x0, mp.mpf(y) - y0
        if kind == "vk":
            u = mp.sqrt(dx * dx + dy * dy) / mp.mpf(ell)
        else:
            u = mp.sqrt(mp.mpf(a) * dx * dx + 2 * mp.mpf(b) * dx * dy + mp.mpf(c) * dy * dy)
        ref[i] = _mpf_to_ld(mp.mpf(amp) * vk_unit_mp(u))
        xs[i] = float(2 * mp.pi * u)
    return ref, xs


# ---------------------------------------------------------------------------------------------------------
# bounds
def diameter_exponent(points, a, b, c):
    """S = max over pairs of points of s(p - p') for a positive semi-definite invLam.  Searched among the extreme points
    of 64 directions of the transformed plane: the pair found is at least cos(1.5 deg)^2 = 0.9993 of the true maximum
    and never above it, which can only tighten a bound that grows with S."""
    P = np.asarray(points, float)
    P = P[np.all(np.isfinite(P), axis=1)]
    l00 = np.sqrt(a)
    l10 = b / l00
    l11 = np.sqrt(max(c - l10 * l10, 0.0))
    c0 = P.mean(axis=0)
    D = P - c0
    V = np.sqrt(0.5) * np.stack([l00 * D[:, 0] + l10 * D[:, 1], l11 * D[:, 1]], axis=1)
    th = np.pi * np.arange(64) / 64
    proj = V @ np.stack([np.cos(th), np.sin(th)])
    idx = np.unique(np.concatenate([proj.argmax(axis=0), proj.argmin(axis=0)]))
    E = V[idx]
    d2 = ((E[:, None, :] - E[None, :, :]) ** 2).sum(axis=2)
    return float(d2.max())


def gauss_bound(ref, s, S=None):
    """|dev - ref| <= (8 + 16 sqrt(s S)) 2^-53 ref + 2 * 2^-1074.

    8: table entry times polynomial <= 1.5 ulp (predict.hip), the amplitude multiply 0.5 ulp, doubled.  16 sqrt(s S): the
    exponent s goes through about a dozen roundings, each relative to a transformed coordinate of size sqrt(S) (S = the
    exponent across the diameter of the points of the call) while the difference is sqrt(s); exp turns an absolute error of
    the exponent into a relative error of the value.  Routes that difference first: S = s (S=None)."""
    s = np.abs(np.asarray(s, float))
    S = s if S is None else np.maximum(S, s)
    return (LD(8.0) + LD(16.0) * np.sqrt(LD(s) * LD(S))) * LD(U53) * np.abs(ref) + LD(2.0) * LD(TINY)


def term_magnitude(Xq, xt, a, b, c):
    """(|a| dx^2 + 2 |b| |dx dy| + |c| dy^2) / 2: what stands in for s in the bound of the routes that evaluate the form
    term by term (K build, kernel matrix, generic predict) when invLam is NOT positive definite (rank one, indefinite).
    There s is no norm: near the null direction of the form the three products cancel, while each of them is rounded
    relative to its own size, so the absolute error of the exponent scales with the sum of their magnitudes, as it does in
    the reference's own fp64 evaluation of the same expression.  For a positive definite form that sum is within
    (1 + rho) / (1 - rho), rho = |b| / sqrt(a c), of s (1.43 for the README's kernel), which the slope 16 absorbs; rho = 1
    for a rank-one form and > 1 for an indefinite one.  The fast path does not evaluate the form by terms (one
    transformed coordinate, squared) and keeps s and S."""
    d = np.asarray(Xq, float) - np.asarray(xt, float)
    return 0.5 * (abs(a) * d[:, 0] ** 2 + 2 * abs(b) * np.abs(d[:, 0] * d[:, 1]) + abs(c) * d[:, 1] ** 2)


def ulp_distance(x, y):
    """largest distance in units of the last place between two arrays of finite fp64 numbers of equal sign"""
    xi = np.ascontiguousarray(x, np.float64).view(np.int64)
    yi = np.ascontiguousarray(y, np.float64).view(np.int64)
    return int(np.abs(xi - yi).max()) if len(xi) else 0


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------
# point sets
GAUSS_XT = np.array([0.3125, 0.6875])
GAUSS_M = 30000


GAUSS_BAND = 300


def gauss_queries(xt=GAUSS_XT, m=GAUSS_M, lo=-8.0, hi=0.4, seed=20240607, band=None):
    """query 0 at the training point itself, m - 1 at distances 10^U(lo, hi) in random directions, and after them (README
    kernel only, band = its (a, b, c)) GAUSS_BAND points with q/2 uniform in [700, 760] in random directions.  The
    log-uniform law alone puts only ~40 of 30 000 points between the last normal number (q/2 = 708.4) and the last
    subnormal (744.4); the band makes that range, where the result loses its bits one by one, hold a few hundred."""
    rng = np.random.default_rng(seed)
    r = 10.0 ** rng.uniform(lo, hi, m)
    th = rng.uniform(0, 2 * np.pi, m)
    if band is not None:
        a, b, c = band
        tb = rng.uniform(0, 2 * np.pi, GAUSS_BAND)
        sb = rng.uniform(700.0, 760.0, GAUSS_BAND)
        rb = np.sqrt(2 * sb / (a * np.cos(tb) ** 2 + 2 * b * np.cos(tb) * np.sin(tb) + c * np.sin(tb) ** 2))
        r, th = np.concatenate([r, rb]), np.concatenate([th, tb])
    Xq = np.asarray(xt, float) + np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    Xq[0] = xt
    return Xq


def gauss_sweep_queries():
    return gauss_queries(band=README_INVLAM)


def gauss_training_pool(n=5000, seed=77):
    """pool[0] is the sweep's training point: every training set of the shape test is pool[:n], so all share the point the
    fused predict takes as the origin of its transform"""
    P = np.random.default_rng(seed).uniform(0, 1, (n, 2))
    P[0] = GAUSS_XT
    return P


def gauss_input_conditions(ref, s):
    """the coverage the Gaussian sweep promises, from the reference alone (amp == 1)"""
    normal = ref >= LD(MIN_NORMAL)
    sub = (ref >= LD(TINY)) & (ref < LD(MIN_NORMAL))
    zero = ref < HALF_TINY
    res = gauss_residues(s[normal])
    return {"residues": int(len(np.unique(res))), "normal": int(normal.sum()), "subnormal": int(sub.sum()),
            "zero": int(zero.sum()), "max_s": float(s.max())}


VK_SEGMENTS = ("series", "[1,2)", "[2,4)", "[4,8)", "[8,16)", "[16,32)", "[32,XMAX]")


def _neighbours(v):
    return [np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)]


def vk_onaxis_u(seed=0):
    """the host test's law made denser where the Chebyshev table is, and the fp64 neighbours of every branch point"""
    rng = np.random.default_rng(seed)
    parts = [[0.0], 10.0 ** rng.uniform(-9, 2.05, 3000), np.exp(rng.uniform(0.0, np.log(700.0), 3000)) / (2 * np.pi),
             [1 / (2 * np.pi), 32 / (2 * np.pi), 111.0, 111.08, 200.0]]
    for xb in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, K56_XMAX):
        parts.append(_neighbours(xb / (2 * np.pi)))
    return np.concatenate([np.asarray(p, float) for p in parts])


def vk_segment_counts(x):
    """points per branch of bessel_k56.h, from 2 pi u of the reference"""
    edges = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    out = {"series": int(((x > 0) & (x <= 1.0)).sum())}
    for k in range(5):
        out[VK_SEGMENTS[k + 1]] = int(((x > edges[k]) & (x < edges[k + 1])).sum())
    out["[32,XMAX]"] = int(((x >= 32.0) & (x <= K56_XMAX)).sum())
    return out


def vk_offaxis_queries(xt, scale, seed=5, m=3000):
    """distances scale * 10^U(-9, 2.05) in random directions around xt"""
    rng = np.random.default_rng(seed)
    r = scale * 10.0 ** rng.uniform(-9, 2.05, m)
    th = rng.uniform(0, 2 * np.pi, m)
    return np.asarray(xt, float) + np.stack([r * np.cos(th), r * np.sin(th)], axis=1)


# ---------------------------------------------------------------------------------------------------------
# device routes: each returns amp k(Xq_i, xt) for all i
def _tg():
    from treegp_amd import _lib, ops
    return _lib, ops, _lib.get_ctx()


def make_spec(kind, amp=1.0, a=1.0, b=0.0, c=1.0, ell=1.0):
    _lib, ops, _ = _tg()
    k = {"gauss": _lib.TGP_ARBF, "vk": _lib.TGP_VK, "avk": _lib.TGP_AVK}[kind]
    return ops.KernelSpec(k, amp=amp, a=a, b=b, c=c, ell=ell)


def route_predict(spec, xt, Xq):
    """the fused predict with n = 1 and alpha = [1]"""
    _, ops, _ = _tg()
    return ops.gp_predict(spec, np.asarray(xt, float).reshape(1, 2), np.ones(1), Xq)


def route_kmat_cross(spec, xt, Xq):
    _, ops, _ = _tg()
    return ops.kernel_matrix(spec, Xq, np.asarray(xt, float).reshape(1, 2))[:, 0].copy()


KB_POSITIONS = (0, 1, 127, 128, 255, 256, 257, 1000, 2047)


def _chunks(m, size):
    return [(i, min(i + size, m)) for i in range(0, m, size)]


def route_kmat_self(spec, xt, Xq, size=2047):
    """self kernel matrices of [chunk with the training point inserted]; returns (values, every diagonal entry == amp)"""
    _, ops, _ = _tg()
    out = np.empty(len(Xq))
    diag_ok = True
    for ci, (i0, i1) in enumerate(_chunks(len(Xq), size)):
        p = min(KB_POSITIONS[ci % len(KB_POSITIONS)], i1 - i0)
        X = np.insert(Xq[i0:i1], p, xt, axis=0)
        K = ops.kernel_matrix(spec, X)
        col, row = np.delete(K[:, p], p), np.delete(K[p, :], p)
        finite = np.isfinite(col)
        diag_ok = diag_ok and bool(np.array_equal(col[finite], row[finite]))           # k(x, x') == k(x', x) bit for bit
        d = np.diag(K)[np.all(np.isfinite(X), axis=1)]
        diag_ok = diag_ok and bool(np.all(d == spec.amp))
        out[i0:i1] = col
    return out, diag_ok


def route_kbuild(spec, xt, Xq, size=2047):
    """the packed K build (what every solve factorises) unpacked again; the training point sits at a different row of
    each chunk's matrix, so its pairs come from a row and a column of the lower triangle"""
    _lib, ops, ctx = _tg()
    lib = _lib.load_library()
    out = np.empty(len(Xq))
    diag_ok = True
    for ci, (i0, i1) in enumerate(_chunks(len(Xq), size)):
        p = min(KB_POSITIONS[ci % len(KB_POSITIONS)], i1 - i0)
        X = np.ascontiguousarray(np.insert(Xq[i0:i1], p, xt, axis=0))
        n = len(X)
        Np = lib.tgp_padded_n(n)
        dX = ops.DeviceBuffer.from_array(ctx, X)
        de = ops.DeviceBuffer.from_array(ctx, np.zeros(n))
        dA = ops.DeviceBuffer(ctx, lib.tgp_panel_elems(Np) * 8)
        _lib.check(ctx, lib.tgp_d_kbuild_lower(ctx, C.byref(spec.to_c()), dX.ptr, n, de.ptr, dA.ptr), "kbuild")
        K = np.empty((n, n))
        _lib.check(ctx, lib.tgp_d_unpack_lower(ctx, dA.ptr, Np, n, K.ctypes.data_as(C.c_void_p)), "unpack")
        for buf in (dX, de, dA):
            buf.free()
        v = np.concatenate([K[p, :p], K[p + 1:, p]])
        d = np.diag(K)[np.all(np.isfinite(X), axis=1)]
        diag_ok = diag_ok and bool(np.all(d == spec.amp))
        out[i0:i1] = v
    return out, diag_ok


# ---------------------------------------------------------------------------------------------------------
# comparisons
def compare(dev, ref, bound, must_be_zero=None):
    """largest error / bound and where; NaN or infinite device values count as infinitely wrong"""
    dev = np.asarray(dev, float)
    err = np.abs(LD(dev) - ref)
    ratio = np.where(np.isfinite(dev), err / bound, np.inf).astype(float)
    i = int(np.argmax(ratio))
    out = {"max_ratio": float(ratio[i]), "at": i, "dev": float(dev[i]), "ref": float(ref[i]), "n_over": int((ratio > 1.0).sum())}
    if must_be_zero is not None:
        out["nonzero_where_zero"] = int((dev[must_be_zero] != 0.0).sum())
    return out


def gauss_compare(dev, ref, s, amp, S=None, kbuild=False):
    """The Gaussian bound.  The packed K build clamps its exponent at 2^-1021 (kernel_eval.h): below that its documented
    stand-in is amp 2^-1021, absolute error < amp 4.5e-308, and it does not return exact zeros."""
    bound = gauss_bound(ref, s, S)
    zero = ref < LD(amp) * HALF_TINY
    if kbuild:
        clamped = ref < LD(amp) * LD(2.0 ** -1021) * (1 + LD(1e-9))
        out = compare(dev, ref, bound + np.where(clamped, LD(amp) * LD(4.5e-308), LD(0.0)))
        out["max_ratio_above_clamp"] = compare(dev[~clamped], ref[~clamped], bound[~clamped])["max_ratio"]
        return out
    return compare(dev, ref, bound, must_be_zero=zero)


def nan_check(spec, xt, Xq, base, at=1000):
    """a NaN coordinate in one query gives NaN there and leaves every other query's bits alone"""
    Xn = Xq.copy()
    Xn[at, 1] = np.nan
    v = route_predict(spec, xt, Xn)
    others = np.arange(len(Xq)) != at
    return bool(np.isnan(v[at])) and bool(np.array_equal(v[others], base[others]))


def gauss_sweep(routes=("predict", "kmat_cross", "kmat_self", "kbuild")):
    """the one-training-point sweep of the README's kernel on the given routes -> dict of measured maxima"""
    a, b, c = README_INVLAM
    Xq = gauss_sweep_queries()
    ref, s = gauss_ref(Xq, GAUSS_XT, a, b, c, 1.0)
    out = {"inputs": gauss_input_conditions(ref, s), "routes": {}}
    S = diameter_exponent(np.vstack([GAUSS_XT[None], Xq]), a, b, c)
    normal = ref >= LD(MIN_NORMAL)
    for amp in (1.0, 1.7):
        spec = make_spec("gauss", amp=amp, a=a, b=b, c=c)
        for r in routes:
            diag_ok = True
            if r == "predict":
                dev = route_predict(spec, GAUSS_XT, Xq)
            elif r == "kmat_cross":
                dev = route_kmat_cross(spec, GAUSS_XT, Xq)
            elif r == "kmat_self":
                dev, diag_ok = route_kmat_self(spec, GAUSS_XT, Xq)
            else:
                dev, diag_ok = route_kbuild(spec, GAUSS_XT, Xq)
            fast = r == "predict" and "TGP_PREDICT_GENERIC" not in os.environ
            if amp == 1.0:
                res = gauss_compare(dev, ref, s, amp, S=S if fast else None, kbuild=(r == "kbuild"))
            else:       # the amplitude multiply, where the value is a normal number (the tiny range is checked at amp = 1)
                refa = ref * LD(amp)
                res = gauss_compare(dev[normal], refa[normal], s[normal], amp, S=S if fast else None, kbuild=(r == "kbuild"))
            refn = ref[normal] * LD(amp)             # reported only: where the relative part of the bound is what decides
            if r != "kbuild":                       # (the K build reports max_ratio_above_clamp)
                res["max_ratio_normal"] = compare(dev[normal], refn, gauss_bound(refn, s[normal], S if fast else None))["max_ratio"]
            res["at_zero_exact"] = bool(dev[0] == amp) and diag_ok
            if r == "predict" and amp == 1.0:
                res["nan_ok"] = nan_check(spec, GAUSS_XT, Xq, dev)
                res["digest"] = digest(dev)
            out["routes"]["%s amp=%g" % (r, amp)] = res
    return out


SHAPE_NS = (1, 2, 255, 256, 257, 600, 5000)
SHAPE_MS = (1, 255, 256, 257)


def shape_js(n):
    return sorted({j for j in (0, 1, 254, 255, 256, n - 1) if 0 <= j < n})


def gauss_shapes():
    """One-hot alpha against training sets of many sizes.  The fused predict takes its first training point as the origin
    of its transform, so every set here starts with the same point (pool[0]) and the value of a pair must then not
    depend on n, m, the number of splits or the position of the training point in the set: bit-identical.  Against the
    n = 1 call with that training point ALONE the origin differs (it is that point), so those two agree only within the
    sum of their bounds."""
    _, ops, _ = _tg()
    a, b, c = README_INVLAM
    spec = make_spec("gauss", amp=1.0, a=a, b=b, c=c)
    P = gauss_training_pool()
    Xq = gauss_sweep_queries()
    base = {}
    for j in sorted({j for n in SHAPE_NS for j in shape_js(n)}):
        X = P[:1] if j == 0 else np.stack([P[0], P[j]])
        base[j] = ops.gp_predict(spec, X, np.eye(len(X))[-1], Xq)
    mismatches, calls = [], 0
    for n in SHAPE_NS:
        for j in shape_js(n):
            v = ops.gp_predict(spec, P[:n], np.eye(n)[j], Xq)
            calls += 1
            if not np.array_equal(v, base[j]):
                mismatches.append(["n", n, j, int((v != base[j]).sum())])
    for m in SHAPE_MS:
        for j in (0, 255, 599):
            v = ops.gp_predict(spec, P[:600], np.eye(600)[j], Xq[:m])
            calls += 1
            if not np.array_equal(v, base[j][:m]):
                mismatches.append(["m", m, j, int((v != base[j][:m]).sum())])
    Xsw = P[:600].copy()
    Xsw[[1, 255]] = Xsw[[255, 1]]                      # the same point at another position of the set
    for j, jb in ((255, 1), (1, 255)):
        v = ops.gp_predict(spec, Xsw, np.eye(600)[j], Xq)
        calls += 1
        if not np.array_equal(v, base[jb]):
            mismatches.append(["position", j, jb, int((v != base[jb]).sum())])
    # against the call with that training point alone: both within the bound of the reference, so within the sum
    S = diameter_exponent(np.vstack([P, Xq]), a, b, c)
    worst = 0.0
    for j in (1, 255, 4999):
        alone = route_predict(spec, P[j], Xq)
        d = Xq - P[j]
        s = 0.5 * (a * d[:, 0] ** 2 + 2 * b * d[:, 0] * d[:, 1] + c * d[:, 1] ** 2)
        tol = 2 * gauss_bound(LD(np.maximum(alone, base[j])), s, S)
        worst = max(worst, float((np.abs(LD(alone) - LD(base[j])) / tol).max()))
    return {"calls": calls, "mismatches": mismatches, "alone_vs_set_max_ratio": worst,
            "digest": digest(*[base[j] for j in sorted(base)])}


FALLBACKS = {
    # name: (a, b, c, log10 of the largest distance, what launch_predict does with it)
    "1-D c=b=0": (0.25, 0.0, 0.0, 1.9, "fast path, t11 = 0"),
    "a=0 c>0": (0.0, 0.0, 300.0, 0.4, "generic path (no Cholesky of invLam)"),
    "rank one": (4.0, 2.0, 1.0, 1.4, "fast path, c - b^2/a == 0 exactly"),
    "indefinite": (1.0, 3.0, 1.0, 0.75, "generic path, values above 1"),
}


def gauss_fallbacks():
    out = {}
    for name, (a, b, c, hi, _) in FALLBACKS.items():
        Xq = gauss_queries(m=4000, lo=-8.0, hi=hi, seed=11)
        ref, s = gauss_ref(Xq, GAUSS_XT, a, b, c, 1.3)
        spec = make_spec("gauss", amp=1.3, a=a, b=b, c=c)
        res = {"min_q": float(2 * s.min()), "max_ref": float(ref.max())}
        fast = name in ("1-D c=b=0", "rank one") and "TGP_PREDICT_GENERIC" not in os.environ
        S = diameter_exponent(np.vstack([GAUSS_XT[None], Xq]), a, b, c) if fast else None
        st = term_magnitude(Xq, GAUSS_XT, a, b, c) if name in ("rank one", "indefinite") else s
        for r, f in (("predict", route_predict), ("kmat_cross", route_kmat_cross)):
            dev = f(spec, GAUSS_XT, Xq)
            if r == "predict" and fast:
                res[r] = gauss_compare(dev, ref, s, 1.3, S=S)
            else:
                res[r] = gauss_compare(dev, ref, st, 1.3)
            res[r]["at_zero_exact"] = bool(dev[0] == 1.3)
        out[name] = res
    return out


VK_CASES = {"vk": dict(ell=0.5), "avk": dict(a=4.0, b=0.0, c=1.0)}        # both: u = 2 |x| exactly for points (x, 0)
VK_OFF = {"vk": dict(ell=0.3), "avk": dict(a=400.0, b=80.0, c=500.0)}
VK_OFF_SCALE = {"vk": 0.3, "avk": 0.05}


def vk_bound(ref, amp, x=None):
    """the host test's own tolerance (rtol 2e-13, atol 1e-13 on the unit value); off the axis u itself is rounded a few
    times and d ln k / d ln u -> -2 pi u, so rtol grows by 8 * 2 pi u * 2^-53"""
    rtol = LD(2e-13) + (LD(8.0) * LD(x) * LD(U53) if x is not None else LD(0.0))
    return LD(amp) * LD(1e-13) + rtol * np.abs(ref)


def vk_sweep():
    out = {}
    u = vk_onaxis_u()
    ref, x = vk_ref_from_u(u)
    out["segments"] = vk_segment_counts(x)
    xt = np.zeros(2)
    Xq = np.stack([u / 2, np.zeros_like(u)], axis=1)
    x64 = (2 * np.pi) * u                        # the function's own fp64 argument (one IEEE multiply by fl(2 pi))
    beyond = x64 > K56_XMAX
    for kind, kw in VK_CASES.items():
        spec = make_spec(kind, amp=1.0, **kw)
        devs = {"predict": route_predict(spec, xt, Xq), "kmat_cross": route_kmat_cross(spec, xt, Xq)}
        devs["kbuild"], diag_ok = route_kbuild(spec, xt, Xq[1:])            # (query 0 is the training point: the diagonal)
        devs["kbuild"] = np.concatenate([[1.0 if diag_ok else np.nan], devs["kbuild"]])
        res = {}
        for r, dev in devs.items():
            res[r] = compare(dev, ref, vk_bound(ref, 1.0), must_be_zero=beyond)
            res[r]["at_zero_exact"] = bool(dev[0] == 1.0)
        res["routes_max_ulp"] = max(ulp_distance(devs["predict"], devs["kmat_cross"]), ulp_distance(devs["predict"], devs["kbuild"]))
        out[kind] = res
        amp = 0.49
        xo = np.array([0.4, -0.2])
        Xo = vk_offaxis_queries(xo, VK_OFF_SCALE[kind])
        refo, xs = vk_ref_offaxis(Xo, xo, kind, amp, **VK_OFF[kind])
        spec = make_spec(kind, amp=amp, **VK_OFF[kind])
        devs = {"predict": route_predict(spec, xo, Xo), "kmat_cross": route_kmat_cross(spec, xo, Xo)}
        devs["kbuild"], _ = route_kbuild(spec, xo, Xo)
        far = xs > K56_XMAX * (1 + 1e-12)
        res = {r: compare(dev, refo, vk_bound(refo, amp, xs), must_be_zero=far) for r, dev in devs.items()}
        res["routes_max_ulp"] = max(ulp_distance(devs["predict"], devs["kmat_cross"]), ulp_distance(devs["predict"], devs["kbuild"]))
        out[kind + " off-axis"] = res
    return out


# ---------------------------------------------------------------------------------------------------------
# translation invariance
TRANSLATIONS = ((0.0, 0.0), (1024.0, 1024.0), (2.0 ** 20, 2.0 ** 20), (-2.0 ** 20, 2.0 ** 17))
TRANSLATION_KERNELS = {"README": README_INVLAM, "ell=0.005": (40000.0, 8000.0, 50000.0)}


def translation_data(n=600, m=1000, seed=9):
    """points of the unit square on a 2^-20 grid: every offset of TRANSLATIONS adds to them exactly"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 2 ** 20, (n, 2)) / 2.0 ** 20
    Xs = rng.integers(0, 2 ** 20, (m, 2)) / 2.0 ** 20
    y = np.sin(7 * X[:, 0]) * np.cos(5 * X[:, 1]) + 0.03 * rng.standard_normal(n)
    e = 0.03 * rng.uniform(0.8, 1.2, n)
    return X, Xs, y, e


def gauss_ref_matrix_ld(Xs, X, a, b, c):
    """exp(-q/2) for all pairs in long double; the differences of grid points are exact in fp64"""
    dx = LD(Xs[:, None, 0] - X[None, :, 0])
    dy = LD(Xs[:, None, 1] - X[None, :, 1])
    return np.exp(-(LD(a) * dx * dx + 2 * LD(b) * dx * dy + LD(c) * dy * dy) / 2)


def translation_sweep():
    _, ops, _ = _tg()
    X, Xs, y, e = translation_data()
    out = {}
    for kname, (a, b, c) in TRANSLATION_KERNELS.items():
        spec = make_spec("gauss", amp=1.0, a=a, b=b, c=c)
        S = diameter_exponent(np.vstack([X, Xs]), a, b, c)
        onehot_ref = {j: gauss_ref(Xs, X[j], a, b, c, 1.0) for j in (0, 299, 599)}
        R = gauss_ref_matrix_ld(Xs, X, a, b, c)
        for t in TRANSLATIONS:
            t = np.asarray(t)
            Xt, Xst = X + t, Xs + t
            assert np.array_equal(Xt - t, X) and np.array_equal(Xst - t, Xs)
            res = {"onehot_max_ratio": 0.0}
            for j, (ref, s) in onehot_ref.items():
                dev = ops.gp_predict(spec, Xt, np.eye(len(X))[j], Xst)
                res["onehot_max_ratio"] = max(res["onehot_max_ratio"], compare(dev, ref, gauss_bound(ref, s, S))["max_ratio"])
            alpha = ops.gp_solve(spec, Xt, y, e)[0]
            yp = ops.gp_predict(spec, Xt, alpha, Xst)
            yref = R @ LD(alpha)
            scale = float(np.abs(yref).max())
            res["predict_vs_ref"] = float(np.abs(LD(yp) - yref).max()) / scale
            res["predict_vs_unshifted"] = float(np.abs(yp - ops.gp_predict(spec, X, alpha, Xs)).max()) / scale
            out["%s t=(%g, %g)" % (kname, t[0], t[1])] = res
    return out


def translation_api():
    """GPInterpolation at an offset of 2^20 against the same object at the origin, singly and through predict_many"""
    import treegp_amd as treegp
    X, Xs, y, e = translation_data()
    kern = "1.0**2 * AnisotropicRBF(invLam=array([[400., 80.], [80., 500.]]))"

    def obj(t):
        gp = treegp.GPInterpolation(kernel=kern, optimizer="none", normalize=True)
        gp.initialize(X + np.asarray(t), y, y_err=e)
        return gp
    y0 = obj((0.0, 0.0)).predict(Xs)
    scale = float(np.abs(y0).max())
    t1, t2 = np.array(TRANSLATIONS[2]), np.array(TRANSLATIONS[3])
    y1 = obj(t1).predict(Xs + t1)
    many = treegp.predict_many([obj(t1), obj(t2)], [Xs + t1, Xs + t2])
    return {"predict": float(np.abs(y1 - y0).max()) / scale,
            "predict_many": max(float(np.abs(np.asarray(v) - y0).max()) for v in many) / scale}


SWEEPS = {"gauss": lambda: gauss_sweep(routes=("predict",)), "gauss_all": gauss_sweep, "shapes": gauss_shapes,
          "fallbacks": gauss_fallbacks, "vk": vk_sweep, "translation": translation_sweep, "translation_api": translation_api}


def run_in_fresh_process(sweeps, env, timeout=900):
    """run the named sweeps as `python <this file> name ...` with `env` added, return the parsed JSON line"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(sweeps), env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, (env, r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return json.loads(lines[-1])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps({name: SWEEPS[name]() for name in sys.argv[1:]}))

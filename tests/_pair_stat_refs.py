"""Host references of the pair-statistics seam (S4 of include/tgp.h: tgp_kk_twod, tgp_kk_log, tgp_kk_partial,
tgp_kk_twod_bootstrap, tgp_vcorr, tgp_knn_mean, tgp_binned_stat_2d), independent of the device and of oracle/gp_oracle.py.

NumPy only.  Which pair goes to which bin is decided in fp64, by the rule the kernels state (kk.hip:7-9, vcorr.hip:4-6)
evaluated exactly as written: the rule is defined in IEEE arithmetic.  Every sum is then formed in np.longdouble (64-bit
mantissa here, eps 1.08e-19, as tests/_dist_block_refs.py assumes) from the fp64 inputs, and travels with the sum of the
absolute values of its terms, which is what an error bound of a floating-point sum scales with.

Error bounds (derived, not tuned).  u = 2^-53, N_b the exact number of terms of bin b.  A sum of N terms in any order is off
by at most (N - 1) u sum|t|; a term is formed with at most three roundings; a quotient adds one:

  raw sum S_b (kk_partial, vcorr)         |got - ref| <= 2 (N_b + 4) u A_b                      `bound_sum`
  xi_b = S_b / W_b, meanr                 <= 2 (N_b + 4) u (A_b / W_b + |ref|)                  `bound_ratio`
  meanlogr, vcorr sums with log / hypot / division by rsq:  the same with N_b + 8 (2 ulp per device function)
  weight                                  <= 2 (N_b + 2) u W_b
  npairs, vcorr counts                    equal

The factor 2 covers the u^2 terms and the reference's own rounding.  What A_b is for a term that is itself a sum of products:
the sum of the absolute values of those products, because a term that cancels inside (u_i u_j - v_i v_j) is off by roundings
of its parts, not of its value.  So for vcorr
  xi+    term u_i u_j + v_i v_j                  magnitude |u_i u_j| + |v_i v_j|
  z2     terms u_i u_j - v_i v_j, u_i v_j + v_i u_j   magnitude (|u_i| + |v_i|) (|u_j| + |v_j|)
  xi-    term z conj(d)^2 / |d|^2                magnitude (|u_i| + |v_i|) (|u_j| + |v_j|) (|dx| + |dy|)^2 / rsq
         (nine rounding levels for a term: 8 + the (N_b - 1) of the summation stay within 2 (N_b + 8))
  log r  term ln hypot(dx, dy)                   magnitude |ln r| + 1: a relative error eps of r moves ln r by eps
         ABSOLUTELY, however small |ln r| is (r near 1), so hypot's 2 ulp enter as 2 u x 1, the log's as 2 u |ln r|.
In kk_log ln r = 0.5 log(rsq) is taken of the fp64 rsq the rule itself defines, so only the log's own error enters and the
magnitude is |ln r|.

Bootstrap (tgp_kk_twod_bootstrap, both device paths).  t = c_i c_j w_i w_j, v = y - mean(yv), mu = mu_b - mean(yv),
eps_c = (n + 2) u max|yv| the uncertainty of a value centred in fp64 (it covers the fp64 means of n terms):
  |xi_b - ref| <= 2 [(N_b + 6) u (sum t|v_i v_j| + |mu| sum t(|v_i| + |v_j|) + mu^2 sum t)
                     + eps_c sum t(|v_i| + |v_j|) + eps_c^2 sum t] / sum t                      `bound_boot`
and twice that between the two device paths.  N_b counts the terms the device adds: the pixel's deposits of the BASE
catalogue (the pair lists visit every base pair, also where a multiplicity is zero), each counted e_i e_j times where
e = max(1, ceil(c / 255)) is the number of byte-sized entries a point drawn c times is split into on the per-resample path
(kk.hip:354-360).
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
KT = 256                        # points per tile of every pair kernel


# ---- small tools ------------------------------------------------------------------------------------------------------

def _binsum(b, t, nb):
    """per-bin long-double sums of the terms t with bin numbers b"""
    out = np.zeros(nb, dtype=LD)
    b = np.asarray(b)
    if b.size == 0:
        return out
    o = np.argsort(b, kind="stable")
    bs_, ts = b[o], np.asarray(t, dtype=LD)[o]
    starts = np.flatnonzero(np.r_[True, bs_[1:] != bs_[:-1]])
    out[bs_[starts]] = np.add.reduceat(ts, starts)
    return out


def _ratio(s, w):
    """s / w in long double, 0 where w == 0 (the library's convention)"""
    nz = w != 0
    return np.where(nz, s / np.where(nz, w, LD(1)), LD(0))


def bound_sum(N, A, extra=4):
    return 2.0 * (np.asarray(N, dtype=np.float64) + extra) * U * np.asarray(A, dtype=np.float64)


def bound_ratio(N, A, W, ref, extra=4):
    W = np.asarray(W, dtype=np.float64)
    nz = W != 0.0
    aw = np.where(nz, np.asarray(A, dtype=np.float64) / np.where(nz, W, 1.0), 0.0)
    return 2.0 * (np.asarray(N, dtype=np.float64) + extra) * U * (aw + np.abs(np.asarray(ref, dtype=np.float64)))


def bound_weight(N, W):
    return bound_sum(N, W, extra=2)


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound (0 / 0 counts as 0: where the bound is zero the values must be equal)"""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD)).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ---- TwoD -------------------------------------------------------------------------------------------------------------

def twod_deposits(x, y, min_sep, max_sep, nbins):
    """Every deposit of the TwoD rule (kk.hip:7-8): arrays i, j (i < j in caller order) and pixel b, two per accepted pair
    (d and -d) unless an orientation falls outside the grid.  Also `edge_gap` (smallest distance of a bin coordinate of an
    accepted pair from an integer, in bin widths) and `on_edge` (deposits with a coordinate exactly on an integer)."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    n = len(x)
    i, j = np.triu_indices(n, 1)
    dx, dy = x[j] - x[i], y[j] - y[i]
    rsq = dx * dx + dy * dy
    ok = (rsq != 0.0) & (rsq >= min_sep * min_sep) & (np.maximum(np.abs(dx), np.abs(dy)) < max_sep)
    i, j, dx, dy = i[ok], j[ok], dx[ok], dy[ok]
    bs = 2.0 * max_sep / nbins
    I, J, B = [], [], []
    gap, on_edge = np.inf, 0
    for sgn in (1.0, -1.0):
        cx, cy = (sgn * dx + max_sep) / bs, (sgn * dy + max_sep) / bs
        ix, iy = cx.astype(np.int64), cy.astype(np.int64)
        good = (ix >= 0) & (ix < nbins) & (iy >= 0) & (iy < nbins)
        I.append(i[good]); J.append(j[good]); B.append(iy[good] * nbins + ix[good])
        if len(cx):
            g = np.minimum(np.abs(cx - np.rint(cx)), np.abs(cy - np.rint(cy)))
            gap = min(gap, float(g.min()))
            on_edge += int(np.count_nonzero(g[good] == 0.0))
    return dict(i=np.concatenate(I), j=np.concatenate(J), b=np.concatenate(B), edge_gap=gap, on_edge=on_edge,
                naccepted=int(len(i)))


def ref_kk_twod(x, y, k, w, min_sep, max_sep, nbins):
    """npairs (exact integers), wkk = sum ww kk, weight = sum ww, A = sum |ww kk|, xi = wkk / weight, edge_gap."""
    n = len(x)
    k = np.asarray(k, dtype=np.float64)
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    d = twod_deposits(x, y, min_sep, max_sep, nbins)
    i, j, b = d["i"], d["j"], d["b"]
    nb2 = nbins * nbins
    ww = w[i].astype(LD) * w[j].astype(LD)
    kk = k[i].astype(LD) * k[j].astype(LD)
    wkk = _binsum(b, ww * kk, nb2)
    wt = _binsum(b, ww, nb2)
    return dict(npairs=np.bincount(b, minlength=nb2).astype(np.int64), wkk=wkk, weight=wt, A=_binsum(b, np.abs(ww * kk), nb2),
                xi=_ratio(wkk, wt), edge_gap=d["edge_gap"], on_edge=d["on_edge"], naccepted=d["naccepted"])


# ---- Log --------------------------------------------------------------------------------------------------------------

def ref_kk_log(x, y, k, w, min_sep, max_sep, nbins):
    """Log rule (kk.hip:9): bin int((ln r - ln min_sep) / bs), ln r = 0.5 log(rsq), for minsq <= rsq < maxsq, each pair
    once.  npairs, wkk, weight, wr = sum ww r, wlogr = sum ww ln r, A = sum |ww kk|, AL = sum ww |ln r|, the quotients xi,
    meanr, meanlogr, `edge_gap` and `range_gap` (smallest relative distance of any rsq from minsq and maxsq)."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64); k = np.asarray(k, dtype=np.float64)
    n = len(x)
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    i, j = np.triu_indices(n, 1)
    dx, dy = x[j] - x[i], y[j] - y[i]
    rsq = dx * dx + dy * dy
    minsq, maxsq = min_sep * min_sep, max_sep * max_sep
    range_gap = float(min(np.abs(rsq - minsq).min() / minsq, np.abs(rsq - maxsq).min() / maxsq))
    ok = (rsq >= minsq) & (rsq < maxsq)
    i, j, rsq = i[ok], j[ok], rsq[ok]
    bs = math.log(max_sep / min_sep) / nbins
    lmin = math.log(min_sep)
    c = (0.5 * np.log(rsq) - lmin) / bs
    b = c.astype(np.int64)
    edge_gap = float(np.abs(c - np.rint(c)).min()) if len(c) else np.inf
    good = (b >= 0) & (b < nbins)
    i, j, rsq, b = i[good], j[good], rsq[good], b[good]
    ww = w[i].astype(LD) * w[j].astype(LD)
    kk = k[i].astype(LD) * k[j].astype(LD)
    rl = rsq.astype(LD)
    lr = LD(0.5) * np.log(rl)
    wkk, wt = _binsum(b, ww * kk, nbins), _binsum(b, ww, nbins)
    wr, wl = _binsum(b, ww * np.sqrt(rl), nbins), _binsum(b, ww * lr, nbins)
    return dict(npairs=np.bincount(b, minlength=nbins).astype(np.int64), wkk=wkk, weight=wt, wr=wr, wlogr=wl,
                A=_binsum(b, np.abs(ww * kk), nbins), AL=_binsum(b, ww * np.abs(lr), nbins),
                xi=_ratio(wkk, wt), meanr=_ratio(wr, wt), meanlogr=_ratio(wl, wt), edge_gap=edge_gap, range_gap=range_gap)


def kk_bounds(ref, log):
    """bounds of the finished outputs of tgp_kk_twod / tgp_kk_log from a reference dict"""
    N = ref["npairs"]
    out = dict(xi=bound_ratio(N, ref["A"], ref["weight"], ref["xi"]), weight=bound_weight(N, ref["weight"]))
    if log:
        out["meanr"] = bound_ratio(N, ref["wr"], ref["weight"], ref["meanr"])
        out["meanlogr"] = bound_ratio(N, ref["AL"], ref["weight"], ref["meanlogr"], extra=8)
    return out


def kk_raw(ref, log):
    """the raw accumulators in tgp_kk_partial's layout with their bounds: (refs, bounds), rows wkk, w, [wr, wlogr,] n"""
    N = ref["npairs"]
    if log:
        refs = [ref["wkk"], ref["weight"], ref["wr"], ref["wlogr"], N]
        bnds = [bound_sum(N, ref["A"]), bound_weight(N, ref["weight"]), bound_sum(N, ref["wr"]),
                bound_sum(N, ref["AL"], extra=8), np.zeros(len(N))]
    else:
        refs = [ref["wkk"], ref["weight"], N]
        bnds = [bound_sum(N, ref["A"]), bound_weight(N, ref["weight"]), np.zeros(len(N))]
    return refs, bnds


# ---- bootstrap --------------------------------------------------------------------------------------------------------

def ref_kk_bootstrap(x, y, yv, yerr, idx, min_sep, max_sep, nbins, chunk=32):
    """TwoD bootstrap (two_pcf.py:342-362): the base pairs and their two pixels are enumerated once; per resample b the
    multiplicities c, w = 1 / yerr^2 (unit weights if sum(yerr) == 0) and mu_b = mean(yv[idx_b]) in long double give
      xi[b] = sum c_i c_j w_i w_j (y_i - mu_b)(y_j - mu_b) / sum c_i c_j w_i w_j      (0 where the denominator is 0)
    Returns xi (n_boot, nbins^2) and `bound` of the same shape (the module docstring's bootstrap bound)."""
    x = np.asarray(x, dtype=np.float64); yv = np.asarray(yv, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    n_boot, n = idx.shape
    nb2 = nbins * nbins
    if yerr is None or np.sum(yerr) == 0:
        w = np.ones(n, dtype=LD)
    else:
        e = np.asarray(yerr, dtype=np.float64).astype(LD)
        w = LD(1) / (e * e)
    d = twod_deposits(x, y, min_sep, max_sep, nbins)
    o = np.argsort(d["b"], kind="stable")
    I, J, B = d["i"][o], d["j"][o], d["b"][o]
    xi = np.zeros((n_boot, nb2), dtype=LD)
    bound = np.zeros((n_boot, nb2))
    if len(B) == 0:
        return dict(xi=xi, bound=bound, ndeposits=0)
    starts = np.flatnonzero(np.r_[True, B[1:] != B[:-1]])
    bins = B[starts]
    yl = yv.astype(LD)
    mean0 = yl.sum() / LD(n)
    v0 = yl - mean0
    ww = w[I] * w[J]
    P = np.abs(v0[I] * v0[J]); Q = np.abs(v0[I]) + np.abs(v0[J])
    eps_c = (n + 2) * U * float(np.abs(yv).max())
    for s in range(0, n_boot, chunk):
        rows = idx[s:s + chunk]
        c = np.stack([np.bincount(r, minlength=n) for r in rows])                    # (chunk, n)
        mu_b = yl[rows].sum(axis=1) / LD(n)
        t = (c[:, I] * c[:, J]).astype(LD) * ww[None, :]
        yi = yl[I][None, :] - mu_b[:, None]; yj = yl[J][None, :] - mu_b[:, None]
        S = np.add.reduceat(t * yi * yj, starts, axis=1)
        T = np.add.reduceat(t, starts, axis=1)
        Pb = np.add.reduceat(t * P[None, :], starts, axis=1).astype(np.float64)
        Qb = np.add.reduceat(t * Q[None, :], starts, axis=1).astype(np.float64)
        ent = np.maximum(1, -(-c // 255))
        Nb = np.add.reduceat(ent[:, I] * ent[:, J], starts, axis=1).astype(np.float64)
        xi[s:s + chunk, bins] = _ratio(S, T)
        Tf = T.astype(np.float64)
        mu = np.abs((mu_b - mean0).astype(np.float64))[:, None]
        num = (Nb + 6) * U * (Pb + mu * Qb + mu * mu * Tf) + eps_c * Qb + eps_c * eps_c * Tf
        bound[s:s + chunk, bins] = np.where(Tf != 0.0, 2.0 * num / np.where(Tf != 0.0, Tf, 1.0), 0.0)
    return dict(xi=xi, bound=bound, ndeposits=int(len(B)))


def reference_stream(n, n_boot, seed=610639139):
    """the index stream of two_pcf.py:264-281, 348-351: one PCG64 generator, integers(0, n - 1, size=n) per resample"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n - 1, size=n) for _ in range(n_boot)]).astype(np.int64)


# ---- vcorr ------------------------------------------------------------------------------------------------------------

def ref_vcorr(x, y, dx, dy, edges):
    """The seven per-bin sums of vcorr.hip over all pairs i < j, bin numbers by np.histogram's rule on the given edges
    (edges[b] <= ln r < edges[b + 1], the last edge inclusive).  `sums` (7, nbins) long double: count, sum ln r, xi+ terms,
    Re and Im of v_i v_j, Re and Im of v_i v_j conj(d)^2 / |d|^2; `mags` the matching sums of magnitudes (module docstring);
    `edge_gap`: smallest distance of any pair's ln r from an edge, in units of the narrowest bin."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    u = np.asarray(dx, dtype=np.float64); v = np.asarray(dy, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    nb = len(edges) - 1
    i, j = np.triu_indices(len(x), 1)
    ddx, ddy = x[j] - x[i], y[j] - y[i]
    with np.errstate(divide="ignore"):
        lr = np.log(np.hypot(ddx, ddy))
    fin = np.isfinite(lr)
    edge_gap = np.inf
    if fin.any():
        p = np.clip(np.searchsorted(edges, lr[fin]), 1, nb)
        near = np.minimum(np.abs(lr[fin] - edges[p - 1]), np.abs(lr[fin] - edges[p]))
        edge_gap = float(near.min() / np.diff(edges).min())
    counts = np.histogram(lr[fin], bins=edges)[0].astype(np.int64)
    b = np.searchsorted(edges, lr, side="right") - 1
    b = np.where(lr == edges[-1], nb - 1, b)
    ok = fin & (lr >= edges[0]) & (lr <= edges[-1])
    i, j, b = i[ok], j[ok], b[ok]
    assert np.array_equal(np.bincount(b, minlength=nb), counts)
    X, Y = ddx[ok].astype(LD), ddy[ok].astype(LD)
    ui, vi, uj, vj = u[i].astype(LD), v[i].astype(LD), u[j].astype(LD), v[j].astype(LD)
    rsq = X * X + Y * Y
    lrl = LD(0.5) * np.log(rsq)
    zr, zi = ui * uj - vi * vj, ui * vj + vi * uj
    cr, ci = X * X - Y * Y, -2 * X * Y                                  # conj(d)^2
    mr, mi = (zr * cr - zi * ci) / rsq, (zr * ci + zi * cr) / rsq
    mz = (np.abs(ui) + np.abs(vi)) * (np.abs(uj) + np.abs(vj))
    one = np.ones(len(b), dtype=LD)
    terms = [one, lrl, ui * uj + vi * vj, zr, zi, mr, mi]
    mm = mz * (np.abs(X) + np.abs(Y)) ** 2 / rsq
    mags = [one, np.abs(lrl) + 1, np.abs(ui * uj) + np.abs(vi * vj), mz, mz, mm, mm]
    return dict(counts=counts, sums=np.stack([_binsum(b, t, nb) for t in terms]),
                mags=np.stack([_binsum(b, t, nb) for t in mags]), edge_gap=edge_gap)


def vcorr_bounds(ref):
    """(7, nbins): row 0 (counts) is zero = equality"""
    N = ref["counts"]
    m = ref["mags"]
    return np.stack([np.zeros(len(N)), bound_sum(N, m[1], 8), bound_sum(N, m[2]), bound_sum(N, m[3]), bound_sum(N, m[4]),
                     bound_sum(N, m[5], 8), bound_sum(N, m[6], 8)])


# ---- knn --------------------------------------------------------------------------------------------------------------

def ref_knn_mean(X0, y0, X, k):
    """The kernel's own arithmetic (knn.hip): d = fl(fl(dx^2) + fl(dy^2)) in fp64, stable order by (d, table row), the k
    values summed nearest first in fp64, divided by k.  Bit for bit."""
    X0 = np.asarray(X0, dtype=np.float64).reshape(len(X0), -1); X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    y0 = np.asarray(y0, dtype=np.float64)
    out = np.empty(len(X))
    for q in range(len(X)):
        dx, dy = X0[:, 0] - X[q, 0], X0[:, 1] - X[q, 1]
        d = dx * dx + dy * dy
        near = np.argsort(d, kind="stable")[:k]
        s = 0.0
        for r in near:
            s = s + y0[r]
        out[q] = s / float(k)
    return out


# ---- binned statistic: the scipy comparison of tests/test_gpu_meanify.py ------------------------------------------------

def _scipy(u, v, val, ue, ve, stat):
    from scipy.stats import binned_statistic_2d
    return binned_statistic_2d(u, v, val, bins=[ue, ve], statistic=stat)[0]


def _check(u, v, val, ue, ve, err=None):
    from treegp_amd import ops
    cnt_ref = _scipy(u, v, val, ue, ve, "count")
    avg, wrms, cnt = ops.binned_stat_2d(u, v, val, ue, ve, "mean")
    np.testing.assert_array_equal(cnt, cnt_ref)                               # bin numbers: exact
    ref = _scipy(u, v, val, ue, ve, "mean")
    np.testing.assert_array_equal(np.isnan(avg), np.isnan(ref))
    np.testing.assert_allclose(avg, ref, rtol=1e-13, atol=1e-13 * np.nanmax(np.abs(ref)), equal_nan=True)
    assert np.all(wrms == 0.0)
    med, _, cnt2 = ops.binned_stat_2d(u, v, val, ue, ve, "median")
    np.testing.assert_array_equal(cnt2, cnt_ref)
    np.testing.assert_array_equal(med, _scipy(u, v, val, ue, ve, "median"))   # order statistics: bit-exact
    if err is not None:
        w = 1.0 / err ** 2
        s_wpp = _scipy(u, v, w * val * val, ue, ve, "sum")
        s_wp = _scipy(u, v, w * val, ue, ve, "sum")
        s_w = _scipy(u, v, w, ue, ve, "sum")
        with np.errstate(invalid="ignore", divide="ignore"):
            a_ref = s_wp / s_w
            r_ref = np.sqrt((1.0 / s_w) * (s_wpp - 2.0 * a_ref * s_wp + a_ref * a_ref * s_w))
        a, r, sw = ops.binned_stat_2d(u, v, val, ue, ve, "weighted", err=err)
        np.testing.assert_allclose(sw, s_w, rtol=1e-13)
        np.testing.assert_allclose(a, a_ref, rtol=1e-12, equal_nan=True)
        ok = np.isfinite(r_ref) & (r_ref > 1e-3 * np.nanmax(r_ref))
        np.testing.assert_allclose(r[ok], r_ref[ok], rtol=1e-9)


# ---- catalogues: every input of tests/test_gpu_pair_regimes.py, checked without a GPU in test_pair_stat_refs_host.py -----

EDGE_GAP_MIN = 1e-7             # a device log / hypot may differ from NumPy's by an ulp: no pair may sit this near an edge

TWOD_NBINS = (24, 25, 31, 32)
TWOD_SEPS = ((0.0, 0.25), (1.0 / 64, 0.25), (0.0, 0.3), (1.0 / 64, 0.3))
LOG_SMALL = dict(min_sep=0.01, max_sep=0.5)
LOG_NBINS = (1, 2, 3, 4, 5)
LOG_WIDE = dict(min_sep=0.002, max_sep=1.2, nbins=256)
STRIPS = dict(min_sep=0.002, max_sep=0.05, nbins=8)
PARTIAL_N = (256, 257, 512, 700)
PARTIAL_PARTS = (1, 2, 5)
PARTIAL_TWOD = dict(min_sep=0.0, max_sep=0.3, nbins=7)
PARTIAL_LOG = dict(min_sep=0.01, max_sep=0.5, nbins=6)
BOOT_E_N = 300
BOOT_E = dict(min_sep=0.0, max_sep=0.2, nbins=9)
BOOT_E_NBOOT = (7, 8, 64, 65, 1024, 1025)
BOOT_F_N, BOOT_F_POINT = 600, 7
BOOT_F = dict(min_sep=0.0, max_sep=0.2, nbins=9)
FAR_N = 300
FAR = dict(min_sep=0.0, max_sep=0.02, nbins=5)
LINE_N = 500
LINE = dict(min_sep=0.001, max_sep=0.3, nbins=6)
VCORR_H = dict(n=700, rmin=2e-3, rmax=1.4, seed=101)
VCORR_NEDGES = (513, 512, 2)     # 512 bins (MAXBINS), 512 edges, one bin


def cat_lattice():
    """TwoD row A: 600 points on the 1/1024 lattice of the unit square plus coincident copies of the first 40, with weights.
    Differences, squares and comparisons are exact in fp64 here, and at max_sep = 0.25, nbins = 32 (pixel = 16 lattice
    steps) a share of the pairs lies exactly on a pixel edge: the dividing branch of bin_of decides them."""
    rng = np.random.default_rng(7)
    x = rng.integers(0, 1024, 600) / 1024.0
    y = rng.integers(0, 1024, 600) / 1024.0
    x, y = np.concatenate([x, x[:40]]), np.concatenate([y, y[:40]])
    k = np.sin(5.0 * x) * np.cos(3.0 * y) + 0.1 * rng.standard_normal(640)
    w = rng.uniform(0.5, 2.0, 640)
    yerr = 1.0 / np.sqrt(w)
    return x, y, k, w, yerr


def cat_uniform(n=700, seed=101):
    """rows B, D: n uniform points of the unit square, values and weights"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(size=n), rng.uniform(size=n)
    k = np.sin(4.0 * x) + np.cos(3.0 * y) * x + 0.2 * rng.standard_normal(n)
    w = rng.uniform(0.5, 2.0, n)
    return x, y, k, w


def weights_with_zeros(x, y, w):
    """only the points within 0.05 of the centre keep their weight: every pair farther apart than 0.1 has weight 0, so
    the Log bins above r = 0.1 hold pairs but no weight (xi = meanr = meanlogr = 0 there)"""
    return np.where(np.hypot(x - 0.5, y - 0.5) < 0.05, w, 0.0)


def cat_strips():
    """row C: 1500 points in six x-strips of width 0.1 with empty lanes between them, sorted by strip and inside a strip by
    y.  Strips of 256, 256, 250, 250, 250, 238 points: the first two are whole 256-point tiles, the later tiles straddle
    two strips.  Lanes are 0.075 wide: tiles two strips apart are out of reach of max_sep = 0.05."""
    rng = np.random.default_rng(11)
    sizes = (256, 256, 250, 250, 250, 238)
    xs, ys = [], []
    for s, m in enumerate(sizes):
        xs.append(0.175 * s + rng.uniform(0.0, 0.1, m))
        ys.append(np.sort(rng.uniform(0.0, 1.0, m)))
    x, y = np.concatenate(xs), np.concatenate(ys)
    k = np.cos(6.0 * x) + y + 0.1 * rng.standard_normal(len(x))
    w = rng.uniform(0.5, 2.0, len(x))
    return x, y, k, w


def tile_bbox_gaps(x, y, kt=KT):
    """gx, gy of every pair of 256-point tiles ti <= tj in caller order (kk.hip:120-126)"""
    n = len(x)
    nt = -(-n // kt)
    bb = [(x[t * kt:(t + 1) * kt].min(), x[t * kt:(t + 1) * kt].max(), y[t * kt:(t + 1) * kt].min(), y[t * kt:(t + 1) * kt].max())
          for t in range(nt)]
    out = []
    for ti in range(nt):
        for tj in range(ti, nt):
            a, b = bb[ti], bb[tj]
            out.append((ti, tj, max(0.0, b[0] - a[1], a[0] - b[1]), max(0.0, b[2] - a[3], a[2] - b[3])))
    return out


def cat_boot(n, seed=23):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(size=n), rng.uniform(size=n)
    yv = 0.3 * np.sin(5.0 * x) + 0.2 * np.cos(4.0 * y) + 0.05 * rng.standard_normal(n)
    yerr = 0.02 + 0.03 * rng.uniform(size=n)
    return x, y, yv, yerr


def idx_extreme(n=600, n_boot=9, point=7):
    """row F: the reference stream, with row 0 drawing `point` 255 times, row 1 256 times and row 2 on every draw"""
    idx = reference_stream(n, n_boot)
    for row, times in ((0, 255), (1, 256), (2, n)):
        r = idx[row]
        r[r == point] = point + 1                               # then exactly `times` draws of it
        r[:times] = point
    return idx


def cat_far(n=300):
    """row G: a 20 x 15 grid with spacing 0.05 > max_sep and jitter below 0.005: no pair within max_sep = 0.02"""
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(20), np.arange(15))
    x = 0.05 * gx.reshape(-1)[:n] + rng.uniform(0, 0.005, n)
    y = 0.05 * gy.reshape(-1)[:n] + rng.uniform(0, 0.005, n)
    yv = rng.standard_normal(n)
    yerr = 0.1 + 0.1 * rng.uniform(size=n)
    return x, y, yv, yerr


def cat_line(n=500, seed=13):
    """row G: equal x, pairwise distinct y (the Morton grid of such a catalogue has no x extent)"""
    rng = np.random.default_rng(seed)
    y = np.sort(rng.uniform(size=n))
    x = np.full(n, 0.375)
    k = np.sin(7.0 * y) + 0.1 * rng.standard_normal(n)
    w = rng.uniform(0.5, 2.0, n)
    return x, y, k, w


def log_edges(rmin, rmax, nedges):
    return np.linspace(math.log(rmin), math.log(rmax), nedges)


def cat_vcorr(n=700, seed=101):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(size=n), rng.uniform(size=n)
    dx = np.sin(3.0 * x) + 0.1 * rng.standard_normal(n)
    dy = np.cos(2.0 * y) * np.sin(x) + 0.1 * rng.standard_normal(n)
    return x, y, dx, dy


def knn_table(n0):
    """row I: the first n0 points of a 25-column integer lattice, values that differ from row to row"""
    r = np.arange(n0)
    X0 = np.stack([(r % 25).astype(np.float64), (r // 25).astype(np.float64)], axis=1)
    y0 = np.sin(0.37 * r) + 1e-3 * r
    return X0, y0


def knn_queries(n0, m):
    """m queries cycling over lattice points (a query on a table row) and cell centres (four equidistant rows)"""
    rows = -(-n0 // 25)
    q = np.arange(m)
    cx, cy = (q * 7) % 25, (q * 3) % max(rows, 1)
    centre = (q % 2 == 1)
    return np.stack([cx + 0.5 * centre, cy + 0.5 * centre], axis=1).astype(np.float64)

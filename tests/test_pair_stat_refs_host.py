"""The host references of tests/_pair_stat_refs.py, checked without a GPU: against oracle/gp_oracle.py on random catalogues,
against exact rational arithmetic at n <= 12, the bootstrap against the materialised resample, and every catalogue of
tests/test_gpu_pair_regimes.py for the property that makes it reach its branch and keeps the exact comparison fair."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pair_stat_refs as R  # noqa: E402

LD, U = R.LD, R.U


def _within(got, ref, bound, what):
    r = R.worst_ratio(got, ref, bound)
    assert r <= 1.0, "%s: error / bound = %.3g" % (what, r)


# ---- against the oracle's fp64 sums -------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,n,weighted", [(1, 400, True), (2, 613, False)])
def test_refs_agree_with_oracle_kk(seed, n, weighted):
    from oracle import gp_oracle as O
    rng = np.random.default_rng(seed)
    x, y, k = rng.uniform(size=n), rng.uniform(size=n), rng.standard_normal(n)
    w = rng.uniform(0.5, 2.0, n) if weighted else None
    ref = R.ref_kk_twod(x, y, k, w, 0.01, 0.2, 11)
    assert ref["edge_gap"] > 0.0
    xi, wt, npairs = O.kk_twod(x, y, k, w, 0.01, 0.2, 11)
    np.testing.assert_array_equal(npairs, ref["npairs"])
    b = R.kk_bounds(ref, False)
    _within(wt, ref["weight"], b["weight"], "twod weight")
    _within(xi, ref["xi"], b["xi"], "twod xi")
    ref = R.ref_kk_log(x, y, k, w, 0.01, 0.6, 13)
    assert ref["edge_gap"] > 1e-9 and ref["range_gap"] > 1e-12
    xi, wt, meanr, meanlogr, npairs = O.kk_log(x, y, k, w, 0.01, 0.6, 13)
    np.testing.assert_array_equal(npairs, ref["npairs"])
    b = R.kk_bounds(ref, True)
    _within(wt, ref["weight"], b["weight"], "log weight")
    _within(xi, ref["xi"], b["xi"], "log xi")
    _within(meanr, ref["meanr"], b["meanr"], "log meanr")
    _within(meanlogr, ref["meanlogr"], b["meanlogr"], "log meanlogr")


def test_refs_agree_with_oracle_vcorr_and_knn():
    from oracle import gp_oracle as O
    x, y, dx, dy = R.cat_vcorr(500, seed=3)
    rmin, rmax, dlogr = 0.01, 0.8, 0.2
    bins = int(np.ceil(np.log(rmax / rmin) / dlogr))
    edges = np.linspace(np.log(rmin), np.log(rmin) + bins * dlogr, bins + 1)     # what np.histogram builds for (bins, range)
    ref = R.ref_vcorr(x, y, dx, dy, edges)
    assert ref["edge_gap"] > 1e-9
    logr, xip, xim, xix, xiz2, counts = O.vcorr(x, y, dx, dy, rmin=rmin, rmax=rmax, dlogr=dlogr)
    np.testing.assert_array_equal(counts, ref["counts"])
    bnd = R.vcorr_bounds(ref)
    c = ref["counts"].astype(np.float64)
    for row, got in ((1, logr), (2, xip), (3, xiz2.real), (4, xiz2.imag), (5, xim), (6, xix)):
        mean_ref = ref["sums"][row] / c.astype(LD)
        _within(got, mean_ref, bnd[row] / c + 2 * U * np.abs(mean_ref.astype(np.float64)), "vcorr row %d" % row)
    # knn: no ties on a random table, so the oracle's argpartition picks the same neighbours; its mean is pairwise
    rng = np.random.default_rng(4)
    X0, y0, X = rng.uniform(size=(300, 2)), rng.standard_normal(300), rng.uniform(size=(50, 2))
    for k in (1, 3, 8):
        np.testing.assert_allclose(R.ref_knn_mean(X0, y0, X, k), O.knn_mean(X0, y0, X, k), rtol=4 * U * k, atol=4 * U * k)


# ---- against exact rational arithmetic ------------------------------------------------------------------------------------

def _F(a):
    return [Fraction(float(v)) for v in a]


def _close(ld, frac, scale):
    """a long-double sum of <= 132 terms against the exact value: 2^-60 of the sum of magnitudes"""
    assert abs(Fraction(float(ld)) - frac) <= Fraction(2) ** -50 * Fraction(float(scale)) + Fraction(2) ** -1000, (ld, float(frac))
    assert abs(ld - LD(frac.numerator) / LD(frac.denominator)) <= LD(2.0) ** -58 * scale + LD(2.0) ** -1000


def test_refs_agree_with_fractions():
    rng = np.random.default_rng(12)
    n = 12
    x, y, k, w = rng.uniform(size=n), rng.uniform(size=n), rng.standard_normal(n), rng.uniform(0.5, 2.0, n)
    x[5], y[5] = x[2], y[2]                                              # a coincident pair
    fx, fy, fk, fw = _F(x), _F(y), _F(k), _F(w)
    # TwoD: pixels by the fp64 rule, sums exact
    mn, mx, nb = 0.05, 0.6, 5
    bs = 2.0 * mx / nb
    cnt = np.zeros(nb * nb, dtype=np.int64); S = [Fraction(0)] * (nb * nb); W = [Fraction(0)] * (nb * nb)
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy = x[j] - x[i], y[j] - y[i]
            rsq = dx * dx + dy * dy
            if rsq == 0.0 or rsq < mn * mn or not max(abs(dx), abs(dy)) < mx:
                continue
            for sgn in (1.0, -1.0):
                ix, iy = int((sgn * dx + mx) / bs), int((sgn * dy + mx) / bs)
                if 0 <= ix < nb and 0 <= iy < nb:
                    b = iy * nb + ix
                    cnt[b] += 1; W[b] += fw[i] * fw[j]; S[b] += fw[i] * fw[j] * fk[i] * fk[j]
    ref = R.ref_kk_twod(x, y, k, w, mn, mx, nb)
    np.testing.assert_array_equal(ref["npairs"], cnt)
    assert cnt.sum() > 60
    for b in range(nb * nb):
        _close(ref["weight"][b], W[b], ref["weight"][b]); _close(ref["wkk"][b], S[b], ref["A"][b])
        if W[b]:
            _close(ref["xi"][b], S[b] / W[b], ref["A"][b] / ref["weight"][b])
    # Log: the rational sums (wkk, weight); bins by the fp64 rule
    mn, mx, nb = 0.05, 0.9, 4
    bs, lmin = np.log(mx / mn) / nb, np.log(mn)
    cnt = np.zeros(nb, dtype=np.int64); S = [Fraction(0)] * nb; W = [Fraction(0)] * nb
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy = x[j] - x[i], y[j] - y[i]
            rsq = dx * dx + dy * dy
            if rsq >= mn * mn and rsq < mx * mx:
                b = int((0.5 * np.log(rsq) - lmin) / bs)
                if 0 <= b < nb:
                    cnt[b] += 1; W[b] += fw[i] * fw[j]; S[b] += fw[i] * fw[j] * fk[i] * fk[j]
    ref = R.ref_kk_log(x, y, k, w, mn, mx, nb)
    np.testing.assert_array_equal(ref["npairs"], cnt)
    assert cnt.sum() > 40 and ref["edge_gap"] > 1e-9
    for b in range(nb):
        _close(ref["weight"][b], W[b], ref["weight"][b]); _close(ref["wkk"][b], S[b], ref["A"][b])
    # vcorr: the five rational sums, from the fp64 separations the kernel forms
    edges = np.linspace(np.log(0.05), np.log(1.2), 4)
    v = rng.standard_normal(n)
    fu, fv = fk, _F(v)
    ref = R.ref_vcorr(x, y, k, v, edges)
    acc = [[Fraction(0)] * 3 for _ in range(5)]
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy = x[j] - x[i], y[j] - y[i]
            if dx == 0.0 and dy == 0.0:
                continue
            lr = np.log(np.hypot(dx, dy))
            if not (edges[0] <= lr <= edges[-1]):
                continue
            b = min(int(np.searchsorted(edges, lr, side="right")) - 1, 2)
            X, Y = Fraction(float(dx)), Fraction(float(dy))
            zr, zi = fu[i] * fu[j] - fv[i] * fv[j], fu[i] * fv[j] + fv[i] * fu[j]
            cr, ci, rsq = X * X - Y * Y, -2 * X * Y, X * X + Y * Y
            for row, t in enumerate((fu[i] * fu[j] + fv[i] * fv[j], zr, zi, (zr * cr - zi * ci) / rsq, (zr * ci + zi * cr) / rsq)):
                acc[row][b] += t
    assert ref["counts"].sum() > 40
    for row, srow in enumerate((2, 3, 4, 5, 6)):
        for b in range(3):
            _close(ref["sums"][srow][b], acc[row][b], ref["mags"][srow][b])
    # bootstrap: xi of every resample exactly
    yv, yerr = rng.standard_normal(n) + 3.0, rng.uniform(0.1, 0.3, n)
    idx = rng.integers(0, n, size=(3, n))
    mn, mx, nb = 0.0, 0.6, 3
    ref = R.ref_kk_bootstrap(x, y, yv, yerr, idx, mn, mx, nb)
    d = R.twod_deposits(x, y, mn, mx, nb)
    fy_, fw_ = _F(yv), [1 / (Fraction(float(e)) ** 2) for e in yerr]
    for r in range(3):
        c = np.bincount(idx[r], minlength=n)
        mu = sum(fy_[p] for p in idx[r]) / n
        S = [Fraction(0)] * (nb * nb); T = [Fraction(0)] * (nb * nb)
        for i, j, b in zip(d["i"], d["j"], d["b"]):
            t = int(c[i]) * int(c[j]) * fw_[i] * fw_[j]
            T[b] += t; S[b] += t * (fy_[i] - mu) * (fy_[j] - mu)
        for b in range(nb * nb):
            exact = S[b] / T[b] if T[b] else Fraction(0)
            assert abs(ref["xi"][r, b] - LD(exact.numerator) / LD(exact.denominator)) <= LD(2.0) ** -50 * (abs(ref["xi"][r, b]) + 1)
            assert abs(Fraction(float(ref["xi"][r, b])) - exact) <= ref["bound"][r, b] + Fraction(2) ** -1000


def test_bootstrap_ref_equals_twod_ref_of_materialised_resample():
    n = 200
    x, y, yv, yerr = R.cat_boot(n, seed=31)
    idx = R.reference_stream(n, 4)
    ref = R.ref_kk_bootstrap(x, y, yv, yerr, idx, 0.0, 0.25, 7)
    for weighted in (True, False):
        e = yerr if weighted else np.zeros(n)
        ref = R.ref_kk_bootstrap(x, y, yv, e, idx, 0.0, 0.25, 7)
        for r in range(4):
            s = idx[r]
            kb = yv[s] - yv[s].mean()
            direct = R.ref_kk_twod(x[s], y[s], kb, 1.0 / yerr[s] ** 2 if weighted else None, 0.0, 0.25, 7)
            assert np.count_nonzero(direct["weight"]) > 20
            _within(ref["xi"][r], direct["xi"], ref["bound"][r], "resample %d" % r)
            np.testing.assert_array_equal(ref["xi"][r] == 0, direct["weight"] == 0)


def test_knn_ref_tie_rule():
    """four equidistant rows around a cell centre: the earlier table rows win, nearest first"""
    X0 = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [5.0, 5.0]])
    y0 = np.array([1.0, 10.0, 100.0, 1000.0, 7.0])
    q = np.array([[0.5, 0.5]])
    assert R.ref_knn_mean(X0, y0, q, 1)[0] == 1.0
    assert R.ref_knn_mean(X0, y0, q, 2)[0] == 5.5
    assert R.ref_knn_mean(X0, y0, q, 3)[0] == 37.0
    assert R.ref_knn_mean(X0, y0, q, 5)[0] == (((1.0 + 10.0) + 100.0) + 1000.0 + 7.0) / 5.0
    X0, y0 = R.knn_table(600)
    Q = R.knn_queries(600, 257)
    d = ((X0[None] - Q[:, None]) ** 2).sum(-1)
    d.sort(axis=1)
    assert np.count_nonzero(d[1::2, 0] == d[1::2, 3]) > 100            # cell centres: four rows tie for nearest
    assert np.count_nonzero(d[0::2, 0] == 0.0) > 100                    # queries on a table row
    assert len(np.unique(y0)) == 600


# ---- the catalogues of the GPU file -----------------------------------------------------------------------------------------

def test_catalogue_lattice_twod():
    x, y, k, w, yerr = R.cat_lattice()
    assert len(x) == 640 and np.array_equal(x * 1024, np.rint(x * 1024)) and np.array_equal(y * 1024, np.rint(y * 1024))
    for nb in R.TWOD_NBINS:
        for mn, mx in R.TWOD_SEPS:
            ref = R.ref_kk_twod(x, y, k, w, mn, mx, nb)
            assert ref["naccepted"] > 30000 and np.count_nonzero(ref["npairs"]) > 0.95 * nb * nb
            if nb == 32 and mx == 0.25:
                assert ref["on_edge"] > 0.05 * 2 * ref["naccepted"]          # the dividing branch of bin_of decides these
            if nb in (25, 31):
                assert ref["on_edge"] == 0 and ref["edge_gap"] >= R.EDGE_GAP_MIN
    # LDS need of the four per-wave histograms (kk.hip:448): above 64 KB from nbins = 25
    assert 4 * 3 * 24 * 24 * 8 + 8192 <= 65536 < 4 * 3 * 25 * 25 * 8 + 8192 and 4 * 3 * 32 * 32 * 8 + 8192 == 106496


def test_catalogue_log_edge_gaps():
    x, y, k, w = R.cat_uniform()
    for nb in R.LOG_NBINS:
        ref = R.ref_kk_log(x, y, k, w, nbins=nb, **R.LOG_SMALL)
        assert ref["edge_gap"] >= R.EDGE_GAP_MIN and ref["range_gap"] >= R.EDGE_GAP_MIN
        assert ref["npairs"].min() >= 296
    ref = R.ref_kk_log(x, y, k, w, **R.LOG_WIDE)
    assert ref["edge_gap"] >= R.EDGE_GAP_MIN and ref["range_gap"] >= R.EDGE_GAP_MIN
    assert np.count_nonzero(ref["npairs"] == 0) == 30                     # empty bins must come back as 0
    wz = R.weights_with_zeros(x, y, w)
    assert 2 <= np.count_nonzero(wz) < len(wz)
    for nb in (3, 4, 5):
        ref = R.ref_kk_log(x, y, k, wz, nbins=nb, **R.LOG_SMALL)
        assert np.any((ref["npairs"] > 0) & (ref["weight"] == 0)) and np.any(ref["weight"] > 0)


def test_catalogue_strips_is_culled():
    x, y, k, w = R.cat_strips()
    assert len(x) == 1500
    ref = R.ref_kk_log(x, y, k, w, **R.STRIPS)
    assert ref["edge_gap"] >= R.EDGE_GAP_MIN and ref["range_gap"] >= R.EDGE_GAP_MIN and ref["npairs"].min() > 0
    gaps = R.tile_bbox_gaps(x, y)
    assert len(gaps) == 21                                                # diagonal tile pairs included
    mx = R.STRIPS["max_sep"]
    culled = [g for g in gaps if g[2] * g[2] + g[3] * g[3] >= mx * mx]
    assert 2 * len(culled) >= len(gaps)
    assert all(max(g[2], g[3]) >= mx for g in culled)                     # here also "bounding-box gap >= max_sep"
    # and pairs in range do cross tiles that are NOT culled
    i, j = np.triu_indices(1500, 1)
    near = np.hypot(x[j] - x[i], y[j] - y[i]) < mx
    assert np.count_nonzero(near & (i // 256 != j // 256)) > 100


def test_catalogue_partial():
    for n in R.PARTIAL_N:
        x, y, k, w = R.cat_uniform(n, seed=200 + n)
        ref = R.ref_kk_log(x, y, k, w, **R.PARTIAL_LOG)
        assert ref["edge_gap"] >= R.EDGE_GAP_MIN and ref["range_gap"] >= R.EDGE_GAP_MIN and ref["npairs"].min() > 0
        ref = R.ref_kk_twod(x, y, k, w, **R.PARTIAL_TWOD)
        assert ref["edge_gap"] >= R.EDGE_GAP_MIN and ref["npairs"].min() > 0
    assert -(-256 // 256) == 1 and -(-257 // 256) == 2                   # nparts = 5 leaves parts without a tile at both


def test_catalogue_bootstrap_rows():
    p, n, pt = R.BOOT_F, R.BOOT_F_N, R.BOOT_F_POINT
    idx = R.idx_extreme(n, 9, pt)
    c = np.stack([np.bincount(r, minlength=n) for r in idx])
    assert [int(c[r, pt]) for r in range(3)] == [255, 256, 600]
    assert c[0].max() == 255 and c[1].max() == 256
    assert np.count_nonzero(c[2]) == 1                                    # one distinct point: no pair
    assert c[3:].max() < 20 and c[:, :].sum(axis=1).tolist() == [600] * 9
    assert idx.min() >= 0 and idx.max() < n
    x, y, yv, yerr = R.cat_boot(n)
    d = R.twod_deposits(x, y, **p)
    assert d["edge_gap"] >= R.EDGE_GAP_MIN
    assert np.count_nonzero((d["i"] == pt) | (d["j"] == pt)) > 50         # the extreme point has partners in range
    x, y, yv, yerr = R.cat_boot(R.BOOT_E_N)
    d = R.twod_deposits(x, y, **R.BOOT_E)
    assert d["edge_gap"] >= R.EDGE_GAP_MIN and np.bincount(d["b"], minlength=81).min() > 0
    assert R.reference_stream(300, 3).max() <= 298                        # the stream never draws the last point


def test_catalogue_far_and_line():
    f = R.FAR
    x, y, yv, yerr = R.cat_far(R.FAR_N)
    i, j = np.triu_indices(R.FAR_N, 1)
    assert np.maximum(np.abs(x[j] - x[i]), np.abs(y[j] - y[i])).min() > 2 * f["max_sep"]       # no pair in range
    assert R.twod_deposits(x, y, **f)["naccepted"] == 0
    ln = R.LINE
    x, y, k, w = R.cat_line(R.LINE_N)
    assert np.all(x == x[0]) and len(np.unique(y)) == R.LINE_N
    ref = R.ref_kk_log(x, y, k, w, **ln)
    assert ref["edge_gap"] >= R.EDGE_GAP_MIN and ref["range_gap"] >= R.EDGE_GAP_MIN and ref["npairs"].min() > 0
    ref = R.ref_kk_twod(x, y, k, w, **ln)
    assert ref["naccepted"] > 1000                                       # dx = 0 sits on a pixel edge for even nbins: exact in fp64
    dxv, dyv = np.cos(y), np.sin(3 * y)
    for nedges in (2, 40):
        ref = R.ref_vcorr(x, y, dxv, dyv, R.log_edges(1e-3, 0.9, nedges))
        assert ref["edge_gap"] >= R.EDGE_GAP_MIN and ref["counts"].min() > 0


def test_catalogue_vcorr_limits():
    h = R.VCORR_H
    x, y, dx, dy = R.cat_vcorr(h["n"], h["seed"])
    for nedges in R.VCORR_NEDGES:
        ref = R.ref_vcorr(x, y, dx, dy, R.log_edges(h["rmin"], h["rmax"], nedges))
        assert ref["edge_gap"] >= R.EDGE_GAP_MIN
        assert ref["counts"].sum() > 200000
    # 127 KB of dynamic LDS at 512 bins (vcorr.hip:124)
    assert (4 * 256 + 513 + 4 * 7 * 512) * 8 == 126984

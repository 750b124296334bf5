"""Every schedule branch of the pair-statistics seam (kk.hip, kk_boot.hip, vcorr.hip, knn.hip, binstat.hip) on the GPU against
the exact host references of tests/_pair_stat_refs.py: the sizes at which each kernel changes path or reaches a limit, not
the sizes of the workload.  Counts are compared for equality, values against the error bounds derived in that module's
docstring (u = 2^-53, no tolerance picked by hand); the catalogues and the properties that make them reach their branch are
checked without a GPU in tests/test_pair_stat_refs_host.py.  Every comparison prints its error / bound ratio (pytest -s);
the largest seen per route are in LAB_NOTES.md, "Pair statistics: regimes"."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pair_stat_refs as R  # noqa: E402

U = R.U


def _hold(route, got, ref, bound):
    r = R.worst_ratio(got, ref, bound)
    print("MARGIN %-28s %.3g" % (route, r))
    assert r <= 1.0, "%s: error / bound = %.3g" % (route, r)


def _equal(got, ref, what):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(ref).astype(np.float64), err_msg=what)


def _hold_twod(route, out, ref):
    xi, wt, npairs = out
    _equal(npairs, ref["npairs"], route + " npairs")
    b = R.kk_bounds(ref, False)
    _hold(route + " weight", wt, ref["weight"], b["weight"])
    _hold(route + " xi", xi, ref["xi"], b["xi"])
    assert np.all(xi[np.asarray(ref["weight"] == 0)] == 0.0)


def _hold_log(route, out, ref):
    xi, wt, meanr, meanlogr, npairs = out
    _equal(npairs, ref["npairs"], route + " npairs")
    b = R.kk_bounds(ref, True)
    _hold(route + " weight", wt, ref["weight"], b["weight"])
    _hold(route + " xi", xi, ref["xi"], b["xi"])
    _hold(route + " meanr", meanr, ref["meanr"], b["meanr"])
    _hold(route + " meanlogr", meanlogr, ref["meanlogr"], b["meanlogr"])
    z = np.asarray(ref["weight"] == 0)
    assert np.all(xi[z] == 0.0) and np.all(meanr[z] == 0.0) and np.all(meanlogr[z] == 0.0) and np.all(wt[z] == 0.0)


def _boot(x, y, yv, yerr, idx, par, lists, monkeypatch):
    """tgp_kk_twod_bootstrap with the pair lists allowed (they still fall back where they do not apply) or switched off"""
    from treegp_amd import ops
    if lists:
        monkeypatch.delenv("TGP_BOOT_LISTS", raising=False)
    else:
        monkeypatch.setenv("TGP_BOOT_LISTS", "0")
    try:
        return ops.kk_twod_bootstrap(x, y, yv, yerr, idx, par["min_sep"], par["max_sep"], par["nbins"])
    finally:
        monkeypatch.delenv("TGP_BOOT_LISTS", raising=False)


# ---- A: TwoD above 64 KB of LDS -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ref_lattice(mn, mx, nb):
    x, y, k, w, yerr = R.cat_lattice()
    return R.ref_kk_twod(x, y, k, w, mn, mx, nb)


@pytest.mark.parametrize("nbins", R.TWOD_NBINS)
@pytest.mark.parametrize("mn,mx", R.TWOD_SEPS)
def test_a_twod_large_grids(nbins, mn, mx):
    """24 is the last grid whose four per-wave histograms fit 64 KB; 25, 31, 32 need the raised dynamic-LDS limit (106 496 B
    at 32).  Lattice catalogue with coincident points: on even grids a share of the pairs sits exactly on a pixel edge."""
    from treegp_amd import ops
    x, y, k, w, yerr = R.cat_lattice()
    ref = _ref_lattice(mn, mx, nbins)
    out = ops.kk_twod(x, y, k, w, mn, mx, nbins)
    _hold_twod("A twod", out, ref)
    if ref["on_edge"] == 0:
        # a pair off the pixel edges deposits into a pixel and its mirror image: the grid is point symmetric, bit for bit
        g = out[2].reshape(nbins, nbins)
        np.testing.assert_array_equal(g, g[::-1, ::-1])
    xi_u, wt_u, np_u = ops.kk_twod(x, y, k, None, mn, mx, nbins)
    _equal(np_u, ref["npairs"], "unweighted npairs")
    _equal(wt_u, ref["npairs"], "unweighted weight")                       # sums of ones: exact


@pytest.mark.parametrize("n_boot", [9, 5])
def test_a_bootstrap_at_32_bins(n_boot, monkeypatch):
    """1024 pixels: the largest pair-list tables (9 resamples) and the per-resample kernel at 106 496 B of LDS (5)"""
    x, y, k, w, yerr = R.cat_lattice()
    yv = k + 0.5
    idx = R.reference_stream(len(x), n_boot)
    par = dict(min_sep=0.0, max_sep=0.25, nbins=32)
    ref = R.ref_kk_bootstrap(x, y, yv, yerr, idx, **par)
    got = _boot(x, y, yv, yerr, idx, par, True, monkeypatch)
    assert np.count_nonzero(ref["xi"]) > 0.9 * ref["xi"].size
    _hold("A boot32 n_boot=%d" % n_boot, got, ref["xi"], ref["bound"])


# ---- B, C: Log ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ref_log(nbins, wkind):
    x, y, k, w = R.cat_uniform()
    wv = {"none": None, "w": w, "zeros": R.weights_with_zeros(x, y, w)}[wkind]
    par = dict(R.LOG_WIDE) if nbins == 256 else dict(nbins=nbins, **R.LOG_SMALL)
    return wv, par, R.ref_kk_log(x, y, k, wv, **par)


@pytest.mark.parametrize("wkind", ["none", "w", "zeros"])
@pytest.mark.parametrize("nbins", R.LOG_NBINS + (256,))
def test_b_log_register_bins(nbins, wkind):
    """1, 2, 3 bins: fewer than the four register accumulators (topbase < 0); 4: every bin in registers; 5: the first LDS
    bin; 256: the limit, with empty bins.  `zeros`: bins that hold pairs but no weight come back as 0."""
    from treegp_amd import ops
    x, y, k, w = R.cat_uniform()
    wv, par, ref = _ref_log(nbins, wkind)
    out = ops.kk_log(x, y, k, wv, par["min_sep"], par["max_sep"], par["nbins"])
    _hold_log("B log", out, ref)
    if nbins == 256:
        assert np.count_nonzero(ref["npairs"] == 0) == 30 and np.all(out[4][ref["npairs"] == 0] == 0.0)


def test_c_log_culls_tiles_of_a_sorted_catalogue():
    from treegp_amd import ops
    x, y, k, w = R.cat_strips()
    ref = R.ref_kk_log(x, y, k, w, **R.STRIPS)
    out = ops.kk_log(x, y, k, w, R.STRIPS["min_sep"], R.STRIPS["max_sep"], R.STRIPS["nbins"])
    _hold_log("C log strips", out, ref)


# ---- D: shards ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bin_type", [0, 1])
@pytest.mark.parametrize("n", R.PARTIAL_N)
def test_d_partial_shards_add_up(n, bin_type):
    from treegp_amd import ops
    x, y, k, w = R.cat_uniform(n, seed=200 + n)
    par = R.PARTIAL_TWOD if bin_type == 0 else R.PARTIAL_LOG
    ref = (R.ref_kk_twod if bin_type == 0 else R.ref_kk_log)(x, y, k, w, **par)
    refs, bnds = R.kk_raw(ref, bin_type == 1)
    ntile = -(-n // R.KT)
    for nparts in R.PARTIAL_PARTS:
        parts = [ops.kk_partial(bin_type, x, y, k, w, par["min_sep"], par["max_sep"], par["nbins"], p, nparts)
                 for p in range(nparts)]
        total = np.sum(np.stack(parts).astype(R.LD), axis=0)
        _equal(total[-1], refs[-1], "counts")
        for row, name in enumerate(("wkk", "w", "wr", "wlogr")[:len(refs) - 1]):
            _hold("D partial %s %s" % ("log" if bin_type else "twod", name), total[row], refs[row], bnds[row])
        for p in range(ntile, nparts):
            assert not parts[p].any()                                      # a shard without a tile: nothing launched, zeros


# ---- E: the switch between the bootstrap's two device paths ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ref_boot_e(n_boot, shift):
    x, y, yv, yerr = R.cat_boot(R.BOOT_E_N)
    idx = R.reference_stream(R.BOOT_E_N, n_boot)
    return idx, R.ref_kk_bootstrap(x, y, yv + shift, yerr, idx, **R.BOOT_E)


@pytest.mark.parametrize("shift", [0.0, 250.0])
@pytest.mark.parametrize("n_boot", R.BOOT_E_NBOOT)
def test_e_bootstrap_path_switch(n_boot, shift, monkeypatch):
    """7 / 8: per-resample kernels vs pair lists; 64 / 65: one or two 64-wide column blocks of the multiplicity matrix;
    1024: a 1024-thread moments kernel; 1025: back on the per-resample kernels with grid.z = 1025."""
    x, y, yv, yerr = R.cat_boot(R.BOOT_E_N)
    idx, ref = _ref_boot_e(n_boot, shift)
    a = _boot(x, y, yv + shift, yerr, idx, R.BOOT_E, True, monkeypatch)
    b = _boot(x, y, yv + shift, yerr, idx, R.BOOT_E, False, monkeypatch)
    tag = "n_boot=%d shift=%g" % (n_boot, shift)
    _hold("E boot default " + tag, a, ref["xi"], ref["bound"])
    _hold("E boot per-resample " + tag, b, ref["xi"], ref["bound"])
    _hold("E boot path-vs-path " + tag, a, b, 2.0 * ref["bound"])


# ---- F: byte multiplicities -------------------------------------------------------------------------------------------------

def test_f_bootstrap_extreme_multiplicities(monkeypatch):
    """a point drawn 255 times (fits a byte), 256 times (the lists give up; the per-resample path splits it into entries of
    255 + 1) and 600 times (three entries of one point, whose mutual pairs have r = 0)"""
    n, pt = R.BOOT_F_N, R.BOOT_F_POINT
    x, y, yv, yerr = R.cat_boot(n)
    idx = R.idx_extreme(n, 9, pt)
    ref = R.ref_kk_bootstrap(x, y, yv, yerr, idx, **R.BOOT_F)
    assert not ref["xi"][2].any() and np.count_nonzero(ref["xi"][0]) > 40 and np.count_nonzero(ref["xi"][1]) > 40
    got = _boot(x, y, yv, yerr, idx, R.BOOT_F, True, monkeypatch)          # row 1, 2 overflow a byte: per-resample path
    _hold("F boot block", got, ref["xi"], ref["bound"])
    assert not got[2].any()
    for r in range(3):                                                     # alone: n_boot = 1 < 8, per-resample path
        one = _boot(x, y, yv, yerr, idx[r:r + 1], R.BOOT_F, True, monkeypatch)
        _hold("F boot row %d alone" % r, one, ref["xi"][r:r + 1], ref["bound"][r:r + 1])
    mild = idx.copy()
    mild[1:3] = R.reference_stream(n, 11)[9:11]                            # only row 0 is extreme: stays on the lists
    ref_m = R.ref_kk_bootstrap(x, y, yv, yerr, mild, **R.BOOT_F)
    a = _boot(x, y, yv, yerr, mild, R.BOOT_F, True, monkeypatch)
    b = _boot(x, y, yv, yerr, mild, R.BOOT_F, False, monkeypatch)
    _hold("F boot lists c=255", a, ref_m["xi"], ref_m["bound"])
    _hold("F boot per-resample c=255", b, ref_m["xi"], ref_m["bound"])
    _hold("F boot path-vs-path c=255", a, b, 2.0 * ref_m["bound"])


# ---- G: nothing in range; a catalogue on one line ---------------------------------------------------------------------------

def test_g_no_pair_in_range(monkeypatch):
    from treegp_amd import ops
    x, y, yv, yerr = R.cat_far(R.FAR_N)
    idx = R.reference_stream(R.FAR_N, 9)
    for lists in (True, False):
        got = _boot(x, y, yv, yerr, idx, R.FAR, lists, monkeypatch)
        assert got.shape == (9, 25) and not got.any()
    xi, wt, npairs = ops.kk_twod(x, y, yv, 1.0 / yerr ** 2, R.FAR["min_sep"], R.FAR["max_sep"], R.FAR["nbins"])
    assert not xi.any() and not wt.any() and not npairs.any()


def test_g_catalogue_on_a_line(monkeypatch):
    from treegp_amd import ops
    x, y, k, w = R.cat_line(R.LINE_N)
    ln = R.LINE
    _hold_twod("G line twod", ops.kk_twod(x, y, k, w, ln["min_sep"], ln["max_sep"], ln["nbins"]), R.ref_kk_twod(x, y, k, w, **ln))
    _hold_log("G line log", ops.kk_log(x, y, k, w, ln["min_sep"], ln["max_sep"], ln["nbins"]), R.ref_kk_log(x, y, k, w, **ln))
    yerr = 1.0 / np.sqrt(w)
    idx = R.reference_stream(R.LINE_N, 9)
    ref = R.ref_kk_bootstrap(x, y, k, yerr, idx, **ln)
    for lists in (True, False):
        got = _boot(x, y, k, yerr, idx, ln, lists, monkeypatch)
        _hold("G line boot lists=%d" % lists, got, ref["xi"], ref["bound"])
    dxv, dyv = np.cos(y), np.sin(3 * y)
    for nedges in (2, 40):
        edges = R.log_edges(1e-3, 0.9, nedges)
        _hold_vcorr("G line vcorr", ops.vcorr_sums(x, y, dxv, dyv, edges), R.ref_vcorr(x, y, dxv, dyv, edges))


# ---- H: vcorr at its LDS limit ------------------------------------------------------------------------------------------------

def _hold_vcorr(route, acc, ref):
    _equal(acc[0], ref["counts"], route + " counts")
    bnd = R.vcorr_bounds(ref)
    for row, name in ((1, "logr"), (2, "plus"), (3, "z2re"), (4, "z2im"), (5, "minus"), (6, "cross")):
        _hold("%s %s" % (route, name), acc[row], ref["sums"][row], bnd[row])


@pytest.mark.parametrize("nedges", R.VCORR_NEDGES)
def test_h_vcorr_bin_limits(nedges):
    """513 edges = 512 bins (MAXBINS, 126 984 B of dynamic LDS), 512 edges, and a single bin"""
    from treegp_amd import ops
    h = R.VCORR_H
    x, y, dx, dy = R.cat_vcorr(h["n"], h["seed"])
    edges = R.log_edges(h["rmin"], h["rmax"], nedges)
    _hold_vcorr("H vcorr", ops.vcorr_sums(x, y, dx, dy, edges), R.ref_vcorr(x, y, dx, dy, edges))


# ---- I: nearest neighbours with real ties -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 16])
def test_i_knn_ties_and_tile_edges(k):
    """integer lattice table: distances are exact and ties real (a cell centre has four equidistant rows with different
    values).  n0 = k (every row is a neighbour), 255 / 256 / 257 (the 256-row tile edge), 600; m = 1, 256, 257."""
    from treegp_amd import ops
    for n0 in sorted({k, 255, 256, 257, 600}):
        X0, y0 = R.knn_table(n0)
        for m in (1, 256, 257):
            X = R.knn_queries(n0, m)
            np.testing.assert_array_equal(ops.knn_mean(X0, y0, X, k), R.ref_knn_mean(X0, y0, X, k),
                                          err_msg="n0=%d m=%d k=%d" % (n0, m, k))


def test_i_knn_random_table():
    from treegp_amd import ops
    rng = np.random.default_rng(9)
    X0, y0, X = rng.uniform(size=(777, 2)), rng.standard_normal(777), rng.uniform(size=(300, 2))
    for k in (3, 5, 6):
        np.testing.assert_allclose(ops.knn_mean(X0, y0, X, k), R.ref_knn_mean(X0, y0, X, k), rtol=4 * U, atol=0)


# ---- J: binned statistic, the instantiations that never ran ----------------------------------------------------------------------

def _edge_points(u, v, ue, ve):
    """points on the first, inner and last edges, just past the last edge, and a NaN (as the existing edge test places them)"""
    u[:9] = ue[[0, 1, 2, 100, 4000, len(ue) - 3, len(ue) - 2, len(ue) - 1, len(ue) - 1]]; v[:9] = 0.5 * (ve[0] + ve[-1])
    u[9:11] = ue[77]; v[9:11] = ve[[0, -1]]
    u[11] = ue[-1]; v[11] = ve[-1]
    u[12] = np.nextafter(ue[-1], np.inf); v[12] = ve[0]
    u[13] = ue[5]; v[13] = np.nan


def test_j_binned_stat_more_edges_than_lds_holds():
    """8200 + 2 edges > 8192: the edge arrays stay in global memory.  n = 270 000: the median's count pass has its histogram in
    LDS (<false, true>), mean and weighted use global atomics (<false, false>); n = 20 000: <false, false> throughout."""
    rng = np.random.default_rng(21)
    ue, ve = np.linspace(0.0, 1.0, 8200), np.array([0.0, 1.0])
    for n in (270000, 20000):
        u, v = rng.uniform(-0.01, 1.01, n), rng.uniform(-0.01, 1.01, n)
        _edge_points(u, v, ue, ve)
        val = 1.0 + 0.1 * rng.standard_normal(n)                          # no bin mean cancels: the comparison is relative
        val[100:140] = 1.25                                                # ties around a median
        R._check(u, v, val, ue, ve, err=0.5 + rng.uniform(size=n))


def test_j_binned_stat_largest_lds_footprint():
    """4097 + 2 edges and 3 x 4096 weighted accumulators: <true, true> at 131 096 B of dynamic LDS"""
    rng = np.random.default_rng(22)
    n = 400000
    ue, ve = np.linspace(0.0, 1.0, 4097), np.array([0.0, 1.0])
    u, v = rng.uniform(-0.01, 1.01, n), rng.uniform(-0.01, 1.01, n)
    _edge_points(u, v, ue, ve)
    assert 3 * 4096 <= 12288 and n >= 32 * 3 * 4096 and (4099 + 12288) * 8 == 131096
    R._check(u, v, 1.0 + 0.1 * rng.standard_normal(n), ue, ve, err=0.5 + rng.uniform(size=n))


# ---- limits are rejected, not run -----------------------------------------------------------------------------------------------

def test_limits_are_rejected_before_anything_is_launched():
    from treegp_amd import ops
    from treegp_amd._lib import TgpError
    x, y, k, w = R.cat_uniform(257, seed=457)
    X0, y0 = R.knn_table(8)
    Xq = R.knn_queries(8, 5)
    idx = R.reference_stream(257, 9)
    bad = idx.copy()
    bad[8, 256] = 257
    calls = [
        lambda: ops.kk_twod(x, y, k, w, 0.0, 0.3, 33),
        lambda: ops.kk_log(x, y, k, w, 0.01, 0.5, 257),
        lambda: ops.vcorr_sums(x, y, k, w, R.log_edges(2e-3, 1.4, 514)),
        lambda: ops.knn_mean(X0, y0, Xq, 9),
        lambda: ops.knn_mean(X0[:3], y0[:3], Xq, 4),
        lambda: ops.kk_partial(0, x, y, k, w, 0.0, 0.3, 7, 2, 2),
        lambda: ops.kk_partial(1, x, y, k, w, 0.01, 0.5, 6, 5, 5),
        lambda: ops.kk_twod_bootstrap(x, y, k, 1.0 / np.sqrt(w), bad, 0.0, 0.3, 7),
    ]
    ref_t = R.ref_kk_twod(x, y, k, w, **R.PARTIAL_TWOD)
    ref_l = R.ref_kk_log(x, y, k, w, **R.PARTIAL_LOG)
    for n, call in enumerate(calls):
        with pytest.raises(TgpError) as e:
            call()
        assert e.value.rc == -1                                           # a bad argument, not a failed HIP call
        # the next valid call on the same context gives the reference's numbers
        if n % 2:
            _hold_twod("after rejection twod", ops.kk_twod(x, y, k, w, 0.0, 0.3, 7), ref_t)
        else:
            _hold_log("after rejection log", ops.kk_log(x, y, k, w, 0.01, 0.5, 6), ref_l)
    yerr = 1.0 / np.sqrt(w)
    ref_b = R.ref_kk_bootstrap(x, y, k, yerr, idx, 0.0, 0.3, 7)
    _hold("after rejection boot", ops.kk_twod_bootstrap(x, y, k, yerr, idx, 0.0, 0.3, 7), ref_b["xi"], ref_b["bound"])
    np.testing.assert_array_equal(ops.knn_mean(X0, y0, Xq, 4), R.ref_knn_mean(X0, y0, Xq, 4))

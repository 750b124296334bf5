"""Every covariance value the device computes, pair by pair, against mpmath.

Four pieces of arithmetic produce amp k(x, x') on the device (the packed K build, the dense kernel matrix, the fused
Gaussian predict with its 2^(j/256) table, the von Karman predict with its LDS Chebyshev table); the rest of the suite
sees them only through sums.  Here a one-hot alpha turns the fused predict into the kernel function itself, and every
route is compared with a 40-digit reference at the places where such arithmetic goes wrong: every table entry, the
subnormal range and the flush to zero, every branch of the Bessel function, the fall-backs of the launcher, NaN, and
coordinates far from the origin.  Point sets, references, bounds and the device drivers live in _kernel_value_helpers.py,
which also runs as a script so that the process-wide switches of the fused predict get a process each.

The host tests (no gpu marker) pin the reference to the reference project's kernel tables and check, from the reference
alone, that the inputs reach what the GPU tests claim to cover.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kernel_value_helpers as H  # noqa: E402

LD = H.LD


def show(x):
    return json.dumps(x, indent=1, sort_keys=True)


# ---- host: the reference and the inputs ----------------------------------------------------------------------------
def test_mpmath_reference_reproduces_reference_kernel_tables(golden):
    """the mpmath formulas are the reference project's kernels: its recorded tables, at the tolerance test_oracle_golden
    holds the oracle to (rtol 2e-12, atol 1e-14)"""
    g = golden("g4_kernels.npz")
    X, Y = g["X"], g["Y"]
    ia, iv = g["arbf_invLam"], g["avk_invLam"]
    rows = np.arange(0, len(Y), 7)         # a subset of the cross tables' rows keeps mpmath's Bessel function to seconds
    cases = {
        "rbf": lambda Q, x: H.gauss_ref(Q, x, 1 / 0.45 ** 2, 0.0, 1 / 0.45 ** 2, 4.0)[0],
        "arbf": lambda Q, x: H.gauss_ref(Q, x, ia[0, 0], ia[0, 1], ia[1, 1], 0.25)[0],
        "vk": lambda Q, x: H.vk_ref_offaxis(Q, x, "vk", 2.25, ell=3.0)[0],
        "avk": lambda Q, x: H.vk_ref_offaxis(Q, x, "avk", 0.7 ** 2, a=iv[0, 0], b=iv[0, 1], c=iv[1, 1])[0],
        "vk_noamp": lambda Q, x: H.vk_ref_offaxis(Q, x, "vk", 1.0, ell=0.02)[0],
    }
    for tag, f in cases.items():
        for j in range(0, len(X), 5):
            np.testing.assert_allclose(f(Y[rows], X[j]).astype(float), g[tag + "_cross"][rows, j], rtol=2e-12, atol=1e-14,
                                       err_msg="%s cross, column %d" % (tag, j))
        for j in range(0, len(X), 11):
            np.testing.assert_allclose(f(X, X[j]).astype(float), g[tag + "_self"][:, j], rtol=2e-12, atol=1e-14,
                                       err_msg="%s self, column %d" % (tag, j))


def test_gaussian_sweep_inputs_cover_table_and_tiny_range():
    """from the reference alone: every entry of the 256-entry table is read (so every 32- and 64-entry one) by a pair
    with a normal result, and the normal, subnormal and flushed ranges hold at least 100 points each"""
    a, b, c = H.README_INVLAM
    Xq = H.gauss_sweep_queries()
    ref, s = H.gauss_ref(Xq, H.GAUSS_XT, a, b, c, 1.0)
    cond = H.gauss_input_conditions(ref, s)
    print(show(cond))
    assert len(Xq) == H.GAUSS_M + H.GAUSS_BAND and np.array_equal(Xq[0], H.GAUSS_XT) and ref[0] == 1
    assert cond["residues"] == 256, cond
    assert cond["normal"] >= 100 and cond["subnormal"] >= 100 and cond["zero"] >= 100, cond
    assert cond["max_s"] > 1600, cond


def test_von_karman_sweep_inputs_cover_every_branch():
    """the series branch and each of the six Chebyshev segments of bessel_k56.h hold at least 200 points"""
    u = H.vk_onaxis_u()
    x = np.array([float(2 * H.mp.pi * H.mp.mpf(v)) for v in u.tolist()])
    seg = H.vk_segment_counts(x)
    print(show(seg))
    assert set(seg) == set(H.VK_SEGMENTS)
    assert all(v >= 200 for v in seg.values()), seg
    assert u[0] == 0.0 and (x > H.K56_XMAX).sum() >= 3       # 111.08, 200 and the neighbour above the cut at least
    assert np.array_equal((u / 2) * 2, u)                  # the device's u = 2 |x| is exact


def test_translations_are_exact_and_fallback_cases_are_what_they_claim():
    X, Xs, _, _ = H.translation_data()
    for t in H.TRANSLATIONS:
        t = np.asarray(t)
        assert np.array_equal((X + t) - t, X) and np.array_equal((Xs + t) - t, Xs)
    a, b, c = H.FALLBACKS["rank one"][:3]
    assert c - (b / np.sqrt(a)) ** 2 == 0.0
    a, b, c = H.FALLBACKS["indefinite"][:3]
    assert c - (b / np.sqrt(a)) ** 2 < 0.0
    Xq = H.gauss_queries(m=4000, lo=-8.0, hi=H.FALLBACKS["indefinite"][3], seed=11)
    ref, s = H.gauss_ref(Xq, H.GAUSS_XT, a, b, c, 1.3)
    assert 2 * s.min() > -100 and 2 * s.min() < -10 and np.isfinite(float(ref.max())) and ref.max() > 100


# ---- GPU -----------------------------------------------------------------------------------------------------------
def assert_gauss_route(name, res):
    assert res["max_ratio"] <= 1.0, (name, show(res))
    assert res.get("nonzero_where_zero", 0) == 0, (name, show(res))
    assert res["at_zero_exact"], (name, show(res))
    assert res.get("nan_ok", True), (name, show(res))


@pytest.fixture(scope="module")
def default_process():
    """the sweeps of the fused predict with no switch set, in this process"""
    return {"gauss": H.gauss_sweep(), "shapes": H.gauss_shapes()}


@pytest.mark.gpu
def test_gaussian_values_every_route(default_process):
    """packed K build, kernel matrix (cross and self) and the fused predict against mpmath within
    (8 + 16 sqrt(s S)) 2^-53 ref + 2 * 2^-1074; exactly amp at distance 0; exactly 0 below 2^-1075"""
    out = default_process["gauss"]
    print(show(out))
    assert out["inputs"]["residues"] == 256
    assert len(out["routes"]) == 8
    for name, res in out["routes"].items():
        assert_gauss_route(name, res)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"TGP_PREDICT_EXP": "0"}, {"TGP_PREDICT_EXP": "32"}, {"TGP_PREDICT_EXP": "64"},
                                 {"TGP_PREDICT_GENERIC": "1"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_gaussian_values_predict_variants(env):
    """the other exponentials of the fused predict (degree-13 polynomial, 32- and 64-entry tables, libm), each in a
    process of its own, same sweep, fall-backs included"""
    out = H.run_in_fresh_process(["gauss", "fallbacks"], env)
    print(show(out))
    for name, res in out["gauss"]["routes"].items():
        assert_gauss_route(name, res)
    assert_fallbacks(out["fallbacks"])


@pytest.mark.gpu
def test_gaussian_shapes_bit_identical(default_process):
    """n in {1, 2, 255, 256, 257, 600, 5000}, one-hot at the tile edges, m in {1, 255, 256, 257, 30000}: the value of a
    pair does not depend on the shape of the call (all sets share their first point, the origin of the transform)"""
    out = default_process["shapes"]
    print(show(out))
    assert out["calls"] >= 40
    assert out["mismatches"] == [], show(out)
    assert out["alone_vs_set_max_ratio"] <= 1.0, show(out)


@pytest.mark.gpu
@pytest.mark.parametrize("wgs", ["1", "100000"])
def test_gaussian_shapes_do_not_depend_on_the_split(default_process, wgs):
    """one split of the training set, and as many splits as it has tiles: the same bits as the default"""
    out = H.run_in_fresh_process(["gauss", "shapes"], {"TGP_PREDICT_WGS": wgs})
    print(show(out))
    assert out["shapes"]["mismatches"] == [], show(out["shapes"])
    assert out["shapes"]["digest"] == default_process["shapes"]["digest"]
    assert out["gauss"]["routes"]["predict amp=1"]["digest"] == default_process["gauss"]["routes"]["predict amp=1"]["digest"]


def assert_fallbacks(out):
    assert set(out) == set(H.FALLBACKS)
    for name, res in out.items():
        for r in ("predict", "kmat_cross"):
            assert res[r]["max_ratio"] <= 1.0, (name, r, show(res))
            assert res[r].get("nonzero_where_zero", 0) == 0, (name, r, show(res))
            assert res[r]["at_zero_exact"], (name, r, show(res))
    assert out["indefinite"]["min_q"] > -100 and out["indefinite"]["max_ref"] > 100


@pytest.mark.gpu
def test_gaussian_fallbacks_of_the_launcher():
    """1-D (c = b = 0), a = 0, a rank-one and an indefinite invLam, each against mpmath"""
    out = H.gauss_fallbacks()
    print(show(out))
    assert_fallbacks(out)


@pytest.mark.gpu
def test_von_karman_values_every_route():
    """K build, kernel matrix and the one-hot predict (LDS table) on the device against mpmath at the host test's
    tolerance (rtol 2e-13, atol 1e-13), every branch of the function; 1 at u = 0, 0 beyond K56_XMAX; the three routes
    run the same function on the same coefficients and agree bit for bit"""
    out = H.vk_sweep()
    print(show(out))
    assert all(v >= 200 for v in out["segments"].values())
    for case in ("vk", "avk", "vk off-axis", "avk off-axis"):
        for r in ("predict", "kmat_cross", "kbuild"):
            res = out[case][r]
            assert res["max_ratio"] <= 1.0, (case, r, show(res))
            assert res["nonzero_where_zero"] == 0, (case, r, show(res))
            assert res.get("at_zero_exact", True), (case, r, show(res))
        assert out[case]["routes_max_ulp"] == 0, (case, show(out[case]))


@pytest.mark.gpu
def test_gaussian_predict_is_translation_invariant():
    """The same points at offsets 0, 1024, 2^20 and (-2^20, 2^17): (a) one-hot values within the Gaussian bound with S
    from the data's own diameter, (b) predictions with alpha solved at the shifted coordinates within 1e-10 max|y| of the
    long-double sum over the reference and within 1e-12 max|y| of the unshifted prediction with the same alpha.

    Before the transform took its origin from the data the same run measured on an MI355X, for the README's kernel /
    ell = 0.005: (a) error / bound = 175 / 117 at 1024 and 1.8e5 / 1.4e5 at 2^20, (b) 1.5e-10 / 1.6e-11 of max|y| at
    1024 and 1.8e-7 / 2.7e-8 at 2^20 (both figures of (b) alike: the unshifted prediction is within 1e-13 of the
    reference).  With it every offset gives the bits of the unshifted call (LAB_NOTES.md)."""
    out = H.translation_sweep()
    print(show(out))
    assert len(out) == 8
    for name, res in out.items():
        assert res["onehot_max_ratio"] <= 1.0, (name, show(res))
        assert res["predict_vs_ref"] <= 1e-10, (name, show(res))
        assert res["predict_vs_unshifted"] <= 1e-12, (name, show(res))


@pytest.mark.gpu
def test_gp_interpolation_is_translation_invariant():
    """(c) GPInterpolation.predict at an offset of 2^20 against the same object at the origin, and predict_many for two
    objects at different offsets: 1e-10 of max|y|"""
    out = H.translation_api()
    print(show(out))
    assert out["predict"] <= 1e-10, show(out)
    assert out["predict_many"] <= 1e-10, show(out)

"""The premises of tests/test_gpu_units.py, asserted on the CPU from oracle/gp_oracle.py and NumPy alone.

Bit-homogeneity legitimately ends where a scaled value enters the subnormal range (the K build's stand-in 2^-1021 p for the
values it clamps is such a place), where a scaling is not exact, or where the dimension table has a wrong power.  None of that
may be assumed: every condition the device test relies on is checked here on the very inputs it uses."""
import numpy as np
import pytest

import _units_helpers as H
from _units_helpers import Units, LD
from oracle import gp_oracle as O

ALL_UNITS = (H.UNIT,) + H.WITH_Y + tuple(Units(p=p) for p in H.BATCH_P) + (Units(p=10, q=12),)
MAX_P = max(abs(u.p) for u in ALL_UNITS)


def _all_inputs():
    """every problem of test_gpu_units.py: (name, Inputs)"""
    out = [("dense n=%d" % n, H.inputs(n)) for n in H.DENSE_N]
    out += [("values n=%d d=%d" % (n, d), H.inputs(n, ndim=d)) for n in (300, 1025) for d in (2, 3)]
    out += [("batch %d" % b, H.inputs(n, seed=7 + b)) for b, n in enumerate(H.BATCH_NS)]
    out += [("local", H.inputs(H.LOCAL_N, seed=2)), ("fisher", H.inputs(H.FISHER_N))]
    out += [("api %d" % i, H.inputs(200 + 57 * i, seed=3 + i)) for i in range(2)]
    return out


def _form_max_over_box(m):
    """the largest d^T M d for d in [-0.5, 0.5]^ndim: a convex form takes its maximum at a corner (2-D: m = (a, b, c); 3-D: six)"""
    if len(m) == 3:
        M = np.array([[m[0], m[1]], [m[1], m[2]]])
    else:
        xx, xy, xz, yy, yz, zz = m
        M = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
    assert np.linalg.eigvalsh(M).min() > 0.0
    corners = np.array(np.meshgrid(*[(-0.5, 0.5)] * len(M))).reshape(len(M), -1).T
    return float(np.einsum("ik,kl,il->i", corners, M, corners).max())


def test_every_problem_lies_in_the_box():
    for name, P in _all_inputs():
        assert P.X.min() >= 0.0 and P.X.max() <= 0.5 and P.Xq.min() >= 0.0 and P.Xq.max() <= 0.5, name


def test_gaussian_exponents_stay_far_from_the_clamp():
    """every Gaussian value of a call: s = q / 2 log2(e) over all pairs (bounded by the form's maximum over the box that holds
    every problem), plus 2 max|p| for the amplitude, plus 64 for the products of the factorisation, stays below 900 of the 1021
    at which the K build clamps"""
    for m in ((H.INVLAM["a"], H.INVLAM["b"], H.INVLAM["c"]), (400.0, 0.0, 400.0), H.M3):
        s = 0.5 * _form_max_over_box(m) * np.log2(np.e)
        assert s + 2 * MAX_P + 64 < H.GAUSS_EXPONENT_MAX, (m, s)


@pytest.mark.parametrize("name,P", [(k, v) for k, v in _all_inputs() if v.n <= 1025], ids=lambda v: v if isinstance(v, str) else "")
def test_von_karman_values_are_zero_or_far_above_the_subnormals(name, P):
    """every von Karman value is exactly 0 (beyond the cut-off) or above 2^-200, so that amp 4^p k stays normal"""
    Z = np.concatenate([P.X, P.Xq])
    if P.ndim == 2:
        vals = [O.kernel_matrix("vk", Z, ell=H.ELL), O.kernel_matrix("avk", Z, a=120.0, b=30.0, c=150.0)]
    else:
        d = Z[:, None, :] - Z[None, :, :]
        vals = [O._vk_of_u(np.sqrt((d ** 2).sum(-1)) / H.ELL)]
    for k in vals:
        assert np.all((k == 0.0) | (k > 2.0 ** -200)), name
        assert np.all(k <= 1.0 + 1e-12)


def test_von_karman_values_in_the_whole_box():
    """the larger problems lie in the same box: the kernel is monotone in u, so its value at the box's diameter bounds them all"""
    for u in (np.sqrt(0.75) / H.ELL, np.sqrt(_form_max_over_box((120.0, 30.0, 150.0)))):
        k = O._vk_of_u(np.array([u]))[0]
        assert k == 0.0 or k > 2.0 ** -200, (u, k)


def test_scaled_inputs_stay_in_range():
    """no |y|, y_err^2 or amp leaves [2^-200, 2^200] at any scale (zeros of y aside: there are none)"""
    lo, hi = 2.0 ** -H.RANGE, 2.0 ** H.RANGE
    for name, P0 in _all_inputs():
        for u in ALL_UNITS:
            P = P0.at(u)
            for what, v in (("y", np.abs(P.y)), ("y_err^2", P.e ** 2), ("amp", np.array([u.amp(H.AMP), u.amp(0.5 * H.AMP)]))):
                assert v.min() >= lo and v.max() <= hi, (name, u, what, v.min(), v.max())
    c = H.pair_catalogue()
    for u in ALL_UNITS:
        for what in ("k", "err", "dx", "dy"):
            v = np.abs(u.val(c[what]))
            assert v.min() >= lo and v.max() <= hi, (u, what)


def test_scalings_are_exact():
    """ldexp(ldexp(x, s), -s) == x bit for bit on every input array, for every scaling in use"""
    arrays = []
    for name, P in _all_inputs():
        arrays += list(P.arrays().values())
    arrays += list(H.pair_catalogue().values())
    arrays += [np.array([H.AMP, 0.5 * H.AMP, 0.75 * H.AMP, H.ELL, 0.03125, 4.0] + list(H.INVLAM.values()) + list(H.M3)
                        + [120.0, 30.0, 150.0] + [H.PAIR_TWOD[k] for k in ("min_sep", "max_sep")]
                        + [H.PAIR_LOG[k] for k in ("min_sep", "max_sep")])]
    shifts = sorted({s for u in ALL_UNITS for s in (u.p, 2 * u.p, u.r, u.p + u.r, u.q, -2 * u.q)})
    for a in arrays:
        for s in shifts:
            back = np.ldexp(np.ldexp(a, s), -s)
            assert np.array_equal(H.bits(back), H.bits(a)), s


def test_shift_of_a_dimension():
    u = Units(p=3, r=5, q=-2)
    assert u.shift("alpha") == -3 + 5 and u.shift("predict_grad") == 3 + 2 + 5 and u.shift("ydota") == 10
    assert u.shift("grad_abc") is None and Units(p=3, q=-2).shift("grad_abc") == -4
    assert np.array_equal(H.fisher_shift(Units(q=1), 1), [[0, 2, 2, 2], [2, 4, 4, 4], [2, 4, 4, 4], [2, 4, 4, 4]])
    assert H.diff_report(np.ldexp(np.array([1.5, -0.0]), 4), np.array([1.5, -0.0]), 4) is None
    assert H.diff_report(np.array([0.0]), np.array([-0.0]), 0) is not None
    assert H.diff_report(np.array([1.5 + 2.0 ** -52]), np.array([1.5]), 0) is not None


@pytest.mark.parametrize("units", H.WITH_Y, ids=[repr(u) for u in H.WITH_Y])
def test_oracle_is_homogeneous_to_rounding(units):
    """alpha, predict, var and logdet of the oracle at each scale agree with the shifted unit-scale values within 1e-12 relative:
    a wrong power in the dimension table fails here, without a GPU"""
    def run(u):
        P = H.inputs(300).at(u)
        kw = u.kw(dict(amp=H.AMP, **H.INVLAM))
        K = O.kernel_matrix("gauss", P.X, **kw)
        alpha, logdet = O.gp_solve(K, P.y, P.e)
        HT = O.kernel_matrix("gauss", P.Xq, P.X, **kw)
        cov = O.gp_predict_cov(K, P.e, HT, O.kernel_matrix("gauss", P.Xq, **kw))
        d = P.Xq[:, None, :] - P.X[None, :, :]
        M = np.array([[kw["a"], kw["b"]], [kw["b"], kw["c"]]])
        grad = -np.einsum("ji,jik->jk", HT * alpha[None, :], d @ M)
        Kinv = np.linalg.inv(K + np.diag(P.e ** 2))
        L = np.linalg.cholesky(K + np.diag(P.e ** 2))
        return [("alpha", "alpha", alpha), ("predict", "predict", O.gp_predict(HT, alpha)), ("var", "var", np.diag(cov).copy()),
                ("cov", "cov", cov), ("K", "K", K), ("ydota", "ydota", float(P.y @ alpha)), ("predict_grad", "predict_grad", grad),
                ("inv_diag", "inv_diag", np.diag(Kinv).copy()), ("factor_solve", "factor_solve", P.B @ Kinv), ("L", "L", L),
                ("factor_lmul", "factor_lmul", P.Z @ L.T)], logdet

    got, ld_s = run(units)
    ref, ld_u = run(H.UNIT)
    for (k, dim, a), (_, _, b) in zip(got, ref):
        want = H.expected(b, units.shift(dim))
        scale = np.abs(want).max()
        assert np.abs(a - want).max() <= 1e-12 * scale, (k, units)
    H.assert_log_shift(ld_s, ld_u, 300, 2 * units.p, "oracle logdet")
    assert abs((ld_s - ld_u) - float(H.log_shift(300, 2 * units.p))) <= 1e-12 * max(abs(ld_s), abs(ld_u), 1.0)


def test_oracle_gradient_dimensions():
    """d logL / d log amp without unit, d / d (a, b, c) with X^2, from the oracle's own gradient"""
    basis = [np.array([[1.0, 0], [0, 0]]), np.array([[0, 1.0], [1.0, 0]]), np.array([[0, 0], [0, 1.0]])]

    def run(u):
        P = H.inputs(130, seed=8).at(u)
        kw = u.kw(dict(amp=H.AMP, **H.INVLAM))
        g_amp, g = O.loglik_grad_invlam(P.X, P.y, P.e, kw["amp"], np.array([[kw["a"], kw["b"]], [kw["b"], kw["c"]]]), basis)
        return np.concatenate([[g_amp], g])
    ref = run(H.UNIT)
    for u in H.NO_Y:
        got = run(u)
        want = np.ldexp(ref, [u.shift(d) for d in ("grad_logamp", "grad_abc", "grad_abc", "grad_abc")])
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want).max()), u


def test_log_binned_pairs_stay_clear_of_the_edges():
    """kk_log and vcorr_sums are held to equal pair counts under S_x: in long double, no pair of the catalogue lies within
    1e-9 bin widths of a bin edge, or of min_sep / max_sep, at any of the three scales"""
    c = H.pair_catalogue()
    lg = H.PAIR_LOG
    i, j = np.triu_indices(len(c["x"]), 1)
    counts = []
    for u in (H.UNIT,) + H.S_X:
        x, y = u.x(c["x"]).astype(LD), u.x(c["y"]).astype(LD)
        dx, dy = x[j] - x[i], y[j] - y[i]
        lr = LD(0.5) * np.log(dx * dx + dy * dy)
        mn, mx = LD(u.sep(lg["min_sep"])), LD(u.sep(lg["max_sep"]))
        bs = np.log(mx / mn) / lg["nbins"]
        cb = (lr - np.log(mn)) / bs
        inside = (cb > -0.5) & (cb < lg["nbins"] + 0.5)
        gap = float(np.abs(cb[inside] - np.rint(cb[inside])).min())
        assert gap > 1e-9, (u, gap)
        b = np.floor(cb).astype(np.int64)
        ok = (b >= 0) & (b < lg["nbins"])
        counts.append(np.bincount(b[ok], minlength=lg["nbins"]))
        edges = H.pair_log_edges(u).astype(LD)
        width = float(np.diff(edges).min())
        near = min(float(np.abs(lr - e).min()) for e in edges)
        assert near / width > 1e-9, (u, near / width)
    assert np.array_equal(counts[0], counts[1]) and np.array_equal(counts[0], counts[2])
    assert counts[0].min() > 0


def test_twod_pairs_stay_clear_of_the_edges():
    """the TwoD rule is exactly homogeneous; still no pair may sit on a pixel edge, where int() of a quotient decides"""
    from _pair_stat_refs import twod_deposits
    c, t = H.pair_catalogue(), H.PAIR_TWOD
    d = twod_deposits(c["x"], c["y"], t["min_sep"], t["max_sep"], t["nbins"])
    assert d["on_edge"] == 0 and d["edge_gap"] > 1e-9 and d["naccepted"] > 10000

"""GPU tests of the Fisher information of the hyper-parameters (include/tgp.h seam S2j: tgp_gp_fisher, tgp_gp_fisher_sum;
ops.gp_fisher, GPInterpolation.return_fisher_information / return_theta_covariance) against the host references of
tests/_fisher_refs.py and the reference project's own kernel derivatives (tests/golden/g16_fisher.npz).

Tolerance throughout, unless stated: |F_dev - F_ref| <= 1e-10 sqrt(F_ii F_jj), the project's standard for predictions; the
float64 LAPACK reference sits at <= 1.5e-14 of the long-double one on these inputs (cond(K + D) <= 1.2e5)."""
import ctypes as C

import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib, kernels, ops

import _fisher_refs as FR
import _ksum_refs as S
import _vk_loglik_grad_refs as V
from _history_helpers import Ctx, raw, rejected_nan

pytestmark = pytest.mark.gpu

TOL = 1e-10
GOLDEN_ARBF = "0.7**2 * AnisotropicRBF(invLam=array([[40., -9.], [-9., 25.]]))"
GOLDEN_RBF = "0.7**2 * RBF(0.2)"
KERNELS = {"arbf": GOLDEN_ARBF, "rbf": GOLDEN_RBF, "avk": V.SET_A["avk"], "vk": V.SET_A["vk"]}


def spec_of(kern):
    return kernels.device_spec(tg.eval_kernel(kern))


def device_fisher(spec, X, y, y_err, ctx=None):
    fac = ops.gp_solve(spec, X, y, y_err, keep=True, want_alpha=False, ctx=ctx)[3]
    try:
        return ops.gp_fisher(spec, fac, X, ctx=ctx)
    finally:
        fac.free()


def assert_same_bits(a, b, what):
    assert np.shape(a) == np.shape(b), what
    assert np.array_equal(raw(a), raw(b)), "%s: %r vs %r" % (what, a, b)


# ---- 1. values on both substitution paths ------------------------------------------------------------------------------------------
# one point; a partial panel; two panels with a partial one; one point past two panels; Np = 2304, the big-step substitution
@pytest.mark.parametrize("n", [1, 129, 300, 513, 2100])
@pytest.mark.parametrize("kind", ["arbf", "rbf", "avk", "vk"])
def test_values_against_the_host_reference(kind, n):
    spec = spec_of(KERNELS[kind])
    X, y, y_err = V.data_a(n)
    F = device_fisher(spec, X, y, y_err)
    assert F.shape == (4, 4) and np.all(np.isfinite(F))
    if n == 1:
        expect = np.zeros((4, 4))
        expect[0, 0] = 0.5 * (spec.amp / (spec.amp + y_err[0] ** 2)) ** 2
        print("fisher %s n=1: F00 = %r, expected %r" % (kind, F[0, 0], expect[0, 0]))
        assert abs(F[0, 0] - expect[0, 0]) <= TOL * expect[0, 0]
        expect[0, 0] = F[0, 0]
        assert np.array_equal(F, expect)                         # the slopes of a single point are exactly 0
        return
    ref = FR.reference(kind, spec, X, y_err, longdouble=n <= FR.LONGDOUBLE_NMAX)
    err = FR.rel_err(F, ref)
    print("fisher %s n=%d: max |F - ref| / sqrt(F_ii F_jj) = %.3e" % (kind, n, err))
    assert err <= TOL, (kind, n, err)


# ---- 2. exact anchor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 513, 2100])
@pytest.mark.parametrize("kind", ["avk", "vk"])
def test_without_noise_the_amplitude_entry_is_half_n(kind, n):
    """y_err = None: D_0 = K, so S_0 is the identity and F[0][0] = n / 2"""
    spec = spec_of(KERNELS[kind])
    X, y, _ = V.data_a(n)
    F = device_fisher(spec, X, y, None)
    print("fisher anchor %s n=%d: F00 - n/2 = %.3e" % (kind, n, F[0, 0] - 0.5 * n))
    assert abs(F[0, 0] - 0.5 * n) <= TOL * n


# ---- 3. sums -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["SUM_A", "SUM_B"])
def test_sums_against_the_host_reference(tag):
    kern = getattr(S, tag)
    spec = spec_of(kern)
    assert isinstance(spec, ops.KernelSumSpec)
    X, y, e, _ = S.data(300)
    F = device_fisher(spec, X, y, e)
    P = 4 * len(spec.terms)
    assert F.shape == (P, P)
    ref = FR.reference(tag, spec, X, e, longdouble=True)
    err = FR.rel_err(F, ref)
    print("fisher %s n=300 (%d matrices): max rel err = %.3e" % (tag, P, err))
    assert err <= TOL
    assert_same_bits(F, F.T, tag + ": symmetric")


def test_a_sum_of_one_term_is_the_single_kernel_entry():
    X, y, e, _ = S.data(300)
    for kind in ("arbf", "vk"):
        one = spec_of(KERNELS[kind])
        fac = ops.gp_solve(one, X, y, e, keep=True, want_alpha=False)[3]
        try:
            assert_same_bits(ops.gp_fisher(ops.KernelSumSpec([one]), fac, X), ops.gp_fisher(one, fac, X), kind)
        finally:
            fac.free()


# ---- 4. golden ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["arbf", "rbf"])
def test_object_methods_against_the_reference_projects_derivatives(golden, tag):
    g = golden("g16_fisher.npz")
    kern = str(g[tag + "_kernel"])
    assert kern == KERNELS[tag]
    X, y, y_err = V.data_a(200)
    assert np.array_equal(X, g["X"]) and np.array_equal(y_err, g["y_err"])
    gp = tg.GPInterpolation(kernel=kern, optimizer="none", normalize=True)
    gp.initialize(X, y, y_err=y_err)
    F = gp.return_fisher_information()
    ref = g[tag + "_F"]
    err = FR.rel_err(F, ref)
    print("fisher golden %s: max rel err = %.3e" % (tag, err))
    assert err <= TOL
    cov = gp.return_theta_covariance()
    inv = np.linalg.inv(ref)
    d = np.sqrt(np.diag(inv))
    cerr = np.max(np.abs(cov - inv) / np.outer(d, d))
    print("fisher golden %s: covariance max rel err = %.3e" % (tag, cerr))
    assert cerr <= 1e-8
    assert gp._alpha is None and gp._factor is None                # a temporary factor of their own


# ---- 5. coincident points and the cutoff -------------------------------------------------------------------------------------------
def test_duplicated_points_and_pairs_beyond_the_cutoff():
    X, y, y_err = V.data_a(300)
    X = X.copy()
    X[7] = X[3]
    X[200] = X[150]
    # invLam 1e3 x set A's: 2 pi u crosses the cutoff 697.87 at |d| = 0.53 .. 0.77 with the direction; length scale 0.004: at 0.44
    for kind, spec in (("avk", ops.KernelSpec(_lib.TGP_AVK, amp=V.AMP, a=4.0e4, b=-9.0e3, c=2.5e4)),
                       ("vk", ops.KernelSpec(_lib.TGP_VK, amp=V.AMP, ell=0.004))):
        _, W, dx, dy = V.kernel_and_slope(spec.kind, X, spec.amp, spec.a, spec.b, spec.c, spec.ell)
        a, b, c = V.abc(spec.kind, spec.a, spec.b, spec.c, spec.ell)
        x = 2.0 * np.pi * np.sqrt(a * dx * dx + 2.0 * b * dx * dy + c * dy * dy)
        off = ~np.eye(len(X), dtype=bool)
        assert (x[off] > V.K56_XMAX).sum() > 1000 and ((x[off] > 0) & (x[off] <= V.K56_XMAX)).sum() > 1000
        assert (x[off] == 0).sum() == 4                            # the two duplicated pairs, both ways round
        F = device_fisher(spec, X, y, y_err)
        assert np.all(np.isfinite(F)), (kind, F)
        ref = FR.reference("cutoff-" + kind, spec, X, y_err, longdouble=True)
        err = FR.rel_err(F, ref)
        print("fisher duplicates + cutoff %s: max rel err = %.3e" % (kind, err))
        assert err <= TOL


# ---- 6. bit stability --------------------------------------------------------------------------------------------------------------
_FRESH = {}


def history_case():
    X, y, e, Xs = S.data(300)
    return spec_of(S.SUM_A), spec_of(KERNELS["avk"]), X, y, e, Xs


def fisher_entries(h):
    """the sum's and the single kernel's Fisher matrices and the variance around them, on context h"""
    sumspec, one, X, y, e, Xs = history_case()
    out = []
    for tag, spec in (("sum", sumspec), ("one", one)):
        fac = ops.gp_solve(spec, X, y, e, keep=True, want_alpha=False, ctx=h)[3]
        try:
            v0 = ops.gp_predict_var(spec, fac, X, Xs, ctx=h)
            F = ops.gp_fisher(spec, fac, X, ctx=h)
            assert_same_bits(ops.gp_fisher(spec, fac, X, ctx=h), F, tag + ": the same call twice")
            assert_same_bits(F, F.T, tag + ": symmetric")
            assert_same_bits(ops.gp_predict_var(spec, fac, X, Xs, ctx=h), v0, tag + ": the variance after the Fisher call")
            out += [(tag + ".F", F), (tag + ".var", v0)]
        finally:
            fac.free()
    return out


def fresh_reference():
    if "ref" not in _FRESH:
        with Ctx() as c:
            _FRESH["ref"] = fisher_entries(c.h)
    return _FRESH["ref"]


def test_same_bits_twice_symmetric_and_the_factor_is_left_as_found():
    fresh_reference()


def test_fisher_does_not_depend_on_what_the_context_did_before():
    ref = fresh_reference()
    Xl, yl, el, _ = S.data(700)
    big = ops.KernelSpec(_lib.TGP_ARBF, amp=1.3e4, a=60.0, b=8.0, c=45.0)
    with Ctx() as c:
        fac = ops.gp_solve(big, Xl + 7.0, yl * 1e8, el * 1e2, keep=True, ctx=c.h)[3]       # a larger, louder solve
        ops.gp_predict_cov(big, fac, Xl + 7.0, Xl[:300] + 7.0, ctx=c.h)
        ops.gp_fisher(big, fac, Xl + 7.0, ctx=c.h)
        fac.free(keep_memory=True)
        rejected_nan(c, 700)                                                               # rejected: not positive definite
        for what in ("after a larger solve, a covariance and a rejected solve", "after tgp_release_caches"):
            got = fisher_entries(c.h)
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, a), (_, b) in zip(got, ref):
                assert_same_bits(a, b, what + ": " + k)
            _lib.check(c.h, c.lib.tgp_release_caches(c.h), "tgp_release_caches")


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_by_name_and_leave_the_context_usable():
    sumspec, one, X, y, e, _ = history_case()
    X = np.ascontiguousarray(X, dtype=np.float64)
    p = _lib.ptr
    with Ctx() as c:
        lib = c.lib
        fac = c.track(ops.gp_solve(one, X, y, e, keep=True, want_alpha=False, ctx=c.h)[3])
        good = ops.gp_fisher(one, fac, X, ctx=c.h)
        out = np.full((16, 16), 7.0)

        def msg():
            return (lib.tgp_last_error(c.h) or b"").decode()
        k1, ks = one.to_c(), sumspec.to_c()
        assert lib.tgp_gp_fisher(c.h, fac._h, C.byref(k1), p(X), len(X) - 1, p(out)) == -1
        assert "tgp_gp_fisher" in msg() and "n = 299" in msg()
        assert lib.tgp_gp_fisher_sum(c.h, fac._h, C.byref(ks), p(X), len(X) + 1, p(out)) == -1
        assert "tgp_gp_fisher_sum" in msg() and "n = 301" in msg()
        bad = one.to_c()
        bad.kind = 99
        assert lib.tgp_gp_fisher(c.h, fac._h, C.byref(bad), p(X), len(X), p(out)) == -1
        assert "tgp_gp_fisher" in msg() and "kind 99" in msg()
        bad = sumspec.to_c()
        bad.term[1].kind = 99
        assert lib.tgp_gp_fisher_sum(c.h, fac._h, C.byref(bad), p(X), len(X), p(out)) == -1
        assert "tgp_gp_fisher_sum" in msg() and "kind 99" in msg() and "term 1" in msg()
        for nterms in (0, 5):
            bad = sumspec.to_c()
            bad.nterms = nterms
            assert lib.tgp_gp_fisher_sum(c.h, fac._h, C.byref(bad), p(X), len(X), p(out)) == -1
            assert "tgp_gp_fisher_sum" in msg() and "nterms = %d" % nterms in msg()
        assert lib.tgp_gp_fisher(c.h, None, C.byref(k1), p(X), len(X), p(out)) == -1 and "tgp_gp_fisher: f " in msg()
        assert lib.tgp_gp_fisher(c.h, fac._h, C.byref(k1), None, len(X), p(out)) == -1 and "tgp_gp_fisher: X " in msg()
        assert lib.tgp_gp_fisher(c.h, fac._h, C.byref(k1), p(X), len(X), None) == -1 and "tgp_gp_fisher: fisher " in msg()
        assert np.all(out == 7.0)                                  # nothing was written
        assert_same_bits(ops.gp_fisher(one, fac, X, ctx=c.h), good, "the context after the rejected calls")
        with pytest.raises(ValueError, match="KernelSpec3"):
            ops.gp_fisher(ops.KernelSpec3(_lib.TGP_ARBF), fac, X, ctx=c.h)
        fac.free()
        with pytest.raises(ValueError, match="freed"):
            ops.gp_fisher(one, fac, X, ctx=c.h)

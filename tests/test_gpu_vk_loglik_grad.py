"""GPU tests of the exact likelihood gradient for all four kernel kinds (include/tgp.h seam S2h: tgp_gp_loglik_grad_any,
tgp_d_gp_solve_grad_any, tgp_gp_solve_grad_batch_any) against the dense reference of tests/_vk_loglik_grad_refs.py, of the bit
identities with the Gaussian-only entries, and of the fits built on it (TGP_ML_GRADIENT=analytic-vk,
solve_many(gradient="analytic-vk"))."""
import ctypes

import numpy as np
import pytest

import treegp_amd as treegp
from treegp_amd import _lib, ops
from treegp_amd.kernels import kernel_to_spec

import _vk_loglik_grad_refs as R

pytestmark = pytest.mark.gpu

# one point, two, a partial 64-row block, one past it, a partial panel, a block that crosses the diagonal panel, one point past a
# panel, more than one panel with partial everything
RAGGED_NS = [1, 2, 63, 64, 65, 255, 256, 257, 300, 513, 1100]
_refs = {}


def reference(tag, spec, X, y, y_err):
    """the dense reference of one input, computed once"""
    if tag not in _refs:
        _refs[tag] = R.spec_solve_grad(spec, X, y, y_err)
    return _refs[tag]


def single(spec, X, y, y_err):
    alpha, ld, chi2, fac = ops.gp_solve(spec, X, y, y_err, keep=True)
    try:
        return ld, chi2, ops.gp_loglik_grad_any(spec, fac, X, alpha)
    finally:
        fac.free()


def set_a(name, n):
    spec = kernel_to_spec(treegp.eval_kernel(R.SET_A[name]))
    return (spec,) + R.data_a(n, 1 if name == "avk1d" else 2)


# ---- 5. ragged sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RAGGED_NS)
def test_gradient_against_the_dense_reference_at_ragged_sizes(n):
    for name in ("avk", "vk", "avk1d"):
        spec, X, y, y_err = set_a(name, n)
        ld, chi2, g4 = single(spec, X, y, y_err)
        ld_ref, chi2_ref, ref, _ = reference((name, n), spec, X, y, y_err)
        print("n=%d %s g4=%r ref=%r" % (n, name, g4, ref))
        np.testing.assert_allclose(g4, ref, rtol=1e-8, atol=1e-8 * max(np.abs(ref).max(), 1.0), err_msg="n=%d %s" % (n, name))
        assert ld == pytest.approx(ld_ref, rel=1e-9, abs=1e-9) and chi2 == pytest.approx(chi2_ref, rel=1e-9)


# ---- 6. the scale ladder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1e-3, 1.0, 1e2, 1e4, 1e6])
def test_scale_ladder_every_branch_of_the_profile(s):
    """n = 300 hard-core points, the last a copy of the first (u == 0 off the diagonal, K + D still positive definite);
    invLam = s [[40, -9], [-9, 25]]: the series (s = 1e-3), every Chebyshev segment including the 64 / x one (1, 1e2), the cutoff
    (1e4 in part, 1e6 for every distinct pair).  Each component against its own sum's scale S[p] = sum |term|."""
    X, y, y_err = R.data_ladder()
    assert np.array_equal(X[-1], X[0])
    spec = ops.KernelSpec(_lib.TGP_AVK, amp=R.AMP, a=s * 40.0, b=s * -9.0, c=s * 25.0)
    _, _, g4 = single(spec, X, y, y_err)
    _, _, ref, S = reference(("ladder", s), spec, X, y, y_err)
    print("s=%g g4=%r ref=%r S=%r" % (s, g4, ref, S))
    assert np.all(np.isfinite(g4))
    for p in range(4):
        assert abs(g4[p] - ref[p]) <= 1e-8 * S[p], (s, p, g4[p], ref[p], S[p])
    if s == 1e6:
        assert np.array_equal(g4[1:], np.zeros(3)) and g4[0] != 0.0


# ---- 7. bit identities -------------------------------------------------------------------------------------------------------------
GAUSS = ["0.7**2 * RBF(0.11)", "0.7**2 * AnisotropicRBF(invLam=array([[40., -9.], [-9., 25.]]))"]


def test_gaussian_kinds_have_the_bits_of_the_old_entries():
    for kern in GAUSS:
        spec = kernel_to_spec(treegp.eval_kernel(kern))
        for n in (300, 513):
            X, y, y_err = R.data_a(n)
            alpha, _, _, fac = ops.gp_solve(spec, X, y, y_err, keep=True)
            try:
                old, new = ops.gp_loglik_grad(spec, fac, X, alpha), ops.gp_loglik_grad_any(spec, fac, X, alpha)
            finally:
                fac.free()
            assert np.array_equal(old, new) and np.all(np.isfinite(new)), (kern, n)
        prob = ops.ResidentProblem(X, y, y_err)
        try:
            old, new = ops.gp_solve_grad_resident(spec, prob), ops.gp_solve_grad_resident_any(spec, prob)
        finally:
            prob.close()
        assert old[0] == new[0] and old[1] == new[1] and np.array_equal(old[2], new[2])
    specs = [kernel_to_spec(treegp.eval_kernel(GAUSS[b % 2])) for b in range(4)]
    data = [R.data_a(n) for n in (300, 1, 257, 63)]
    args = (specs, [d[0] for d in data], [d[1] for d in data], [d[2] for d in data])
    old, new = ops.gp_solve_grad_batch(*args), ops.gp_solve_grad_batch_any(*args)
    for o, v in zip(old, new):
        assert np.array_equal(o, v)


def test_every_entry_is_bit_identical_from_run_to_run():
    for name in ("avk", "vk", "avk1d"):
        spec, X, y, y_err = set_a(name, 513)
        first, second = single(spec, X, y, y_err), single(spec, X, y, y_err)
        assert first[0] == second[0] and first[1] == second[1] and np.array_equal(first[2], second[2])
        prob = ops.ResidentProblem(X, y, y_err)
        try:
            r1, r2 = ops.gp_solve_grad_resident_any(spec, prob), ops.gp_solve_grad_resident_any(spec, prob)
        finally:
            prob.close()
        assert r1[0] == r2[0] and r1[1] == r2[1] and np.array_equal(r1[2], r2[2])
        assert np.array_equal(r1[2], first[2]) and r1[0] == first[0]          # the fused call is the two-step route


# ---- 8. the batch ------------------------------------------------------------------------------------------------------------------
MIX = [("0.7**2 * AnisotropicRBF(invLam=array([[40., -9.], [-9., 25.]]))", 300), (R.SET_A["vk"], 1), (R.SET_A["avk"], 257),
       ("0.7**2 * RBF(0.11)", 63), ("0.6**2 * AnisotropicVonKarman(invLam=array([[30., 5.], [5., 60.]]))", 512)]


def _call(problems, order=None):
    order = list(range(len(problems))) if order is None else list(order)
    p = [problems[i] for i in order]
    return ops.gp_solve_grad_batch_any([q[0] for q in p], [q[1] for q in p], [q[2] for q in p], [q[3] for q in p])


@pytest.fixture(scope="module")
def mixed():
    problems = [(kernel_to_spec(treegp.eval_kernel(kern)),) + R.data_a(n) for kern, n in MIX]
    return problems, _call(problems)


def test_mixed_batch_against_the_single_problem_entry(mixed):
    problems, (log_det, chi2, g4, info) = mixed
    assert g4.shape == (5, 4) and not info.any()
    for b, (spec, X, y, y_err) in enumerate(problems):
        _, _, ref = single(spec, X, y, y_err)
        print("problem %d g4=%r single=%r" % (b, g4[b], ref))
        np.testing.assert_allclose(g4[b], ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max(), err_msg="problem %d" % b)
    _, ld, c2, inf = ops.gp_solve_batch([q[0] for q in problems], [q[1] for q in problems], [q[2] for q in problems],
                                        [q[3] for q in problems], want_alpha=True)
    assert np.array_equal(log_det, ld) and np.array_equal(chi2, c2) and np.array_equal(info, inf)


def test_mixed_batch_bits_do_not_depend_on_the_batch(mixed, monkeypatch):
    problems, (log_det, chi2, g4, info) = mixed
    monkeypatch.delenv("TGP_BATCH_CHUNK", raising=False)
    again = _call(problems)                                                    # run to run
    assert np.array_equal(again[2], g4) and np.array_equal(again[0], log_det) and np.array_equal(again[1], chi2)
    for b in range(len(problems)):                                             # alone: its own nmax and Np
        assert np.array_equal(_call(problems, [b])[2][0], g4[b]), "problem %d alone" % b
    rev = _call(problems, range(len(problems) - 1, -1, -1))
    assert np.array_equal(rev[2][::-1], g4)
    monkeypatch.setenv("TGP_BATCH_CHUNK", "1")
    assert np.array_equal(_call(problems)[2], g4)
    monkeypatch.delenv("TGP_BATCH_CHUNK")
    wide = problems + [(problems[2][0],) + R.data_a(700)]                       # a larger nmax: Np 512 -> 768
    assert np.array_equal(_call(wide)[2][:5], g4)


def test_one_bad_problem_leaves_the_others_alone(mixed):
    problems, (log_det, chi2, g4, info) = mixed
    for mid in (2, 0):                                                         # a von Karman problem, a Gaussian one
        bad = list(problems)
        spec, X, y, y_err = bad[mid]
        bad[mid] = (ops.KernelSpec(spec.kind, -spec.amp, spec.a, spec.b, spec.c, spec.ell), X, y, y_err)
        ld2, c2, g2, info2 = _call(bad)
        assert info2[mid] > 0
        keep = [b for b in range(len(problems)) if b != mid]
        assert not info2[keep].any()
        assert np.array_equal(g2[keep], g4[keep]) and np.array_equal(ld2[keep], log_det[keep]) and np.array_equal(c2[keep], chi2[keep])


# ---- 9. rejections and after-effects -----------------------------------------------------------------------------------------------
def test_rejections_and_the_context_afterwards():
    X, y, e = R.data_a(40)
    vk = kernel_to_spec(treegp.eval_kernel(R.SET_A["vk"]))
    unknown = ops.KernelSpec(17, amp=1.0, a=1.0, b=0.0, c=1.0)
    alpha, _, _, fac = ops.gp_solve(vk, X, y, e, keep=True)
    try:
        with pytest.raises(_lib.TgpError, match="tgp_gp_loglik_grad_any"):
            ops.gp_loglik_grad_any(unknown, fac, X, alpha)
        with pytest.raises(_lib.TgpError, match="Gaussian"):                   # the old entries answer as before, same process
            ops.gp_loglik_grad(vk, fac, X, alpha)
        before = ops.gp_loglik_grad_any(vk, fac, X, alpha)
    finally:
        fac.free()
    prob = ops.ResidentProblem(X, y, e)
    try:
        with pytest.raises(_lib.TgpError, match="tgp_d_gp_solve_grad_any"):
            ops.gp_solve_grad_resident_any(unknown, prob)
        with pytest.raises(_lib.TgpError, match="Gaussian"):
            ops.gp_solve_grad_resident(vk, prob)
        after = ops.gp_solve_grad_resident_any(vk, prob)
    finally:
        prob.close()
    assert np.array_equal(after[2], before)
    with pytest.raises(_lib.TgpError, match="tgp_gp_solve_grad_batch_any"):
        ops.gp_solve_grad_batch_any([vk, unknown], [X] * 2, [y] * 2, [e] * 2)
    with pytest.raises(_lib.TgpError, match=r"ks\[0\].*Gaussian"):
        ops.gp_solve_grad_batch([vk], [X], [y], [e])
    with pytest.raises(ValueError):
        ops.gp_solve_grad_batch_any([vk], [np.zeros((4097, 2))], [np.zeros(4097)])
    lib = _lib.load_library()
    ctx = _lib.get_ctx()
    ns = np.array([4097], dtype=np.int64)
    out = np.zeros(8)
    info = np.zeros(1, dtype=np.int32)
    ks = (_lib.TgpKernel * 1)(vk.to_c())
    big = np.zeros((4097, 2))
    rc = lib.tgp_gp_solve_grad_batch_any(ctx, 1, ctypes.cast(ks, ctypes.c_void_p), _lib.ptr(ns), 4097, _lib.ptr(big),
                                         _lib.ptr(big[:, 0].copy()), None, _lib.ptr(out), None, _lib.ptr(out[4:]), _lib.ptr(info))
    assert rc == -1 and b"nmax" in lib.tgp_last_error(ctx)
    ld, c2, g4, inf = ops.gp_solve_grad_batch_any([vk], [X], [y], [e])          # the context still works afterwards
    assert inf[0] == 0 and np.array_equal(g4[0], before)


# ---- 10. fits ----------------------------------------------------------------------------------------------------------------------
FITS = ["0.5**2 * VonKarman(length_scale=0.5)", "0.5**2 * AnisotropicVonKarman(invLam=array([[4., 0.], [0., 4.]]))"]


def _fit_object(kernel, n=200, seed=1):
    r = np.random.default_rng(seed)                                            # test_gpu_fit_many.py::test_mixed_list's data
    X = r.uniform(0, 1, (n, 2))
    y = np.sin(6 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.05 * r.standard_normal(n)
    gp = treegp.GPInterpolation(kernel=kernel, optimizer="log-likelihood", normalize=True)
    gp.initialize(X, y, y_err=0.05 * np.ones(n))
    return gp


def test_fits_with_the_exact_gradient_reach_the_finite_difference_optimum(monkeypatch):
    monkeypatch.setenv("TGP_ML_GRADIENT", "fd")
    refs = []
    for kern in FITS:
        gp = _fit_object(kern)
        gp.solve()                                                             # the finite-difference route, as before
        refs.append(gp._optimizer._logL)
    many = [_fit_object(kern) for kern in FITS]
    calls = []
    real = ops.gp_solve_grad_batch_any
    monkeypatch.setattr(ops, "gp_solve_grad_batch_any", lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1])
    treegp.solve_many(many, gradient="analytic-vk")
    assert len(calls) >= 3 and calls[0] == 2
    monkeypatch.setenv("TGP_ML_GRADIENT", "analytic-vk")
    for kern, gp, ref in zip(FITS, many, refs):
        print("%s: solve_many logL=%r fd logL=%r" % (kern, gp._optimizer._logL, ref))
        assert gp._optimizer._logL >= ref - 1e-6 * abs(ref), (kern, gp._optimizer._logL, ref)
        own = _fit_object(kern)
        own.solve()
        assert own._optimizer.gradient == "analytic-vk"
        print("%s: solve() logL=%r" % (kern, own._optimizer._logL))
        assert own._optimizer._logL >= ref - 1e-6 * abs(ref), (kern, own._optimizer._logL, ref)
    rng = np.random.default_rng(11)
    Xq = [rng.uniform(0, 1, (50, 2)) for _ in many]
    out = treegp.predict_many(many, Xq, return_var=True)
    for yq, var in out:
        assert yq.shape == (50,) and var.shape == (50,) and np.all(np.isfinite(yq)) and np.all(np.isfinite(var))

"""GPU tests of the batched likelihood gradient (include/tgp.h seam S2f, ops.gp_solve_grad_batch) and of the lockstep fits built
on it (treegp_amd.solve_many)."""
import ctypes

import numpy as np
import pytest

import treegp_amd as treegp
from treegp_amd import _lib, ops
from treegp_amd.kernels import kernel_to_spec

pytestmark = pytest.mark.gpu

# one point, partial tiles, one past a tile, one past a panel, one past a 1024 block: all under one Np, each with its own n_b
RAGGED_NS = [1, 2, 63, 128, 129, 255, 256, 257, 300, 513, 1025]
KERNELS = [(2, "AnisotropicRBF(invLam=array([[40., -9.], [-9., 25.]]))"), (1, "AnisotropicRBF(scale_length=[0.2])"),
           (2, "RBF(0.07)")]


def _problem(b, n):
    nd, kern = KERNELS[b % len(KERNELS)]
    rng = np.random.default_rng(500 + n)
    X = rng.uniform(0, 1, (n, nd))
    y = np.sin(5 * X[:, 0]) + 0.1 * rng.standard_normal(n)
    y_err = 0.1 * rng.uniform(0.8, 1.2, n)
    spec = kernel_to_spec(treegp.eval_kernel("%r**2 * %s" % (0.6 + 0.05 * b, kern)))
    return nd, spec, X, y, y_err


def _oracle_gradient(nd, spec, X, y, y_err):
    from oracle import gp_oracle as O
    invLam = np.array([[spec.a, spec.b], [spec.b, spec.c]])[:nd, :nd]
    basis = [np.array([[1.0, 0], [0, 0]])[:nd, :nd], np.array([[0, 1.0], [1.0, 0]])[:nd, :nd], np.array([[0, 0], [0, 1.0]])[:nd, :nd]]
    g_amp, g_abc = O.loglik_grad_invlam(X, y, y_err, spec.amp, invLam, basis)
    return np.concatenate([[g_amp], g_abc])


def _call(problems, order=None):
    order = list(range(len(problems))) if order is None else list(order)
    p = [problems[i] for i in order]
    return ops.gp_solve_grad_batch([q[1] for q in p], [q[2] for q in p], [q[3] for q in p], [q[4] for q in p])


@pytest.fixture(scope="module")
def ragged():
    problems = [_problem(b, n) for b, n in enumerate(RAGGED_NS)]
    return problems, _call(problems)


def test_ragged_batch_against_the_oracle(ragged):
    problems, (log_det, chi2, g4, info) = ragged
    assert g4.shape == (len(RAGGED_NS), 4) and not info.any()
    for b, (nd, spec, X, y, y_err) in enumerate(problems):
        ref = _oracle_gradient(nd, spec, X, y, y_err)
        np.testing.assert_allclose(g4[b], ref, rtol=1e-8, atol=1e-8 * max(np.abs(ref).max(), 1.0),
                                   err_msg="problem %d n=%d nd=%d" % (b, len(X), nd))


def test_same_bits_as_the_batched_solve(ragged):
    problems, (log_det, chi2, g4, info) = ragged
    _, ld, c2, inf = ops.gp_solve_batch([q[1] for q in problems], [q[2] for q in problems], [q[3] for q in problems],
                                        [q[4] for q in problems], want_alpha=True)
    assert np.array_equal(log_det, ld) and np.array_equal(chi2, c2) and np.array_equal(info, inf)


def test_gradient_bits_do_not_depend_on_the_batch(ragged, monkeypatch):
    problems, (log_det, chi2, g4, info) = ragged
    monkeypatch.delenv("TGP_BATCH_CHUNK", raising=False)
    again = _call(problems)                                                    # run to run
    assert np.array_equal(again[2], g4) and np.array_equal(again[0], log_det) and np.array_equal(again[1], chi2)
    for b in range(len(problems)):                                             # alone: its own nmax and Np
        assert np.array_equal(_call(problems, [b])[2][0], g4[b]), "problem %d alone" % b
    rev = _call(problems, range(len(problems) - 1, -1, -1))
    assert np.array_equal(rev[2][::-1], g4)
    for chunk in ("1", "3"):
        monkeypatch.setenv("TGP_BATCH_CHUNK", chunk)
        assert np.array_equal(_call(problems)[2], g4), "TGP_BATCH_CHUNK=%s" % chunk


def test_one_bad_problem_leaves_the_others_alone(ragged):
    problems, (log_det, chi2, g4, info) = ragged
    mid = len(problems) // 2
    bad = list(problems)
    nd, spec, X, y, y_err = bad[mid]
    bad[mid] = (nd, ops.KernelSpec(spec.kind, -spec.amp, spec.a, spec.b, spec.c), X, y, y_err)
    ld2, c2, g2, info2 = _call(bad)
    assert info2[mid] > 0
    keep = [b for b in range(len(problems)) if b != mid]
    assert not info2[keep].any()
    assert np.array_equal(g2[keep], g4[keep]) and np.array_equal(ld2[keep], log_det[keep]) and np.array_equal(c2[keep], chi2[keep])


def test_large_tiles_against_the_single_problem_gradient():
    """ns = [2049, 4096]: the deepest sums and the largest tile grids of the batched route, against tgp_gp_loglik_grad alone"""
    spec = kernel_to_spec(treegp.eval_kernel("1.0**2 * AnisotropicRBF(invLam=array([[300., 40.], [40., 200.]]))"))
    probs = []
    for n in (2049, 4096):
        rng = np.random.default_rng(n)
        X = rng.uniform(0, 1, (n, 2))
        probs.append((X, rng.standard_normal(n), 0.1 * np.ones(n)))
    _, _, g4, info = ops.gp_solve_grad_batch([spec, spec], [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs])
    assert not info.any()
    for b, (X, y, y_err) in enumerate(probs):
        alpha, _, _, fac = ops.gp_solve(spec, X, y, y_err, keep=True)
        try:
            ref = ops.gp_loglik_grad(spec, fac, X, alpha)
        finally:
            fac.free()
        np.testing.assert_allclose(g4[b], ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max(), err_msg="n=%d" % len(X))


def test_rejections():
    rng = np.random.default_rng(2)
    X = rng.uniform(0, 1, (40, 2))
    y = rng.standard_normal(40)
    e = 0.1 * np.ones(40)
    gauss = kernel_to_spec(treegp.eval_kernel("1.0**2 * RBF(0.3)"))
    vk = kernel_to_spec(treegp.eval_kernel("1.0**2 * VonKarman(length_scale=0.3)"))
    with pytest.raises(_lib.TgpError, match=r"ks\[2\].*Gaussian"):
        ops.gp_solve_grad_batch([gauss, gauss, vk, gauss], [X] * 4, [y] * 4, [e] * 4)
    with pytest.raises(ValueError):
        ops.gp_solve_grad_batch([gauss], [np.zeros((4097, 2))], [np.zeros(4097)])
    lib = _lib.load_library()
    ctx = _lib.get_ctx()
    ns = np.array([4097], dtype=np.int64)
    out = np.zeros(8)
    info = np.zeros(1, dtype=np.int32)
    ks = (_lib.TgpKernel * 1)(gauss.to_c())
    big = np.zeros((4097, 2))
    rc = lib.tgp_gp_solve_grad_batch(ctx, 1, ctypes.cast(ks, ctypes.c_void_p), _lib.ptr(ns), 4097, _lib.ptr(big), _lib.ptr(big[:, 0].copy()), None, _lib.ptr(out),
                                     None, _lib.ptr(out[4:]), _lib.ptr(info))
    assert rc == -1 and b"nmax" in lib.tgp_last_error(ctx)
    # the single-problem entry keeps rejecting the von Karman kinds as before
    alpha, _, _, fac = ops.gp_solve(vk, X, y, e, keep=True)
    try:
        with pytest.raises(_lib.TgpError, match="Gaussian"):
            ops.gp_loglik_grad(vk, fac, X, alpha)
    finally:
        fac.free()
    ld, c2, g4, inf = ops.gp_solve_grad_batch([gauss], [X], [y], [e])              # the context still works afterwards
    assert inf[0] == 0 and np.all(np.isfinite(g4))


def _g11_objects(g):
    gps = []
    for tag, yerr in (("rbf1d", 0.01), ("arbf2d", 0.02), ("rbf1d", 0.01)):
        gp = treegp.GPInterpolation(kernel=str(g[tag + "_kernel0"]), optimizer="log-likelihood", normalize=True)
        gp.initialize(g[tag + "_X"], g[tag + "_y"], y_err=yerr * np.ones(len(g[tag + "_y"])))
        gps.append((tag, gp))
    return gps


@pytest.mark.parametrize("gradient", ["auto", "fd"])
def test_fits_reach_the_reference_optimum(golden, gradient):
    """g11: the reference's fits; the lockstep fits end at the same optimum, and two copies of one object at the same bits"""
    g = golden("g11_ml_fit.npz")
    objs = _g11_objects(g)
    treegp.solve_many([gp for _, gp in objs], gradient=gradient)
    for tag, gp in objs:
        ref_l = float(g[tag + "_logL"])
        assert gp._optimizer._logL >= ref_l - 1e-6 * abs(ref_l), (tag, gp._optimizer._logL, ref_l)
        np.testing.assert_allclose(gp.kernel.theta, g[tag + "_theta"], atol=2e-3)
        assert gp._alpha is None and len(gp._init_theta) == 1
    assert np.array_equal(objs[0][1].kernel.theta, objs[2][1].kernel.theta)
    assert objs[0][1]._optimizer._logL == objs[2][1]._optimizer._logL


def test_mixed_list():
    """von Karman through the batched finite differences, Matern through its own solve(), "none" untouched, Gaussian ones
    through the batched gradient; predict_many then serves the whole list"""
    rng = np.random.default_rng(11)

    def make(kernel, optimizer, n, seed):
        r = np.random.default_rng(seed)
        X = r.uniform(0, 1, (n, 2))
        y = np.sin(6 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.05 * r.standard_normal(n)
        gp = treegp.GPInterpolation(kernel=kernel, optimizer=optimizer, normalize=True)
        gp.initialize(X, y, y_err=0.05 * np.ones(n))
        return gp
    vk = make("0.5**2 * VonKarman(length_scale=0.5)", "log-likelihood", 200, 1)
    vk_alone = make("0.5**2 * VonKarman(length_scale=0.5)", "log-likelihood", 200, 1)
    matern = make("0.5**2 * Matern(length_scale=0.3, nu=1.5)", "log-likelihood", 150, 2)
    fixed = make("0.5**2 * RBF(0.2)", "none", 300, 3)
    g1 = make("0.5**2 * RBF(0.3)", "log-likelihood", 600, 4)
    g2 = make("0.5**2 * AnisotropicRBF(invLam=array([[20., 0.], [0., 20.]]))", "log-likelihood", 257, 5)
    gps = [g1, vk, matern, fixed, g2]
    fixed_theta = fixed.kernel.theta.copy()
    l0 = [gp.return_log_likelihood() for gp in (g1, g2)]
    calls = {"grad": 0, "own": []}
    real_grad, real_solve = ops.gp_solve_grad_batch, treegp.GPInterpolation.solve

    def counted(*a, **k):
        calls["grad"] += 1
        return real_grad(*a, **k)

    def own_solve(self):
        calls["own"].append(self)
        return real_solve(self)
    ops.gp_solve_grad_batch, treegp.GPInterpolation.solve = counted, own_solve
    try:
        treegp.solve_many(gps)
    finally:
        ops.gp_solve_grad_batch, treegp.GPInterpolation.solve = real_grad, real_solve
    assert calls["own"] == [matern, fixed] and calls["grad"] >= 3
    assert np.array_equal(fixed.kernel.theta, fixed_theta)
    assert "Matern" in repr(matern.kernel) and np.isfinite(matern._optimizer._logL)
    for gp, start in zip((g1, g2), l0):
        assert gp._optimizer._logL > start
    vk_alone.solve()
    ref = vk_alone._optimizer._logL
    assert vk._optimizer._logL >= ref - 1e-6 * abs(ref), (vk._optimizer._logL, ref)
    Xq = [rng.uniform(0, 1, (50, 2)) for _ in gps]
    out = treegp.predict_many(gps, Xq, return_var=True)
    assert len(out) == len(gps)
    for (yq, var), gp, X in zip(out, gps, Xq):
        assert yq.shape == (50,) and var.shape == (50,) and np.all(np.isfinite(yq)) and np.all(np.isfinite(var))

"""Batched solves of many small GPs (tgp_gp_solve_batch, ops.gp_solve_batch, log_likelihood_many, predict_many) on the GPU:
against the oracle and the single solve at DESIGN.md §5's tolerances, bit-independence of a problem from its batch, failure
isolation, the reference's goldens and the C-ABI's argument errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import treegp_amd as treegp
from treegp_amd import _lib, ops
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"rbf": ("gauss", _lib.TGP_RBF), "arbf": ("gauss", _lib.TGP_ARBF), "vk": ("vk", _lib.TGP_VK), "avk": ("avk", _lib.TGP_AVK)}


def problem(kind, n, dim, with_err, seed):
    """(spec, oracle kind, oracle kwargs, X, y, y_err or None): points with unit mean spacing, correlation lengths of a few
    spacings with noise, below one spacing without (well-conditioned either way)"""
    rng = np.random.default_rng(seed)
    side = n ** (1.0 / dim)
    X = rng.uniform(0.0, side, (n, dim))
    ell = rng.uniform(2.0, 4.0) if with_err else rng.uniform(0.2, 0.4)
    amp = rng.uniform(0.5, 2.0)
    if kind == "rbf":
        kw = dict(amp=amp, a=1.0 / ell ** 2, b=0.0, c=1.0 / ell ** 2)
    elif kind in ("arbf", "avk"):
        a, c = 1.0 / ell ** 2, 1.0 / (1.3 * ell) ** 2
        kw = dict(amp=amp, a=a, b=0.3 * np.sqrt(a * c), c=c)
    else:
        kw = dict(amp=amp, ell=ell)
    okind, ckind = KINDS[kind]
    spec = ops.KernelSpec(ckind, **kw)
    y = np.sin(X[:, 0]) + 0.3 * rng.standard_normal(n)
    e = rng.uniform(0.1, 0.3, n) if with_err else None
    return spec, okind, kw, X, y, e


def mixed_batch(ns, seed0, with_err=True):
    kinds = ["rbf", "arbf", "vk", "avk"]
    return [problem(kinds[i % 4], n, 1 + (i % 2), with_err, seed0 + i) for i, n in enumerate(ns)]


def run(batch, want_alpha=True, ctx=None):
    errs = [p[5] for p in batch]
    y_errs = None if all(e is None for e in errs) else [np.zeros(len(p[4])) if p[5] is None else p[5] for p in batch]
    return ops.gp_solve_batch([p[0] for p in batch], [p[3] for p in batch], [p[4] for p in batch], y_errs,
                              want_alpha=want_alpha, ctx=ctx)


def oracle(p):
    spec, okind, kw, X, y, e = p
    K = O.kernel_matrix(okind, X, **kw)
    ee = np.zeros(len(y)) if e is None else e
    alpha, logdet = O.gp_solve(K, y, ee)
    return alpha, logdet, O.log_likelihood(K, y, ee)


def loglike(n, logdet, chi2):
    return -0.5 * chi2 - 0.5 * n * np.log(2.0 * np.pi) - 0.5 * logdet


def test_oracle_and_single_solve_on_a_ragged_mixed_batch():
    ns = [1, 40, 255, 256, 700, 1024, 4096, 300, 1, 129]
    batch = mixed_batch(ns, 11)
    batch[7] = problem("vk", 300, 2, False, 99)               # without errors: short correlation length
    batch[8] = problem("arbf", 1, 1, False, 98)
    batch[9] = problem("rbf", 129, 1, False, 97)
    alphas, logdets, chi2, info = run(batch)
    assert list(info) == [0] * len(ns)
    for b, p in enumerate(batch):
        n = len(p[4])
        assert alphas[b].shape == (n,)
        a_ref, ld_ref, ll_ref = oracle(p)
        tag = "problem %d (n = %d)" % (b, n)
        np.testing.assert_allclose(alphas[b], a_ref, rtol=0, atol=1e-9 * np.abs(a_ref).max(), err_msg=tag)
        np.testing.assert_allclose(chi2[b], np.dot(p[4], a_ref), rtol=1e-11, err_msg=tag)
        np.testing.assert_allclose(loglike(n, logdets[b], chi2[b]), ll_ref, rtol=1e-11, err_msg=tag)
        a1, ld1, c1, _ = ops.gp_solve(p[0], p[3], p[4], p[5])
        np.testing.assert_allclose(alphas[b], a1, rtol=0, atol=1e-9 * np.abs(a1).max(), err_msg=tag)
        np.testing.assert_allclose(loglike(n, logdets[b], chi2[b]), loglike(n, ld1, c1), rtol=1e-11, err_msg=tag)
    # the likelihood-only route (no backward sweep) gives the same logdet and chi2 bits
    none, ld2, c2, info2 = run(batch, want_alpha=False)
    assert none is None and list(info2) == [0] * len(ns)
    assert np.array_equal(ld2, logdets) and np.array_equal(c2, chi2)


N_FIXED = 1000


def fixed_problem():
    return problem("arbf", N_FIXED, 2, True, 4242)


def companions(seed, count):
    rng = np.random.default_rng(seed)
    ns = rng.integers(1, N_FIXED + 1, count)
    return mixed_batch(list(ns), seed * 1000)


def outputs_of(batch, b):
    alphas, logdets, chi2, info = run(batch)
    return alphas[b], logdets[b], chi2[b], info[b]


def same_bits(u, v):
    assert np.array_equal(u[0], v[0]) and u[1] == v[1] and u[2] == v[2] and u[3] == v[3] == 0


def test_a_problem_does_not_depend_on_its_batch_bit_for_bit():
    P = fixed_problem()
    A, B = companions(5, 63), companions(6, 63)
    alone = outputs_of([P], 0)
    same_bits(outputs_of([P] + A, 0), alone)
    same_bits(outputs_of(A[:31] + [P] + A[31:], 31), alone)
    same_bits(outputs_of(A + [P], 63), alone)
    same_bits(outputs_of(B[:31] + [P] + B[31:], 31), alone)
    # problems of one kind next to others of other kinds: the companions' results are theirs alone as well
    mixed = outputs_of(A[:31] + [P] + A[31:], 5)
    same_bits(outputs_of([A[5]] + [P], 0), mixed)


CHUNK_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_solve_batch as T
P = T.fixed_problem()
A = T.companions(5, 63)
alphas, logdets, chi2, info = T.run(A[:31] + [P] + A[31:])
np.savez(%r, alpha=np.concatenate(alphas), logdet=logdets, chi2=chi2, info=info)
print("OK")
'''


def test_chunking_does_not_change_a_bit(tmp_path):
    results = []
    for chunk in ("1", "3", None):
        out = str(tmp_path / ("chunk_%s.npz" % chunk))
        env = dict(os.environ)
        env.pop("TGP_BATCH_CHUNK", None)
        if chunk is not None:
            env["TGP_BATCH_CHUNK"] = chunk
        code = CHUNK_SCRIPT % (ROOT, os.path.join(ROOT, "tests"), out)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "OK" in r.stdout, (chunk, r.stdout[-500:], r.stderr[-1500:])
        results.append(np.load(out))
    for r in results[1:]:
        for key in ("alpha", "logdet", "chi2", "info"):
            assert np.array_equal(r[key], results[0][key]), key
    alone = outputs_of([fixed_problem()], 0)
    assert results[0]["logdet"][31] == alone[1] and results[0]["chi2"][31] == alone[2]


def test_a_singular_problem_fails_alone():
    good = mixed_batch([300, 513, 64, 1000, 257], 77)
    rng = np.random.default_rng(1)
    Xs = np.tile(rng.uniform(0, 10, (10, 2)), (20, 1))        # ten points, each twenty times, no noise: K has rank 10
    bad = (ops.KernelSpec(_lib.TGP_RBF, amp=1.0, a=0.25, b=0.0, c=0.25), "gauss", {}, Xs, rng.standard_normal(200), None)
    ref = run(good)
    with_bad = run(good[:2] + [bad] + good[2:])
    assert with_bad[3][2] > 0 and list(np.delete(with_bad[3], 2)) == [0] * 5
    for b, bb in zip(range(5), [0, 1, 3, 4, 5]):
        assert np.array_equal(ref[0][b], with_bad[0][bb])
        assert ref[1][b] == with_bad[1][bb] and ref[2][b] == with_bad[2][bb]


def test_goldens_through_the_batched_routes(golden):
    g = golden("g5_loglike.npz")
    gp = treegp.GPInterpolation(kernel=str(g["kernel"]), optimizer="none", normalize=True)
    gp.initialize(g["X"], g["y"], y_err=g["y_err"])
    like = treegp.log_likelihood(gp._X, gp._residual(), gp._y_err)
    kernels = [gp.kernel.clone_with_theta(t) for t in g["thetas"]]
    np.testing.assert_allclose(like.log_likelihood_many(kernels), g["logL"], rtol=1e-11)
    # the zero-error data of the same test: its singular kernel and a well-conditioned one
    gp2 = treegp.GPInterpolation(kernel="1.0**2 * AnisotropicRBF(scale_length=[50., 50.])", optimizer="none", normalize=False)
    gp2.initialize(g["X"], g["y"], y_err=np.zeros(len(g["y"])))
    like2 = treegp.log_likelihood(gp2._X, gp2._residual(), gp2._y_err)
    sharp = treegp.eval_kernel("1.0**2 * AnisotropicRBF(scale_length=[0.01, 0.01])")
    ll = like2.log_likelihood_many([gp2.kernel, sharp])
    assert ll[0] == -np.inf == float(g["logL_singular"]) and np.isfinite(ll[1])
    assert ll[1] == like2.log_likelihood(sharp) or abs(ll[1] - like2.log_likelihood(sharp)) <= 1e-11 * abs(ll[1])

    g1, g2 = golden("g1_c1_rbf1d.npz"), golden("g2_aniso2d.npz")
    a = treegp.GPInterpolation(kernel=str(g1["kernel"]), optimizer="none", normalize=True, white_noise=0.0)
    a.initialize(g1["X"], g1["y"], y_err=g1["y_err"])
    b = treegp.GPInterpolation(kernel=str(g2["kernel"]), optimizer="none", normalize=True, white_noise=0.01)
    b.initialize(g2["X"], g2["y"], y_err=g2["y_err"])
    preds = treegp.predict_many([a, b], [g1["Xs"], g2["Xs"]])
    for p, gg in zip(preds, (g1, g2)):
        np.testing.assert_allclose(p, gg["y_pred"], rtol=0, atol=1e-10 * np.abs(gg["y_pred"]).max())
    cached = a._alpha
    assert cached is not None and b._alpha is not None

    def no_solve(*args, **kw):
        raise AssertionError("predict solved again")
    import treegp_amd.gp_interp as gi
    orig = gi.ops.gp_solve
    gi.ops.gp_solve = no_solve
    try:
        np.testing.assert_allclose(a.predict(g1["Xs"]), preds[0], rtol=0, atol=0)
    finally:
        gi.ops.gp_solve = orig
    assert a._alpha is cached


def test_argument_errors_of_the_c_abi():
    lib = _lib.load_library()
    ctx = _lib.get_ctx()
    X = np.zeros((2, 4097, 2))
    y = np.zeros((2, 4097))
    out = np.zeros(2)
    info = np.zeros(2, dtype=np.int32)
    good = ops.KernelSpec(_lib.TGP_RBF).to_c()

    def call(ns, nmax, kinds=(0, 0), nb=2):
        ks = (_lib.TgpKernel * 2)(good, good)
        for i, k in enumerate(kinds):
            ks[i].kind = k
        ns = np.asarray(ns, dtype=np.int64)
        rc = lib.tgp_gp_solve_batch(ctx, nb, C.cast(ks, C.c_void_p), _lib.ptr(ns), nmax, _lib.ptr(X), _lib.ptr(y), None, None,
                                    _lib.ptr(out), None, _lib.ptr(info))
        return rc, (lib.tgp_last_error(ctx) or b"").decode()

    for args in (([10, 10], 4097), ([0, 10], 10), ([10, 11], 10), ([10, 10], 10, (0, 7)), ([10, 10], 10, (0, 0), 0)):
        rc, msg = call(*args)
        assert rc == -1 and "tgp_gp_solve_batch" in msg, (args, rc, msg)
    rc, msg = call([10, 10], 10)
    assert rc == 0                                  # (all points at one place without noise: both problems report info > 0)
    assert info[0] > 0 and info[1] > 0
    with pytest.raises(ValueError):
        ops.gp_solve_batch([ops.KernelSpec(0)], [np.zeros((5000, 2))], [np.zeros(5000)])


def test_c_abi_ignores_rows_beyond_n_and_zeroes_alpha_there():
    """Direct call on a ragged batch: rows >= ns[b] of X, y and yerr hold NaN and are not read; alpha is exactly 0 there and
    the rest is what ops.gp_solve_batch returns; the timing slots the call does not fill are 0."""
    batch = mixed_batch([5, 300, 129, 256, 1], 31)
    ns = np.array([len(p[4]) for p in batch], dtype=np.int64)
    nb, nmax = len(batch), int(ns.max())
    X = np.full((nb, nmax, 2), np.nan)
    y = np.full((nb, nmax), np.nan)
    e = np.full((nb, nmax), np.nan)
    for b, p in enumerate(batch):
        X[b, :ns[b]] = _lib.as_xy(p[3])
        y[b, :ns[b]] = p[4]
        e[b, :ns[b]] = p[5]
    alpha = np.full((nb, nmax), np.nan)
    logdet, chi2 = np.empty(nb), np.empty(nb)
    info = np.full(nb, -1, dtype=np.int32)
    ks = (_lib.TgpKernel * nb)(*[p[0].to_c() for p in batch])
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    ops.gp_solve(batch[0][0], batch[0][3], batch[0][4], batch[0][5])       # a single solve fills other timing slots first
    rc = lib.tgp_gp_solve_batch(ctx, nb, C.cast(ks, C.c_void_p), _lib.ptr(ns), nmax, _lib.ptr(X), _lib.ptr(y), _lib.ptr(e),
                                _lib.ptr(alpha), _lib.ptr(logdet), _lib.ptr(chi2), _lib.ptr(info))
    assert rc == 0 and list(info) == [0] * nb
    tm = _lib.timings(ctx)
    assert tm[1] > 0 and tm[10] == 2 and all(tm[i] == 0 for i in range(len(tm)) if i not in (0, 1, 2, 10))
    alphas, ld2, c2, _ = run(batch)
    for b in range(nb):
        assert np.array_equal(alpha[b, :ns[b]], alphas[b])
        assert np.all(alpha[b, ns[b]:] == 0.0) and not np.signbit(alpha[b, ns[b]:]).any()
    assert np.array_equal(logdet, ld2) and np.array_equal(chi2, c2)

"""Posterior variance and covariance of many small GPs in one batch (tgp_gp_posterior_batch, ops.gp_posterior_batch,
predict_many(..., return_var / return_cov)) on the GPU: against the oracle and the single route on a kept factor, the
batched solve's bits, bit-independence of a problem from its batch and the chunking, failure isolation, the reference's
goldens, mixed lists of objects and the C-ABI's contract."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import treegp_amd as treegp
from treegp_amd import _lib, ops
from oracle import gp_oracle as O

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
from test_gpu_solve_batch import problem, mixed_batch  # noqa: E402  (the batched solve's problem generator)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(TESTS)


def queries(p, m, seed):
    """m query points in the problem's box (its dimension)"""
    X = p[3]
    rng = np.random.default_rng(seed)
    return rng.uniform(X.min(axis=0) - 0.5, X.max(axis=0) + 0.5, (m, X.shape[1]))


def errs(batch):
    es = [p[5] for p in batch]
    return None if all(e is None for e in es) else [np.zeros(len(p[4])) if p[5] is None else p[5] for p in batch]


def post(batch, Xq, what):
    return ops.gp_posterior_batch([p[0] for p in batch], [p[3] for p in batch], [p[4] for p in batch], errs(batch), Xq, what=what)


def solve(batch):
    return ops.gp_solve_batch([p[0] for p in batch], [p[3] for p in batch], [p[4] for p in batch], errs(batch))


def oracle_cov(p, Xq):
    spec, okind, kw, X, y, e = p
    K = O.kernel_matrix(okind, X, **kw)
    HT = O.kernel_matrix(okind, Xq, X, **kw)
    Kss = O.kernel_matrix(okind, Xq, **kw)
    return O.gp_predict_cov(K, np.zeros(len(y)) if e is None else e, HT, Kss)


def test_oracle_single_route_and_solve_bits_on_a_ragged_mixed_batch():
    ns = [1, 40, 255, 256, 700, 1024, 4096, 129]
    ms = [3, 1000, 1, 257, 256, 255, 1000, 3]
    batch = mixed_batch(ns, 21)
    batch[3] = problem("vk", 256, 2, False, 91)             # without errors: short correlation length
    batch[7] = problem("rbf", 129, 1, False, 92)
    Xq = [queries(p, m, 500 + b) for b, (p, m) in enumerate(zip(batch, ms))]
    av, var, ldv, c2v, infov = post(batch, Xq, "var")
    ac, cov, ldc, c2c, infoc = post(batch, Xq, "cov")
    a0, ld0, c20, info0 = solve(batch)
    assert list(info0) == [0] * len(ns)
    for r in ((av, ldv, c2v, infov), (ac, ldc, c2c, infoc)):
        assert all(np.array_equal(u, v) for u, v in zip(r[0], a0))
        assert np.array_equal(r[1], ld0) and np.array_equal(r[2], c20) and np.array_equal(r[3], info0)
    for b, (p, m) in enumerate(zip(batch, ms)):
        amp, tag = p[0].amp, "problem %d (n = %d, m = %d)" % (b, len(p[4]), m)
        assert var[b].shape == (m,) and cov[b].shape == (m, m)
        ref = oracle_cov(p, Xq[b])
        np.testing.assert_allclose(cov[b], ref, rtol=0, atol=1e-10 * amp, err_msg=tag)
        np.testing.assert_allclose(var[b], np.diag(ref), rtol=0, atol=1e-10 * amp, err_msg=tag)
        np.testing.assert_allclose(var[b], np.diag(cov[b]), rtol=0, atol=1e-12 * amp, err_msg=tag)
        _, _, _, f = ops.gp_solve(p[0], p[3], p[4], p[5], keep=True)
        try:
            np.testing.assert_allclose(cov[b], ops.gp_predict_cov(p[0], f, p[3], Xq[b]), rtol=0, atol=1e-12 * amp, err_msg=tag)
            np.testing.assert_allclose(var[b], ops.gp_predict_var(p[0], f, p[3], Xq[b]), rtol=0, atol=1e-12 * amp, err_msg=tag)
        finally:
            f.free()


N_FIXED, M_FIXED, NMAX, MMAX = 1000, 300, 1024, 512     # every batch below pads to Np = 1024 and Mp = 512


def fixed_problem():
    p = problem("avk", N_FIXED, 2, True, 4343)
    return p, queries(p, M_FIXED, 4344)


def companions(seed, count):
    """count problems of order <= NMAX with at most MMAX query points each"""
    rng = np.random.default_rng(seed)
    batch = mixed_batch(list(rng.integers(1, NMAX + 1, count)), seed * 1000)
    ms = rng.integers(1, MMAX + 1, count)
    return batch, [queries(p, int(m), seed + i) for i, (p, m) in enumerate(zip(batch, ms))]


def bits_of(batch, Xq, b):
    _, var, _, _, info_v = post(batch, Xq, "var")
    _, cov, _, _, info_c = post(batch, Xq, "cov")
    assert info_v[b] == 0 and info_c[b] == 0
    return var[b], cov[b]


def same(u, v):
    assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])


def test_a_problem_does_not_depend_on_its_batch_bit_for_bit():
    P, Pq = fixed_problem()
    A, Aq = companions(7, 63)
    alone = bits_of([P], [Pq], 0)
    same(bits_of([P] + A, [Pq] + Aq, 0), alone)
    same(bits_of(A[:31] + [P] + A[31:], Aq[:31] + [Pq] + Aq[31:], 31), alone)
    same(bits_of(A + [P], Aq + [Pq], 63), alone)


CHUNK_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_predict_batch as T
P, Pq = T.fixed_problem()
A, Aq = T.companions(7, 63)
_, var, _, _, iv = T.post(A[:31] + [P] + A[31:], Aq[:31] + [Pq] + Aq[31:], "var")
_, cov, _, _, ic = T.post(A[:31] + [P] + A[31:], Aq[:31] + [Pq] + Aq[31:], "cov")
np.savez(%r, var=np.concatenate(var), cov=np.concatenate([c.ravel() for c in cov]), iv=iv, ic=ic)
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
        code = CHUNK_SCRIPT % (ROOT, TESTS, out)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "OK" in r.stdout, (chunk, r.stdout[-500:], r.stderr[-1500:])
        results.append(np.load(out))
    assert list(results[0]["iv"]) == [0] * 64 and list(results[0]["ic"]) == [0] * 64
    for r in results[1:]:
        for key in ("var", "cov", "iv", "ic"):
            assert np.array_equal(r[key], results[0][key]), key
    P, Pq = fixed_problem()
    var, cov = bits_of([P], [Pq], 0)
    A, Aq = companions(7, 63)
    off_v = sum(len(q) for q in Aq[:31])
    off_c = sum(len(q) ** 2 for q in Aq[:31])
    assert np.array_equal(results[0]["var"][off_v:off_v + M_FIXED], var)
    assert np.array_equal(results[0]["cov"][off_c:off_c + M_FIXED ** 2], cov.ravel())


def test_a_singular_problem_fails_alone():
    good = mixed_batch([300, 513, 64, 1000, 257], 78)
    gq = [queries(p, m, 60 + i) for i, (p, m) in enumerate(zip(good, [5, 300, 257, 1, 100]))]
    rng = np.random.default_rng(2)
    Xs = np.tile(rng.uniform(0, 10, (10, 2)), (20, 1))        # ten points, each twenty times, no noise: K has rank 10
    bad = (ops.KernelSpec(_lib.TGP_RBF, amp=1.0, a=0.25, b=0.0, c=0.25), "gauss", {}, Xs, rng.standard_normal(200), None)
    bq = rng.uniform(0, 10, (40, 2))
    for what in ("var", "cov"):
        ref = post(good, gq, what)
        with_bad = post(good[:2] + [bad] + good[2:], gq[:2] + [bq] + gq[2:], what)
        assert with_bad[4][2] > 0 and list(np.delete(with_bad[4], 2)) == [0] * 5
        for b, bb in zip(range(5), [0, 1, 3, 4, 5]):
            assert np.array_equal(ref[1][b], with_bad[1][bb]), (what, b)
            assert np.array_equal(ref[0][b], with_bad[0][bb]) and ref[2][b] == with_bad[2][bb] and ref[3][b] == with_bad[3][bb]


def golden_objects(golden):
    """(gp, X, cov golden) of test_gpu_api's covariance goldens: g2 (AnisotropicRBF), g3 (von Karman, both), g8 (RBF and
    von Karman, at the data and far from it)"""
    out = []
    g = golden("g2_aniso2d.npz")
    gp = treegp.GPInterpolation(kernel=str(g["kernel"]), optimizer="none", normalize=True, white_noise=0.01)
    gp.initialize(g["X"], g["y"], y_err=g["y_err"])
    out.append((gp, g["Xs"][:256], g["cov256"]))
    g = golden("g3_vonkarman.npz")
    for tag in ("vk", "avk"):
        gp = treegp.GPInterpolation(kernel=str(g[tag + "_kernel"]), optimizer="none", normalize=True)
        gp.initialize(g["X"], g["y"], y_err=g["y_err"])
        out.append((gp, g["Xs"][:200], g[tag + "_cov200"]))
    g = golden("g8_reftests.npz")
    x = g["x"]
    for tag in ("rbf", "vk"):
        kern = str(g[tag + "_kernel"])
        gp = treegp.GPInterpolation(kernel=kern, optimizer="none", white_noise=0.0)
        gp.initialize(x, g[tag + "_y"], y_err=0.1 * np.ones(len(x)))
        out.append((gp, x, g[tag + "_cov"]))
        gpb = treegp.GPInterpolation(kernel=kern, optimizer="none", normalize=False, white_noise=0.0)
        gpb.initialize(x, g[tag + "_y"], y_err=0.1 * np.ones(len(x)))
        out.append((gpb, g[tag + "_new_x"], g[tag + "_cov_far"]))
    return out


def test_goldens_through_predict_many(golden):
    objs = golden_objects(golden)
    gps, Xs = [o[0] for o in objs], [o[1] for o in objs]
    with_cov = treegp.predict_many(gps, Xs, return_cov=True)
    for (y, cov), o in zip(with_cov, objs):
        np.testing.assert_allclose(cov, o[2], rtol=0, atol=1e-9 * np.abs(o[2]).max())
    fresh = golden_objects(golden)
    with_var = treegp.predict_many([o[0] for o in fresh], Xs, return_var=True)
    for (y, var), o in zip(with_var, fresh):
        np.testing.assert_allclose(var, np.diag(o[2]), rtol=0, atol=1e-9 * np.abs(o[2]).max())
    means = treegp.predict_many([o[0] for o in golden_objects(golden)], Xs)
    for (y, _), (yv, _), ym in zip(with_cov, with_var, means):
        assert np.array_equal(y, ym) and np.array_equal(yv, ym)


def test_mixed_list_matches_each_objects_own_predict():
    rng = np.random.default_rng(3)

    def make(kernel, n, seed):
        r = np.random.default_rng(seed)
        X = r.uniform(0, 20, (n, 2))
        y = np.sin(X[:, 0] / 3.0) + 0.1 * r.standard_normal(n)
        gp = treegp.GPInterpolation(kernel=kernel, optimizer="none", normalize=True)
        gp.initialize(X, y, y_err=r.uniform(0.05, 0.1, n))
        return gp

    def objects():
        return [
            make("1.0**2 * RBF(2.0) + WhiteKernel(0.01)", 150, 1),               # dense route
            make("1.5**2 * RBF(2.0)", ops.BATCH_NMAX + 100, 2),                  # n > 4096
            make("1.0**2 * AnisotropicRBF(scale_length=[2.0, 3.0])", 400, 3),   # cached alpha (below)
            make("1.0**2 * VonKarman(4.0)", 300, 4),                            # kept factor of its own data (below)
            make("0.8**2 * RBF(1.5)", 700, 5),
            make("1.2**2 * AnisotropicVonKarman(scale_length=[3.0, 2.0])", 257, 6),
        ]
    Xq = [rng.uniform(0, 20, (m, 2)) for m in (40, 70, 300, 129, 256, 1)]
    for what in ("var", "cov"):
        kw = {"return_" + what: True}
        mine, theirs = objects(), objects()
        for gps in (mine, theirs):
            gps[2].predict(Xq[2])                                  # caches alpha, no factor
            gps[3].predict(Xq[3], **kw)                            # keeps the factor its predict(..., return_*) reuses
        cached = mine[2]._alpha
        got = treegp.predict_many(mine, Xq, **kw)
        want = [gp.predict(X, **kw) for gp, X in zip(theirs, Xq)]
        assert mine[2]._alpha is cached
        for i, ((y, u), (yw, uw)) in enumerate(zip(got, want)):
            assert u.shape == uw.shape, (what, i)
            if i in (0, 1, 3):                                     # through their own predict
                assert np.array_equal(y, yw) and np.array_equal(u, uw), (what, i)
            else:
                amp = mine[i].kernel.k1.constant_value
                np.testing.assert_allclose(u, uw, rtol=0, atol=1e-12 * amp, err_msg="%s %d" % (what, i))
                np.testing.assert_allclose(y, yw, rtol=0, atol=1e-10 * np.abs(yw).max(), err_msg="%s %d" % (what, i))
        for i in (2, 4, 5):
            assert mine[i]._factor is None and mine[i]._alpha is not None
    with pytest.raises(ValueError):
        treegp.predict_many(objects()[4:], Xq[4:], return_cov=True, return_var=True)


def test_c_abi_argument_errors_padding_and_timings():
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    batch = mixed_batch([5, 300, 129, 256, 1], 33)
    ms_l = [7, 1, 260, 256, 3]
    Xq = [queries(p, m, 80 + b) for b, (p, m) in enumerate(zip(batch, ms_l))]
    ns = np.array([len(p[4]) for p in batch], dtype=np.int64)
    ms = np.array(ms_l, dtype=np.int64)
    nb, nmax, mmax = len(batch), int(ns.max()), int(ms.max())
    X = np.full((nb, nmax, 2), np.nan)
    y = np.full((nb, nmax), np.nan)
    e = np.full((nb, nmax), np.nan)
    Xs = np.full((nb, mmax, 2), np.nan)
    for b, p in enumerate(batch):
        X[b, :ns[b]] = _lib.as_xy(p[3])
        y[b, :ns[b]] = p[4]
        e[b, :ns[b]] = p[5]
        Xs[b, :ms[b]] = _lib.as_xy(Xq[b])
    ks = (_lib.TgpKernel * nb)(*[p[0].to_c() for p in batch])

    def call(what, ns=ns, nmax=nmax, ms=ms, mmax=mmax, nb=nb, kinds=None):
        kk = (_lib.TgpKernel * len(ks))(*ks)
        if kinds is not None:
            kk[0].kind = kinds
        alpha = np.full((len(ks), max(nmax, 1)), np.nan)
        unc = np.full((len(ks), max(mmax, 1), max(mmax, 1)) if what == 2 else (len(ks), max(mmax, 1)), np.nan)
        logdet, chi2 = np.empty(len(ks)), np.empty(len(ks))
        info = np.full(len(ks), -1, dtype=np.int32)
        rc = lib.tgp_gp_posterior_batch(ctx, nb, C.cast(kk, C.c_void_p), _lib.ptr(ns), nmax, _lib.ptr(X), _lib.ptr(y), _lib.ptr(e),
                                        _lib.ptr(ms), mmax, _lib.ptr(Xs), what, _lib.ptr(alpha), _lib.ptr(unc), _lib.ptr(logdet),
                                        _lib.ptr(chi2), _lib.ptr(info))
        return rc, (lib.tgp_last_error(ctx) or b"").decode(), (alpha, unc, logdet, chi2, info)

    bad = [dict(what=3), dict(what=0), dict(what=1, nb=0), dict(what=1, nmax=4097), dict(what=1, kinds=9),
           dict(what=1, ns=np.array([0, 300, 129, 256, 1], dtype=np.int64)), dict(what=1, ms=np.array([7, 0, 260, 256, 3], dtype=np.int64)),
           dict(what=1, ms=np.array([7, 1, 261, 256, 3], dtype=np.int64)), dict(what=2, mmax=4097), dict(what=1, mmax=65281),
           dict(what=1, mmax=0)]
    for kw in bad:
        rc, msg, _ = call(**kw)
        assert rc == -1 and "tgp_gp_posterior_batch" in msg, (kw, rc, msg)
    with pytest.raises(ValueError):
        ops.gp_posterior_batch([ops.KernelSpec(0)], [np.zeros((3, 2))], [np.zeros(3)], None, [np.zeros((4097, 2))], what="cov")
    with pytest.raises(ValueError):
        ops.gp_posterior_batch([ops.KernelSpec(0)], [np.zeros((3, 2))], [np.zeros(3)], None, [np.zeros((3, 2))], what="std")

    for what, key in ((1, "var"), (2, "cov")):
        ops.gp_solve(batch[0][0], batch[0][3], batch[0][4], batch[0][5])   # a single solve fills other timing slots first
        rc, msg, (alpha, unc, logdet, chi2, info) = call(what)
        assert rc == 0 and list(info) == [0] * nb, msg
        tm = _lib.timings(ctx)
        assert tm[1] > 0 and tm[3] > 0 and all(tm[i] == 0 for i in range(len(tm)) if i not in (0, 1, 2, 3, 9)), tm
        a2, u2, ld2, c2, _ = post(batch, Xq, key)
        assert np.array_equal(logdet, ld2) and np.array_equal(chi2, c2)
        for b in range(nb):
            assert np.array_equal(alpha[b, :ns[b]], a2[b]) and np.all(alpha[b, ns[b]:] == 0.0)
            m = ms[b]
            if what == 1:
                assert np.array_equal(unc[b, :m], u2[b])
                assert np.all(unc[b, m:] == 0.0) and not np.signbit(unc[b, m:]).any()
            else:
                assert np.array_equal(unc[b, :m, :m], u2[b])
                outside = np.ones((mmax, mmax), dtype=bool)
                outside[:m, :m] = False
                assert np.all(unc[b][outside] == 0.0) and not np.signbit(unc[b][outside]).any()

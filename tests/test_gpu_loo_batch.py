"""GPU tests of batched leave-one-out (seam S2g: tgp_gp_loo_batch, ops.gp_loo_batch, predict_loo_many,
loo_log_predictive_many): diag(K^-1) against a dense inverse at the tile and panel edges of the 128 / 256 layout, the solve's
own bits, bit-independence of a problem from its batch, nmax and the chunking, failure isolation, the single-object route and
the C-ABI's rejections."""
import ctypes as C

import numpy as np
import pytest

import treegp_amd as tg
from treegp_amd import _lib, ops
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

KINDS = {                       # tag -> (oracle kind, C kind, parameters): the kernels of tests/test_gpu_loo.py
    "rbf": ("gauss", _lib.TGP_RBF, dict(amp=1.3, a=1.0 / 0.2 ** 2, b=0.0, c=1.0 / 0.2 ** 2)),
    "arbf": ("gauss", _lib.TGP_ARBF, dict(amp=1.3, a=30.0, b=4.0, c=20.0)),
    "vk": ("vk", _lib.TGP_VK, dict(amp=0.8, ell=0.3)),
    "avk": ("avk", _lib.TGP_AVK, dict(amp=0.8, a=12.0, b=2.0, c=9.0)),
}
SIZES = [1, 2, 127, 128, 129, 255, 256, 257, 300, 513]


def problem(tag, n, dim, seed):
    """(spec, oracle kind, oracle kwargs, X, y, y_err): points uniform in the unit square (or interval), y_err = 0.1 U(0.8, 1.2)"""
    okind, ckind, kw = KINDS[tag]
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, dim))
    y = rng.standard_normal(n)
    e = 0.1 * rng.uniform(0.8, 1.2, n)
    return ops.KernelSpec(ckind, **kw), okind, kw, X, y, e


def edge_batch():
    """every size with every kind in 2-D, and the Gaussian kernel in 1-D at every size: one ragged, mixed batch"""
    batch = [problem(tag, n, 2, 3000 + 10 * n + k) for n in SIZES for k, tag in enumerate(KINDS)]
    return batch + [problem("rbf", n, 1, 7000 + n) for n in SIZES]


def dense(p):
    return O.kernel_matrix(p[1], p[3], **p[2]) + np.diag(p[5] ** 2)


def run(batch, ctx=None):
    return ops.gp_loo_batch([p[0] for p in batch], [p[3] for p in batch], [p[4] for p in batch], [p[5] for p in batch], ctx=ctx)


@pytest.fixture(scope="module")
def edges():
    batch = edge_batch()
    return batch, run(batch)


def test_inv_diag_against_a_dense_inverse(edges):
    import scipy.linalg
    batch, (alphas, ds, logdet, chi2, info) = edges
    assert list(info) == [0] * len(batch)
    for b, p in enumerate(batch):
        n = len(p[4])
        tag = "problem %d (n = %d, kind %d, %d-D)" % (b, n, p[0].kind, p[3].shape[1])
        assert ds[b].shape == alphas[b].shape == (n,), tag
        A = dense(p)
        ref = np.diag(np.linalg.inv(A))
        # the reference reproduces itself: |L^-1 e_i|^2 from an independent factorisation
        Li = scipy.linalg.solve_triangular(scipy.linalg.cholesky(A, lower=True), np.eye(n), lower=True)
        np.testing.assert_allclose(ref, (Li * Li).sum(axis=0), rtol=1e-11, atol=0, err_msg="reference, " + tag)
        np.testing.assert_allclose(ds[b], ref, rtol=1e-9, atol=0, err_msg=tag)


def test_same_bits_as_the_batched_solve(edges):
    batch, (alphas, ds, logdet, chi2, info) = edges
    a2, ld2, c2, info2 = ops.gp_solve_batch([p[0] for p in batch], [p[3] for p in batch], [p[4] for p in batch],
                                            [p[5] for p in batch])
    assert np.array_equal(info, info2) and np.array_equal(logdet, ld2) and np.array_equal(chi2, c2)
    for b in range(len(batch)):
        assert np.array_equal(alphas[b], a2[b]), b


IND_SIZES = (130, 257, 64, 513)


def ind_batch():
    return [problem(tag, n, 2, 500 + n) for tag, n in zip(("arbf", "vk", "rbf", "avk"), IND_SIZES)]


def test_a_problem_does_not_depend_on_its_batch_nmax_or_the_chunk(monkeypatch):
    monkeypatch.delenv("TGP_BATCH_CHUNK", raising=False)
    batch = ind_batch()
    alone = [run([p])[1][0] for p in batch]
    for b, n in enumerate(IND_SIZES):
        assert alone[b].shape == (n,) and np.all(alone[b] > 0)

    def check(order, out, what, first=0):
        assert list(out[4]) == [0] * len(out[4]), what
        for place, b in enumerate(order):
            assert np.array_equal(out[1][first + place], alone[b]), (what, place, b)

    for shift in range(4):                                    # every problem at each place of the batch
        order = [(k + shift) % 4 for k in range(4)]
        check(order, run([batch[b] for b in order]), "rotated by %d" % shift)
    check([3, 2, 1, 0], run(batch[::-1]), "reversed")
    big = problem("rbf", 1025, 2, 77)                         # nmax 1025: Np goes from 768 to 1280
    check([0, 1, 2, 3], run(batch + [big]), "beside n = 1025")
    check([0, 1, 2, 3], run([big] + batch), "behind n = 1025", first=1)
    default = run(batch + [big])
    for chunk in ("1", "3"):
        monkeypatch.setenv("TGP_BATCH_CHUNK", chunk)
        out = run(batch + [big])
        check([0, 1, 2, 3], out, "TGP_BATCH_CHUNK=" + chunk)
        for k in range(5):
            assert np.array_equal(out[0][k], default[0][k]) and np.array_equal(out[1][k], default[1][k]), (chunk, k)
        assert np.array_equal(out[2], default[2]) and np.array_equal(out[3], default[3])


def test_a_singular_problem_fails_alone():
    good = ind_batch()
    x = np.array([[0.25, 0.75], [0.25, 0.75]])                # two coincident points, no error: K = [[1, 1], [1, 1]]
    bad = (ops.KernelSpec(_lib.TGP_RBF, amp=1.0, a=25.0, b=0.0, c=25.0), "gauss", {}, x, np.array([0.5, -0.5]), np.zeros(2))
    ref = run(good)
    with_bad = run(good[:2] + [bad] + good[2:])
    assert with_bad[4][2] > 0 and list(np.delete(with_bad[4], 2)) == [0] * 4
    for b, bb in zip(range(4), [0, 1, 3, 4]):
        assert np.array_equal(ref[0][b], with_bad[0][bb]) and np.array_equal(ref[1][b], with_bad[1][bb])
        assert ref[2][b] == with_bad[2][bb] and ref[3][b] == with_bad[3][bb]
    again = run(good)                                         # the context works afterwards
    for b in range(4):
        assert np.array_equal(ref[1][b], again[1][b])


KERNELS = {
    "rbf": "1.1**2 * RBF(0.3)",
    "arbf": "1.0**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))",
    "vk": "0.8**2 * VonKarman(length_scale=0.4)",
    "avk": "0.9**2 * AnisotropicVonKarman(invLam=array([[12., 2.], [2., 9.]]))",
}


def make_gp(tag, n, seed, normalize=True):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    y = np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.3 + 0.05 * rng.standard_normal(n)
    gp = tg.GPInterpolation(kernel=KERNELS[tag], optimizer="none", normalize=normalize)
    gp.initialize(X, y, y_err=rng.uniform(0.02, 0.1, n))
    return gp


def loo_cases():
    return [(tag, n, 100 + n + k, normalize) for n in (300, 700) for k, tag in enumerate(KERNELS) for normalize in (True, False)]


def oracle_kernel(gp):
    spec = tg.kernel_to_spec(gp.kernel)
    kind = {_lib.TGP_RBF: "gauss", _lib.TGP_ARBF: "gauss", _lib.TGP_VK: "vk", _lib.TGP_AVK: "avk"}[spec.kind]
    return O.kernel_matrix(kind, gp._X, amp=spec.amp, a=spec.a, b=spec.b, c=spec.c, ell=spec.ell), spec.amp


def brute_loo(gp, K0, idx):
    """point i removed and the residual problem solved again, _mean and the mean function held fixed: (y_loo, latent var)"""
    r = gp._y - gp._mean - gp._spatial_average
    s2 = np.asarray(gp._y_err) ** 2
    out = []
    for i in idx:
        keep = np.delete(np.arange(len(r)), i)
        w = np.linalg.solve(K0[np.ix_(keep, keep)] + np.diag(s2[keep]), K0[i, keep])
        out.append((w.dot(r[keep]) + gp._mean + gp._spatial_average[i], K0[i, i] - K0[i, keep].dot(w)))
    return np.array(out).T


def test_predict_loo_many_against_the_single_route_and_deleting_points():
    cases = loo_cases()
    gps = [make_gp(*c) for c in cases]
    got = tg.predict_loo_many(gps, return_var=True)
    plain = tg.predict_loo_many([make_gp(*c) for c in cases[:2]])
    assert np.array_equal(plain[0], got[0][0]) and np.array_equal(plain[1], got[1][0])
    for c, gp, (y_loo, var_loo) in zip(cases, gps, got):
        assert gp._alpha is not None and gp._factor is None, c
        ref_y, ref_v = make_gp(*c).predict_loo(return_var=True)
        amp = tg.kernel_to_spec(gp.kernel).amp
        assert y_loo.shape == var_loo.shape == (c[1],)
        np.testing.assert_allclose(y_loo, ref_y, rtol=0, atol=1e-9 * amp, err_msg=str(c))
        np.testing.assert_allclose(var_loo, ref_v, rtol=0, atol=1e-9 * amp, err_msg=str(c))
        if c[1] == 300:
            rng = np.random.default_rng(c[2])
            idx = np.concatenate([[0, 299], rng.choice(np.arange(1, 299), 6, replace=False)])
            K0, amp0 = oracle_kernel(gp)
            by, bv = brute_loo(gp, K0, idx)
            np.testing.assert_allclose(y_loo[idx], by, rtol=0, atol=1e-9 * amp0, err_msg=str(c))
            np.testing.assert_allclose(var_loo[idx], bv, rtol=0, atol=1e-9 * amp0, err_msg=str(c))


def test_predict_loo_many_of_one_point_is_the_prior():
    gp = tg.GPInterpolation(kernel="1.7**2 * RBF(0.3)", optimizer="none", normalize=False)
    gp.initialize(np.array([[0.3, 0.4]]), np.array([2.5]), y_err=np.array([0.1]))
    (y_loo, var_loo), = tg.predict_loo_many([gp], return_var=True)
    np.testing.assert_allclose(y_loo, [gp._mean + gp._spatial_average[0]], rtol=0, atol=1e-12 * 2.5)
    np.testing.assert_allclose(var_loo, [1.7 ** 2], rtol=1e-12)


def test_loo_log_predictive_many_against_the_single_method():
    cases = [c for c in loo_cases() if c[1] == 300]
    gps = [make_gp(*c) for c in cases]
    got = tg.loo_log_predictive_many(gps)
    assert got.shape == (len(gps),) and np.all(np.isfinite(got))
    for c, gp, s in zip(cases, gps, got):
        assert gp._alpha is None and gp._factor is None
        np.testing.assert_allclose(s, gp.return_loo_log_predictive(), rtol=1e-10, err_msg=str(c))
    thetas = [gp.kernel.theta + 0.05 * (1 + k % 3) for k, gp in enumerate(gps)]
    thetas[1] = None
    before = [gp.kernel.theta.copy() for gp in gps]
    got_theta = tg.loo_log_predictive_many(gps, thetas)
    for c, gp, s, th, th0 in zip(cases, gps, got_theta, thetas, before):
        assert np.array_equal(gp.kernel.theta, th0)
        np.testing.assert_allclose(s, gp.return_loo_log_predictive(th), rtol=1e-10, err_msg=str(c))
    assert got_theta[1] == got[1] and got_theta[0] != got[0]
    # a kernel whose matrix is not positive definite scores -inf and leaves its companions alone
    flat = tg.GPInterpolation(kernel="1.0**2 * AnisotropicRBF(scale_length=[50., 50.])", optimizer="none", normalize=False)
    flat.initialize(gps[0]._X, gps[0]._y, y_err=np.zeros(300))
    mixed = tg.loo_log_predictive_many([gps[0], flat, gps[2]])
    assert mixed[1] == -np.inf == flat.return_loo_log_predictive()
    assert mixed[0] == got[0] and mixed[2] == got[2]


def test_rejections_leave_the_context_usable():
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    p = problem("arbf", 40, 2, 5)
    ref = run([p])
    ns = np.array([40], dtype=np.int64)
    ks = (_lib.TgpKernel * 1)(p[0].to_c())
    X, y, e = _lib.as_xy(p[3]).reshape(1, 40, 2), p[4].reshape(1, 40), p[5].reshape(1, 40)
    alpha, d, out = np.empty((1, 40)), np.empty((1, 40)), np.empty(1)
    info = np.zeros(1, dtype=np.int32)

    def call(invdiag, nmax=40):
        rc = lib.tgp_gp_loo_batch(ctx, 1, C.cast(ks, C.c_void_p), _lib.ptr(ns), nmax, _lib.ptr(X), _lib.ptr(y), _lib.ptr(e),
                                  _lib.ptr(alpha), _lib.ptr(invdiag), _lib.ptr(out), None, _lib.ptr(info))
        return rc, (lib.tgp_last_error(ctx) or b"").decode()

    rc, msg = call(None)
    assert rc == -1 and "tgp_gp_loo_batch" in msg and "invdiag" in msg
    rc, msg = call(d, nmax=4097)
    assert rc == -1 and "tgp_gp_loo_batch" in msg
    rc, msg = call(d)                                          # the direct call: ydota = NULL, the same bits as through ops
    assert rc == 0 and info[0] == 0
    assert np.array_equal(d[0], ref[1][0]) and np.array_equal(alpha[0], ref[0][0]) and out[0] == ref[2][0]
    tm = _lib.timings(ctx)
    assert tm[1] > 0 and tm[3] > 0 and all(tm[i] == 0 for i in range(len(tm)) if i not in (0, 1, 2, 3))
    with pytest.raises(ValueError):
        ops.gp_loo_batch([p[0]], [np.zeros((4097, 2))], [np.zeros(4097)])
    with pytest.raises(ValueError):
        ops.gp_loo_batch([p[0]], [np.zeros((5, 3))], [np.zeros(5)])
    assert np.array_equal(run([p])[1][0], ref[1][0])

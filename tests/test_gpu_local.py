"""Local kriging on the device (include/tgp.h, seam S3l) against the host references of tests/_local_refs.py.

Every comparison of values is made ON THE NEIGHBOUR SET THE DEVICE RETURNED, after that set has been checked to be a valid
nearest set (k different rows of the table, nearest first, the farthest member no farther than (1 + 1e-12) x the nearest row left
out), so a near-tie between two candidates cannot fail a correct kernel.  Bounds, from the issue: |dys| <= 1e-10 max|y|,
|dvar| <= 1e-10 amp at yerr^2 = 2.5e-3 amp, where cond(K_S) <= k amp / yerr^2 + 1 <= 5.2e4 for k <= 128 (trace bound); the exact
limit (k >= n) against ``predict`` within 2e-10 of scale (both sides within 1e-10 of the truth).

Run as a program (``python test_gpu_local.py OUT.npz``) it makes the call of the chunking test and saves its outputs: the
test starts it in fresh processes with TGP_LOCAL_CHUNK set."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import treegp_amd as tg
from treegp_amd import _lib, ops

import _local_refs as LR

pytestmark = pytest.mark.gpu

N, M = 2000, 2048
KS = (1, 2, 31, 32, 33, 64, 65, 128)
MS = (1, 257, 2048)
KINDS = ("rbf", "arbf", "vk", "avk")

_CASES, _REFS, _DEVICE = {}, {}, {}


def case(name):
    """the data of one kernel kind with everything the references share, computed once and never changed"""
    if name not in _CASES:
        spec = LR.make_spec(name)
        X, y, y_err, Xs = LR.uniform_data(N, M)
        D = LR.dist2(spec, X, Xs)
        c = dict(spec=spec, X=X, y=y, y_err=y_err, Xs=Xs, D=D, K=LR.kernel_values(spec, X), Kx=LR.kernel_values(spec, Xs, X),
                 order=np.argsort(D, axis=1, kind="stable").astype(np.int32))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def reference(name, k):
    """brute-force neighbours of all M queries and the long-double solve on them, once per (kind, k)"""
    if (name, k) not in _REFS:
        c = case(name)
        nbr = np.ascontiguousarray(c["order"][:, :k])
        ys, var, info = LR.local_predict_ld(c["spec"], c["X"], c["y"], c["y_err"], c["Xs"], nbr, K=c["K"], Kx=c["Kx"])
        assert not info.any()
        for v in (nbr, ys, var):
            v.setflags(write=False)
        _REFS[(name, k)] = (nbr, ys, var)
    return _REFS[(name, k)]


def errors_on_returned_sets(spec, X, y, y_err, Xs, ys, var, nbr, K=None, Kx=None, ref=None):
    """max |dys| / max|y| and max |dvar| / amp against the long-double solve on the returned sets; ``ref`` = (nbr, ys, var) of
    the brute-force sets: rows whose returned set equals it reuse its solve"""
    if ref is not None:
        same = (nbr == ref[0]).all(axis=1)
        ys_r, var_r = np.array(ref[1]), np.array(ref[2])
        if not same.all():
            rows = np.flatnonzero(~same)
            a, b, info = LR.local_predict_ld(spec, X, y, y_err, Xs[rows], nbr[rows], K=K, Kx=None if Kx is None else Kx[rows])
            assert not info.any()
            ys_r[rows], var_r[rows] = a, b
    else:
        ys_r, var_r, info = LR.local_predict_ld(spec, X, y, y_err, Xs, nbr, K=K, Kx=Kx)
        assert not info.any()
    return np.abs(ys - ys_r).max() / np.abs(y).max(), np.abs(var - var_r).max() / spec.amp


# ---------------------------------------------------------------------------------------------------------
# values
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", KINDS)
def test_values(name, k, m):
    c = case(name)
    spec, X, y, y_err, Xs = c["spec"], c["X"], c["y"], c["y_err"], c["Xs"][:m]
    ys, var, nbr = ops.gp_predict_local(spec, X, y, y_err, Xs, k=k, return_var=True, return_neighbors=True)
    assert ys.shape == (m,) and var.shape == (m,) and nbr.shape == (m, k)
    LR.check_neighbor_sets(spec, X, Xs, nbr, D=c["D"][:m])
    rn, rys, rvar = reference(name, k)
    e_y, e_v = errors_on_returned_sets(spec, X, y, y_err, Xs, ys, var, nbr, K=c["K"], Kx=c["Kx"][:m], ref=(rn[:m], rys[:m], rvar[:m]))
    print("%s k = %d m = %d: |dys| = %.3e max|y|, |dvar| = %.3e amp, %d of %d sets differ from brute force"
          % (name, k, m, e_y, e_v, int((nbr != rn[:m]).any(axis=1).sum()), m))
    assert e_y <= 1e-10 and e_v <= 1e-10
    if k == 1:
        # closed form: ys = k* y / (amp + yerr^2), var = amp - k*^2 / (amp + yerr^2).  Three roundings on either side and the
        # evaluators' own error (the von Karman profile is held to 2e-13 of the value by the project's kernel-value tests)
        ks = np.take_along_axis(c["Kx"][:m], nbr.astype(np.int64), axis=1)[:, 0]
        d = spec.amp + y_err[nbr[:, 0]] ** 2
        assert np.abs(ys - ks * y[nbr[:, 0]] / d).max() <= 1e-12 * np.abs(y).max()
        assert np.abs(var - (spec.amp - ks * ks / d)).max() <= 1e-12 * spec.amp
    # the same query gives the same bits whatever m is
    first = _DEVICE.setdefault((name, k), (ys[:1].copy(), var[:1].copy(), nbr[:1].copy()))
    assert ys[0].tobytes() == first[0][0].tobytes() and var[0].tobytes() == first[1][0].tobytes() and np.array_equal(nbr[0], first[2][0])


# ---------------------------------------------------------------------------------------------------------
# the exact limit: k >= n
KERNEL_STRINGS = {
    "arbf": "0.8**2 * AnisotropicRBF(invLam=array([[60., -14.], [-14., 35.]]))",
    "vk": "0.8**2 * VonKarman(length_scale=0.6)",
}


@pytest.mark.parametrize("n", [5, 64, 128])
@pytest.mark.parametrize("name,table", [("arbf", False), ("vk", False), ("arbf", True)])
def test_exact_limit_is_predict(name, n, table):
    X, y, y_err, Xs = LR.uniform_data(n, 150, seed=100 + n)
    y = y + 3.0
    Xs = np.vstack([Xs, X])                                              # the stars themselves among the queries
    gp = tg.GPInterpolation(kernel=KERNEL_STRINGS[name], optimizer="none", normalize=True)
    if table:                                                            # a KNN mean function over a coarse table
        g = np.linspace(0.0, 1.0, 7)
        gp._X0 = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2) + 0.013
        gp._y0 = 3.0 + np.sin(4.0 * gp._X0[:, 0])
    gp.initialize(X, y, y_err=y_err)
    ys, var = gp.predict_local(Xs, k=128, return_var=True)
    assert gp._alpha is None and gp._factor is None
    ref, ref_var = gp.predict(Xs, return_var=True)
    scale = np.abs(gp._residual()).max()
    e_y, e_v = np.abs(ys - ref).max() / scale, np.abs(var - ref_var).max() / 0.64
    print("exact limit %s n = %d table %s: |dys| = %.3e of max|residual|, |dvar| = %.3e amp" % (name, n, table, e_y, e_v))
    assert e_y <= 2e-10 and e_v <= 2e-10
    if table:
        assert np.abs(gp._spatial_average).max() > 1.0 and abs(gp._mean) > 0.0


# ---------------------------------------------------------------------------------------------------------
# the search on degenerate inputs
def rotated_invlam(big, small, angle):
    cs, sn = np.cos(angle), np.sin(angle)
    return dict(a=big * cs * cs + small * sn * sn, b=(big - small) * cs * sn, c=big * sn * sn + small * cs * cs)


def search_case(tag):
    rng = np.random.default_rng(17)
    spec = LR.make_spec("rbf")
    if tag == "cluster":
        # 2900 of 3000 points inside one cell-sized cluster (the grid of k = 32 has cells of ~0.07): queries in and far from it
        X = np.vstack([0.41 + 0.05 * rng.uniform(size=(2900, 2)), rng.uniform(size=(100, 2))])
        Xs = np.vstack([0.41 + 0.05 * rng.uniform(size=(60, 2)), rng.uniform(size=(60, 2)), [[0.43, 0.43], [0.0, 0.0], [1.0, 1.0]]])
    elif tag == "collinear":
        X = np.stack([rng.uniform(size=1500), np.full(1500, 0.3)], axis=1)
        Xs = np.vstack([np.stack([rng.uniform(size=80), np.full(80, 0.3)], axis=1), rng.uniform(size=(40, 2))])
    elif tag == "one-dimensional":
        X, Xs = rng.uniform(size=1500), rng.uniform(-0.1, 1.1, size=120)
    elif tag == "far outside":
        X = rng.uniform(size=(1500, 2))
        Xs = np.array([[100.0, 0.5], [-100.0, 0.5], [0.5, 100.0], [0.5, -100.0], [100.0, 100.0], [-100.0, 100.0], [100.5, -99.0],
                       [1.05, 0.5], [0.5, -0.05], [2.0, 0.3], [0.3, -1.0]])
    elif tag == "axis ratio 1000":
        # lengths 0.005 and 5 (invLam eigenvalues 4e4 and 4e-2), rotated by 30 degrees.  The scale is set by the REFERENCE's own
        # error: q = a dx^2 + 2 b dx dy + c dy^2 is evaluated in float64 on the original coordinates by both sides, its terms
        # cancel, and its rounding error is ~ eps x 4e4 |d|^2 <= 2e-11 over the unit square, half of that in exp(-q / 2), on
        # either side; the nearly singular K_S of so long a correlation length passes it on: 3e-11 of max|y| is measured, a
        # third of the bound.  (With eigenvalues 4e6 and 4 the two float64 evaluations differ by more: 5e-11.)
        spec = LR.make_spec("arbf", **rotated_invlam(4.0e4, 4.0e-2, np.pi / 6))
        X = rng.uniform(size=(2000, 2))
        Xs = np.vstack([rng.uniform(size=(150, 2)), X[:10], [[3.0, 3.0], [-1.0, 0.5]]])
    elif tag == "duplicated rows":
        base = rng.uniform(size=(700, 2))
        X = np.vstack([base, base, base[:100]])
        Xs = np.vstack([rng.uniform(size=(100, 2)), base[:30]])
    else:
        raise ValueError(tag)
    n = len(X)
    XX = LR.as_xy(X)
    y = np.sin(5.0 * XX[:, 0]) + XX[:, 1] + 0.05 * rng.standard_normal(n)
    return spec, X, y, np.full(n, np.sqrt(LR.NOISE2)), Xs


@pytest.mark.parametrize("k", [32, 77])
@pytest.mark.parametrize("tag", ["cluster", "collinear", "one-dimensional", "far outside", "axis ratio 1000", "duplicated rows"])
def test_search_on_degenerate_inputs(tag, k):
    spec, X, y, y_err, Xs = search_case(tag)
    ys, var, nbr = ops.gp_predict_local(spec, X, y, y_err, Xs, k=k, return_var=True, return_neighbors=True)
    assert nbr.shape == (len(Xs), k)
    LR.check_neighbor_sets(spec, X, Xs, nbr)
    e_y, e_v = errors_on_returned_sets(spec, LR.as_xy(X), y, y_err, LR.as_xy(Xs), ys, var, nbr, K=LR.kernel_values(spec, X),
                                       Kx=LR.kernel_values(spec, Xs, X))
    same = (nbr == LR.brute_neighbors(spec, X, Xs, k)).all(axis=1)
    print("%s k = %d: |dys| = %.3e max|y|, |dvar| = %.3e amp, %d of %d sets differ from brute force" % (tag, k, e_y, e_v, int((~same).sum()), len(Xs)))
    assert e_y <= 1e-10 and e_v <= 1e-10


@pytest.mark.parametrize("k", [1, 11, 32, 64, 100])
def test_exact_ties_go_to_the_lower_row(k):
    # a 40 x 50 lattice of integers, queries on lattice sites (corners, edges, interior) and half way between: every distance is
    # an exact small integer (or quarter), ties abound, and the returned lists must be the stable sort's, row for row
    spec = LR.make_spec("rbf", a=0.25, b=0.0, c=0.25)
    gx, gy = np.meshgrid(np.arange(40.0), np.arange(50.0), indexing="ij")
    X = np.stack([gx.ravel(), gy.ravel()], axis=1)
    rng = np.random.default_rng(4)
    X = X[rng.permutation(len(X))]                                     # rows in no order of the plane
    Xs = np.vstack([X[:150], [[0.0, 0.0], [39.0, 49.0], [0.0, 49.0], [39.0, 0.0], [20.0, 0.0], [0.0, 25.0]], X[150:200] + 0.5, [[-3.0, 60.0]]])
    y = np.sin(0.4 * X[:, 0]) + np.cos(0.3 * X[:, 1])
    y_err = np.full(len(X), np.sqrt(LR.NOISE2))
    ys, var, nbr = ops.gp_predict_local(spec, X, y, y_err, Xs, k=k, return_var=True, return_neighbors=True)
    LR.check_neighbor_sets(spec, X, Xs, nbr)
    ref = LR.brute_neighbors(spec, X, Xs, k)
    assert np.array_equal(nbr, ref), "rows %s" % np.flatnonzero((nbr != ref).any(axis=1))[:10]
    e_y, e_v = errors_on_returned_sets(spec, X, y, y_err, Xs, ys, var, nbr, K=LR.kernel_values(spec, X), Kx=LR.kernel_values(spec, Xs, X))
    print("lattice k = %d: |dys| = %.3e max|y|, |dvar| = %.3e amp" % (k, e_y, e_v))
    assert e_y <= 1e-10 and e_v <= 1e-10


# ---------------------------------------------------------------------------------------------------------
# independence
def independence_call():
    """ys, var, nbr, info of 257 queries straight from the library"""
    c = case("arbf")
    rc, msg, ys, var, nbr, info = raw_call(c["spec"], c["X"], c["y"], c["y_err"], c["Xs"][:257], 33)
    assert rc == 0, msg
    return ys, var, nbr, info


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_outputs_do_not_depend_on_the_other_queries():
    c = case("arbf")
    ys, var, nbr, info = independence_call()
    assert not info.any()
    perm = np.random.default_rng(8).permutation(257)
    ys_p, var_p, nbr_p = ops.gp_predict_local(c["spec"], c["X"], c["y"], c["y_err"], c["Xs"][:257][perm], k=33, return_var=True,
                                              return_neighbors=True)
    assert same_bits(ys_p, ys[perm]) and same_bits(var_p, var[perm]) and same_bits(nbr_p, nbr[perm])
    pick = np.array([200, 3, 77])
    ys_s, var_s, nbr_s = ops.gp_predict_local(c["spec"], c["X"], c["y"], c["y_err"], c["Xs"][pick], k=33, return_var=True,
                                              return_neighbors=True)
    assert same_bits(ys_s, ys[pick]) and same_bits(var_s, var[pick]) and same_bits(nbr_s, nbr[pick])
    # without the variance and the lists the means are the same bits
    assert same_bits(ops.gp_predict_local(c["spec"], c["X"], c["y"], c["y_err"], c["Xs"][:257], k=33), ys)


@pytest.mark.parametrize("chunk", ["1", "37"])
def test_outputs_do_not_depend_on_the_chunk(chunk):
    ys, var, nbr, info = independence_call()
    with tempfile.TemporaryDirectory() as folder:
        out = os.path.join(folder, "chunk.npz")
        env = dict(os.environ, TGP_LOCAL_CHUNK=chunk)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.load(out)
        assert str(got["chunk"]) == chunk
        assert same_bits(got["ys"], ys) and same_bits(got["var"], var) and same_bits(got["nbr"], nbr) and same_bits(got["info"], info)


# ---------------------------------------------------------------------------------------------------------
# failure
def test_a_failed_query_leaves_the_others_alone():
    # amp = 1/4: sqrt(amp) and the first column of the factor are exact, so two coincident rows without noise at the head of a
    # list give a second pivot of exactly 0 in any arithmetic: info = 2.  The pair sits far from every other query's neighbours.
    spec = LR.make_spec("rbf", amp=0.25)
    rng = np.random.default_rng(23)
    X = np.vstack([rng.uniform(size=(1000, 2)), [[2.0, 2.0], [2.0, 2.0]]])
    y = np.sin(5.0 * X[:, 0]) + X[:, 1]
    y_err = np.append(np.full(1000, np.sqrt(2.5e-3 * 0.25)), [0.0, 0.0])
    Xs = np.vstack([rng.uniform(size=(40, 2)), [[2.0, 2.0]], rng.uniform(size=(30, 2))])
    j = 40
    with pytest.raises(np.linalg.LinAlgError, match=r"query 40: the 2-th leading minor") as ei:
        ops.gp_predict_local(spec, X, y, y_err, Xs, k=8, return_var=True, return_neighbors=True)
    info = ei.value.info
    ys, var, nbr = ei.value.results
    assert info[j] == 2 and np.count_nonzero(info) == 1
    assert np.isnan(ys[j]) and np.isnan(var[j]) and list(nbr[j][:2]) == [1000, 1001]
    _, _, ref_info = LR.local_predict_ld(spec, X, y, y_err, Xs[j:j + 1], nbr[j:j + 1])
    assert ref_info[0] == 2
    keep = np.arange(len(Xs)) != j
    ys_o, var_o, nbr_o = ops.gp_predict_local(spec, X, y, y_err, Xs[keep], k=8, return_var=True, return_neighbors=True)
    assert same_bits(ys_o, ys[keep]) and same_bits(var_o, var[keep]) and same_bits(nbr_o, nbr[keep])
    LR.check_neighbor_sets(spec, X, Xs, nbr)
    e_y, e_v = errors_on_returned_sets(spec, X, y, y_err, Xs[keep], ys_o, var_o, nbr_o)
    assert e_y <= 1e-10 and e_v <= 1e-10
    # through the object: the same error, naming the point
    gp = tg.GPInterpolation(kernel="0.5**2 * RBF(0.15)", optimizer="none", normalize=False)
    gp.initialize(X, y, y_err=y_err)
    with pytest.raises(np.linalg.LinAlgError, match="query 40"):
        gp.predict_local(Xs, k=8)


# ---------------------------------------------------------------------------------------------------------
# arguments
def raw_call(spec, X, y, y_err, Xs, kn, want_var=True, want_nbr=True, want_info=True, n=None):
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    X2, Xs2 = _lib.as_xy(X), _lib.as_xy(Xs)
    n = X2.shape[0] if n is None else n
    m = Xs2.shape[0]
    ys, var = np.full(m, -7.0), (np.full(m, -7.0) if want_var else None)
    nbr = np.full((m, max(kn, 1)), -7, dtype=np.int32) if want_nbr else None
    info = np.full(m, -7, dtype=np.int32) if want_info else None
    rc = lib.tgp_gp_predict_local(ctx, C.byref(spec.to_c()), _lib.ptr(X2), n, _lib.ptr(_lib.f64(y)), _lib.ptr(None if y_err is None else _lib.f64(y_err)),
                                  _lib.ptr(Xs2), m, kn, _lib.ptr(ys), _lib.ptr(var), _lib.ptr(nbr), _lib.ptr(info))
    msg = lib.tgp_last_error(ctx)
    return rc, (msg.decode() if msg else ""), ys, var, nbr, info


def test_arguments():
    c = case("arbf")
    spec, X, y, y_err, Xs = c["spec"], c["X"][:300], c["y"][:300], c["y_err"][:300], c["Xs"][:20]
    for kn in (0, 129, -1):
        rc, msg, ys, _, _, _ = raw_call(spec, X, y, y_err, Xs, kn)
        assert rc == -1 and "kn" in msg and (ys == -7.0).all()
    rc, msg, ys, _, _, _ = raw_call(spec, X, y, y_err, Xs, 8, want_info=False)
    assert rc == -1 and "info" in msg and (ys == -7.0).all()
    rc, msg, _, _, _, _ = raw_call(LR.make_spec("arbf", a=1.0, b=2.0, c=1.0), X, y, y_err, Xs, 8)
    assert rc == -1 and "Cholesky" in msg
    rc, msg, _, _, _, _ = raw_call(LR.make_spec("avk", a=-1.0), X, y, y_err, Xs, 8)
    assert rc == -1 and "Cholesky" in msg
    rc, msg, _, _, _, _ = raw_call(ops.KernelSpec(9), X, y, y_err, Xs, 8)
    assert rc == -1 and "kind" in msg
    rc, msg, _, _, _, _ = raw_call(spec, X, y, y_err, Xs, 8, n=0)
    assert rc == -1
    # an isotropic kind never looks at a, b, c for the metric
    rc, msg, _, _, _, info = raw_call(LR.make_spec("vk", a=-1.0, b=5.0, c=-1.0), X, y, y_err, Xs, 8)
    assert rc == 0 and not info.any()
    # var and nbr are optional, and leaving them out changes nothing
    rc, _, ys, var, nbr, info = raw_call(spec, X, y, y_err, Xs, 8)
    assert rc == 0 and not info.any() and (nbr >= 0).all()
    rc, _, ys2, var2, nbr2, info2 = raw_call(spec, X, y, y_err, Xs, 8, want_var=False, want_nbr=False)
    assert rc == 0 and same_bits(ys2, ys) and same_bits(info2, info)
    # no errors given: no noise on the diagonal (k = 2 keeps the matrices well conditioned)
    rc, _, ys3, var3, nbr3, info3 = raw_call(spec, X, y, None, Xs, 2)
    assert rc == 0 and not info3.any()
    r_ys, r_var, r_info = LR.local_predict_ld(spec, X, y, None, Xs, nbr3)
    assert np.abs(ys3 - r_ys).max() <= 1e-10 * np.abs(y).max() and np.abs(var3 - r_var).max() <= 1e-10 * spec.amp
    # n = 1: one neighbour whatever kn asks for, the lists padded with -1; the closed form
    rc, _, ys4, var4, nbr4, info4 = raw_call(spec, X[:1], y[:1], y_err[:1], Xs, 5)
    assert rc == 0 and not info4.any() and (nbr4[:, 0] == 0).all() and (nbr4[:, 1:] == -1).all()
    ks = LR.kernel_values(spec, Xs, X[:1])[:, 0]
    d = spec.amp + y_err[0] ** 2
    assert np.abs(ys4 - ks * y[0] / d).max() <= 1e-12 * abs(y[0]) and np.abs(var4 - (spec.amp - ks * ks / d)).max() <= 1e-12 * spec.amp
    # the Python layer clips k itself
    out = ops.gp_predict_local(spec, X[:3], y[:3], y_err[:3], Xs, k=64, return_neighbors=True)
    assert out[1].shape == (20, 3) and (np.sort(out[1], axis=1) == np.arange(3)).all()
    t = _lib.timings(_lib.get_ctx())
    assert t[0] > 0 and t[2] > 0 and t[3] > 0 and t[1] == 0 and all(v == 0 for v in t[4:])


# ---------------------------------------------------------------------------------------------------------
# what a context carries between calls
def test_predict_bits_do_not_move_across_a_local_call():
    c = case("arbf")
    spec, X, y, y_err, Xs = c["spec"], c["X"][:700], c["y"][:700], c["y_err"][:700], c["Xs"][:300]
    alpha = ops.gp_solve(spec, X, y, y_err)[0]
    before = ops.gp_predict(spec, X, alpha, Xs)
    ys = ops.gp_predict_local(spec, X, y, y_err, Xs, k=64)
    after = ops.gp_predict(spec, X, alpha, Xs)
    assert same_bits(before, after)
    assert same_bits(ops.gp_predict_local(spec, X, y, y_err, Xs, k=64), ys)
    assert same_bits(ops.gp_solve(spec, X, y, y_err)[0], alpha)
    # k = 64 of 700 stars against the dense GP: close, not equal (a property of the method, reported only)
    print("k = 64 of 700: max |local - dense| = %.3e max|y|" % (np.abs(ys - before).max() / np.abs(y).max()))


if __name__ == "__main__":
    ys, var, nbr, info = independence_call()
    np.savez(sys.argv[1], ys=ys, var=var, nbr=nbr, info=info, chunk=os.environ.get("TGP_LOCAL_CHUNK", ""))

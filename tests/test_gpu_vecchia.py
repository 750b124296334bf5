"""Local conditionals on the device (include/tgp.h, seam S3v) against the host references of tests/_vecchia_refs.py.

As in test_gpu_local.py every comparison of values is made ON THE LISTS THE DEVICE RETURNED, after those lists have been checked
to be valid nearest-eligible sets (cnt = min(k, eligible rows), eligible rows only, all different, nearest first, the farthest
member no farther than (1 + 1e-12) x the nearest eligible row left out).  Bounds, from the issue, the ones S3l is held to on this
data (yerr^2 = 2.5e-3 amp, cond(K_S) <= 5.2e4 by the trace bound): |dmu| <= 1e-10 max|y|, |dvar| <= 1e-10 amp.

Run as a program (``python test_gpu_vecchia.py OUT.npz``) it makes the calls of the chunking test and saves their outputs: the
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
import _vecchia_refs as VR

pytestmark = pytest.mark.gpu

LD = np.longdouble
N = 2000
KS = (1, 2, 31, 32, 33, 64, 65, 128)
KINDS = ("rbf", "arbf", "vk", "avk")
MODES = ("loo", "prior")
RANK = ops.vecchia_rank(N, seed=0)
RANK.setflags(write=False)

_CASES = {}


def case(name):
    """the data of one kernel kind with everything the references share, computed once and never changed"""
    if name not in _CASES:
        spec = LR.make_spec(name)
        X, y, y_err, _ = LR.uniform_data(N, 1)
        c = dict(spec=spec, X=X, y=y, y_err=y_err, D=VR.self_dist2(spec, X), K=LR.kernel_values(spec, X))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def value_errors(spec, X, y, y_err, mu, var, nbr, cnt, K=None):
    """max |dmu| / max|y| and max |dvar| / amp against the long-double solve on the returned lists, and that reference"""
    r_mu, r_var, r_info = VR.cond_ld(spec, X, y, y_err, nbr, cnt, K=K)
    assert not r_info.any()
    return np.abs(mu - r_mu).max() / np.abs(y).max(), np.abs(var - r_var).max() / spec.amp, r_mu, r_var


check_sums = VR.check_sums


# ---------------------------------------------------------------------------------------------------------
# values
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", KINDS)
def test_values(name, k, mode):
    c = case(name)
    spec, X, y, y_err = c["spec"], c["X"], c["y"], c["y_err"]
    rank = RANK if mode == "prior" else None
    mu, var, sums, nbr, cnt = ops.gp_local_cond(spec, X, y, y_err, k=k, mode=mode, rank=rank, return_neighbors=True)
    assert mu.shape == (N,) and var.shape == (N,) and sums.shape == (3,)
    VR.check_lists(spec, X, nbr, cnt, k, mode, rank, D=c["D"])
    e_m, e_v, _, _ = value_errors(spec, X, y, y_err, mu, var, nbr, cnt, K=c["K"])
    ref_nbr, _ = VR.brute_lists(spec, X, k, mode, rank, D=c["D"])
    print("%s %s k = %d: |dmu| = %.3e max|y|, |dvar| = %.3e amp, %d of %d lists differ from brute force"
          % (name, mode, k, e_m, e_v, int((nbr != ref_nbr).any(axis=1).sum()), N))
    assert e_m <= 1e-10 and e_v <= 1e-10
    if mode == "prior":
        first = int(np.flatnonzero(RANK == 0)[0])
        assert cnt[first] == 0 and mu[first] == 0.0 and var[first] == spec.amp          # exactly
    check_sums(y, y_err, mu, var, sums, "%s %s k = %d" % (name, mode, k))
    # without the lists the values and the sums are the same bits
    mu2, var2, sums2 = ops.gp_local_cond(spec, X, y, y_err, k=k, mode=mode, rank=rank)
    assert same_bits(mu2, mu) and same_bits(var2, var) and same_bits(sums2, sums)


# ---------------------------------------------------------------------------------------------------------
# the two identities with gp_predict_local
def identity_data(name):
    """the shared data with row 7 moved to a corner of the bounding box of the WHITENED points (the grid's box)"""
    c = case(name)
    spec = c["spec"]
    X = np.array(c["X"])
    U = LR.whiten(spec, X)
    r00, r01, r11 = LR.whitening(spec)
    u0, u1 = U[:, 0].max() + 0.01, U[:, 1].max() + 0.01
    X[7, 1] = u1 / r11
    X[7, 0] = (u0 - r01 * X[7, 1]) / r00
    U = LR.whiten(spec, X)
    assert U[:, 0].argmax() == 7 and U[:, 1].argmax() == 7
    return spec, X, c["y"], c["y_err"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["arbf", "avk"])
def test_rows_are_predict_local_on_the_eligible_rows(name, mode):
    k = 33
    spec, X, y, y_err = identity_data(name)
    rank = RANK if mode == "prior" else None
    mu, var, sums, nbr, cnt = ops.gp_local_cond(spec, X, y, y_err, k=k, mode=mode, rank=rank, return_neighbors=True)
    by_rank = np.argsort(RANK)
    rows = [int(by_rank[r]) for r in (0, 1, k - 1, k, N - 1)] + [7, 0, N - 1, 500, 1001, 1500, 1999]
    assert len(rows) == 12
    for i in rows:
        keep = np.flatnonzero(RANK < RANK[i]) if mode == "prior" else np.flatnonzero(np.arange(N) != i)      # in row order
        if len(keep) == 0:
            assert cnt[i] == 0 and (nbr[i] == -1).all() and mu[i] == 0.0 and var[i] == spec.amp
            continue
        ys_p, var_p, nbr_p = ops.gp_predict_local(spec, X[keep], y[keep], y_err[keep], X[i:i + 1], k=k, return_var=True,
                                                  return_neighbors=True)
        assert cnt[i] == min(k, len(keep)) == nbr_p.shape[1]
        assert np.array_equal(keep[nbr_p[0]], nbr[i, :cnt[i]]) and (nbr[i, cnt[i]:] == -1).all(), "row %d" % i
        assert ys_p[0].tobytes() == mu[i].tobytes() and var_p[0].tobytes() == var[i].tobytes(), "row %d (rank %d)" % (i, RANK[i])


# ---------------------------------------------------------------------------------------------------------
# the exact limits: k reaches every eligible row
KERNEL_STRINGS = {
    "arbf": "0.8**2 * AnisotropicRBF(invLam=array([[60., -14.], [-14., 35.]]))",
    "vk": "0.8**2 * VonKarman(length_scale=0.6)",
}


@pytest.mark.parametrize("name", KINDS)
def test_prior_with_the_identity_ordering_is_the_dense_likelihood(name):
    n, k = 129, 128
    spec = LR.make_spec(name)
    X, y, y_err, _ = LR.uniform_data(n, 1, seed=129)
    rank = np.arange(n, dtype=np.int32)
    mu, var, sums, nbr, cnt = ops.gp_local_cond(spec, X, y, y_err, k=k, mode="prior", rank=rank, return_neighbors=True)
    assert np.array_equal(cnt, np.minimum(rank, k)) and np.array_equal(cnt, rank)        # every predecessor
    K = LR.kernel_values(spec, X)
    ll_dense, _, _ = VR.dense_loglik_ld(K, y, y_err)
    # the per-row bounds pushed through log N(y_i | mu_i, s2_i), at the reference's own r_i and s2_i
    r_mu, r_var, r_info = VR.cond_ld(spec, X, y, y_err, *VR.brute_lists(spec, X, k, "prior", rank), K=K)
    assert not r_info.any()
    _, _, r, s2 = VR.terms_ld(y, y_err, r_mu, r_var)
    dv, dm = LD(1e-10) * spec.amp, LD(1e-10) * np.abs(y).max()
    bound = float((LD(0.5) * dv / s2 + np.abs(r) * dm / s2 + LD(0.5) * r * r * dv / (s2 * s2)).sum())
    ll = -LD(0.5) * LD(sums[1]) - LD(0.5) * LD(sums[0]) - LD(0.5) * n * VR.LOG_2PI
    print("%s: log L local - dense = %.3e, bound %.3e (log L = %.6f)" % (name, float(ll - ll_dense), bound, float(ll_dense)))
    assert abs(float(ll - ll_dense)) <= bound


@pytest.mark.parametrize("name,table", [("arbf", False), ("vk", False), ("arbf", True)])
def test_loo_with_every_other_row_is_predict_loo(name, table):
    n = 129
    X, y, y_err, _ = LR.uniform_data(n, 1, seed=229)
    y = y + 3.0
    gp = tg.GPInterpolation(kernel=KERNEL_STRINGS[name], optimizer="none", normalize=True)
    if table:
        g = np.linspace(0.0, 1.0, 7)
        gp._X0 = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2) + 0.013
        gp._y0 = 3.0 + np.sin(4.0 * gp._X0[:, 0])
    gp.initialize(X, y, y_err=y_err)
    y_loo, var, nbr, cnt = gp.predict_loo_local(k=128, return_var=True, return_neighbors=True)
    assert gp._alpha is None and gp._factor is None and (cnt == 128).all()
    ref, ref_var = gp.predict_loo(return_var=True)
    scale = np.abs(gp._residual()).max()
    e_y, e_v = np.abs(y_loo - ref).max() / scale, np.abs(var - ref_var).max() / 0.64
    print("exact limit %s table %s: |dy_loo| = %.3e of max|residual|, |dvar| = %.3e amp" % (name, table, e_y, e_v))
    assert e_y <= 2e-10 and e_v <= 2e-10
    # the scores in the same limit: the dense ones
    ll, ll_d = gp.return_log_likelihood_local(k=128), gp.return_log_likelihood()
    lp, lp_d = gp.return_loo_log_predictive_local(k=128), gp.return_loo_log_predictive()
    print("   log L %.9f / dense %.9f, LOO score %.9f / dense %.9f" % (ll, ll_d, lp, lp_d))
    assert abs(ll - ll_d) <= 1e-9 * (abs(ll_d) + n) and abs(lp - lp_d) <= 1e-9 * (abs(lp_d) + n)


# ---------------------------------------------------------------------------------------------------------
# the search on degenerate inputs
def search_case(tag):
    """the shapes of test_gpu_local.search_case, as training sets"""
    rng = np.random.default_rng(17)
    spec = LR.make_spec("rbf")
    if tag == "cluster":
        # 2900 of 3000 points inside one cell-sized cluster
        X = np.vstack([0.41 + 0.05 * rng.uniform(size=(2900, 2)), rng.uniform(size=(100, 2))])
    elif tag == "collinear":
        X = np.stack([rng.uniform(size=1500), np.full(1500, 0.3)], axis=1)
    elif tag == "one-dimensional":
        X = rng.uniform(size=1500)
    elif tag == "duplicated rows":
        base = rng.uniform(size=(700, 2))
        X = np.vstack([base, base, base[:100]])
    elif tag == "lattice":
        # a 40 x 50 lattice of integers in no order of the plane: every distance is an exact small integer, ties abound
        spec = LR.make_spec("rbf", a=0.25, b=0.0, c=0.25)
        gx, gy = np.meshgrid(np.arange(40.0), np.arange(50.0), indexing="ij")
        X = np.stack([gx.ravel(), gy.ravel()], axis=1)
        X = X[np.random.default_rng(4).permutation(len(X))]
    else:
        raise ValueError(tag)
    n = len(X)
    XX = LR.as_xy(X)
    y = np.sin(5.0 * XX[:, 0]) + XX[:, 1] + 0.05 * rng.standard_normal(n)
    if tag == "lattice":
        y = np.sin(0.4 * XX[:, 0]) + np.cos(0.3 * XX[:, 1])
    return spec, X, y, np.full(n, np.sqrt(LR.NOISE2))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [32, 77])
@pytest.mark.parametrize("tag", ["cluster", "collinear", "one-dimensional", "duplicated rows", "lattice"])
def test_search_on_degenerate_inputs(tag, k, mode):
    spec, X, y, y_err = search_case(tag)
    n = len(y)
    rank = ops.vecchia_rank(n, seed=5) if mode == "prior" else None
    mu, var, sums, nbr, cnt = ops.gp_local_cond(spec, X, y, y_err, k=k, mode=mode, rank=rank, return_neighbors=True)
    X2 = LR.as_xy(X)
    D = VR.self_dist2(spec, X2)
    VR.check_lists(spec, X2, nbr, cnt, k, mode, rank, D=D)
    ref_nbr, ref_cnt = VR.brute_lists(spec, X2, k, mode, rank, D=D)
    if tag in ("lattice", "duplicated rows"):
        # exact ties (equal distances on the lattice, coincident points among the duplicates) go to the lower row: the lists are
        # the stable sort's, row for row; a duplicate of row i at another row is its first neighbour in LOO mode
        assert np.array_equal(nbr, ref_nbr), "rows %s" % np.flatnonzero((nbr != ref_nbr).any(axis=1))[:10]
    if tag == "duplicated rows" and mode == "loo":
        assert (nbr[:700, 0] == np.arange(700, 1400)).all() and (nbr[700:1400, 0] == np.arange(700)).all()
    e_m, e_v, _, _ = value_errors(spec, X2, y, y_err, mu, var, nbr, cnt, K=LR.kernel_values(spec, X2))
    print("%s %s k = %d: |dmu| = %.3e max|y|, |dvar| = %.3e amp, %d of %d lists differ from brute force"
          % (tag, mode, k, e_m, e_v, int((nbr != ref_nbr).any(axis=1).sum()), n))
    assert e_m <= 1e-10 and e_v <= 1e-10
    check_sums(y, y_err, mu, var, sums, tag)


# ---------------------------------------------------------------------------------------------------------
# given lists
def raw_call(spec, X, y, y_err, kn, mode=0, rank=None, nbr_in=None, want=("mu", "var", "nbr", "cnt", "info", "sums")):
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    X2 = _lib.as_xy(X)
    n = X2.shape[0]
    out = dict(mu=np.full(n, -7.0), var=np.full(n, -7.0), nbr=np.full((n, max(kn, 1)), -7, dtype=np.int32),
               cnt=np.full(n, -7, dtype=np.int32), info=np.full(n, -7, dtype=np.int32), sums=np.full(3, -7.0))
    p = {key: _lib.ptr(v if key in want else None) for key, v in out.items()}
    rank = None if rank is None else np.ascontiguousarray(rank, dtype=np.int32)
    nbr_in = None if nbr_in is None else np.ascontiguousarray(nbr_in, dtype=np.int32)
    rc = lib.tgp_gp_local_cond(ctx, C.byref(spec.to_c()), _lib.ptr(X2), n, _lib.ptr(_lib.f64(y)),
                               _lib.ptr(None if y_err is None else _lib.f64(y_err)), mode, _lib.ptr(rank), kn, _lib.ptr(nbr_in),
                               p["mu"], p["var"], p["nbr"], p["cnt"], p["info"], p["sums"])
    msg = lib.tgp_last_error(ctx)
    return rc, (msg.decode() if msg else ""), out


def untouched(out):
    return all((v == -7).all() for v in out.values())


@pytest.mark.parametrize("mode", MODES)
def test_given_lists_give_the_same_bits(mode):
    c = case("arbf")
    spec, X, y, y_err = c["spec"], c["X"][:600], c["y"][:600], c["y_err"][:600]
    rank = ops.vecchia_rank(600, seed=2) if mode == "prior" else None
    mu, var, sums, nbr, cnt = ops.gp_local_cond(spec, X, y, y_err, k=33, mode=mode, rank=rank, return_neighbors=True)
    # neither mode nor rank is consulted: the other mode's name, no rank
    mu2, var2, sums2, nbr2, cnt2 = ops.gp_local_cond(spec, X, y, y_err, k=33, mode="loo", neighbors=nbr, return_neighbors=True)
    assert same_bits(mu2, mu) and same_bits(var2, var) and same_bits(sums2, sums) and same_bits(nbr2, nbr) and same_bits(cnt2, cnt)
    # lists of one's own: every row from rows 0 .. 2 (or fewer), whatever the metric says
    own = np.full((600, 33), -1, dtype=np.int32)
    for i in range(600):
        rows = [r for r in (0, 1, 2) if r != i][:i % 3 + (i > 2)]
        own[i, :len(rows)] = rows
    mu3, var3, sums3, nbr3, cnt3 = ops.gp_local_cond(spec, X, y, y_err, k=33, neighbors=own, return_neighbors=True)
    assert same_bits(nbr3, own) and np.array_equal(cnt3, (own >= 0).sum(axis=1))
    r_mu, r_var, r_info = VR.cond_ld(spec, X, y, y_err, own, cnt3)
    assert np.abs(mu3 - r_mu).max() <= 1e-10 * np.abs(y).max() and np.abs(var3 - r_var).max() <= 1e-10 * spec.amp


def test_bad_lists_and_bad_ranks_are_argument_errors():
    c = case("arbf")
    spec, X, y, y_err = c["spec"], c["X"][:300], c["y"][:300], c["y_err"][:300]
    rc, msg, good = raw_call(spec, X, y, y_err, 8)
    assert rc == 0 and not good["info"].any(), msg
    nbr = good["nbr"]
    bad = nbr.copy()
    bad[41, 3] = 41
    rc, msg, out = raw_call(spec, X, y, y_err, 8, nbr_in=bad)
    assert rc == -1 and "row 41" in msg and "itself" in msg and untouched(out)
    with pytest.raises(_lib.TgpError, match="row 41"):
        ops.gp_local_cond(spec, X, y, y_err, k=8, neighbors=bad)
    bad = nbr.copy()
    bad[17, 2] = -1
    rc, msg, out = raw_call(spec, X, y, y_err, 8, nbr_in=bad)
    assert rc == -1 and "row 17" in msg and "-1" in msg and untouched(out)
    for v in (300, -2, 2 ** 31 - 1):
        bad = nbr.copy()
        bad[299, 7] = v
        rc, msg, out = raw_call(spec, X, y, y_err, 8, nbr_in=bad)
        assert rc == -1 and "row 299" in msg and "outside" in msg and untouched(out)
    # a row repeated within a list is not an argument error: that row's matrix is singular, and only that row fails
    bad = nbr.copy()
    bad[5, 1] = bad[5, 0]
    rc, msg, out = raw_call(spec, X, y, None, 8, nbr_in=bad)
    assert rc == 0 and out["info"][5] > 0 and np.count_nonzero(out["info"]) == 1 and out["sums"][2] == 1.0
    # ranks
    rank = ops.vecchia_rank(300, seed=1)
    for at, v in ((120, int(rank[3])), (0, 300), (299, -1)):
        r = rank.copy()
        r[at] = v
        rc, msg, out = raw_call(spec, X, y, y_err, 8, mode=1, rank=r)
        # the entry named is the first offender: for a repeat the later of the two
        assert rc == -1 and "rank[%d]" % at in msg and "permutation" in msg and untouched(out), msg
    rc, msg, out = raw_call(spec, X, y, y_err, 8, mode=1, rank=None)
    assert rc == -1 and "rank" in msg and untouched(out)
    rc, msg, out = raw_call(spec, X, y, y_err, 8, mode=2)
    assert rc == -1 and "mode" in msg and untouched(out)
    for kn in (0, 129, -1):
        rc, msg, out = raw_call(spec, X, y, y_err, kn)
        assert rc == -1 and "kn" in msg and untouched(out)
    rc, msg, out = raw_call(spec, X, y, y_err, 8, want=("mu", "var", "nbr", "cnt", "sums"))
    assert rc == -1 and "info" in msg and untouched(out)
    rc, msg, out = raw_call(LR.make_spec("arbf", a=1.0, b=2.0, c=1.0), X, y, y_err, 8)
    assert rc == -1 and "Cholesky" in msg and untouched(out)
    # every output but info is optional, and leaving them out changes nothing
    rc, msg, only = raw_call(spec, X, y, y_err, 8, want=("info",))
    assert rc == 0 and same_bits(only["info"], good["info"]) and all((only[key] == -7).all() for key in ("mu", "var", "nbr", "cnt", "sums"))
    rc, msg, some = raw_call(spec, X, y, y_err, 8, want=("info", "sums", "mu"))
    assert rc == 0 and same_bits(some["sums"], good["sums"]) and same_bits(some["mu"], good["mu"])
    # n = 1: nothing is eligible in either mode
    for mode, rank1 in ((0, None), (1, np.zeros(1, dtype=np.int32))):
        rc, msg, one = raw_call(spec, X[:1], y[:1], y_err[:1], 5, mode=mode, rank=rank1)
        assert rc == 0 and one["cnt"][0] == 0 and (one["nbr"] == -1).all() and one["mu"][0] == 0.0 and one["var"][0] == spec.amp
        s2 = spec.amp + y_err[0] ** 2
        assert abs(one["sums"][0] - np.log(s2)) <= 4e-16 * abs(np.log(s2)) and abs(one["sums"][1] - y[0] ** 2 / s2) <= 4e-16 * y[0] ** 2 / s2
    t = _lib.timings(_lib.get_ctx())
    assert t[0] > 0 and t[2] > 0 and t[3] > 0 and t[1] == 0 and all(v == 0 for v in t[4:])


# ---------------------------------------------------------------------------------------------------------
# independence
def independence_call():
    """mu, var, nbr, cnt, info, sums of 257 rows in both modes, straight from the library"""
    c = case("arbf")
    out = {}
    for mode, rank in ((0, None), (1, ops.vecchia_rank(257, seed=3))):
        rc, msg, o = raw_call(c["spec"], c["X"][:257], c["y"][:257], c["y_err"][:257], 33, mode=mode, rank=rank)
        assert rc == 0, msg
        out.update({"%s%d" % (key, mode): v for key, v in o.items()})
    return out


@pytest.mark.parametrize("chunk", ["1", "37"])
def test_outputs_do_not_depend_on_the_chunk(chunk):
    here = independence_call()
    assert not here["info0"].any() and not here["info1"].any()
    with tempfile.TemporaryDirectory() as folder:
        out = os.path.join(folder, "chunk.npz")
        env = dict(os.environ, TGP_LOCAL_CHUNK=chunk)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.load(out)
        assert str(got["chunk"]) == chunk
        for key, v in here.items():
            assert same_bits(got[key], v), key


def test_a_row_does_not_depend_on_rows_it_cannot_see():
    # PRIOR: the rows of rank above r play no part in the rows of rank <= r -- drop them and the bits stay
    c = case("avk")
    spec, X, y, y_err = c["spec"], c["X"][:257], c["y"][:257], c["y_err"][:257]
    rank = ops.vecchia_rank(257, seed=3)
    mu, var, sums, nbr, cnt = ops.gp_local_cond(spec, X, y, y_err, k=33, mode="prior", rank=rank, return_neighbors=True)
    keep = np.flatnonzero(rank < 100)
    mu_s, var_s, _, nbr_s, cnt_s = ops.gp_local_cond(spec, X[keep], y[keep], y_err[keep], k=33, mode="prior", rank=rank[keep],
                                                     return_neighbors=True)
    assert same_bits(mu_s, mu[keep]) and same_bits(var_s, var[keep]) and same_bits(cnt_s, cnt[keep])
    assert np.array_equal(np.where(nbr_s >= 0, keep[nbr_s], -1), nbr[keep])


@pytest.mark.parametrize("k", [1, 2, 4])
def test_low_ranks_that_examine_the_whole_table(k):
    # PRIOR: the rows of rank below max(n / 1024, k) examine the whole table instead of walking rings.  At the other tests' sizes only
    # rank < k does; at n = 8192 the ranks k .. 7 do as well, with more predecessors than they keep, and rank 8 on walks rings: the
    # lists of the first 24 ranks against brute force, row for row (uniform points: no ties), and their values
    n = 8192
    spec = LR.make_spec("arbf")
    X, y, y_err, _ = LR.uniform_data(n, 1, seed=8192)
    rank = ops.vecchia_rank(n, seed=7)
    mu, var, sums, nbr, cnt = ops.gp_local_cond(spec, X, y, y_err, k=k, mode="prior", rank=rank, return_neighbors=True)
    rows = np.argsort(rank)[:24]
    D = LR.dist2(spec, X, X[rows])                                        # (24, n)
    E = rank[None, :] < rank[rows][:, None]
    order = np.argsort(np.where(E, D, np.inf), axis=1, kind="stable")
    for j, i in enumerate(rows):
        c = min(k, j)
        assert cnt[i] == c and list(nbr[i, :c]) == list(order[j, :c]) and (nbr[i, c:] == -1).all(), "rank %d" % j
    assert np.array_equal(cnt, np.minimum(rank, k))
    r_mu, r_var, r_info = VR.cond_ld(spec, X, y, y_err, nbr, cnt, rows=rows)
    assert not r_info.any()
    assert np.abs(mu[rows] - r_mu).max() <= 1e-10 * np.abs(y).max() and np.abs(var[rows] - r_var).max() <= 1e-10 * spec.amp
    check_sums(y, y_err, mu, var, sums, "n = 8192 k = %d" % k)


# ---------------------------------------------------------------------------------------------------------
# failure
def test_failed_rows_leave_the_others_alone():
    """The coincident-noiseless construction of test_gpu_local.test_a_failed_query_leaves_the_others_alone: amp = 1/4 makes
    sqrt(amp) and the first column of the factor exact, so two coincident rows without noise at the head of a list give a second
    pivot of exactly 0 in any arithmetic.  In LOO mode a row is not in its own list, so a coincident PAIR shows each of its rows
    one copy only and nothing fails; three coincident rows show each of them the other two: these three rows report info = 2."""
    spec = LR.make_spec("rbf", amp=0.25)
    rng = np.random.default_rng(23)
    X = np.vstack([rng.uniform(size=(1000, 2)), [[2.0, 2.0], [2.0, 2.0], [2.0, 2.0]]])
    y = np.sin(5.0 * X[:, 0]) + X[:, 1]
    y_err = np.append(np.full(1000, np.sqrt(2.5e-3 * 0.25)), [0.0, 0.0, 0.0])
    with pytest.raises(np.linalg.LinAlgError, match=r"row 1000: the 2-th leading minor .* \(3 of 1003 rows failed\)") as ei:
        ops.gp_local_cond(spec, X, y, y_err, k=8, return_neighbors=True)
    info = ei.value.info
    mu, var, sums, nbr, cnt = ei.value.results
    assert list(info[1000:]) == [2, 2, 2] and np.count_nonzero(info) == 3 and sums[2] == 3.0
    assert np.isnan(mu[1000:]).all() and np.isnan(var[1000:]).all()
    assert list(nbr[1000, :2]) == [1001, 1002] and list(nbr[1001, :2]) == [1000, 1002] and list(nbr[1002, :2]) == [1000, 1001]
    _, _, ref_info = VR.cond_ld(spec, X, y, y_err, nbr, cnt, rows=[1000, 1001, 1002])
    assert list(ref_info) == [2, 2, 2]
    # every other row: the bits of a call without the three, the sums included (they run over the rows that did not fail)
    mu_o, var_o, sums_o, nbr_o, cnt_o = ops.gp_local_cond(spec, X[:1000], y[:1000], y_err[:1000], k=8, return_neighbors=True)
    assert same_bits(mu_o, mu[:1000]) and same_bits(var_o, var[:1000]) and same_bits(nbr_o, nbr[:1000]) and same_bits(cnt_o, cnt[:1000])
    assert same_bits(sums_o[:2], sums[:2]) and sums_o[2] == 0.0
    VR.check_lists(spec, X[:1000], nbr_o, cnt_o, 8, "loo")
    e_m, e_v, _, _ = value_errors(spec, X[:1000], y[:1000], y_err[:1000], mu_o, var_o, nbr_o, cnt_o)
    assert e_m <= 1e-10 and e_v <= 1e-10
    check_sums(y[:1000], y_err[:1000], mu[:1000], var[:1000], np.array([sums[0], sums[1], 0.0]), "failed rows left out")
    # a coincident pair alone fails nowhere in LOO mode
    mu_p, var_p, sums_p = ops.gp_local_cond(spec, X[:1002], y[:1002], y_err[:1002], k=8)
    assert sums_p[2] == 0.0 and np.isfinite(mu_p).all()
    # through the object: -inf for the scores, an error naming the row for the predictions
    gp = tg.GPInterpolation(kernel="0.5**2 * RBF(0.15)", optimizer="none", normalize=False)
    gp.initialize(X, y, y_err=y_err)
    assert gp.return_loo_log_predictive_local(k=8) == -np.inf
    rank = ops.vecchia_rank(1003, seed=0)
    last = int(np.argmax(rank[1000:])) + 1000                     # the last of the three in the ordering sees the other two
    with pytest.raises(np.linalg.LinAlgError, match="row %d" % last):
        ops.gp_local_cond(spec, X, y, y_err, k=8, mode="prior", rank=rank)
    assert gp.return_log_likelihood_local(k=8) == -np.inf
    with pytest.raises(np.linalg.LinAlgError, match="row 1000"):
        gp.predict_loo_local(k=8)


# ---------------------------------------------------------------------------------------------------------
# what a context carries between calls
def test_predict_bits_do_not_move_across_a_local_cond_call():
    c = case("arbf")
    spec, X, y, y_err = c["spec"], c["X"][:700], c["y"][:700], c["y_err"][:700]
    Xs = np.random.default_rng(3).uniform(size=(300, 2))
    alpha = ops.gp_solve(spec, X, y, y_err)[0]
    before = ops.gp_predict(spec, X, alpha, Xs)
    before_local = ops.gp_predict_local(spec, X, y, y_err, Xs, k=64, return_var=True, return_neighbors=True)
    first = ops.gp_local_cond(spec, X, y, y_err, k=64, mode="prior", rank=ops.vecchia_rank(700), return_neighbors=True)
    ops.gp_local_cond(spec, X, y, y_err, k=17)
    assert same_bits(ops.gp_predict(spec, X, alpha, Xs), before)
    after_local = ops.gp_predict_local(spec, X, y, y_err, Xs, k=64, return_var=True, return_neighbors=True)
    assert all(same_bits(a, b) for a, b in zip(before_local, after_local))
    again = ops.gp_local_cond(spec, X, y, y_err, k=64, mode="prior", rank=ops.vecchia_rank(700), return_neighbors=True)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    assert same_bits(ops.gp_solve(spec, X, y, y_err)[0], alpha)


# ---------------------------------------------------------------------------------------------------------
# the fit
def test_local_likelihood_fit(monkeypatch):
    from treegp_amd.sampling import gaussian_random_field
    n = 1500
    rng = np.random.default_rng(31)
    X = rng.uniform(size=(n, 2))
    y_err = np.full(n, 0.05)
    truth = "0.8**2 * AnisotropicRBF(invLam=array([[60., -14.], [-14., 35.]]))"
    y = gaussian_random_field(truth, X, random_state=5, y_err=y_err)[:, 0]
    start = "0.5**2 * AnisotropicRBF(invLam=array([[30., 0.], [0., 30.]]))"
    gp = tg.GPInterpolation(kernel=start, optimizer="local-likelihood", normalize=False, local_k=32, local_seed=1)
    gp.initialize(X, y, y_err=y_err)
    ll_local_start, ll_dense_start = gp.return_log_likelihood_local(k=32, seed=1), gp.return_log_likelihood()
    seen = []
    real = ops.gp_local_cond

    def spy(*a, **kw):
        seen.append(kw.get("neighbors"))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "gp_local_cond", spy)
    gp.solve()
    monkeypatch.setattr(ops, "gp_local_cond", real)
    # one search, at the starting kernel; then one list for every evaluation
    assert seen[0] is None and len(seen) > 5 and all(s is seen[1] for s in seen[1:]) and seen[1] is gp._optimizer._neighbors
    lists0, _ = ops.gp_local_cond(gp._local_spec("test", gp.kernel.clone_with_theta(gp._init_theta[0])), X, y, y_err, k=32,
                                  mode="prior", rank=ops.vecchia_rank(n, 1), return_neighbors=True)[3:]
    assert same_bits(lists0, seen[1])
    ll_local, ll_dense = gp._optimizer._logL, gp.return_log_likelihood()
    print("local-likelihood fit, n = %d, k = 32, %d evaluations: local log L %.3f -> %.3f, dense log L %.3f -> %.3f"
          % (n, len(seen) - 1, ll_local_start, ll_local, ll_dense_start, ll_dense))
    print("   fitted kernel: %r" % (gp.kernel,))
    assert np.isfinite(ll_local) and ll_local > ll_local_start
    assert ll_dense >= ll_dense_start
    # how far from the dense fit's optimum: a property of the method, reported and not asserted
    gd = tg.GPInterpolation(kernel=start, optimizer="log-likelihood", normalize=False)
    gd.initialize(X, y, y_err=y_err)
    gd.solve()
    print("   dense fit: log L %.3f, kernel %r; theta local - dense = %s" % (gd._optimizer._logL, gd.kernel, gp.kernel.theta - gd.kernel.theta))


if __name__ == "__main__":
    np.savez(sys.argv[1], chunk=os.environ.get("TGP_LOCAL_CHUNK", ""), **independence_call())

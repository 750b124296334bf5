"""GPU tests of the batched routes for sums of kernels (include/tgp.h, seam S2i).

The values the batched K build stores are read back through ``ops.kbuild_batch`` and compared bit for bit with the fp64 sum, in
term order, of what the one-term batched build stores for each term; the one-term batched build itself is held to mpmath here,
pair by pair (test_gpu_kernel_values.py does that for the single-problem routes only), so bit equality is the whole accuracy
statement of a stored value.  Solve, leave-one-out, posterior and gradient are held to the tolerances test_gpu_ksum.py and
test_gpu_solve_batch.py use at this conditioning.

cond(K + diag(y_err^2)) of the accuracy batch on the CPU (numpy.linalg.cond of S.sum_matrix, the inputs of S.data(n)):
    n = 1     Sum A          1.0
    n = 40    Sum B          1.6e2
    n = 255   three terms    2.8e3
    n = 256   Sum A          2.8e3
    n = 257   Sum B          6.4e3
    n = 513   three terms    7.8e3
    n = 700   Sum A          9.5e3
    n = 1024  Sum B          3.3e4
all below 5e4.  The fixed problem of the independence test (Sum B, n = 700, y_err) has 1.4e4; the
sum of Gaussian terms only among its companions (n = 200, y_err) 2.0e4."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _kernel_value_helpers as H
import _ksum_refs as S
from _history_helpers import Ctx, raw
from test_gpu_ksum import assert_same_bits, in_term_order

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSS2 = "0.7**2 * RBF(0.1) + 0.5**2 * AnisotropicRBF(invLam=array([[30., 4.], [4., 20.]]))"      # every term Gaussian
GAUSS3 = GAUSS2 + " + 0.3**2 * RBF(0.25)"
M_QUERY = 257


def mods():
    import treegp_amd as tg
    from treegp_amd import _lib, kernels, ops
    return tg, _lib, kernels, ops


def sumspec(kern):
    tg, _, kernels, _ = mods()
    return kernels.kernel_to_sum_spec(tg.eval_kernel(kern))


def three_terms():
    ops = mods()[3]
    return ops.KernelSumSpec(sumspec(S.SUM_B).terms[:3])


def rotation():
    """Sum A, Sum B, the three-term sum, two single kernels, a sum of Gaussian terms only"""
    b = sumspec(S.SUM_B)
    return [sumspec(S.SUM_A), b, three_terms(), b.terms[1], b.terms[2], sumspec(GAUSS2)]


def terms_of(spec):
    return list(getattr(spec, "terms", [spec]))


def amp_of(spec):
    return spec.amp


# ---- 1. stored values, bit for bit ---------------------------------------------------------------------------------------------
KB_NS = (1, 127, 128, 129, 255, 256, 257, 513)


def kbuild_problems():
    rot = rotation()
    return [(rot[i % len(rot)], S.data(n)[0], S.data(n)[2]) for i, n in enumerate(KB_NS)]


@pytest.mark.parametrize("with_yerr", [True, False])
def test_batched_kbuild_of_a_sum_is_the_sum_of_the_one_term_builds_bit_for_bit(with_yerr):
    ops = mods()[3]
    probs = kbuild_problems()
    Ks = ops.kbuild_batch([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs] if with_yerr else None)
    # every term of every problem alone, all in one batch of one-term problems
    flat = [(b, t) for b, p in enumerate(probs) for t in terms_of(p[0])]
    Ts = ops.kbuild_batch([t for _, t in flat], [probs[b][1] for b, _ in flat])
    for b, (spec, X, e) in enumerate(probs):
        n = len(X)
        K = Ks[b]
        assert K.shape == (n, n)
        want = in_term_order([T for (bb, _), T in zip(flat, Ts) if bb == b])
        low = np.tril(np.ones((n, n), dtype=bool), -1)
        assert_same_bits(K[low], want[low], "problem %d (n = %d): strict lower triangle" % (b, n))
        assert not K[np.triu(np.ones((n, n), dtype=bool), 1)].any(), "problem %d: above the diagonal" % b
        d = amp_of(spec) + (e * e if with_yerr else 0.0) * np.ones(n)
        assert np.all(np.abs(np.diag(K) - d) <= 2 * np.spacing(d)), (b, np.abs(np.diag(K) - d).max())
        if not with_yerr:
            assert_same_bits(np.diag(K), np.full(n, amp_of(spec)), "problem %d: diagonal without noise" % b)


def test_batched_kbuild_is_exactly_zero_beyond_n_and_above_the_diagonal():
    """the raw (nb, nmax, nmax) array of the C entry, filled with NaN before the call"""
    _, _lib, _, ops = mods()
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    probs = kbuild_problems()[1:5]
    specs = [ops._as_sum(p[0]) for p in probs]
    ns, nmax, Xb, _, eb = ops.pad_batch([p[1] for p in probs], [np.zeros(len(p[1])) for p in probs], [p[2] for p in probs])
    ks = (_lib.TgpKernelSum * len(probs))(*[s.to_c() for s in specs])
    K = np.full((len(probs), nmax, nmax), np.nan)
    _lib.check(ctx, lib.tgp_kbuild_batch_sum(ctx, len(probs), ks, _lib.ptr(ns), nmax, _lib.ptr(Xb), _lib.ptr(eb), _lib.ptr(K)),
               "tgp_kbuild_batch_sum")
    i, j = np.meshgrid(np.arange(nmax), np.arange(nmax), indexing="ij")
    for b, n in enumerate(ns):
        outside = (i >= n) | (j > i)
        assert_same_bits(K[b][outside], np.zeros(int(outside.sum())), "problem %d: outside its lower triangle" % b)
        assert np.all(np.isfinite(K[b])) and np.all(np.diag(K[b])[:n] > 0)


def fixed_kbuild():
    return (sumspec(S.SUM_B), S.data(513)[0], S.data(513)[2])


def test_batched_kbuild_does_not_depend_on_companions_place_or_chunk():
    ops = mods()[3]
    P = fixed_kbuild()
    A = kbuild_problems()

    def build(batch, b):
        return ops.kbuild_batch([p[0] for p in batch], [p[1] for p in batch], [p[2] for p in batch])[b]
    alone = build([P], 0)
    assert_same_bits(build([P] + A, 0), alone, "first among companions")
    assert_same_bits(build(A[:3] + [P] + A[3:], 3), alone, "in the middle")
    assert_same_bits(build(A[5:] + [P], len(A[5:])), alone, "last, other companions")
    assert_same_bits(chunked()["kbuild"], alone, "TGP_BATCH_CHUNK=1")


# ---- 2. the batched single-kernel build against mpmath -------------------------------------------------------------------------
N_VALUES = 1024
POSITIONS = tuple(p for p in H.KB_POSITIONS if p < N_VALUES)


def value_case(kind):
    """(spec, training point, the 1023 other points, mpmath reference, bound, where the value must be 0)"""
    _, _lib, _, ops = mods()
    m = N_VALUES - 1
    if kind in ("rbf", "arbf"):
        a, b, c = (400.0, 0.0, 400.0) if kind == "rbf" else H.README_INVLAM
        spec = ops.KernelSpec(_lib.TGP_RBF if kind == "rbf" else _lib.TGP_ARBF, amp=1.7, a=a, b=b, c=c)
        Xq = H.gauss_queries(m=m + 1, seed=31)[1:]                   # (query 0 is the training point itself: the diagonal)
        ref, s = H.gauss_ref(Xq, H.GAUSS_XT, a, b, c, 1.7)
        return spec, H.GAUSS_XT, Xq, ref, H.gauss_bound(ref, s), ref < H.LD(1.7) * H.HALF_TINY
    amp, xo = 0.49, np.array([0.4, -0.2])
    Xo = H.vk_offaxis_queries(xo, H.VK_OFF_SCALE[kind], m=m)
    ref, xs = H.vk_ref_offaxis(Xo, xo, kind, amp, **H.VK_OFF[kind])
    return H.make_spec(kind, amp=amp, **H.VK_OFF[kind]), xo, Xo, ref, H.vk_bound(ref, amp, xs), xs > H.K56_XMAX * (1 + 1e-12)


@pytest.mark.parametrize("kind", ["rbf", "arbf", "vk", "avk"])
def test_batched_one_term_build_against_mpmath(kind):
    ops = mods()[3]
    spec, xt, Xq, ref, bound, zero = value_case(kind)
    Xs = [np.ascontiguousarray(np.insert(Xq, p, xt, axis=0)) for p in POSITIONS]
    Ks = ops.kbuild_batch([spec] * len(Xs), Xs)
    for p, K in zip(POSITIONS, Ks):
        assert K.shape == (N_VALUES, N_VALUES)
        v = np.concatenate([K[p, :p], K[p + 1:, p]])
        res = H.compare(v, ref, bound, must_be_zero=zero)
        print("%s, training point at row %d: worst error %.3f of the bound, %d values nonzero where the kernel is 0"
              % (kind, p, res["max_ratio"], res["nonzero_where_zero"]))
        assert res["max_ratio"] <= 1.0 and res["nonzero_where_zero"] == 0, (kind, p, res)
        assert np.all(np.diag(K) == spec.amp), (kind, p)


# ---- shared: every batched entry on one batch ----------------------------------------------------------------------------------
def every_entry(batch, Xq=None, ctx=None):
    """{name: list over the problems} of every batched entry that takes kernels; batch: [(spec, X, y, e)]"""
    ops = mods()[3]
    specs, Xs, ys = [p[0] for p in batch], [p[1] for p in batch], [p[2] for p in batch]
    es = None if batch[0][3] is None else [p[3] for p in batch]
    if Xq is None:
        Xq = [S.data(len(p[1]))[3] for p in batch]
    out = {}
    al, ld, c2, info = ops.gp_solve_batch(specs, Xs, ys, es, ctx=ctx)
    out.update({"solve.alpha": al, "solve.logdet": ld, "solve.chi2": c2, "solve.info": info})
    _, ld, c2, info = ops.gp_solve_batch(specs, Xs, ys, es, want_alpha=False, ctx=ctx)
    out.update({"noalpha.logdet": ld, "noalpha.chi2": c2, "noalpha.info": info})
    al, dg, ld, c2, info = ops.gp_loo_batch(specs, Xs, ys, es, ctx=ctx)
    out.update({"loo.alpha": al, "loo.invdiag": dg, "loo.logdet": ld, "loo.chi2": c2, "loo.info": info})
    for what in ("var", "cov"):
        al, un, ld, c2, info = ops.gp_posterior_batch(specs, Xs, ys, es, Xq, what=what, ctx=ctx)
        out.update({what + ".alpha": al, what + ".unc": un, what + ".logdet": ld, what + ".chi2": c2, what + ".info": info})
    ld, c2, g, info = ops.gp_solve_grad_batch_sum(specs, Xs, ys, es, ctx=ctx)
    out.update({"grad.logdet": ld, "grad.chi2": c2, "grad.rows": g, "grad.info": info})
    return out


def assert_problem_bits(got, b, ref, rb, what, skip=()):
    for k in ref:
        if k.endswith(".info"):
            assert got[k][b] == ref[k][rb] == 0, (what, k)
        elif k not in skip:
            assert_same_bits(got[k][b], ref[k][rb], "%s: %s" % (what, k))


# ---- 3. a zero-amplitude term changes no bit -----------------------------------------------------------------------------------
def test_a_zero_amplitude_term_changes_no_bit():
    _, _lib, _, ops = mods()
    avk = sumspec(S.SUM_A).terms[0]
    zero = ops.KernelSpec(_lib.TGP_ARBF, amp=0.0, a=30.0, b=4.0, c=20.0)
    data = [S.data(n) for n in (257, 513)]
    single = every_entry([(avk, X, y, None) for X, y, _, _ in data])
    for order in ([avk, zero], [zero, avk]):
        spec = ops.KernelSumSpec(order)
        got = every_entry([(spec, X, y, None) for X, y, _, _ in data])
        for b in range(2):
            assert_problem_bits(got, b, single, b, "zero term %s, n = %d" % ("last" if order[0] is avk else "first", len(data[b][0])),
                                skip=("grad.rows",))          # (the gradient has a row per term: not among the outputs compared)


# ---- 4. one term is the namesake -----------------------------------------------------------------------------------------------
def test_one_term_sums_are_the_namesakes_bit_for_bit():
    ops = mods()[3]
    b4 = sumspec(S.SUM_B).terms                                       # AVK, ARBF, VK, RBF
    ns = (40, 129, 257, 300)
    plain = [(t, S.data(n)[0], S.data(n)[1], S.data(n)[2]) for t, n in zip(b4, ns)]
    wrapped = [(ops.KernelSumSpec([p[0]]),) + p[1:] for p in plain]
    Xq = [S.data(n)[3][:m] for n, m in zip(ns, (1, 130, 257, 64))]
    with Ctx() as c:
        one = every_entry(wrapped, Xq, ctx=c.h)                      # every spec a KernelSumSpec: the _sum entries
    with Ctx() as c:
        ref = every_entry(plain, Xq, ctx=c.h)                        # none: the namesakes (the gradient: its own entry below)
        ld, c2, g4, info = ops.gp_solve_grad_batch_any([p[0] for p in plain], [p[1] for p in plain], [p[2] for p in plain],
                                                       [p[3] for p in plain], ctx=c.h)
    ref.update({"grad.logdet": ld, "grad.chi2": c2, "grad.rows": [g.reshape(1, 4) for g in g4], "grad.info": info})
    for b in range(4):
        assert one["grad.rows"][b].shape == (1, 4)
        assert_problem_bits(one, b, ref, b, "one-term problem %d" % b)


# ---- 5. accuracy ---------------------------------------------------------------------------------------------------------------
ACC_NS = (1, 40, 255, 256, 257, 513, 700, 1024)
_ACC = {}


def accuracy_batch():
    rot = [sumspec(S.SUM_A), sumspec(S.SUM_B), three_terms()]
    return [(rot[i % 3],) + S.data(n)[:3] for i, n in enumerate(ACC_NS)]


def accuracy_run():
    """the accuracy batch through every entry and its host references, made once and left unchanged"""
    if not _ACC:
        batch = accuracy_batch()
        _ACC["got"] = every_entry(batch)
        _ACC["host"] = [S.host_solve(S.sum_matrix(spec, X), y, e) for spec, X, y, e in batch]
    return accuracy_batch(), _ACC["got"], _ACC["host"]


def loglike(n, logdet, chi2):
    return -0.5 * chi2 - 0.5 * n * np.log(2 * np.pi) - 0.5 * logdet


def test_accuracy_of_the_batched_solve_of_sums():
    ops = mods()[3]
    batch, got, host = accuracy_run()
    assert not got["solve.info"].any()
    for b, ((spec, X, y, e), (ah, ldh, ydh, _)) in enumerate(zip(batch, host)):
        n, tag = len(X), "problem %d, n = %d" % (b, len(X))
        a1, ld1, yd1, _ = ops.gp_solve(spec, X, y, e)
        alpha, ld, c2 = got["solve.alpha"][b], got["solve.logdet"][b], got["solve.chi2"][b]
        print("%s: alpha %.2e (host) %.2e (single) of max, logdet %.2e, chi2 %.2e relative"
              % (tag, np.abs(alpha - ah).max() / np.abs(ah).max(), np.abs(alpha - a1).max() / np.abs(a1).max(),
                 abs(ld / ldh - 1), abs(c2 / ydh - 1)))
        for ar, ldr, ydr in ((ah, ldh, ydh), (a1, ld1, yd1)):
            np.testing.assert_allclose(alpha, ar, rtol=0, atol=1e-9 * np.abs(ar).max(), err_msg=tag)
            np.testing.assert_allclose([ld, c2], [ldr, ydr], rtol=1e-11, err_msg=tag)
            np.testing.assert_allclose(loglike(n, ld, c2), loglike(n, ldr, ydr), rtol=1e-11, err_msg=tag)
        for other in ("noalpha", "loo", "var", "cov", "grad"):
            assert got[other + ".logdet"][b] == ld and got[other + ".chi2"][b] == c2, (tag, other)


def test_accuracy_of_the_batched_inverse_diagonal_of_sums():
    batch, got, host = accuracy_run()
    for b, (_, _, _, Kinv) in enumerate(host):
        np.testing.assert_allclose(got["loo.invdiag"][b], np.diag(Kinv), rtol=1e-9, atol=0, err_msg="problem %d" % b)
        assert_same_bits(got["loo.alpha"][b], got["solve.alpha"][b], "alpha of the loo entry, problem %d" % b)


def test_accuracy_of_the_batched_posterior_of_sums():
    ops = mods()[3]
    batch, got, _ = accuracy_run()
    for b, (spec, X, y, e) in enumerate(batch):
        Xs = S.data(len(X))[3]
        _, _, _, fac = ops.gp_solve(spec, X, y, e, keep=True)
        try:
            cov1 = ops.gp_predict_cov(spec, fac, X, Xs)
            var1 = ops.gp_predict_var(spec, fac, X, Xs)
        finally:
            fac.free()
        cov, var = got["cov.unc"][b], got["var.unc"][b]
        print("problem %d, n = %d: cov %.2e, var %.2e of the sum's amplitude"
              % (b, len(X), np.abs(cov - cov1).max() / spec.amp, np.abs(var - var1).max() / spec.amp))
        np.testing.assert_allclose(cov, cov1, rtol=0, atol=1e-9 * spec.amp, err_msg="problem %d" % b)
        np.testing.assert_allclose(var, var1, rtol=0, atol=1e-9 * spec.amp, err_msg="problem %d" % b)
        np.testing.assert_allclose(var, np.diag(cov), rtol=0, atol=1e-12 * spec.amp, err_msg="problem %d" % b)
        for what in ("var", "cov"):
            assert_same_bits(got[what + ".alpha"][b], got["solve.alpha"][b], "alpha of the %s entry, problem %d" % (what, b))


def test_accuracy_of_the_batched_gradient_rows_of_sums():
    batch, got, host = accuracy_run()
    for b, ((spec, X, y, e), (ah, _, _, Kinv)) in enumerate(zip(batch, host)):
        ref = S.host_grad_rows(spec, X, ah, Kinv)
        g = got["grad.rows"][b]
        assert g.shape == ref.shape == (len(spec.terms), 4)
        print("problem %d, n = %d: worst |g - ref| / max(|ref|, 1) = %.3e"
              % (b, len(X), (np.abs(g - ref) / np.maximum(np.abs(ref), 1.0)).max()))
        np.testing.assert_allclose(g, ref, rtol=1e-8, atol=1e-8 * max(np.abs(ref).max(), 1.0), err_msg="problem %d" % b)


def test_gradient_rows_beyond_the_term_count_are_exactly_zero():
    """the raw (nb, TGP_SUM_MAX, 4) array of the C entry, filled with NaN before the call"""
    _, _lib, _, ops = mods()
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    batch = accuracy_batch()[2:5]                                    # three, two and four terms
    ns, nmax, Xb, yb, eb = ops.pad_batch([p[1] for p in batch], [p[2] for p in batch], [p[3] for p in batch])
    nb = len(batch)
    ks = (_lib.TgpKernelSum * nb)(*[p[0].to_c() for p in batch])
    ld, c2, info = np.empty(nb), np.empty(nb), np.zeros(nb, dtype=np.int32)
    g = np.full((nb, _lib.TGP_SUM_MAX, 4), np.nan)
    _lib.check(ctx, lib.tgp_gp_solve_grad_batch_sum(ctx, nb, ks, _lib.ptr(ns), nmax, _lib.ptr(Xb), _lib.ptr(yb), _lib.ptr(eb),
                                                    _lib.ptr(ld), _lib.ptr(c2), _lib.ptr(g), _lib.ptr(info)), "grad")
    for b, p in enumerate(batch):
        nt = len(p[0].terms)
        assert np.all(np.isfinite(g[b, :nt])) and g[b, :nt].any()
        assert_same_bits(g[b, nt:], np.zeros((_lib.TGP_SUM_MAX - nt, 4)), "problem %d: rows from %d on" % (b, nt))


# ---- 6. independence and isolation ---------------------------------------------------------------------------------------------
def fixed_problem():
    return (sumspec(S.SUM_B),) + S.data(700)[:3]


def companions(which):
    """three different sets: other term counts and kinds, sums of Gaussian terms only among them"""
    rot = rotation() + [sumspec(GAUSS3)]
    ns = [(300, 64, 513, 129), (257, 1, 700, 40, 130), (90, 513, 256)][which]
    return [(rot[(i + 2 * which) % len(rot)],) + S.data(n)[:3] for i, n in enumerate(ns)] + \
           [(sumspec(GAUSS2 if which != 1 else GAUSS3),) + S.data(200)[:3]]


def query_points(batch):
    return [S.data(len(p[1]))[3][:M_QUERY] for p in batch]


_ALONE = {}


def alone():
    if not _ALONE:
        _ALONE.update(every_entry([fixed_problem()]))
    return _ALONE


CHUNK_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_ksum_batch as T
from treegp_amd import ops
P, Q = T.fixed_problem(), T.fixed_kbuild()
A, B = T.companions(0), T.kbuild_problems()
out = T.every_entry(A[:2] + [P] + A[2:])
flat = {k: np.asarray(v[2], dtype=np.float64) for k, v in out.items()}
batch = B[:3] + [Q] + B[3:]
flat["kbuild"] = ops.kbuild_batch([p[0] for p in batch], [p[1] for p in batch], [p[2] for p in batch])[3]
np.savez(%r, **flat)
print("OK")
'''
_CHUNKED = {}


def chunked():
    """the fixed problems among companions with TGP_BATCH_CHUNK=1, in a process of their own with that environment (as
    test_gpu_solve_batch.py sets it); run once"""
    if not _CHUNKED:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "chunk1.npz")
            env = dict(os.environ, TGP_BATCH_CHUNK="1")
            code = CHUNK_SCRIPT % (ROOT, os.path.join(ROOT, "tests"), out)
            r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
            with np.load(out) as z:
                _CHUNKED.update({k: z[k] for k in z.files})
    return _CHUNKED


def test_a_sum_problem_does_not_depend_on_its_batch_bit_for_bit(monkeypatch):
    monkeypatch.delenv("TGP_BATCH_CHUNK", raising=False)
    P, ref = fixed_problem(), alone()
    for which, place in ((0, 0), (1, 3), (2, 4)):
        A = companions(which)
        batch = A[:place] + [P] + A[place:]
        assert_problem_bits(every_entry(batch), place, ref, 0, "companions %d, place %d" % (which, place))
    one = chunked()
    for k in ref:
        if k.endswith(".info"):
            assert one[k] == 0, k
        else:
            assert_same_bits(one[k], ref[k][0], "TGP_BATCH_CHUNK=1: " + k)


def test_a_singular_sum_problem_fails_alone():
    rng = np.random.default_rng(1)
    A = companions(0)
    good = A[:2] + [fixed_problem()] + A[2:]
    Xd = np.tile(rng.uniform(0, 1, (10, 2)), (20, 1))              # ten points, each twenty times, no noise: K has rank 10
    bad = (sumspec(GAUSS2), Xd, rng.standard_normal(200), np.zeros(200))
    ref = every_entry(good)
    at = 3
    with_bad = every_entry(good[:at] + [bad] + good[at:])
    for k in ref:
        if k.endswith(".info"):
            assert with_bad[k][at] > 0, (k, with_bad[k])
            assert not np.delete(with_bad[k], at).any(), (k, with_bad[k])
    for b in range(len(good)):
        assert_problem_bits(with_bad, b + (b >= at), ref, b, "problem %d beside the singular one" % b)
    assert_problem_bits(ref, 2, alone(), 0, "the fixed problem in this batch")


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------
def raw_batch_calls(c, ks, nb, ns, nmax, Xb, yb, eb, Xq):
    """{entry: (return code, message)} of the five entries of seam S2i called with the ctypes sums `ks`"""
    _lib = mods()[1]
    lib, p = c.lib, _lib.ptr
    m = Xq.shape[1]
    ms = np.full(nb, m, dtype=np.int64)
    out = np.empty(nb * max(nmax * nmax, m * m, 16))
    alpha, ld, c2, info = np.empty((nb, nmax)), np.empty(nb), np.empty(nb), np.zeros(nb, dtype=np.int32)
    calls = {
        "tgp_gp_solve_batch_sum": lambda: lib.tgp_gp_solve_batch_sum(c.h, nb, ks, p(ns), nmax, p(Xb), p(yb), p(eb), p(alpha), p(ld),
                                                                     p(c2), p(info)),
        "tgp_gp_posterior_batch_sum": lambda: lib.tgp_gp_posterior_batch_sum(c.h, nb, ks, p(ns), nmax, p(Xb), p(yb), p(eb), p(ms), m,
                                                                             p(Xq), 1, p(alpha), p(out), p(ld), p(c2), p(info)),
        "tgp_gp_loo_batch_sum": lambda: lib.tgp_gp_loo_batch_sum(c.h, nb, ks, p(ns), nmax, p(Xb), p(yb), p(eb), p(alpha), p(out),
                                                                 p(ld), p(c2), p(info)),
        "tgp_gp_solve_grad_batch_sum": lambda: lib.tgp_gp_solve_grad_batch_sum(c.h, nb, ks, p(ns), nmax, p(Xb), p(yb), p(eb), p(ld),
                                                                               p(c2), p(out), p(info)),
        "tgp_kbuild_batch_sum": lambda: lib.tgp_kbuild_batch_sum(c.h, nb, ks, p(ns), nmax, p(Xb), p(eb), p(out)),
    }
    res = {}
    for name, fn in calls.items():
        rc = fn()
        res[name] = (rc, (lib.tgp_last_error(c.h) or b"").decode())
    return res


def test_bad_sums_are_rejected_by_name_problem_and_term_and_leave_the_context_as_new():
    _, _lib, _, ops = mods()
    batch = [(sumspec(S.SUM_B),) + S.data(n)[:3] for n in (130, 64, 200, 257, 90)]
    Xq = [S.data(len(p[1]))[3][:70] for p in batch]
    with Ctx() as c:
        fresh = every_entry(batch, Xq, ctx=c.h)
    ns, nmax, Xb, yb, eb = ops.pad_batch([p[1] for p in batch], [p[2] for p in batch], [p[3] for p in batch])
    nb = len(batch)
    Xqb = np.ascontiguousarray(np.stack(Xq))
    with Ctx() as c:
        for what, where, edit in (("nterms = 0", "ks[1]", lambda ks: setattr(ks[1], "nterms", 0)),
                                  ("nterms = 5", "ks[4]", lambda ks: setattr(ks[4], "nterms", 5)),
                                  ("unknown kind", "ks[3].term[2]", lambda ks: setattr(ks[3].term[2], "kind", 99))):
            ks = (_lib.TgpKernelSum * nb)(*[p[0].to_c() for p in batch])
            edit(ks)
            for name, (rc, msg) in raw_batch_calls(c, ks, nb, ns, nmax, Xb, yb, eb, Xqb).items():
                assert rc == -1, (what, name, rc, msg)
                assert name + ":" in msg and where in msg, (what, name, msg)
        again = every_entry(batch, Xq, ctx=c.h)
    for b in range(nb):
        assert_problem_bits(again, b, fresh, b, "after the rejected calls, problem %d" % b)


# ---- 8. the API ----------------------------------------------------------------------------------------------------------------
TREE = "0.5**2 * RBF(0.2) + WhiteKernel(0.01)"
API_KERNELS = [(S.SUM_A, 300), ("0.5**2 * RBF(0.2)", 257), (S.SUM_B, 513), (TREE, 150), (GAUSS2, 200),
               ("0.3**2 * AnisotropicVonKarman(invLam=array([[40., -9.], [-9., 25.]]))", 129)]
BATCHED = (0, 1, 2, 4, 5)


def make_gp(kern, n, **kw):
    tg = mods()[0]
    X, y, e, _ = S.data(n)
    gp = tg.GPInterpolation(kernel=kern, optimizer=kw.pop("optimizer", "none"), normalize=True, **kw)
    gp.initialize(np.array(X), np.array(y), y_err=np.array(e))
    return gp


def api_objects():
    return [make_gp(k, n) for k, n in API_KERNELS]


def prior_amp(gp):
    return mods()[2].device_spec(gp.kernel).amp


class Counted(object):
    """counts the sums and single kernels a batched ops call is handed"""

    def __init__(self, monkeypatch, name):
        ops = mods()[3]
        self.real, self.sums, self.singles = getattr(ops, name), 0, 0
        monkeypatch.setattr(ops, name, self)

    def __call__(self, specs, *a, **k):
        ops = mods()[3]
        specs = list(specs)
        self.sums += sum(isinstance(s, ops.KernelSumSpec) for s in specs)
        self.singles += sum(isinstance(s, ops.KernelSpec) for s in specs)
        return self.real(specs, *a, **k)


@pytest.mark.parametrize("what", [None, "var", "cov"])
def test_predict_many_takes_sums_into_the_batch(what, monkeypatch):
    tg = mods()[0]
    kw = {} if what is None else {"return_" + what: True}
    Xq = [S.data(n)[3][:m] for (_, n), m in zip(API_KERNELS, (40, 257, 130, 70, 1, 64))]
    seen = Counted(monkeypatch, "gp_solve_batch" if what is None else "gp_posterior_batch")
    got = tg.predict_many(api_objects(), Xq, **kw)
    assert (seen.sums, seen.singles) == (3, 2)
    want = [gp.predict(X, **kw) for gp, X in zip(api_objects(), Xq)]
    for i, (g, w, gp) in enumerate(zip(got, want, api_objects())):
        y, yw = (g, w) if what is None else (g[0], w[0])
        if i not in BATCHED:
            assert np.array_equal(y, yw), i
            continue
        np.testing.assert_allclose(y, yw, rtol=0, atol=1e-10 * np.abs(yw).max(), err_msg="%s %d" % (what, i))
        if what is not None:
            assert g[1].shape == w[1].shape
            np.testing.assert_allclose(g[1], w[1], rtol=0, atol=1e-12 * prior_amp(gp), err_msg="%s %d" % (what, i))


def test_predict_loo_many_and_loo_log_predictive_many_take_sums_into_the_batch(monkeypatch):
    tg = mods()[0]
    seen = Counted(monkeypatch, "gp_loo_batch")
    got = tg.predict_loo_many(api_objects(), return_var=True)
    assert (seen.sums, seen.singles) == (3, 2)
    for i, ((y, v), gp) in enumerate(zip(got, api_objects())):
        yw, vw = gp.predict_loo(return_var=True)
        if i not in BATCHED:
            assert np.array_equal(y, yw) and np.array_equal(v, vw), i
            continue
        np.testing.assert_allclose(y, yw, rtol=0, atol=1e-9 * prior_amp(gp), err_msg=str(i))
        np.testing.assert_allclose(v, vw, rtol=0, atol=1e-9 * prior_amp(gp), err_msg=str(i))
    scores = tg.loo_log_predictive_many(api_objects())
    assert (seen.sums, seen.singles) == (6, 4)
    for i, (s, gp) in enumerate(zip(scores, api_objects())):
        np.testing.assert_allclose(s, gp.return_loo_log_predictive(), rtol=1e-10, err_msg=str(i))


def test_log_likelihood_many_takes_sums_into_the_batch(monkeypatch):
    tg = mods()[0]
    from treegp_amd.log_likelihood import log_likelihood
    X, y, e, _ = S.data(300)
    kernels = [tg.eval_kernel(k) for k, _ in API_KERNELS]
    like = log_likelihood(np.array(X), np.array(y), np.array(e))
    seen = Counted(monkeypatch, "gp_solve_batch")
    got = like.log_likelihood_many(kernels)
    assert (seen.sums, seen.singles) == (3, 2)
    want = [like.log_likelihood(k) for k in kernels]
    np.testing.assert_allclose(got, want, rtol=1e-11)


FIT_N = 300
_FIT = {}


def fit_objects():
    """B = 4 objects with the two-term Sum A as the start, each with a field of its own drawn from that kernel"""
    tg = mods()[0]
    X, e = np.array(S.data(FIT_N)[0]), np.array(S.data(FIT_N)[2])
    if "y" not in _FIT:
        _FIT["y"] = tg.gaussian_random_field(S.SUM_A, X, n_samples=4, random_state=2, y_err=e)
    gps = []
    for b in range(4):
        gp = tg.GPInterpolation(kernel=S.SUM_A, optimizer="log-likelihood", normalize=False)
        gp.initialize(X, _FIT["y"][:, b].copy(), y_err=e)
        gps.append(gp)
    return gps


def own_fits():
    """each object's own solve(): (theta, log L), made once"""
    if "own" not in _FIT:
        own = []
        for gp in fit_objects():
            gp.solve()
            own.append((gp.kernel.theta.copy(), gp._optimizer._logL))
        _FIT["own"] = own
    return _FIT["own"]


@pytest.mark.parametrize("gradient", ["auto", "analytic-vk"])
def test_solve_many_of_sums_reaches_each_objects_own_optimum(gradient, monkeypatch):
    tg = mods()[0]
    monkeypatch.delenv("TGP_ML_GRADIENT", raising=False)
    own = own_fits()
    exact = Counted(monkeypatch, "gp_solve_grad_batch_sum")
    fd = Counted(monkeypatch, "gp_solve_batch")
    gps = fit_objects()
    tg.solve_many(gps, gradient=gradient)
    assert (exact.sums > 0) == (gradient == "analytic-vk") and fd.sums > 0 and fd.singles == 0
    for b, (gp, (theta, logl)) in enumerate(zip(gps, own)):
        print("%s, object %d: log L %.10f against its own solve()'s %.10f, theta off by %.2e"
              % (gradient, b, gp._optimizer._logL, logl, np.abs(gp.kernel.theta - theta).max()))
        assert gp._optimizer._logL >= logl - 1e-6 * abs(logl), (gradient, b, gp._optimizer._logL, logl)
        np.testing.assert_allclose(gp.kernel.theta, theta, atol=2e-3, err_msg="%s, object %d" % (gradient, b))
        assert gp._alpha is None and len(gp._init_theta) == 1

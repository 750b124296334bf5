"""Helpers of tests/test_gpu_history.py: problems, routes, histories and oracle checks.

A *route* is one public call sequence whose outputs are compared bit for bit (``exact``) or, for the fp64-atomic sums whose
order of addition is not fixed, against the oracle (``sums``).  A *history* is a sequence of legal public calls that leaves
the context's recycled state (scratch, staging, factor cache, slabs, counters, accumulators) in a particular condition.
Nothing here touches a context other than through treegp_amd.ops / the C ABI."""
import ctypes as C
import os

import numpy as np

from oracle import gp_oracle as O

SIZES = dict(S=130, M=1290, L=2100, XL=4479)          # Np = 256, 1536, 2304, 4608: all with live padding
LARGER = dict(S=1290, M=2100, L=4479, XL=4900)        # the next size class up
QUERIES = (1, 130, 300)                               # query counts of the kept-factor routes
PREDICT_M = (1, 257, 700)


def padded(n):
    return (n + 255) // 256 * 256


def _mods():
    from treegp_amd import _lib, ops
    return _lib, ops


class Ctx(object):
    """A context of its own (``_lib.new_ctx(0)``), destroyed on exit after the factors made on it."""

    def __init__(self):
        _lib, _ = _mods()
        self.lib = _lib.load_library()
        self.h = _lib.new_ctx(0)
        self.facs = []

    def track(self, fac):
        self.facs.append(fac)
        return fac

    def close(self):
        try:
            for f in self.facs:
                f.free()
        finally:
            self.facs = []
            if self.h is not None:
                self.lib.tgp_destroy(self.h)
                self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ---- comparison -----------------------------------------------------------------------------------------------------------

def raw(a):
    a = np.asarray(a)
    if a.dtype.kind in "iub":
        return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.int64)


def assert_same_bits(got, ref, what):
    assert [k for k, _ in got] == [k for k, _ in ref], (what, [k for k, _ in got], [k for k, _ in ref])
    for (k, a), (_, b) in zip(got, ref):
        ra, rb = raw(a), raw(b)
        assert np.shape(a) == np.shape(b), (what, k, np.shape(a), np.shape(b))
        if not np.array_equal(ra, rb):
            bad = np.nonzero(ra != rb)[0]
            fa, fb = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
            raise AssertionError("%s: output %r differs from the fresh context's at %d of %d values, first at %d: %r vs %r"
                                 % (what, k, len(bad), len(ra), bad[0], fa[bad[0]], fb[bad[0]]))


def close_abs(got, ref, tol, what):
    """max |got - ref| <= tol, NaN pattern equal"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok]).max(initial=0.0)
    assert err <= tol, "%s: error %.3e above %.3e" % (what, err, tol)


# ---- problems -------------------------------------------------------------------------------------------------------------

class Problem(object):
    """One GP problem.  Clean: the ARBF amp=1.3 a=30 b=4 c=20, e in [0.05, 0.2] problem of test_gpu_edge_cases up to n = 1300,
    the a=60 b=8 c=45, e in [0.05, 0.1] problem of test_alternative_kernel_paths_agree above.  Loud: coordinates elsewhere,
    y x 1e8, amp x 1e4, y_err x 1e2 (K + D scales by 1e4 as a whole: as positive definite as the clean one)."""

    def __init__(self, n, seed=0, loud=False):
        _lib, ops = _mods()
        rng = np.random.default_rng(1000 * seed + n)
        self.n, self.loud = n, loud
        self.X = rng.uniform(0, 1, (n, 2))
        if n <= 1300:
            self.y = rng.standard_normal(n)
            self.e = rng.uniform(0.05, 0.2, n)
            self.kw = dict(amp=1.3, a=30.0, b=4.0, c=20.0)
        else:
            self.y = np.sin(5 * self.X[:, 0]) + 0.1 * rng.standard_normal(n)
            self.e = rng.uniform(0.05, 0.1, n)
            self.kw = dict(amp=1.3, a=60.0, b=8.0, c=45.0)
        self.Xq = rng.uniform(0, 1, (max(PREDICT_M), 2))
        self.B = rng.standard_normal((3, n))
        self.Z = rng.standard_normal((3, n))
        self.vk = dict(amp=2.0, ell=0.3)
        if loud:
            self.X = self.X + 7.0
            self.Xq = self.Xq + 7.0
            self.y = self.y * 1e8
            self.e = self.e * 1e2
            self.B = self.B * 1e8
            self.Z = self.Z * 1e8
            self.kw = dict(self.kw, amp=self.kw["amp"] * 1e4)
            self.vk = dict(self.vk, amp=self.vk["amp"] * 1e4)
        self.spec = ops.KernelSpec(_lib.TGP_ARBF, **self.kw)
        self.vkspec = ops.KernelSpec(_lib.TGP_VK, **self.vk)
        self._c = {}

    def cached(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    @property
    def K(self):
        return self.cached("K", lambda: O.kernel_matrix("gauss", self.X, **self.kw))

    @property
    def alpha_ref(self):
        return self.cached("solve", lambda: O.gp_solve(self.K, self.y, self.e))[0]

    @property
    def logdet_ref(self):
        return self.cached("solve", lambda: O.gp_solve(self.K, self.y, self.e))[1]

    @property
    def alpha_in(self):
        """the weights handed to the predict routes (a route's input, so the same on every context)"""
        return self.B[0] if self.loud else self.alpha_ref

    def HT(self, m):
        return self.cached(("HT", m), lambda: O.kernel_matrix("gauss", self.Xq[:m], self.X, **self.kw))

    def Kss(self, m):
        return self.cached(("Kss", m), lambda: O.kernel_matrix("gauss", self.Xq[:m], **self.kw))

    @property
    def Kinv(self):
        return self.cached("Kinv", lambda: np.linalg.inv(self.K + np.diag(self.e ** 2)))

    @property
    def starts(self):
        """inv_blocks groups of 1, 64 and 128 rows in turn"""
        s, i = [0], 0
        while s[-1] < self.n:
            s.append(min(self.n, s[-1] + (1, 64, 128)[i % 3]))
            i += 1
        return np.array(s, dtype=np.int64)


_PROBLEMS = {}


def problem(n, seed=0, loud=False):
    key = (n, seed, loud)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(n, seed, loud)
    return _PROBLEMS[key]


# ---- kept-factor calls ----------------------------------------------------------------------------------------------------

KEPT_CALLS = ("factor_solve", "gp_predict_var", "gp_predict_cov", "factor_inv_diag", "factor_inv_blocks", "factor_lmul",
              "gp_loglik_grad")


def kept_call_fns(c, P, alpha):
    """(name, fn(factor)) for every route that takes a kept factor; alpha is the argument of the likelihood gradient"""
    _, ops = _mods()
    fns = [("factor_solve", lambda f: ops.factor_solve(f, P.B, ctx=c.h))]
    for m in QUERIES:
        fns.append(("gp_predict_var[%d]" % m, lambda f, m=m: ops.gp_predict_var(P.spec, f, P.X, P.Xq[:m], ctx=c.h)))
    for m in QUERIES:
        fns.append(("gp_predict_cov[%d]" % m, lambda f, m=m: ops.gp_predict_cov(P.spec, f, P.X, P.Xq[:m], ctx=c.h)))
    fns.append(("factor_inv_diag", lambda f: ops.factor_inv_diag(f, ctx=c.h)))
    fns.append(("factor_inv_blocks",
                lambda f: np.concatenate([b.reshape(-1) for b in ops.factor_inv_blocks(f, P.starts, ctx=c.h)])))
    fns.append(("factor_lmul", lambda f: ops.factor_lmul(f, P.Z, ctx=c.h)))
    fns.append(("gp_loglik_grad", lambda f: ops.gp_loglik_grad(P.spec, f, P.X, alpha, ctx=c.h)))
    return fns


def kept_calls(c, fac, P, alpha):
    return [(name, fn(fac)) for name, fn in kept_call_fns(c, P, alpha)]


def oracle_gradient(P):
    def go():
        invLam = np.array([[P.kw["a"], P.kw["b"]], [P.kw["b"], P.kw["c"]]])
        basis = [np.array([[1.0, 0], [0, 0]]), np.array([[0, 1.0], [1.0, 0]]), np.array([[0, 0], [0, 1.0]])]
        g_amp, g_abc = O.loglik_grad_invlam(P.X, P.y, P.e, P.kw["amp"], invLam, basis)
        return np.concatenate([[g_amp], g_abc])
    return P.cached("grad", go)


def check_solve_oracle(P, d, what, alpha=True):
    """alpha to 1e-10 max|ref| and logdet to 1e-11 relative (test_gpu_edge_cases); y . alpha to 1e-10 relative (test_gpu_core)"""
    if alpha:
        close_abs(d["alpha"], P.alpha_ref, 1e-10 * np.abs(P.alpha_ref).max(), what + " alpha")
    np.testing.assert_allclose(d["logdet"], P.logdet_ref, rtol=1e-11, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(d["ydota"], float(P.y @ P.alpha_ref), rtol=1e-10, err_msg=what)


def check_kept_oracle(P, d, what):
    """the kept-factor outputs of a reference: solve / covariance / variance to 1e-10 of their scale (test_gpu_edge_cases),
    diag(K^-1) and its blocks to 1e-9 relative (test_gpu_loo), the gradient to 1e-9 (test_gpu_fit_many)"""
    Kinv = P.Kinv
    ref = P.B @ Kinv
    close_abs(d["factor_solve"], ref, 1e-10 * np.abs(ref).max(), what + " factor_solve")
    for m in QUERIES:
        HT = P.HT(m)
        cref = P.Kss(m) - HT @ Kinv @ HT.T
        close_abs(d["gp_predict_cov[%d]" % m], cref, 1e-10 * P.kw["amp"], what + " cov")
        close_abs(d["gp_predict_var[%d]" % m], np.diag(cref), 1e-10 * P.kw["amp"], what + " var")
    np.testing.assert_allclose(d["factor_inv_diag"], np.diag(Kinv), rtol=1e-9, atol=0, err_msg=what)
    s = P.starts
    bref = np.concatenate([Kinv[s[g]:s[g + 1], s[g]:s[g + 1]].reshape(-1) for g in range(len(s) - 1)])
    close_abs(d["factor_inv_blocks"], bref, 1e-9 * np.abs(np.diag(Kinv)).max(), what + " inv_blocks")
    Lref = np.linalg.cholesky(P.K + np.diag(P.e ** 2))
    yref = P.Z @ Lref.T
    close_abs(d["factor_lmul"], yref, 1e-10 * np.abs(yref).max(), what + " lmul")
    g = oracle_gradient(P)
    np.testing.assert_allclose(d["gp_loglik_grad"], g, rtol=1e-9, atol=1e-9 * np.abs(g).max(), err_msg=what)


# ---- routes ---------------------------------------------------------------------------------------------------------------

class Route(object):
    """run(c, P) -> (exact, sums): lists of (name, array).  ``exact`` is compared bit for bit with a fresh context's, ``sums``
    (fp64-atomic accumulations only) with the oracle.  problems(size) / larger / loud give the route's own inputs."""
    name = "?"
    sizes = ("S", "M", "L")
    dirty_n = None               # size of the generic dirtying problems when the route has no Np of its own

    def clean(self, size):
        return problem(SIZES[size])

    def larger(self, size):
        return problem(LARGER[size], seed=4)

    def loud(self, size, ragged):
        Np = padded(self.np_n(size))
        return problem(Np - 127 if ragged else Np, seed=5, loud=True)

    def np_n(self, size):
        """the n whose Np the generic histories dirty"""
        return self.dirty_n or SIZES[size]

    def check_oracle(self, P, exact, sums):
        raise NotImplementedError

    def check_sums(self, P, sums):
        assert not sums


class SolveRoute(Route):
    def __init__(self, form):
        self.form = form
        self.name = "gp_solve-" + form
        self.sizes = ("S", "M", "L") if form == "keep" else ("S", "M", "L", "XL")

    def run(self, c, P):
        _, ops = _mods()
        alpha, logdet, ydota, fac = ops.gp_solve(P.spec, P.X, P.y, P.e, keep=self.form == "keep",
                                                 want_alpha=self.form != "noalpha", ctx=c.h)
        out = [("logdet", logdet), ("ydota", ydota), ("info", 0)]
        if alpha is not None:
            out.append(("alpha", alpha))
        if fac is not None:
            c.track(fac)
            out += kept_calls(c, fac, P, alpha)
            fac.free(keep_memory=True)
        return out, []

    def check_oracle(self, P, exact, sums):
        d = dict(exact)
        check_solve_oracle(P, d, self.name, alpha=self.form != "noalpha")
        if self.form == "keep":
            check_kept_oracle(P, d, self.name)


class DenseRoute(Route):
    name = "gp_solve_dense"

    def run(self, c, P):
        _, ops = _mods()
        alpha, logdet, ydota, fac = ops.gp_solve_dense(P.K, P.y, P.e, keep=True, ctx=c.h)
        c.track(fac)
        out = [("logdet", logdet), ("ydota", ydota), ("info", 0), ("alpha", alpha)]
        for m in QUERIES:
            out.append(("cov_dense[%d]" % m, ops.gp_predict_cov_dense(fac, P.HT(m), P.Kss(m), ctx=c.h)))
            out.append(("var_dense[%d]" % m, ops.gp_predict_var_dense(fac, P.HT(m), np.diag(P.Kss(m)).copy(), ctx=c.h)))
        fac.free(keep_memory=True)
        return out, []

    def check_oracle(self, P, exact, sums):
        d = dict(exact)
        check_solve_oracle(P, d, self.name)
        for m in QUERIES:
            HT = P.HT(m)
            cref = P.Kss(m) - HT @ P.Kinv @ HT.T
            close_abs(d["cov_dense[%d]" % m], cref, 1e-10 * P.kw["amp"], "cov_dense")
            close_abs(d["var_dense[%d]" % m], np.diag(cref), 1e-10 * P.kw["amp"], "var_dense")


def _vk_pairs(P, m):
    """k(u) and w(u) = 2 pi u^(-1/6) K_{1/6}(2 pi u) / lim0 of the von Karman kernel between the queries and the training points"""
    from scipy import special
    d = P.Xq[:m, None, :] - P.X[None, :, :]
    u = np.sqrt((d ** 2).sum(-1)) / P.vk["ell"]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 2 * np.pi * u ** (-1.0 / 6.0) * special.kv(1.0 / 6.0, 2 * np.pi * u) / O.LIM0
    return d, np.where(u > 0, w, 0.0)


class PredictRoute(Route):
    """tgp_gp_predict / tgp_gp_predict_grad, one Gaussian and one von Karman kernel.  The weights are an input (the oracle's
    alpha), so a stale alpha in the staging arena cannot hide behind a solve of its own."""
    name = "gp_predict"

    def run(self, c, P):
        _, ops = _mods()
        out = []
        for tag, spec in (("gauss", P.spec), ("vk", P.vkspec)):
            for m in PREDICT_M:
                out.append(("predict-%s[%d]" % (tag, m), ops.gp_predict(spec, P.X, P.alpha_in, P.Xq[:m], ctx=c.h)))
                out.append(("grad-%s[%d]" % (tag, m), ops.gp_predict_grad(spec, P.X, P.alpha_in, P.Xq[:m], ctx=c.h)))
        return out, []

    def check_oracle(self, P, exact, sums):
        d = dict(exact)
        a = P.alpha_in
        M = np.array([[P.kw["a"], P.kw["b"]], [P.kw["b"], P.kw["c"]]])
        for m in PREDICT_M:
            HT = P.HT(m)
            ref = HT @ a
            close_abs(d["predict-gauss[%d]" % m], ref, 1e-10 * max(np.abs(ref).max(), 1e-3), "predict gauss")
            dd = P.Xq[:m, None, :] - P.X[None, :, :]
            gref = -np.einsum("ji,jik->jk", HT * a[None, :], dd @ M)
            close_abs(d["grad-gauss[%d]" % m], gref, 1e-10 * np.abs(gref).max(), "grad gauss")
            HV = O.kernel_matrix("vk", P.Xq[:m], P.X, **P.vk)
            ref = HV @ a
            close_abs(d["predict-vk[%d]" % m], ref, 1e-10 * max(np.abs(ref).max(), 1e-3), "predict vk")
            dd, w = _vk_pairs(P, m)
            gref = -P.vk["amp"] / P.vk["ell"] ** 2 * np.einsum("ji,jik->jk", w * a[None, :], dd)
            close_abs(d["grad-vk[%d]" % m], gref, 1e-10 * np.abs(gref).max(), "grad vk")


def _minor(exc):
    return int(str(exc).split("-th")[0])


class ResidentRoute(Route):
    """gp_solve_resident / gp_solve_grad_resident on one ResidentProblem: theta good, rejected, good again; then the same on a
    second ResidentProblem of the same size opened after the first is closed."""
    name = "resident"

    def run(self, c, P):
        _lib, ops = _mods()
        bad = ops.KernelSpec(_lib.TGP_ARBF, amp=P.kw["amp"], a=np.nan, b=0.0, c=1.0)
        out = []
        for r in range(2):
            rp = ops.ResidentProblem(P.X, P.y, P.e, ctx=c.h)
            try:
                for step, spec in enumerate((P.spec, bad, P.spec)):
                    tag = "%d.%d" % (r, step)
                    for fn in (ops.gp_solve_resident, ops.gp_solve_grad_resident):
                        try:
                            res = fn(spec, rp, ctx=c.h)
                            assert spec is not bad, "a NaN theta was accepted"
                            out.append((fn.__name__ + tag, np.concatenate([np.atleast_1d(v) for v in res])))
                        except np.linalg.LinAlgError as exc:
                            assert spec is bad, exc
                            out.append((fn.__name__ + tag + "-info", _minor(exc)))
            finally:
                rp.close()
        return out, []

    def check_oracle(self, P, exact, sums):
        g = oracle_gradient(P)
        chi2 = float(P.y @ P.alpha_ref)
        for k, v in exact:
            if k.endswith("-info"):
                continue
            np.testing.assert_allclose(v[0], P.logdet_ref, rtol=1e-11, atol=1e-12, err_msg=k)
            np.testing.assert_allclose(v[1], chi2, rtol=1e-10, err_msg=k)
            if len(v) > 2:
                np.testing.assert_allclose(v[2:], g, rtol=1e-9, atol=1e-9 * np.abs(g).max(), err_msg=k)


class _Batch(object):
    def __init__(self, ns, ms, seed, loud):
        self.P = [problem(n, seed=seed + b, loud=loud) for b, n in enumerate(ns)]
        self.ms = ms
        self.loud = loud


class BatchRoute(Route):
    """the batched routes on a ragged batch, ns = [130, 257, 64, 200]"""
    name = "batch"
    sizes = ("B",)
    dirty_n = 400                # Np = 512 for the generic histories: above every member, below the batch's workspace

    def clean(self, size):
        return _Batch([130, 257, 64, 200], [1, 130, 300, 257], 20, False)

    def larger(self, size):
        return _Batch([300, 513, 200, 400, 90, 700], [300, 1, 400, 130, 257, 10], 30, True)

    def loud(self, size, ragged):
        return _Batch([257, 200, 130, 64] if ragged else [130, 257, 64, 200], [300, 257, 1, 130], 40, True)

    def run(self, c, Bt, bad=None):
        _, ops = _mods()
        specs = [p.spec for p in Bt.P]
        Xs = [p.X.copy() for p in Bt.P]
        ys, es = [p.y for p in Bt.P], [p.e for p in Bt.P]
        Xq = [p.Xq[:m] for p, m in zip(Bt.P, Bt.ms)]
        if bad is not None:
            Xs[bad][len(Xs[bad]) // 2, 1] = np.nan
        out = []

        def put(tag, lists, arrays):
            for nm, l in lists:
                if l is not None:
                    for b, a in enumerate(l):
                        if b != bad:
                            out.append(("%s.%s[%d]" % (tag, nm, b), a))
            for nm, a in arrays:
                keep = [b for b in range(len(specs)) if b != bad or nm == "info"]
                out.append(("%s.%s" % (tag, nm), np.asarray(a)[keep]))

        al, ld, c2, info = ops.gp_solve_batch(specs, Xs, ys, es, ctx=c.h)
        put("solve", [("alpha", al)], [("logdet", ld), ("chi2", c2), ("info", info)])
        ld, c2, g4, info = ops.gp_solve_grad_batch(specs, Xs, ys, es, ctx=c.h)
        put("grad", [], [("logdet", ld), ("chi2", c2), ("g4", g4), ("info", info)])
        al, dg, ld, c2, info = ops.gp_loo_batch(specs, Xs, ys, es, ctx=c.h)
        put("loo", [("alpha", al), ("invdiag", dg)], [("logdet", ld), ("chi2", c2), ("info", info)])
        for what in ("var", "cov"):
            al, un, ld, c2, info = ops.gp_posterior_batch(specs, Xs, ys, es, Xq, what=what, ctx=c.h)
            put(what, [("alpha", al), ("unc", un)], [("logdet", ld), ("chi2", c2), ("info", info)])
        if bad is not None:
            assert info[bad] > 0, info
        return out, []

    def check_oracle(self, Bt, exact, sums):
        d = dict(exact)
        for b, (P, m) in enumerate(zip(Bt.P, Bt.ms)):
            chi2 = float(P.y @ P.alpha_ref)
            for tag in ("solve", "grad", "loo", "var", "cov"):
                assert d[tag + ".info"][b] == 0
                np.testing.assert_allclose(d[tag + ".logdet"][b], P.logdet_ref, rtol=1e-11, atol=1e-12)
                np.testing.assert_allclose(d[tag + ".chi2"][b], chi2, rtol=1e-10)
                if tag != "grad":
                    close_abs(d["%s.alpha[%d]" % (tag, b)], P.alpha_ref, 1e-10 * np.abs(P.alpha_ref).max(), "batch alpha")
            g = oracle_gradient(P)
            np.testing.assert_allclose(d["grad.g4"][b], g, rtol=1e-9, atol=1e-9 * np.abs(g).max())
            np.testing.assert_allclose(d["loo.invdiag[%d]" % b], np.diag(P.Kinv), rtol=1e-9, atol=0)
            HT = P.HT(m)
            cref = P.Kss(m) - HT @ P.Kinv @ HT.T
            close_abs(d["cov.unc[%d]" % b], cref, 1e-10 * P.kw["amp"], "batch cov")
            close_abs(d["var.unc[%d]" % b], np.diag(cref), 1e-10 * P.kw["amp"], "batch var")


class _Pairs(object):
    def __init__(self, n, nb, weighted, scale=1.0, seed=0):
        rng = np.random.default_rng(7000 + 10 * n + nb + (1 if weighted else 0) + 100000 * seed)
        self.n, self.nb, self.scale = n, nb, scale
        self.x, self.y = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
        self.k = rng.standard_normal(n) * scale
        self.w = rng.uniform(0.5, 2.0, n) * scale if weighted else None
        self.err = rng.uniform(0.05, 0.1, n) / scale if weighted else np.zeros(n)
        self.dx, self.dy = rng.standard_normal(n) * scale, rng.standard_normal(n) * scale
        self.val = (0.5 + rng.standard_normal(n)) * scale
        self.Xq = rng.uniform(0, 1, (300, 2))
        self.idx = O.bootstrap_indices(n, 9)
        self._c = {}

    def cached(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]


PAIR_CASES = [(n, nb, w) for n in (257, 1500) for nb in (7, 21) for w in (False, True)]
_PAIRS = {}


def _pairs(case, scale=1.0, seed=0):
    key = (case, scale, seed)
    if key not in _PAIRS:
        _PAIRS[key] = _Pairs(*case, scale=scale, seed=seed)
    return _PAIRS[key]


def _edges(nb):
    from treegp_amd import utils
    return utils._log_edges(0.01, 0.8, np.log(80.0) / nb)[0]


class PairsRoute(Route):
    """the pair and bin kernels.  Exact: pair counts, bin counts, medians, k-nearest-neighbour means.  Sums: everything that is
    accumulated with fp64 atomics (kk.hip, kk_boot.hip, vcorr.hip, binstat.hip mean), held to the oracle after every history."""
    name = "pairs"
    sizes = ("P",)
    dirty_n = 400

    def clean(self, size):
        return [_pairs(cs) for cs in PAIR_CASES]

    def larger(self, size):
        return [_pairs((3000, 23, True), scale=1e8, seed=1)]

    def loud(self, size, ragged):
        return [_pairs((n + (63 if ragged else 0), nb, w), scale=1e8, seed=2) for n, nb, w in PAIR_CASES]

    def run(self, c, cases):
        _, ops = _mods()
        exact, sums = [], []
        for i, p in enumerate(cases):
            t = "%d:" % i
            xi, wt, npairs = ops.kk_twod(p.x, p.y, p.k, p.w, 0.0, 0.4, p.nb, ctx=c.h)
            exact.append((t + "twod.npairs", npairs))
            sums += [(t + "twod.xi", xi), (t + "twod.weight", wt)]
            xi, wt, mr, mlr, npairs = ops.kk_log(p.x, p.y, p.k, p.w, 0.01, 0.5, p.nb, ctx=c.h)
            exact.append((t + "log.npairs", npairs))
            sums += [(t + "log.xi", xi), (t + "log.weight", wt), (t + "log.meanr", mr), (t + "log.meanlogr", mlr)]
            old = os.environ.get("TGP_BOOT_LISTS")
            try:
                for lists in ("0", "1"):
                    os.environ["TGP_BOOT_LISTS"] = lists
                    sums.append((t + "boot" + lists, ops.kk_twod_bootstrap(p.x, p.y, p.k, p.err, p.idx, 0.0, 0.3, p.nb, ctx=c.h)))
            finally:
                if old is None:
                    del os.environ["TGP_BOOT_LISTS"]
                else:
                    os.environ["TGP_BOOT_LISTS"] = old
            acc = ops.vcorr_sums(p.x, p.y, p.dx, p.dy, _edges(p.nb), ctx=c.h)
            exact.append((t + "vcorr.counts", acc[0]))
            sums.append((t + "vcorr.sums", acc[1:]))
            ue = np.linspace(0.0, 1.0, p.nb + 1)
            avg, _, cnt = ops.binned_stat_2d(p.x, p.y, p.val, ue, ue, "mean", ctx=c.h)
            med, _, cnt2 = ops.binned_stat_2d(p.x, p.y, p.val, ue, ue, "median", ctx=c.h)
            exact += [(t + "bin.count", cnt), (t + "bin.count2", cnt2), (t + "bin.median", med)]
            sums.append((t + "bin.mean", avg))
            for k in (1, 4, 16):
                exact.append((t + "knn%d" % k, ops.knn_mean(np.column_stack([p.x, p.y]), p.val, p.Xq, k, ctx=c.h)))
        return exact, sums

    @staticmethod
    def _oracle(p):
        def go():
            from scipy.stats import binned_statistic_2d
            r = {}
            r["twod"] = O.kk_twod(p.x, p.y, p.k, p.w, 0.0, 0.4, p.nb)
            r["log"] = O.kk_log(p.x, p.y, p.k, p.w, 0.01, 0.5, p.nb)
            X = np.column_stack([p.x, p.y])
            r["boot"] = np.array([O.comp_2pcf(X[ii], p.k[ii], p.err[ii], 0.0, 0.3, p.nb, True)[0] for ii in p.idx])
            r["vcorr"] = O.vcorr(p.x, p.y, p.dx, p.dy, rmin=0.01, rmax=0.8, dlogr=np.log(80.0) / p.nb)
            ue = np.linspace(0.0, 1.0, p.nb + 1)
            for st in ("count", "mean", "median"):
                r[st] = binned_statistic_2d(p.x, p.y, p.val, bins=[ue, ue], statistic=st)[0]
            r["knn"] = {k: O.knn_mean(X, p.val, p.Xq, k) for k in (1, 4, 16)}
            return r
        return p.cached("oracle", go)

    def check_sums(self, cases, sums):
        """test_gpu_soak's tolerance: 1e-11 max(|ref|, 1) (of the scale of the case's values for the scaled quantities)"""
        d = dict(sums)
        for i, p in enumerate(cases):
            t, r = "%d:" % i, self._oracle(p)

            def tol(ref):
                return 1e-11 * max(np.nanmax(np.abs(ref), initial=0.0), 1.0)
            for nm, ref in zip(("xi", "weight"), r["twod"][:2]):
                close_abs(d[t + "twod." + nm], ref, tol(ref), "kk_twod " + nm)
            for nm, ref in zip(("xi", "weight", "meanr", "meanlogr"), r["log"][:4]):
                close_abs(d[t + "log." + nm], ref, tol(ref), "kk_log " + nm)
            for lists in ("0", "1"):
                close_abs(d[t + "boot" + lists], r["boot"], tol(r["boot"]), "bootstrap lists=" + lists)
            acc, (logr, xip, xim, xix, xiz2, counts) = d[t + "vcorr.sums"], r["vcorr"]
            ok = counts > 0
            cn = counts[ok]
            for row, ref in ((acc[0], logr), (acc[1], xip), (acc[2], xiz2.real), (acc[3], xiz2.imag), (acc[4], xim), (acc[5], xix)):
                close_abs(row[ok] / cn, np.asarray(ref)[ok], tol(np.asarray(ref)[ok]), "vcorr")
                assert np.all(row[~ok] == 0.0), "vcorr: an empty bin has a sum"
            close_abs(d[t + "bin.mean"], r["mean"], tol(r["mean"]), "binned mean")

    def check_oracle(self, cases, exact, sums):
        d = dict(exact)
        for i, p in enumerate(cases):
            t, r = "%d:" % i, self._oracle(p)
            assert np.array_equal(d[t + "twod.npairs"], r["twod"][2])
            assert np.array_equal(d[t + "log.npairs"], r["log"][4])
            assert np.array_equal(d[t + "vcorr.counts"], r["vcorr"][5])
            assert np.array_equal(d[t + "bin.count"], r["count"]) and np.array_equal(d[t + "bin.count2"], r["count"])
            np.testing.assert_array_equal(d[t + "bin.median"], r["median"])
            for k in (1, 4, 16):
                np.testing.assert_allclose(d[t + "knn%d" % k], r["knn"][k], rtol=1e-13)
        self.check_sums(cases, sums)


ROUTES = [SolveRoute("alpha"), SolveRoute("noalpha"), SolveRoute("keep"), DenseRoute(), PredictRoute(), ResidentRoute(),
          BatchRoute(), PairsRoute()]
ROUTE_BY_NAME = {r.name: r for r in ROUTES}


# ---- histories ------------------------------------------------------------------------------------------------------------

def _rejected_dense(c, n, j, keep, want_alpha):
    """tgp_d_gp_solve_dense of A = L0 D L0^T with D_jj = -1 (test_gpu_factor.check_first_failing_pivot): the first failing pivot
    is exactly j"""
    _, ops = _mods()
    L0, A0 = _unit_lower(n)
    l = L0[:, j - 1]
    A = A0 - 2.0 * np.outer(l, l)
    try:
        ops.gp_solve_dense(A, np.ones(n), keep=keep, want_alpha=want_alpha, ctx=c.h)
        raise AssertionError("rejected history: an indefinite matrix was accepted (n=%d, pivot %d)" % (n, j))
    except np.linalg.LinAlgError as exc:
        assert _minor(exc) == j, ("rejected history: first failing pivot", n, j, str(exc))


_UNIT_LOWER = {}


def _unit_lower(n):
    """L0 = I + 0.3 / sqrt(n) * strictly lower Gaussian, and L0 L0^T exactly symmetric (test_gpu_factor._unit_lower, on the host),
    made once per size"""
    if n not in _UNIT_LOWER:
        rng = np.random.default_rng(1000 + n)
        L0 = np.tril(rng.standard_normal((n, n)), -1) * (0.3 / np.sqrt(n))
        L0[np.diag_indices(n)] = 1.0
        A0 = L0 @ L0.T
        _UNIT_LOWER[n] = (L0, (A0 + A0.T) * 0.5)
    return _UNIT_LOWER[n]


def failing_positions(n):
    """(middle panel, last panel) pivot positions, as test_first_failing_pivot_in_schedule_steps places them"""
    nP = padded(n) // 256
    mid = 256 * (nP // 2)
    return mid + max(2, min(256, n - mid) // 2), min(256 * (nP - 1) + 5, n)


def _rejected_duplicates(c, n, j, keep, want_alpha):
    """a clean problem whose point j - 1 repeats point j - 2 with no noise on either: pivot j is zero up to rounding, of either
    sign, so the solve is rejected there, or later, or (all roundings positive) not at all -- whichever it is, it is a legal
    call.  The rejection at exactly j is _rejected_dense's."""
    _, ops = _mods()
    P = problem(n, seed=6)
    X, e = P.X.copy(), P.e.copy()
    X[j - 1] = X[j - 2]
    e[j - 1] = e[j - 2] = 0.0
    try:
        fac = ops.gp_solve(P.spec, X, P.y, e, keep=keep, want_alpha=want_alpha, ctx=c.h)[3]
        if fac is not None:
            c.track(fac).free(keep_memory=True)
    except np.linalg.LinAlgError:
        pass


def h_again(c, R, size):
    R.run(c, R.clean(size))


def h_larger(c, R, size):
    R.run(c, R.larger(size))


def _loud(c, R, size, ragged):
    _, ops = _mods()
    R.run(c, R.loud(size, ragged))
    # and a loud factor left in the cache of this Np, its slabs with the context
    P = problem((padded(R.np_n(size)) - 127) if ragged else padded(R.np_n(size)), seed=5, loud=True)
    c.track(ops.gp_solve(P.spec, P.X, P.y, P.e, keep=True, ctx=c.h)[3]).free(keep_memory=True)


def h_loud_full(c, R, size):
    _loud(c, R, size, False)


def h_loud_ragged(c, R, size):
    _loud(c, R, size, True)


def _rejected(c, R, size, which):
    if isinstance(R, BatchRoute):
        Bt = R.clean(size)
        R.run(c, Bt, bad=(1, len(Bt.P) - 1)[which])
        return
    n = R.np_n(size)
    j = failing_positions(n)[which]
    forms = [((False, True), (True, False)), ((False, False), (True, True))][which]
    for keep, want_alpha in forms:
        _rejected_duplicates(c, n, j, keep, want_alpha)
        _rejected_dense(c, n, j, keep, want_alpha)


def h_rejected_mid(c, R, size):
    _rejected(c, R, size, 0)


def h_rejected_last(c, R, size):
    _rejected(c, R, size, 1)


def rejected_nan(c, n):
    """solves with a NaN coordinate (test_nan_coordinate_or_parameter_is_not_positive_definite), the last one with NaN in every
    coordinate of the second half: staged at the front of the arena, they then cover doubles n .. 2n - 1 of it -- where the
    padding of the first row of a (nrhs, Np) block of tgp_factor_solve / tgp_factor_lmul lies"""
    _, ops = _mods()
    P = problem(n, seed=7)
    Xn = P.X.copy()
    Xn[n // 2, 1] = np.nan
    Xt = P.X.copy()
    Xt[n // 2:] = np.nan
    for X, keep, want_alpha in ((Xn, False, True), (Xn, True, True), (Xn, False, False), (Xt, False, True)):
        try:
            ops.gp_solve(P.spec, X, P.y, P.e, keep=keep, want_alpha=want_alpha, ctx=c.h)
            raise AssertionError("a NaN coordinate was accepted")
        except np.linalg.LinAlgError:
            pass


def h_rejected_nan(c, R, size):
    rejected_nan(c, R.np_n(size))


def h_other_routes(c, R, size):
    """other routes with loud values on the same context: they share scratch, scratch2 and the staging arena"""
    _, ops = _mods()
    P = problem(R.np_n(size), seed=8, loud=True)
    alpha, _, _, fac = ops.gp_solve(P.spec, P.X, P.y, P.e, keep=True, ctx=c.h)
    c.track(fac)
    ops.gp_predict_cov(P.spec, fac, P.X, P.Xq[:300], ctx=c.h)
    ops.gp_predict_var(P.spec, fac, P.X, P.Xq[:700], ctx=c.h)
    ops.factor_inv_diag(fac, ctx=c.h)
    ops.factor_lmul(fac, P.Z, ctx=c.h)
    fac.free(keep_memory=True)
    Bt = _Batch([300, 90, 513], [1, 1, 1], 50, True)
    ops.gp_solve_batch([p.spec for p in Bt.P], [p.X for p in Bt.P], [p.y for p in Bt.P], [p.e for p in Bt.P], ctx=c.h)
    p = _pairs((700, 13, True), scale=1e8, seed=3)
    ops.kk_twod(p.x, p.y, p.k, p.w, 0.0, 0.4, p.nb, ctx=c.h)
    ops.knn_mean(np.column_stack([p.x, p.y]), p.val, p.Xq, 4, ctx=c.h)
    ue = np.linspace(0.0, 1.0, p.nb + 1)
    ops.binned_stat_2d(p.x, p.y, p.val, ue, ue, "mean", ctx=c.h)


def h_released(c, R, size):
    _lib, _ = _mods()
    _lib.check(c.h, c.lib.tgp_release_caches(c.h), "tgp_release_caches")


def h_loud_released(c, R, size):
    _loud(c, R, size, True)
    h_released(c, R, size)


def kept_traffic(c, n):
    """keep A; solve B with keep; A back to the cache; solve C without keep (augmented where the size has big-step sweeps: row
    Np - 1 of the cached matrix carries y); B back to the cache"""
    _, ops = _mods()
    A, B, Cc = problem(n, seed=9, loud=True), problem(n, seed=10), problem(n, seed=11, loud=True)
    fa = c.track(ops.gp_solve(A.spec, A.X, A.y, A.e, keep=True, ctx=c.h)[3])
    fb = c.track(ops.gp_solve(B.spec, B.X, B.y, B.e, keep=True, ctx=c.h)[3])
    ops.factor_solve(fb, B.B, ctx=c.h)                        # B's slabs exist
    fa.free(keep_memory=True)
    ops.gp_solve(Cc.spec, Cc.X, Cc.y, Cc.e, ctx=c.h)
    ops.gp_solve(Cc.spec, Cc.X, Cc.y, Cc.e, want_alpha=False, ctx=c.h)
    fb.free(keep_memory=True)


def h_kept_traffic(c, R, size):
    kept_traffic(c, R.np_n(size))


HISTORIES = [("again", h_again), ("larger", h_larger), ("loud-n=Np", h_loud_full), ("loud-n=Np-127", h_loud_ragged),
             ("rejected-mid-panel", h_rejected_mid), ("rejected-last-panel", h_rejected_last), ("rejected-nan", h_rejected_nan),
             ("other-routes", h_other_routes), ("released", h_released), ("loud-then-released", h_loud_released),
             ("kept-traffic", h_kept_traffic)]


# ---- references -----------------------------------------------------------------------------------------------------------

_REFS = {}


def reference(R, size):
    """R(P) as the first call on a new context, held to the oracle once; shared by every test and left unchanged"""
    key = (R.name, size)
    if key not in _REFS:
        P = R.clean(size)
        with Ctx() as c:
            exact, sums = R.run(c, P)
        R.check_oracle(P, exact, sums)
        _REFS[key] = exact
    return _REFS[key]

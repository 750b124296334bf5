"""Where the entries read and write: guard bands around every pointer argument (tests/_guard_helpers.py).

No tolerance anywhere: a case runs its entry on plain exact-size buffers (twice: the route must reproduce its own bits), then
once per fill pattern with every pointer argument in the middle of a larger allocation whose guards hold a quiet NaN or a
finite sentinel.  Asserted: both guards of every argument untouched; every `const` input unchanged in bits; outputs and scalar
results (logdet, ydota, grad, info, the return code) bit-identical across the runs -- a kernel that stored past an extent, wrote
into an input, left an output element unwritten, or let what lies behind an input into its result fails one of them.

  1. device-pointer entries, whose kernels store straight into caller memory: torch device tensors, `data_ptr()`, the library
     loaded before torch as in tests/test_gpu_factor.py.  n in {1, 129, 255, 256, 257, 300} (Np = 256, 512), Np = 768 for the
     factorisation and the sweeps, m in {1, 255, 257, 300}, nrhs in {1, 4, 5}.  tgp_d_gp_predict runs in fresh processes with
     TGP_PREDICT_GENERIC set and unset (read once per process).
  2. a kept factor and a borrowed one are read-only to every consumer (include/tgp.h: kept factors "must stay clean",
     tgp_factor_device "changes nothing"): the packed panels and W through tgp_factor_device, bits compared after every call, at
     n = 300 and n = 2304 (inverse slabs), with the default substitution and TGP_COV_BIG=0.
  3. host-boundary entries through raw ctypes: banded NumPy buffers, results also against the ops wrapper's bits -- a copy-out of
     the wrong length or stride (nmax-strided batches, kn-strided neighbour lists, the (nrhs, n) / (nrhs, Np) 2-D copies).

Nothing here plants a violation (tests/test_guard_helpers_host.py does, on the host), and nothing passes a pointer, size or
alignment that include/tgp.h does not allow."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                        # run as a script (the fresh-process cases): no conftest has done it
    sys.path.insert(0, ROOT)

import _guard_helpers as G  # noqa: E402
import _local_refs as LR  # noqa: E402
from _guard_helpers import Arg  # noqa: E402

pytestmark = pytest.mark.gpu

NS = [1, 129, 255, 256, 257, 300]               # Np = 256 and 512; one point, tile edges, ragged
MS = [1, 255, 257, 300]                         # around the 256-query workgroup of predict.hip
NM = [(1, 300), (129, 1), (255, 257), (256, 255), (257, 300), (300, 257), (300, 1), (1, 255)]      # every n, every m
KINDS = ["rbf", "arbf", "vk", "avk"]
TB = 128


class _Env(object):
    pass


_ENV = None


def _env():
    global _ENV
    if _ENV is None:
        from treegp_amd import _lib, ops
        lib = _lib.load_library()          # (before torch: the library and torch share one HIP runtime)
        import torch
        e = _Env()
        e.lib, e._lib, e.ops, e.torch = lib, _lib, ops, torch
        e.ctx = _lib.get_ctx()
        e.dev = torch.device("cuda", 0)
        e.X, e.y, e.yerr, e.Xs = LR.uniform_data(2304, 300, seed=23)
        rng = np.random.default_rng(29)
        e.X3 = rng.uniform(size=(300, 3))
        _ENV = e
    return _ENV


@pytest.fixture(scope="module")
def env():
    return _env()


def vp(buf):
    p = G.ptr_of(buf)
    return None if p is None else C.c_void_p(p)


def spec_of(e, name):
    if name == "sum":
        return e.ops.KernelSumSpec([LR.make_spec("rbf", amp=0.4), LR.make_spec("avk", amp=0.24)])
    if name == "3d":
        return e.ops.KernelSpec3(e._lib.TGP_ARBF, amp=LR.AMP, m=(40.0, -5.0, 3.0, 30.0, 2.0, 25.0))
    return LR.make_spec(name)


def guarded(e, entry, args, call, compare=None):
    return G.run_guarded(entry, args, call, e.dev, before_call=e.torch.cuda.synchronize, compare=compare)


def checked(e, rc, what):
    e._lib.check(e.ctx, rc, what)
    return rc


# ---- 1. device-pointer entries -------------------------------------------------------------------------------------------------

def kbuild_args_call(e, name, n, with_yerr):
    spec = spec_of(e, name)
    entry = {"sum": "tgp_d_kbuild_lower_sum", "3d": "tgp_d_kbuild_lower3"}.get(name, "tgp_d_kbuild_lower")
    fn, kc = getattr(e.lib, entry), spec.to_c()
    Np = int(e.lib.tgp_padded_n(n))
    # d_A goes in holding 7.0: the build never writes the tile above the diagonal of a panel's first 128 rows
    args = [Arg("d_X", "in", e.X3[:n] if name == "3d" else e.X[:n]),
            Arg("d_yerr", "in", e.yerr[:n] if with_yerr else None),
            Arg("d_A", "inout", np.full(int(e.lib.tgp_panel_elems(Np)), 7.0))]

    def call(b):
        return {"rc": checked(e, fn(e.ctx, C.byref(kc), vp(b["d_X"]), n, vp(b["d_yerr"]), vp(b["d_A"])), entry)}
    return entry, args, call, Np


@pytest.mark.parametrize("name", KINDS + ["sum", "3d"])
def test_kbuild_lower(env, name):
    """tgp_d_kbuild_lower / _sum / 3: d_X (n, 2) or (n, 3), d_yerr (n) or NULL, d_A (tgp_panel_elems(Np)) banded"""
    e = env
    for n in NS:
        for with_yerr in ((True, False) if n in (129, 257) else (True,)):
            entry, args, call, Np = kbuild_args_call(e, name, n, with_yerr)
            outs, _ = guarded(e, "%s n=%d%s" % (entry, n, "" if with_yerr else " yerr=NULL"), args, call)
            A = outs["d_A"]
            assert A[0] >= spec_of(e, name).amp and (A[-1] == 1.0 or n == Np)      # element (0, 0); identity padding at (Np-1, Np-1)


def packed_matrix(e, n):
    """the packed K + diag(yerr^2) of order n, identity-padded to Np, as the device builds it (the tiles the build leaves alone
    hold 0)"""
    entry, args, call, Np = kbuild_args_call(e, "arbf", n, True)
    t = e.torch
    dX, de = t.from_numpy(e.X[:n].copy()).to(e.dev), t.from_numpy(e.yerr[:n].copy()).to(e.dev)
    dA = t.zeros(int(e.lib.tgp_panel_elems(Np)), dtype=t.float64, device=e.dev)
    t.cuda.synchronize()
    call({"d_X": dX, "d_yerr": de, "d_A": dA})
    return dA.cpu().numpy(), Np


_FACTORS = {}


def factored(e, n):
    """(packed L, W, Np) of packed_matrix(n) from a guarded tgp_d_potrf: the case of test_potrf, its plain outputs kept"""
    if n not in _FACTORS:
        A, Np = packed_matrix(e, n)
        args = [Arg("d_A", "inout", A), Arg("d_W", "out", shape=(Np * TB,))]

        def call(b):
            return {"info": checked(e, e.lib.tgp_d_potrf(e.ctx, vp(b["d_A"]), Np, vp(b["d_W"])), "tgp_d_potrf")}
        outs, scal = guarded(e, "tgp_d_potrf Np=%d (n=%d)" % (Np, n), args, call)
        assert scal["info"] == 0
        _FACTORS[n] = (outs["d_A"], outs["d_W"], Np)
    return _FACTORS[n]


POTRF_N = [211, 512, 700]                      # Np = 256, 512, 768; identity padding of 45, 0 and 68 rows


@pytest.mark.parametrize("n", POTRF_N)
def test_potrf(env, n):
    """tgp_d_potrf: d_A in place, d_W (Np x 128) banded"""
    L, W, Np = factored(env, n)
    assert np.isfinite(W).all() and np.isfinite(L[:256]).all()


@pytest.mark.parametrize("n", POTRF_N)
def test_potrs(env, n):
    """tgp_d_potrs: d_A, d_W const, d_b (Np) in place; tgp_d_potrs_multi: d_B (nrhs, Np) for nrhs = 1, 4, 5"""
    e = env
    L, W, Np = factored(e, n)
    rng = np.random.default_rng(n)
    for nrhs in (0, 1, 4, 5):                    # 0: the single right-hand-side entry
        B = np.zeros((max(nrhs, 1), Np))
        B[:, :n] = rng.standard_normal((max(nrhs, 1), n))
        args = [Arg("d_A", "in", L), Arg("d_W", "in", W), Arg("d_b", "inout", B[0] if nrhs == 0 else B)]
        if nrhs == 0:
            def call(b):
                return {"rc": checked(e, e.lib.tgp_d_potrs(e.ctx, vp(b["d_A"]), vp(b["d_W"]), Np, vp(b["d_b"])), "tgp_d_potrs")}
        else:
            def call(b, nrhs=nrhs):
                return {"rc": checked(e, e.lib.tgp_d_potrs_multi(e.ctx, vp(b["d_A"]), vp(b["d_W"]), Np, vp(b["d_b"]), nrhs),
                                      "tgp_d_potrs_multi")}
        outs, _ = guarded(e, "%s Np=%d nrhs=%d" % ("tgp_d_potrs" if nrhs == 0 else "tgp_d_potrs_multi", Np, nrhs), args, call)
        x = outs["d_b"].reshape(max(nrhs, 1), Np)
        assert np.isfinite(x).all() and (x[:, n:] == 0.0).all()


@pytest.mark.parametrize("n", NS)
def test_unpack_lower(env, n):
    """tgp_d_unpack_lower: d_A const on the device, out a host (n, n) buffer"""
    e = env
    A, Np = packed_matrix(e, n)
    args = [Arg("d_A", "in", A), Arg("out", "out", shape=(n, n), where="numpy")]

    def call(b):
        return {"rc": checked(e, e.lib.tgp_d_unpack_lower(e.ctx, vp(b["d_A"]), Np, n, vp(b["out"])), "tgp_d_unpack_lower")}
    outs, _ = guarded(e, "tgp_d_unpack_lower n=%d" % n, args, call)
    K = outs["out"]
    assert (np.triu(K, 1) == 0.0).all() and (np.diag(K) >= LR.AMP).all()


def solve_forms(n):
    """(keep, alpha wanted): both sweeps, the kept factor's clean route, the likelihood-only route (y as a matrix row for n < Np)"""
    return [(False, True), (True, True), (False, False)] + ([(True, False)] if n in (257, 300) else [])


def solve_call(e, fn, entry, head, n, keep):
    def call(b):
        logdet, ydota, h = C.c_double(0.0), C.c_double(0.0), C.c_void_p()
        rc = checked(e, fn(e.ctx, *(head(b) + [n, vp(b["d_y"]), vp(b["d_yerr"]), vp(b["d_alpha"]), C.byref(logdet), C.byref(ydota),
                                               C.byref(h) if keep else None])), entry)
        if keep and rc == 0:
            e.lib.tgp_factor_free(e.ctx, h)
        return {"rc": rc, "logdet": logdet.value, "ydota": ydota.value}
    return call


@pytest.mark.parametrize("name", KINDS)
def test_gp_solve(env, name):
    """tgp_d_gp_solve: d_X (n, 2), d_y, d_yerr (n) const, d_alpha (n) or NULL, with and without `keep`"""
    e = env
    kc = spec_of(e, name).to_c()
    for n in NS:
        for keep, want_alpha in solve_forms(n):
            args = [Arg("d_X", "in", e.X[:n]), Arg("d_y", "in", e.y[:n]), Arg("d_yerr", "in", e.yerr[:n] if n != 129 else None),
                    Arg("d_alpha", "out", shape=(n,) if want_alpha else None)]
            call = solve_call(e, e.lib.tgp_d_gp_solve, "tgp_d_gp_solve", lambda b: [C.byref(kc), vp(b["d_X"])], n, keep)
            outs, scal = guarded(e, "tgp_d_gp_solve %s n=%d keep=%d alpha=%d" % (name, n, keep, want_alpha), args, call)
            assert scal["rc"] == 0 and np.isfinite([scal["logdet"], scal["ydota"]]).all()
            assert not want_alpha or np.isfinite(outs["d_alpha"]).all()


def test_gp_solve_dense(env):
    """tgp_d_gp_solve_dense: d_K (n, n) const, the rest as tgp_d_gp_solve"""
    e = env
    spec = spec_of(e, "arbf")
    for n in NS:
        K = e.ops.kernel_matrix(spec, e.X[:n])
        for keep, want_alpha in solve_forms(n):
            args = [Arg("d_K", "in", K), Arg("d_y", "in", e.y[:n]), Arg("d_yerr", "in", e.yerr[:n] if n != 255 else None),
                    Arg("d_alpha", "out", shape=(n,) if want_alpha else None)]
            if n == 255:
                args[0] = Arg("d_K", "in", K + np.diag(e.yerr[:n] ** 2))
            call = solve_call(e, e.lib.tgp_d_gp_solve_dense, "tgp_d_gp_solve_dense", lambda b: [vp(b["d_K"])], n, keep)
            outs, scal = guarded(e, "tgp_d_gp_solve_dense n=%d keep=%d alpha=%d" % (n, keep, want_alpha), args, call)
            assert scal["rc"] == 0 and np.isfinite([scal["logdet"], scal["ydota"]]).all()


def predict_cases(e, entries=("tgp_d_gp_predict", "tgp_d_gp_predict_grad")):
    """tgp_d_gp_predict: d_X, d_alpha, d_Xs const, d_ys (m); tgp_d_gp_predict_grad: d_gs (m, 2).  Every kind, every n, every m."""
    rng = np.random.default_rng(31)
    alpha = rng.standard_normal(300)
    done = 0
    for name in KINDS:
        kc = spec_of(e, name).to_c()
        for entry in entries:
            fn, width = getattr(e.lib, entry), (1 if entry == "tgp_d_gp_predict" else 2)
            for n, m in NM:
                args = [Arg("d_X", "in", e.X[:n]), Arg("d_alpha", "in", alpha[:n]), Arg("d_Xs", "in", e.Xs[:m]),
                        Arg("d_out", "out", shape=(m,) if width == 1 else (m, 2))]

                def call(b):
                    return {"rc": checked(e, fn(e.ctx, C.byref(kc), vp(b["d_X"]), n, vp(b["d_alpha"]), vp(b["d_Xs"]), m,
                                                vp(b["d_out"])), entry)}
                outs, _ = guarded(e, "%s %s n=%d m=%d" % (entry, name, n, m), args, call)
                assert np.isfinite(outs["d_out"]).all()
                done += 1
    return done


def test_predict_grad(env):
    assert predict_cases(env, entries=("tgp_d_gp_predict_grad",)) == len(KINDS) * len(NM)


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "TGP_PREDICT_GENERIC=1"])
def test_predict_in_a_fresh_process(generic):
    """TGP_PREDICT_GENERIC is read once per process: a child per setting runs predict_cases (the mean and, while it is up, the
    gradient) on the route the setting selects"""
    child_env = {k: v for k, v in os.environ.items() if k != "TGP_PREDICT_GENERIC"}
    if generic:
        child_env["TGP_PREDICT_GENERIC"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "predict"], env=child_env, capture_output=True, text=True,
                       timeout=300)
    want = "GUARD OK generic=%d cases=%d" % (generic, 2 * len(KINDS) * len(NM))
    assert r.returncode == 0 and want in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


@pytest.mark.parametrize("entry,names", [("tgp_d_gp_solve_grad", ["rbf", "arbf"]), ("tgp_d_gp_solve_grad_any", KINDS)])
def test_gp_solve_grad(env, entry, names):
    """tgp_d_gp_solve_grad / _any: d_X, d_y, d_yerr const on the device; grad (4) a banded host buffer; logdet, ydota scalars"""
    e = env
    fn = getattr(e.lib, entry)
    for name in names:
        kc = spec_of(e, name).to_c()
        for n in NS:
            args = [Arg("d_X", "in", e.X[:n]), Arg("d_y", "in", e.y[:n]), Arg("d_yerr", "in", e.yerr[:n] if n != 256 else None),
                    Arg("grad", "out", shape=(4,), where="numpy")]

            def call(b):
                logdet, ydota = C.c_double(0.0), C.c_double(0.0)
                rc = checked(e, fn(e.ctx, C.byref(kc), vp(b["d_X"]), n, vp(b["d_y"]), vp(b["d_yerr"]), C.byref(logdet),
                                   C.byref(ydota), vp(b["grad"])), entry)
                return {"rc": rc, "logdet": logdet.value, "ydota": ydota.value}
            outs, scal = guarded(e, "%s %s n=%d" % (entry, name, n), args, call)
            assert scal["rc"] == 0 and np.isfinite(outs["grad"]).all()


# ---- 2. a factor is read-only to its consumers -----------------------------------------------------------------------------------

class _DeviceArray(object):
    """library-owned device memory as a torch tensor without a copy"""

    def __init__(self, ptr, numel):
        self.__cuda_array_interface__ = {"shape": (int(numel),), "typestr": "<f8", "data": (int(ptr), False), "strides": None,
                                         "version": 2}


def factor_views(e, h):
    """live views of a factor's packed panels and W through tgp_factor_device, and Np"""
    dA, dW, Np = C.c_void_p(), C.c_void_p(), C.c_int64()
    checked(e, e.lib.tgp_factor_device(e.ctx, h, C.byref(dA), C.byref(dW), C.byref(Np)), "tgp_factor_device")
    P = e.torch.as_tensor(_DeviceArray(dA.value, e.lib.tgp_panel_elems(Np.value)), device=e.dev)
    W = e.torch.as_tensor(_DeviceArray(dW.value, Np.value * TB), device=e.dev)
    return P, W, Np.value, dA.value, dW.value


def consumers(e, spec, fac, n, alpha):
    """(name, thunk) of every entry that takes a tgp_factor, each called once through its wrapper"""
    ops = e.ops
    X, Xq = e.X[:n], e.Xs[:261]
    rng = np.random.default_rng(n)
    B = rng.standard_normal((5, n))
    HT = ops.kernel_matrix(spec, Xq, X)
    Kss = ops.kernel_matrix(spec, Xq)
    starts = np.array([0, 1, 130, 257, n] if n == 300 else [0, 7, 300, 1100, 1101, 2048, n], dtype=np.int64)
    return [
        ("tgp_factor_solve", lambda: ops.factor_solve(fac, B)),
        ("tgp_factor_lmul", lambda: ops.factor_lmul(fac, B)),
        ("tgp_factor_inv_diag", lambda: ops.factor_inv_diag(fac)),
        ("tgp_factor_inv_blocks", lambda: ops.factor_inv_blocks(fac, starts)),
        ("tgp_gp_predict_var", lambda: ops.gp_predict_var(spec, fac, X, Xq)),
        ("tgp_gp_predict_var_dense", lambda: ops.gp_predict_var_dense(fac, HT, np.diag(Kss).copy())),
        ("tgp_gp_predict_cov", lambda: ops.gp_predict_cov(spec, fac, X, Xq)),
        ("tgp_gp_predict_cov_dense", lambda: ops.gp_predict_cov_dense(fac, HT, Kss)),
        ("tgp_gp_loglik_grad", lambda: ops.gp_loglik_grad(spec, fac, X, alpha)),
        ("tgp_gp_loglik_grad_any", lambda: ops.gp_loglik_grad_any(spec, fac, X, alpha)),
        ("tgp_gp_fisher", lambda: ops.gp_fisher(spec, fac, X)),
    ]


def _cov_big(monkeypatch, subst):
    monkeypatch.delenv("TGP_COV_BIG", raising=False)
    if subst == "128-blocks":
        monkeypatch.setenv("TGP_COV_BIG", "0")


@pytest.mark.parametrize("subst", ["default", "128-blocks"])
@pytest.mark.parametrize("n", [300, 2304])
def test_kept_factor_is_read_only(env, monkeypatch, n, subst):
    """n = 2304: the first size whose default sweeps go through the inverse slabs (tests/test_gpu_cond_ladder.py)"""
    e = env
    _cov_big(monkeypatch, subst)
    spec = spec_of(e, "arbf")
    alpha, _, _, fac = e.ops.gp_solve(spec, e.X[:n], e.y[:n], e.yerr[:n], keep=True)
    try:
        P, W, Np, pA, pW = factor_views(e, fac._h)
        sP, sW = G.snapshot(P), G.snapshot(W)
        for name, thunk in consumers(e, spec, fac, n, alpha):
            res = thunk()
            assert np.isfinite(np.concatenate([np.ravel(r) for r in res]) if isinstance(res, list) else res).all(), name
            P2, W2, Np2, pA2, pW2 = factor_views(e, fac._h)
            assert (Np2, pA2, pW2) == (Np, pA, pW), name
            G.assert_same_bits(P, sP, "kept factor, n=%d, %s: packed panels after %s" % (n, subst, name))
            G.assert_same_bits(W, sW, "kept factor, n=%d, %s: W after %s" % (n, subst, name))
    finally:
        fac.free()


@pytest.mark.parametrize("subst", ["default", "128-blocks"])
@pytest.mark.parametrize("n", [300, 2304])
def test_borrowed_factor_is_read_only_and_its_guards_hold(env, monkeypatch, n, subst):
    """tgp_factor_borrow on banded d_A (tgp_panel_elems(Np)) and d_W (Np x 128): the caller's memory, both fills"""
    e = env
    _cov_big(monkeypatch, subst)
    spec = spec_of(e, "arbf")
    alpha, _, _, kept = e.ops.gp_solve(spec, e.X[:n], e.y[:n], e.yerr[:n], keep=True)
    try:
        P, W, Np = factor_views(e, kept._h)[:3]
        results = {}
        for fill in G.FILLS:
            dA, hA = G.banded(P.numel(), np.float64, fill, e.dev, name="borrowed d_A [guards = %s]" % fill)
            dW, hW = G.banded(W.numel(), np.float64, fill, e.dev, name="borrowed d_W [guards = %s]" % fill)
            dA.copy_(P)
            dW.copy_(W)
            sP, sW = G.snapshot(dA), G.snapshot(dW)
            e.torch.cuda.synchronize()
            h = C.c_void_p()
            checked(e, e.lib.tgp_factor_borrow(e.ctx, vp(dA), vp(dW), n, C.byref(h)), "tgp_factor_borrow")
            fac = e.ops.Factor(e.ctx, h, n, keepalive=(dA, dW))
            try:
                P2, W2, Np2, pA2, pW2 = factor_views(e, h)
                assert (Np2, pA2, pW2) == (Np, G.ptr_of(dA), G.ptr_of(dW))
                for name, thunk in consumers(e, spec, fac, n, alpha):
                    res = thunk()
                    what = "borrowed factor, n=%d, %s, guards = %s, after %s" % (n, subst, fill, name)
                    hA.name, hW.name = what + ": d_A", what + ": d_W"
                    hA.assert_untouched()
                    hW.assert_untouched()
                    G.assert_same_bits(dA, sP, what + ": packed panels")
                    G.assert_same_bits(dW, sW, what + ": W")
                    # the same factor bits in other memory, other surroundings: the same result bits
                    flat = np.concatenate([np.ravel(r) for r in res]) if isinstance(res, list) else np.asarray(res)
                    if name in results:
                        G.assert_same_bits(flat, results[name], what + ": the result against the other fill's")
                    results[name] = G.snapshot(flat)
            finally:
                fac.free()
    finally:
        kept.free()


# ---- 3. host-boundary entries through raw ctypes ------------------------------------------------------------------------------

def host(e, entry, args, call):
    return G.run_guarded(entry, args, call, "numpy")


def same_as_wrapper(raw, wrapped, what):
    G.assert_same_bits(np.ascontiguousarray(raw), G.snapshot(np.ascontiguousarray(wrapped)), what + ": raw call against the ops wrapper")


@pytest.mark.parametrize("name", KINDS)
def test_host_kernel_matrix_predict_and_solve(env, name):
    """tgp_kernel_matrix with m != n; tgp_gp_solve; tgp_gp_predict; tgp_gp_predict_grad"""
    e = env
    lib, ctx, ops = e.lib, e.ctx, e.ops
    spec = spec_of(e, name)
    kc = spec.to_c()
    n, m = 300, 37
    X, y, yerr, Xq = e.X[:n], e.y[:n], e.yerr[:n], e.Xs[:m]
    for nn, mm in ((n, m), (m, n), (257, 1)):
        args = [Arg("X", "in", X[:nn]), Arg("Y", "in", e.Xs[:mm]), Arg("out", "out", shape=(nn, mm))]
        outs, _ = host(e, "tgp_kernel_matrix %s (%d, %d)" % (name, nn, mm), args, lambda b: {"rc": checked(e, lib.tgp_kernel_matrix(
            ctx, C.byref(kc), vp(b["X"]), nn, vp(b["Y"]), mm, vp(b["out"])), "tgp_kernel_matrix")})
        same_as_wrapper(outs["out"], ops.kernel_matrix(spec, X[:nn], e.Xs[:mm]), "tgp_kernel_matrix")

    def solve(b):
        logdet, ydota = C.c_double(0.0), C.c_double(0.0)
        rc = checked(e, lib.tgp_gp_solve(ctx, C.byref(kc), vp(b["X"]), n, vp(b["y"]), vp(b["yerr"]), vp(b["alpha"]), C.byref(logdet),
                                         C.byref(ydota), None), "tgp_gp_solve")
        return {"rc": rc, "logdet": logdet.value, "ydota": ydota.value}
    args = [Arg("X", "in", X), Arg("y", "in", y), Arg("yerr", "in", yerr), Arg("alpha", "out", shape=(n,))]
    outs, scal = host(e, "tgp_gp_solve %s" % name, args, solve)
    alpha, logdet, ydota, _ = ops.gp_solve(spec, X, y, yerr)
    same_as_wrapper(outs["alpha"], alpha, "tgp_gp_solve alpha")
    same_as_wrapper([scal["logdet"], scal["ydota"]], [logdet, ydota], "tgp_gp_solve logdet, ydota")

    for entry, wrapper, width in (("tgp_gp_predict", ops.gp_predict, 1), ("tgp_gp_predict_grad", ops.gp_predict_grad, 2)):
        for mm in (m, 257):
            args = [Arg("X", "in", X), Arg("alpha", "in", alpha), Arg("Xs", "in", e.Xs[:mm]),
                    Arg("out", "out", shape=(mm,) if width == 1 else (mm, 2))]
            outs, _ = host(e, "%s %s m=%d" % (entry, name, mm), args, lambda b: {"rc": checked(e, getattr(lib, entry)(
                ctx, C.byref(kc), vp(b["X"]), n, vp(b["alpha"]), vp(b["Xs"]), mm, vp(b["out"])), entry)})
            same_as_wrapper(outs["out"], wrapper(spec, X, alpha, e.Xs[:mm]), entry)


def test_host_posterior_and_factor_solve(env):
    """tgp_gp_predict_var (m), tgp_gp_predict_cov (m, m), tgp_factor_solve (nrhs, n) against (nrhs, Np) on the device"""
    e = env
    lib, ctx, ops = e.lib, e.ctx, e.ops
    spec = spec_of(e, "arbf")
    kc = spec.to_c()
    n = 300
    X, y, yerr = e.X[:n], e.y[:n], e.yerr[:n]
    _, _, _, fac = ops.gp_solve(spec, X, y, yerr, keep=True)
    try:
        for m in (37, 257):
            Xq = e.Xs[:m]
            for entry, wrapper, shape in (("tgp_gp_predict_var", ops.gp_predict_var, (m,)), ("tgp_gp_predict_cov", ops.gp_predict_cov, (m, m))):
                args = [Arg("X", "in", X), Arg("Xs", "in", Xq), Arg("out", "out", shape=shape)]
                outs, _ = host(e, "%s m=%d" % (entry, m), args, lambda b: {"rc": checked(e, getattr(lib, entry)(
                    ctx, fac._h, C.byref(kc), vp(b["X"]), n, vp(b["Xs"]), m, vp(b["out"])), entry)})
                same_as_wrapper(outs["out"], wrapper(spec, fac, X, Xq), entry)
        rng = np.random.default_rng(41)
        for nrhs in (1, 4, 5):
            B = rng.standard_normal((nrhs, n))
            args = [Arg("B", "in", B), Arg("Xout", "out", shape=(nrhs, n))]
            outs, _ = host(e, "tgp_factor_solve nrhs=%d" % nrhs, args, lambda b: {"rc": checked(e, lib.tgp_factor_solve(
                ctx, fac._h, vp(b["B"]), nrhs, vp(b["Xout"])), "tgp_factor_solve")})
            same_as_wrapper(outs["Xout"], ops.factor_solve(fac, B), "tgp_factor_solve")
    finally:
        fac.free()


NB, BATCH_NS, NMAX = 3, (1, 100, 257), 300           # nmax > max ns: whole rows of padding behind the longest problem
BATCH_MS, MMAX = (1, 37, 60), 64


def batch_inputs(e):
    names = ("arbf", "vk", "rbf")
    ks = (e._lib.TgpKernel * NB)(*[spec_of(e, k).to_c() for k in names])
    ns = np.array(BATCH_NS, dtype=np.int64)
    X, y, yerr = np.zeros((NB, NMAX, 2)), np.zeros((NB, NMAX)), np.zeros((NB, NMAX))
    off = 0
    parts = []
    for b, n in enumerate(BATCH_NS):
        X[b, :n], y[b, :n], yerr[b, :n] = e.X[off:off + n], e.y[off:off + n], e.yerr[off:off + n]
        parts.append((e.X[off:off + n], e.y[off:off + n], e.yerr[off:off + n]))
        off += n
    ms = np.array(BATCH_MS, dtype=np.int64)
    Xq = np.zeros((NB, MMAX, 2))
    for b, m in enumerate(BATCH_MS):
        Xq[b, :m] = e.Xs[40 * b:40 * b + m]
    return names, ks, ns, X, y, yerr, parts, ms, Xq


def batch_args(ns, X, y, yerr):
    return [Arg("ns", "in", ns), Arg("X", "in", X), Arg("y", "in", y), Arg("yerr", "in", yerr)]


def rows_beyond_are_zero(a, counts, what):
    for b, c in enumerate(counts):
        assert not a[b, c:].any(), "%s: problem %d is not exactly 0 from row %d on" % (what, b, c)


def test_host_batched_entries(env):
    """tgp_gp_solve_batch, tgp_gp_loo_batch, tgp_gp_posterior_batch (variance and covariance): nb = 3, ns = (1, 100, 257) in rows of
    nmax = 300; ms = (1, 37, 60) in rows of mmax = 64.  The documented zeros behind ns[b] / ms[b] are asserted as well."""
    e = env
    lib, ctx, ops = e.lib, e.ctx, e.ops
    names, ks, ns, X, y, yerr, parts, ms, Xq = batch_inputs(e)
    kp = C.cast(ks, C.c_void_p)
    specs = [spec_of(e, k) for k in names]
    pX, py, pe = [p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts]
    common = [Arg("logdet", "out", shape=(NB,)), Arg("ydota", "out", shape=(NB,)), Arg("info", "out", shape=(NB,), dtype=np.int32)]

    args = batch_args(ns, X, y, yerr) + [Arg("alpha", "out", shape=(NB, NMAX))] + common
    outs, _ = host(e, "tgp_gp_solve_batch", args, lambda b: {"rc": checked(e, lib.tgp_gp_solve_batch(
        ctx, NB, kp, vp(b["ns"]), NMAX, vp(b["X"]), vp(b["y"]), vp(b["yerr"]), vp(b["alpha"]), vp(b["logdet"]), vp(b["ydota"]),
        vp(b["info"])), "tgp_gp_solve_batch")})
    assert not outs["info"].any()
    rows_beyond_are_zero(outs["alpha"], BATCH_NS, "tgp_gp_solve_batch alpha")
    w_alpha, w_logdet, w_chi2, _ = ops.gp_solve_batch(specs, pX, py, pe)
    for b, n in enumerate(BATCH_NS):
        same_as_wrapper(outs["alpha"][b, :n], w_alpha[b], "tgp_gp_solve_batch alpha[%d]" % b)
    same_as_wrapper(outs["logdet"], w_logdet, "tgp_gp_solve_batch logdet")
    same_as_wrapper(outs["ydota"], w_chi2, "tgp_gp_solve_batch ydota")
    solve_outs = outs

    args = batch_args(ns, X, y, yerr) + [Arg("alpha", "out", shape=(NB, NMAX)), Arg("invdiag", "out", shape=(NB, NMAX))] + common
    outs, _ = host(e, "tgp_gp_loo_batch", args, lambda b: {"rc": checked(e, lib.tgp_gp_loo_batch(
        ctx, NB, kp, vp(b["ns"]), NMAX, vp(b["X"]), vp(b["y"]), vp(b["yerr"]), vp(b["alpha"]), vp(b["invdiag"]), vp(b["logdet"]),
        vp(b["ydota"]), vp(b["info"])), "tgp_gp_loo_batch")})
    rows_beyond_are_zero(outs["alpha"], BATCH_NS, "tgp_gp_loo_batch alpha")
    rows_beyond_are_zero(outs["invdiag"], BATCH_NS, "tgp_gp_loo_batch invdiag")
    for k in ("alpha", "logdet", "ydota", "info"):                 # include/tgp.h: "as tgp_gp_solve_batch, bit for bit"
        same_as_wrapper(outs[k], solve_outs[k], "tgp_gp_loo_batch %s against tgp_gp_solve_batch" % k)
    w_invdiag = ops.gp_loo_batch(specs, pX, py, pe)[1]
    for b, n in enumerate(BATCH_NS):
        same_as_wrapper(outs["invdiag"][b, :n], w_invdiag[b], "tgp_gp_loo_batch invdiag[%d]" % b)

    pq = [Xq[b, :m] for b, m in enumerate(BATCH_MS)]
    for what, shape in ((1, (NB, MMAX)), (2, (NB, MMAX, MMAX))):
        args = batch_args(ns, X, y, yerr) + [Arg("ms", "in", ms), Arg("Xs", "in", Xq), Arg("alpha", "out", shape=(NB, NMAX)),
                                             Arg("unc", "out", shape=shape)] + common
        outs, _ = host(e, "tgp_gp_posterior_batch what=%d" % what, args, lambda b: {"rc": checked(e, lib.tgp_gp_posterior_batch(
            ctx, NB, kp, vp(b["ns"]), NMAX, vp(b["X"]), vp(b["y"]), vp(b["yerr"]), vp(b["ms"]), MMAX, vp(b["Xs"]), what, vp(b["alpha"]),
            vp(b["unc"]), vp(b["logdet"]), vp(b["ydota"]), vp(b["info"])), "tgp_gp_posterior_batch")})
        for k in ("alpha", "logdet", "ydota", "info"):
            same_as_wrapper(outs[k], solve_outs[k], "tgp_gp_posterior_batch %s against tgp_gp_solve_batch" % k)
        w_unc = ops.gp_posterior_batch(specs, pX, py, pe, pq, what="var" if what == 1 else "cov")[1]
        for b, m in enumerate(BATCH_MS):
            u = outs["unc"][b]
            if what == 1:
                same_as_wrapper(u[:m], w_unc[b], "tgp_gp_posterior_batch var[%d]" % b)
                assert not u[m:].any(), b
            else:
                same_as_wrapper(u[:m, :m], w_unc[b], "tgp_gp_posterior_batch cov[%d]" % b)
                assert not u[m:].any() and not u[:, m:].any(), b


@pytest.mark.parametrize("kn", [1, 33, 128])
def test_host_local_entries(env, kn):
    """tgp_gp_predict_local (m = 37 queries) and tgp_gp_local_cond on n = 20 training rows: nbr (m, kn) / (n, kn) int32, the -1
    padding from column 20 (19 for leave-one-out) on and nothing behind it, cnt, info, sums"""
    import test_gpu_local as TL               # their raw-call helpers: optional outputs as NULL
    import test_gpu_vecchia as TV
    e = env
    lib, ctx, ops = e.lib, e.ctx, e.ops
    n, m = 20, 37
    X, y, yerr, Xq = e.X[:n], e.y[:n], e.yerr[:n], e.Xs[:m]
    i32 = np.int32
    for name in ("arbf", "vk"):
        spec = spec_of(e, name)
        kc = spec.to_c()
        args = [Arg("X", "in", X), Arg("y", "in", y), Arg("yerr", "in", yerr), Arg("Xs", "in", Xq), Arg("ys", "out", shape=(m,)),
                Arg("var", "out", shape=(m,)), Arg("nbr", "out", shape=(m, kn), dtype=i32), Arg("info", "out", shape=(m,), dtype=i32)]
        outs, _ = host(e, "tgp_gp_predict_local %s kn=%d" % (name, kn), args, lambda b: {"rc": checked(e, lib.tgp_gp_predict_local(
            ctx, C.byref(kc), vp(b["X"]), n, vp(b["y"]), vp(b["yerr"]), vp(b["Xs"]), m, kn, vp(b["ys"]), vp(b["var"]), vp(b["nbr"]),
            vp(b["info"])), "tgp_gp_predict_local")})
        assert not outs["info"].any()
        w_ys, w_var, w_nbr = ops.gp_predict_local(spec, X, y, yerr, Xq, k=kn, return_var=True, return_neighbors=True)
        same_as_wrapper(outs["ys"], w_ys, "tgp_gp_predict_local ys")
        same_as_wrapper(outs["var"], w_var, "tgp_gp_predict_local var")
        same_as_wrapper(outs["nbr"][:, :min(kn, n)], w_nbr, "tgp_gp_predict_local nbr")
        assert (outs["nbr"][:, n:] == -1).all() and (outs["nbr"][:, :min(kn, n)] >= 0).all()
        rc, _, ys0, _, _, info0 = TL.raw_call(spec, X, y, yerr, Xq, kn, want_var=False, want_nbr=False)
        assert rc == 0
        same_as_wrapper(ys0, outs["ys"], "tgp_gp_predict_local ys with var = nbr = NULL")
        same_as_wrapper(info0, outs["info"], "tgp_gp_predict_local info with var = nbr = NULL")

        args = [Arg("X", "in", X), Arg("y", "in", y), Arg("yerr", "in", yerr), Arg("mu", "out", shape=(n,)), Arg("var", "out", shape=(n,)),
                Arg("nbr", "out", shape=(n, kn), dtype=i32), Arg("cnt", "out", shape=(n,), dtype=i32),
                Arg("info", "out", shape=(n,), dtype=i32), Arg("sums", "out", shape=(3,))]
        outs, _ = host(e, "tgp_gp_local_cond %s kn=%d" % (name, kn), args, lambda b: {"rc": checked(e, lib.tgp_gp_local_cond(
            ctx, C.byref(kc), vp(b["X"]), n, vp(b["y"]), vp(b["yerr"]), 0, None, kn, None, vp(b["mu"]), vp(b["var"]), vp(b["nbr"]),
            vp(b["cnt"]), vp(b["info"]), vp(b["sums"])), "tgp_gp_local_cond")})
        assert not outs["info"].any() and (outs["cnt"] == min(kn, n - 1)).all()
        w_mu, w_var, w_sums, w_nbr, w_cnt = ops.gp_local_cond(spec, X, y, yerr, k=kn, mode="loo", return_neighbors=True)
        for k, w in (("mu", w_mu), ("var", w_var), ("sums", w_sums), ("nbr", w_nbr), ("cnt", w_cnt)):
            same_as_wrapper(outs[k], w, "tgp_gp_local_cond %s" % k)
        assert (outs["nbr"][:, n - 1:] == -1).all() and (outs["nbr"][:, :min(kn, n - 1)] >= 0).all()
        rc, _, o = TV.raw_call(spec, X, y, yerr, kn, want=("var", "info", "sums"))
        assert rc == 0 and (o["mu"] == -7.0).all() and (o["nbr"] == -7).all() and (o["cnt"] == -7).all()
        for k in ("var", "info", "sums"):
            same_as_wrapper(o[k], outs[k], "tgp_gp_local_cond %s with mu = nbr = cnt = NULL" % k)


if __name__ == "__main__":
    assert sys.argv[1:] == ["predict"]
    print("GUARD OK generic=%d cases=%d" % ("TGP_PREDICT_GENERIC" in os.environ, predict_cases(_env())))

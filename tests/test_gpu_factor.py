"""The packed Cholesky factor itself, in every schedule regime of launch_potrf (csrc/chol.hip), against plain fp64 references.

The references are torch on the device (rocBLAS GEMMs, torch.linalg.cholesky_ex / cholesky_solve where a reference factor is
needed): nothing shared with libtgp.so.  Two matrix families:
  (W) A = G G^T / n + I, G Gaussian: eigenvalues in [1, 5], and every panel's update moves every trailing entry by far more
      than round-off, so a wrong or missing update of any tile shows -- the tight, a-priori bounds are asserted on these;
  (K) the GP kernel matrices the package factors in practice (star field, headline kernel, y_err^2), late pivots small.
Matrices go to tgp_d_potrf in the panel layout of include/tgp.h with the tile above the diagonal in each panel's first 128 rows
(rows 0..127, columns 128..255 -- never written by the K build, stale in the context's factor cache) set to NaN: a factorisation
or sweep that read it would return NaN.

Run as a script (`python tests/test_gpu_factor.py Np,Np,...`) it checks the factor, the inverted blocks and the failing-pivot
index at those sizes under whatever schedule the environment forces (test_forced_schedules)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53                  # unit round-off of fp64
PW, TB = 256, 128               # panel width, diagonal block


def gamma(k):
    return k * U / (1.0 - k * U)


# Sizes (Np = n rounded up to 256) and the branch of launch_potrf each one is for.  T = tile rows of the trailing matrix,
# T3 = T2 - 4 = the bulk update of a pair step (queued for small_t = 8 < T3 <= 64, units kept clear: 1 from T3 = 42 up, 2 from 26,
# else 3); U1 / U2a above 128 tile rows take syrk_dtv_kernel with a strip; groups of four (mode 3) from Np = 18432, handing over to
# pairs once T4 <= 96.
SIZES = [
    1280,       # mode 1: pairs on one stream
    1536,       # mode 2, T3 = 4 then 0: the chain has the chip to itself, no queued step
    2304,       # mode 2, T3 = 10: queued bulk keeping 3 units clear
    4608,       # mode 2, T3 = 28, 24, ...: queued with 2, then 3 units clear
    6912,       # mode 2, T3 = 46, 42, 38, ..., 26, 22, ...: queued with 1, 2, 3 units clear
    9472,       # mode 2, T3 = 66 (plain bulk launch, U2a not split), then 62, ...: queued
    17920,      # mode 2, U1 at T1 = 138, U2a at T2 = 136: syrk_dtv_kernel strips
    18432,      # mode 3, nP = 72 (nP % 4 = 0), hand-over at k = 20
    18688,      # mode 3, nP = 73 (1)
    18944,      # mode 3, nP = 74 (2)
    19200,      # mode 3, nP = 75 (3)
]
RAGGED_AT = [1280, 4608, 18432]          # one per mode: n = Np - 1, Np - 128 (last panel's second block all padding), Np - 129
RAGGED = [Np - d for Np in RAGGED_AT for d in (1, 128, 129)]


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
        _ENV = e
    return _ENV


@pytest.fixture(scope="module")
def env():
    return _env()


def _vp(t):
    return C.c_void_p(t.data_ptr())


class _DeviceArray(object):
    """library-owned device memory as a torch tensor without a copy"""

    def __init__(self, ptr, numel):
        self.__cuda_array_interface__ = {"shape": (int(numel),), "typestr": "<f8", "data": (int(ptr), False), "strides": None,
                                         "version": 2}


def padded(e, A, n):
    """(n, n) -> (Np, Np) with identity padding, as the library pads"""
    Np = int(e.lib.tgp_padded_n(n))
    if Np == n:
        return A
    Ap = e.torch.zeros(Np, Np, dtype=A.dtype, device=A.device)
    Ap[:n, :n] = A
    Ap.diagonal()[n:] = 1.0
    return Ap


def pack(e, Ap):
    """dense (Np, Np) device matrix -> the packed panels of tgp.h: panel p = rows 256 p .. Np-1 of columns 256 p .. +255.  The
    128 x 128 diagonal blocks are taken whole (symmetric for a symmetric Ap); the tile above the diagonal in each panel's first
    128 rows is NaN."""
    Np = Ap.shape[0]
    P = e.torch.empty(int(e.lib.tgp_panel_elems(Np)), dtype=e.torch.float64, device=e.dev)
    for p in range(Np // PW):
        off, m = int(e.lib.tgp_panel_off(p, Np)), Np - PW * p
        blk = P[off:off + m * PW].view(m, PW)
        blk.copy_(Ap[PW * p:, PW * p:PW * (p + 1)])
        blk[:TB, TB:] = float("nan")
    return P


def unpack(e, P, Np):
    """packed panels -> dense lower-triangular (Np, Np)"""
    L = e.torch.zeros(Np, Np, dtype=e.torch.float64, device=e.dev)
    for p in range(Np // PW):
        off, m = int(e.lib.tgp_panel_off(p, Np)), Np - PW * p
        L[PW * p:, PW * p:PW * (p + 1)] = P[off:off + m * PW].view(m, PW)
    return L.tril_()


def potrf(e, P, Np):
    """tgp_d_potrf in place on P; returns (info, W) with W the (Np / 128, 128, 128) inverted diagonal blocks"""
    W = e.torch.empty(Np // TB, TB, TB, dtype=e.torch.float64, device=e.dev)
    e.torch.cuda.synchronize()
    info = e.lib.tgp_d_potrf(e.ctx, _vp(P), Np, _vp(W))
    e._lib.check(e.ctx, info, "tgp_d_potrf")
    return info, W


def family_w(e, n, seed):
    """A = G G^T / n + I, exactly symmetric; eigenvalues in [1, 5]"""
    torch = e.torch
    g = torch.Generator(device=e.dev).manual_seed(seed)
    G = torch.randn(n, n, generator=g, dtype=torch.float64, device=e.dev)
    A = G @ G.T
    del G
    A = (A + A.T) * (0.5 / n)
    A.diagonal().add_(1.0)
    return A


def family_k(e, n):
    """K = amp k(X) + diag(y_err^2) of the star field with the headline kernel, built by torch elementwise ops; and the solve's
    inputs"""
    from treegp_amd.synthetic import star_field, headline_invlam
    torch = e.torch
    X, y, y_err, _ = star_field(n, 16)
    iL = headline_invlam()
    a, b, c = iL[0, 0], iL[0, 1], iL[1, 1]
    tX = torch.from_numpy(X).to(e.dev)
    K = torch.empty(n, n, dtype=torch.float64, device=e.dev)
    for s in range(0, n, 4096):
        d0 = tX[s:s + 4096, None, 0] - tX[None, :, 0]
        d1 = tX[s:s + 4096, None, 1] - tX[None, :, 1]
        K[s:s + 4096] = torch.exp(-0.5 * (a * d0 * d0 + 2.0 * b * d0 * d1 + c * d1 * d1))
    K.diagonal().copy_(1.0 + torch.from_numpy(y_err ** 2).to(e.dev))
    spec = e.ops.KernelSpec(e._lib.TGP_ARBF, amp=1.0, a=a, b=b, c=c)
    return K, spec, X, y - y.mean(), y_err


def componentwise_backward(A, L):
    """max_ij |A - L L^T|_ij / sqrt(A_ii A_jj)"""
    R = A - L @ L.T
    d = A.diagonal().abs().sqrt()
    R.abs_().div_(d[:, None]).div_(d[None, :])
    return float(R.max())


def check_factor(e, Ap, L, n, label):
    """test 1's bounds on a factor L of the padded matrix Ap: componentwise backward error <= gamma_{n+1} (the standard bound
    for Cholesky, with |L||L|^T <= sqrt(A_ii A_jj)), forward error <= 1e-12 max|L_ref| against rocSOLVER's factor.
    Returns (backward, forward) for the record."""
    torch = e.torch
    assert bool(torch.isfinite(L).all()), "%s: the factor holds non-finite values" % label
    bwd = componentwise_backward(Ap, L)
    Lref, info = torch.linalg.cholesky_ex(Ap)
    assert int(info) == 0
    scale = float(Lref.abs().max())
    fwd = float(Lref.sub_(L).abs_().max()) / scale
    del Lref
    print("%s n=%d: backward %.3e (bound %.3e)  forward %.3e (bound 1e-12)" % (label, n, bwd, gamma(n + 1), fwd))
    assert bwd <= gamma(n + 1), (label, n, bwd, gamma(n + 1))
    assert fwd <= 1e-12, (label, n, fwd)
    return bwd, fwd


def check_inverted_blocks(e, W, L, n, label, c=4.0, identity_blocks_exact=False):
    """test 2: |W_b L_bb - I| <= c 128 u (|W_b| |L_bb|) elementwise for every 128-block b (the triangular inverse's residual
    bound plus the product's own rounding); blocks wholly in the padding are I to the same bound (exactly I where
    `identity_blocks_exact` -- set_identity128_kernel wrote them)."""
    torch = e.torch
    Np = L.shape[0]
    nb = Np // TB
    L = L.contiguous()
    Lb = L.as_strided((nb, TB, TB), ((Np + 1) * TB, Np, 1))
    I = torch.eye(TB, dtype=torch.float64, device=e.dev)
    assert bool(torch.isfinite(W).all()), "%s: inverted blocks hold non-finite values" % label
    E = (torch.bmm(W, Lb) - I).abs_()
    B = torch.bmm(W.abs(), Lb.abs())
    ratio = float((E / B.clamp_min(1e-300)).max()) / U          # in units of u, for the record
    bad = (E > B.mul_(c * TB * U)).nonzero()
    assert bad.shape[0] == 0, "%s n=%d: W_b L_bb - I out of bound at (block, i, j) %s" % (label, n, bad[:5].tolist())
    first_pad = -(-n // TB)
    if first_pad < nb:
        D = (W[first_pad:] - I).abs_()
        assert float(D.max()) <= c * TB * U, (label, n, float(D.max()))
        off = D * (1.0 - I)
        assert float(off.max()) == 0.0, (label, n)
        if identity_blocks_exact:
            assert float(D.max()) == 0.0, (label, n)
    return ratio


# ---- 1 + 2: tgp_d_potrf on family (W), every regime -----------------------------------------------------------------------

def _potrf_w(e, n, seed=None):
    A = family_w(e, n, seed if seed is not None else n)
    Ap = padded(e, A, n)
    del A
    Np = Ap.shape[0]
    P = pack(e, Ap)
    info, W = potrf(e, P, Np)
    assert info == 0, (n, info)
    L = unpack(e, P, Np)
    return Ap, P, W, L


@pytest.mark.parametrize("n", SIZES + RAGGED)
def test_potrf_backward_and_forward_error(env, n):
    """tgp_d_potrf on (W): componentwise backward error <= gamma_{n+1}, forward error <= 1e-12 max|L_ref|.
    Measured on an MI355X: backward 2.6e-15 (n = 1280), 6.8e-15 (4608), 1.0e-14 (9472), 1.4 - 1.7e-14 (17920 - 19200), i.e.
    ~2 % of gamma_{n+1} at n = 1280 and under 1 % from 4608 on; forward 6e-16 (1280) rising to 1.0e-14 (17920), at most 1 % of
    the 1e-12 bound.  The ragged sizes read the same as their Np."""
    Ap, P, W, L = _potrf_w(env, n)
    del P, W
    check_factor(env, Ap, L, n, "potrf")


@pytest.mark.parametrize("n", SIZES + RAGGED)
def test_potrf_inverted_diagonal_blocks(env, n):
    """Every 128-block of d_W (the sweeps are built on all of them), padding blocks included, against the factor's own
    diagonal blocks."""
    Ap, P, W, L = _potrf_w(env, n)
    ratio = check_inverted_blocks(env, W, L, n, "potrf")
    print("n=%d: max |W L - I| / (|W||L|) = %.2f u (bound %d u)" % (n, ratio, 4 * TB))


# ---- 3: the production solve's factor (panel_mid_kernel, the n_data identity branch) ----------------------------------------

def _dense_solve(e, K, n, y=None, want_alpha=True, keep=False):
    """tgp_d_gp_solve_dense on a dense device (n, n) matrix -> (rc, alpha, logdet, ydota, handle)"""
    torch = e.torch
    if y is None:
        y = torch.ones(n, dtype=torch.float64, device=e.dev)
    alpha = torch.empty(n, dtype=torch.float64, device=e.dev) if want_alpha else None
    logdet, ydota, h = C.c_double(0.0), C.c_double(0.0), C.c_void_p()
    torch.cuda.synchronize()
    rc = e.lib.tgp_d_gp_solve_dense(e.ctx, _vp(K), n, _vp(y), None, _vp(alpha) if want_alpha else None, C.byref(logdet),
                                    C.byref(ydota), C.byref(h) if keep else None)
    e._lib.check(e.ctx, rc, "tgp_d_gp_solve_dense")
    return rc, alpha, logdet.value, ydota.value, (h if keep and rc == 0 else None)


def kept_factor(e, h):
    """(packed panels, inverted blocks, Np) of a kept factor, copied out through tgp_factor_device"""
    dA, dW, Np = C.c_void_p(), C.c_void_p(), C.c_int64()
    e._lib.check(e.ctx, e.lib.tgp_factor_device(e.ctx, h, C.byref(dA), C.byref(dW), C.byref(Np)), "tgp_factor_device")
    Np = Np.value
    torch = e.torch
    P = torch.as_tensor(_DeviceArray(dA.value, e.lib.tgp_panel_elems(Np)), device=e.dev).clone()
    W = torch.as_tensor(_DeviceArray(dW.value, Np * TB), device=e.dev).clone().view(Np // TB, TB, TB)
    return P, W, Np


@pytest.mark.parametrize("n", RAGGED)
def test_production_solve_factor(env, n):
    """The factor tgp_d_gp_solve_dense keeps (what tgp_d_potrf cannot reach: panel_mid_kernel, and the identity branch for a
    last panel whose second block is all padding): the bounds of tests 1 and 2, and padding rows that are exactly those of
    the identity (off-diagonal == 0, diagonal within 2u of 1)."""
    e = env
    A = family_w(e, n, n + 1)
    rc, _, _, _, h = _dense_solve(e, A, n, keep=True)
    assert rc == 0
    try:
        P, W, Np = kept_factor(e, h)
    finally:
        e.lib.tgp_factor_free(e.ctx, h)
    L = unpack(e, P, Np)
    Ap = padded(e, A, n)
    del A
    check_factor(e, Ap, L, n, "solve")
    check_inverted_blocks(e, W, L, n, "solve", identity_blocks_exact=(Np - n >= TB))
    pad = L[n:]
    off = pad.clone()
    off[:, n:].diagonal().zero_()
    assert float(off.abs().max()) == 0.0
    assert float((pad[:, n:].diagonal() - 1.0).abs().max()) <= 2 * U


@pytest.mark.parametrize("n", [4608, 18432])
def test_production_solve_factor_has_the_bits_of_potrf(env, n):
    """n = Np: the kept factor of the production solve (panel_mid_kernel in the chain-alone steps) equals tgp_d_potrf's factor of
    the same matrix bit for bit (factor_panel: the launch-by-launch twin does the same arithmetic).  tgp_d_potrf's input has the
    tiles above the diagonal NaN, the solve's the true values: equal bits also say that nobody read them."""
    e = env
    A = family_w(e, n, n + 2)
    rc, _, _, _, h = _dense_solve(e, A, n, keep=True)
    assert rc == 0
    try:
        P1, W1, Np = kept_factor(e, h)
    finally:
        e.lib.tgp_factor_free(e.ctx, h)
    P2 = pack(e, A)
    info, W2 = potrf(e, P2, n)
    assert info == 0
    L1, L2 = unpack(e, P1, Np), unpack(e, P2, Np)
    assert bool(e.torch.equal(L1, L2)), "factor differs at %d entries" % int((L1 != L2).sum())
    assert bool(e.torch.equal(W1, W2)), "inverted blocks differ at %d entries" % int((W1 != W2).sum())


# ---- 4: kernel matrices (K) through the parametrised solve ----------------------------------------------------------------

@pytest.mark.parametrize("n", [9000, 18500])          # Np = 9216 (mode 2, queued steps), 18688 (mode 3, nP % 4 = 1)
def test_kernel_matrix_factor_residual_against_rocsolver(env, n):
    """ops.gp_solve(keep=True) on (K).  The componentwise bound does not hold here (the inverted diagonal blocks make the error
    scale with cond(L_kk)): the normwise residual ||A - L L^T||_F / ||A||_F is held to max(16 x rocSOLVER's on the same matrix,
    n u).  Before the solve the context's factor cache is left with NaN in every tile above the diagonal (a dense solve whose
    mirrored entries there are NaN, and fails at pivot 129): the K build does not write those tiles, so the solve must not read
    them."""
    e = env
    torch = e.torch
    Np = int(e.lib.tgp_padded_n(n))
    poison = torch.eye(n, dtype=torch.float64, device=e.dev)
    for p in range(Np // PW):
        poison[PW * p + TB:PW * (p + 1), PW * p:PW * p + TB] = float("nan")
    rc = _dense_solve(e, poison, n, want_alpha=False)[0]
    assert rc == TB + 1, rc
    del poison
    K, spec, X, y, y_err = family_k(e, n)
    alpha, logdet, _, fac = e.ops.gp_solve(spec, X, y, y_err, keep=True)
    try:
        P, W, Np2 = kept_factor(e, fac._h)
    finally:
        fac.free()
    assert Np2 == Np
    Ap = padded(e, K, n)
    del K
    L = unpack(e, P, Np)
    del P
    nA = float(torch.linalg.norm(Ap))
    ours = float(torch.linalg.norm(Ap - L @ L.T)) / nA
    Lref, info = torch.linalg.cholesky_ex(Ap)
    assert int(info) == 0
    ref = float(torch.linalg.norm(Ap - Lref @ Lref.T)) / nA
    print("K n=%d: ||A - LL^T||_F / ||A||_F = %.3e, rocSOLVER %.3e" % (n, ours, ref))
    assert ours <= max(16.0 * ref, n * U), (ours, ref)
    assert np.isfinite(alpha).all() and math.isfinite(logdet)


# ---- 5: solves on the factor -------------------------------------------------------------------------------------------

def _normwise_backward(A, x, b):
    """||A x - b||_inf / (||A||_inf ||x||_inf + ||b||_inf), column by column"""
    r = (A @ x - b).abs().max(dim=0).values
    nA = float(A.abs().sum(dim=1).max())
    return (r / (nA * x.abs().max(dim=0).values + b.abs().max(dim=0).values)).max().item()


@pytest.mark.parametrize("n", [1280, 4608 - 129, 9472, 18688 - 1])
def test_potrs_on_the_factor(env, n):
    """tgp_d_potrs (one right-hand side) and tgp_d_potrs_multi (4 and 5: the factor is read once per 4 fields): normwise
    backward error <= n u; padding entries of x stay exactly 0 where b's are 0."""
    e = env
    torch = e.torch
    Ap, P, W, L = _potrf_w(e, n)
    del L
    Np = Ap.shape[0]
    g = torch.Generator(device=e.dev).manual_seed(7)
    for nrhs in (1, 4, 5):
        B = torch.zeros(nrhs, Np, dtype=torch.float64, device=e.dev)
        B[:, :n] = torch.randn(nrhs, n, generator=g, dtype=torch.float64, device=e.dev)
        X = B.clone()
        torch.cuda.synchronize()
        if nrhs == 1:
            rc = e.lib.tgp_d_potrs(e.ctx, _vp(P), _vp(W), Np, _vp(X))
        else:
            rc = e.lib.tgp_d_potrs_multi(e.ctx, _vp(P), _vp(W), Np, _vp(X), nrhs)
        e._lib.check(e.ctx, rc, "potrs")
        assert bool(torch.isfinite(X).all())
        if Np > n:
            assert float(X[:, n:].abs().max()) == 0.0
        eta = _normwise_backward(Ap, X.T, B.T)
        print("n=%d nrhs=%d: normwise backward error %.3e (bound %.3e)" % (n, nrhs, eta, n * U))
        assert eta <= n * U, (n, nrhs, eta)


@pytest.mark.parametrize("n", [4608 - 129, 9472 - 1])
def test_augmented_row_solve_against_torch(env, n):
    """n < Np, factor not kept: y rides through the factorisation as a matrix row (ops.gp_solve_dense with and without alpha).
    alpha and the log-determinant to 1e-12 relative, y . alpha to 1e-11 relative against cholesky_ex / cholesky_solve."""
    e = env
    torch = e.torch
    A = family_w(e, n, n + 3)
    g = torch.Generator(device=e.dev).manual_seed(n)
    ty = torch.randn(n, generator=g, dtype=torch.float64, device=e.dev)
    Lref, info = torch.linalg.cholesky_ex(A)
    assert int(info) == 0
    a_ref = torch.cholesky_solve(ty[:, None], Lref)[:, 0]
    ld_ref = float(2.0 * torch.log(Lref.diagonal()).sum())
    del Lref
    yd_ref = float(ty @ a_ref)
    a_ref = a_ref.cpu().numpy()
    K, y = A.cpu().numpy(), ty.cpu().numpy()
    del A
    alpha, logdet, ydota, _ = e.ops.gp_solve_dense(K, y)
    _, logdet2, ydota2, _ = e.ops.gp_solve_dense(K, y, want_alpha=False)
    err_a = np.abs(alpha - a_ref).max() / np.abs(a_ref).max()
    print("n=%d: alpha %.2e  logdet %.2e / %.2e  y.alpha %.2e / %.2e" % (
        n, err_a, abs(logdet - ld_ref) / abs(ld_ref), abs(logdet2 - ld_ref) / abs(ld_ref), abs(ydota - yd_ref) / abs(yd_ref),
        abs(ydota2 - yd_ref) / abs(yd_ref)))
    assert err_a <= 1e-12, err_a
    for ld, yd in ((logdet, ydota), (logdet2, ydota2)):
        assert abs(ld - ld_ref) <= 1e-12 * abs(ld_ref), (ld, ld_ref)
        assert abs(yd - yd_ref) <= 1e-11 * abs(yd_ref), (yd, yd_ref)


# ---- 6: the first failing pivot ------------------------------------------------------------------------------------------

def _unit_lower(e, n, seed):
    """L0 = I + 0.3 / sqrt(n) * strictly lower Gaussian, and L0 L0^T (exactly symmetric)"""
    torch = e.torch
    g = torch.Generator(device=e.dev).manual_seed(seed)
    L0 = torch.randn(n, n, generator=g, dtype=torch.float64, device=e.dev).tril_(-1).mul_(0.3 / math.sqrt(n))
    L0.diagonal().fill_(1.0)
    A0 = L0 @ L0.T
    A0 = (A0 + A0.T) * 0.5
    return L0, A0


# the four forms of the production solve, taken in turn over the positions (augmented row or not, panel_mid_kernel)
_SOLVE_FORMS = [(False, True), (False, False), (True, True), (True, False)]     # (keep, want_alpha)


def check_first_failing_pivot(e, n, positions, nan_entries=(), host_api=False, form0=0):
    """A = L0 D L0^T with D = I but D_jj = -1: the leading minors of order < j are positive definite, the one of order j is
    not -- LAPACK's answer is exactly j, by construction.  A NaN at (i, k), i > k (upper mirror finite, in another 256-panel):
    the answer is i + 1.  tgp_d_potrf must return the raw index (never one in the padding); the production solve must report it
    too (through ops.gp_solve_dense and its LinAlgError message where `host_api`)."""
    torch = e.torch
    L0, A0 = _unit_lower(e, n, 1000 + n)
    Np = int(e.lib.tgp_padded_n(n))
    cases = [(j, ("pivot", j)) for j in positions] + [(i + 1, ("nan", i, k)) for i, k in nan_entries]
    form = form0
    for expect, what in cases:
        if what[0] == "pivot":
            j = what[1]
            l = L0[:, j - 1]
            A = A0 - 2.0 * torch.outer(l, l)
        else:
            _, i, k = what
            assert i > k and i // PW != k // PW
            A = A0.clone()
            A[i, k] = float("nan")
        info, _ = potrf(e, pack(e, padded(e, A, n)), Np)
        assert info == expect, ("tgp_d_potrf", n, what, info)
        keep, want_alpha = _SOLVE_FORMS[form % 4]
        form += 1
        if host_api:
            with pytest.raises(np.linalg.LinAlgError, match=r"^%d-th leading minor " % expect):
                e.ops.gp_solve_dense(A.cpu().numpy(), np.ones(n), keep=keep, want_alpha=want_alpha)
        else:
            rc = _dense_solve(e, A, n, want_alpha=want_alpha, keep=keep)[0]
            assert rc == expect, ("tgp_d_gp_solve_dense", n, what, keep, want_alpha, rc)
        del A
    return form


EDGE_POSITIONS = [1, 16, 17, 32, 33, 128, 129, 256, 257]      # 16-row halves of the sweep, block and panel edges


@pytest.mark.parametrize("n", [1536, 1536 - 128, 4608, 4608 - 128])
def test_first_failing_pivot_at_the_edges(env, n):
    """Edge positions, the last data row n (n = Np - 128: the last panel's second block is padding), and NaN entries."""
    positions = EDGE_POSITIONS if n % PW == 0 else [1, 17, 129, 257]
    check_first_failing_pivot(env, n, positions + [n], nan_entries=[(300, 10), (n - 1, 255)], host_api=True, form0=n // PW)


# (n, positions): a pivot where a particular step of the schedule factors it
SCHEDULE_POSITIONS = [
    (4608, [PW * 2 + 140, PW * 3 + 5]),                       # panels 2, 3: the first queued step (potrf128_solo_kernel)
    (9472, [PW * 2 + 77, PW * 4 + 200]),                      # panel 2 beside the plain bulk of T3 = 66; panel 4: first queued step
    (17920, [PW * 1 + 3, PW * 2 + 130]),                      # right after U1 / U2a on syrk_dtv_kernel strips
    (18688, [PW * 9 + 1, PW * 10 + 128, PW * 11 + 255,        # panels 1, 2, 3 of the group k0 = 8 (side stream)
             PW * 31 + 64, 18688]),                           # the pair tail after the hand-over at k = 24; the last row
]


@pytest.mark.parametrize("n,positions", SCHEDULE_POSITIONS, ids=[str(n) for n, _ in SCHEDULE_POSITIONS])
def test_first_failing_pivot_in_schedule_steps(env, n, positions):
    check_first_failing_pivot(env, n, positions, form0=1)


# ---- 7: forced schedules, one fresh process each (the switches are read once per process) -----------------------------------

FORCED = [
    ({"TGP_CHOL_MODE": "0"}, [3328, 3584, 3840, 4096]),
    ({"TGP_CHOL_MODE": "1"}, [3328, 3584, 3840, 4096]),
    ({"TGP_CHOL_MODE": "2"}, [3328, 3584, 3840, 4096]),
    ({"TGP_CHOL_MODE": "3", "TGP_QUAD_TAIL_TILES": "0"}, [3328, 3584, 3840, 4096]),     # nP % 4 = 1, 2, 3, 0: partial last group
    ({"TGP_SYNC_EVENTS": "1"}, [4608, 18688]),
]


def run_sizes(sizes):
    """tests 1, 2 and 6 at these sizes, under the schedule the environment selects"""
    e = _env()
    for Np in sizes:
        Ap, P, W, L = _potrf_w(e, Np)
        check_factor(e, Ap, L, Np, "forced")
        check_inverted_blocks(e, W, L, Np, "forced")
        del Ap, P, W, L
        last = Np // PW - 1
        check_first_failing_pivot(e, Np, [1, 129, 257, PW * (last - 1) + 100, PW * last + 129, Np],
                                  nan_entries=[(PW * last + 3, PW * (last - 2) + 7)], form0=Np // PW)
    print("FORCED OK")


@pytest.mark.parametrize("setting,sizes", FORCED, ids=["-".join("%s=%s" % kv for kv in s.items()) for s, _ in FORCED])
def test_forced_schedules(setting, sizes):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), ",".join(str(s) for s in sizes)],
                       env=dict(os.environ, **setting), capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "FORCED OK" in r.stdout, (setting, r.stdout[-1500:], r.stderr[-3000:])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    run_sizes([int(s) for s in sys.argv[1].split(",")])

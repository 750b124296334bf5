"""Every tgp_dd_* building block of the distributed Cholesky against a dense long-double reference of one rank's share, and the
whole distributed factor twice, bit for bit.

Single-threaded part: a `HipLocalOps` in the test thread, the entry point called directly (no virtual ranks, no communicator).
The rank's share and the all-gathered panels come from a host (NumPy fp64) partial factorisation of a dense matrix -- operands
with the factor's structure -- through the index helpers of tests/_dist_block_refs.py; every region the K build or the panel
exchange never writes (the tile above the diagonal in a diagonal block's first 128 rows, gathered slots beyond a rank's count,
the share's slack) is NaN, so a kernel that read it would return NaN.  Families as in test_gpu_factor.py: (W) A = G G^T / n + I,
on which every tile's update moves far more than round-off, and (K) the star-field kernel matrix.

Shapes (n = Np unless said; nB = Np / 256) and the branch each is for:

  operation       shape                                   branch
  kbuild          G 1/3/8 x n 257/1100/1279, +- yerr      per-value bound of DESIGN section 5 (not bit equality with the single-GPU
                                                          build: see the test); ragged last block (n = 257: one data row in it); G = 8 > nB: empty ranks
  factor_diag     G 1, nB 15, panel 0 / panel 3           14 blocks below: throughput form / 11 below (<= 12): latency form; family (W)
                                                          at the a-priori bounds, family (K) at the checks that hold at any conditioning
  trsm            G 1, nB 15, panel 0 / panel 3           28 row tiles (> 24): 128-row tiles / 22: 16-row slices
  trsm            G 3, nB 5, panels 0 1 2, every rank     owner and receiver with zero, one and two blocks below
  update*         (G, g, nB, nseg, k) of UPDATE_CASES     nseg 1..4; nB = nseg + 1 (one trailing block) .. 9; g first / middle /
                                                          last of G 1/3/8; a rank without rows (8, 0); five column windows each
  queued / fused  G 3, g 2, nB 9, nseg 2                  the persistent grid with 1, 2, 3 clear units; the fused launch; the rank's
                                                          rows (blocks 2, 5, 8) reach the last tile column, so the window's end is checked
  strip_left      (G, g, nB, kgroup, j) of STRIP_CASES    j 1..3, owner (d_ext NULL) and receiver, kgroup 0 and > 0, b the last block,
                                                          G 8 / nB 9: the rank's first row block is five blocks below b
  keep / tail     G 1/3/8 x nB 5, k0 0 / 1 / nB - 1       tails of 5, 4, 1 blocks (no multiples of 3 or 8), NULL operands
  sweeps          G 1/3, nB 5, every panel, every rank    owner's diagonal steps, ranks with and without rows below
  logdet          G 1/3, nB 5, n = Np, Np - 1, Np - 255   padding rows in the last block

Bounds (u = 2^-53, gamma(k) = k u / (1 - k u)); the references' own error is 2^-11 u per operation (long double):
  factor_diag   as test_gpu_factor.py: |S - L L^T| <= gamma(257) sqrt(S_ii S_jj), |L - L_ref| <= 1e-12 max|L_ref|,
                |W_b L_bb - I| <= 4 * 128 u |W_b||L_bb|
  trsm          X0 = A0 W0^T and X1 = (A1 - X0 L10^T) W1^T are products with explicit inverses, so the residual of X L_kk^T = A is
                bounded through them: |R_h| <= gamma(129) M_h + 6 * 129 u M_h |W_h|^T |L_hh|^T with M_0 = |A_0|,
                M_1 = |A_1| + |X_0||L_10|^T (gamma(129): the inner GEMM; 4 * 128 u: W's own residual as asserted above; 128 u + 129 u:
                the product with W and the inner GEMM's error carried through it, plus one for second-order terms)
  updates       |C' - (C - sum A_s B_s^T)| <= gamma(256 nseg + 1) (|C| + sum |A_s||B_s|^T), any summation order
  sweeps        fwd_update: gamma(257)(|y| + |L||z|); bwd_partial: gamma(rows + 1) |L|^T|a| (its partial sums, one per 128 rows,
                are added in a fixed order; the bound holds for any order); diagonal steps multiply by W_h:
                |L_kk x - y| <= gamma(260) |L_d| (|W_d| t), t = |y| + |L_10||x_0| (and the transposed form with s), L_d / W_d the
                block diagonals.  This is NOT the gamma(257) |L||x| of a substitution: the kernels multiply by explicit inverses,
                whose residual goes through |L_d||W_d| (as the panel solve's does), so that is the form asserted; the error against
                gamma(257) |L_kk||x| is printed beside it for the record
  logdet        (gamma(terms) + 4 u) sum |2 log d|: the sum in any order, two roundings per term, log to one ulp
Products of the kernel family's far-off-diagonal entries underflow; the update and solve bounds carry 2^-1074 per operation
for that (the standard model with underflow)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_block_refs import (BB, LD, TB, U, cholesky_ld, family_k, family_w, first_difference, gamma, gather_panel,  # noqa: E402, F401
                              own_blocks, pack_share, pack_single, packed_offsets, padded_dense, partial_factor, share_offsets,
                              share_slot, shares_to_dense_lower, tail_blocks, unpack_share, update_reference, written_mask)
from treegp_amd.dist import BCAST_ELEMS, BLK, block_of, owner, panel_blocks, panel_cmax  # noqa: E402

gpu = pytest.mark.gpu
NAN = float("nan")
ETA = 2.0 ** -1074              # a product that underflows is off by up to half of this, absolutely (kernel matrices hold such entries)


# ---- 1: the index helpers, without a GPU ----------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("nB", [1, 2, 5, 9])
def test_share_helpers_round_trip_and_agree_with_the_numpy_stand_in(G, nB):
    import torch  # noqa: F401  (NumpyLocalOps returns torch tensors)
    from _dist_helpers import NumpyLocalOps
    Np = nB * BLK
    rng = np.random.default_rng(100 * G + nB)
    R = rng.standard_normal((Np, Np))
    R = R + R.T
    dense = np.zeros((Np, Np))
    seen = np.zeros((nB, nB), dtype=int)
    for g in range(G):
        share = pack_share(R, G, g, poison=False)
        off = share_offsets(nB, G, g)
        assert len(share) == off[-1] == sum(panel_blocks(p, nB, g, G) for p in range(nB)) * BB
        back = unpack_share(share, Np, G, g)
        mine = own_blocks(nB, G, g)
        assert mine == [b for b in range(nB) if owner(b, G) == g]
        for b in range(nB):
            for p in range(nB):
                blk = back[b * BLK:(b + 1) * BLK, p * BLK:(p + 1) * BLK]
                if b in mine and p <= b:
                    assert np.array_equal(blk, R[b * BLK:(b + 1) * BLK, p * BLK:(p + 1) * BLK])
                    assert share_slot(nB, G, g, p, b) == off[p] + [x for x in mine if x >= p].index(b) * BB
                    seen[b, p] += 1
                else:
                    assert np.isnan(blk).all()
        unpack_share(share, Np, G, g, out=dense)
        # the NumPy stand-in of the CPU tests stores full-width rows: its send views are the same blocks in the same order
        ref = NumpyLocalOps(R, Np, G, g)
        for k in range(nB):
            cmax = panel_cmax(k + 1, nB, G)
            view = ref.panel_send_view(k, cmax).numpy()
            skip = BB if owner(k, G) == g else 0
            cnt = panel_blocks(k + 1, nB, g, G)
            assert np.array_equal(view[:cnt * BB], share[int(off[k]) + skip:int(off[k]) + skip + cnt * BB])
        for k0 in range(nB):
            assert tail_blocks(k0, nB, G, g) == ref._tail_blocks(k0, g)
            t = tail_blocks(k0, nB, G, g)
            assert len(t) * BB == off[-1] - off[k0]
            for i, (p, b) in enumerate(t):
                assert share_slot(nB, G, g, p, b) == off[k0] + i * BB
        # the poisoned tile is the only difference poisoning makes
        ps = pack_share(R, G, g, poison=True)
        assert int(np.isnan(ps).sum()) == TB * TB * len(mine)
    assert np.array_equal(seen, np.tril(np.ones((nB, nB), dtype=int)))          # every lower block on exactly one rank
    assert np.array_equal(np.tril(dense), np.tril(R))
    assert np.array_equal(shares_to_dense_lower([pack_share(R, G, g) for g in range(G)], Np, G), np.tril(R))
    for k in range(nB):
        P, cmax = gather_panel(R, k, G)
        assert cmax == panel_cmax(k + 1, nB, G) and len(P) == max(G * cmax, 1) * BB
        for r in range(G):
            below = own_blocks(nB, G, r, k + 1)
            for i in range(cmax):
                blk = P[(r * cmax + i) * BB:(r * cmax + i + 1) * BB]
                if i < len(below):
                    assert np.array_equal(blk.reshape(BLK, BLK), R[below[i] * BLK:(below[i] + 1) * BLK, k * BLK:(k + 1) * BLK])
                else:
                    assert np.isnan(blk).all()
    assert np.array_equal(pack_single(R, poison=False), pack_share(R, 1, 0, poison=False))
    assert packed_offsets(Np)[-1] == len(pack_single(R))


# ---- plumbing of the GPU tests ----------------------------------------------------------------------------------------------

class _Env(object):
    pass


@functools.lru_cache(maxsize=None)
def _env():
    from treegp_amd import _lib, ops
    lib = _lib.load_library()
    import torch
    e = _Env()
    e.lib, e._lib, e.ops, e.torch = lib, _lib, ops, torch
    e.dev = torch.device("cuda", 0)
    from treegp_amd.synthetic import headline_invlam
    iL = headline_invlam()
    e.spec = ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=iL[0, 0], b=iL[0, 1], c=iL[1, 1])
    return e


def _local_ops(n, G, g):
    from treegp_amd.dist import HipLocalOps
    e = _env()
    o = HipLocalOps(e._lib.new_ctx(0), e.spec, n, G, g, e.dev, replicate=False)
    assert np.array_equal(o.loff, share_offsets(o.nB, G, g))                    # the helper's offsets are tgp_dist_panel_off's
    o.A.fill_(NAN)
    o.W.fill_(NAN)
    o.bcast_full.fill_(NAN)
    return o


def _ctx():
    """a context of its own whose launches go to torch's current stream, so that they order with the tensors' fills and copies"""
    e = _env()
    ctx = e._lib.new_ctx(0)
    e.lib.tgp_set_stream(ctx, C.c_void_p(e.torch.cuda.current_stream(e.dev).cuda_stream))
    return ctx


def _done(o):
    e = _env()
    e.torch.cuda.synchronize()
    e.lib.tgp_reset_stream(o.ctx)


def _put(o, share):
    t = _env().torch
    o.A.fill_(NAN)
    o.A[:len(share)].copy_(t.from_numpy(share))


def _get(o):
    _env().torch.cuda.synchronize()
    return o.A.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _inverse_ld(L):
    """inverse of a small lower-triangular block by forward substitution in long double (L W = I row after row: the residual is
    small element by element, |L W - I| <= gamma |L||W|, also where L's entries span hundreds of decades), rounded to fp64"""
    n = L.shape[0]
    Lq = L.astype(LD)
    W = np.zeros((n, n), dtype=LD)
    for i in range(n):
        rhs = -(Lq[i, :i] @ W[:i, :i + 1])
        rhs[i] += 1.0
        W[i, :i + 1] = rhs / Lq[i, i]
    return W.astype(np.float64)


def _bcast_of(Lkk):
    """[L_kk | W0 | W1] as the owner broadcasts it, from a host factor of the diagonal block"""
    return np.concatenate([Lkk.ravel(), _inverse_ld(Lkk[:TB, :TB]).ravel(), _inverse_ld(Lkk[TB:, TB:]).ravel()])


def _sym(M):
    return M + np.tril(M, -1).T


@functools.lru_cache(maxsize=None)
def _matrix(family, Np, seed=1):
    A = family_w(Np, seed) if family == "W" else family_k(Np, seed)[0]
    A.setflags(write=False)
    return A


# ---- 2a: K build --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _kbuild_reference(n):
    """the padded kernel matrix of the star field in long double (difference first, then the form, then exp: the reference's
    own error is (s + 3) 2^-64 relative, against a bound of (8 + 16 s) 2^-53), its exponents s, and the inputs"""
    from treegp_amd.synthetic import star_field
    e = _env()
    X, y, y_err, _ = star_field(n, 4, seed=n)
    sp = e.spec
    dx = X[:, None, 0].astype(LD) - X[None, :, 0].astype(LD)
    dy = X[:, None, 1].astype(LD) - X[None, :, 1].astype(LD)
    h = (LD(sp.a) * dx * dx + 2 * LD(sp.b) * dx * dy + LD(sp.c) * dy * dy) / 2
    return X, y_err, LD(sp.amp) * np.exp(-h), h.astype(np.float64)


@gpu
@pytest.mark.parametrize("with_yerr", [True, False])
@pytest.mark.parametrize("n", [257, 1100, 1279])
@pytest.mark.parametrize("G", [1, 3, 8])
def test_kbuild_share_values_and_layout(G, n, with_yerr):
    """tgp_dd_kbuild on every rank of G.  Its bits are NOT those of tgp_d_kbuild_lower (the single-GPU build evaluates a pair in
    256-row slabs, the distributed one in 128 x 128 tiles with another order of the exponent's operations: on an MI355X 97 % of
    the data values differ at n = 1279, by up to 951 ulp where the exponent is large -- (8 + 16 s) ulp is the accuracy of either),
    so every stored element is held to the per-value bound of DESIGN section 5
    instead, (8 + 16 s) 2^-53 ref + 2 * 2^-1074 with s = q / 2 (both builds difference first: S = s), plus the documented
    stand-in below the clamp -- the single-GPU build is held to the same bound beside it, and the number of differing elements
    and their largest distance in ulps are printed.  Layout: exactly the rank's blocks are written (the tile above the diagonal
    and the share's slack stay NaN), padding rows and columns are the identity's, the diagonal is amp + yerr^2 to one rounding
    (the kernel may fuse the multiply-add)."""
    from _kernel_value_helpers import gauss_bound
    e = _env()
    torch, lib = e.torch, e.lib
    from treegp_amd._lib import as_xy
    X, y_err, ref, h = _kbuild_reference(n)
    amp = float(e.spec.amp)
    Np = int(lib.tgp_padded_n(n))
    dX = torch.from_numpy(np.ascontiguousarray(as_xy(X))).to(e.dev)
    de = torch.from_numpy(y_err).to(e.dev) if with_yerr else None
    pe = C.c_void_p(de.data_ptr()) if with_yerr else None
    kc = e.spec.to_c()
    ctx = _ctx()
    single = torch.full((int(lib.tgp_panel_elems(Np)),), NAN, dtype=torch.float64, device=e.dev)
    e._lib.check(ctx, lib.tgp_d_kbuild_lower(ctx, C.byref(kc), C.c_void_p(dX.data_ptr()), n, pe, C.c_void_p(single.data_ptr())),
                 "tgp_d_kbuild_lower")
    torch.cuda.synchronize()
    one = unpack_share(single.cpu().numpy(), Np, 1, 0)
    bound = gauss_bound(ref, h) + np.where(ref < LD(amp) * LD(2.0 ** -1021) * (1 + LD(1e-9)), LD(amp) * LD(4.5e-308), LD(0.0))
    want_d = (LD(amp) + (y_err.astype(LD) ** 2 if with_yerr else LD(0.0))) * np.ones(n, dtype=LD)
    off_diag = ~np.eye(n, dtype=bool)

    def check(dense, stored, label):
        """`dense`: (Np, Np) with NaN where nothing is stored; `stored`: the same pattern from the index helpers"""
        assert np.array_equal(np.isnan(dense), np.isnan(stored)), "%s: other elements written than the layout says" % label
        m = ~np.isnan(stored[:n, :n]) & off_diag
        ratio = float((np.abs(dense[:n, :n].astype(LD) - ref)[m] / bound[m]).max()) if m.any() else 0.0
        assert ratio <= 1.0, "%s: a value is %.2f of its bound away from the reference" % (label, ratio)
        d = np.diag(dense)[:n]
        ok = ~np.isnan(d)
        assert (np.abs(d[ok].astype(LD) - want_d[ok]) <= 2 * U * want_d[ok]).all(), "%s: diagonal is not amp + yerr^2" % label
        pad = np.where(np.isnan(stored), NAN, np.eye(Np))
        assert np.array_equal(dense[n:, :], pad[n:, :], equal_nan=True) and np.array_equal(dense[:, n:], pad[:, n:], equal_nan=True), \
            "%s: padding is not the identity" % label
        return ratio

    r1 = check(one, unpack_share(pack_share(np.ones((Np, Np)), 1, 0), Np, 1, 0), "single-GPU build")
    worst, ndiff, ulps, total = 0.0, 0, 0, 0
    for g in range(G):
        o = _local_ops(n, G, g)
        e._lib.check(o.ctx, lib.tgp_dd_kbuild(o.ctx, C.byref(kc), C.c_void_p(dX.data_ptr()), n, pe, o._p(o.A), o._p(o.d_loff), G, g),
                     "tgp_dd_kbuild")
        got = _get(o)
        size = int(o.loff[-1])
        assert np.isnan(got[size:]).all(), "rank %d wrote behind its share" % g
        dense = unpack_share(got[:size], Np, G, g)
        worst = max(worst, check(dense, unpack_share(pack_share(np.ones((Np, Np)), G, g), Np, G, g), "rank %d of %d" % (g, G)))
        m = ~np.isnan(dense)
        total += int(m.sum())
        ne = m & (dense != one)
        ndiff += int(ne.sum())
        ne &= np.abs(one) > 1e-290                 # (below the clamp the two builds return different stand-ins)
        if ne.any():
            ulps = max(ulps, int(np.abs(dense[ne].view(np.int64) - one[ne].view(np.int64)).max()))
        _done(o)
    lib.tgp_reset_stream(ctx)
    assert total == Np * (Np + BLK) // 2 - (Np // BLK) * TB * TB                   # the ranks' shares tile the lower triangle
    print("kbuild G=%d n=%d yerr=%s: error / bound %.3f (single-GPU build %.3f); %d of %d elements differ from the single-GPU build, "
          "at most %d ulp above 1e-290" % (G, n, with_yerr, worst, r1, ndiff, total, ulps))


# ---- 2b: diagonal block -------------------------------------------------------------------------------------------------

def _diag_input(family, nB, k):
    """the 256 x 256 diagonal block of panel k after the panels before it (host fp64), symmetric"""
    Ap = _matrix(family, nB * BLK)
    M = partial_factor(Ap, k) if k else np.tril(Ap)
    return _sym(M[k * BLK:(k + 1) * BLK, k * BLK:(k + 1) * BLK])


def _check_diag_outputs(S, L, W0, W1, label, apriori=True):
    """`apriori` False (family (K)): finite outputs are asserted, the three figures are printed only -- the block's second half
    goes through W0, so the errors of L scale with cond(L_00), and the inverse is built column by column, so it is its right
    residual L W - I, not the left one measured here, that is free of the conditioning"""
    Lq = np.tril(L).astype(LD)
    assert np.isfinite(L[np.tril_indices(BLK)]).all() and np.isfinite(W0).all() and np.isfinite(W1).all(), label
    d = np.sqrt(np.abs(np.diag(S)))
    bwd = float((np.abs(S.astype(LD) - Lq @ Lq.T) / d[:, None] / d[None, :]).max())
    Lref = cholesky_ld(S)
    fwd = float(np.abs(Lq - Lref).max() / np.abs(Lref).max())
    ratios = []
    for W, sl in ((W0, slice(0, TB)), (W1, slice(TB, BLK))):
        Lb = Lq[sl, sl]
        E = np.abs(W.astype(LD) @ Lb - np.eye(TB, dtype=LD))
        B = np.abs(W).astype(LD) @ np.abs(Lb)
        ratios.append(float((E / np.maximum(B, 1e-300)).max()) / U)
        assert not apriori or (E <= 4 * TB * U * B).all(), (label, ratios)
    print("%s: backward %.3e / %.3e  forward %.3e / 1e-12  |WL - I| %.1f u, %.1f u / %d u" % (label, bwd, gamma(BLK + 1), fwd, ratios[0],
                                                                                           ratios[1], 4 * TB))
    assert not apriori or bwd <= gamma(BLK + 1), (label, bwd)
    assert not apriori or fwd <= 1e-12, (label, fwd)
    return bwd / gamma(BLK + 1), fwd / 1e-12, max(ratios) / (4 * TB)


@gpu
@pytest.mark.parametrize("family", ["W", "K"])     # (test_gpu_factor.py's a-priori bounds on L hold on (W) only: see its test 4)
@pytest.mark.parametrize("k", [0, 3])
def test_factor_diag_both_forms(k, family):
    """tgp_dd_factor_diag on the owner, G = 1, 15 blocks: panel 0 (14 blocks below) takes the throughput form, panel 3 (11) the
    latency form.  L_kk, W0, W1 against long double at test_gpu_factor.py's bounds, both copies (share + d_W, d_bcast) the same
    bytes, and a planted non-positive pivot at row r reports 256 k + r + 1 once.  The kernel family's block is held to what does
    not depend on its conditioning: finite outputs, the equal copies, the untouched surroundings and the pivot's index (its error
    figures are printed)."""
    e = _env()
    nB = 15
    o = _local_ops(nB * BLK, 1, 0)
    assert (panel_blocks(k + 1, nB, 0, 1) <= 12) == (k == 3)
    S = _diag_input(family, nB, k)
    at = share_slot(nB, 1, 0, k, k)

    def run(Sin):
        blk = Sin.copy()
        blk[:TB, TB:] = NAN
        o.A.fill_(NAN)
        o.W.fill_(NAN)
        o.bcast_full.fill_(NAN)
        o.A[at:at + BB].copy_(e.torch.from_numpy(blk.ravel()))
        o.factor_diag(k)
        e.torch.cuda.synchronize()
        return o.A.cpu().numpy(), o.W.cpu().numpy(), o.bcast_full.cpu().numpy()

    A, W, bc = run(S)
    Lblk = A[at:at + BB].reshape(BLK, BLK)
    assert np.isnan(Lblk[:TB, TB:]).all(), "the tile above the diagonal was written"
    w = W[2 * k * TB * TB:(2 * k + 2) * TB * TB]
    assert _same_bits(bc[:BB], A[at:at + BB]) and _same_bits(bc[BB:BCAST_ELEMS], w), "the broadcast copy differs from the kept one"
    assert np.isnan(bc[BCAST_ELEMS:]).all() and np.isnan(np.delete(W, np.s_[2 * k * TB * TB:(2 * k + 2) * TB * TB])).all()
    assert np.isnan(np.delete(A, np.s_[at:at + BB])).all(), "something outside the diagonal block was written"
    assert int(e.lib.tgp_dd_info(o.ctx_side, 1)) == 0
    _check_diag_outputs(S, Lblk, w[:TB * TB].reshape(TB, TB), w[TB * TB:].reshape(TB, TB), "factor_diag %s k=%d" % (family, k),
                        apriori=(family == "W"))
    Lref = cholesky_ld(S)
    for r in (5, 200):                       # first and second 128-block
        Sbad = S.copy()
        Sbad[r, r] -= 2.0 * float(Lref[r, r]) ** 2          # pivot r becomes -L_rr^2; the leading minors before it are untouched
        run(Sbad)
        assert int(e.lib.tgp_dd_info(o.ctx_side, 1)) == BLK * k + r + 1
        assert int(e.lib.tgp_dd_info(o.ctx_side, 1)) == 0
    _done(o)


# ---- 2c: panel solve ---------------------------------------------------------------------------------------------------------

def _trsm_bound(Arows, X, Lkk, W0, W1):
    """the docstring's bound on |X L_kk^T - A|, (rows, 256)"""
    L00, L10, L11 = np.abs(Lkk[:TB, :TB]), np.abs(Lkk[TB:, :TB]), np.abs(Lkk[TB:, TB:])
    M0 = np.abs(Arows[:, :TB])
    M1 = np.abs(Arows[:, TB:]) + np.abs(X[:, :TB]) @ L10.T
    c = 6 * (TB + 1) * U
    G0, G1 = np.abs(W0).T @ L00.T, np.abs(W1).T @ L11.T
    eta = 2 * BLK * ETA * (1.0 + max(G0.sum(axis=0).max(), G1.sum(axis=0).max()))        # products that underflow, carried through W
    return np.concatenate([gamma(TB + 1) * M0 + c * (M0 @ G0), gamma(TB + 1) * M1 + c * (M1 @ G1)], axis=1) + eta


def _check_trsm(G, g, nB, k, family):
    e = _env()
    Ap = _matrix(family, nB * BLK)
    M = partial_factor(Ap, k) if k else np.tril(Ap)            # panel k's column carries the panels before it
    s = slice(k * BLK, (k + 1) * BLK)
    Lkk = np.linalg.cholesky(_sym(M[s, s]))
    M = M.copy()
    M[s, s] = Lkk
    bc = _bcast_of(Lkk)
    o = _local_ops(nB * BLK, G, g)
    share = pack_share(_sym(M), G, g)
    _put(o, share)
    o.bcast_full[:BCAST_ELEMS].copy_(e.torch.from_numpy(bc))
    o.trsm(k)
    got = _get(o)
    W = o.W.cpu().numpy()
    w = W[2 * k * TB * TB:(2 * k + 2) * TB * TB]
    if owner(k, G) == g:
        assert np.isnan(W).all(), "the owner's d_W is written by tgp_dd_factor_diag, not by the solve"
    else:
        assert _same_bits(w, bc[BB:]), "a receiver's d_W must get the inverted blocks"
        assert np.isnan(np.delete(W, np.s_[2 * k * TB * TB:(2 * k + 2) * TB * TB])).all()
    below = own_blocks(nB, G, g, k + 1)
    touched = np.zeros(len(got), dtype=bool)
    worst = 0.0
    for b in below:
        at = share_slot(nB, G, g, k, b)
        touched[at:at + BB] = True
        X = got[at:at + BB].reshape(BLK, BLK)
        Ain = share[at:at + BB].reshape(BLK, BLK)
        assert np.isfinite(X).all()
        R = np.abs(X.astype(LD) @ Lkk.astype(LD).T - Ain.astype(LD))
        bound = _trsm_bound(Ain, X, Lkk, bc[BB:BB + TB * TB].reshape(TB, TB), bc[BB + TB * TB:].reshape(TB, TB))
        worst = max(worst, float((R / bound).max()))
        assert (R <= bound).all(), ("tgp_dd_trsm", G, g, k, b, worst)
        assert not np.array_equal(X, Ain)
    rest = ~touched
    assert _same_bits(got[:len(share)][rest[:len(share)]], share[rest[:len(share)]]), "rows outside panel %d's solve changed" % k
    assert np.isnan(got[len(share):]).all()
    _done(o)
    return worst


@gpu
@pytest.mark.parametrize("family", ["W", "K"])
@pytest.mark.parametrize("k", [0, 3])
def test_trsm_both_row_forms(k, family):
    """G = 1, 15 blocks: panel 0 has 28 row tiles below (128-row tiles), panel 3 has 22 (16-row slices)"""
    print("trsm %s k=%d: residual / bound %.3f" % (family, k, _check_trsm(1, 0, 15, k, family)))


@gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_trsm_owner_and_receivers_on_three_ranks(k):
    """G = 3, nB = 5 (blocks 0 | 1 4 | 2 3): over the panels 0, 1, 2 every rank is owner or receiver with zero, one or two blocks
    below"""
    counts = set()
    for g in range(3):
        counts.add((owner(k, 3) == g, panel_blocks(k + 1, 5, g, 3)))
        print("trsm G=3 g=%d k=%d: residual / bound %.3f" % (g, k, _check_trsm(3, g, 5, k, "W")))
    assert counts == {0: {(True, 0), (False, 2)}, 1: {(False, 0), (True, 1), (False, 2)}, 2: {(False, 0), (False, 1), (True, 1)}}[k]


# ---- 2d: trailing updates ---------------------------------------------------------------------------------------------------

# (G, g, nB, nseg, first panel of the group, family)
UPDATE_CASES = [
    (1, 0, 2, 1, 0, "W"), (1, 0, 3, 2, 0, "W"), (1, 0, 4, 3, 0, "K"), (1, 0, 5, 4, 0, "W"),      # one trailing block
    (1, 0, 5, 2, 0, "K"),                                                                     # world of one, three trailing blocks
    (3, 0, 9, 1, 0, "W"), (3, 1, 9, 3, 0, "W"), (3, 2, 9, 4, 0, "W"),                          # first, middle, last of three
    (8, 0, 9, 2, 0, "W"),                                                                     # a rank without rows below the group
    (8, 3, 9, 1, 1, "W"), (8, 7, 9, 3, 2, "K"),                                               # middle and last of eight
]


@functools.lru_cache(maxsize=4)
def _update_setup(G, g, nB, ns, k, family):
    """share before the group's update, the group's gathered panels, and per (row block, column block) the long-double result
    and the bound's magnitude"""
    Ap = _matrix(family, nB * BLK)
    M = partial_factor(Ap, k + ns, group_from=k)
    Ms = _sym(M)
    share = pack_share(Ms, G, g)
    gathered = [gather_panel(M, k + s, G) for s in range(ns)]
    refs = {}
    for bi in own_blocks(nB, G, g, k + ns):
        As = [M[bi * BLK:(bi + 1) * BLK, (k + s) * BLK:(k + s + 1) * BLK] for s in range(ns)]
        cols = slice((k + ns) * BLK, (bi + 1) * BLK)
        Cs = Ms[bi * BLK:(bi + 1) * BLK, cols]
        Bs = [M[cols, (k + s) * BLK:(k + s + 1) * BLK] for s in range(ns)]
        ref, mag = update_reference(Cs, As, Bs)
        for bj in range(k + ns, bi + 1):
            c = slice((bj - k - ns) * BLK, (bj - k - ns + 1) * BLK)
            refs[(bi, bj)] = (ref[:, c], mag[:, c])
    return share, gathered, refs


def _windows(nB, ns, k):
    ncol = 2 * (nB - k - ns)
    return [("whole", 0, -1), ("head", 0, 2 * ns), ("rest", 2 * ns, -1), ("empty", 1, 1), ("last column", ncol - 1, ncol)]


def _check_update(got, share, refs, G, g, nB, ns, k, lo, hi, label, moves=True):
    """elements of tile columns [lo, hi) (counted from block k + ns) against the reference at gamma(256 ns + 1); everything else
    keeps its bits.  Returns the largest error / bound."""
    ncol = 2 * (nB - k - ns)
    if hi < 0 or hi > ncol:
        hi = ncol
    expect_same = np.ones(len(share), dtype=bool)
    worst = 0.0
    for (bi, bj), (ref, mag) in refs.items():
        at = share_slot(nB, G, g, bj, bi)
        blk = got[at:at + BB].reshape(BLK, BLK)
        for half in (0, 1):
            if not lo <= 2 * (bj - k - ns) + half < hi:
                continue
            cs = slice(half * TB, (half + 1) * TB)
            rows = slice(TB, BLK) if (bi == bj and half == 1) else slice(0, BLK)         # (the tile above the diagonal is not stored)
            m = np.zeros((BLK, BLK), dtype=bool)
            m[rows, cs] = True
            expect_same[at:at + BB] &= ~m.ravel()
            err = np.abs(blk[rows, cs].astype(LD) - ref[rows, cs])
            bound = gamma(BLK * ns + 1) * mag[rows, cs] + (BLK * ns + 1) * ETA
            assert np.isfinite(blk[rows, cs]).all(), (label, bi, bj, half)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), "%s: block row %d, column %d.%d off by %.2f of the bound" % (label, bi, bj, half, worst)
            if moves:            # family (W): the update is far above round-off everywhere
                assert (blk[rows, cs] != share[at:at + BB].reshape(BLK, BLK)[rows, cs]).mean() > 0.99, (label, "tile not updated", bi, bj, half)
    n = len(share)
    bad = ~(got[:n].view(np.int64) == share.view(np.int64)) & expect_same
    assert not bad.any(), "%s: %d elements outside the window or the rank's rows changed (first at %d)" % (label, int(bad.sum()),
                                                                                                          int(np.argmax(bad)))
    assert np.isnan(got[n:]).all(), label
    return worst


def _device_bufs(o, gathered):
    return [o.to_device(P) for P, _ in gathered], [c for _, c in gathered]


@gpu
@pytest.mark.parametrize("G,g,nB,ns,k,family", UPDATE_CASES)
def test_update_entry_points_against_long_double(G, g, nB, ns, k, family):
    """tgp_dd_update (nseg 1), tgp_dd_update2 (nseg 2) and tgp_dd_update_group on one rank's share with the gathered panels of a
    host partial factorisation, five column windows each"""
    share, gathered, refs = _update_setup(G, g, nB, ns, k, family)
    o = _local_ops(nB * BLK, G, g)
    bufs, cm = _device_bufs(o, gathered)
    forms = [("update_group", lambda lo, hi: o.update_group(k, bufs, cm, lo, hi))]
    if ns == 1:
        forms.append(("update", lambda lo, hi: o.update(k, bufs[0], cm[0], lo, hi)))
    if ns == 2:
        forms.append(("update2", lambda lo, hi: o.update2(k, bufs[0], cm[0], bufs[1], cm[1], lo, hi)))
    worst = 0.0
    for name, call in forms:
        for wname, lo, hi in _windows(nB, ns, k):
            _put(o, share)
            call(lo, hi)
            label = "%s G=%d g=%d nB=%d nseg=%d k=%d %s" % (name, G, g, nB, ns, k, wname)
            worst = max(worst, _check_update(_get(o), share, refs, G, g, nB, ns, k, lo, hi, label, moves=(family == "W")))
    print("update G=%d g=%d nB=%d nseg=%d k=%d %s: %d tiles, error / bound %.3f" % (G, g, nB, ns, k, family, 2 * len(refs), worst))
    assert refs or panel_blocks(k + ns, nB, g, G) == 0
    _done(o)


QF_CASE = (3, 2, 9, 2, 0, "W")          # rows 2, 5, 8: block 8 puts the last tile column into every window that ends there


@gpu
@pytest.mark.parametrize("nres", [1, 2, 3])
def test_queued_update_against_long_double(nres):
    """tgp_dd_update_group_queued, the persistent grid that keeps 1, 2 or 3 compute units per shader engine clear"""
    G, g, nB, ns, k, family = QF_CASE
    share, gathered, refs = _update_setup(*QF_CASE)
    o = _local_ops(nB * BLK, G, g)
    bufs, cm = _device_bufs(o, gathered)
    for wname, lo, hi in (("whole", 0, -1), ("rest", 2 * ns, -1)):
        _put(o, share)
        o.queue_reset()
        o.update_group(k, bufs, cm, lo, hi, queue_nres=nres)
        worst = _check_update(_get(o), share, refs, G, g, nB, ns, k, lo, hi, "queued nres=%d %s" % (nres, wname))
        print("queued nres=%d %s: error / bound %.3f" % (nres, wname, worst))
    _done(o)


@gpu
@pytest.mark.parametrize("nres", [0, 2])
def test_fused_update_against_long_double(nres):
    """tgp_dd_update_group_fused (head columns first, flag from inside), plain and as the persistent grid"""
    e = _env()
    G, g, nB, ns, k, family = QF_CASE
    share, gathered, refs = _update_setup(*QF_CASE)
    o = _local_ops(nB * BLK, G, g)
    if e.lib.tgp_handoff_mode(o.ctx) != 1:
        pytest.skip("hand-offs by events on this box")
    bufs, cm = _device_bufs(o, gathered)
    _put(o, share)
    o.queue_reset()
    o.update_group_fused(k, bufs, cm, 2 * ns, queue_nres=nres)
    o.side_wait_head()
    worst = _check_update(_get(o), share, refs, G, g, nB, ns, k, 0, -1, "fused nres=%d" % nres)
    print("fused nres=%d: error / bound %.3f" % (nres, worst))
    _done(o)


# ---- 2e: left-looking strip -----------------------------------------------------------------------------------------------

# (G, g, nB, kgroup, j): block b = kgroup + j against the panels kgroup .. b - 1
STRIP_CASES = [
    (1, 0, 4, 0, 3),          # b the last block, the owner, depth 768
    (1, 0, 5, 1, 1),          # kgroup > 0, rows 2 3 4
    (2, 0, 6, 2, 2),          # owner of b = 4 (rows: 4)
    (2, 1, 6, 2, 2),          # receiver (rows: 5)
    (3, 0, 9, 0, 3),          # receiver, rows 5 6
    (3, 2, 9, 0, 3),          # owner of b = 3, rows 3 8
    (3, 1, 9, 4, 1),          # receiver, kgroup > 0, rows 7
    (8, 7, 9, 0, 2),          # receiver whose first row block (7) is five blocks below b = 2
    (8, 2, 9, 0, 2),          # owner with its diagonal block alone
    (8, 7, 9, 5, 3),          # b = 8 the last block, owner, kgroup > 0
    (8, 0, 9, 1, 1),          # a rank without rows
]


@gpu
@pytest.mark.parametrize("G,g,nB,kgroup,j", STRIP_CASES)
def test_strip_left_against_long_double_and_the_right_looking_strips(G, g, nB, kgroup, j):
    """tgp_dd_strip_left: this rank's rows (blocks >= b) of block b's two tile columns against the j earlier panels of the group
    in one pass of depth 256 j; the column operand from d_ext on a receiver, from the rank's own rows on the owner.  The bits are
    those of the right-looking strips (tgp_dd_update_group panel by panel on block b's window)."""
    e = _env()
    b = kgroup + j
    Ap = _matrix("W", nB * BLK, seed=2)
    M = partial_factor(Ap, b, group_from=kgroup, stop_cols=b)          # block b's columns lack the panels kgroup .. b - 1
    share = pack_share(_sym(M), G, g)
    is_owner = owner(b, G) == g
    rows = own_blocks(nB, G, g, b)
    assert is_owner == (b in rows)
    o = _local_ops(nB * BLK, G, g)
    _put(o, share)
    ext = np.concatenate([M[b * BLK:(b + 1) * BLK, (kgroup + s) * BLK:(kgroup + s + 1) * BLK].ravel() for s in range(j)])
    if not is_owner:
        o.bcast_full[BCAST_ELEMS:BCAST_ELEMS + j * BB].copy_(e.torch.from_numpy(ext))
    o.strip_left(b, kgroup, not is_owner)
    got = _get(o)
    expect_same = np.ones(len(share), dtype=bool)
    worst = 0.0
    Bs = [M[b * BLK:(b + 1) * BLK, (kgroup + s) * BLK:(kgroup + s + 1) * BLK] for s in range(j)]
    for bi in rows:
        at = share_slot(nB, G, g, b, bi)
        As = [M[bi * BLK:(bi + 1) * BLK, (kgroup + s) * BLK:(kgroup + s + 1) * BLK] for s in range(j)]
        Cin = share[at:at + BB].reshape(BLK, BLK)
        ref, mag = update_reference(np.nan_to_num(Cin, nan=0.0), As, Bs)
        m = np.ones((BLK, BLK), dtype=bool)
        if bi == b:
            m[:TB, TB:] = False
        expect_same[at:at + BB] = ~m.ravel()
        blk = got[at:at + BB].reshape(BLK, BLK)
        assert np.isfinite(blk[m]).all()
        err = np.abs(blk.astype(LD) - ref)[m]
        bound = (gamma(BLK * j + 1) * mag)[m] + (BLK * j + 1) * ETA
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), ("tgp_dd_strip_left", G, g, b, bi, worst)
        assert (blk[m] != Cin[m]).mean() > 0.99
    n = len(share)
    bad = ~(got[:n].view(np.int64) == share.view(np.int64)) & expect_same
    assert not bad.any(), "%d elements outside block %d's columns or the rank's rows changed" % (int(bad.sum()), b)
    assert np.isnan(got[n:]).all()
    # the right-looking strips: panel m against block b's two tile columns, one launch per panel
    _put(o, share)
    for m_ in range(kgroup, b):
        P, c = gather_panel(M, m_, G)
        lo = 2 * (b - m_ - 1)
        o.update_group(m_, [o.to_device(P)], [c], lo, lo + 2)
    right = _get(o)
    assert _same_bits(right, got), "left-looking strip and right-looking strips differ in %d elements" % int(
        (right.view(np.int64) != got.view(np.int64)).sum())
    print("strip_left G=%d g=%d nB=%d kgroup=%d j=%d: %d row blocks, error / bound %.3f" % (G, g, nB, kgroup, j, len(rows), worst))
    _done(o)


# ---- 2f: copies ------------------------------------------------------------------------------------------------------------

def _labelled(Np, seed):
    """a dense matrix whose every element is different (so a misplaced copy cannot go unnoticed)"""
    rng = np.random.default_rng(seed)
    return rng.permutation(Np * Np).astype(np.float64).reshape(Np, Np) + 0.5


@gpu
@pytest.mark.parametrize("G", [1, 3, 8])
def test_keep_panel_is_the_index_helpers_copy(G):
    """tgp_dd_keep_panel: the diagonal block from d_bcast and / or the rows below from the gathered panel into the replicated
    packed factor, k in {0, 1, nB - 1}; either operand NULL; nothing else written"""
    e = _env()
    torch, lib = e.torch, e.lib
    nB = 5
    Np = nB * BLK
    R = _labelled(Np, G)
    want_all = pack_single(R, poison=False)
    poff = packed_offsets(Np)
    ctx = _ctx()
    full = torch.empty(len(want_all), dtype=torch.float64, device=e.dev)
    for k in (0, 1, nB - 1):
        P, cmax = gather_panel(R, k, G)
        dP = torch.from_numpy(P).to(e.dev)
        bc = torch.from_numpy(np.concatenate([R[k * BLK:(k + 1) * BLK, k * BLK:(k + 1) * BLK].ravel(), np.full(2 * TB * TB, NAN)])).to(e.dev)
        for use_b, use_g in ((True, False), (False, True), (True, True)):
            full.fill_(NAN)
            e._lib.check(ctx, lib.tgp_dd_keep_panel(ctx, C.c_void_p(full.data_ptr()), Np, k, G, C.c_void_p(bc.data_ptr()) if use_b else None,
                                                    C.c_void_p(dP.data_ptr()) if use_g else None, cmax), "tgp_dd_keep_panel")
            torch.cuda.synchronize()
            got = full.cpu().numpy()
            want = np.full(len(want_all), NAN)
            if use_b:
                want[poff[k]:poff[k] + BB] = want_all[poff[k]:poff[k] + BB]
            if use_g:
                want[poff[k] + BB:poff[k + 1]] = want_all[poff[k] + BB:poff[k + 1]]
            assert _same_bits(got, want), (G, k, use_b, use_g, int((got.view(np.int64) != want.view(np.int64)).sum()))
    e.lib.tgp_reset_stream(ctx)


@gpu
@pytest.mark.parametrize("G", [1, 3, 8])
def test_tail_assemble_and_scatter_are_the_index_helpers_copies(G):
    """tgp_dd_tail_assemble ([G][stride] shares from panel k0 on -> the packed matrix of order Np - 256 k0) and tgp_dd_tail_scatter
    (back into one rank's share), k0 in {0, 1, nB - 1}: tails of 5, 4 and 1 blocks, no multiples of 3 or 8"""
    e = _env()
    torch, lib = e.torch, e.lib
    nB = 5
    Np = nB * BLK
    R = _labelled(Np, 10 + G)
    shares = [pack_share(R, G, r, poison=False) for r in range(G)]
    offs = [share_offsets(nB, G, r) for r in range(G)]
    ctx = _ctx()
    for k0 in (0, 1, nB - 1):
        m = Np - BLK * k0
        stride = max(int(offs[r][-1] - offs[r][k0]) for r in range(G))
        gathered = np.full(G * stride, NAN)
        for r in range(G):
            t = shares[r][int(offs[r][k0]):]
            gathered[r * stride:r * stride + len(t)] = t
        want = pack_single(R[k0 * BLK:, k0 * BLK:], poison=False)
        dG = torch.from_numpy(gathered).to(e.dev)
        tail = torch.full((len(want) + BB,), NAN, dtype=torch.float64, device=e.dev)
        e._lib.check(ctx, lib.tgp_dd_tail_assemble(ctx, C.c_void_p(dG.data_ptr()), stride, Np, k0, G, C.c_void_p(tail.data_ptr())),
                     "tgp_dd_tail_assemble")
        torch.cuda.synchronize()
        got = tail.cpu().numpy()
        assert len(want) == int(lib.tgp_panel_elems(m))
        assert _same_bits(got[:len(want)], want), (G, k0, int((got[:len(want)].view(np.int64) != want.view(np.int64)).sum()))
        assert np.isnan(got[len(want):]).all(), (G, k0, "written behind the packed tail")
        for g in range(G):
            o = _local_ops(Np, G, g)
            other = -shares[g] - 1.0                                            # what must survive in front of panel k0
            _put(o, other)
            e._lib.check(o.ctx, lib.tgp_dd_tail_scatter(o.ctx, C.c_void_p(tail.data_ptr()), Np, k0, G, g, o._p(o.A), o._p(o.d_loff)),
                         "tgp_dd_tail_scatter")
            back = _get(o)
            cut = int(offs[g][k0])
            assert _same_bits(back[:cut], other[:cut]), (G, g, k0, "front of the share changed")
            assert _same_bits(back[cut:len(other)], shares[g][cut:]), (G, g, k0)
            assert np.isnan(back[len(other):]).all()
            _done(o)
    e.lib.tgp_reset_stream(ctx)


# ---- 2g: the sweeps' pieces and the log-determinant ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference_factor(nB):
    """fp64 factor of family (W) (padded dense, lower) and the inverted 128-blocks of its diagonal, as d_W holds them"""
    L = np.linalg.cholesky(_matrix("W", nB * BLK, seed=3))
    W = np.concatenate([_inverse_ld(L[i * TB:(i + 1) * TB, i * TB:(i + 1) * TB]).ravel() for i in range(2 * nB)])
    return L, W


@gpu
@pytest.mark.parametrize("G", [1, 3])
def test_sweep_pieces_one_block_step_each(G):
    """tgp_dd_fwd_diag / fwd_update / bwd_partial / bwd_diag (with and without d_s) for every panel of nB = 5 on every rank: owners'
    diagonal steps, ranks with one or several blocks below and with none"""
    e = _env()
    torch = e.torch
    nB = 5
    Np = nB * BLK
    L, W = _reference_factor(nB)
    rng = np.random.default_rng(7 + G)
    worst = dict(fwd_diag=0.0, fwd_update=0.0, bwd_partial=0.0, bwd_diag=0.0, bwd_diag_s=0.0)
    subst = dict(fwd_diag=0.0, bwd_diag=0.0, bwd_diag_s=0.0)         # the same residuals over gamma(257) |L_kk||x|: printed, not asserted
    none_below = 0
    for g in range(G):
        o = _local_ops(Np, G, g)
        _put(o, pack_share(_sym(L), G, g))
        o.W.copy_(torch.from_numpy(W))
        mine = own_blocks(nB, G, g)
        for kb in range(nB):
            s = slice(kb * BLK, (kb + 1) * BLK)
            Lkk = L[s, s]
            Ld = np.abs(Lkk).copy()
            Ld[TB:, :TB] = 0.0
            Wd = np.zeros((BLK, BLK))
            Wd[:TB, :TB] = np.abs(W[2 * kb * TB * TB:(2 * kb + 1) * TB * TB].reshape(TB, TB))
            Wd[TB:, TB:] = np.abs(W[(2 * kb + 1) * TB * TB:(2 * kb + 2) * TB * TB].reshape(TB, TB))
            L10 = np.zeros((BLK, BLK))
            L10[TB:, :TB] = np.abs(Lkk[TB:, :TB])
            if owner(kb, G) == g:
                y = rng.standard_normal(BLK)
                d = o.to_device(y)
                o.fwd_diag(kb, d)
                torch.cuda.synchronize()
                x = d.cpu().numpy()
                r = np.abs(Lkk.astype(LD) @ x.astype(LD) - y.astype(LD))
                bound = gamma(260) * (Ld @ (Wd @ (np.abs(y) + L10 @ np.abs(x))))
                worst["fwd_diag"] = max(worst["fwd_diag"], float((r / bound).max()))
                subst["fwd_diag"] = max(subst["fwd_diag"], float((r / (gamma(BLK + 1) * (np.abs(Lkk) @ np.abs(x)))).max()))
                assert (r <= bound).all(), ("fwd_diag", G, g, kb)
                for with_s in (False, True):
                    a, sv = rng.standard_normal(BLK), rng.standard_normal(BLK)
                    d = o.to_device(a)
                    ds = o.to_device(sv) if with_s else None
                    o.bwd_diag(kb, d, ds)
                    torch.cuda.synchronize()
                    x = d.cpu().numpy()
                    rhs = a.astype(LD) - (sv.astype(LD) if with_s else 0)
                    r = np.abs(Lkk.astype(LD).T @ x.astype(LD) - rhs)
                    t = np.abs(a) + (np.abs(sv) if with_s else 0) + L10.T @ np.abs(x)
                    bound = gamma(260) * (Ld.T @ (Wd.T @ t))
                    key = "bwd_diag_s" if with_s else "bwd_diag"
                    worst[key] = max(worst[key], float((r / bound).max()))
                    subst[key] = max(subst[key], float((r / (gamma(BLK + 1) * (np.abs(Lkk).T @ np.abs(x)))).max()))
                    assert (r <= bound).all(), (key, G, g, kb)
            below = [b for b in mine if b > kb]
            none_below += not below
            rowsL = np.concatenate([L[b * BLK:(b + 1) * BLK, s] for b in below]) if below else np.zeros((0, BLK))
            z = rng.standard_normal(BLK)
            yloc = rng.standard_normal(max(len(mine), 1) * BLK)
            dz, dy = o.to_device(z), o.to_device(yloc)
            o.fwd_update(kb, dz, dy)
            torch.cuda.synchronize()
            got = dy.cpu().numpy()
            lb0 = len(mine) - len(below)
            assert _same_bits(got[:lb0 * BLK], yloc[:lb0 * BLK]), "fwd_update touched rows that are not below the panel"
            if below:
                yin = yloc[lb0 * BLK:len(mine) * BLK]
                ref = yin.astype(LD) - rowsL.astype(LD) @ z.astype(LD)
                bound = gamma(BLK + 1) * (np.abs(yin) + np.abs(rowsL) @ np.abs(z))
                err = np.abs(got[lb0 * BLK:len(mine) * BLK].astype(LD) - ref)
                worst["fwd_update"] = max(worst["fwd_update"], float((err / bound).max()))
                assert (err <= bound).all(), ("fwd_update", G, g, kb)
            aloc = rng.standard_normal(max(len(mine), 1) * BLK)
            da, dsum = o.to_device(aloc), o.to_device(np.full(BLK, NAN))
            o.bwd_partial(kb, da, dsum)
            torch.cuda.synchronize()
            got = dsum.cpu().numpy()
            if below:
                av = aloc[lb0 * BLK:len(mine) * BLK]
                ref = rowsL.astype(LD).T @ av.astype(LD)
                bound = gamma(len(av) + 1) * (np.abs(rowsL).T @ np.abs(av))
                err = np.abs(got.astype(LD) - ref)
                worst["bwd_partial"] = max(worst["bwd_partial"], float((err / bound).max()))
                assert (err <= bound).all(), ("bwd_partial", G, g, kb)
            else:
                assert np.array_equal(got, np.zeros(BLK)), "a rank without rows below contributes exactly 0"
        _done(o)
    assert none_below > 0
    print("sweeps G=%d: error / bound %s; diagonal steps over gamma(257) |L_kk||x|: %s"
          % (G, ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), ", ".join("%s %.3f" % kv for kv in sorted(subst.items()))))


@gpu
@pytest.mark.parametrize("G", [1, 3])
def test_logdet_local_counts_data_rows_only(G):
    """tgp_dd_logdet_local for n = Np, Np - 1, Np - 255: padding rows (their diagonal set to 7 here) do not count, and the ranks'
    shares add up to 2 sum log diag"""
    e = _env()
    nB = 5
    Np = nB * BLK
    L, _ = _reference_factor(nB)
    for n in (Np, Np - 1, Np - 255):
        Ln = L.copy()
        Ln[np.arange(n, Np), np.arange(n, Np)] = 7.0
        total, total_bound = LD(0.0), 0.0
        for g in range(G):
            o = _local_ops(n, G, g)
            assert o.Np == Np
            _put(o, pack_share(_sym(Ln), G, g))
            out = o.to_device(np.full(1, NAN))
            o.logdet_local(out)
            e.torch.cuda.synchronize()
            rows = [b * BLK + r for b in own_blocks(nB, G, g) for r in range(BLK) if b * BLK + r < n]
            terms = 2.0 * np.log(np.diag(L)[rows].astype(LD))
            bound = (gamma(max(len(rows), 1)) + 4 * U) * float(np.abs(terms).sum())
            got = float(out[0])
            assert abs(LD(got) - terms.sum()) <= bound, (G, g, n, got, float(terms.sum()), bound)
            total += LD(got)
            total_bound += bound
            _done(o)
        want = 2.0 * np.log(np.diag(L)[:n].astype(LD)).sum()
        assert abs(total - want) <= total_bound, (G, n)


# ---- 3: the whole distributed factor, twice ---------------------------------------------------------------------------------

TWICE = [
    # (G, n, environment)
    (8, 6000, dict(TGP_DIST_GROUP="4", TGP_DIST_QUEUE="0", TGP_DIST_FUSED="0")),                  # recorded: split_update_with_events
    (4, 7000, dict(TGP_DIST_GROUP="4", TGP_DIST_FINISH="9", TGP_DIST_REPLICATE="0")),            # recorded: replicated_finish
    (4, 1100, dict(TGP_DIST_GROUP="2")),                                                         # the default form
    (3, 2300, dict(TGP_DIST_GROUP="3", TGP_DIST_FINISH="4", TGP_DIST_CHAIN_BCAST="1")),          # panel exchange off the chain
]


def _capture_run(G, n):
    """one virtual-rank factorisation and solve (test_gpu_dist._run_virtual_ranks, its own assertions included); per rank a
    clone of the share, of d_W, of the replicated factor where there is one, alpha and the log-determinant"""
    from test_gpu_dist import _run_virtual_ranks
    kept = [None] * G

    def capture(rank, gp):
        o = gp.ops
        kept[rank] = dict(share=o.A[:int(o.loff[-1])].cpu().numpy(), W=o.W.cpu().numpy(),
                          full=None if (o.Afull is None or not o.keep_copies) else o.Afull.cpu().numpy(),
                          alpha=gp.alpha.cpu().numpy(), logdet=gp.logdet.cpu().numpy(), Np=o.Np)
    _run_virtual_ranks(G, n, capture=capture)
    return kept


def compare_runs(one, two, G):
    """bit equality of everything two runs captured; the message names the rank, the first panel and block, and the counts"""
    problems = []
    for r in range(G):
        a, b = one[r], two[r]
        Np = a["Np"]
        d = first_difference(a["share"], b["share"], Np, G, r, written_only=True)
        if d is not None:
            problems.append("rank %d share: first at panel %d block %d (%d elements there, %d in all)" % ((r,) + d))
        if not _same_bits(a["W"], b["W"]):
            ne = a["W"].view(np.int64) != b["W"].view(np.int64)
            problems.append("rank %d d_W: first at 128-block %d of panel %d (%d elements in all)" % (
                r, int(np.argmax(ne)) // (TB * TB), int(np.argmax(ne)) // (2 * TB * TB), int(ne.sum())))
        d = None if a["full"] is None else first_difference(a["full"], b["full"], Np, 1, 0, written_only=True)
        if d is not None:
            problems.append("rank %d replicated factor: first at panel %d block %d (%d elements there, %d in all)" % ((r,) + d))
        for key in ("alpha", "logdet"):
            if not _same_bits(a[key], b[key]):
                problems.append("rank %d %s: %d elements differ between the runs" % (r, key, int((a[key].view(np.int64) != b[key].view(np.int64)).sum())))
            if not _same_bits(a[key], one[0][key]):
                problems.append("rank %d %s differs from rank 0's in the same run" % (r, key))
    return problems


@gpu
@pytest.mark.parametrize("G,n,env", TWICE, ids=["G%d-n%d-%s" % (G, n, "-".join("%s=%s" % (k[9:], v) for k, v in sorted(e_.items())))
                                                 for G, n, e_ in TWICE])
def test_distributed_factor_twice_bit_for_bit(G, n, env, monkeypatch):
    """Two virtual-rank factorisations and solves of the same problem under the same settings leave the same bytes in every
    rank's share and replicated factor (the never-written tile above each diagonal block's diagonal left out: it holds what the
    allocation held), d_W, alpha and log-determinant (no arithmetic of the factorisation depends on timing), and
    alpha and the log-determinant are the same on every rank.  The shares, mapped back to dense, are a Cholesky factor of the
    kernel matrix at test_gpu_factor.py's normwise bound for kernel matrices: ||K - L L^T||_F / ||K||_F <= max(16 x rocSOLVER's on
    the same matrix, n u)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = _env()
    torch = e.torch
    one = _capture_run(G, n)
    two = _capture_run(G, n)
    problems = compare_runs(one, two, G)
    assert not problems, "\n".join(problems)
    Np = one[0]["Np"]
    L = torch.from_numpy(shares_to_dense_lower([one[r]["share"] for r in range(G)], Np, G)).to(e.dev)
    assert bool(torch.isfinite(L).all())
    from test_gpu_dist import _problem
    spec, X, y, y_err, _ = _problem(n, 777, seed=G)
    tX = torch.from_numpy(X).to(e.dev)
    d0 = tX[:, None, 0] - tX[None, :, 0]
    d1 = tX[:, None, 1] - tX[None, :, 1]
    K = torch.eye(Np, dtype=torch.float64, device=e.dev)
    K[:n, :n] = spec.amp * torch.exp(-0.5 * (spec.a * d0 * d0 + 2.0 * spec.b * d0 * d1 + spec.c * d1 * d1))
    K.diagonal()[:n] = spec.amp + torch.from_numpy(y_err ** 2).to(e.dev)
    del d0, d1
    nK = float(torch.linalg.norm(K))
    ours = float(torch.linalg.norm(K - L @ L.T)) / nK
    Lref, info = torch.linalg.cholesky_ex(K)
    assert int(info) == 0
    ref = float(torch.linalg.norm(K - Lref @ Lref.T)) / nK
    print("G=%d n=%d: ||K - LL^T||_F / ||K||_F = %.3e, rocSOLVER %.3e" % (G, n, ours, ref))
    assert ours <= max(16.0 * ref, n * U), (ours, ref)
    if one[0]["full"] is not None:                       # the replicated factor is the same factor in the single-GPU layout
        full = shares_to_dense_lower([one[0]["full"]], Np, 1)
        assert np.array_equal(full, L.cpu().numpy()), "rank 0's replicated factor is not the ranks' shares"

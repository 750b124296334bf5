"""Dense NumPy references of one rank's share of the distributed Cholesky (layout of include/tgp.h, "multi-GPU tier").

Index helpers: a dense symmetric (Np, Np) matrix <-> what rank g of G stores (`pack_share` / `unpack_share`), the all-gathered
panel [rank][cmax][256][256] (`gather_panel`), the share's tail from panel k0 on (`tail_blocks`).  They are built on the index
functions of treegp_amd/dist.py only (owner, block_of, panel_blocks, panel_cmax, gathered_index) and are checked without a
GPU in tests/test_gpu_dist_blocks.py (its first test carries no gpu marker).  Arithmetic references form every product in np.longdouble (64-bit mantissa: a reference
then carries 2^-11 of an fp64 rounding of its own); the |.| sums that only scale a bound are fp64."""
import numpy as np

from treegp_amd.dist import BLK, block_of, gathered_index, owner, panel_blocks, panel_cmax

LD = np.longdouble
U = 2.0 ** -53                  # unit round-off of fp64
TB = 128                        # diagonal sub-block
BB = BLK * BLK


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- index helpers ----------------------------------------------------------------------------------------------------

def own_blocks(nB, G, g, first=0):
    """rank g's blocks first <= b < nB, ascending"""
    return [block_of(q, g, G) for q in range(panel_blocks(0, nB, g, G)) if block_of(q, g, G) >= first]


def share_offsets(nB, G, g):
    """element offset of every panel's part of rank g's share (nB + 1 entries; tgp_dist_panel_off)"""
    off = np.zeros(nB + 1, dtype=np.int64)
    for p in range(nB):
        off[p + 1] = off[p] + panel_blocks(p, nB, g, G) * BB
    return off


def share_slot(nB, G, g, p, b):
    """element offset of block b's rows of panel p (b >= p, owner(b) == g) inside rank g's share"""
    assert owner(b, G) == g and p <= b < nB
    return int(share_offsets(nB, G, g)[p]) + own_blocks(nB, G, g, p).index(b) * BB


def padded_dense(A, n):
    """(n, n) -> (Np, Np) with identity padding, as the library pads"""
    Np = -(-n // BLK) * BLK
    Ap = np.eye(Np, dtype=A.dtype)
    Ap[:n, :n] = A
    return Ap


def pack_share(Ap, G, g, poison=True):
    """dense (Np, Np) -> rank g's share: panel after panel, inside a panel the rank's blocks b >= p in ascending order, each the
    256 x 256 rows of block b in columns 256 p .. 256 p + 255 (row-major).  `poison`: the tile above the diagonal in a diagonal
    block's first 128 rows (never written by the K build) is NaN."""
    nB = Ap.shape[0] // BLK
    off = share_offsets(nB, G, g)
    out = np.empty(int(off[-1]), dtype=np.float64)
    for p in range(nB):
        for i, b in enumerate(own_blocks(nB, G, g, p)):
            blk = np.array(Ap[b * BLK:(b + 1) * BLK, p * BLK:(p + 1) * BLK], dtype=np.float64)
            if b == p and poison:
                blk[:TB, TB:] = np.nan
            out[int(off[p]) + i * BB:int(off[p]) + (i + 1) * BB] = blk.ravel()
    return out


def unpack_share(share, Np, G, g, out=None):
    """rank g's share -> dense (Np, Np): its blocks' lower part filled in (a diagonal block's upper tile as stored), everything
    else as in `out` (default NaN)"""
    nB = Np // BLK
    off = share_offsets(nB, G, g)
    D = np.full((Np, Np), np.nan) if out is None else out
    for p in range(nB):
        for i, b in enumerate(own_blocks(nB, G, g, p)):
            o = int(off[p]) + i * BB
            D[b * BLK:(b + 1) * BLK, p * BLK:(p + 1) * BLK] = np.asarray(share[o:o + BB]).reshape(BLK, BLK)
    return D


def shares_to_dense_lower(shares, Np, G):
    """every rank's share -> the dense lower triangle (upper part zero)"""
    D = np.zeros((Np, Np))
    for g in range(G):
        unpack_share(shares[g], Np, G, g, out=D)
    return np.tril(D)


def gather_panel(Ap, k, G, poison=True):
    """the all-gathered panel k as every rank receives it: [rank][cmax][256][256] with rank r's blocks > k in ascending order;
    slots beyond a rank's count are NaN (`poison`) or 0.  Returns (flat array of max(G cmax, 1) blocks, cmax)."""
    nB = Ap.shape[0] // BLK
    cmax = panel_cmax(k + 1, nB, G)
    P = np.full(max(G * cmax, 1) * BB, np.nan if poison else 0.0)
    for b in range(k + 1, nB):
        r, idx = gathered_index(b, k + 1, G)
        o = (r * cmax + idx) * BB
        P[o:o + BB] = np.asarray(Ap[b * BLK:(b + 1) * BLK, k * BLK:(k + 1) * BLK], dtype=np.float64).ravel()
    return P, cmax


def tail_blocks(k0, nB, G, r):
    """(panel, block) pairs of rank r's share from panel k0 on, in storage order"""
    return [(p, b) for p in range(k0, nB) for b in own_blocks(nB, G, r, p)]


def packed_offsets(Np):
    """single-GPU packed layout: element offset of panel p (rows 256 p .. Np - 1 of columns 256 p .. + 255)"""
    nB = Np // BLK
    off = np.zeros(nB + 1, dtype=np.int64)
    for p in range(nB):
        off[p + 1] = off[p] + (Np - BLK * p) * BLK
    return off


def pack_single(Ap, poison=True):
    """dense -> the single-GPU packed panels (= the share of a world of one)"""
    return pack_share(Ap, 1, 0, poison)


def written_mask(nB, G, g):
    """True for every element of rank g's share that the K build writes: all but the tile above the diagonal in the first 128
    rows of each of its diagonal blocks (that tile is never written and never read: it holds whatever the allocation held)"""
    off = share_offsets(nB, G, g)
    m = np.ones(int(off[-1]), dtype=bool)
    for b in own_blocks(nB, G, g):
        blk = m[int(off[b]):int(off[b]) + BB].reshape(BLK, BLK)       # a rank's diagonal block is the first of its panel
        blk[:TB, TB:] = False
    return m


def first_difference(a, b, Np, G, g, written_only=False):
    """where two copies of rank g's share differ in bits: (panel, block, count in that block, total count), or None.
    `written_only`: the never-written tiles (written_mask) are left out"""
    a, b = np.asarray(a), np.asarray(b)
    nB = Np // BLK
    off = share_offsets(nB, G, g)
    ne = a.view(np.int64)[:int(off[-1])] != b.view(np.int64)[:int(off[-1])]
    if written_only:
        ne &= written_mask(nB, G, g)
    if not ne.any():
        return None
    at = int(np.argmax(ne))
    p = int(np.searchsorted(off, at, side="right")) - 1
    i = (at - int(off[p])) // BB
    blk = own_blocks(nB, G, g, p)[i]
    return p, blk, int(ne[int(off[p]) + i * BB:int(off[p]) + (i + 1) * BB].sum()), int(ne.sum())


# ---- test matrices ------------------------------------------------------------------------------------------------------

def family_w(n, seed):
    """A = G G^T / n + I, exactly symmetric; eigenvalues in [1, 5]: every panel's update moves every trailing entry by far
    more than round-off"""
    rng = np.random.default_rng(seed)
    Gm = rng.standard_normal((n, n))
    A = Gm @ Gm.T
    A = (A + A.T) * (0.5 / n)
    A[np.diag_indices(n)] += 1.0
    return A


def family_k(n, seed=0):
    """the star-field kernel matrix with the headline kernel and y_err^2 on the diagonal (NumPy fp64), and the solve's inputs"""
    from treegp_amd.synthetic import star_field, headline_invlam
    X, y, y_err, _ = star_field(n, 16, seed=seed)
    iL = headline_invlam()
    a, b, c = iL[0, 0], iL[0, 1], iL[1, 1]
    d0 = X[:, None, 0] - X[None, :, 0]
    d1 = X[:, None, 1] - X[None, :, 1]
    K = np.exp(-0.5 * (a * d0 * d0 + 2.0 * b * d0 * d1 + c * d1 * d1))
    K[np.diag_indices(n)] = 1.0 + y_err ** 2
    return K, X, y - y.mean(), y_err


# ---- arithmetic references ----------------------------------------------------------------------------------------------

def cholesky_ld(S):
    """lower Cholesky factor of a small symmetric matrix in long double (column by column)"""
    S = np.array(S, dtype=LD)
    n = S.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = S[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def partial_factor(Ap, upto, group_from=None, stop_cols=None):
    """fp64 right-looking block factorisation of the dense Ap: panels 0 .. upto - 1 are factored (diagonal block and the rows
    below).  Panels p < group_from update everything right of them; panels p >= group_from (the group in flight) update only the
    columns of the blocks p + 1 .. stop_cols - 1 (default upto: the group's own later panels), as the panel chain's strips do --
    what lies right of that still lacks the whole group, which is the state the group's update finds.  Returns the dense
    lower-triangular work matrix (symmetric counterpart not kept)."""
    M = np.tril(Ap).copy()
    Np = M.shape[0]
    group_from = upto if group_from is None else group_from
    stop_cols = upto if stop_cols is None else stop_cols
    for p in range(upto):
        s = slice(p * BLK, (p + 1) * BLK)
        D = np.tril(M[s, s])
        L = np.linalg.cholesky(D + np.tril(D, -1).T)
        M[s, s] = L
        lo = (p + 1) * BLK
        if lo >= Np:
            break
        M[lo:, s] = np.linalg.solve(L, M[lo:, s].T).T
        hi = Np if p < group_from else stop_cols * BLK
        if hi > lo:
            M[lo:, lo:hi] -= M[lo:, s] @ M[lo:hi, s].T
            M[lo:hi, lo:hi] = np.tril(M[lo:hi, lo:hi])
    return np.tril(M)


def update_reference(C, As, Bs):
    """(C - sum_s A_s B_s^T in long double, |C| + sum_s |A_s| |B_s|^T in fp64) for one 256-row block against a set of columns"""
    ref = np.array(C, dtype=LD)
    mag = np.abs(C).astype(np.float64)
    for A, B in zip(As, Bs):
        ref -= np.asarray(A, dtype=LD) @ np.asarray(B, dtype=LD).T
        mag += np.abs(A) @ np.abs(B).T
    return ref, mag

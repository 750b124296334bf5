"""References and bounds for the 3-D entries (include/tgp.h, "S1, S2, S3 in three dimensions"), used by test_nd3_host.py and
test_gpu_nd3.py.  Nothing here calls the library or oracle/: the four kernels and the slope w are restated with mpmath at 40
digits from the published formulas (treegp/kernels.py:114-126, 249-276, 355-381), the dense solve / predict / covariance in x87
long doubles.

A kernel is (kind, amp, M, ell): kind in "rbf" / "arbf" / "vk" / "avk", M the symmetric 3 x 3 invLam (None for "vk").

Bounds (u = 2^-53, derived from the arithmetic of csrc/nd3.hip as written, never from the device's output):

  direct Gaussian form (K build, dense matrix, cross panels, generic predict).  The exponent is
      q / 2,  q = xx dx dx + 2xy dx dy + 2xz dx dz + yy dy dy + 2yz dy dz + zz dz dz
  Each of the six products carries: two rounded differences (2 u), two multiplications (2 u) and, in the K build, the coefficient
  pre-scaled by 0.5 log2 e (1 u): 5 u relative to itself.  The six are added with five additions, each 1 u relative to a
  partial sum that is at most T = the sum of the six magnitudes: 5 u T.  So |delta (q/2)| <= 10 u (T / 2); fused multiply-adds
  only remove roundings.  exp turns an absolute error of the exponent into a relative error of the value; exp itself (libm, or
  tgp_exp2_neg: <= 1 ulp = 2 u) and the amplitude multiply (1 u) add 3 u.  Both counts doubled, as gauss_bound of
  _kernel_value_helpers.py doubles its own:
      |dev - ref| <= (8 + 20 T/2) u ref + 2 * 2^-1074
  T / 2 stands where s = q / 2 would: for a positive definite invLam the two agree within the form's condition, for a rank-
  deficient or indefinite one the products cancel and only T measures their rounding (term_magnitude of the 2-D helper).

  transformed Gaussian form (fused predict when invLam has a Cholesky factor): the three transformed coordinates of a point
  are U_k = sum_j t_kj (x_j - x0_j): one rounded difference per coordinate, up to three products, two additions and the
  coefficient t = sc l (the product and l's own rounding): 8 roundings, each relative to a quantity of the size sqrt(W), W the
  squared transformed diameter of the call's points.  A pair's dU_k = U_k(q) - U_k(i) carries both points' errors: 16 u sqrt(W)
  per component.  w = |dU|^2, so |delta w| <= 2 |dU| |delta dU| <= 2 sqrt(w) sqrt(3) 16 u sqrt(W) = 55.4 u sqrt(w W), plus the
  three squares and two additions of w itself, 5 u w <= 5 u sqrt(w W): 61, rounded up to 64.  In units of the exponent
  (s = w ln 2 / 256, S likewise) the ratio is the same; the value's own roundings are the table path's: entry times polynomial
  <= 1.5 ulp, the amplitude 0.5 ulp, doubled = 8:
      |dev - ref| <= (8 + 64 sqrt(s S)) u ref + 2 * 2^-1074

  von Karman: the tolerance of the 2-D helper's vk_bound on the profile (rtol 2e-13, atol 1e-13 on the unit value: the
  Chebyshev tables' own accuracy, tests/test_host_logic.py) plus the rounding of u: u^2 is the direct form above (relative
  error 10 u T / q of q, doubled), the square root halves it and adds 1 u, the isotropic kind's multiply by 1 / ell adds 2 u;
  d ln k / d ln u -> -(2 pi u) for large u and is below 2 pi u + 5/3 everywhere:
      rtol = 2e-13 + (2 pi u + 2) (10 T / q + 3) u
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 40

LD = np.longdouble
U53 = 2.0 ** -53
TINY = 2.0 ** -1074
K56_XMAX = 697.8738840444552   # bessel_k56.h

INVLAM = np.array([[30.0, 4.0, -3.0], [4.0, 20.0, 5.0], [-3.0, 5.0, 12.0]])
# invLam without a Cholesky factor: the launcher evaluates the quadratic form directly
RANK_ONE = np.outer([3.0, -2.0, 1.0], [3.0, -2.0, 1.0])                      # v v^T: d11 == 0
INDEFINITE = np.array([[4.0, 1.0, 0.0], [1.0, -2.0, 0.5], [0.0, 0.5, 3.0]])  # d11 < 0
KERNELS = {
    "arbf": ("arbf", 0.8 ** 2, INVLAM, None),
    "avk": ("avk", 0.8 ** 2, INVLAM, None),
    "rbf": ("rbf", 0.8 ** 2, np.diag(1.0 / np.array([0.2, 0.3, 0.5]) ** 2), None),
    "vk": ("vk", 0.8 ** 2, None, 0.4),
}


def _mpf_to_ld(v):
    """mpf -> long double to its full 64 bits, also far below the fp64 range"""
    if v == 0:
        return LD(0.0)
    man, e = mp.frexp(v)
    hi = float(man)
    lo = float(man - hi)
    return np.ldexp(LD(hi) + LD(lo), int(e))


def quad_mp(M, d):
    """d^T M d in mpmath from fp64 entries"""
    return sum(mp.mpf(float(M[a][b])) * d[a] * d[b] for a in range(3) for b in range(3))


def vk_unit_mp(u):
    """u^(5/6) K_{5/6}(2 pi u) / lim0, 1 at u == 0 (treegp/kernels.py:249-276)"""
    if u == 0:
        return mp.mpf(1)
    nu = mp.mpf(5) / 6
    lim0 = mp.gamma(nu) / (2 * mp.pi ** nu)
    return u ** nu * mp.besselk(nu, 2 * mp.pi * u) / lim0


def vk_slope_mp(u):
    """w(u) = -f'(u) / u = 2 pi u^(-1/6) K_{1/6}(2 pi u) / lim0 (A&S 9.6.28), u > 0"""
    nu = mp.mpf(5) / 6
    lim0 = mp.gamma(nu) / (2 * mp.pi ** nu)
    return 2 * mp.pi * u ** (-mp.mpf(1) / 6) * mp.besselk(mp.mpf(1) / 6, 2 * mp.pi * u) / lim0


def pair_mp(kernel, p, q):
    """(value, u or None, q/2 or None) of one pair in mpmath; the coordinates are fp64 numbers, differenced first"""
    return value_of_d_mp(kernel, [mp.mpf(float(p[a])) - mp.mpf(float(q[a])) for a in range(3)])


def value_of_d_mp(kernel, d):
    """the same for a displacement d given as three mpf"""
    kind, amp, M, ell = kernel
    if kind == "vk":
        u = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / mp.mpf(ell)
        return mp.mpf(amp) * vk_unit_mp(u), u, None
    qf = quad_mp(M, d)
    if kind == "avk":
        u = mp.sqrt(qf)
        return mp.mpf(amp) * vk_unit_mp(u), u, None
    return mp.mpf(amp) * mp.exp(-qf / 2), None, qf / 2


def kernel_matrix_mp(kernel, A, B=None):
    """(ref long double (len A, len B), x = 2 pi u as fp64 or None, s = q/2 as fp64 or None); B=None: the self matrix"""
    self_ = B is None
    B = A if self_ else B
    A, B = np.asarray(A, float), np.asarray(B, float)
    ref = np.empty((len(A), len(B)), LD)
    aux = np.zeros((len(A), len(B)))
    for i in range(len(A)):
        for j in range(len(B)):
            if self_ and j < i:
                ref[i, j], aux[i, j] = ref[j, i], aux[j, i]
                continue
            v, u, s = pair_mp(kernel, A[i], B[j])
            ref[i, j] = _mpf_to_ld(v)
            aux[i, j] = float(2 * mp.pi * u) if u is not None else float(s)
    return ref, aux


def grad_pair_mp(kernel, xq, xi):
    """d/dxq of amp k(xq - xi): -amp k M d (Gaussian), -amp w(u) M d (von Karman), exactly 0 at u == 0; three mpf"""
    kind, amp, M, ell = kernel
    d = [mp.mpf(float(xq[a])) - mp.mpf(float(xi[a])) for a in range(3)]
    if kind == "vk":
        Mm = [[(1 / mp.mpf(ell) ** 2 if a == b else mp.mpf(0)) for b in range(3)] for a in range(3)]
    else:
        Mm = [[mp.mpf(float(M[a][b])) for b in range(3)] for a in range(3)]
    Md = [sum(Mm[a][b] * d[b] for b in range(3)) for a in range(3)]
    q = sum(d[a] * Md[a] for a in range(3))
    if kind in ("rbf", "arbf"):
        f = mp.exp(-q / 2)
    else:
        if q == 0:
            return [mp.mpf(0)] * 3
        f = vk_slope_mp(mp.sqrt(q))
    return [-mp.mpf(amp) * f * Md[a] for a in range(3)]


# ---- long-double restatements (Gaussian kinds: numpy's long-double exp) ------------------------------------------------------------
def gauss_matrix_ld(kernel, A, B):
    kind, amp, M, _ = kernel
    assert kind in ("rbf", "arbf")
    D = LD(np.asarray(A, float))[:, None, :] - LD(np.asarray(B, float))[None, :, :]
    q = np.zeros(D.shape[:2], LD)
    for a in range(3):
        for b in range(3):
            q += LD(float(M[a][b])) * D[:, :, a] * D[:, :, b]
    return LD(amp) * np.exp(-q / 2)


def cholesky_ld(A):
    A = np.array(A, LD)
    n = len(A)
    L = np.zeros((n, n), LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - np.dot(L[j, :j], L[j, :j]))
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower_ld(L, B):
    B = np.array(B, LD)
    X = np.zeros_like(B)
    for i in range(len(L)):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_upper_ld(U, B):
    B = np.array(B, LD)
    X = np.zeros_like(B)
    for i in range(len(U) - 1, -1, -1):
        X[i] = (B[i] - U[i, i + 1:] @ X[i + 1:]) / U[i, i]
    return X


class DenseGP(object):
    """K + diag(yerr^2) = L L^T in long doubles for a Gaussian kernel; alpha, predictions, covariance, K^-1"""

    def __init__(self, kernel, X, yerr):
        self.kernel, self.X = kernel, np.asarray(X, float)
        K = gauss_matrix_ld(kernel, X, X)
        K[np.diag_indices(len(K))] = LD(kernel[1]) + LD(np.asarray(yerr, float)) ** 2
        self.K, self.L = K, cholesky_ld(K)

    def solve(self, B):
        return solve_upper_ld(self.L.T, solve_lower_ld(self.L, B))

    def logdet(self):
        return 2 * np.sum(np.log(np.diag(self.L)))

    def cross(self, Xs):
        return gauss_matrix_ld(self.kernel, Xs, self.X)

    def predict(self, alpha, Xs):
        return self.cross(Xs) @ LD(alpha)

    def cov(self, Xs):
        H = self.cross(Xs)
        Kss = gauss_matrix_ld(self.kernel, Xs, Xs)
        Kss[np.diag_indices(len(Kss))] = LD(self.kernel[1])
        Bt = solve_lower_ld(self.L, H.T)
        return Kss - Bt.T @ Bt

    def inverse(self):
        return self.solve(np.eye(len(self.K), dtype=LD))


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def term_magnitude(M, A, B):
    """T / 2 for every pair: half the sum of the magnitudes of the six products of the direct form"""
    D = np.asarray(A, float)[:, None, :] - np.asarray(B, float)[None, :, :]
    T = np.zeros(D.shape[:2])
    for a in range(3):
        for b in range(3):
            T += abs(float(M[a][b])) * np.abs(D[:, :, a] * D[:, :, b])
    return 0.5 * T


def gauss_bound_direct(ref, half_T, amp=1.0, kbuild=False):
    """(8 + 20 T/2) u ref + 2 * 2^-1074; the packed K build clamps its exponent (kernel_eval.h: tgp_exp2_neg), below 2^-1021 its
    documented stand-in is amp 2^-1021 p: absolute error < amp 4.5e-308 there"""
    b = (LD(8.0) + LD(20.0) * LD(half_T)) * LD(U53) * np.abs(ref) + LD(2.0) * LD(TINY)
    if kbuild:
        b = b + np.where(np.abs(ref) < LD(amp) * LD(2.0 ** -1021) * (1 + LD(1e-9)), LD(amp) * LD(4.5e-308), LD(0.0))
    return b


def gauss_bound_transformed(ref, s, S):
    """(8 + 64 sqrt(s S)) u ref + 2 * 2^-1074, S = the exponent across the diameter of the call's points"""
    s = np.abs(np.asarray(s, float))
    S = np.maximum(S, s)
    return (LD(8.0) + LD(64.0) * np.sqrt(LD(s) * LD(S))) * LD(U53) * np.abs(ref) + LD(2.0) * LD(TINY)


def diameter_exponent(M, points):
    """max over pairs of points of d^T M d / 2 (all pairs: the point sets of these tests are small)"""
    P = np.asarray(points, float)
    P = P[np.all(np.isfinite(P), axis=1)]
    D = P[:, None, :] - P[None, :, :]
    return float(0.5 * np.einsum("ija,ab,ijb->ij", D, np.asarray(M, float), D).max())


def vk_bound(ref, amp, x, half_T_over_q):
    """amp 1e-13 + (2e-13 + (x + 2) (10 T / q + 3) u) |ref|, x = 2 pi u; half_T_over_q = (T/2) / (q/2) >= 1 (1 for the isotropic kind)"""
    rtol = LD(2e-13) + (LD(x) + LD(2.0)) * (LD(10.0) * LD(half_T_over_q) + LD(3.0)) * LD(U53)
    return LD(amp) * LD(1e-13) + rtol * np.abs(ref)


def predict_sum_bound(terms_abs_sum, n):
    """|ys - ref| <= c u sum_i |alpha_i k_i| + (the values' own bound, added by the caller).  Summation order of nd3.hip: one (generic)
    or two interleaved (table path) running sums per split of at most ceil(n / 256) * 256 terms, then the splits in order and one
    multiply by the amplitude: every term passes through at most n + 2 additions (its split's running sum, the pair of
    accumulators, the splits) and its own fused multiply-add, so c = n + 4."""
    return LD(n + 4) * LD(U53) * LD(terms_abs_sum)


# ---- inputs that reach every branch (checked by test_nd3_host.py from these references alone) ---------------------------------------
def gauss_residues(s):
    """round(256 log2(e) s) mod 256: the entry of the 2^(j/256) table the pair reads on the transformed path"""
    k = np.rint(LD(s) * (LD(256.0) / np.log(LD(2.0))))
    return (k % 256).astype(np.int64)


VK_SEGMENTS = ("series", "[1,2)", "[2,4)", "[4,8)", "[8,16)", "[16,32)", "[32,XMAX]", "beyond")


def vk_segment(x):
    """index into VK_SEGMENTS of x = 2 pi u (bessel_k56.h: series up to 1, octaves, the tail, exactly 0 beyond the cut)"""
    x = np.asarray(x, float)
    seg = np.where(x <= 1.0, 0, np.minimum(np.floor(np.log2(np.maximum(x, 1.0))).astype(int) + 1, 6))
    return np.where(x > K56_XMAX, 7, seg)


def direction_points(n, seed, scale_lo, scale_hi, center):
    """n points around `center`: random directions, log-uniform distances in [scale_lo, scale_hi]; exact fp64 numbers"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    r = np.exp(rng.uniform(np.log(scale_lo), np.log(scale_hi), n))
    return np.asarray(center, float) + v * r[:, None]


VALUE_CENTER = np.array([0.3125, 0.6875, -0.25])


def value_queries(kind):
    """query points around VALUE_CENTER for the pair-by-pair tests.  Gaussian kinds: exponents from 1e-9 to beyond the
    underflow (s > 745: subnormal and flushed values) with every table residue; von Karman kinds: every Chebyshev segment,
    the series and pairs beyond the cut.  Row 0 is the centre itself (a coincident point)."""
    if kind in ("rbf", "arbf"):
        P = direction_points(1144, 11, 1e-5, 14.0, VALUE_CENTER)
        # every residue j of the 256-entry table, on the x axis: s = (512 + j + 1/4) ln 2 / 256 = xx r^2 / 2
        j = np.arange(256)
        r = np.sqrt(2.0 * (512 + j + 0.25) * np.log(2.0) / 256 / KERNELS[kind][2][0, 0])
        # subnormal results (709 < s < 745) and flushed ones, on the same axis
        r = np.concatenate([r, np.sqrt(2.0 * np.array([712.0, 720.0, 730.0, 738.0, 743.0, 750.0, 800.0]) / KERNELS[kind][2][0, 0])])
        P = np.concatenate([P, VALUE_CENTER + np.stack([r, 0 * r, 0 * r], axis=1)])
    elif kind == "avk":
        P = direction_points(500, 12, 1e-4, 60.0, VALUE_CENTER)
    else:
        P = direction_points(500, 13, 1e-4, 80.0, VALUE_CENTER)
    P[0] = VALUE_CENTER
    return P

"""Helpers of tests/test_gpu_units.py and tests/test_units_host.py: exact changes of units, the dimension of every output, and
the comparisons.  Nothing here calls the library.

A change of units is a triple of integers (p, r, q):

  S_a(p)  the unit of the values:       amp * 4^p,  y, y_err, white_noise, kk values * 2^p
  S_y(r)  the data alone:               y * 2^r, the kernel and the errors fixed (the solve is linear in y)
  S_x(q)  the unit of the coordinates:  X, Xs, min_sep, max_sep, tables * 2^q;  invLam a, b, c and KernelSpec3.m * 4^-q;
                                        ell * 2^q

All of them are powers of two, applied with ``np.ldexp``: no rounding happens anywhere, so a homogeneous route must return the
same significands with shifted exponents.  The expected result of an output of dimension Y^i X^j is
``np.ldexp(unscaled, i * p + j * q)``, compared on the int64 view of the doubles (so -0.0 against 0.0 and NaN payloads count).
Under S_y(r) an output that is homogeneous of degree d in y shifts by d * r (third entry of the table; None where the output is
not homogeneous in y alone, e.g. the likelihood gradient, a difference of a quadratic and a constant term).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


class Units(object):
    """one change of units; ``Units()`` is the identity"""

    def __init__(self, p=0, r=0, q=0):
        self.p, self.r, self.q = int(p), int(r), int(q)

    def __repr__(self):
        parts = [n + "(%+d)" % v for n, v in (("S_a", self.p), ("S_y", self.r), ("S_x", self.q)) if v]
        return "*".join(parts) or "unit"

    # what is applied to the inputs
    def y(self, v):
        return np.ldexp(np.asarray(v, dtype=np.float64), self.p + self.r)

    def err(self, v):
        return None if v is None else np.ldexp(np.asarray(v, dtype=np.float64), self.p)

    def val(self, v):
        """values that carry the unit Y but are not the solve's right-hand side (kk values, white noise)"""
        return np.ldexp(np.asarray(v, dtype=np.float64), self.p)

    def amp(self, v):
        return float(np.ldexp(np.float64(v), 2 * self.p))

    def x(self, v):
        return np.ldexp(np.asarray(v, dtype=np.float64), self.q)

    def sep(self, v):
        return float(np.ldexp(np.float64(v), self.q))

    def invlam(self, v):
        return np.ldexp(np.asarray(v, dtype=np.float64), -2 * self.q)

    def ell(self, v):
        return float(np.ldexp(np.float64(v), self.q))

    def kw(self, kw):
        """a dict of KernelSpec arguments (amp, a, b, c, ell) in the new units"""
        out = {}
        for k, v in kw.items():
            if k == "amp":
                out[k] = self.amp(v)
            elif k in ("a", "b", "c"):
                out[k] = float(self.invlam(v))
            elif k == "ell":
                out[k] = self.ell(v)
            elif k == "m":
                out[k] = tuple(float(t) for t in self.invlam(v))
            else:
                out[k] = v
        return out

    def shift(self, dim):
        """the exponent shift of an output of dimension ``dim`` (a name of DIMENSIONS or a triple); None: not homogeneous"""
        py, px, dy = DIMENSIONS[dim] if isinstance(dim, str) else dim
        if self.r and dy is None:
            return None
        return py * self.p + px * self.q + (dy or 0) * self.r


UNIT = Units()
S_A = (Units(p=-25), Units(p=10))
S_Y = (Units(r=-40), Units(r=40))
S_X = (Units(q=-17), Units(q=12))
COMBINED = Units(p=-25, q=12)
WITH_Y = S_A + S_Y + S_X + (COMBINED,)           # routes that y enters
NO_Y = S_A + S_X + (COMBINED,)                   # routes without data

# output -> (power of Y, power of X, degree in y alone or None)
DIMENSIONS = {
    "alpha": (-1, 0, 1),
    "K": (2, 0, 0), "cov": (2, 0, 0), "var": (2, 0, 0),
    "L": (1, 0, 0),                              # the packed factor
    "W": (-1, 0, 0),                             # its inverted diagonal blocks
    "factor_solve": (-2, 0, 0),                  # of a B that stays as it is
    "factor_lmul": (1, 0, 0),                    # of a Z that stays as it is
    "inv_diag": (-2, 0, 0), "inv_blocks": (-2, 0, 0),
    "predict": (1, 0, 1),
    "predict_grad": (1, -1, 1),
    "ydota": (0, 0, 2),
    "grad_logamp": (0, 0, None),
    "grad_abc": (0, 2, None),
    "grad_ell": (0, -1, None),                   # (of a theta-space gradient; the device's four slots are log amp, a, b, c)
    "local_mean": (1, 0, 1),
    "local_var": (2, 0, 0),
    "int": (0, 0, 0),                            # neighbour lists, counts, info, pair counts: identical integers
    "chi2_sum": (0, 0, 2),                       # sum r^2 / s^2
    "xi": (2, 0, 0),
    "weight": (0, 0, 0),                         # pair weights (the w of the catalogue are not values)
    "knn_mean": (1, 0, 1),
    "field": (1, 0, 1),                          # realisations
}


def fisher_shift(units, nterms=1):
    """(4 T, 4 T) exponent shifts of a Fisher matrix in the device's parameters (log amp, a, b, c) per term: an entry has the
    inverse dimensions of its two parameters, i.e. X^2 per invLam parameter"""
    per = np.array([0, 2, 2, 2] * nterms) * units.q
    return per[:, None] + per[None, :]


def bits(a):
    a = np.asarray(a)
    if a.dtype.kind in "iub":
        return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.int64)


def expected(unscaled, shift):
    u = np.asarray(unscaled)
    if u.dtype.kind in "iub":
        assert np.all(np.asarray(shift) == 0)
        return u
    return np.ldexp(np.asarray(u, dtype=np.float64), shift)


def ulp_distance(a, b):
    """largest distance in units of the last place between two float64 arrays (inf where the signs differ)"""
    ia, ib = bits(a), bits(b)
    if len(ia) == 0:
        return 0.0
    same = (ia < 0) == (ib < 0)
    d = np.abs(np.where(same, ia - ib, 0)).astype(np.float64)              # int64: exact for equal signs
    return float(np.where(same, d, np.inf).max())


def diff_report(got, unscaled, shift):
    """None when ``got`` has exactly the bits of ldexp(unscaled, shift), else one line that says how far off it is"""
    exp = expected(unscaled, shift)
    if np.shape(got) != np.shape(exp):
        return "shape %r against %r" % (np.shape(got), np.shape(exp))
    g, e = bits(got), bits(exp)
    if np.array_equal(g, e):
        return None
    bad = np.nonzero(g != e)[0]
    fg, fe = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(exp, dtype=np.float64).reshape(-1)
    i = bad[0]
    return ("%d of %d values differ, up to %.0f ulp; first at %d: %r (%s) against %r (%s)"
            % (len(bad), len(g), ulp_distance(fg[bad], fe[bad]), i, fg[i], float(fg[i]).hex(), fe[i], float(fe[i]).hex()))


def assert_shifted_within(got, ref, bound, shift, what):
    """For sums whose order of addition the device does not fix (fp64 atomics): two calls at ONE scale already differ in the
    last bits, so equal bits cannot be asked across scales.  ``ref`` (long double) and ``bound`` are the exact value and the
    error bound of the unit-scale call, derived from u = 2^-53 and the terms' magnitudes; both scale exactly, so the call in
    other units must lie within ldexp(bound, shift) of ldexp(ref, shift).  Returns the largest error / bound."""
    want = np.ldexp(np.asarray(ref, dtype=LD).reshape(-1), shift)
    bnd = np.ldexp(np.asarray(bound, dtype=np.float64).reshape(-1), shift)
    g = np.asarray(got, dtype=np.float64).reshape(-1)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    assert np.all(np.isfinite(g)), what
    err = np.abs(g.astype(LD) - want).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bnd)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, "%s: error / bound %.3f at %d" % (what, worst, int(np.argmax(ratio)))
    return worst


def assert_homogeneous(scaled, unscaled, units, what):
    """``scaled`` and ``unscaled``: lists of (name, dimension, value) from the same route at the two scales.  Every output
    that is homogeneous under ``units`` must have the bits of its shifted unit-scale value; all are checked before failing."""
    assert [(k, d) for k, d, _ in scaled] == [(k, d) for k, d, _ in unscaled], what
    failures = []
    for (k, dim, a), (_, _, b) in zip(scaled, unscaled):
        if dim is None:
            continue
        sh = dim if isinstance(dim, np.ndarray) else units.shift(dim)
        if sh is None:
            continue
        rep = diff_report(a, b, sh)
        if rep is not None:
            failures.append("%s [%s, shift %s]: %s" % (k, dim if isinstance(dim, str) else "matrix", np.max(sh), rep))
    assert not failures, "%s under %r is not bit-homogeneous:\n  %s" % (what, units, "\n  ".join(failures))


# ---- outputs that go through a logarithm ----------------------------------------------------------------------------------

def log_shift(count, per_row_exponent):
    """the exact change of a sum of ``count`` logarithms whose arguments are multiplied by 2^per_row_exponent, long double"""
    return LD(count) * LD(per_row_exponent) * np.log(LD(2.0))


def log_tolerance(n, value, per_row_exponent):
    """4 n 2^-53 max(|value|, n |shift per row|).

    A sum of n logarithms: each term log(x_i 2^e) is the correctly rounded e ln 2 + log x_i to about 1 ulp of itself, and is at
    most |log x_i| + |e| ln 2 in size, so the n terms together carry at most n 2^-53 (sum |log x_i| + n |e| ln 2) of rounding;
    adding them in any order loses at most another (n - 1) 2^-53 times the sum of the magnitudes of the partial sums.  With
    |value| standing for sum |log x_i| (all diagonal entries on one side of 1 in the worst case) both runs together stay
    within 4 n 2^-53 max(|value|, n |e| ln 2): the bound the issue states, taken from the arithmetic, not from the device."""
    return 4.0 * n * U * max(abs(float(value)), n * abs(per_row_exponent) * float(np.log(2.0)))


def assert_log_shift(scaled, unscaled, n, per_row_exponent, what, count=None):
    count = n if count is None else count
    want = log_shift(count, per_row_exponent)
    got = LD(scaled) - LD(unscaled)
    tol = log_tolerance(n, max(abs(scaled), abs(unscaled)), per_row_exponent)
    err = abs(float(got - want))
    assert err <= tol, "%s: log quantity moved by %r, exact shift %r: off by %.3e, allowed %.3e" % (what, float(got), float(want), err, tol)
    return err, tol


# ---- inputs ---------------------------------------------------------------------------------------------------------------

INVLAM = dict(a=400.0, b=80.0, c=500.0)          # the README's invLam [[400, 80], [80, 500]]
ELL = 0.1
AMP = 1.3
M3 = (400.0, 80.0, 40.0, 500.0, 60.0, 450.0)     # KernelSpec3.m: xx, xy, xz, yy, yz, zz (diagonally dominant)
DENSE_N = (300, 2300, 2304)
QUERY_M = (1, 257)
BATCH_NS = (1, 130, 256, 1000, 1025)
BATCH_MS = (1, 257, 130, 1, 257)
BATCH_P = (-25, 0, 10, -25, 10)
LOCAL_N, LOCAL_M = 3000, 257
FISHER_N = 700
PAIR_N, PAIR_NBOOT = 2000, 8
RANGE = 200                                       # no |y|, y_err^2 or amp leaves [2^-200, 2^200]
GAUSS_EXPONENT_MAX = 900


class Inputs(object):
    """points in [0, 0.5]^d, values of order one, y_err uniform in [0.05, 0.2]: cond(K + D) ~ 1e3"""

    def __init__(self, n, seed=0, ndim=2, m=max(QUERY_M)):
        rng = np.random.default_rng(52000 + 17 * n + seed)
        self.n, self.ndim = n, ndim
        self.X = rng.uniform(0.0, 0.5, (n, ndim))
        self.y = np.sin(9.0 * self.X[:, 0]) * np.cos(7.0 * self.X[:, 1]) + 0.3 * rng.standard_normal(n)
        self.e = rng.uniform(0.05, 0.2, n)
        self.Xq = rng.uniform(0.0, 0.5, (m, ndim))
        self.B = rng.standard_normal((5, n))
        self.Z = rng.standard_normal((3, n))

    def at(self, units):
        """the same problem in other units (a plain namespace: X, y, e, Xq; B and Z stay as they are)"""
        s = Inputs.__new__(Inputs)
        s.n, s.ndim = self.n, self.ndim
        s.X, s.Xq = units.x(self.X), units.x(self.Xq)
        s.y, s.e = units.y(self.y), units.err(self.e)
        s.B, s.Z = self.B, self.Z
        return s

    def arrays(self):
        return dict(X=self.X, y=self.y, e=self.e, Xq=self.Xq, B=self.B, Z=self.Z)


_INPUTS = {}


def inputs(n, seed=0, ndim=2):
    key = (n, seed, ndim)
    if key not in _INPUTS:
        _INPUTS[key] = Inputs(n, seed, ndim)
    return _INPUTS[key]


def inv_block_starts(n):
    """groups of factor_inv_blocks: single rows, a group that crosses row 1024 where n allows, ragged sizes"""
    if n > 1100:
        s = [0, 1, 129, 1000, 1060, 1061, 1300, n]
    else:
        s = [0, 1, 65, 200, n]
    return np.array(s, dtype=np.int64)


def pair_catalogue(n=PAIR_N, seed=3):
    rng = np.random.default_rng(61000 + n + seed)
    return dict(x=rng.uniform(0.0, 0.5, n), y=rng.uniform(0.0, 0.5, n), k=rng.standard_normal(n),
                w=rng.uniform(0.5, 2.0, n), err=rng.uniform(0.05, 0.2, n),
                dx=rng.standard_normal(n), dy=rng.standard_normal(n))


PAIR_TWOD = dict(min_sep=0.0, max_sep=0.0625, nbins=11)
PAIR_LOG = dict(min_sep=0.01, max_sep=0.3, nbins=9)


def pair_log_edges(units):
    """the ln r edges handed to vcorr_sums at a scale: linspace between the logarithms of the scaled separations"""
    lg = PAIR_LOG
    return np.linspace(np.log(units.sep(lg["min_sep"])), np.log(units.sep(lg["max_sep"])), lg["nbins"] + 1)

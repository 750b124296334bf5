"""Gradient of the predicted mean on the GPU (tgp_gp_predict_grad, seam S3g) against the long-double oracle of
tests/_predict_grad_refs.py, every output within

    |g_jc - ref_jc| <= 2^-53 sum_i (n + E_ijc) |t_ijc|

(E: _predict_grad_refs.pair_slack, derived there from the number formats; nothing is tuned against device output), plus the
special inputs, determinism, the generic Gaussian route in a fresh process, the device-resident entry point and the Python API.
One pool of 2049 training points and 257 queries per kernel serves every shape: a call's reference is a prefix sum.

    python tests/test_gpu_predict_grad.py            # the Gaussian cases in this process: one JSON line of max error / bound
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _predict_grad_refs as R
from _kernel_value_helpers import K56_XMAX, LD, U53

pytestmark = pytest.mark.gpu

NS = (1, 255, 256, 257, 513, 2049)      # a partial LDS tile, a full one, one point past it, a split with a ragged last chunk
MS = (1, 255, 257)
SHEAR = dict(a=400.0, b=80.0, c=500.0)
CASES = {
    "rbf": ("rbf", dict(amp=1.3, a=100.0, b=0.0, c=100.0, ell=1.0), 2),
    "arbf": ("arbf", dict(amp=0.7, ell=1.0, **SHEAR), 2),
    "vk": ("vk", dict(amp=0.49, a=1.0, b=0.0, c=1.0, ell=0.3), 2),
    "avk": ("avk", dict(amp=0.9, a=40.0, b=8.0, c=50.0, ell=1.0), 2),
    "gauss1d": ("arbf", dict(amp=1.1, a=25.0, b=0.0, c=0.0, ell=1.0), 1),
    "vk1d": ("vk", dict(amp=2.0, a=1.0, b=0.0, c=1.0, ell=0.2), 1),
}


def _tg():
    from treegp_amd import _lib, ops
    return _lib, ops


def make_spec(kind, p):
    _lib, ops = _tg()
    k = {"rbf": _lib.TGP_RBF, "arbf": _lib.TGP_ARBF, "vk": _lib.TGP_VK, "avk": _lib.TGP_AVK}[kind]
    return ops.KernelSpec(k, amp=p["amp"], a=p["a"], b=p["b"], c=p["c"], ell=p["ell"])


def pool(ndim, shift=0.0, seed=42):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (NS[-1], 2))
    Xs = rng.uniform(0, 1, (MS[-1], 2))
    alpha = rng.standard_normal(NS[-1])
    if ndim == 1:
        X[:, 1] = 0.0
        Xs[:, 1] = 0.0
    if shift:
        X[:, :ndim] += shift
        Xs[:, :ndim] += shift
    return X, alpha, Xs


class Oracle(object):
    """reference and bound of every prefix call (X[:n], alpha[:n], Xs[:m]) of one pool, from one pass over its pairs"""

    def __init__(self, kind, p, X, alpha, Xs, fast):
        terms = R.grad_terms(kind, p, X, alpha, Xs)
        S = R.call_exponent(kind, p, X, Xs) if fast else None          # the pool's diameter bounds every prefix call's
        slack = R.pair_slack(kind, p, X, alpha, Xs, terms, fast, S)
        self.ref = np.cumsum(terms["T"], axis=0)
        self.abs = np.cumsum(np.abs(terms["T"]), axis=0)
        self.slack = np.cumsum(slack, axis=0)

    def check(self, g, n, m, what):
        ref = self.ref[n - 1, :m]
        bound = R.grad_bound(n, self.abs[n - 1, :m], self.slack[n - 1, :m])
        g = np.asarray(g, float)
        assert g.shape == (m, 2) and np.all(np.isfinite(g)), what
        err = np.abs(LD(g) - ref)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0)).astype(float)
        worst = float(ratio.max())
        print("%s: max |g - ref| / bound = %.3g" % (what, worst))
        assert worst <= 1.0, (what, worst, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        return worst


def is_fast(kind, p):
    return R.takes_fast_path(kind, p) and "TGP_PREDICT_GENERIC" not in os.environ


_ORACLES = {}


def oracle(name, shift=0.0, nmax=NS[-1], mmax=MS[-1]):
    key = (name, shift, nmax, mmax, "TGP_PREDICT_GENERIC" in os.environ)
    if key not in _ORACLES:
        kind, p, ndim = CASES[name]
        X, alpha, Xs = pool(ndim, shift)
        X, alpha, Xs = X[:nmax], alpha[:nmax], Xs[:mmax]
        _ORACLES[key] = (X, alpha, Xs, Oracle(kind, p, X, alpha, Xs, is_fast(kind, p)))
    return _ORACLES[key]


def run(name, n, m, shift=0.0, own=False):
    """own: an oracle of this call's pairs alone instead of the pool's"""
    _, ops = _tg()
    kind, p, _ = CASES[name]
    X, alpha, Xs, orc = oracle(name, shift, n, m) if own else oracle(name, shift)
    g = ops.gp_predict_grad(make_spec(kind, p), X[:n], alpha[:n], Xs[:m])
    return g, orc


# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_shapes_within_bound(name):
    for n in NS:
        for m in MS:
            g, orc = run(name, n, m)
            orc.check(g, n, m, "%s n=%d m=%d" % (name, n, m))
            if CASES[name][2] == 1:
                assert np.all(g[:, 1] == 0.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_query_on_training_points(name):
    """queries equal to training points: finite, within the bound (the pair at zero distance contributes exactly 0 to the
    reference as well); one point against itself: exactly (0, 0)"""
    _, ops = _tg()
    kind, p, ndim = CASES[name]
    spec = make_spec(kind, p)
    X, alpha, _ = pool(ndim)
    n, Xs = 513, np.concatenate([X[[0, 1, 255, 256, 300, 512]], X[600:603]])
    g = ops.gp_predict_grad(spec, X[:n], alpha[:n], Xs)
    Oracle(kind, p, X[:n], alpha[:n], Xs, is_fast(kind, p)).check(g, n, len(Xs), name + " on training points")
    for x in (X[:1], X[5:6]):
        z = ops.gp_predict_grad(spec, x, np.array([1.7]), x)
        assert z.shape == (1, 2) and np.all(z == 0.0), (name, z)


@pytest.mark.parametrize("name", ["vk", "avk", "vk1d"])
def test_beyond_the_cutoff_is_exactly_zero(name):
    _, ops = _tg()
    kind, p, ndim = CASES[name]
    X, alpha, _ = pool(ndim)
    # the unit square is within u <= sqrt(2 * 50) / ... of itself; (200, 0) and beyond are farther than the cutoff from all of it
    scale = p["ell"] if kind == "vk" else 1 / np.sqrt(min(np.linalg.eigvalsh([[p["a"], p["b"]], [p["b"], p["c"]]])))
    far = np.array([[1.0 + 1.01 * (K56_XMAX / (2 * np.pi)) * scale, 0.0], [-200.0 * scale, 0.0 if ndim == 1 else 300.0 * scale]])
    g = ops.gp_predict_grad(make_spec(kind, p), X[:600], alpha[:600], np.vstack([far, X[:1] + 0.01 * (np.arange(2) < ndim)]))
    assert np.all(g[:2] == 0.0) and np.any(g[2] != 0.0)


@pytest.mark.parametrize("name", ["rbf", "arbf", "vk", "avk"])
def test_shifted_by_2_to_the_20(name):
    """the same data 2^20 away, reference and bound from the shifted float64 inputs"""
    g, orc = run(name, 513, 255, shift=2.0 ** 20, own=True)
    orc.check(g, 513, 255, name + " shifted")


@pytest.mark.parametrize("name", ["arbf", "avk"])
def test_bits_do_not_depend_on_run_or_on_m(name):
    _, ops = _tg()
    kind, p, ndim = CASES[name]
    spec = make_spec(kind, p)
    X, alpha, Xs = pool(ndim)
    rng = np.random.default_rng(3)
    big = np.vstack([Xs, rng.uniform(0, 1, (40000, 2))])        # more than one slab of queries
    for n in (513, 2049):
        g = ops.gp_predict_grad(spec, X[:n], alpha[:n], Xs)
        assert np.array_equal(g, ops.gp_predict_grad(spec, X[:n], alpha[:n], Xs))
        assert np.array_equal(g[:255], ops.gp_predict_grad(spec, X[:n], alpha[:n], Xs[:255]))
        assert np.array_equal(g[100:131], ops.gp_predict_grad(spec, X[:n], alpha[:n], Xs[100:131]))
    gb = ops.gp_predict_grad(spec, X, alpha, big)
    assert np.array_equal(gb[:257], g)
    assert np.array_equal(gb[32700:32800], ops.gp_predict_grad(spec, X, alpha, big[32700:32800]))     # across the slab edge


def gauss_cases_here():
    """max error / bound of the Gaussian cases on whatever route this process takes"""
    out = {"generic": "TGP_PREDICT_GENERIC" in os.environ}
    for name in ("rbf", "arbf", "gauss1d"):
        for n, m in ((257, 257), (2049, 255)):
            g, orc = run(name, n, m)
            out["%s n=%d m=%d" % (name, n, m)] = orc.check(g, n, m, name)
    return out


def test_generic_gaussian_route_in_a_fresh_process():
    """TGP_PREDICT_GENERIC is read once per process: a child takes the generic route and meets its bound there"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, TGP_PREDICT_GENERIC="1"),
                       capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert res.pop("generic") is True and len(res) == 6 and max(res.values()) <= 1.0, res
    # and the two routes are different code: they agree within the sum of their bounds, not bit for bit
    g, _ = run("arbf", 2049, 255)
    assert np.all(np.isfinite(g))


def test_device_resident_entry_point_agrees_bit_for_bit():
    _lib, ops = _tg()
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    for name in ("arbf", "vk"):
        kind, p, ndim = CASES[name]
        spec = make_spec(kind, p)
        X, alpha, Xs = pool(ndim)
        n, m = 513, 257
        bufs = [ops.DeviceBuffer.from_array(ctx, a) for a in (X[:n], alpha[:n], Xs[:m])] + [ops.DeviceBuffer(ctx, m * 16)]
        rc = lib.tgp_d_gp_predict_grad(ctx, C.byref(spec.to_c()), bufs[0].ptr, n, bufs[1].ptr, bufs[2].ptr, m, bufs[3].ptr)
        _lib.check(ctx, rc, "tgp_d_gp_predict_grad")
        g = bufs[3].to_array((m, 2))
        assert _lib.timings(ctx)[3] > 0.0
        for b in bufs:
            b.free()
        assert np.array_equal(g, ops.gp_predict_grad(spec, X[:n], alpha[:n], Xs[:m]))


def test_argument_errors():
    _lib, ops = _tg()
    X, alpha, Xs = pool(2)
    bad = ops.KernelSpec(7, amp=1.0, a=1.0, b=0.0, c=1.0, ell=1.0)
    with pytest.raises(_lib.TgpError, match="kind") as ex:
        ops.gp_predict_grad(bad, X[:10], alpha[:10], Xs[:5])
    assert ex.value.rc == -1
    with pytest.raises(_lib.TgpError, match="m > 0") as ex:
        ops.gp_predict_grad(make_spec(*CASES["arbf"][:2]), X[:10], alpha[:10], np.empty((0, 2)))
    assert ex.value.rc == -1


# ---------------------------------------------------------------------------------------------------------
# the Python API on the golden problems
def _golden_gps(golden):
    import treegp_amd as treegp
    g2, g3 = golden("g2_aniso2d.npz"), golden("g3_vonkarman.npz")
    out = []
    gp = treegp.GPInterpolation(kernel=str(g2["kernel"]), optimizer="none", normalize=True, white_noise=0.01)
    gp.initialize(g2["X"], g2["y"], y_err=g2["y_err"])
    out.append(("g2", "arbf", gp, g2["Xs"][:64]))
    for tag in ("vk", "avk"):
        gp = treegp.GPInterpolation(kernel=str(g3[tag + "_kernel"]), optimizer="none", normalize=True)
        gp.initialize(g3["X"], g3["y"], y_err=g3["y_err"])
        out.append(("g3 " + tag, tag, gp, g3["Xs"][:64]))
    return out


def test_api_equals_ops_and_the_central_difference_of_predict(golden):
    """gp.predict_gradient is ops.gp_predict_grad on the object's alpha, and agrees with (predict(x + h e_c) - predict(x - h e_c))
    / 2h at h = 1e-3 kernel lengths within  h^2 / 6 max |d^3 f / dx_c^3| + eps_y / h:  the first from the oracle (the second
    difference of its gradient over the same stencil, maximum over the queries, doubled because that is the third derivative's
    mean over the stencil and not its maximum), eps_y = (n 2^-53 + 4e-13) sum_i |alpha_i amp k_ij| + 2^-53 max |y| the
    rounding of one predicted value (4e-13: the value's pair criteria of tests/_kernel_value_helpers.py; k <= 1 stands in for
    the von Karman values)."""
    from treegp_amd import ops
    from treegp_amd.kernels import kernel_to_spec
    for label, kind, gp, Xq in _golden_gps(golden):
        gp.solve()
        spec = kernel_to_spec(gp.kernel)
        g = gp.predict_gradient(Xq)
        assert g.shape == (len(Xq), 2)
        assert np.array_equal(g, ops.gp_predict_grad(spec, gp._X, gp._alpha, Xq))
        p = dict(amp=spec.amp, a=spec.a, b=spec.b, c=spec.c, ell=spec.ell)
        M = np.eye(2) / spec.ell ** 2 if kind == "vk" else np.array([[spec.a, spec.b], [spec.b, spec.c]])
        h = 1e-3 / np.sqrt(np.linalg.eigvalsh(M).max())
        X, alpha, n = np.asarray(gp._X, float), gp._alpha, len(gp._X)
        y0 = gp.predict(Xq)
        for c in range(2):
            e = np.zeros(2)
            e[c] = h
            plus, minus = Xq + e, Xq - e
            hh = (plus[:, c] - minus[:, c]) / 2                                  # the step actually taken
            fd = (gp.predict(plus) - gp.predict(minus)) / (2 * hh)
            gs = [R.grad_terms(kind, p, X, alpha, Q) for Q in (minus, Xq, plus)]
            G = [t["T"].sum(axis=0)[:, c] for t in gs]
            third = float(np.abs(G[2] - 2 * G[1] + G[0]).max()) / h ** 2
            kabs = np.abs(gs[1]["k"]) if kind == "arbf" else np.ones_like(gs[1]["k"])
            eps_y = (n * U53 + 4e-13) * float((np.abs(spec.amp * alpha)[:, None] * kabs).sum(axis=0).max()) + U53 * float(np.abs(y0).max())
            tol = 2 * h ** 2 / 6 * third + eps_y / h
            err = float(np.abs(fd - g[:, c]).max())
            print("%s component %d: |central difference - gradient| = %.3g, tolerance %.3g (truncation %.3g, rounding %.3g), "
                  "max |g| = %.3g" % (label, c, err, tol, 2 * h ** 2 / 6 * third, eps_y / h, float(np.abs(g[:, c]).max())))
            assert err <= tol, (label, c, err, tol)
            assert float(np.abs(LD(g[:, c]) - G[1]).max()) <= tol                # (and the oracle itself, far inside it)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(gauss_cases_here()))

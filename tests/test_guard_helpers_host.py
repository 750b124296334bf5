"""The guard-band detector detects (tests/_guard_helpers.py): stand-in "entries" written in NumPy over raw addresses, as the
library sees its arguments, that store one element behind an output, one in front of it, at the far end of a guard, modify a
`const` input, read the element behind an input into the result, or leave an output element unwritten.  Each must be caught with
the right argument named, whichever fill shows it; a clean stand-in must pass.  On NumPy buffers and on torch (CPU) tensors: the
two code paths of the helper.  This is the only place where a violation is planted; nothing of the kind runs on a device.

Every expectation is a pytest.raises: the file fails if `assert_untouched` or `assert_same_bits` is made a no-op."""
import ctypes as C

import numpy as np
import pytest

import _guard_helpers as G

WHERE = ["numpy", "cpu"]
N = 300


def _view(addr, n, ctype=C.c_double, first=0):
    """elements first .. n - 1 at a raw address (first < 0, n beyond the extent: what a wrong mask reaches)"""
    size = C.sizeof(ctype)
    return np.ctypeslib.as_array((ctype * (n - first)).from_address(addr + first * size))


def is_banded(buf):
    """the buffer is the middle of a larger allocation.  The stand-ins misbehave only then: outside a plain exact-size buffer
    lies memory that is not theirs to touch, which is the very reason for the bands"""
    return buf.storage_offset() > 0 if G._is_torch(buf) else buf.base is not None and buf.base.size > buf.size


def standin(fault=None):
    """call(bufs) of an entry  out[i] = 2 x[i] + w[i],  cnt[i] = i or -1 from N - 5 on,  s = sum x  -- with one planted fault"""
    def call(bufs, fault=fault):
        assert bufs["absent"] is None
        if not is_banded(bufs["out"]):
            fault = None
        px, pw, po, pc = (G.ptr_of(bufs[k]) for k in ("x", "w", "out", "cnt"))
        x, w, out, cnt = _view(px, N), _view(pw, N), _view(po, N), _view(pc, N, C.c_int32)
        held = out[N - 1]
        out[:] = 2.0 * x + w
        cnt[:] = np.arange(N)
        cnt[N - 5:] = -1
        s = float(np.sum(x))
        if fault == "store behind out":
            _view(po, N + 1)[N] = 1.0
        elif fault == "store in front of out":
            _view(po, N, first=-1)[0] = 1.0
        elif fault == "store at the far end of the guard behind cnt":
            _view(pc, N + G.guard_elems(np.int32), C.c_int32)[-1] = -1
        elif fault == "store at the far end of the guard in front of out":
            _view(po, N, first=-G.guard_elems(np.float64))[0] = 0.0
        elif fault == "modify const w":
            w[3] = -w[3]
        elif fault == "flip the sign of a zero in const x":
            x[7] = -0.0
        elif fault == "read behind x into out":
            out[N - 1] += 1e-300 * _view(px, N + 1)[N]
        elif fault == "read in front of w into s":
            s += 1e-300 * float(_view(pw, N, first=-1)[0])
        elif fault == "leave out unwritten":
            out[N - 1] = held                    # a last lane masked off by mistake: the element keeps what it held
        else:
            assert fault is None
        return {"rc": 0, "s": s}
    return call


def arguments():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(N)
    x[7] = 0.0
    return [G.Arg("x", "in", x), G.Arg("w", "in", rng.standard_normal(N)), G.Arg("out", "out", shape=(N,)),
            G.Arg("cnt", "out", shape=(N,), dtype=np.int32), G.Arg("absent", "out")]


def run(where, fault):
    return G.run_guarded("standin", arguments(), standin(fault), where)


@pytest.mark.parametrize("where", WHERE)
def test_clean_standin_passes(where):
    outs, scal = run(where, None)
    args = arguments()
    assert np.array_equal(outs["out"], 2.0 * args[0].value + args[1].value)
    assert outs["cnt"].dtype == np.int32 and (outs["cnt"][N - 5:] == -1).all() and outs["cnt"][N - 6] == N - 6
    assert scal["rc"] == 0 and scal["s"] == float(np.sum(args[0].value))


CAUGHT = [
    ("store behind out", r"guards = nan\]: out: 1 guard element\(s\) behind the payload .* first at offset 300 of a payload of 300"),
    ("store in front of out", r"guards = nan\]: out: 1 guard element\(s\) in front of the payload .* first at offset -1 "),
    ("store at the far end of the guard behind cnt", r"guards = nan\]: cnt: 1 guard element\(s\) behind .* first at offset %d "
     % (N + G.guard_elems(np.int32) - 1)),
    ("store at the far end of the guard in front of out", r"guards = nan\]: out: 1 guard element\(s\) in front .* first at offset -%d "
     % G.guard_elems(np.float64)),
    ("modify const w", r"guards = nan\]: const input w: 1 of 300 elements changed bits; the first at flat index 3:"),
    ("flip the sign of a zero in const x", r"guards = nan\]: const input x: 1 of 300 elements changed bits; the first at flat index 7: -0\.0"),
    ("read behind x into out", r"guards = nan\]: output out against the plain call's: 1 of 300 elements changed bits; the first at "
                               r"flat index 299: nan"),
    ("read in front of w into s", r"guards = nan\]: scalar s against the plain call's: 1 of 1 elements changed bits"),
    ("leave out unwritten", r"guards = nan\]: output out against the plain call's: 1 of 300 elements changed bits; the first at "
                            r"flat index 299: nan"),
]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("fault,message", CAUGHT, ids=[c[0].replace(" ", "-") for c in CAUGHT])
def test_each_planted_violation_is_caught_and_named(where, fault, message):
    with pytest.raises(AssertionError, match=message):
        run(where, fault)


@pytest.mark.parametrize("where", WHERE)
def test_the_finite_fill_alone_shows_a_read_too(where):
    """an entry that multiplied what it read behind x by zero would hide a finite value and show a NaN; one that compares
    (max, a neighbour search) hides a NaN and shows a finite value: the protocol runs both fills"""
    def call(bufs):
        x, out = _view(G.ptr_of(bufs["x"]), N + 1 if is_banded(bufs["x"]) else N), _view(G.ptr_of(bufs["out"]), N)
        out[:] = x[:N]
        out[0] = np.fmax.reduce(x)                       # a NaN loses every comparison
        return {}
    args = [G.Arg("x", "in", np.linspace(2.0, 1.0, N)), G.Arg("out", "out", shape=(N,))]
    with pytest.raises(AssertionError, match=r"guards = sentinel\]: output out against the plain call's: 1 of 300"):
        G.run_guarded("standin", args, call, where)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32, np.int64])
@pytest.mark.parametrize("shape", [1, 300, (37, 33), (3, 4, 5)])
def test_banded_layout(where, dtype, shape):
    for fill in G.FILLS:
        p, h = G.banded(shape, dtype, fill, where, name="b")
        numel = int(np.prod(shape))
        g = h.guard
        assert g >= G.GUARD_MIN_ELEMS and g * np.dtype(dtype).itemsize >= G.GUARD_MIN_BYTES
        assert (g * np.dtype(dtype).itemsize) % 4096 == 0
        assert tuple(p.shape) == ((shape,) if np.ndim(shape) == 0 else tuple(shape)) and h.numel == numel
        assert G.ptr_of(p) - G.ptr_of(h.flat) == g * np.dtype(dtype).itemsize          # the payload is the middle of the flat buffer
        assert G.ptr_of(p) % 256 == G.ptr_of(h.flat) % 256                               # ... on the allocation's own alignment
        flat = G._to_numpy(h.flat)
        assert flat.size == 2 * g + numel
        assert (G._to_numpy(G._int_view(h.flat)) == G.pattern_bits(fill, dtype)).all()  # one pattern in every element
        if np.dtype(dtype).kind == "f":
            assert np.isnan(flat).all() if fill == "nan" else (np.isfinite(flat).all() and (np.abs(flat) > 1e15).all())
        h.assert_untouched()
        p[...] = 0                                                                       # the payload is the caller's
        h.assert_untouched()
    assert G.pattern_bits("nan", dtype) != G.pattern_bits("sentinel", dtype)


def test_the_nan_fill_is_quiet():
    for dt, quiet_bit in ((np.float64, 1 << 51), (np.float32, 1 << 22)):
        v = G.pattern_value("nan", dt)
        assert np.isnan(v) and G.pattern_bits("nan", dt) > 0 and G.pattern_bits("nan", dt) & quiet_bit
        assert np.isfinite(G.pattern_value("sentinel", dt))


@pytest.mark.parametrize("where", WHERE)
def test_same_bits_is_about_bits(where):
    a = np.array([0.0, np.nan, 1.0, -3.5])
    if where == "cpu":
        import torch
        a = torch.from_numpy(a)
    snap = G.snapshot(a)
    G.assert_same_bits(a, snap, "a")                       # a NaN has its own bits
    a[0] = -0.0                                            # equal as a value, not in bits
    with pytest.raises(AssertionError, match=r"^a: 1 of 4 elements changed bits; the first at flat index 0: -0\.0 \(0x8000000000000000\) "
                                             r"where the snapshot has 0\.0 \(0x0\)"):
        G.assert_same_bits(a, snap, "a")
    a[0] = 0.0
    G.assert_same_bits(a, snap, "a")
    with pytest.raises(AssertionError, match="3 elements, the snapshot has 4"):
        G.assert_same_bits(a[:3], snap, "a")
    i = np.arange(6, dtype=np.int32).reshape(2, 3)
    snap = G.snapshot(i)
    i[1, 2] = -1
    with pytest.raises(AssertionError, match=r"^nbr: 1 of 6 elements changed bits; the first at flat index 5: -1 \(0xffffffff\) where the "
                                             r"snapshot has 5 "):
        G.assert_same_bits(i, snap, "nbr")
    G.assert_same_bits(2.5, G.snapshot(2.5), "scalar")
    with pytest.raises(AssertionError, match="^info: 1 of 1"):
        G.assert_same_bits(3, G.snapshot(0), "info")


def test_compare_hook_replaces_the_bitwise_check_for_named_results_only():
    seen, calls = [], []

    def call(bufs):
        out = _view(G.ptr_of(bufs["out"]), N)
        out[:] = 1.0
        out[0] += (2.0 ** -52) * (len(calls) % 4)         # a result that moves from call to call
        calls.append(1)
        return {"s": 1.0}

    def close(name, a, b):
        seen.append(name)
        assert np.abs(a - b).max() <= 1e-14
    args = [G.Arg("out", "out", shape=(N,))]
    G.run_guarded("standin", args, call, "numpy", compare={"out": close})
    assert seen == ["out", "out", "out"]
    with pytest.raises(AssertionError, match=r"plain, again\]: output out against the plain call's"):
        G.run_guarded("standin", args, call, "numpy")

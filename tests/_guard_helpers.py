"""Guard bands: where an entry reads and writes, not what it computes.

Every other test hands the library exact-size buffers and looks only inside them.  Here a buffer is the middle of a larger
allocation, `guard | payload | guard`, with both guards holding one known bit pattern; after the call the guards must still hold
it (nothing was stored outside the payload), every `const` input must have its bits (nothing was stored into it), and the
results must have the bits of a call on plain exact-size buffers, whichever pattern the guards hold (nothing was read from
outside the payload and used).  Everything is compared as integers: a NaN equals itself, -0.0 differs from 0.0, no tolerance.

Works on NumPy arrays (host-boundary entries) and on torch tensors of any device (device-pointer entries; `where="cpu"` lets the
host test drive the torch code without a GPU).  Neither torch nor the library is imported at module level.

`run_guarded` is the protocol of tests/test_gpu_guard_bands.py; tests/test_guard_helpers_host.py runs it on stand-in entries
that misbehave on purpose, to show that each kind of violation is caught and attributed to the right argument."""
import struct

import numpy as np

GUARD_MIN_ELEMS = 512           # two rows of a 256-wide panel
GUARD_MIN_BYTES = 4096          # and a whole number of 256-byte lines: the payload keeps the alignment of a plain allocation

# One pattern in every element.  "nan": a quiet NaN (sign 0, exponent all ones, top mantissa bit set) with a payload that no
# arithmetic produces; "sentinel": a finite value (of the order of 1e50 / 1e16) of no special meaning.  The integer types have no NaN:
# their "nan" fill is the bit pattern of the NaN of their width, so that the two fills still differ.
_PATTERNS = {
    ("nan", 8): 0x7FF85EED0BADC0DE,
    ("sentinel", 8): 0x4A5AC3D2E1F09687,
    ("nan", 4): 0x7FC5EED1,
    ("sentinel", 4): 0x5A5AC3D2,
}
FILLS = ("nan", "sentinel")

_INT_OF_SIZE = {8: np.int64, 4: np.int32}


def pattern_bits(fill, dtype):
    """the fill's bit pattern for `dtype` as a signed integer of the same width (what the integer views are compared with)"""
    size = np.dtype(dtype).itemsize
    p = _PATTERNS[(fill, size)]
    return p - (1 << (8 * size)) if p >> (8 * size - 1) else p


def pattern_value(fill, dtype):
    """the fill as a value of `dtype` (for messages and for the host test)"""
    size = np.dtype(dtype).itemsize
    return np.array([_PATTERNS[(fill, size)]], dtype={8: np.uint64, 4: np.uint32}[size]).view(np.dtype(dtype))[0]


def _np_dtype(dtype):
    """NumPy dtype of a NumPy or torch dtype"""
    try:
        return np.dtype(dtype)
    except TypeError:
        return np.dtype(str(dtype).replace("torch.", ""))


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _int_view(x):
    """flat integer view (same width, same memory) of a contiguous NumPy array or torch tensor"""
    if _is_torch(x):
        import torch
        assert x.is_contiguous()
        return x.reshape(-1).view({8: torch.int64, 4: torch.int32}[x.element_size()])
    assert x.flags["C_CONTIGUOUS"]
    return x.reshape(-1).view(_INT_OF_SIZE[x.dtype.itemsize])


def _to_numpy(iv):
    return iv.cpu().numpy() if _is_torch(iv) else iv


def guard_elems(dtype):
    """elements of one guard: at least GUARD_MIN_ELEMS and at least GUARD_MIN_BYTES, a whole number of 4096-byte pages"""
    size = _np_dtype(dtype).itemsize
    nbytes = max(GUARD_MIN_ELEMS * size, GUARD_MIN_BYTES)
    nbytes = -(-nbytes // GUARD_MIN_BYTES) * GUARD_MIN_BYTES
    return nbytes // size


class Banded(object):
    """handle on one `guard | payload | guard` allocation"""

    def __init__(self, flat, guard, numel, fill, name):
        self.flat, self.guard, self.numel, self.fill, self.name = flat, guard, numel, fill, name
        self.bits = pattern_bits(fill, _np_dtype(flat.dtype))

    def _first_changed(self, lo, hi):
        g = _to_numpy(_int_view(self.flat)[lo:hi])
        bad = np.flatnonzero(g != self.bits)
        return None if bad.size == 0 else (int(bad[0]), int(bad.size), int(g[bad[0]]))

    def assert_untouched(self):
        """both guards still hold the pattern, bit for bit; else AssertionError naming the buffer and the first changed element's
        offset relative to the payload (-1 = the element in front of it, numel = the first one behind it)"""
        g, n = self.guard, self.numel
        for side, lo, hi, base in (("in front of", 0, g, -g), ("behind", g + n, g + n + g, n)):
            hit = self._first_changed(lo, hi)
            if hit is not None:
                at, count, got = hit
                raise AssertionError(
                    "%s: %d guard element(s) %s the payload were written; the first at offset %d of a payload of %d elements "
                    "(%d %s it) now holds bits 0x%x, the %s fill is 0x%x"
                    % (self.name, count, side, base + at, n, (g - at) if base < 0 else at + 1, side,
                       got & ((1 << (8 * _np_dtype(self.flat.dtype).itemsize)) - 1), self.fill,
                       _PATTERNS[(self.fill, _np_dtype(self.flat.dtype).itemsize)]))


def banded(shape, dtype, fill, where, name="buffer"):
    """One flat allocation `guard | payload | guard`, every element (payload included) holding the `fill` pattern.
    `where`: "numpy", or a torch device (object or string).  Returns (payload view of `shape`, handle)."""
    assert fill in FILLS, fill
    shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(s) for s in shape)
    numel = int(np.prod(shape, dtype=np.int64))
    g = guard_elems(dtype)
    if isinstance(where, str) and where == "numpy":
        flat = np.empty(g + numel + g, dtype=np.dtype(dtype))
        _int_view(flat)[:] = pattern_bits(fill, flat.dtype)
    else:
        import torch
        tdtype = dtype if isinstance(dtype, torch.dtype) else getattr(torch, np.dtype(dtype).name)
        flat = torch.empty(g + numel + g, dtype=tdtype, device=where)
        _int_view(flat).fill_(pattern_bits(fill, _np_dtype(tdtype)))
    payload = flat[g:g + numel].reshape(shape)
    return payload, Banded(flat, g, numel, fill, name)


def snapshot(x):
    """the bits of x (NumPy array, torch tensor, or a Python / ctypes-derived scalar), copied"""
    if _is_torch(x):
        return _int_view(x.detach().contiguous()).clone()
    a = np.ascontiguousarray(x)
    if a.dtype.kind == "f" and a.dtype.itemsize not in _INT_OF_SIZE:
        a = a.astype(np.float64)
    if a.dtype == np.bool_:
        a = a.astype(np.int32)
    return _int_view(a).copy()


def assert_same_bits(x, snap, name):
    """x has exactly the bits of the snapshot; else AssertionError naming `name`, the first differing element and both values"""
    now = snapshot(x)
    if _is_torch(now) and _is_torch(snap):
        import torch
        assert now.shape == snap.shape, "%s: %d elements, the snapshot has %d" % (name, now.numel(), snap.numel())
        if torch.equal(now, snap):
            return
    a, b = _to_numpy(now), _to_numpy(snap)
    assert a.shape == b.shape, "%s: %d elements, the snapshot has %d" % (name, a.size, b.size)
    bad = np.flatnonzero(a != b)
    if bad.size:
        i = int(bad[0])
        fl = {8: np.float64, 4: np.float32}[a.dtype.itemsize]
        kind = _np_dtype(x.dtype).kind if _is_torch(x) else np.asarray(x).dtype.kind
        show = (lambda v: repr(float(v.view(fl)[0]))) if kind == "f" else (lambda v: repr(int(v[0])))
        raise AssertionError("%s: %d of %d elements changed bits; the first at flat index %d: %s (0x%x) where the snapshot has "
                             "%s (0x%x)" % (name, bad.size, a.size, i, show(a[i:i + 1]), int(a[i]) & ((1 << 8 * a.dtype.itemsize) - 1),
                                            show(b[i:i + 1]), int(b[i]) & ((1 << 8 * b.dtype.itemsize) - 1)))


def ptr_of(buf):
    """the address an entry gets: None for NULL, data_ptr() of a tensor, the data address of an array"""
    if buf is None:
        return None
    return int(buf.data_ptr()) if _is_torch(buf) else int(buf.ctypes.data)


def double_bits(v):
    return struct.unpack("<q", struct.pack("<d", float(v)))[0]


# ---- the protocol -----------------------------------------------------------------------------------------------------------

class Arg(object):
    """One pointer argument of an entry.  role "in": `value` goes in and must come out with its bits (a `const` pointer);
    "out": the entry writes all of shape x dtype; "inout": `value` goes in, the entry's result comes out in the same memory.
    value None with role "in" / "out" and no shape = the argument is passed as NULL."""

    def __init__(self, name, role, value=None, shape=None, dtype=np.float64, where=None):
        assert role in ("in", "out", "inout")
        self.name, self.role, self.value = name, role, value
        self.where = where                    # None: where run_guarded says; "numpy" for a host pointer among device ones
        if value is not None:
            value = np.ascontiguousarray(value)
            self.value, shape, dtype = value, value.shape, value.dtype
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.null = value is None and shape is None


def _plain(arg, where):
    """an exact-size buffer of its own: the input's values, zeros for an output"""
    if isinstance(where, str) and where == "numpy":
        return np.zeros(arg.shape, dtype=arg.dtype) if arg.value is None else arg.value.copy()
    import torch
    if arg.value is None:
        return torch.zeros(arg.shape, dtype=getattr(torch, arg.dtype.name), device=where)
    return torch.from_numpy(arg.value.copy()).to(where)


def _store(payload, value):
    if _is_torch(payload):
        import torch
        payload.copy_(torch.from_numpy(value))
    else:
        payload[...] = value


def run_guarded(entry, args, call, where, before_call=None, compare=None):
    """The runs of one case: plain exact-size buffers, twice, then every pointer argument banded, once per fill.

    call(bufs) runs the entry on bufs[name] (buffer or None) and returns a dict of its scalar results (return code, logdet, ...).
    before_call(): e.g. torch.cuda.synchronize, between filling the buffers and the call.
    After each banded run: every guard untouched, every "in" argument's bits unchanged (also in the plain run).  Then every "out"
    / "inout" buffer and every scalar of the later runs against the first plain run's: bit for bit, or through
    compare[name](name, plain_array, other_array) -> None / AssertionError for the names in `compare` (a dict), where a route's own
    two plain calls are known not to agree in bits.  The second plain run is there to tell such a route (it fails as "plain,
    again") from one whose result moves with what lies around its buffers.
    Returns the plain run's outputs {name: NumPy array} and scalars."""
    compare = compare or {}
    runs = []
    for fill in (None, None) + FILLS:
        tag = "%s [%s]" % (entry, ("plain, again" if runs else "plain") if fill is None else "guards = " + fill)
        bufs, handles, snaps = {}, [], {}
        for a in args:
            if a.null:
                bufs[a.name] = None
                continue
            if fill is None:
                buf = _plain(a, a.where or where)
            else:
                buf, h = banded(a.shape, a.dtype, fill, a.where or where, name="%s: %s" % (tag, a.name))
                handles.append(h)
                if a.value is not None:
                    _store(buf, a.value)
            bufs[a.name] = buf
            if a.role == "in":
                snaps[a.name] = snapshot(buf)
        if before_call is not None:
            before_call()
        scalars = call(bufs)
        for h in handles:
            h.assert_untouched()
        for a in args:
            if a.role == "in" and not a.null:
                assert_same_bits(bufs[a.name], snaps[a.name], "%s: const input %s" % (tag, a.name))
        outs = {a.name: _to_numpy(bufs[a.name].detach().clone() if _is_torch(bufs[a.name]) else bufs[a.name].copy())
                for a in args if a.role != "in" and not a.null}
        runs.append((tag, outs, dict(scalars or {})))
    tag0, outs0, scal0 = runs[0]
    for tag, outs, scal in runs[1:]:
        assert sorted(scal) == sorted(scal0)
        for k in sorted(scal0):
            if k in compare:
                compare[k](k, scal0[k], scal[k])
            else:
                assert_same_bits(scal[k], snapshot(scal0[k]), "%s: scalar %s against the plain call's" % (tag, k))
        for k in sorted(outs0):
            if k in compare:
                compare[k](k, outs0[k], outs[k])
            else:
                assert_same_bits(outs[k], snapshot(outs0[k]), "%s: output %s against the plain call's" % (tag, k))
    return outs0, scal0

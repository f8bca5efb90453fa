"""
Operand placement for tests: the same logical operand at another address and in other surroundings.

A result may depend on the logical operand only -- never on where it lies in memory (16-byte aligned or not: the library's loaders
choose between 16-byte vector loads and scalar loads by the pointer) and never on what lies next to it (the columns behind k of a
row stride ld > k, the rows behind n_verts of a padded batch, the memory in front of and behind the array).

    place(array, offset_elems=1, ld=k + 5, pad="+inf")

builds the operand inside a larger flat buffer whose every other element holds the fill and returns a CONTIGUOUS view of the padded
shape (..., rows, ld); the logical operand is view[..., :R, :W].  tests/test_placement_cpu.py pins this module.
"""
import numpy as np
import torch

PADS = ("nan", "+inf", "-inf", "huge", "tiny")

# offsets (in elements) at which a view of that dtype leaves the 16-byte grid
OFFSETS = {torch.float32: (1, 2, 3), torch.int32: (1, 2, 3), torch.float64: (1,), torch.float16: (1, 2, 3, 4, 5, 6, 7)}

GUARD_BYTES = 256       # filled memory in front of and behind every view (a multiple of 16)

_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


INT_FILL = 2 ** 30      # index padding: outside every mesh of the tests


def fill_value(dtype, pad):
    """the number a fill name stands for in `dtype`.  None: NaN (floating point) or INT_FILL (integers, an index no mesh here has);
    integer dtypes otherwise take an integer `pad` as it is"""
    if not dtype.is_floating_point:
        if pad is None:
            return INT_FILL
        if isinstance(pad, str):
            raise ValueError(f"an integer operand needs an integer fill, not {pad!r}")
        return int(pad)
    if pad is None:
        pad = "nan"
    fi = torch.finfo(dtype)
    if pad == "nan":
        return float("nan")
    if pad == "+inf":
        return float("inf")
    if pad == "-inf":
        return float("-inf")
    if pad == "huge":
        return fi.max / 2          # half the largest finite value
    if pad == "tiny":
        return fi.smallest_normal * fi.eps      # the smallest subnormal
    raise ValueError(f"unknown fill {pad!r} (one of {PADS})")


def bits(t):
    """the tensor's bit patterns as integers of the same width (NaN compares equal to itself)"""
    return t.contiguous().view(_BITS[t.element_size()])


def mod16(t):
    return t.data_ptr() % 16


def _aligned_buffer(n, dtype, device, value):
    """n elements of `dtype` that start on a 16-byte boundary, all set to `value`"""
    isz = torch.empty((), dtype=dtype).element_size()
    raw = torch.empty(n + 16 // isz, dtype=dtype, device=device)
    skip = (-raw.data_ptr() % 16) // isz
    buf = raw[skip:skip + n]
    assert buf.data_ptr() % 16 == 0
    buf.fill_(value)
    return buf


def place(array, *, offset_elems=0, ld=None, rows=None, pad=None, slice_of_batch=False, device=None):
    """`array` (numpy or torch, at least 1-D) inside a larger flat buffer filled with `pad`.
    offset_elems   the view starts that many elements behind a 16-byte boundary
    ld             row stride > the last dimension: the columns behind it hold the fill
    rows           row count > the second-to-last dimension (padded-batch entries): the rows behind it hold the fill
    slice_of_batch the view is pairs 1: of a batch one larger that starts on a 16-byte boundary (what a shard of a batch is): its
                   address is (elements per pair * element size) mod 16
    Returns the contiguous view of shape (..., rows, ld).  Asserted here: contiguity, data_ptr() % 16, that the logical content
    equals `array` bit for bit, and that every other element of the buffer -- guards included -- holds the fill."""
    src = array if isinstance(array, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(array))
    if device is None:
        device = src.device
    device = torch.device(device)
    src = src.to(device)
    dtype, isz = src.dtype, src.element_size()
    if src.dim() < 1:
        raise ValueError("place: the operand needs at least one dimension")
    shape = list(src.shape)
    W = shape[-1]
    if ld is not None:
        if ld < W:
            raise ValueError("place: ld below the logical width")
        shape[-1] = ld
    if rows is not None:
        if src.dim() < 2 or rows < shape[-2]:
            raise ValueError("place: rows below the logical row count")
        shape[-2] = rows
    if offset_elems and slice_of_batch:
        raise ValueError("place: offset_elems and slice_of_batch are two placements, not one")
    if offset_elems < 0 or offset_elems * isz >= 16:
        raise ValueError("place: offset_elems must stay inside one 16-byte line")
    fill = fill_value(dtype, pad)
    n = int(np.prod(shape))
    guard = GUARD_BYTES // isz
    if slice_of_batch:
        if src.dim() < 2:
            raise ValueError("place: a batch slice needs a batch axis")
        per_pair = n // shape[0]
        start = guard + per_pair                                 # pair 0 of the larger batch is fill
        want = (per_pair * isz) % 16
    else:
        start = guard + offset_elems
        want = (offset_elems * isz) % 16
    buf = _aligned_buffer(start + n + guard + 16 // isz, dtype, device, fill)
    view = buf[start:start + n].view(shape)
    idx = tuple(slice(0, s) for s in src.shape)
    view[idx] = src
    # ---- what the tests rely on
    assert view.is_contiguous() and tuple(view.shape) == tuple(shape)
    assert view.data_ptr() == buf.data_ptr() + start * isz and view.data_ptr() % 16 == want, (view.data_ptr() % 16, want)
    assert torch.equal(bits(view[idx]), bits(src))
    mask = torch.ones(buf.shape, dtype=torch.bool, device=device)
    mask[start:start + n].view(shape)[idx] = False
    fb = bits(torch.full((1,), fill, dtype=dtype, device=device))
    assert bool((bits(buf)[mask] == fb).all())
    return view


def logical(view, like):
    """the logical operand of a placed view: its leading block of the shape of `like`"""
    return view[tuple(slice(0, s) for s in like.shape)]


def placements(dtype, *, lds=(), rows=(), squares=(), batch=True):
    """The placements of one operand as (name, keywords for place()): every offset of the dtype, the batch slice, every fill with
    each padding asked for (row strides `lds`, row counts `rows`, both at once `squares`) -- without any padding the five fills
    surround the array as it is, front and back guards --, and the largest offset combined with the +inf fill once."""
    out = [("off%d" % o, dict(offset_elems=o)) for o in OFFSETS[dtype]]
    if batch:
        out.append(("slice", dict(slice_of_batch=True)))
    geoms = ([("ld%d" % v, dict(ld=v)) for v in lds] + [("rows%d" % v, dict(rows=v)) for v in rows] +
             [("sq%d" % v, dict(ld=v, rows=v)) for v in squares])
    if dtype.is_floating_point:
        for gname, geom in geoms or [("guard", {})]:
            out += [("%s/%s" % (gname, p), dict(pad=p, **geom)) for p in PADS]
        gname, geom = (geoms or [("guard", {})])[-1]
        o = OFFSETS[dtype][-1]
        out.append(("off%d/%s/+inf" % (o, gname), dict(offset_elems=o, pad="+inf", **geom)))
        if batch:
            out.append(("slice/%s/huge" % gname, dict(slice_of_batch=True, pad="huge", **geom)))
    else:
        out += [(gname, geom) for gname, geom in geoms]
    return out


class PointerRecorder:
    """Wraps one entry of the loaded library (eng.lib.dm_*) and records the pointer arguments of every call, so that a test can
    assert that the placed address is what the library received -- not a copy torch made on the way.

        with PointerRecorder(eng.lib, "dm_project") as rec:
            eng.project(...)
        assert rec.saw(Phi)
    """

    def __init__(self, lib, name):
        self.lib, self.name, self.calls = lib, name, []

    def __enter__(self):
        import ctypes
        self._orig = getattr(self.lib, self.name)

        def shim(*args):
            self.calls.append([a.value for a in args if isinstance(a, ctypes.c_void_p)])
            return self._orig(*args)
        setattr(self.lib, self.name, shim)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self._orig)
        return False

    def saw(self, *tensors):
        return bool(self.calls) and all(any(t.data_ptr() in c for c in self.calls) for t in tensors)

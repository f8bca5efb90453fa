"""
CPU: pins tests/placement.py (alignment arithmetic for every dtype, fills, logical content, contiguity, the batch-slice form) and
the condition the inputs of tests/test_gpu_placement.py must satisfy: the float64 oracle, run on the logical operands cut out of
every placement's buffer, is finite and identical for every fill -- the reference alone never sees the padding.
"""
import numpy as np
import pytest
import torch

import placement as pl
import placement_cases as pc

DTYPES = (torch.float32, torch.float64, torch.float16, torch.int32)


def _sample(dtype, shape, seed=0):
    rng = np.random.default_rng(seed)
    if dtype.is_floating_point:
        return torch.as_tensor(rng.standard_normal(shape)).to(dtype)
    return torch.as_tensor(rng.integers(0, 100, shape).astype(np.int32))


def test_fill_values():
    for dt in (torch.float16, torch.float32, torch.float64):
        fi = torch.finfo(dt)
        one = lambda p: torch.full((1,), pl.fill_value(dt, p), dtype=dt)
        assert torch.isnan(one("nan")).all() and torch.isnan(one(None)).all()
        assert one("+inf").item() == float("inf") and one("-inf").item() == float("-inf")
        huge, tiny = one("huge"), one("tiny")
        assert torch.isfinite(huge).all() and huge.item() == fi.max / 2 and (huge * 2).item() == fi.max      # half the largest finite value
        assert tiny.item() > 0 and (tiny / 2).item() == 0.0 and tiny.item() < fi.smallest_normal            # the smallest subnormal
        assert pl.bits(tiny).item() == 1
    assert pl.fill_value(torch.int32, None) == pl.INT_FILL and pl.fill_value(torch.int32, -7) == -7
    with pytest.raises(ValueError):
        pl.fill_value(torch.int32, "nan")
    with pytest.raises(ValueError):
        pl.fill_value(torch.float32, "big")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_offsets_leave_the_16_byte_grid(dtype):
    isz = torch.empty((), dtype=dtype).element_size()
    assert pl.OFFSETS[dtype] == tuple(range(1, 16 // isz))             # every element offset inside one 16-byte line
    src = _sample(dtype, (2, 7, 5))
    v0 = pl.place(src)
    assert v0.data_ptr() % 16 == 0 and v0.is_contiguous() and torch.equal(v0, src)
    for off in pl.OFFSETS[dtype]:
        v = pl.place(src, offset_elems=off)
        assert v.data_ptr() % 16 == off * isz and v.is_contiguous() and v.shape == src.shape
        assert torch.equal(pl.bits(v), pl.bits(src))
    with pytest.raises(ValueError):
        pl.place(src, offset_elems=16 // isz)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64, torch.float16), ids=str)
@pytest.mark.parametrize("pad", pl.PADS)
def test_padding_and_guards_hold_the_fill(dtype, pad):
    src = _sample(dtype, (2, 7, 5), seed=1)
    v = pl.place(src, offset_elems=1, ld=9, rows=10, pad=pad)
    assert v.shape == (2, 10, 9) and v.is_contiguous()
    assert torch.equal(pl.bits(pl.logical(v, src)), pl.bits(src))
    fb = pl.bits(torch.full((1,), pl.fill_value(dtype, pad), dtype=dtype)).item()
    assert bool((pl.bits(v[:, :, 5:]) == fb).all()) and bool((pl.bits(v[:, 7:, :]) == fb).all())
    # the guards: the storage in front of and behind the view
    isz = src.element_size()
    whole = torch.empty(0, dtype=dtype).set_(v.untyped_storage())
    first = (v.data_ptr() - whole.data_ptr()) // isz
    guard = pl.GUARD_BYTES // isz
    assert first >= guard and whole.numel() - (first + v.numel()) >= guard
    assert bool((pl.bits(whole[first - guard:first]) == fb).all())
    assert bool((pl.bits(whole[first + v.numel():first + v.numel() + guard]) == fb).all())


def test_place_refuses_what_it_cannot_build():
    src = _sample(torch.float32, (2, 7, 5))
    for kw in (dict(ld=4), dict(rows=6), dict(offset_elems=1, slice_of_batch=True), dict(offset_elems=-1)):
        with pytest.raises(ValueError):
            pl.place(src, **kw)
    with pytest.raises(ValueError):
        pl.place(_sample(torch.float32, (5,)), slice_of_batch=True)


@pytest.mark.parametrize("dtype,shape,ld,want", [(torch.float32, (3, 333, 15), None, 12), (torch.float32, (3, 333, 15), 18, 8),
                                                 (torch.float64, (3, 17, 15), None, 8), (torch.float64, (3, 16, 16), None, 0),
                                                 (torch.float16, (3, 333, 24), None, 0), (torch.int32, (3, 517), None, 4)], ids=str)
def test_batch_slice(dtype, shape, ld, want):
    """pairs 1: of a batch one larger: the address is (elements per pair x element size) mod 16 -- 333 x 15 floats put a shard
    12 bytes off the grid, a 17 x 15 float64 map 8 bytes; fp16 features with D % 8 == 0 stay on it"""
    src = _sample(dtype, shape, seed=2)
    v = pl.place(src, slice_of_batch=True, ld=ld)
    assert v.data_ptr() % 16 == want and v.is_contiguous()
    assert torch.equal(pl.bits(pl.logical(v, src)), pl.bits(src))


def test_placements_enumerates_what_the_gpu_tests_walk():
    names = [n for n, _ in pl.placements(torch.float32, lds=(16, 20))]
    assert names[:4] == ["off1", "off2", "off3", "slice"]
    assert all(f"ld{ld}/{p}" in names for ld in (16, 20) for p in pl.PADS)
    assert "off3/ld20/+inf" in names and "slice/ld20/huge" in names and len(names) == len(set(names))
    assert [n for n, _ in pl.placements(torch.float64)] == ["off1", "slice"] + ["guard/" + p for p in pl.PADS] + ["off1/guard/+inf", "slice/guard/huge"]
    assert len(pl.placements(torch.float16, batch=False)) == 7 + 5 + 1
    assert [n for n, _ in pl.placements(torch.int32)] == ["off1", "off2", "off3", "slice"]
    sq = dict(pl.placements(torch.float64, squares=(19,)))
    assert sq["sq19/nan"] == dict(pad="nan", ld=19, rows=19) and sq["off1/sq19/+inf"] == dict(offset_elems=1, pad="+inf", ld=19, rows=19)


def test_pointer_recorder():
    import ctypes

    class Lib:
        def dm_x(self, *a):
            return 0
    lib = Lib()
    orig = lib.dm_x
    t, u = torch.zeros(4), torch.zeros(4)
    with pl.PointerRecorder(lib, "dm_x") as rec:
        assert lib.dm_x(ctypes.c_void_p(t.data_ptr()), 3, ctypes.c_void_p(0)) == 0
    assert rec.saw(t) and not rec.saw(u) and not rec.saw(t, u)
    assert lib.dm_x == orig and not pl.PointerRecorder(lib, "dm_x").saw(t)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.all_cases(), ids=pc.case_id)
def test_oracle_never_sees_the_padding(case):
    """every case of tests/test_gpu_placement.py: the oracle on the logical operands of each placement (all operands displaced,
    eigenvector arrays at ld = k + 5, every fill) is finite and bit-identical to the oracle on the operands as built"""
    entry, cfg = case
    ops = entry.build(cfg)
    ref = entry.oracle(ops, cfg)
    for name, r in ref.items():
        assert np.isfinite(np.asarray(r, np.float64)).all(), name
    for pad in pl.PADS:
        placed = {}
        for name, arr in ops.items():
            t = torch.as_tensor(arr)
            kw = dict(offset_elems=pl.OFFSETS[t.dtype][-1]) if t.dtype in pl.OFFSETS else {}
            if t.dtype.is_floating_point:
                kw["pad"] = pad
            if name in entry.ld_of:
                kw["ld"] = arr.shape[-1] + 5
            if name in entry.rows_of or name in entry.rows_only:
                kw["rows"] = arr.shape[-2] + 5
            placed[name] = np.ascontiguousarray(pl.logical(pl.place(t, **kw), t).numpy())
        got = entry.oracle(placed, cfg)
        for name, r in ref.items():
            assert np.array_equal(np.asarray(got[name]), np.asarray(r)), (pad, name)

"""JBU feature upsampling on the GPU (dm_jbu_filters_f32, dm_jbu_apply, MatchEngine.jbu_filters / jbu_apply / jbu_stack, the device route
of featup.upsamplers) against the float64 restatement tests/jbu_restate.py and the reference's recorded run tests/golden/fx_jbu.npz.

Kernel shapes (B, C, h, w), output (2h, 2w): (1, 1, 2, 2) -- a 4 x 4 output, where the reflection by 3 spans the whole image;
(2, 5, 3, 2) non-square; (1, 70, 5, 7): more than one pass of four channels and not a multiple of four; (1, 3, 9, 17): the output
18 x 34 is one source texel more than the apply kernel's 16 x 32 pixel tile in both directions (outputs are even, so one pixel more
cannot occur) and 612 pixels are two workgroups and a part of the filter kernel.
Bound: lift_checks.bound; for the fixture's cases with the floor it records, for the seeded stages with the floor jbu_checks.seeded_stage
measures: the reference's expressions in float32 on the CPU against the restatement on the same inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import jbu_checks as jc
import jbu_restate as rs
import lift_checks as lc
import placement as pl
from densematcher_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 2, 2), (2, 5, 3, 2), (1, 70, 5, 7), (1, 3, 9, 17)]


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                       # a copy: the shared references are read-only
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("shape", SHAPES)
def test_filters_against_the_restatement(eng, shape):
    st = jc.seeded_stage(*shape)
    got = eng.jbu_filters(dev(st["g"]), st["up"].packed(eng.device))
    assert got.shape == st["f64"].shape and got.dtype == torch.float32
    jc.check(got, st["f64"], st["floor_filters"], f"filters {shape} (floor {st['floor_filters']:.2e})")


@pytest.mark.parametrize("shape", SHAPES)
def test_apply_against_the_restatement(eng, shape):
    st = jc.seeded_stage(*shape)
    got = eng.jbu_apply(dev(st["src"]), dev(st["f32"]))
    assert got.shape == st["apply64"].shape and got.dtype == torch.float32 and got.is_contiguous()
    jc.check(got, st["apply64"], st["floor_apply"], f"apply {shape} (floor {st['floor_apply']:.2e})")


@pytest.mark.parametrize("shape", SHAPES[1:3])
def test_stage_module_on_the_device(eng, shape):
    st = jc.seeded_stage(*shape)
    up = st["up"].to(DEV)
    try:
        with torch.no_grad():
            got = up(dev(st["src"]), dev(st["g"]), route="device")
            jc.check(got, st["out64"], st["floor_stage"], f"stage {shape} (floor {st['floor_stage']:.2e})")
            jc.check(up(dev(st["src"]), dev(st["g"]), route="torch"), st["out64"], st["floor_stage"], f"stage {shape}, torch route on the GPU")
    finally:
        up.to("cpu")


# ---------------------------------------------------------------------------------------------------------------- 2. the stack
@pytest.mark.parametrize("c", jc.CASES)
def test_stack_against_the_reference_run(eng, c):
    d, m = jc.case(c), jc.model(c, DEV)
    src, img = dev(d["src"]), dev(d["img"])
    with torch.no_grad():
        y = m(src, img, route="device")
        auto = m(src, img, route="auto")
    assert y.dtype == torch.float32 and y.shape == d["y_ref32"].shape
    assert y.permute(0, 2, 3, 1).is_contiguous()                    # NCHW-shaped over channels-last memory
    jc.check(y, d["y_ref32"], d["f32_floor"], f"case {c}: device stack")
    jc.check(auto, d["y_ref32"], d["f32_floor"], f"case {c}: auto stack")
    # the stages on their own, so that a failure points to one
    x = src
    with torch.no_grad():
        for s in range(1, 5):
            x = m.upsample(x, img, getattr(m, f"up{s}"), route="device")
            jc.check(x, d[f"stage{s}"], d["f32_floor"], f"case {c}: device stage {s}")


def test_batching_and_chunking_give_the_same_bits(eng):
    m = jc.model("b", DEV)
    gen = torch.Generator().manual_seed(11)
    src, img = torch.randn((3, 5, 2, 3), generator=gen).to(DEV), torch.randn((3, 3, 32, 48), generator=gen).to(DEV)
    with torch.no_grad():
        together = m(src, img, route="device")
        alone = torch.cat([m(src[b:b + 1], img[b:b + 1], route="device") for b in range(3)])
        chunked = m(src, img, route="device", chunk=1)
        two = m(src, img, route="device", chunk=2)
    assert torch.equal(pl.bits(together), pl.bits(alone))
    assert torch.equal(pl.bits(together), pl.bits(chunked)) and torch.equal(pl.bits(together), pl.bits(two))
    assert not torch.equal(together[0], together[1])


def test_out_dtype_and_memory_format_convert_with_torch(eng):
    d, m = jc.case("a"), jc.model("a", DEV)
    with torch.no_grad():
        y = m(dev(d["src"]), dev(d["img"]), route="device")
        h = m(dev(d["src"]), dev(d["img"]), route="device", out_dtype=torch.float16, memory_format=torch.contiguous_format)
    assert h.dtype == torch.float16 and h.is_contiguous() and torch.equal(h, y.half())


# ---------------------------------------------------------------------------------------------------------------- 3. dtypes and layouts
def test_fp16_source_is_the_fp32_route_on_the_rounded_source(eng):
    st = jc.seeded_stage(*SHAPES[2])
    src, f32 = st["src"], dev(st["f32"])
    half = dev(src).half()
    a, b = eng.jbu_apply(half, f32), eng.jbu_apply(half.float(), f32)
    assert torch.equal(pl.bits(a), pl.bits(b))
    assert not torch.equal(a, eng.jbu_apply(dev(src), f32))


def test_fp16_output_is_the_rounded_fp32_output(eng):
    st = jc.seeded_stage(*SHAPES[2])
    src, f32 = st["src"], dev(st["f32"])
    o32 = eng.jbu_apply(dev(src), f32)
    for cl in (False, True):
        o16 = eng.jbu_apply(dev(src), f32, out_dtype=torch.float16, channels_last=cl)
        assert o16.dtype == torch.float16 and torch.equal(pl.bits(o16), pl.bits(o32.half()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_source_layout_makes_no_difference(eng, dtype):
    st = jc.seeded_stage(*SHAPES[2])
    src, f32 = st["src"], dev(st["f32"])
    s = dev(src).to(dtype)
    Bn, Cw, h, w = s.shape
    want = eng.jbu_apply(s, f32)
    cl = s.contiguous(memory_format=torch.channels_last)
    assert cl.stride(1) == 1
    assert torch.equal(pl.bits(eng.jbu_apply(cl, f32)), pl.bits(want))
    for pad in ("nan", "huge"):
        placed = pl.place(s, offset_elems=1, ld=w + 3, rows=h + 2, pad=pad, device=DEV)
        view = placed[..., :h, :w]
        assert not view.is_contiguous() and pl.mod16(view) != 0
        with pl.PointerRecorder(eng.lib, "dm_jbu_apply") as rec:
            got = eng.jbu_apply(view, f32)
        assert rec.saw(view), "the source was copied instead of being read where it lies"
        assert torch.equal(pl.bits(got), pl.bits(want)), pad


def test_output_layouts(eng):
    st = jc.seeded_stage(*SHAPES[2])
    src, f32 = st["src"], dev(st["f32"])
    s = dev(src)
    Bn, Cw, h, w = s.shape
    want = eng.jbu_apply(s, f32)
    cl = eng.jbu_apply(s, f32, channels_last=True)
    assert cl.shape == want.shape and cl.permute(0, 2, 3, 1).is_contiguous() and torch.equal(pl.bits(cl), pl.bits(want))
    # a given output: a view of a larger poisoned buffer; what lies around it is not written
    big = torch.full((Bn, Cw, 2 * h + 2, 2 * w + 3), float("nan"), device=DEV)
    view = big[:, :, 1:2 * h + 1, 2:2 * w + 2]
    assert eng.jbu_apply(s, f32, out=view) is view
    assert torch.equal(pl.bits(view), pl.bits(want))
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, :, 1:2 * h + 1, 2:2 * w + 2] = False
    assert bool(torch.isnan(big[mask]).all())


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_invalid_arguments(eng):
    null, P = C.c_void_p(0), (lambda t: C.c_void_p(t.data_ptr()))
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    lib, F32 = eng.lib, _lib.DM_F32
    for H, W in ((3, 8), (8, 2), (0, 8)):
        assert lib.dm_jbu_filters_f32(eng.ctx, 1, H, W, P(buf), P(buf), P(buf)) == _lib.DM_EINVAL, (H, W)
    for args in ((null, P(buf), P(buf)), (P(buf), null, P(buf)), (P(buf), P(buf), null)):
        assert lib.dm_jbu_filters_f32(eng.ctx, 1, 8, 8, *args) == _lib.DM_EINVAL
    assert lib.dm_jbu_filters_f32(eng.ctx, 0, 8, 8, P(buf), P(buf), P(buf)) == _lib.DM_EINVAL

    def apply(h=4, w=4, Cw=3, src=buf, filt=buf, out=buf, ss=None, os_=None, sd=F32, od=F32):
        ss = ss or (Cw * h * w, h * w, w, 1)
        os_ = os_ or (Cw * 4 * h * w, 4 * h * w, 2 * w, 1)
        return lib.dm_jbu_apply(eng.ctx, 1, Cw, h, w, sd, null if src is None else P(src), *ss, null if filt is None else P(filt), od,
                                null if out is None else P(out), *os_)
    assert apply() == _lib.DM_OK
    for kw in (dict(h=1), dict(w=1), dict(Cw=0), dict(src=None), dict(filt=None), dict(out=None), dict(sd=7), dict(od=7),
               dict(ss=(48, 16, -4, 1)),
               dict(os_=(192, 64, 8, 0)),                     # every column of a row on one address
               dict(os_=(192, 1, 8, 1)),                      # channels and columns on the same addresses
               dict(os_=(192, 64, 7, 1)),                     # rows that overlap
               dict(os_=(192, 3, 24, 1))):                    # channels-last strides with the column stride of NCHW
        assert apply(**kw) == _lib.DM_EINVAL, kw
    assert apply(os_=(192, 1, 24, 3)) == _lib.DM_OK            # channels-last
    # the Python layer
    st = jc.seeded_stage(*SHAPES[1])
    src, g, up = st["src"], st["g"], st["up"]
    with pytest.raises(ValueError, match="filters"):
        eng.jbu_apply(dev(src), dev(st["f32"])[:, :-1])
    with pytest.raises(ValueError, match="out"):
        eng.jbu_apply(dev(src), dev(st["f32"]), out=torch.empty(2, 5, 6, 5, device=DEV))
    with pytest.raises(ValueError, match="params"):
        eng.jbu_filters(dev(g), torch.zeros(10, device=DEV))
    with pytest.raises(ValueError):
        eng.jbu_filters(dev(g)[:, :, :3], up.packed(eng.device))       # H = 3
    up.train()
    try:
        with pytest.raises(ValueError, match="training"):
            up(dev(src), dev(g), route="device")
    finally:
        up.eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="twice"):
            up(dev(src), dev(g)[:, :, :5], route="device")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def test_featurizer_upsamples_on_the_way_into_lifting():
    from densematcher_amd.featup.upsamplers import JBUStack
    from densematcher_amd.model import MeshFeaturizer
    fx = lc.golden("fx_featurizer.npz")
    names = [str(n) for n in fx["names"]]
    Cw = fx["fts"].shape[1]
    torch.manual_seed(3)
    up = JBUStack(Cw).eval()
    model = MeshFeaturizer(None, (3, 1), int(fx["blocks"]), int(fx["width"]), num_features=Cw, upsampler=up)
    model.load_state_dict({n: torch.from_numpy(fx[f"p{i}"].copy()) for i, n in enumerate(names)}, strict=False)
    model = model.to(DEV).eval()
    mesh, ops, cams, fts, _ = lc.featurizer_inputs(DEV)
    views = fts.shape[0]
    lr, images = torch.randn(views, Cw, 2, 2).to(DEV), torch.randn(views, 3, 32, 32).to(DEV)
    with torch.no_grad():
        maps = model.upsampler(lr, images, route="device")
        want = model(None, mesh, ops, cams, return_mvfeatures=True, fts=maps, route="device")
        got = model(None, mesh, ops, cams, return_mvfeatures=True, fts_lr=lr, images=images, route="device")
        host = model(None, mesh, ops, cams, return_mvfeatures=True, fts_lr=lr.cpu(), images=images.cpu(), route="host")
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    floor = max(float(jc.case(c)["f32_floor"]) for c in jc.CASES)     # two fp32 routes of the same upsampling, then the same lifting
    jc.check(got[2], host[2].cpu().numpy(), floor, "multi-view features: device against the host route")

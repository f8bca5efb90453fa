"""The backward of the JBU apply on the GPU (dm_jbu_apply_bwd_filters_f32, dm_jbu_apply_bwd_source_f32, MatchEngine.jbu_apply_bwd_*,
featup.backward, the route="device", differentiable=True of featup.upsamplers) against float64 autograd of the reference's expressions
(tests/jbu_bwd_checks.py) within lift_checks.bound of the floor measured on the same inputs.

Shapes (B, C, h, w), jbu_bwd_checks.SHAPES: (1, 1, 2, 2) -- reflection and clamping span the whole image, every fold overlaps;
(2, 5, 3, 2) non-square; (1, 70, 5, 7): more than one pass of four channels, not a multiple of four, and a channel sum cut into nine
chunks; (1, 3, 9, 17): one texel more than the forward's 16 x 32 tile in both directions; (1, 3, 11, 11): ONE TEXEL MORE THAN THE SOURCE
KERNEL'S OWN 10 x 10 TILE in both directions, so that the first tile meets both borders and the second holds a single texel;
(1, 2, 24, 13): a row tile that touches no border and a padded window filled to its last column; (1, 2, 64, 128): 64 output tiles, the
smallest count at which the channel sum of gfilt is NOT cut into chunks."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import jbu_bwd_checks as bc
import jbu_checks as jc
import placement as pl
from densematcher_amd import _lib
from densematcher_amd.featup import backward as fb

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODULE_SHAPES = [bc.SHAPES[1], bc.SHAPES[2]]


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                       # a copy: the shared references are read-only
    return t if dtype is None else t.to(dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(pl.bits(a), pl.bits(b))


# ---------------------------------------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("shape", bc.SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_gfilt_against_the_oracle(eng, shape, dtype):
    o = bc.oracle(shape, "normal", dtype == torch.float16)
    src, gout = dev(o["src"], dtype), dev(o["gout"])
    got = eng.jbu_apply_bwd_filters(gout, src)
    assert got.shape == o["gfilt64"].shape and got.dtype == torch.float32 and got.is_contiguous()
    bc.check(got, o["gfilt64"], o["floor_gfilt"], f"gfilt {shape} {dtype} (floor {o['floor_gfilt']:.2e})")
    # the layouts of gout and of the source change no bit
    cl = gout.contiguous(memory_format=torch.channels_last)
    assert same_bits(eng.jbu_apply_bwd_filters(cl, src), got)
    assert same_bits(eng.jbu_apply_bwd_filters(gout, src.contiguous(memory_format=torch.channels_last)), got)


@pytest.mark.parametrize("shape", bc.SHAPES)
def test_gsrc_against_the_oracle(eng, shape):
    o = bc.oracle(shape)
    gout, filt = dev(o["gout"]), dev(o["filt"])
    got = eng.jbu_apply_bwd_source(gout, filt)
    assert got.shape == o["gsrc64"].shape and got.dtype == torch.float32 and got.is_contiguous()
    bc.check(got, o["gsrc64"], o["floor_gsrc"], f"gsrc {shape} (floor {o['floor_gsrc']:.2e})")
    cl = gout.contiguous(memory_format=torch.channels_last)
    assert shape[1] == 1 or cl.stride(1) == 1
    assert same_bits(eng.jbu_apply_bwd_source(cl, filt), got)
    half = eng.jbu_apply_bwd_source(gout, filt, out_dtype=torch.float16)
    assert same_bits(half, got.half())


@pytest.mark.parametrize("shape", bc.SHAPES)
def test_zero_stride_gout_is_read_as_it_lies(eng, shape):
    """what out.sum().backward() hands over: one element, every stride zero"""
    o = bc.oracle(shape, "ones")
    src, filt = dev(o["src"]), dev(o["filt"])
    gout = torch.ones((), device=DEV).expand(o["gout"].shape)
    assert set(gout.stride()) == {0}
    with pl.PointerRecorder(eng.lib, "dm_jbu_apply_bwd_filters_f32") as rf, pl.PointerRecorder(eng.lib, "dm_jbu_apply_bwd_source_f32") as rs_:
        gfilt, gsrc = eng.jbu_apply_bwd_filters(gout, src), eng.jbu_apply_bwd_source(gout, filt)
    assert rf.saw(gout) and rs_.saw(gout), "gout was copied instead of being read where it lies"
    bc.check(gfilt, o["gfilt64"], o["floor_gfilt"], f"gfilt {shape}, zero strides (floor {o['floor_gfilt']:.2e})")
    bc.check(gsrc, o["gsrc64"], o["floor_gsrc"], f"gsrc {shape}, zero strides (floor {o['floor_gsrc']:.2e})")
    dense = dev(o["gout"])
    assert same_bits(eng.jbu_apply_bwd_filters(dense, src), gfilt) and same_bits(eng.jbu_apply_bwd_source(dense, filt), gsrc)
    # and through autograd
    s, f = src.clone().requires_grad_(True), filt.clone().requires_grad_(True)
    out = fb.jbu_apply(s, f)
    assert same_bits(out.detach(), eng.jbu_apply(src, filt))
    out.sum().backward()
    assert same_bits(s.grad, gsrc) and same_bits(f.grad, gfilt)


def test_gout_inside_a_larger_poisoned_buffer(eng):
    o = bc.oracle(bc.SHAPES[2])
    gout, src, filt = dev(o["gout"]), dev(o["src"]), dev(o["filt"])
    Bn, Cw, H, W = gout.shape
    for pad in ("nan", "huge"):
        view = pl.place(gout, offset_elems=1, ld=W + 3, rows=H + 2, pad=pad, device=DEV)[..., :H, :W]
        assert not view.is_contiguous()
        with pl.PointerRecorder(eng.lib, "dm_jbu_apply_bwd_source_f32") as rec:
            gsrc = eng.jbu_apply_bwd_source(view, filt)
        assert rec.saw(view)
        assert same_bits(gsrc, eng.jbu_apply_bwd_source(gout, filt)), pad
        assert same_bits(eng.jbu_apply_bwd_filters(view, src), eng.jbu_apply_bwd_filters(gout, src)), pad


# ---------------------------------------------------------------------------------------------------------------- 2. through the modules
@pytest.mark.parametrize("shape", MODULE_SHAPES)
def test_stage_module_gradients(eng, shape):
    st, mo = jc.seeded_stage(*shape), bc.module_oracle(shape)
    up = copy.deepcopy(st["up"]).to(DEV).eval()
    s, g = dev(st["src"]).requires_grad_(True), dev(st["g"])
    out = up(s, g, route="device", differentiable=True)
    assert out.requires_grad
    with torch.no_grad():
        inference = up(s.detach(), g, route="device")
        assert same_bits(up(s.detach(), g, route="device", differentiable=True), inference)
    assert same_bits(out.detach(), inference), "the flag changed the output of the device route"
    out.backward(dev(mo["gout"]))
    got = {"source": s.grad}
    got.update({n: p.grad for n, p in up.named_parameters()})
    assert set(got) == set(mo["grads64"]) and all(v is not None for v in got.values())
    for n, ref in mo["grads64"].items():
        bc.check(got[n], ref, mo["floors"][n], f"{shape} grad of {n} (floor {mo['floors'][n]:.2e})")


def test_stack_without_a_graph_matches_the_reference_run(eng):
    c = jc.CASES[0]
    d, m = jc.case(c), jc.model(c, DEV)
    with torch.no_grad():
        y = m(dev(d["src"]), dev(d["img"]), route="device", differentiable=True)
    assert y.dtype == torch.float32 and not y.requires_grad
    jc.check(y, d["y_ref32"], d["f32_floor"], f"case {c}: differentiable device stack under no_grad")


def test_one_training_step(eng):
    from densematcher_amd.extractor import upsample_features
    d = jc.case("b")
    m = jc.model("b", DEV).train()
    torch.manual_seed(0)
    s = dev(d["src"]).half().requires_grad_(True)                       # an fp16 source: its gradient comes back in fp16
    y = upsample_features(m, s, dev(d["img"]), route="device", differentiable=True)
    assert y.dtype == torch.float32 and y.shape == d["y_ref32"].shape and bool(torch.isfinite(y).all())
    y.square().mean().backward()
    assert s.grad.dtype == torch.float16 and bool(torch.isfinite(s.grad).all()) and float(s.grad.abs().max()) > 0
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    torch.optim.SGD(m.parameters(), lr=1e-3).step()
    with torch.no_grad():                                               # the stepped weights reach the eval-mode kernels
        z = m.eval()(s.detach(), dev(d["img"]), route="device", differentiable=True)
    assert bool(torch.isfinite(z).all())


def test_only_the_gradients_asked_for_are_computed(eng, monkeypatch):
    """A frozen source: no source gradient is computed and the parameters' gradients are those of the unfrozen call.  Bit for bit that
    holds for what the kernels hand to autograd (gfilt) and for every parameter whose chain through torch is reproducible: range_temp,
    sigma_spatial and fixup_proj.  range_proj lies behind F.pad(mode="reflect"), whose backward on the GPU adds with float atomics
    (torch lists it as non-deterministic): two identical unfrozen calls already differ there in the last bits (measured on an MI355X:
    up to 5.1e-7 on gradients of magnitude 4, gfilt bitwise equal), so those four are held to the oracle's bound instead."""
    shape = bc.SHAPES[1]
    st, mo = jc.seeded_stage(*shape), bc.module_oracle(shape)
    up = copy.deepcopy(st["up"]).to(DEV).eval()
    g, gout = dev(st["g"]), dev(mo["gout"])
    handed, kernel = [], eng.jbu_apply_bwd_filters

    def recorded(*a, **k):
        handed.append(kernel(*a, **k))
        return handed[-1]

    def grads(source):
        up.zero_grad()
        up(source, g, route="device", differentiable=True).backward(gout)
        return {n: p.grad.clone() for n, p in up.named_parameters()}

    def refuse(*a, **k):
        raise AssertionError("a gradient nobody asked for was computed")
    monkeypatch.setattr(eng, "jbu_apply_bwd_filters", recorded)
    s = dev(st["src"]).requires_grad_(True)
    both = grads(s)
    assert s.grad is not None
    frozen = dev(st["src"])
    monkeypatch.setattr(eng, "jbu_apply_bwd_source", refuse)
    alone = grads(frozen)
    monkeypatch.undo()
    assert frozen.grad is None and set(alone) == set(both)
    assert len(handed) == 2 and same_bits(handed[0], handed[1])
    for n in both:
        if n.startswith("range_proj."):
            bc.check(alone[n], mo["grads64"][n], mo["floors"][n], f"frozen source, grad of {n}")
        else:
            assert same_bits(alone[n], both[n]), n
    # frozen parameters: the source's gradient alone, the same bits
    for p in up.parameters():
        p.requires_grad_(False)
    monkeypatch.setattr(eng, "jbu_apply_bwd_filters", refuse)
    s2 = dev(st["src"]).requires_grad_(True)
    up(s2, g, route="device", differentiable=True).backward(gout)
    monkeypatch.undo()
    assert same_bits(s2.grad, s.grad)


def test_a_view_has_the_same_bits_alone_and_in_a_batch(eng):
    gen = torch.Generator().manual_seed(13)
    Bn, Cw, h, w = 3, 9, 11, 12                                          # two source tiles, three channel chunks of gfilt
    src = torch.randn((Bn, Cw, h, w), generator=gen).to(DEV)
    filt = torch.randn((Bn, 2 * h, 2 * w, 49), generator=gen).to(DEV)
    gout = torch.randn((Bn, Cw, 2 * h, 2 * w), generator=gen).to(DEV)
    gsrc, gfilt = eng.jbu_apply_bwd_source(gout, filt), eng.jbu_apply_bwd_filters(gout, src)
    for b in range(Bn):
        assert same_bits(eng.jbu_apply_bwd_source(gout[b:b + 1], filt[b:b + 1]), gsrc[b:b + 1]), b
        assert same_bits(eng.jbu_apply_bwd_filters(gout[b:b + 1], src[b:b + 1]), gfilt[b:b + 1]), b
    assert not torch.equal(gsrc[0], gsrc[1]) and not torch.equal(gfilt[0], gfilt[1])
    # a second call gives the first one's bits
    assert same_bits(eng.jbu_apply_bwd_source(gout, filt), gsrc) and same_bits(eng.jbu_apply_bwd_filters(gout, src), gfilt)


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_device_route_without_the_flag_still_refuses_a_gradient(eng):
    st = jc.seeded_stage(*bc.SHAPES[1])
    up = copy.deepcopy(st["up"]).to(DEV).eval()
    with pytest.raises(ValueError, match="grad"):
        up(dev(st["src"]).requires_grad_(True), dev(st["g"]), route="device")
    with pytest.raises(ValueError, match="grad"):
        up(dev(st["src"]), dev(st["g"]), route="device", differentiable=False)      # the parameters require grad
    up.train()
    with pytest.raises(ValueError, match="training"):
        up(dev(st["src"]), dev(st["g"]), route="device")
    with pytest.raises(ValueError, match="GPU"):                                     # named: an operand on the CPU
        up(torch.from_numpy(np.array(st["src"])), dev(st["g"]), route="device", differentiable=True)
    m = jc.model("a", DEV)
    d = jc.case("a")
    with pytest.raises(ValueError, match="grad"):
        m(dev(d["src"]), dev(d["img"]), route="device")


def test_invalid_arguments(eng):
    null, P = C.c_void_p(0), (lambda t: C.c_void_p(t.data_ptr()))
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    lib, F32 = eng.lib, _lib.DM_F32

    def filters(h=4, w=4, Cw=3, Bn=1, src=buf, gout=buf, gfilt=buf, ss=None, gs=None, sd=F32):
        ss = ss or (Cw * h * w, h * w, w, 1)
        gs = gs or (Cw * 4 * h * w, 4 * h * w, 2 * w, 1)
        return lib.dm_jbu_apply_bwd_filters_f32(eng.ctx, Bn, Cw, h, w, sd, null if src is None else P(src), *ss,
                                                null if gout is None else P(gout), *gs, null if gfilt is None else P(gfilt))

    def source(h=4, w=4, Cw=3, Bn=1, gout=buf, filt=buf, gsrc=buf, gs=None):
        gs = gs or (Cw * 4 * h * w, 4 * h * w, 2 * w, 1)
        return lib.dm_jbu_apply_bwd_source_f32(eng.ctx, Bn, Cw, h, w, null if gout is None else P(gout), *gs,
                                               null if filt is None else P(filt), null if gsrc is None else P(gsrc))
    assert filters() == _lib.DM_OK and source() == _lib.DM_OK
    assert filters(gs=(0, 0, 0, 0)) == _lib.DM_OK and source(gs=(0, 0, 0, 0)) == _lib.DM_OK
    for kw in (dict(h=1), dict(w=1), dict(Cw=0), dict(Bn=0), dict(src=None), dict(gout=None), dict(gfilt=None), dict(sd=7),
               dict(ss=(48, 16, -4, 1)), dict(gs=(192, 64, -8, 1))):
        assert filters(**kw) == _lib.DM_EINVAL, kw
        assert eng.lib.dm_last_error(eng.ctx)
    for kw in (dict(h=1), dict(w=1), dict(Cw=0), dict(Bn=0), dict(gout=None), dict(filt=None), dict(gsrc=None), dict(gs=(192, 64, 8, -1))):
        assert source(**kw) == _lib.DM_EINVAL, kw
    torch.cuda.synchronize()
    # the Python layer
    o = bc.oracle(bc.SHAPES[1])
    gout, src, filt = dev(o["gout"]), dev(o["src"]), dev(o["filt"])
    with pytest.raises(ValueError, match="grad_out"):
        eng.jbu_apply_bwd_filters(gout[:, :, :-1], src)
    with pytest.raises(ValueError, match="grad_out"):
        eng.jbu_apply_bwd_filters(gout[0], src)
    with pytest.raises(ValueError, match="filters"):
        eng.jbu_apply_bwd_source(gout, filt[:, :-1])
    with pytest.raises(ValueError, match="grad_out"):
        eng.jbu_apply_bwd_source(gout[:, :, :-1], filt)
    with pytest.raises(ValueError, match="out_dtype"):
        eng.jbu_apply_bwd_source(gout, filt, out_dtype=torch.float64)

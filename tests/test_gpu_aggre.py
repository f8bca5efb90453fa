"""The aggregation network on the GPU (dm_agg_gather_f32, dm_groupnorm_stats_f32, dm_groupnorm_relu_f32, dm_conv3x3_f32, dm_agg_mix_f32,
MatchEngine.aggregate, the device route of featurizers) against the float64 restatement tests/aggre_restate.py and the reference's
recorded run tests/golden/fx_aggre.npz.

3 x 3 shapes (L, B, P_h, P_w, C_in, C_out): (1,1,1,1,1,1) the centre tap alone; (1,2,2,3,5,7); (2,2,3,5,12,12) where a neighbour must not
wrap to the next row, image or level; (1,1,9,9,70,33): 81 pixels are more than one 64-row tile, K = 630 is no multiple of 32 and one
output channel lies past a 32-wide block.  GroupNorm shapes (n_img, npix, C, G): (1,1,2,2) variance 0; (3,15,12,4); (2,81,70,5), the
last again around 100 and with a leading dimension over NaN padding.  Gather: R in {1, 4} on 4 x 4 and 5 x 5 grids from sources of 4 x 4,
2 x 2 and 1 x 1 (35 channels: more than one 32-channel tile), R = 3 on 5 x 4, and R = 2 on 7 x 6 (42 pixels: more than one 32-pixel tile).
Case a of the fixture has a level with as many channels in as out, hence no shortcut convolution (like the DINO level of the released
network); aggre_checks.seeded_network is the same size with a shortcut in every level.
Bound: lift_checks.bound; the floors are the fixture's or measured by aggre_checks on the CPU (the reference's expressions in float32
against the restatement), never taken from the device."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import aggre_checks as ac
import aggre_restate as rs
import lift_checks as lc
import placement as pl
from densematcher_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONV_SHAPES = [(1, 1, 1, 1, 1, 1), (1, 2, 2, 3, 5, 7), (2, 2, 3, 5, 12, 12), (1, 1, 9, 9, 70, 33)]
GN_SHAPES = [(1, 1, 2, 2, 0.0, 1), (3, 15, 12, 4, 0.0, 3), (2, 81, 70, 5, 0.0, 2), (2, 81, 70, 5, 100.0, 2)]
SMALL = ((3, 4, 4), (35, 2, 2), (2, 1, 1))
GATHERS = [((P, P), SMALL + ((4, P, P),), R) for P in (4, 5) for R in (1, 4)] + [
    ((5, 4), ((3, 5, 4), (5, 3, 2), (2, 1, 1), (4, 5, 4)), 3), ((7, 6), ((3, 7, 6), (35, 4, 3), (4, 7, 6)), 2)]


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                       # a copy: the shared references are read-only
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- 1. the 3 x 3 convolution
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3_against_the_restatement(eng, shape):
    d = ac.seeded_conv(*shape)
    got = eng.conv3x3(dev(d["x"]), dev(d["packed"]))
    assert got.shape == d["ref64"].shape and got.dtype == torch.float32 and got.is_contiguous()
    ac.check(got, d["ref64"], d["floor"], f"conv3x3 {shape} (floor {d['floor']:.2e})")


def test_conv3x3_reads_its_own_image_only(eng):
    d = ac.seeded_conv(*CONV_SHAPES[2])
    x, w = dev(d["x"]), dev(d["packed"])
    L, Bn = x.shape[:2]
    want = eng.conv3x3(x, w)
    for l in range(L):
        for b in range(Bn):
            poisoned = torch.full_like(x, float("nan"))
            poisoned[l, b] = x[l, b]
            got = eng.conv3x3(poisoned, w)
            assert torch.equal(pl.bits(got[l, b]), pl.bits(want[l, b])), (l, b)
            alone = eng.conv3x3(x[l:l + 1, b:b + 1].contiguous(), w[l:l + 1])
            assert torch.equal(pl.bits(alone[0, 0]), pl.bits(want[l, b])), (l, b)


# ---------------------------------------------------------------------------------------------------------------- 2. GroupNorm
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_groupnorm_stats_against_the_restatement(eng, shape):
    n_img, npix, Cw, G, offset, levels = shape
    d = ac.seeded_groupnorm(*shape)
    mean, rstd = eng.groupnorm_stats(dev(d["x"]), G)
    assert mean.shape == rstd.shape == (n_img, G) and mean.dtype == rstd.dtype == torch.float32
    ac.check(mean, d["mean64"], d["floor_mean"], f"mean {shape} (floor {d['floor_mean']:.2e})")
    ac.check(rstd, d["rstd64"], d["floor_rstd"], f"rstd {shape} (floor {d['floor_rstd']:.2e})")
    # both are float64 values rounded once: around 100 a one-pass fp32 variance would lose every digit of rstd
    assert torch.equal(mean, dev(d["mean32"])) and torch.equal(rstd, dev(d["rstd32"]))


@pytest.mark.parametrize("shape", GN_SHAPES)
def test_groupnorm_relu_against_the_restatement(eng, shape):
    d = ac.seeded_groupnorm(*shape)
    got = eng.groupnorm_relu(dev(d["x"]), dev(d["mean32"]), dev(d["rstd32"]), dev(d["gamma"]), dev(d["beta"]))
    assert got.shape == d["out64"].shape and float(got.min()) >= 0.0
    ac.check(got, d["out64"], d["floor_out"], f"groupnorm_relu {shape} (floor {d['floor_out']:.2e})")


def test_groupnorm_reads_rows_where_they_lie(eng):
    n_img, npix, Cw, G, _, levels = GN_SHAPES[2]
    d = ac.seeded_groupnorm(*GN_SHAPES[2])
    x = dev(d["x"])
    mean, rstd = eng.groupnorm_stats(x, G)
    out = eng.groupnorm_relu(x, mean, rstd, dev(d["gamma"]), dev(d["beta"]))
    placed = pl.place(x, offset_elems=1, ld=Cw + 3, pad="nan", device=DEV)
    view = placed[..., :Cw]
    assert not view.is_contiguous()
    with pl.PointerRecorder(eng.lib, "dm_groupnorm_stats_f32") as rec:
        m2, r2 = eng.groupnorm_stats(view, G)
    assert rec.saw(view), "the rows were copied instead of being read where they lie"
    assert torch.equal(pl.bits(m2), pl.bits(mean)) and torch.equal(pl.bits(r2), pl.bits(rstd))
    with pl.PointerRecorder(eng.lib, "dm_groupnorm_relu_f32") as rec:
        o2 = eng.groupnorm_relu(view, mean, rstd, dev(d["gamma"]), dev(d["beta"]))
    assert rec.saw(view) and torch.equal(pl.bits(o2), pl.bits(out))
    # an image's statistics alone and in the batch
    m1, r1 = eng.groupnorm_stats(x[1:2], G)
    assert torch.equal(pl.bits(m1), pl.bits(mean[1:2])) and torch.equal(pl.bits(r1), pl.bits(rstd[1:2]))


# ---------------------------------------------------------------------------------------------------------------- 3. gather
@pytest.mark.parametrize("size,shapes,R", GATHERS)
def test_gather_against_the_restatement(eng, size, shapes, R):
    d = ac.seeded_gather(size, shapes, R)
    got = eng.agg_gather([dev(s) for s in d["sources"]], num_rotations=R, step_deg=d["step"], size=size)
    assert got.shape == d["ref64"].shape and got.dtype == torch.float32
    ac.check(got, d["ref64"], d["floor"], f"gather {size} R = {R} (floor {d['floor']:.2e})")


def test_gather_of_one_rotation_is_the_concatenation(eng):
    d = ac.seeded_gather((4, 4), SMALL[:1] + ((4, 4, 4),), 1)
    srcs = [dev(s) for s in d["sources"]]
    got = eng.agg_gather(srcs)
    assert torch.equal(got, torch.cat(srcs, 1).permute(0, 2, 3, 1).reshape(got.shape))


def test_gather_fp16_source_is_the_fp32_route_on_the_rounded_source(eng):
    size, shapes, R = GATHERS[3]
    d = ac.seeded_gather(size, shapes, R)
    full = [dev(s) for s in d["sources"]]
    half = [s.half() for s in full]
    a = eng.agg_gather(half, R, d["step"], size)
    b = eng.agg_gather([h.float() for h in half], R, d["step"], size)
    mixed = eng.agg_gather([half[0], half[1].float(), half[2], half[3].float()], R, d["step"], size)
    assert torch.equal(pl.bits(a), pl.bits(b)) and torch.equal(pl.bits(a), pl.bits(mixed))
    assert not torch.equal(a, eng.agg_gather(full, R, d["step"], size))


def test_gather_reads_a_permuted_token_view_where_it_lies(eng):
    size, shapes, R = GATHERS[3]
    d = ac.seeded_gather(size, shapes, R)
    srcs = [dev(s) for s in d["sources"]]
    want = eng.agg_gather(srcs, R, d["step"], size)
    tokens = srcs[3].permute(0, 2, 3, 1).contiguous()               # (R B, P, P, C): what a ViT returns, up to a reshape
    view = tokens.permute(0, 3, 1, 2)
    assert view.stride(1) == 1 and not view.is_contiguous()
    for dtype in (torch.float32, torch.float16):
        v = view if dtype == torch.float32 else tokens.to(dtype).permute(0, 3, 1, 2)
        ref = want if dtype == torch.float32 else eng.agg_gather(srcs[:3] + [srcs[3].half()], R, d["step"], size)
        with pl.PointerRecorder(eng.lib, "dm_agg_gather_f32") as rec:
            got = eng.agg_gather(srcs[:3] + [v], R, d["step"], size)
        assert rec.saw(v), "the token view was copied instead of being read where it lies"
        assert torch.equal(pl.bits(got), pl.bits(ref))


# ---------------------------------------------------------------------------------------------------------------- 4. the network
def one_level(packed, l):
    """the same weights with the mixture replaced by level l alone: 1 * level_l + 0 * the others is level l exactly"""
    p = copy.copy(packed)
    p.mix = torch.zeros_like(packed.mix)
    p.mix[l] = 1.0
    return p


@pytest.mark.parametrize("c", ac.CASES)
def test_cases_against_the_reference_run(eng, c):
    d, m = ac.case(c), ac.model(c, DEV)
    x = dev(d["x"])
    with torch.no_grad():
        y = m(x, route="device")
        auto = m(x, route="auto")
        ac.check(m(x, route="torch"), d["y_ref32"], d["f32_floor"], f"case {c}: torch route on the GPU")
    assert y.dtype == torch.float32 and y.shape == d["y_ref32"].shape
    assert y.permute(0, 2, 3, 1).is_contiguous()                    # NCHW-shaped over channels-last memory
    ac.check(y, d["y_ref32"], d["f32_floor"], f"case {c}: device route")
    ac.check(auto, d["y_ref32"], d["f32_floor"], f"case {c}: auto route")
    rows = eng.agg_gather([x])
    for l in range(len(d["dims"])):
        level = eng.aggregate(one_level(m.packed(eng.device), l), rows, *x.shape[2:])
        ac.check(level, d[f"level{l}"], d["f32_floor"], f"case {c}: device level {l}")


def test_seeded_network_on_the_device(eng):
    d = ac.seeded_network()
    m = copy.deepcopy(d["net"]).to(DEV)
    x = dev(d["x"])
    with torch.no_grad():
        y = m(x, route="device")
    ac.check(y, d["y64"], d["floor"], f"seeded network: device route (floor {d['floor']:.2e})")
    rows = eng.agg_gather([x])
    for l, ref in enumerate(d["levels64"]):
        ac.check(eng.aggregate(one_level(m.packed(eng.device), l), rows, *x.shape[2:]), ref, d["floor"], f"seeded network: device level {l}")
    # the packed blocks follow the parameters
    before = m.packed(eng.device)
    assert m.packed(eng.device) is before
    with torch.no_grad():
        m.mixing_weights[0] += 1.0
        assert m.packed(eng.device) is not before and not torch.equal(m(x, route="device"), y)


def rotinv_sources(Bn, R=4, seed=8):
    dims = ac.case("b")["dims"]
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(R * Bn, c, h, h, generator=gen) for c, h in zip(dims, (6, 3, 2, 6))]


def test_rotation_averaged_features_against_the_restatement(eng):
    from densematcher_amd.featurizers import aggregate_features
    d, R, Bn = ac.case("b"), 4, 2
    srcs = rotinv_sources(Bn)
    ref = rs.network(rs.gather([s.numpy() for s in srcs], None, R, 90.0), d["state"], d["dims"], d["groups"])["y"]
    with torch.no_grad():
        floor = ac.floor(aggregate_features(ac.model("b"), *srcs, num_rotations=R, rot_inv=True, route="torch"), ref)      # on the CPU
        m = ac.model("b", DEV)
        got = aggregate_features(m, *[s.to(DEV) for s in srcs], num_rotations=R, rot_inv=True, route="device")
        auto = aggregate_features(m, *[s.to(DEV) for s in srcs], num_rotations=R, rot_inv=True)
    assert got.shape == ref.shape
    ac.check(got, ref, floor, f"rotation-averaged features: device route (floor {floor:.2e})")
    ac.check(auto, ref, floor, "rotation-averaged features: auto route")


def test_batching_and_chunking_give_the_same_bits(eng):
    from densematcher_amd.featurizers import aggregate_features
    R, Bn = 4, 3
    m = ac.model("b", DEV)
    srcs = [s.to(DEV) for s in rotinv_sources(Bn, seed=9)]
    part = lambda b0, b1: [s.view(R, Bn, *s.shape[1:])[:, b0:b1].reshape(R * (b1 - b0), *s.shape[1:]) for s in srcs]
    run = lambda ss: aggregate_features(m, *ss, num_rotations=R, rot_inv=True, route="device")
    with torch.no_grad():
        together = run(srcs)
        alone = torch.cat([run(part(b, b + 1)) for b in range(Bn)])
        chunks = torch.cat([run(part(0, 2)), run(part(2, 3))])
    assert torch.equal(pl.bits(together), pl.bits(alone)) and torch.equal(pl.bits(together), pl.bits(chunks))
    assert not torch.equal(together[0], together[1])


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_invalid_arguments(eng):
    null, P = C.c_void_p(0), (lambda t: C.c_void_p(t.data_ptr()))
    lib, E, b = eng.lib, _lib.DM_EINVAL, P(torch.zeros(1 << 16, dtype=torch.float32, device=DEV))

    def gather(n_src=1, desc=(2, 4, 4, 32, 16, 4, 1, _lib.DM_F32), srcs=None, R=1, Bn=1, Ph=4, Pw=4, out=b, ld=2, no_desc=False):
        arr = (C.c_longlong * (8 * max(n_src, 1)))(*(list(desc) * max(n_src, 1)))
        srcs = [b] * min(n_src, 8) + [null] * (8 - min(n_src, 8)) if srcs is None else srcs
        return lib.dm_agg_gather_f32(eng.ctx, n_src, null if no_desc else C.cast(arr, C.c_void_p), *srcs, R, Bn, Ph, Pw, 90.0, out, ld)
    assert gather() == _lib.DM_OK
    assert gather(n_src=8, ld=16) == _lib.DM_OK and gather(R=16, desc=(2, 4, 4, 0, 16, 4, 1, _lib.DM_F32)) == _lib.DM_OK
    for kw in (dict(n_src=0), dict(n_src=9, ld=18), dict(R=0), dict(R=17), dict(Bn=0), dict(Ph=0), dict(Pw=-1), dict(out=null), dict(no_desc=True),
               dict(srcs=[null] * 8), dict(ld=1), dict(desc=(0, 4, 4, 32, 16, 4, 1, 1)), dict(desc=(2, 0, 4, 32, 16, 4, 1, 1)),
               dict(desc=(2, 4, 4, 32, 16, -4, 1, 1)), dict(desc=(2, 4, 4, -32, 16, 4, 1, 1)), dict(desc=(2, 4, 4, 32, 16, 4, 1, 7))):
        assert gather(**kw) == E, kw

    def stats(n=1, npix=4, Cw=6, G=3, x=b, ld=6, mean=b, rstd=b):
        return lib.dm_groupnorm_stats_f32(eng.ctx, n, npix, Cw, G, x, ld, mean, rstd)
    assert stats() == _lib.DM_OK
    for kw in (dict(n=0), dict(npix=0), dict(Cw=0), dict(G=0), dict(G=4), dict(ld=5), dict(x=null), dict(mean=null), dict(rstd=null)):
        assert stats(**kw) == E, kw

    def relu(n=2, Bn=1, npix=4, Cw=6, G=3, x=b, ldx=6, mean=b, rstd=b, gamma=b, beta=b, out=b, ldo=6):
        return lib.dm_groupnorm_relu_f32(eng.ctx, n, Bn, npix, Cw, G, x, ldx, mean, rstd, gamma, beta, out, ldo)
    assert relu() == _lib.DM_OK
    for kw in (dict(n=0), dict(Bn=0), dict(n=3, Bn=2), dict(npix=0), dict(Cw=0), dict(G=0), dict(G=4), dict(ldx=5), dict(ldo=5), dict(x=null),
               dict(mean=null), dict(rstd=null), dict(gamma=null), dict(beta=null), dict(out=null)):
        assert relu(**kw) == E, kw

    def conv(L=1, Bn=1, Ph=3, Pw=3, Ci=4, Co=5, x=b, ldx=4, w=b, out=b, ldo=5):
        return lib.dm_conv3x3_f32(eng.ctx, L, Bn, Ph, Pw, Ci, Co, x, ldx, w, out, ldo)
    assert conv() == _lib.DM_OK
    for kw in (dict(L=0), dict(Bn=0), dict(Ph=0), dict(Pw=0), dict(Ci=0), dict(Co=0), dict(ldx=3), dict(ldo=4), dict(x=null), dict(w=null), dict(out=null)):
        assert conv(**kw) == E, kw

    def mix(L=2, Bn=1, npix=4, Cw=6, G=3, ld3=6, lds=6, ldo=6, ptrs=None, mask=0):
        ptrs = [b] * 12 if ptrs is None else ptrs              # y3, ys, 8 statistics and parameters, mix, out
        return lib.dm_agg_mix_f32(eng.ctx, L, Bn, npix, Cw, G, ptrs[0], ld3, ptrs[1], lds, *ptrs[2:10], mask, ptrs[10], ptrs[11], ldo)
    assert mix() == _lib.DM_OK and mix(mask=3) == _lib.DM_OK
    for kw in (dict(L=0), dict(Bn=0), dict(npix=0), dict(Cw=0), dict(G=0), dict(G=4), dict(ld3=5), dict(lds=5), dict(ldo=5), dict(mask=4), dict(L=33)):
        assert mix(**kw) == E, kw
    for i in range(12):
        assert mix(ptrs=[null if j == i else b for j in range(12)]) == E, i
    torch.cuda.synchronize()

    # the Python layer
    x = torch.zeros(2, 3, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="sources"):
        eng.agg_gather([x] * 9)
    with pytest.raises(ValueError, match="num_rotations"):
        eng.agg_gather([x], num_rotations=17)
    with pytest.raises(ValueError, match="multiple"):
        eng.agg_gather([x], num_rotations=4)
    with pytest.raises(ValueError):
        eng.groupnorm_stats(torch.zeros(1, 4, 6, device=DEV), 4)
    with pytest.raises(ValueError, match="weight"):
        eng.conv3x3(torch.zeros(1, 1, 3, 3, 4, device=DEV), torch.zeros(1, 5, 35, device=DEV))
    m = ac.model("b", DEV)
    with pytest.raises(ValueError, match="rows"):
        eng.aggregate(m.packed(eng.device), torch.zeros(1, 36, 7, device=DEV), 6, 6)
    m.train()
    with torch.no_grad(), pytest.raises(ValueError, match="training"):
        m(dev(ac.case("b")["x"]), route="device")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def test_featurizer_takes_the_raw_backbone_outputs():
    from densematcher_amd.featup.upsamplers import JBUStack
    from densematcher_amd.featurizers import AggregationNetwork, aggregate_features
    from densematcher_amd.model import MeshFeaturizer
    fx = lc.golden("fx_featurizer.npz")
    names = [str(n) for n in fx["names"]]
    Cw = fx["fts"].shape[1]
    torch.manual_seed(5)
    up = JBUStack(Cw).eval()
    net = AggregationNetwork(feature_dims=[5, 7, 6, 4], projection_dim=Cw, num_norm_groups=3).eval()
    model = MeshFeaturizer(None, (3, 1), int(fx["blocks"]), int(fx["width"]), num_features=Cw, upsampler=up, aggre_net=net)
    assert any(k.startswith("aggre_net.bottleneck_layers.") for k in model.state_dict())
    model.load_state_dict({n: torch.from_numpy(fx[f"p{i}"].copy()) for i, n in enumerate(names)}, strict=False)
    model = model.to(DEV).eval()
    mesh, ops, cams, fts, _ = lc.featurizer_inputs(DEV)
    views = fts.shape[0]
    raw = tuple(torch.randn(views, c, h, h).to(DEV) for c, h in ((5, 2), (7, 1), (6, 1), (4, 2)))
    images = torch.randn(views, 3, 32, 32).to(DEV)
    with torch.no_grad():
        lr = aggregate_features(model.aggre_net, *raw, route="device")
        want = model(None, mesh, ops, cams, return_mvfeatures=True, fts_lr=lr, images=images, route="device")
        got = model(None, mesh, ops, cams, return_mvfeatures=True, raw=raw, images=images, route="device")
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="aggre_net"):
        MeshFeaturizer(None, (3, 1), int(fx["blocks"]), int(fx["width"]), num_features=Cw, upsampler=up).to(DEV)(
            None, mesh, ops, cams, raw=raw, images=images, route="device")

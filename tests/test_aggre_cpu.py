"""CPU: the aggregation network behind the 2D backbones (densematcher_amd.featurizers) against the reference's recorded float32 run
tests/golden/fx_aggre.npz, and the float64 restatement tests/aggre_restate.py against that run and against torch's own interpolation and
grid sampling.  Bound: lift_checks.bound with the floor the fixture records."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aggre_checks as ac
import aggre_restate as rs
from densematcher_amd import extractor
from densematcher_amd.featurizers import AggregationNetwork, aggregate_features, gather_features, rotate
from densematcher_amd.featurizers.modules.resnet import BottleneckBlock, Conv2d, ResNet, get_norm


# ---------------------------------------------------------------------------------------------------------------- the network
@pytest.mark.parametrize("c", ac.CASES)
def test_state_dict_of_the_reference_loads_strict(c):
    d = ac.case(c)
    m = AggregationNetwork(feature_dims=d["dims"], projection_dim=d["proj"], num_norm_groups=d["groups"])
    assert list(m.state_dict()) == d["names"]                          # the reference's keys in the reference's order
    m.load_state_dict({n: torch.from_numpy(np.array(v)) for n, v in d["state"].items()}, strict=True)
    assert all(tuple(m.state_dict()[n].shape) == v.shape for n, v in d["state"].items())


@pytest.mark.parametrize("c", ac.CASES)
def test_torch_route_against_the_reference_run(c):
    d, m = ac.case(c), ac.model(c)
    levels = {}
    hooks = [layer.register_forward_hook(lambda mod, i, o, l=l: levels.__setitem__(l, o.detach().clone())) for l, layer in enumerate(m.bottleneck_layers)]
    with torch.no_grad():
        y = m(torch.from_numpy(np.array(d["x"])), route="torch")
        auto = m(torch.from_numpy(np.array(d["x"])))                   # no GPU tensors: auto is the torch route
    for h in hooks:
        h.remove()
    ac.check(y, d["y_ref32"], d["f32_floor"], f"case {c}: torch route")
    assert torch.equal(y, auto)
    for l in range(len(d["dims"])):
        ac.check(levels[l], d[f"level{l}"], d["f32_floor"], f"case {c}: level {l}")


@pytest.mark.parametrize("c", ac.CASES)
def test_restatement_against_the_reference_run(c):
    d, r = ac.case(c), ac.restated(c)
    ac.check(d["y_ref32"], r["y"], d["f32_floor"], f"case {c}: recorded run against the restatement")
    for l in range(len(d["dims"])):
        ac.check(d[f"level{l}"], r["levels"][l], d["f32_floor"], f"case {c}: level {l} against the restatement")
    assert abs(r["mix"].sum() - 1.0) < 1e-12


def test_constructor_defaults_and_parameters():
    m = AggregationNetwork()
    assert m.feature_dims == [640, 1280, 1280, 768] and m.mixing_weights.shape == (4,)
    assert set(n for n, _ in m.named_parameters() if "." not in n) == {"logit_scale", "self_logit_scale", "mixing_weights"}
    assert abs(m.logit_scale.item() - np.log(1 / 0.07)) < 1e-6 and abs(m.self_logit_scale.item() - np.log(10)) < 1e-6
    blk = m.bottleneck_layers[0][0]
    assert isinstance(blk, BottleneckBlock) and blk.conv2.weight.shape == (96, 96, 3, 3) and blk.shortcut.weight.shape == (384, 640, 1, 1)
    assert isinstance(blk.conv1, Conv2d) and isinstance(blk.conv1.norm, torch.nn.GroupNorm) and blk.conv1.norm.num_groups == 32
    assert get_norm("", 8) is None and get_norm(None, 8) is None
    stage = ResNet.make_stage(BottleneckBlock, 2, in_channels=8, out_channels=16, bottleneck_channels=4, num_norm_groups=2, stride_per_block=[1, 1])
    assert [b.in_channels for b in stage] == [8, 16] and stage[1].shortcut is None
    # Kaiming-normal with fan-out: std = sqrt(2 / (C_out k k))
    w = m.bottleneck_layers[1][0].shortcut.weight
    assert abs(float(w.detach().std()) / (2.0 / 384) ** 0.5 - 1.0) < 0.02


def test_load_pretrained_weights_with_a_fifth_mixing_weight():
    d = ac.case("a")
    state = {n: torch.from_numpy(np.array(v)) for n, v in d["state"].items()}
    state["mixing_weights"] = torch.cat([state["mixing_weights"], torch.tensor([7.0])])
    state["not.a.key"] = torch.zeros(3)
    m = AggregationNetwork(feature_dims=d["dims"], projection_dim=d["proj"], num_norm_groups=d["groups"])
    m.load_pretrained_weights(state)
    assert torch.equal(m.mixing_weights.data, state["mixing_weights"][:4])
    for n, v in m.state_dict().items():
        if n != "mixing_weights":
            assert torch.equal(v, state[n]), n
    net = extractor.load_aggre_net(state, feature_dims=d["dims"], projection_dim=d["proj"], num_norm_groups=d["groups"])
    assert not net.training and torch.equal(net.mixing_weights.data, state["mixing_weights"][:4])


def test_device_route_refuses_training_gradients_and_unknown_routes():
    xb = torch.from_numpy(np.array(ac.case("b")["x"]))
    b = ac.model("b")
    with torch.no_grad():
        b.train()
        with pytest.raises(ValueError, match="training"):
            b(xb, route="device")
        b.eval()
        with pytest.raises(ValueError, match="route"):
            b(xb, route="gpu")
    with pytest.raises(ValueError, match="grad"):
        b(xb, route="device")
    odd = AggregationNetwork(feature_dims=[8, 6], projection_dim=8, num_norm_groups=2, kernel_size=[1, 1, 1]).eval()
    with torch.no_grad(), pytest.raises(ValueError, match="kernels"):
        odd(torch.zeros(1, 14, 2, 2), route="device")
    if not torch.cuda.is_available():
        with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
            b(xb, route="device")


def test_packed_blocks_and_a_level_without_shortcut():
    """case a's level 2 has 16 channels in and out, like the DINO level of the released network (768): no shortcut convolution"""
    d, a = ac.case("a"), ac.model("a")
    assert a.bottleneck_layers[2][0].shortcut is None and a.device_obstacle() is None
    p = a.packed("cpu")
    Cb, Co = d["proj"] // 4, d["proj"]
    assert p.identity == (2,) and p.feature_dims == tuple(d["dims"]) and (p.bottleneck, p.out_channels, p.groups) == (Cb, Co, d["groups"])
    assert [tuple(w.shape) for w in p.w1] == [(Cb + Co, 8), (Cb + Co, 12), (Cb, 16), (Cb + Co, 6)]
    assert p.w2.shape == (4, Cb, 9 * Cb) and p.w3.shape == (4, Co, Cb) and p.gs.shape == (4, Co) and p.g1.shape == (4, Cb)
    w = a.bottleneck_layers[1][0].conv2.weight.detach()
    assert p.w2[1, 3, (3 * 2 + 1) * Cb + 2] == w[3, 2, 2, 1]          # contraction index (3 dy + dx) C_in + c
    assert torch.equal(p.w1[0][Cb:], a.bottleneck_layers[0][0].shortcut.weight.detach().reshape(Co, 8))
    assert torch.allclose(p.mix, torch.from_numpy(np.array(ac.restated("a")["mix"])).float(), atol=1e-7)
    assert a.packed("cpu") is p
    with torch.no_grad():
        a.bottleneck_layers[0][0].conv1.norm.bias[0] += 1.0
    assert a.packed("cpu") is not p


# ---------------------------------------------------------------------------------------------------------------- rotate, gather
@pytest.mark.parametrize("size", [4, 5])
def test_rotate_by_quarter_turns_is_rot90(size):
    img = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(size))
    for k in range(-1, 5):
        assert torch.equal(rotate(img, 90 * k), torch.rot90(img, k, (2, 3))), k


def test_rotate_at_24_and_direction():
    img = torch.randn(1, 2, 24, 24, generator=torch.Generator().manual_seed(24))
    for k in range(4):
        err = float((rotate(img, 90 * k) - torch.rot90(img, k, (2, 3))).abs().max())
        assert err < 1e-5 * float(img.abs().max()), (k, err)       # float32 grid coordinates: 3.6e-6 at this size
        assert np.abs(rs.rotate(img.numpy(), 90 * k) - torch.rot90(img, k, (2, 3)).numpy()).max() < 1e-13
    spot = torch.zeros(1, 1, 5, 5)
    spot[0, 0, 0, 4] = 1.0                                          # row 0, last column: +90 degrees turns it to row 0, column 0
    out = rotate(spot, 90)
    assert out[0, 0, 0, 0] == 1.0 and float(out.sum()) == 1.0
    assert rs.rotate(spot.numpy(), 90)[0, 0, 0, 0] == 1.0


@pytest.mark.parametrize("angle", [0.0, 30.0, 120.0, -45.0, 200.0])
def test_restated_rotation_is_grid_sample_in_float64(angle):
    img = torch.randn(2, 3, 5, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    got = rs.rotate(img.numpy(), angle)
    assert np.abs(got - rotate(img, angle).numpy()).max() < 1e-13
    assert rotate(img[0, 0], angle).shape == (5, 4)


def test_restated_interpolation_is_torch_in_float64():
    x = torch.randn(2, 3, 4, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    for size in ((5, 5), (8, 4), (4, 2), (3, 7)):
        want = F.interpolate(x, size=size, mode="bilinear", align_corners=False).numpy()
        assert np.abs(rs.interp(x.numpy(), size) - want).max() < 1e-14, size
    one = torch.randn(1, 2, 1, 1, dtype=torch.float64)
    assert np.array_equal(rs.interp(one.numpy(), (3, 3)), one.expand(1, 2, 3, 3).numpy())


def test_gather_features_against_torch_and_the_restatement():
    gen = torch.Generator().manual_seed(3)
    s3, s4, s5, dino = (torch.randn(2, c, h, h, generator=gen) for c, h in ((3, 8), (5, 4), (4, 2), (2, 8)))
    got = gather_features(s3, s4, s5, dino)
    up = lambda t: F.interpolate(t, size=(8, 8), mode="bilinear", align_corners=False)
    assert torch.equal(got, torch.cat([s3, up(s4), up(s5), dino], 1)) and torch.equal(got, gather_features(s3, s4, s5, dino, num_patches=8))
    ref = rs.gather([t.numpy() for t in (s3, s4, s5, dino)])
    ac.check(got, ref, ac.floor(got, ref), "gather_features")
    assert ac.floor(got, ref) < 2e-7


def test_aggregate_features_on_torch_against_the_restatement():
    d, m = ac.case("b"), ac.model("b")
    gen = torch.Generator().manual_seed(4)
    R, Bn = 4, 2
    srcs = [torch.randn(R * Bn, c, h, h, generator=gen) for c, h in zip(d["dims"], (6, 3, 2, 6))]
    with torch.no_grad():
        plain = aggregate_features(m, *[s[:Bn] for s in srcs], route="torch")
        rotinv = aggregate_features(m, *srcs, num_rotations=R, rot_inv=True, route="torch")
    np_srcs = [s.numpy() for s in srcs]
    ref_plain = rs.network(rs.gather([s[:Bn] for s in np_srcs]), d["state"], d["dims"], d["groups"])["y"]
    ref_rot = rs.network(rs.gather(np_srcs, None, R, 90.0), d["state"], d["dims"], d["groups"])["y"]
    assert plain.shape == rotinv.shape == (Bn, d["proj"], 6, 6)
    # two float32 stages in a row (gather, network): the bound with twice the network's recorded floor
    ac.check(plain, ref_plain, 2 * d["f32_floor"], "aggregate_features, one rotation")
    ac.check(rotinv, ref_rot, 2 * d["f32_floor"], "aggregate_features, four rotations")
    with pytest.raises(ValueError, match="rotations"):
        aggregate_features(m, *[s[:3] for s in srcs], num_rotations=4, rot_inv=True, route="torch")


def test_upsampler_name_gains_rotinv():
    s = extractor.parse_upsampler_name("ckpt/jbu_imsize=384_channelnorm=False_unitnorm=True_rotinv=True.ckpt")
    assert s == {"imsize": 384, "channelnorm": False, "unitnorm": True, "rotinv": True}
    assert extractor.parse_upsampler_name("jbu_imsize=224_unitnorm=True.ckpt")["rotinv"] is False

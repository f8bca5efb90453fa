"""CPU: FeatUp's JBU upsampling on the torch route against the reference's recorded float32 run (tests/golden/fx_jbu.npz,
tools/make_golden_jbu.py) and its float64 restatement (tests/jbu_restate.py): every stage, the checkpoint's names, the gradients of the
adaptive convolution, the featurizer's fts_lr= / images= path and the refusals of the device route."""
import numpy as np
import pytest
import torch

import jbu_checks as jc
import lift_checks as lc
from densematcher_amd import extractor
from densematcher_amd.featup import ChannelNorm, UnitNorm, adaptive_conv, get_upsampler
from densematcher_amd.featup.upsamplers import Bilinear, JBULearnedRange, JBUStack


@pytest.mark.parametrize("c", jc.CASES)
def test_restatement_matches_the_reference_at_every_stage(c):
    d, res = jc.case(c), jc.restated(c)
    jc.check(res["kernel1"], d["kernel1"], d["f32_floor"], f"case {c}: restated kernel of stage 1")
    for s in range(4):
        jc.check(res["stages"][s], d[f"stage{s + 1}"], d["f32_floor"], f"case {c}: restated stage {s + 1}")
    jc.check(res["y"], d["y_ref32"], d["f32_floor"], f"case {c}: restated output")
    floor = float(np.abs(d["y_ref32"] - res["y"]).max() / np.abs(res["y"]).max())
    print(f"case {c}: f32_floor recomputed {floor:.3e}, recorded {float(d['f32_floor']):.3e}")
    assert abs(floor - float(d["f32_floor"])) <= 1e-9


@pytest.mark.parametrize("c", jc.CASES)
def test_torch_route_matches_the_reference_at_every_stage(c):
    d, m = jc.case(c), jc.model(c)
    stages = {}
    hooks = [getattr(m, f"up{s}").register_forward_hook(lambda mod, i, o, s=s: stages.__setitem__(s, o)) for s in range(1, 5)]
    with torch.no_grad():
        y = m(torch.from_numpy(d["src"]), torch.from_numpy(d["img"]), route="torch")
        g1 = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(d["img"]), tuple(2 * s for s in d["src"].shape[2:]))
        k1 = m.up1.combined_kernel(g1)
    for h in hooks:
        h.remove()
    jc.check(k1, d["kernel1"], d["f32_floor"], f"case {c}: torch kernel of stage 1")
    for s in range(1, 5):
        jc.check(stages[s], d[f"stage{s}"], d["f32_floor"], f"case {c}: torch stage {s}")
    jc.check(y, d["y_ref32"], d["f32_floor"], f"case {c}: torch output")
    assert y.shape[2:] == tuple(16 * s for s in d["src"].shape[2:])


def test_recorded_keys_load_strict_and_load_upsampler_strips_the_prefix(tmp_path):
    d = jc.case("a")
    m = get_upsampler("jbu_stack", 6)
    assert isinstance(m, JBUStack) and list(m.state_dict().keys()) == d["names"]
    m.load_state_dict({n: torch.from_numpy(np.array(v)) for n, v in d["state"].items()}, strict=True)
    assert isinstance(get_upsampler("bilinear", 6), Bilinear)
    with pytest.raises(ValueError):
        get_upsampler("nearest", 6)
    # a checkpoint as released: {'state_dict': {'upsampler.*': ..., other entries}}, the settings in the file's name
    ckpt = {"state_dict": {"upsampler." + n: torch.from_numpy(np.array(v)) for n, v in d["state"].items()}}
    ckpt["state_dict"]["model.other.weight"] = torch.zeros(3)
    path = tmp_path / "jbu_imsize=384_channelnorm=False_unitnorm=True_rotinv=True.ckpt"
    torch.save(ckpt, path)
    up, settings = extractor.load_upsampler(str(path), 6)
    assert settings == {"imsize": 384, "channelnorm": False, "unitnorm": True} and not up.training
    for n, v in up.state_dict().items():
        assert torch.equal(v, torch.from_numpy(np.array(d["state"][n]))), n
    up2, none = extractor.load_upsampler(ckpt, 6)
    assert none == {} and all(torch.equal(a, b) for a, b in zip(up.state_dict().values(), up2.state_dict().values()))
    with pytest.raises(RuntimeError):
        extractor.load_upsampler(ckpt, 7)              # strict: another width does not load


def test_upsample_features_is_the_extractor_forward_without_the_backbone():
    d, m = jc.case("b"), jc.model("b")
    src, img = torch.from_numpy(d["src"]), torch.from_numpy(d["img"])
    with torch.no_grad():
        plain = extractor.upsample_features(m, src, img, route="torch")
        jc.check(plain, d["y_ref32"], d["f32_floor"], "upsample_features")
        both = extractor.upsample_features(m, src, img, use_unitnorm=True, use_channelnorm=True, route="torch")
        want = m(ChannelNorm(5)(UnitNorm(5)(src)), img, route="torch")
    assert torch.equal(both, want)
    unit = UnitNorm(5)(src)
    assert torch.allclose(unit.norm(dim=1), torch.ones_like(unit[:, 0]), atol=1e-6)
    assert torch.allclose(ChannelNorm(5)(src).mean(dim=1), torch.zeros_like(unit[:, 0]), atol=1e-6)
    half = m(src, img, route="torch", out_dtype=torch.float16, memory_format=torch.channels_last)
    assert half.dtype == torch.float16 and half.is_contiguous(memory_format=torch.channels_last)


def test_adaptive_conv_gradcheck_float64():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((1, 2, 4 + 6, 5 + 6), generator=gen, dtype=torch.float64, requires_grad=True)
    f = torch.randn((1, 4, 5, 7, 7), generator=gen, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: adaptive_conv(a, b, route="torch"), (x, f), eps=1e-6, atol=1e-7, rtol=1e-6)
    # the value: the definition, one output at a time
    y = adaptive_conv(x, f, route="torch").detach()
    want = torch.stack([torch.stack([(f[0, r, q] * x[0, :, r:r + 7, q:q + 7]).sum((1, 2)) for q in range(5)], -1) for r in range(4)], -2)
    assert torch.allclose(y[0], want.detach(), atol=1e-12)
    with pytest.raises(ValueError):
        adaptive_conv(x[:, :, :-1], f)


def test_featurizer_takes_low_resolution_features_and_images():
    from densematcher_amd.model import MeshFeaturizer
    fx = lc.golden("fx_featurizer.npz")
    names = [str(n) for n in fx["names"]]
    Cw = fx["fts"].shape[1]
    torch.manual_seed(3)
    up = JBUStack(Cw).eval()
    model = MeshFeaturizer(None, (3, 1), int(fx["blocks"]), int(fx["width"]), num_features=Cw, upsampler=up)
    model.load_state_dict({n: torch.from_numpy(fx[f"p{i}"].copy()) for i, n in enumerate(names)}, strict=False)
    assert [k for k in model.state_dict() if not k.startswith("upsampler.")] == names
    model.eval()
    mesh, ops, cams, fts, _ = lc.featurizer_inputs()
    views = fts.shape[0]
    lr, images = torch.randn(views, Cw, 2, 2), torch.randn(views, 3, 32, 32)
    with torch.no_grad():
        maps = up(lr, images, route="torch")
        want = model(None, mesh, ops, cams, return_mvfeatures=True, fts=maps, route="host")
        got = model(None, mesh, ops, cams, return_mvfeatures=True, fts_lr=lr, images=images, route="host")
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    plain, _ = lc.featurizer()
    with pytest.raises(ValueError, match="upsampler"):
        plain(None, mesh, ops, cams, fts_lr=lr, images=images)
    with pytest.raises(ValueError, match="images"):
        model(None, mesh, ops, cams, fts_lr=lr)


def test_device_route_refusals():
    m = jc.model("a")
    d = jc.case("a")
    src, img = torch.from_numpy(d["src"]), torch.from_numpy(d["img"])
    with pytest.raises(ValueError, match="route"):
        m(src, img, route="gpu")
    m.train()
    with pytest.raises(ValueError, match="training"):
        m(src, img, route="device")
    with pytest.raises(ValueError, match="training"):
        m.up1(src, img[:, :, :6, :6], route="device")
    m.eval()
    with pytest.raises(ValueError, match="grad"):
        m(src, img, route="device")                                  # parameters require grad and grad mode is on
    with torch.no_grad():
        with pytest.raises(ValueError, match="twice"):
            m.up1(src, img[:, :, :7, :6], route="device")            # guidance 7 x 6 for a 3 x 3 source
        with pytest.raises(ValueError, match="twice"):
            m.up1(src, img, route="device")                          # 16x: JBULearnedRange alone allows it, on torch only
        y = m.up1(src, img[:, :, :7, :6], route="auto")              # auto falls back to torch for it
        assert tuple(y.shape) == (1, 6, 7, 6)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="GPU"):
                m(src, img, route="device")
            assert tuple(m(src, img, route="auto").shape) == (1, 6, 48, 48)

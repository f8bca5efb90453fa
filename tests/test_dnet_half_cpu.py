"""CPU: what the fp16 route through DiffusionNet needs off the GPU -- PackedOperators.half_operands() against NumPy, the refusals of
DiffusionNet's device route for halved and mixed modules, route="auto" without a GPU, and the accuracy of the route's restatement
(tests/dnet_half_restate.py) against the torch route run as the reference runs it."""
import copy
import functools

import numpy as np
import pytest
import torch

import dnet_half_restate as hs
import dnet_layers_checks as lc
import dnet_layers_restate as rs
from densematcher_amd.diffusion_net import layers

KEYS = ("t", "r", "f")


@functools.lru_cache(maxsize=None)
def packed():
    return layers.pack_operators([lc.operators(k) for k in KEYS])


# ---------------------------------------------------------------------------------------------------------------- half_operands
def test_half_operands_against_numpy():
    p = packed()
    assert p.n_verts == [160, 96, 81]
    evecs_h, mevecs_h, e1, e2 = p.half_operands()
    assert evecs_h.dtype == mevecs_h.dtype == torch.float16 and evecs_h.shape == mevecs_h.shape == p.evecs.shape
    assert e1.dtype == e2.dtype == torch.int32 and tuple(e1.shape) == tuple(e2.shape) == (3,)
    bits = lambda a: np.ascontiguousarray(a).view(np.int16)
    for b, n in enumerate(p.n_verts):
        mass, evecs = p.mass[b, :n].numpy(), p.evecs[b, :n].numpy()
        for name, exact, got, e in (("evecs", evecs.astype(np.float64), evecs_h, e1), ("mevecs", mass.astype(np.float64)[:, None] * evecs, mevecs_h, e2)):
            assert int(e[b]) == hs.window_exponent(exact), (name, b)
            scaled = np.ldexp(exact, int(e[b]))
            assert 2.0 ** 14 <= np.abs(scaled).max() < 2.0 ** 15, (name, b)
            # 2^-e operand_h is the fp16 rounding of the scaled operand: one rounding of the exact float64 value, bit for bit
            assert np.array_equal(bits(got[b, :n].numpy()), bits(scaled.astype(np.float16))), (name, b)
            assert float(got[b, :n].abs().max()) <= 2.0 ** 15
            assert bool((got[b, n:] == 0).all()), (name, b, "padding")
        want = hs.half_operands(mass, evecs)
        assert (int(e1[b]), int(e2[b])) == want[2:]


def test_half_operands_of_zeros_and_hostile_padding():
    op = lc.operators("f")
    zero = (None, op[1], None, op[3], torch.zeros_like(op[4]), op[5], op[6])
    p = layers.pack_operators([lc.operators("t"), zero])
    p.evecs[1, 81:] = float("nan")                              # rows behind a mesh's count are not looked at
    evecs_h, mevecs_h, e1, e2 = p.half_operands()
    assert int(e1[1]) == 0 and int(e2[1]) == 0
    assert bool((evecs_h[1] == 0).all()) and bool((mevecs_h[1] == 0).all())
    assert bool(torch.isfinite(evecs_h).all()) and bool(torch.isfinite(mevecs_h).all())


def test_half_operands_round_once():
    """a product mass * evecs whose float32 rounding lands on an fp16 tie: two roundings would go to the even neighbour, one does not"""
    one = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30], dtype=torch.float64)      # just above the tie between 1 and 1 + 2^-10
    assert float(one.to(torch.float32).to(torch.float16)) == 1.0                  # (float32 first: the tie, then to even)
    assert float(layers._round_to_half(one)) == 1.0 + 2.0 ** -10
    assert float(layers._round_to_half(-one)) == -(1.0 + 2.0 ** -10)
    grid = torch.tensor([0.0, 1.0, -2.5, 65504.0, 2.0 ** -24, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=torch.float64)
    assert torch.equal(layers._round_to_half(grid), torch.from_numpy(grid.numpy().astype(np.float16)))


def test_half_operands_are_cached_until_the_pack_moves():
    p = layers.pack_operators([lc.operators("t")])
    first = p.half_operands()
    assert all(a is b for a, b in zip(first, p.half_operands()))
    moved = p.to("cpu")
    assert moved._half is None and p._half is first
    assert torch.equal(moved.half_operands()[0], first[0]) and moved.half_operands()[0] is not first[0]
    assert [tuple(getattr(moved, k).shape) for k in p.FIELDS] == [tuple(getattr(p, k).shape) for k in p.FIELDS]


# ---------------------------------------------------------------------------------------------------------------- refusals, routing
def test_dtype_obstacles_name_the_condition():
    net = lc.network("a")
    f32, f16, bf16 = (torch.zeros((4, 19), dtype=d) for d in (torch.float32, torch.float16, torch.bfloat16))
    assert net._dtype_obstacle([f32]) is None
    assert "float32" in net._dtype_obstacle([f16])
    half = copy.deepcopy(net).half()
    assert half.is_half() and not net.is_half()
    assert half._dtype_obstacle([f32]) is None and half._dtype_obstacle([f16, f32]) is None
    assert "float16 or float32" in half._dtype_obstacle([f16, bf16])
    mixed = copy.deepcopy(net).half()
    mixed.last_lin.float()
    why = mixed._dtype_obstacle([f32])
    assert "all float32 or all float16" in why and "float16, float32" in why
    assert "bfloat16" in copy.deepcopy(net).bfloat16()._dtype_obstacle([f32])
    assert {k: layers.AUTO_DEVICE[k] for k in ("single", "batch")} == {"single": True, "batch": True}
    assert set(layers.AUTO_DEVICE) == {"single", "batch", "single_half", "batch_half"}


def test_half_module_on_the_cpu_is_refused_by_the_device_route():
    net = lc.network("a").half()
    x, kw = lc.call_arguments("a")
    with pytest.raises(RuntimeError, match="route='device'.*GPU"):
        net(x, route="device", **kw)


def autocast_run(net, x, kw):
    """the torch route as the reference's driver runs a halved model: torch.no_grad() under autocast (here the CPU's, in float16)"""
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
        return net(x, route="auto", **kw)


def test_auto_takes_torch_for_a_half_module_without_a_gpu():
    net = lc.network("a").half()
    x, kw = lc.call_arguments("a")
    y = autocast_run(net, x, kw)
    assert net.last_route == "torch" and y.shape == (lc.golden()["a_y_ref32"].shape) and bool(torch.isfinite(y).all())


# ---------------------------------------------------------------------------------------------------------------- accuracy of the route
def seeded(width, blocks, seed):
    torch.manual_seed(seed)
    net = layers.DiffusionNet(C_in=24, C_out=16, C_width=width, N_block=blocks).eval()
    with torch.no_grad():
        for b in net.blocks:
            b.diffusion.diffusion_time.copy_(0.05 * torch.rand(width))
    x = torch.randn((160, 24))
    _, mass, _, evals, evecs, gX, gY = lc.operators("t")
    cfg = dict(N_block=blocks, with_gradient_features=True, with_gradient_rotations=True, outputs_at="vertices", last_activation=None)
    return net, cfg, x, dict(mass=mass, evals=evals, evecs=evecs, gradX=gX, gradY=gY)


def fixture_case(case):
    net = lc.network(case)
    x, kw = lc.call_arguments(case)
    return net, lc.config(case), x, kw


def restate_arguments(x, kw):
    """the call's tensors as dnet_layers_restate.forward and dnet_half_restate.forward take them"""
    dense = lambda t: None if t is None else t.to_dense().double().numpy()
    return dict(x=x.numpy(), mass=kw["mass"].numpy(), evals=kw["evals"].numpy(), evecs=kw["evecs"].numpy(), Gx=dense(kw.get("gradX")), Gy=dense(kw.get("gradY")),
                faces=None if kw.get("faces") is None else kw["faces"].numpy())


CASES = [("w128", lambda: seeded(128, 4, 1)), ("w256", lambda: seeded(256, 8, 2))] + [(c, functools.partial(fixture_case, c)) for c in lc.CASES]


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_restatement_is_no_worse_than_the_autocast_route(name, make):
    """Against the float64 network on the half-rounded parameters, the RMS error of the route (its roundings, exact sums) does not exceed
    that of the torch route under torch.autocast("cpu", dtype=torch.float16): that route rounds every intermediate to fp16, this one
    the matrix operands only."""
    net, cfg, x, kw = make()
    half = copy.deepcopy(net).half()
    args = restate_arguments(x, kw)
    params = hs.half_params({k: v.detach().numpy() for k, v in net.state_dict().items()})
    exact, _ = rs.forward(cfg, params, args["x"].astype(np.float64), args["mass"], args["evals"], args["evecs"], args["Gx"], args["Gy"], args["faces"])
    torch_err = hs.rms(autocast_run(half, x, kw).double().numpy(), exact)
    for out16 in (False, True):
        got = hs.forward(cfg, params, **args, out16=out16)
        err = hs.rms(got, exact)
        print(f"{name}: rms error of the restated route ({'fp16' if out16 else 'unrounded'} output) {err:.3e}, of the autocast torch route {torch_err:.3e}, "
              f"ratio {err / torch_err:.3f}")
        assert np.all(np.isfinite(got)) and err <= torch_err, (name, out16, err, torch_err)

"""The restatements of the mixed-precision DiffusionNet backward (tests/dnet_mixed_restate.py) and the parts of the route that need no
GPU: each restated formula against float64 autograd of the same expression on operands that the declared roundings leave unchanged,
the masked oracle against plain float64 autograd, the loss scales of the whole-network cases, what compute_dtype= does without a GPU,
and the CPU emulation of the GPU acceptance: the route restated with every rounding applied against the torch route under
torch.autocast("cpu", dtype=torch.float16), both compared with the masked oracle under their own masks."""
import copy
import math

import numpy as np
import pytest
import torch

import dnet_backward_restate as br
import dnet_half_restate as hr
import dnet_layers_checks as lc
import dnet_mixed_checks as mc
import dnet_mixed_restate as mr
from densematcher_amd.diffusion_net import layers


def rnd16(seed, *shape, scale=1.0):
    """random values that fp16 holds exactly: the roundings of the restatement leave them unchanged"""
    return mr.h16(scale * np.random.default_rng(seed).standard_normal(shape))


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def close(got, ref, tag):
    err = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
    print(f"{tag}: max |numpy - autograd| / max |autograd| = {err:.3e}")
    assert err <= 1e-12, (tag, err)


# ---------------------------------------------------------------------------------------------------------------- 1. formulas
@pytest.mark.parametrize("act", [0, 1])
def test_linear_backward_formula(act):
    N, Co, widths = 23, 7, (5, 3, 4)
    srcs, W, b, dY = [rnd16(i, N, w) for i, w in enumerate(widths)], rnd16(5, Co, sum(widths)), rnd16(6, Co), rnd16(7, N, Co)
    srcs[1] = srcs[1].astype(np.float16)                                    # an fp16 source is read as it is
    ts, tW, tb = [t64(s) for s in srcs], t64(W), t64(b)
    y = torch.cat(ts, -1) @ tW.T + tb
    y = torch.relu(y) if act else y
    (y * t64(dY, False)).sum().backward()
    d_src, dW, db = mr.linear_backward(dY, srcs, W, y.detach().numpy() if act else None)
    for i in range(3):
        close(d_src[i], ts[i].grad.numpy(), f"linear d_src{i} act={act}")
    close(dW, tW.grad.numpy(), "linear dW")
    close(db, tb.grad.numpy(), "linear db")
    for bound in mr.linear_backward_bound(dY, srcs, W, y.detach().numpy() if act else None)[1:]:
        assert np.all(np.isfinite(bound)) and np.all(bound >= 0)


def test_diffuse_backward_formula():
    """masses that are powers of two and eigenvectors that fp16 holds: half_operands() rounds nothing.  The coefficient is rounded to
    fp32 by definition: autograd differentiates c(t) = coef * exp(-evals (t - t0)) at t0, whose value is coef and slope -evals coef."""
    N, K, Cw = 31, 6, 5
    g = np.random.default_rng(0)
    x, evecs, dO = rnd16(1, N, Cw), rnd16(2, N, K, scale=0.3), rnd16(3, N, Cw)
    mass, evals = 2.0 ** -g.integers(6, 9, N), np.sort(40.0 * g.random(K)).astype(np.float32)
    times = (0.05 * g.random(Cw) + 1e-3).astype(np.float32)
    eh, mh, e1, e2 = mr.half_operands(mass, evecs)
    assert np.array_equal(np.ldexp(eh, -e1), evecs) and np.array_equal(np.ldexp(mh, -e2), mass[:, None] * evecs)
    coef = hr.coefficients(evals, times)
    tx, tt, E, m, ev = t64(x), t64(times), t64(evecs, False), t64(mass, False), t64(evals, False)
    c = t64(coef, False) * torch.exp(-ev[:, None] * (tt - tt.detach())[None, :])
    out = E @ (c * (E.T @ (m[:, None] * tx)))
    np.testing.assert_allclose(out.detach().numpy(), hr.diffuse(x, mass, evals, evecs, times), rtol=1e-12, atol=1e-15)
    (out * t64(dO, False)).sum().backward()
    dx, dt = mr.diffuse_backward(dO, x, mass, evals, evecs, times)
    close(dx, tx.grad.numpy(), "diffuse dx")
    close(dt, tt.grad.numpy(), "diffuse dtimes")
    only_x = mr.diffuse_backward(dO, None, mass, evals, evecs, times)
    assert only_x[1] is None and np.array_equal(only_x[0], dx)
    for bound in mr.diffuse_backward_bound(dO, x, mass, evals, evecs, times):
        assert np.all(np.isfinite(bound)) and np.all(bound >= 0)


@pytest.mark.parametrize("rot", [True, False])
def test_gradfeat_backward_formula(rot):
    N, Cw = 17, 6
    g = np.random.default_rng(4)
    Gx = np.random.default_rng(10).standard_normal((N, N)) * (g.random((N, N)) < 0.3)
    Gy = np.random.default_rng(11).standard_normal((N, N)) * (g.random((N, N)) < 0.3)
    x, dO = np.random.default_rng(12).standard_normal((N, Cw)) * 0.3, np.random.default_rng(13).standard_normal((N, Cw))
    A_re, A_im = rnd16(14, Cw, Cw, scale=0.4), (rnd16(15, Cw, Cw, scale=0.4) if rot else None)
    tx, tR, tI = t64(x), t64(A_re), (t64(A_im) if rot else None)
    vx, vy = t64(Gx, False) @ tx, t64(Gy, False) @ tx
    b_re, b_im = (vx @ tR.T - vy @ tI.T, vy @ tR.T + vx @ tI.T) if rot else (vx @ tR.T, vy @ tR.T)
    out = torch.tanh(vx * b_re + vy * b_im)
    np.testing.assert_allclose(out.detach().numpy(), hr.gradfeat(x, Gx, Gy, A_re, A_im)[0], rtol=1e-12, atol=1e-15)
    (out * t64(dO, False)).sum().backward()
    dx, dRe, dIm = mr.gradfeat_backward(dO, x, Gx, Gy, A_re, A_im)         # (round_mid=False: the intermediates are not rounded)
    close(dx, tx.grad.numpy(), f"gradfeat dx rotations={rot}")
    close(dRe, tR.grad.numpy(), "gradfeat dA_re")
    if rot:
        close(dIm, tI.grad.numpy(), "gradfeat dA_im")
    else:
        assert dIm is None
    mid = mr.gradfeat_backward(dO, x, Gx, Gy, A_re, A_im, round_mid=True)
    bounds = mr.gradfeat_backward_bound(dO, x, Gx, Gy, A_re, A_im)
    for got, ref, bound in zip(mid, (dx, dRe, dIm), bounds):                # the declared roundings of the intermediates lie inside the bound
        assert bound is None or (np.all(np.isfinite(bound)) and np.all(np.abs(got - ref) <= bound))


# ---------------------------------------------------------------------------------------------------------------- 2. the masked oracle
@pytest.mark.parametrize("case", ["a", "c"])
def test_masked_oracle_under_the_float64_masks_is_float64_autograd(case):
    c = mc.Case(case, "cpu")
    ops = br.dense_operators(c.packed, torch.float64)
    params = mr.rounded_parameters(c.net, torch.float64)
    leaves = [x.double().requires_grad_() for x in c.xs]
    ys, pre = br.dense_network(c.net, params, leaves, ops, faces=c.faces)
    sum((y * g.double()).sum() for y, g in zip(ys, c.gs)).backward()
    masks = [[z.detach() > 0 for z in per_mesh] for per_mesh in pre]
    want = {name: p.grad for name, p in params.items()}
    got, top, _ = mr.oracle_gradients(c.net, c.xs, ops, c.gs, masks, scale=1.0, faces=c.faces)
    for name, w in want.items():
        assert float((got[name] - w).abs().max()) <= 1e-12 * float(w.abs().max()), name
    for x, leaf in zip(got["x"], leaves):
        assert float((x.grad - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
    assert top > 0


# ---------------------------------------------------------------------------------------------------------------- 3. the switch
def test_mixed_device_route_without_a_gpu_names_the_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    net = lc.network("a")
    x, kw = lc.call_arguments("a")
    with pytest.raises(RuntimeError, match="GPU"):
        net(x, route="device", differentiable=True, compute_dtype=torch.float16, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        net.forward_many([x], layers.pack_operators([lc.operators("t")]), differentiable=True, compute_dtype=torch.float16)


def test_obstacles_of_the_mixed_route(monkeypatch):
    """the dtype obstacles, reached on the CPU by letting the two device checks in front of them pass"""
    net = lc.network("a")
    x, kw = lc.call_arguments("a")
    half = copy.deepcopy(net).half()
    for cd in (None, torch.float16):                          # a halved module: today's text, with or without compute_dtype
        why = half._device_obstacle([x], (), True, 16, cd is not None)
        assert why is None or "GPU" in why
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    fake = lambda t: type("OnGpu", (), {"is_cuda": True, "dtype": t.dtype, "requires_grad": t.requires_grad})()
    for cd in (False, True):
        assert half._device_obstacle([fake(x)], (), True, 16, cd) == "the parameters and inputs must be float32 (the fp16 kernels have no backward)"
    assert "float32 or float16, not float64" in net._device_obstacle([fake(x.double())], (), True, 16, True)
    assert "must not require grad" in net._device_obstacle([fake(x.half().requires_grad_())], (), True, 16, True)
    assert net._device_obstacle([fake(x.half())], (), True, 16, True) == "the parameters must be on the GPU"      # (the next check: the dtypes passed)
    assert net._device_obstacle([fake(x.half())], (), True, 16, False) == "the parameters and inputs must be float32 (the fp16 kernels have no backward)"
    imp = copy.deepcopy(net)
    imp.diffusion_method = "implicit_dense"
    assert "spectral" in imp._device_obstacle([fake(x)], (), True, 16, True)


@pytest.mark.parametrize("route", ["torch", "auto", "device"])
def test_another_compute_dtype_is_a_value_error(route):
    net = lc.network("a")
    x, kw = lc.call_arguments("a")
    for bad in (torch.bfloat16, torch.float32, torch.float64):
        with pytest.raises(ValueError, match="compute_dtype"):
            net(x, route=route, differentiable=True, compute_dtype=bad, **kw)
        with pytest.raises(ValueError, match="compute_dtype"):
            net.forward_many([x], layers.pack_operators([lc.operators("t")]), differentiable=True, compute_dtype=bad)


@pytest.mark.parametrize("route", ["torch", "auto"])
def test_compute_dtype_is_ignored_by_the_other_routes(route):
    net = lc.network("a")                                                   # (module and input on the CPU: 'auto' has an obstacle anywhere)
    x, kw = lc.call_arguments("a")
    g = torch.from_numpy(mc.rnd(3, 160, 24))
    grads = []
    for cd in (None, torch.float16):
        net.zero_grad()
        xi = x.clone().requires_grad_()
        y = net(xi, route=route, differentiable=True, compute_dtype=cd, **kw)
        assert net.last_route == "torch" and y.requires_grad and y.dtype == torch.float32
        (y * g).sum().backward()
        grads.append([y.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert all(float(t.abs().max()) > 0 for t in grads[0])


# ---------------------------------------------------------------------------------------------------------------- 4. the acceptance, emulated
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "many"])
def test_the_loss_scales(case):
    """SCALE is the largest s that keeps the largest staged gradient operand of the masked oracle (under the emulated route's masks) below
    2^13 and every gradient below 2^16"""
    c = mc.Case(case, "cpu")
    _, masks = mc.emulated_run(c)
    grads, top = c.oracle(masks)
    largest = max(float(g.abs().max()) for g in grads.values())
    print(f"case {case}: s = {mc.SCALE[case]}: the largest staged gradient operand {top:.4e} = 2^{math.log2(top):.2f}, the largest gradient "
          f"{largest:.4e} = 2^{math.log2(largest):.2f}")
    assert top < 2.0 ** 13 and largest < 2.0 ** 16
    assert 2 * top >= 2.0 ** 13 or 2 * largest >= 2.0 ** 16           # s + 1 would break one of the two


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "many"])
def test_cpu_emulation_of_the_acceptance(case):
    """The GPU acceptance (tests/test_gpu_dnet_mixed.py) with both sides on the CPU: the restated route in place of the kernels, CPU
    autocast in place of the GPU's.  The figures are printed (DESIGN.md records them beside the GPU's); asserted is the acceptance's rule."""
    c = mc.Case(case, "cpu")
    emu, emu_masks = mc.emulated_run(c)
    auto, auto_masks = mc.autocast_run(c, "cpu")
    ref_emu, top = c.oracle(emu_masks)
    ref_auto, _ = c.oracle(auto_masks)
    flips = sum(int((a != b).sum()) for la, lb in zip(emu_masks, auto_masks) for a, b in zip(la, lb))
    print(f"case {case}: {flips} ReLU mask entries differ between the two runs; largest staged operand 2^{math.log2(top):.2f}")
    top_e, top_a = mc.report(f"case {case} (CPU emulation)", br.figures(emu, ref_emu), br.figures(auto, ref_auto), ("restated route", "CPU autocast"))
    assert top_e <= top_a, (case, top_e, top_a)

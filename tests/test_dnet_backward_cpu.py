"""The restatements of the DiffusionNet backward pass (tests/dnet_backward_restate.py) and the parts of the differentiable device route that
need no GPU: each NumPy backward formula against float64 autograd of the matching torch expression, the dense network restatement
against route="torch", PackedOperators.transposed_rows() against the dense operators, and what differentiable= does without a GPU."""
import numpy as np
import pytest
import torch

import dnet_backward_restate as br
import dnet_layers_checks as lc
import dnet_layers_restate as rs
from densematcher_amd.diffusion_net import layers


def rnd(seed, *shape, scale=1.0):
    return scale * np.random.default_rng(seed).standard_normal(shape)


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def close(got, ref, tag):
    err = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
    print(f"{tag}: max |numpy - autograd| / max |autograd| = {err:.3e}")
    assert err <= 1e-12, (tag, err)                     # two float64 evaluations of sums of at most a few hundred terms


# ---------------------------------------------------------------------------------------------------------------- 1. formulas
@pytest.mark.parametrize("relu", [False, True])
def test_linear_backward_formula(relu):
    N, Co, widths = 23, 7, (5, 3, 4)
    srcs, W, b, dY = [rnd(i, N, w) for i, w in enumerate(widths)], rnd(5, Co, sum(widths)), rnd(6, Co), rnd(7, N, Co)
    ts, tW, tb = [t64(s) for s in srcs], t64(W), t64(b)
    y = torch.cat(ts, -1) @ tW.T + tb
    y = torch.relu(y) if relu else y
    (y * t64(dY, False)).sum().backward()
    d_src, dW, db = br.linear_backward(dY, srcs, W, y.detach().numpy() if relu else None)
    for i in range(3):
        close(d_src[i], ts[i].grad.numpy(), f"linear d_src{i} relu={relu}")
    close(dW, tW.grad.numpy(), "linear dW")
    close(db, tb.grad.numpy(), "linear db")
    assert y.detach().numpy().shape == rs.linear(srcs, W, b, None, relu).shape


def test_diffuse_backward_formula():
    N, K, Cw = 31, 6, 5
    g = np.random.default_rng(0)
    x, evecs, dO = rnd(1, N, Cw), rnd(2, N, K, scale=0.3), rnd(3, N, Cw)
    mass, evals = 0.002 + 0.01 * g.random(N), np.sort(40.0 * g.random(K))
    times = (0.05 * g.random(Cw) + 1e-3).astype(np.float32).astype(np.float64)      # (the restatement takes the times in float32)
    tx, tt, E, m, ev = t64(x), t64(times), t64(evecs, False), t64(mass, False), t64(evals, False)
    out = E @ (torch.exp(-ev[:, None] * tt[None, :]) * (E.T @ (m[:, None] * tx)))
    np.testing.assert_allclose(out.detach().numpy(), rs.diffuse(x, mass, evals, evecs, times), rtol=1e-12, atol=1e-15)
    (out * t64(dO, False)).sum().backward()
    dx, dt = br.diffuse_backward(dO, x, mass, evals, evecs, times)
    close(dx, tx.grad.numpy(), "diffuse dx")
    close(dt, tt.grad.numpy(), "diffuse dtimes")


@pytest.mark.parametrize("rot", [True, False])
def test_gradfeat_backward_formula(rot):
    N, Cw = 17, 6
    g = np.random.default_rng(4)
    Gx, Gy = rnd(10, N, N) * (g.random((N, N)) < 0.3), rnd(11, N, N) * (g.random((N, N)) < 0.3)
    x, dO, A_re, A_im = rnd(12, N, Cw, scale=0.3), rnd(13, N, Cw), rnd(14, Cw, Cw, scale=0.4), (rnd(15, Cw, Cw, scale=0.4) if rot else None)
    tx, tR, tI = t64(x), t64(A_re), (t64(A_im) if rot else None)
    vx, vy = t64(Gx, False) @ tx, t64(Gy, False) @ tx
    b_re, b_im = (vx @ tR.T - vy @ tI.T, vy @ tR.T + vx @ tI.T) if rot else (vx @ tR.T, vy @ tR.T)
    out = torch.tanh(vx * b_re + vy * b_im)
    np.testing.assert_allclose(out.detach().numpy(), rs.gradfeat(x, Gx, Gy, A_re, A_im)[0], rtol=1e-12, atol=1e-15)
    (out * t64(dO, False)).sum().backward()
    dx, dRe, dIm = br.gradfeat_backward(dO, x, Gx, Gy, A_re, A_im)
    close(dx, tx.grad.numpy(), f"gradfeat dx rotations={rot}")
    close(dRe, tR.grad.numpy(), "gradfeat dA_re")
    if rot:
        close(dIm, tI.grad.numpy(), "gradfeat dA_im")
    else:
        assert dIm is None
    for bound in br.gradfeat_backward_bound(dO, x, Gx, Gy, A_re, A_im):
        assert bound is None or (np.all(np.isfinite(bound)) and np.all(bound >= 0))


# ---------------------------------------------------------------------------------------------------------------- 2. network
@pytest.mark.parametrize("case", ["a", "b"])
def test_dense_network_reproduces_the_torch_route_in_float32(case):
    """two fp32 evaluations of the same expressions (sparse and dense gradient products): check_output's margin for another order"""
    net = lc.network(case)
    x, kw = lc.call_arguments(case)
    with torch.no_grad():
        want = net(x, route="torch", **kw)
        packed = layers.pack_operators([lc.operators(k) for k in lc.config(case)["meshes"]])
        got, pre = br.dense_network(net, br.leaf_parameters(net, torch.float32), [x], br.dense_operators(packed, torch.float32))
    figure = float((got[0] - want).abs().max() / want.abs().max())
    bound = 4.0 * float(lc.golden()[f"{case}_f32_floor"]) + 2.0 ** -23
    print(f"case {case}: dense restatement against route='torch', max |diff| / max |ref| = {figure:.3e} (bound {bound:.3e}); "
          f"{len(pre)} ReLU layers, margin {br.relu_margin(pre):.3e}")
    assert got[0].shape == want.shape and figure <= bound


def test_dense_network_float64_is_close_to_the_recorded_reference():
    net = lc.network("a")
    x, _ = lc.call_arguments("a")
    packed = layers.pack_operators([lc.operators("t")])
    with torch.no_grad():
        got, _ = br.dense_network(net, br.leaf_parameters(net, torch.float64), [x.double()], br.dense_operators(packed, torch.float64))
    lc.check_output("a", got[0], "float64 dense restatement")


# ---------------------------------------------------------------------------------------------------------------- 3. transposed rows
def test_transposed_rows_of_a_ragged_pack():
    keys = ("t", "r", "f")
    p = layers.pack_operators([lc.operators(k) for k in keys])
    rl, cols, gx, gy = p.transposed_rows()
    assert p.transposed_rows()[1] is cols                                   # built once
    Bn, N, w = cols.shape
    assert rl.dtype == torch.int32 and cols.dtype == torch.int32 and gx.dtype == torch.float32 and tuple(rl.shape) == (Bn, N) and gx.shape == gy.shape == cols.shape
    assert int(rl.max()) == w
    for b, n in enumerate(p.n_verts):
        for which, vals in (("gx", gx), ("gy", gy)):
            dense = torch.from_numpy(rs.dense_rows(rl[b, :n].numpy(), cols[b, :n].numpy(), vals[b, :n].numpy(), n))
            assert torch.equal(dense, p.dense_grad(b, which).T.double()), (b, which)
        for i in range(n):
            c = cols[b, i, :int(rl[b, i])]
            assert bool((c[1:] > c[:-1]).all()) and int(c.max()) < n
        assert bool((rl[b, n:] == 1).all()) and bool((cols[b, n:, 0] == torch.arange(n, N)).all())
        assert bool((gx[b, n:] == 0).all()) and bool((gy[b, n:] == 0).all())


def test_transposed_rows_of_an_unsymmetric_pattern():
    n = 5
    ix = torch.tensor([[0, 0, 1, 3, 3, 3], [1, 4, 4, 0, 1, 2]])             # no (j, i) for any (i, j); vertex 2 and 4 have empty rows
    iy = torch.tensor([[0, 1, 3], [2, 4, 0]])
    gX = torch.sparse_coo_tensor(ix, torch.arange(1.0, 7.0), (n, n)).coalesce()
    gY = torch.sparse_coo_tensor(iy, torch.tensor([-1.0, -2.0, -3.0]), (n, n)).coalesce()
    p = layers.pack_operators([(None, torch.ones(n), None, torch.zeros(1), torch.zeros((n, 1)), gX, gY)])
    rl, cols, gx, gy = p.transposed_rows()
    # the empty rows 2 and 4 are stored as (2, 2) and (4, 4) with value 0 and transpose as such; column 3 has no entry: the padding row
    assert rl[0].tolist() == [1, 2, 3, 1, 3] and cols[0, 2, :3].tolist() == [0, 2, 3] and cols[0, 4, :3].tolist() == [0, 1, 4]
    assert int(cols[0, 3, 0]) == 3 and float(gx[0, 3, 0]) == 0.0 and float(gy[0, 3, 0]) == 0.0
    for which, vals, ref in (("gx", gx, gX), ("gy", gy, gY)):
        dense = torch.from_numpy(rs.dense_rows(rl[0].numpy(), cols[0].numpy(), vals[0].numpy(), n)).float()
        assert torch.equal(dense, ref.to_dense().T) and torch.equal(dense, p.dense_grad(0, which).T)


# ---------------------------------------------------------------------------------------------------------------- 4. the switch
def test_differentiable_device_route_without_a_gpu_names_the_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    net = lc.network("a")
    x, kw = lc.call_arguments("a")
    with pytest.raises(RuntimeError, match="GPU"):
        net(x, route="device", differentiable=True, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        net.forward_many([x], layers.pack_operators([lc.operators("t")]), differentiable=True)


@pytest.mark.parametrize("route", ["torch", "auto"])
def test_differentiable_is_ignored_by_the_other_routes(route):
    net = lc.network("a")                                                   # (module and input on the CPU: 'auto' has an obstacle anywhere)
    x, kw = lc.call_arguments("a")
    g = torch.from_numpy(rnd(3, 160, 24)).float()
    grads = []
    for flag in (False, True):
        net.zero_grad()
        xi = x.clone().requires_grad_()
        y = net(xi, route=route, differentiable=flag, **kw)
        assert net.last_route == "torch" and y.requires_grad
        (y * g).sum().backward()
        grads.append([xi.grad.clone()] + [p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert all(float(t.abs().max()) > 0 for t in grads[0])

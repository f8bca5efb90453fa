"""diffusion_net.layers without a GPU: the reference's parameter names, the torch route against the reference's recorded float32 run
(tests/golden/fx_dnet_layers.npz), the float64 restatement, the in-place clamp of the times, pack_operators and the choice of route."""
import numpy as np
import pytest
import torch

import dnet_checks as dc
import dnet_layers_checks as lc
import dnet_layers_restate as rs
from densematcher_amd.diffusion_net import layers


@pytest.mark.parametrize("case", lc.CASES)
def test_parameter_names_order_and_shapes(case):
    fx = lc.golden()
    net = lc.network(case, load=False)
    got = [(n, tuple(p.shape)) for n, p in net.named_parameters()]
    want = [(n, tuple(fx[f"{case}_p{i}"].shape)) for i, n in enumerate(lc.names(case))]
    assert got == want
    assert list(net.state_dict().keys()) == lc.names(case)
    net.load_state_dict(lc.state(case), strict=True)
    if case == "a":
        assert {"first_lin.weight", "block_1.diffusion.diffusion_time", "block_1.gradient_features.A_re.weight",
                "block_1.mlp.miniMLP_mlp_layer_001.bias"} <= set(net.state_dict())
        # dropout=True by default: a Dropout in front of every MLP layer but the first, as the reference places them
        assert [type(m).__name__ for m in net.blocks[0].mlp] == ["Linear", "ReLU", "Dropout", "Linear", "ReLU", "Dropout", "Linear"]
        assert [n for n, _ in net.blocks[0].mlp.named_children()][2] == "miniMLP_mlp_layer_dropout_001"


@pytest.mark.parametrize("case", lc.CASES)
def test_torch_route_against_the_reference_float32_run(case):
    net = lc.network(case)
    x, kw = lc.call_arguments(case)
    with torch.no_grad():
        y = net(x, route="torch", **kw)
    assert net.last_route == "torch" and y.dtype == torch.float32
    lc.check_output(case, y, "torch route (CPU)")


@pytest.mark.parametrize("case", lc.CASES)
def test_restatement_is_pinned_to_the_recorded_run(case):
    """max |y_ref32 - y64| / max |y64| <= f32_floor, the figure tools/make_golden_dnet_layers.py recorded from this same restatement;
    2^-40 on top is the freedom of the float64 evaluation order (another BLAS) in y64, nine orders below the floor"""
    fx, cfg = lc.golden(), lc.config(case)
    keys = cfg["meshes"]
    params = {n: fx[f"{case}_p{i}"] for i, n in enumerate(lc.names(case))}
    dense = lambda k, name: dc.dense(lc.operators(k)[{"gradX": 5, "gradY": 6}[name]])
    st = lambda name: np.stack([fx[f"{name}_{k}"] for k in keys])
    Gx, Gy = np.stack([dense(k, "gradX") for k in keys]), np.stack([dense(k, "gradY") for k in keys])
    if len(keys) == 1:
        y64, _ = rs.forward(cfg, params, fx[f"{case}_x"], st("mass")[0], st("evals")[0], st("evecs")[0], Gx[0], Gy[0], fx[f"faces_{keys[0]}"])
    else:
        y64, _ = rs.forward(cfg, params, fx[f"{case}_x"], st("mass"), st("evals"), st("evecs"), Gx, Gy)
    figure = np.abs(fx[f"{case}_y_ref32"].astype(np.float64) - y64).max() / np.abs(y64).max()
    print(f"case {case}: max |y_ref32 - y64| / max |y64| = {figure:.3e} (f32_floor {float(fx[f'{case}_f32_floor']):.3e})")
    assert figure <= float(fx[f"{case}_f32_floor"]) + 2.0 ** -40


def test_diffusion_time_is_clamped_in_place():
    fx = lc.golden()
    net = lc.network("a")
    before = [b.diffusion.diffusion_time.detach().clone() for b in net.blocks]
    assert all(float(t[0]) == 0.0 and float(t[1]) < 0.0 for t in before)
    x, kw = lc.call_arguments("a")
    with torch.no_grad():
        net(x, route="torch", **kw)
    for b, t in zip(net.blocks, before):
        assert torch.equal(b.diffusion.diffusion_time.data, torch.clamp(t, min=1e-8))
        assert isinstance(b.diffusion.diffusion_time, torch.nn.Parameter)
    assert np.array_equal(before[0].numpy(), fx["a_p4"])


# ---------------------------------------------------------------------------------------------------------------------
def _numpy_ell(key):
    """the ELL rows of mesh `key` built entry by entry from the fixture's triplets (float64 values), as the dict of
    MatchEngine.diffusion_operators holds them"""
    fx = lc.golden()
    n = fx[f"mass_{key}"].shape[0]
    rows = {}
    for name, slot in (("gradX", 0), ("gradY", 1)):
        for r, c, v in zip(fx[f"{name}_row_{key}"], fx[f"{name}_col_{key}"], fx[f"{name}_val_{key}"]):
            rows.setdefault(int(r), {}).setdefault(int(c), [0.0, 0.0])[slot] = float(v)
    nnz = max(len(v) for v in rows.values())
    row_len = np.ones(n, np.int32)
    cols = np.repeat(np.arange(n, dtype=np.int32)[:, None], nnz, axis=1)
    gx, gy = np.zeros((n, nnz)), np.zeros((n, nnz))
    for r, entries in rows.items():
        row_len[r] = len(entries)
        for q, c in enumerate(sorted(entries)):
            cols[r, q], gx[r, q], gy[r, q] = c, entries[c][0], entries[c][1]
    t = torch.from_numpy
    return {"mass": t(fx[f"mass_{key}"].astype(np.float64)), "evals": t(fx[f"evals_{key}"].astype(np.float64)),
            "evecs": t(fx[f"evecs_{key}"].astype(np.float64)), "row_len": t(row_len), "cols": t(cols), "gx": t(gx), "gy": t(gy)}


@pytest.mark.parametrize("key", ["t", "f"])
def test_pack_operators_rows_equal_the_sparse_matrices(key):
    op = lc.operators(key)
    p = layers.pack_operators([op])
    n = op[1].shape[0]
    assert p.n_verts == [n] and p.n_verts_dev is None
    assert p.cols.dtype == torch.int32 and p.row_len.dtype == torch.int32 and p.gx.dtype == torch.float32
    assert torch.equal(p.dense_grad(0, "gx"), op[5].to_dense()) and torch.equal(p.dense_grad(0, "gy"), op[6].to_dense())
    rl = p.row_len[0]
    assert int(rl.max()) == p.cols.shape[2] and int(rl.min()) >= 1
    for i in (0, n // 2, n - 1):                                     # ascending columns in a row
        c = p.cols[0, i, :int(rl[i])]
        assert bool((c[1:] > c[:-1]).all())
    if key == "f":
        assert int(rl.min()) == 4 and int(rl.max()) == 41
    assert torch.equal(p.mass[0], op[1]) and torch.equal(p.evals[0], op[3]) and torch.equal(p.evecs[0], op[4])


def test_pack_operators_ragged_and_dict_input():
    t, f = lc.operators("t"), lc.operators("f")
    p = layers.pack_operators([t, f])
    assert p.n_verts == [160, 81] and p.n_verts_dev.tolist() == [160, 81] and p.n_verts_dev.dtype == torch.int32
    assert p.mass.shape == (2, 160) and p.evecs.shape == (2, 160, 16) and p.cols.shape[:2] == (2, 160)
    assert bool((p.evecs[1, 81:] == 0).all()) and bool((p.mass[1, 81:] == 1).all()) and bool((p.gx[1, 81:] == 0).all())
    assert bool((p.row_len[1, 81:] == 1).all()) and torch.equal(p.cols[1, 81:, 0], torch.arange(81, 160, dtype=torch.int32))
    assert torch.equal(p.dense_grad(1, "gx"), f[5].to_dense()) and torch.equal(p.dense_grad(0, "gy"), t[6].to_dense())
    for key, op in (("t", t), ("f", f)):
        a, b = layers.pack_operators([op]), layers.pack_operators([_numpy_ell(key)])
        assert a.n_verts == b.n_verts
        for name in layers.PackedOperators.FIELDS:
            assert torch.equal(getattr(a, name), getattr(b, name)), (key, name)
    # the seven lists of get_all_operators are a mesh set too
    many = layers.pack_operators(tuple([t[i], f[i]] for i in range(7)))
    assert all(torch.equal(getattr(many, name), getattr(p, name)) for name in layers.PackedOperators.FIELDS)


# ---------------------------------------------------------------------------------------------------------------------
def test_routes():
    net = lc.network("a")
    x, kw = lc.call_arguments("a")
    with pytest.raises(RuntimeError, match="route='device'"):       # no GPU, or an input that is not on it
        net(x, route="device", **kw)
    with pytest.raises(ValueError):
        net(x, route="fast", **kw)
    with torch.no_grad():
        want = net(x, route="torch", **kw)
    # training mode with dropout
    net.train()
    assert net._device_obstacle([x]) is not None
    torch.manual_seed(0)
    y = net(x, route="auto", **kw)
    assert net.last_route == "torch" and y.requires_grad and not torch.equal(y.detach(), want)
    net.eval()
    # an input that requires grad
    xg = x.clone().requires_grad_(True)
    y = net(xg, route="auto", **kw)
    assert net.last_route == "torch"
    y.sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    with pytest.raises(RuntimeError):
        net(xg, route="device", **kw)
    # implicit_dense
    fx = dc.golden()
    n = fx["verts_t"].shape[0]
    L = torch.sparse_coo_tensor(torch.from_numpy(np.stack((fx["L_row_t"], fx["L_col_t"])).astype(np.int64)),
                                torch.from_numpy(fx["L_val_t"].astype(np.float32)), (n, n)).coalesce()
    imp = layers.DiffusionNet(C_in=19, C_out=4, C_width=8, N_block=1, dropout=False, diffusion_method="implicit_dense").eval()
    with torch.no_grad():
        y = imp(x, kw["mass"], L=L, gradX=kw["gradX"], gradY=kw["gradY"], route="auto")
    assert imp.last_route == "torch" and y.shape == (n, 4) and bool(torch.isfinite(y).all())
    assert "implicit_dense" in (imp._device_obstacle([x]) or "implicit_dense") or not torch.cuda.is_available()
    with pytest.raises(RuntimeError):
        imp(x, kw["mass"], L=L, gradX=kw["gradX"], gradY=kw["gradY"], route="device")


def test_tuple_input_equals_the_concatenated_input_on_the_torch_route():
    net = lc.network("a")
    x, kw = lc.call_arguments("a")
    parts = (x[:, :12].contiguous(), x[:, 12:16].contiguous(), x[:, 16:].contiguous())
    with torch.no_grad():
        assert torch.equal(net(parts, route="torch", **kw), net(x, route="torch", **kw))
        assert torch.equal(net(list(parts[:1]) + [x[:, 12:]], route="torch", **kw), net(x, route="torch", **kw))
    with pytest.raises(ValueError):
        net((x, x), route="torch", **kw)

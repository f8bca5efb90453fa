"""Shared by the aggregation network tests (CPU and GPU): the fixture tests/golden/fx_aggre.npz (tools/make_golden_aggre.py: the
reference's own float32 run of AggregationNetwork), one float64 restatement per case (tests/aggre_restate.py; computed once, shared, never
modified) and seeded cases for the kernel tests.  The bound is the project's: lift_checks.bound = (4 f32_floor + 2^-23) max |ref|, the
floor being the distance of the reference's float32 evaluation from exact arithmetic on the same inputs -- recorded in the fixture for
its cases, measured here for the seeded ones: the reference's torch expressions in float32 on the CPU against the restatement.  Never
the device code."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import aggre_restate as rs
import lift_checks as lc

CASES = ("a", "b")
check = lc.check


def golden():
    return lc.golden("fx_aggre.npz")


def case(c):
    """case c as a dict: names, state (name -> array), dims, proj, groups, x, level0.., y_ref32, f32_floor"""
    fx = golden()
    d = {k[2:]: v for k, v in fx.items() if k.startswith(c + "_")}
    d["names"] = [str(n) for n in d["names"]]
    d["state"] = {n: d[f"p{i}"] for i, n in enumerate(d["names"])}
    d["dims"], d["proj"], d["groups"] = [int(v) for v in d["dims"]], int(d["proj"]), int(d["groups"])
    return d


def _freeze(d):
    for v in d.values():
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def restated(c):
    d = case(c)
    return _freeze(rs.network(d["x"], d["state"], d["dims"], d["groups"]))


def model(c, device="cpu"):
    """AggregationNetwork with case c's weights, strict, in eval mode"""
    from densematcher_amd.featurizers.modules.projection_network import AggregationNetwork
    d = case(c)
    m = AggregationNetwork(feature_dims=d["dims"], projection_dim=d["proj"], num_norm_groups=d["groups"])
    m.load_state_dict({n: torch.from_numpy(np.array(v)) for n, v in d["state"].items()}, strict=True)
    return m.to(device).eval()


def floor(got32, ref64):
    ref64 = np.asarray(ref64, np.float64)
    got = got32.detach().cpu().double().numpy() if isinstance(got32, torch.Tensor) else np.asarray(got32, np.float64)
    return float(np.abs(got - ref64).max() / max(np.abs(ref64).max(), np.finfo(np.float64).tiny))


def _rng(*key):
    return np.random.default_rng([2024] + [int(k) for k in key])      # NumPy's PCG64: the same numbers on every machine


# ------------------------------------------------------------------------------------------------------------------ seeded networks
@functools.lru_cache(maxsize=None)
def seeded_network(dims=(8, 12, 20, 6), proj=16, groups=2, Bn=2, hw=(3, 5), seed=5):
    """A network in which every level has a shortcut (case a of the fixture has one without: the device route refuses it), every
    parameter from rng, an input, the restatement and the floor of the torch route on the CPU: a dict with net (on the CPU, eval), x,
    y64, levels64, floor."""
    from densematcher_amd.featurizers.modules.projection_network import AggregationNetwork
    rng = _rng(seed, proj, Bn, *hw)
    net = AggregationNetwork(feature_dims=list(dims), projection_dim=proj, num_norm_groups=groups).eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 4:
                v = rng.standard_normal(tuple(p.shape)) * (p.shape[1] * p.shape[2] * p.shape[3]) ** -0.5
            elif name.endswith("norm.weight"):
                v = 1.0 + 0.25 * rng.standard_normal(tuple(p.shape))
            else:
                v = 0.25 * rng.standard_normal(tuple(p.shape))
            p.copy_(torch.from_numpy(np.asarray(v, np.float32)))
    x = rng.standard_normal((Bn, sum(dims)) + tuple(hw)).astype(np.float32)
    state = {k: v.numpy().astype(np.float64) for k, v in net.state_dict().items()}
    ref = rs.network(x, state, list(dims), groups)
    with torch.no_grad():
        y32 = net(torch.from_numpy(x), route="torch")
    return _freeze({"net": net, "x": x, "y64": ref["y"], "levels64": ref["levels"], "floor": floor(y32, ref["y"])})


# ------------------------------------------------------------------------------------------------------------------ seeded kernel cases
@functools.lru_cache(maxsize=None)
def seeded_conv(L, Bn, P_h, P_w, Cin, Cout):
    """x (L, B, P_h, P_w, C_in) channels-last, w (L, C_out, C_in, 3, 3), packed (L, C_out, 9 C_in), ref64 (L, B, P_h, P_w, C_out), floor
    (F.conv2d in float32 on the CPU against the restatement)"""
    rng = _rng(3, L, Bn, P_h, P_w, Cin, Cout)
    x = rng.standard_normal((L, Bn, P_h, P_w, Cin)).astype(np.float32)
    w = (rng.standard_normal((L, Cout, Cin, 3, 3)) * (9 * Cin) ** -0.5).astype(np.float32)
    ref = np.stack([rs.conv3x3(x[l].transpose(0, 3, 1, 2), w[l]).transpose(0, 2, 3, 1) for l in range(L)])
    got = np.stack([F.conv2d(torch.from_numpy(x[l]).permute(0, 3, 1, 2), torch.from_numpy(w[l]), padding=1).permute(0, 2, 3, 1).numpy()
                    for l in range(L)])
    packed = np.ascontiguousarray(w.transpose(0, 1, 3, 4, 2).reshape(L, Cout, 9 * Cin))
    return _freeze({"x": x, "w": w, "packed": packed, "ref64": ref, "floor": floor(got, ref)})


@functools.lru_cache(maxsize=None)
def seeded_groupnorm(n_img, npix, Cw, G, offset=0.0, levels=1):
    """x (n_img, npix, C) rows; mean64 / rstd64 (n_img, G) with the floors of torch.native_group_norm in float32 on the CPU; gamma, beta
    (levels, C); mean32 / rstd32 the restated statistics rounded to fp32 and out64 = relu(((x - mean32) rstd32) gamma + beta) on them, with
    the floor of that expression in float32 on the CPU"""
    rng = _rng(4, n_img, npix, Cw, G, int(offset), levels)
    x = (offset + rng.standard_normal((n_img, npix, Cw))).astype(np.float32)
    gamma = (1.0 + 0.25 * rng.standard_normal((levels, Cw))).astype(np.float32)
    beta = (0.25 * rng.standard_normal((levels, Cw))).astype(np.float32)
    nchw = np.ascontiguousarray(x.transpose(0, 2, 1))[..., None]                      # (n_img, C, npix, 1)
    mean64, rstd64 = rs.group_stats(nchw, G)
    _, m32, r32 = torch.native_group_norm(torch.from_numpy(nchw), None, None, n_img, Cw, npix, G, rs.EPS)
    mean32, rstd32 = mean64.astype(np.float32), rstd64.astype(np.float32)
    lvl = np.arange(n_img) // (n_img // levels)
    rep = lambda s: np.repeat(s, Cw // G, axis=1)[:, None, :]                         # (n_img, 1, C)
    out64 = np.maximum((x.astype(np.float64) - rep(mean32).astype(np.float64)) * rep(rstd32) * gamma[lvl][:, None, :] + beta[lvl][:, None, :], 0.0)
    t = torch.from_numpy
    out32 = torch.relu((t(x) - t(rep(mean32))) * t(rep(rstd32)) * t(gamma[lvl][:, None, :]) + t(beta[lvl][:, None, :]))
    return _freeze({"x": x, "gamma": gamma, "beta": beta, "mean64": mean64, "rstd64": rstd64, "mean32": mean32, "rstd32": rstd32,
                    "floor_mean": floor(m32.reshape(n_img, G), mean64), "floor_rstd": floor(r32.reshape(n_img, G), rstd64),
                    "out64": out64, "floor_out": floor(out32, out64)})


def torch_gather(sources, size, R, step):
    """the reference's expressions (SDDINO.py:53-57, 76-88) in torch on whatever the sources are: interpolate, cat, rotate back, mean"""
    from densematcher_amd.featurizers.util import rotate
    cat = torch.cat([s if tuple(s.shape[2:]) == tuple(size) else F.interpolate(s, size=tuple(size), mode="bilinear", align_corners=False)
                     for s in sources], dim=1)
    if R == 1 and step == 0.0:
        return cat
    parts = cat.chunk(R, dim=0)
    total = torch.zeros_like(parts[0])
    for r in range(R):
        total += rotate(parts[r], -r * step)
    return total / R


@functools.lru_cache(maxsize=None)
def seeded_gather(size, shapes, R, Bn=2):
    """shapes ((C, h, w), ...): sources (R B, C, h, w) float32; ref64 the rows (B, P_h P_w, sum C) of the restatement with the rotation
    step 360 / R (0 for R = 1); floor: torch_gather in float32 on the CPU"""
    rng = _rng(6, R, Bn, *size, *[v for s in shapes for v in s])
    step = 360.0 / R if R > 1 else 0.0
    sources = [rng.standard_normal((R * Bn,) + tuple(s)).astype(np.float32) for s in shapes]
    ref = rs.gather(sources, size, R, step)
    got = torch_gather([torch.from_numpy(s) for s in sources], size, R, step)
    return _freeze({"sources": sources, "step": step, "ref64": rs.rows(ref), "floor": floor(rs.rows(got.numpy()), rs.rows(ref))})

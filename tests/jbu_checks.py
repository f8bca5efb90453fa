"""Shared by the JBU upsampling tests (CPU and GPU): the fixture tests/golden/fx_jbu.npz (tools/make_golden_jbu.py: the reference's own
float32 run of JBUStack), one float64 restatement per case (tests/jbu_restate.py; computed once, shared, never modified) and seeded
stages for the kernel tests.  The bound is the project's: lift_checks.bound = (4 f32_floor + 2^-23) max |ref|, the floor being the
distance of the reference's float32 evaluation from exact arithmetic on the same inputs (recorded in the fixture for its cases,
measured by seeded_stage for its own)."""
import functools

import numpy as np
import torch

import jbu_restate as rs
import lift_checks as lc

CASES = ("a", "b")
check = lc.check


def golden():
    return lc.golden("fx_jbu.npz")


def case(c):
    """case c as a dict: names, state (name -> array), src, img, stage1..4, kernel1, y_ref32, f32_floor"""
    fx = golden()
    d = {k[2:]: v for k, v in fx.items() if k.startswith(c + "_")}
    d["names"] = [str(n) for n in d["names"]]
    d["state"] = {n: d[f"p{i}"] for i, n in enumerate(d["names"])}
    return d


@functools.lru_cache(maxsize=None)
def restated(c):
    d = case(c)
    res = rs.stack(d["src"], d["img"], d["state"])
    for v in [res["y"], res["kernel1"]] + res["stages"]:
        v.setflags(write=False)
    return res


def model(c, device="cpu"):
    """JBUStack with case c's weights, strict, in eval mode"""
    from densematcher_amd.featup.upsamplers import JBUStack
    d = case(c)
    m = JBUStack(d["src"].shape[1])
    m.load_state_dict({n: torch.from_numpy(np.array(v)) for n, v in d["state"].items()}, strict=True)
    return m.to(device).eval()


def _floor(got32, ref64):
    return float(np.abs(np.asarray(got32, np.float64) - ref64).max() / np.abs(ref64).max())


@functools.lru_cache(maxsize=None)
def seeded_stage(Bn, Cw, h, w, seed=7):
    """One JBULearnedRange with seeded parameters (weights of standard deviation 1 / sqrt(fan_in), biases 0.1, range_temp 0 and
    sigma_spatial 1 moved by 0.25 standard deviations), a source and a guidance at twice its size (NumPy's PCG64:
    the same numbers on every machine), the float64 restatement of its kernels and output, and the floors of the three things the
    kernel tests compare -- the distance of the REFERENCE's expressions in float32 on the CPU (the torch route, pinned to the
    reference's recorded run by tests/test_jbu_cpu.py) from the restatement on these very inputs, relative to max |restatement|:
    a dict with up (module on the CPU), src, g, f64 (kernels), f32 (f64 rounded), out64 (the stage), apply64 (jbu_restate.apply on f32),
    floor_filters, floor_apply, floor_stage; arrays read-only."""
    import torch.nn.functional as F
    from densematcher_amd.featup.adaptive_conv import adaptive_conv
    from densematcher_amd.featup.upsamplers import JBULearnedRange
    rng = np.random.default_rng(seed + 1000 * Cw + 10 * h + w)
    up = JBULearnedRange(3, Cw, 32, radius=3).eval()
    with torch.no_grad():                  # every parameter from rng (the constructor's own values come from torch's global generator)
        for name, p in up.named_parameters():
            base = 1.0 if name == "sigma_spatial" else 0.0
            scale = 0.25 if p.dim() == 0 else (0.1 if p.dim() == 1 else p.shape[1] ** -0.5)        # weights: 1 / sqrt(fan_in)
            p.copy_(torch.from_numpy(np.asarray(base + scale * rng.standard_normal(tuple(p.shape)), np.float32)))
    src = rng.standard_normal((Bn, Cw, h, w)).astype(np.float32)
    g = rng.standard_normal((Bn, 3, 2 * h, 2 * w)).astype(np.float32)
    Wt = {k: v.numpy().astype(np.float64) for k, v in up.state_dict().items()}
    out64, f64 = rs.stage(src, g, Wt)
    f32 = f64.astype(np.float32)
    apply64 = rs.apply(src, f32)
    with torch.no_grad():
        ts, tg = torch.from_numpy(src), torch.from_numpy(g)
        k32 = up.combined_kernel(tg).reshape(f64.shape).numpy()
        hr = F.pad(F.interpolate(ts, size=tuple(g.shape[2:]), mode="bicubic", align_corners=False), [3] * 4, mode="reflect")
        a32 = adaptive_conv(hr, torch.from_numpy(f32).reshape(f32.shape[:3] + (7, 7)), route="torch").numpy()
        o32 = up(ts, tg, route="torch").numpy()
    d = {"up": up, "src": src, "g": g, "f64": f64, "f32": f32, "out64": out64, "apply64": apply64,
         "floor_filters": _floor(k32, f64), "floor_apply": _floor(a32, apply64), "floor_stage": _floor(o32, out64)}
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d

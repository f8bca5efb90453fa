#!/usr/bin/env python
"""
Time of a DiffusionNet forward pass at the shipped configuration on one GPU: the device route (DiffusionNet.forward_many on packed
operators: dm_dnet_linear_f32 / dm_dnet_diffuse_f32 / dm_dnet_gradfeat_f32) against the torch route (the reference's expressions on
PyTorch-ROCm, torch.mm with a sparse gradX / gradY per mesh) -- the baseline -- in the same process.

    python tools/dnet_forward_time.py [--meshes 16] [--half] [--out result.json]

Input: 16 perturbed tori of 2048 vertices (synth.torus_mesh(64, 32, perturb=0.1, seed=s)), k_eig = 128, operators from
MatchEngine.diffusion_operators.  Network: width 512, 8 blocks, C_in = 768 + 51 + 16 = 835 as three sources, C_out 512, eval mode,
seeded weights, times uniform in [0, 0.05).  Per route and per case (one mesh; the batch) two warm-up calls, then five timed windows
taken alternately between the routes; a window is `reps` calls between two device synchronisations on the host clock, and the figure
is the median window over reps.  The two routes' outputs are compared first (max |device - torch| / max |torch|).  Prints one JSON line.

--half: the same settings for the module after .half() (dm_dnet_linear_f16 / dm_dnet_diffuse_f16 / dm_dnet_gradfeat_f16).  Three routes
in the same process, windows taken alternately: the fp16 device route, the fp32 device route of the unhalved module, and the torch route
of the halved module under torch.autocast("cuda") -- what such a module runs without the device route, the baseline that decides
layers.AUTO_DEVICE["single_half" / "batch_half"].  Then one profiled call of the fp16 route: the share of its three kernels and the
TFLOP/s of its linears (2 rows C_out sum w per launch) next to the measured fp16 matrix-core peak.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def half_mode(a, net, xs, ref_ops, cases, result, eng):
    import copy
    half = copy.deepcopy(net).half()
    widths, n = [x.shape[1] for x in xs[0]], xs[0][0].shape[0]
    per_row = 2 * (sum(widths) * a.width + a.blocks * (3 * a.width * a.width + 2 * a.width * a.width) + a.width * a.width)      # linears, FLOP
    result["mode"] = "half"
    result["fp16_peak_tflops"] = round(eng.measure_peak("mfma_f16_random_operands") / 1e12, 1)

    def torch_half(idx):
        with torch.autocast("cuda"):
            return [half(xs[i], ref_ops[i][1], evals=ref_ops[i][3], evecs=ref_ops[i][4], gradX=ref_ops[i][5], gradY=ref_ops[i][6], route="torch") for i in idx]

    with torch.no_grad():
        for name, (idx, packed, reps) in cases.items():
            routes = {"device_half": lambda: half.forward_many([xs[i] for i in idx], packed),
                      "device_f32": lambda: net.forward_many([xs[i] for i in idx], packed),
                      "torch_half_autocast": lambda: torch_half(idx)}
            first = {k: fn() for k, fn in routes.items()}
            rel = lambda k: max(float((d.float() - t.float()).abs().max() / t.float().abs().max()) for d, t in zip(first[k], first["device_f32"]))
            for _ in range(2):
                for fn in routes.values():
                    fn()
            times = {k: [] for k in routes}
            for _ in range(5):
                for k, fn in routes.items():
                    times[k].append(window(fn, reps))
            entry = {k + "_ms": round(statistics.median(v), 3) for k, v in times.items()}
            entry.update({k + "_ms_all": [round(t, 3) for t in v] for k, v in times.items()})
            entry["max_rel_diff_to_device_f32"] = {k: rel(k) for k in ("device_half", "torch_half_autocast")}
            eng.profile_kernel("*")
            routes["device_half"]()
            torch.cuda.synchronize()
            report = eng.profile_report()
            eng.profile_kernel(None)
            total = sum(ms for _, ms in report.values())
            entry["kernels_ms"] = {k: round(ms, 3) for k, (_, ms) in report.items()}
            entry["kernels_share"] = {k: round(ms / total, 3) for k, (_, ms) in report.items()}
            lin_ms = report.get("dnet_linear_f16", (0, 0.0))[1]
            entry["linear_tflops"] = round(per_row * n * len(idx) / (lin_ms * 1e-3) / 1e12, 1) if lin_ms else None
            result[name] = entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=16)
    ap.add_argument("--grid", type=int, nargs=2, default=(64, 32))
    ap.add_argument("--k-eig", type=int, default=128)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dnet_forward_time: needs a ROCm GPU; a time taken elsewhere says nothing")
    from densematcher_amd import synth
    from densematcher_amd.diffusion_net import geometry as geo, layers
    from densematcher_amd.engine import default_engine
    dev = torch.device("cuda")
    eng = default_engine()
    meshes = [synth.torus_mesh(a.grid[0], a.grid[1], perturb=0.1, seed=100 + s) for s in range(a.meshes)]
    raw = eng.diffusion_operators([m[0] for m in meshes], [m[1] for m in meshes], a.k_eig)
    packed_all = layers.pack_operators(raw, device=dev)
    packed_one = layers.pack_operators(raw[:1], device=dev)
    ref_ops = [geo._from_device(op, dev, torch.float32) for op in raw]          # the reference's tensors: sparse COO gradX / gradY
    widths = (768, 51, 16)
    torch.manual_seed(0)
    net = layers.DiffusionNet(C_in=sum(widths), C_out=a.width, C_width=a.width, N_block=a.blocks).to(dev).eval()
    with torch.no_grad():
        for b in net.blocks:
            b.diffusion.diffusion_time.copy_(0.05 * torch.rand(a.width, device=dev))
    n = meshes[0][0].shape[0]
    xs = [tuple(torch.randn((n, w), device=dev) for w in widths) for _ in range(a.meshes)]

    def torch_route(idx):
        return [net(xs[i], ref_ops[i][1], evals=ref_ops[i][3], evecs=ref_ops[i][4], gradX=ref_ops[i][5], gradY=ref_ops[i][6], route="torch") for i in idx]

    cases = {"one_mesh": ([0], packed_one, 5), "batch": (list(range(a.meshes)), packed_all, 1)}
    result = {"tool": "tools/dnet_forward_time.py", "meshes": a.meshes, "vertices": n, "k_eig": a.k_eig, "width": a.width, "blocks": a.blocks,
              "C_in": list(widths), "gpu": torch.cuda.get_device_name(0)}
    if a.half:
        half_mode(a, net, xs, ref_ops, cases, result, eng)
    with torch.no_grad():
        for name, (idx, packed, reps) in ({} if a.half else cases).items():
            device_route = lambda: net.forward_many([xs[i] for i in idx], packed)
            yd, yt = device_route(), torch_route(idx)
            diff = max(float((d - t).abs().max() / t.abs().max()) for d, t in zip(yd, yt))
            for _ in range(2):
                device_route(), torch_route(idx)
            td, tt = [], []
            for _ in range(5):
                td.append(window(device_route, reps))
                tt.append(window(lambda: torch_route(idx), reps))
            result[name] = {"device_ms": round(statistics.median(td), 3), "torch_ms": round(statistics.median(tt), 3),
                            "device_ms_all": [round(v, 3) for v in td], "torch_ms_all": [round(v, 3) for v in tt],
                            "max_rel_diff": diff}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

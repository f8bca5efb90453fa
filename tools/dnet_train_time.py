#!/usr/bin/env python
"""
Time of one DiffusionNet training step (forward and backward, nothing else) at the shipped configuration on one GPU: the differentiable
device route (route="device", differentiable=True: the fp32 forward kernels recorded as torch.autograd.Functions whose backward is
dm_dnet_linear_bwd_data_f32 / dm_dnet_linear_bwd_weight_f32, dm_dnet_diffuse_bwd_f32, dm_dnet_gradfeat_bwd_f32) against the torch route
(the reference's expressions on PyTorch-ROCm with its autograd) -- the baseline -- both in fp32, in the same process.

    python tools/dnet_train_time.py [--meshes 16] [--out result.json]

Input and network as tools/dnet_forward_time.py: perturbed tori of 2048 vertices, k_eig = 128, width 512, 8 blocks, C_in = 768 + 51 + 16
as three sources, seeded weights, times uniform in [0, 0.05).  Every parameter requires grad, the inputs do not.  Eval mode: dropout is
the same torch kernel behind both routes and would only make the two routes' gradients incomparable.  A step is loss = sum_b (y_b * g_b)
.sum() and loss.backward() with the gradients set to None before it.  Per route and per case (one mesh; the batch) two warm-up steps,
then five timed windows taken alternately between the routes; a window is `reps` steps between two device synchronisations on the host
clock, and the figure is the median window over reps.  The two routes' gradients are compared first (per tensor max |device - torch| /
max |torch|, the largest).  Then one profiled device step: milliseconds and share per kernel name, and the TFLOP/s of the two linear
backward kernels (2 rows C_out sum w each per layer).  Prints one JSON line.

    python tools/dnet_train_time.py --mixed [--meshes 16] [--out result.json]

--mixed times three arms instead, windows taken alternately in the same way: the mixed-precision device route (compute_dtype=
torch.float16: float32 masters, the fp16 forward kernels, dm_dnet_*_bwd_f16), the fp32 differentiable device route, and the torch route
under torch.autocast("cuda", dtype=torch.float16).  It profiles one mixed step per kernel name and reports the largest workspace the
backward entries ask for at this configuration.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=16)
    ap.add_argument("--grid", type=int, nargs=2, default=(64, 32))
    ap.add_argument("--k-eig", type=int, default=128)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--mixed", action="store_true", help="time the mixed-precision route against the fp32 device route and torch autocast")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dnet_train_time: needs a ROCm GPU; a time taken elsewhere says nothing")
    from densematcher_amd import synth
    from densematcher_amd.diffusion_net import geometry as geo, layers
    from densematcher_amd.engine import default_engine
    dev = torch.device("cuda")
    eng = default_engine()
    meshes = [synth.torus_mesh(a.grid[0], a.grid[1], perturb=0.1, seed=100 + s) for s in range(a.meshes)]
    raw = eng.diffusion_operators([m[0] for m in meshes], [m[1] for m in meshes], a.k_eig)
    packed_all = layers.pack_operators(raw, device=dev)
    packed_one = layers.pack_operators(raw[:1], device=dev)
    for p in (packed_all, packed_one):
        p.transposed_rows()                                                    # built once per pack, not part of a step
    ref_ops = [geo._from_device(op, dev, torch.float32) for op in raw]          # the reference's tensors: sparse COO gradX / gradY
    widths = (768, 51, 16)
    torch.manual_seed(0)
    net = layers.DiffusionNet(C_in=sum(widths), C_out=a.width, C_width=a.width, N_block=a.blocks).to(dev).eval()
    with torch.no_grad():
        for b in net.blocks:
            b.diffusion.diffusion_time.copy_(0.05 * torch.rand(a.width, device=dev))
    n = meshes[0][0].shape[0]
    xs = [tuple(torch.randn((n, w), device=dev) for w in widths) for _ in range(a.meshes)]
    gs = [torch.randn((n, a.width), device=dev) for _ in range(a.meshes)]

    def step(outputs, idx):
        net.zero_grad(set_to_none=True)
        sum((y * gs[i]).sum() for y, i in zip(outputs(), idx)).backward()

    def torch_outputs(idx):
        return [net(xs[i], ref_ops[i][1], evals=ref_ops[i][3], evecs=ref_ops[i][4], gradX=ref_ops[i][5], gradY=ref_ops[i][6], route="torch") for i in idx]

    grads = lambda: {name: p.grad.clone() for name, p in net.named_parameters()}
    cases = {"one_mesh": ([0], packed_one, 3), "batch": (list(range(a.meshes)), packed_all, 1)}
    result = {"tool": "tools/dnet_train_time.py", "meshes": a.meshes, "vertices": n, "k_eig": a.k_eig, "width": a.width, "blocks": a.blocks,
              "C_in": list(widths), "gpu": torch.cuda.get_device_name(0)}
    per_row = 2 * (sum(widths) * a.width + a.blocks * (3 * a.width * a.width + 2 * a.width * a.width) + a.width * a.width)      # linears, FLOP
    for name, (idx, packed, reps) in cases.items() if a.mixed else ():
        many = lambda **kw: step(lambda: net.forward_many([xs[i] for i in idx], packed, differentiable=True, **kw), idx)
        mixed_step, fp32_step = (lambda: many(compute_dtype=torch.float16)), (lambda: many())

        def autocast_step():
            with torch.autocast("cuda", dtype=torch.float16):
                outs = torch_outputs(idx)
            step(lambda: [y.float() for y in outs], idx)
        arms = {"mixed": mixed_step, "device_fp32": fp32_step, "torch_autocast": autocast_step}
        fp32_step()
        g32 = grads()
        mixed_step()
        gm = grads()
        diff = {k: float((gm[k] - g32[k]).abs().max() / g32[k].abs().max()) for k in g32}
        worst = max(diff, key=diff.get)
        for _ in range(2):
            for fn in arms.values():
                fn()
        times = {k: [] for k in arms}
        for _ in range(5):
            for k, fn in arms.items():
                times[k].append(window(fn, reps))
        entry = {k + "_ms": round(statistics.median(v), 3) for k, v in times.items()}
        entry.update({k + "_ms_all": [round(t, 3) for t in v] for k, v in times.items()})
        entry.update({"max_rel_grad_diff_mixed_vs_fp32": diff[worst], "max_rel_grad_diff_at": worst})
        eng.profile_kernel("*")
        mixed_step()
        torch.cuda.synchronize()
        report = eng.profile_report()
        eng.profile_kernel(None)
        total = sum(ms for _, ms in report.values())
        entry["kernels_ms"] = {k: round(ms, 3) for k, (_, ms) in report.items()}
        entry["kernels_share"] = {k: round(ms / total, 3) for k, (_, ms) in report.items()}
        entry["kernels_launches"] = {k: int(c) for k, (c, _) in report.items()}
        Bn, w = len(idx), a.width
        entry["workspace_bytes"] = {"linear": int(eng.lib.dm_dnet_linear_bwd_f16_bytes(Bn, w, max(sum(widths), 3 * w))),
                                    "diffuse": int(eng.lib.dm_dnet_diffuse_bwd_f16_bytes(Bn, a.k_eig, w)),
                                    "gradfeat": int(eng.lib.dm_dnet_gradfeat_bwd_f16_bytes(Bn, n, w))}
        result[name] = entry
    for name, (idx, packed, reps) in () if a.mixed else cases.items():
        device_step = lambda: step(lambda: net.forward_many([xs[i] for i in idx], packed, differentiable=True), idx)
        torch_step = lambda: step(lambda: torch_outputs(idx), idx)
        device_step()
        gd = grads()
        torch_step()
        gt = grads()
        diff = {k: float((gd[k] - gt[k]).abs().max() / gt[k].abs().max()) for k in gt}
        worst = max(diff, key=diff.get)
        for _ in range(2):
            device_step(), torch_step()
        td, tt = [], []
        for _ in range(5):
            td.append(window(device_step, reps))
            tt.append(window(torch_step, reps))
        entry = {"device_ms": round(statistics.median(td), 3), "torch_ms": round(statistics.median(tt), 3),
                 "device_ms_all": [round(v, 3) for v in td], "torch_ms_all": [round(v, 3) for v in tt],
                 "max_rel_grad_diff": diff[worst], "max_rel_grad_diff_at": worst}
        eng.profile_kernel("*")
        device_step()
        torch.cuda.synchronize()
        report = eng.profile_report()
        eng.profile_kernel(None)
        total = sum(ms for _, ms in report.values())
        entry["kernels_ms"] = {k: round(ms, 3) for k, (_, ms) in report.items()}
        entry["kernels_share"] = {k: round(ms / total, 3) for k, (_, ms) in report.items()}
        entry["kernels_launches"] = {k: int(c) for k, (c, _) in report.items()}
        for k in ("dnet_linear", "dnet_linear_bwd_data", "dnet_linear_bwd_weight"):
            ms = report.get(k, (0, 0.0))[1]
            # (first_lin's input needs no gradient: its share of the data kernel's work is not run)
            flop = per_row - (2 * sum(widths) * a.width if k == "dnet_linear_bwd_data" else 0)
            entry[k + "_tflops"] = round(flop * n * len(idx) / (ms * 1e-3) / 1e12, 1) if ms else None
        result[name] = entry
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""
Time of the aggregation network behind the 2D backbones (featurizers.SDDINO.aggregate_features, rot_inv) at the workload's size on one
GPU: the device route (MatchEngine.agg_gather + MatchEngine.aggregate: dm_agg_gather_f32, dm_dnet_linear_f32, dm_groupnorm_stats_f32,
dm_groupnorm_relu_f32, dm_conv3x3_f32, dm_agg_mix_f32) against the torch route of the same process (the reference's expressions:
F.interpolate, cat, grid_sample per rotation, MIOpen convolutions, nn.GroupNorm) -- the baseline: the parent commit has no such stage.

    python tools/aggre_time.py [--views 5] [--out result.json]

Input: 5 views, 4 rotations, P = 24, feature_dims 640 / 1280 / 1280 / 768, projection_dim 768, seeded weights moved off their initial
values, fp16 sources of 24 x 24 (s3), 12 x 12 (s4), 6 x 6 (s5) and 24 x 24 (dino, as the permuted view of a token tensor).  The source
sizes are an ASSUMPTION of this tool -- the UNet's decoder halves the grid per level in SD-1.5 -- that nothing here can confirm: the SD
model is not part of this package.  The routes' outputs are compared first.  Two warm-up calls per route, then five timed windows taken
alternately between the routes; a window is `reps` calls between two device synchronisations on the host clock, the figure is the median
window over reps.  "kernels": launches and milliseconds per kernel name over one device call (dm_profile_kernel("*"): HIP events around
every launch, which serialises them -- the sum is an upper bound of the call).  Prints one JSON line.

featurizers.modules.projection_network.AUTO_DEVICE is True where device_ms < torch_ms here.
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
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--rotations", type=int, default=4)
    ap.add_argument("--patches", type=int, default=24)
    ap.add_argument("--projection", type=int, default=768)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aggre_time: needs a ROCm GPU; a time taken elsewhere says nothing")
    from densematcher_amd.engine import default_engine
    from densematcher_amd.featurizers import AggregationNetwork, aggregate_features
    dev = torch.device("cuda")
    eng = default_engine()
    torch.manual_seed(0)
    dims = [640, 1280, 1280, 768]
    net = AggregationNetwork(feature_dims=dims, projection_dim=a.projection).eval()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    net = net.to(dev)
    P, R, n = a.patches, a.rotations, a.views * a.rotations
    s3 = torch.randn((n, dims[0], P, P), device=dev).half()
    s4 = torch.randn((n, dims[1], P // 2, P // 2), device=dev).half()
    s5 = torch.randn((n, dims[2], P // 4, P // 4), device=dev).half()
    dino = torch.randn((n, P, P, dims[3]), device=dev).half().permute(0, 3, 1, 2)
    result = {"tool": "tools/aggre_time.py", "views": a.views, "rotations": R, "patches": P, "feature_dims": dims, "projection_dim": a.projection,
              "dtype": "float16", "gpu": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        run = lambda route: aggregate_features(net, s3, s4, s5, dino, num_rotations=R, rot_inv=True, route=route)
        device_route, torch_route = (lambda: run("device")), (lambda: run("torch"))
        yd, yt = device_route(), torch_route()
        result["max_rel_diff"] = float((yd - yt).abs().max() / yt.abs().max())
        del yd, yt
        for _ in range(2):
            device_route(), torch_route()
        td, tt = [], []
        for _ in range(5):
            td.append(window(device_route, a.reps))
            tt.append(window(torch_route, a.reps))
        result.update({"device_ms": round(statistics.median(td), 3), "torch_ms": round(statistics.median(tt), 3),
                       "device_ms_all": [round(v, 3) for v in td], "torch_ms_all": [round(v, 3) for v in tt]})
        result["auto_device"] = result["device_ms"] < result["torch_ms"]
        # ---- the device route's parts
        gather = lambda: eng.agg_gather([s3, s4, s5, dino], num_rotations=R, step_deg=360.0 / R, size=(P, P))
        rows, packed = gather(), net.packed(eng.device)
        for _ in range(2):
            gather(), eng.aggregate(packed, rows, P, P)
        result["gather_ms"] = round(statistics.median([window(gather, a.reps) for _ in range(5)]), 3)
        result["network_ms"] = round(statistics.median([window(lambda: eng.aggregate(packed, rows, P, P), a.reps) for _ in range(5)]), 3)
        eng.profile_kernel("*")
        device_route()
        torch.cuda.synchronize()
        result["kernels"] = {k: [v[0], round(v[1], 3)] for k, v in eng.profile_report().items()}
        eng.profile_kernel(None)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

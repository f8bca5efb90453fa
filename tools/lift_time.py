#!/usr/bin/env python
"""
Time of multi-view feature lifting at the workload's size on one GPU: the device route (MatchEngine.lift_features: dm_raster_pix2face +
dm_lift_features, the whole batch in two device calls) against the torch route (projection._torch_lift: the same stage on
PyTorch-ROCm, one mesh and one view at a time) -- the baseline -- in the same process.

    python tools/lift_time.py [--meshes 4] [--out result.json]

Input: 4 perturbed tori of 2048 vertices (synth.torus_mesh(64, 32, perturb=0.1, seed=s)), centred, 5 views each at distance 2 x the
largest coordinate, maps 5 x 768 x 384 x 384 fp16 per mesh, once as NCHW and once as channels-last tensors.  Both routes are given the
same pix2face (the device raster's), so that they time the same work: visible sets, projection, sampling, the mean.  The device route is
timed a second time with its own raster pass in it ("device_total_ms"), and the raster pass alone ("raster_ms").  Per figure two warm-up
calls, then five timed windows taken alternately between the routes; a window is `reps` calls between two device synchronisations on the
host clock, the figure is the median window over reps.  The routes' outputs are compared first.  Prints one JSON line.

projection.AUTO_DEVICE takes the device route for a layout where device_total_ms <= torch_ms.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
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


def orbit(dist, elev_deg, azim_deg):
    e, a = np.deg2rad(elev_deg), np.deg2rad(azim_deg)
    eye = dist * np.array([np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)])
    z = -eye / np.linalg.norm(eye)
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    R = np.stack((x, np.cross(z, x), z), axis=1)
    return R, -eye @ R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=4)
    ap.add_argument("--grid", type=int, nargs=2, default=(64, 32))
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--channels", type=int, default=768)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lift_time: needs a ROCm GPU; a time taken elsewhere says nothing")
    from densematcher_amd import projection as pj, synth
    from densematcher_amd.engine import default_engine
    dev = torch.device("cuda")
    eng = default_engine()
    V, F, cams = [], [], []
    for s in range(a.meshes):
        v, f = synth.torus_mesh(a.grid[0], a.grid[1], perturb=0.1, seed=100 + s)
        v = v - 0.5 * (v.max(0) + v.min(0))
        dist = 2.0 * np.abs(v).max()
        rt = [orbit(dist, 20.0 * (i % 2), 360.0 * i / a.views + 7.0 * s) for i in range(a.views)]
        V.append(v), F.append(f), cams.append((np.stack([r for r, _ in rt]), np.stack([t for _, t in rt])))
    H = a.size
    torch.manual_seed(0)
    nchw = [torch.randn((a.views, a.channels, H, H), device=dev, dtype=torch.float16) for _ in range(a.meshes)]
    p2f, _ = eng.raster_visibility(V, F, cams, H, H)
    tv = [torch.from_numpy(v.astype(np.float32)).to(dev) for v in V]
    tf = [torch.from_numpy(f).to(dev) for f in F]
    tc = [(torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev)) for r, t in cams]
    result = {"tool": "tools/lift_time.py", "meshes": a.meshes, "vertices": int(V[0].shape[0]), "views": a.views, "channels": a.channels,
              "size": H, "dtype": "float16", "gpu": torch.cuda.get_device_name(0)}
    raster = lambda: eng.raster_visibility(V, F, cams, H, H)
    for _ in range(2):
        raster()
    result["raster_ms"] = round(statistics.median([window(raster, a.reps) for _ in range(5)]), 3)
    for layout in ("nchw", "channels_last"):
        maps = nchw if layout == "nchw" else [m.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for m in nchw]
        device_given = lambda: eng.lift_features(maps, V, F, cams, pix2face_list=p2f)
        device_total = lambda: eng.lift_features(maps, V, F, cams)
        torch_route = lambda: [pj._torch_lift(maps[b], tv[b], tf[b], tc[b][0], tc[b][1], p2f[b], 1.0, dev)[0] for b in range(a.meshes)]
        yd, yt = device_given(), torch_route()
        diff = max(float((d - t).abs().max() / t.abs().max()) for d, t in zip(yd, yt))
        for _ in range(2):
            device_given(), device_total(), torch_route()
        td, tg, tt = [], [], []
        for _ in range(5):
            tg.append(window(device_given, a.reps))
            td.append(window(device_total, a.reps))
            tt.append(window(torch_route, a.reps))
        med = lambda v: round(statistics.median(v), 3)
        result[layout] = {"device_given_ms": med(tg), "device_total_ms": med(td), "torch_ms": med(tt), "device_given_ms_all": [round(v, 3) for v in tg],
                          "device_total_ms_all": [round(v, 3) for v in td], "torch_ms_all": [round(v, 3) for v in tt], "max_rel_diff": diff,
                          "auto_device": med(td) <= med(tt)}
        if layout != "nchw":
            del maps
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

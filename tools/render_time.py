#!/usr/bin/env python
"""
Time of textured-mesh rendering at the notebook's size on one GPU: the device route (MatchEngine.render_phong: dm_render_phong, every
mesh and view in one device call) against the host route of the same process (render.py: NumPy float64 raster, torch shading on the
CPU) -- the only other implementation there is: the reference renders with pytorch3d, which has no ROCm build.

    python tools/render_time.py [--meshes 4] [--out result.json]

Input: raw meshes of about 100 k faces (synth.torus_mesh(320, 160, perturb=0.1, seed=s): 51 200 vertices, 102 400 faces), a 1024 x 1024
UV map each, the five views of num_views = (3, 1) generated as run_rendering does without cameras, 512 x 512 images.  Two workloads: one
mesh, and --meshes meshes in one call.  Per figure two warm-up calls, then five timed calls taken alternately between the routes; a
call ends in a device synchronisation and is timed on the host clock; the figure is the median.  The routes' images are compared
first.  --host-warmup / --host-calls shorten the host route's share (it takes tens of seconds per mesh); what was used is in the result.
Prints one JSON line.

render.AUTO_DEVICE is set where device_ms <= host_ms.
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=4)
    ap.add_argument("--grid", type=int, nargs=2, default=(320, 160))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--map", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-warmup", type=int, default=2)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--host-meshes", type=int, default=None, help="time the host route of the batch on this many meshes only and scale (it is a loop over meshes)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_time: needs a ROCm GPU; a time taken elsewhere says nothing")
    from densematcher_amd import render as rd, synth
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    meshes = []
    for s in range(a.meshes):
        v, f = synth.torus_mesh(a.grid[0], a.grid[1], perturb=0.1, seed=100 + s)
        v = v - 0.5 * (v.max(0) + v.min(0))
        i, j = np.divmod(np.arange(len(v)), a.grid[1])
        uv = np.stack((i / a.grid[0], j / a.grid[1]), axis=1).astype(np.float32)
        tmap = torch.from_numpy(rng.uniform(0, 1, (a.map, a.map, 3)).astype(np.float32)).to(dev)
        meshes.append(rd.Meshes(torch.from_numpy(v), torch.from_numpy(f), rd.TexturesUV([tmap], [torch.from_numpy(f)], [torch.from_numpy(uv)])))
    H = a.size
    result = {"tool": "tools/render_time.py", "faces": int(meshes[0].faces_list()[0].shape[0]), "vertices": int(meshes[0].verts_list()[0].shape[0]),
              "views": 5, "size": H, "map": a.map, "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "calls": a.calls,
              "host_warmup": a.host_warmup, "host_calls": a.host_calls}
    med = lambda v: round(statistics.median(v), 3) if v else None
    for name, batch in (("one_mesh", meshes[:1]), (f"{a.meshes}_meshes", meshes)):
        host_batch = batch if a.host_meshes is None else batch[:a.host_meshes]
        scale = len(batch) / len(host_batch)
        device = lambda: rd.render_many(dev, batch, (3, 1), H, H, route="device")
        host = lambda: rd.render_many(dev, host_batch, (3, 1), H, H, route="host")
        yd, yh = device(), host()
        diff = max(float((d[0] - h[0]).abs().max()) for d, h in zip(yd, yh))
        differ = sum(int((d[3] != h[3]).sum()) for d, h in zip(yd, yh))
        for k in range(max(a.warmup, a.host_warmup) - 1):              # (the comparison above was the first warm-up call of both)
            if k < a.warmup - 1:
                device()
            if k < a.host_warmup - 1:
                host()
        td, th = [], []
        for k in range(max(a.calls, a.host_calls)):
            if k < a.calls:
                td.append(timed(device))
            if k < a.host_calls:
                th.append(timed(host) * scale)
        result[name] = {"device_ms": med(td), "host_ms": med(th), "device_ms_all": [round(v, 3) for v in td], "host_ms_all": [round(v, 3) for v in th],
                        "host_meshes_timed": len(host_batch), "max_abs_diff": diff, "pix2face_differ": differ, "auto_device": None if not (td and th) else med(td) <= med(th)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

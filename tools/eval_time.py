#!/usr/bin/env python
"""
Timing of the map quality measures, device route against host route on the same box (one process, the arms alternating, every arm
after a warm-up, a host clock around work that ends with the results on the host: median and min - max are reported).

    python tools/eval_time.py [--meshes 16] [--pairs 64] [--maps 8] [--repeats 5] [--out profiles/eval_time.txt]

Input: --meshes tori of 2 048 vertices (4 096 faces, seeded perturbations), --pairs (source, target) pairs among them, --maps seeded
vertex maps per pair, one ground truth per pair.  Both arms start from the meshes (their Laplacians assembled) and end with accuracy,
continuity and coverage of every map:
    device   pyFM.eval.evaluate_pairs(robust=False): the heat-method matrices of the batch on the device, three dm_map_metrics
             launches on them, 3 x pairs x maps numbers cross to the host
    host     TriMesh.get_geodesic_many(robust=False) -- the same matrices, copied to the host -- then pyFM.eval.accuracy /
             continuity / coverage per map (what a sweep ran before the device route existed)
and, with the matrices already where each route wants them, the evaluation alone ("measures only").
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from densematcher_amd import synth  # noqa: E402
from densematcher_amd.pyFM import TriMesh  # noqa: E402
from densematcher_amd.pyFM import eval as ev  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ts):
    return f"{statistics.median(ts):10.3f} ms  ({min(ts):.3f} - {max(ts):.3f}, n = {len(ts)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_time: no GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    meshes = [TriMesh(*synth.torus_mesh(64, 32, perturb=0.1, seed=s)) for s in range(args.meshes)]
    n = meshes[0].n_vertices
    pairs = [(int(rng.integers(0, args.meshes)), int(rng.integers(0, args.meshes))) for _ in range(args.pairs)]
    maps = [{f"map{m}": rng.integers(0, n, n) for m in range(args.maps)} for _ in pairs]
    gts = [rng.integers(0, n, n) for _ in pairs]
    say(f"# {torch.cuda.get_device_name(0)}; {args.meshes} meshes of {n} vertices, {args.pairs} pairs, {args.maps} maps each; repeats {args.repeats}")

    def device():
        return ev.evaluate_pairs(meshes, pairs, maps, gts, robust=False)

    def host_measures(D):
        out = []
        for (i, j), named, gt in zip(pairs, maps, gts):
            area, edges = meshes[i].vertex_areas, meshes[j].edges
            out.append({name: {"accuracy": ev.accuracy(m, gt, D[i]), "continuity": ev.continuity(m, D[i], D[j], edges),
                               "coverage": ev.coverage(m, area)} for name, m in named.items()})
        return out

    def host():
        return host_measures(TriMesh.get_geodesic_many(meshes, robust=False))

    got, ref = device(), host()                                  # warm-up of both arms, and the comparison
    worst = 0.0
    for a, b in zip(got, ref):
        for name in a:
            for key in ("accuracy", "continuity", "coverage"):
                x, y = float(a[name][key]), float(b[name][key])
                if np.isfinite(y):
                    worst = max(worst, abs(x - y) / abs(y))
                else:
                    assert (np.isnan(x) and np.isnan(y)) or x == y, (name, key, x, y)
    say(f"largest relative difference device / host over {3 * args.pairs * args.maps} numbers: {worst:.3e}")

    D_host = TriMesh.get_geodesic_many(meshes, robust=False)
    D_dev = TriMesh._heat_geodesic_many_device(meshes, False)
    nv = [m.n_vertices for m in meshes]
    src = [i for (i, j), named in zip(pairs, maps) for _ in named]
    tgt = [j for (i, j), named in zip(pairs, maps) for _ in named]
    flat = [m for named in maps for m in named.values()]
    flat_gt = [gt for gt, named in zip(gts, maps) for _ in named]
    edges = [m.edges for m in meshes]
    areas = torch.as_tensor(np.stack([m.vertex_areas for m in meshes])).to(D_dev.device)

    def device_measures():
        return (ev.accuracy_many(flat, flat_gt, D_dev, mesh=src, n_verts=nv),
                ev.continuity_many(flat, D_dev, None, [edges[t] for t in tgt], mesh1=src, mesh2=tgt, n_verts1=nv),
                ev.coverage_many(flat, areas, mesh=src, n_verts=nv))

    device_measures()
    host_measures(D_host)
    td, th, tdm, thm = [], [], [], []
    for _ in range(args.repeats):                                # (the arms alternate)
        td.append(timed(device)[0])
        th.append(timed(host)[0])
        tdm.append(timed(device_measures)[0])
        thm.append(timed(lambda: host_measures(D_host))[0])
    say(f"device  evaluate_pairs(robust=False)                      {fmt(td)}")
    say(f"host    get_geodesic_many(robust=False) + host functions  {fmt(th)}")
    say(f"device  measures only (matrices on the device)            {fmt(tdm)}")
    say(f"host    measures only (matrices on the host)              {fmt(thm)}")
    say(f"host / device = {statistics.median(th) / statistics.median(td):.1f} (end to end), "
        f"{statistics.median(thm) / statistics.median(tdm):.1f} (measures only)")
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

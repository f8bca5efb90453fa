#!/usr/bin/env python
"""
Shortest paths along mesh edges, device route against the host route it replaces, timed per call through the mesh layer:
TriMesh.extract_fps_many (the default sampler: dm_fps_graph against one SciPy Dijkstra per sample) and TriMesh.get_geodesic_many(
dijkstra=True) (dm_graph_geodesic against all-pairs csgraph.dijkstra) on perturbed tori, the two routes INTERLEAVED in one process
("graph_geod_device" 1 / 0), bracketed with HIP events after one untimed call of the same shape, profiler off.  The bracket holds the
whole call: building the graphs, uploads, the kernel, the copy back.  One JSON line per case: ms per call and per mesh (median of
--reps; the host route of the long cases runs --host-reps times), and whether the two routes returned equal arrays.

    python tools/graph_geodesic_timing.py                 # the table of DESIGN.md section 4
    python tools/graph_geodesic_timing.py --cases fps     # fps | allpairs | zoomout | sweeps
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densematcher_amd import synth  # noqa: E402
from densematcher_amd.engine import default_engine  # noqa: E402
from densematcher_amd.pyFM.mesh.trimesh import TriMesh  # noqa: E402

GRIDS = {512: (32, 16), 2048: (64, 32), 8192: (128, 64), 16384: (128, 128)}


def meshes_of(N, B):
    nu, nv = GRIDS[N]
    base = [TriMesh(*synth.torus_mesh(nu, nv, perturb=0.05, seed=s)) for s in range(min(B, 4))]
    return [base[b % len(base)] for b in range(B)]


def timed(fn, reps):
    out = fn()                                                            # warm-up, untimed
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def both_routes(eng, fn, reps, host_reps):
    res = {}
    try:
        for mode, r in ((1, reps), (0, host_reps), (1, reps)):           # device, host, device again: drift shows as a gap
            eng.set_option("graph_geod_device", mode)
            ms, out = timed(fn, r)
            res.setdefault(mode, []).append(ms)
            res["out%d" % mode] = out
    finally:
        eng.set_option("graph_geod_device", 1)
    same = all(np.array_equal(a, b) for a, b in zip(res["out0"], res["out1"]))
    return res[1], res[0][0], same


def case_fps(eng, N, B, size, reps, host_reps):
    ms = meshes_of(N, B)
    starts = [(7 * b) % N for b in range(B)]
    dev, host, same = both_routes(eng, lambda: TriMesh.extract_fps_many(ms, size, starts=starts), reps, host_reps)
    return {"case": "extract_fps_many", "N": N, "B": B, "samples": size, "device_ms": [round(x, 3) for x in dev],
            "device_ms_per_mesh": round(min(dev) / B, 3), "host_ms": round(host, 1), "host_ms_per_mesh": round(host / B, 1), "equal": same}


def case_allpairs(eng, N, B, reps, host_reps):
    ms = meshes_of(N, B)
    dev, host, same = both_routes(eng, lambda: TriMesh.get_geodesic_many(ms, dijkstra=True), reps, host_reps)
    return {"case": "get_geodesic_many(dijkstra=True)", "N": N, "B": B, "device_ms": [round(x, 2) for x in dev],
            "device_ms_per_mesh": round(min(dev) / B, 2), "host_ms": round(host, 1), "host_ms_per_mesh": round(host / B, 1), "equal": same}


def case_zoomout(eng, reps, host_reps):
    """mesh_zoomout_refine(subsample=512) end to end, 50 -> 200 at N = 2048: the sampling of both meshes + the device loop"""
    from densematcher_amd.pyFM import refine
    m1, m2 = (TriMesh(*synth.torus_mesh(64, 32, perturb=p, seed=s)) for p, s in ((0.0, 0), (0.05, 1)))
    TriMesh.process_many([m1, m2], [200, 200])
    C0 = np.eye(50)

    def run():
        return [refine.mesh_zoomout_refine(C0, m1, m2, nit=150, step=1, subsample=512)]
    res = {}
    try:
        for mode, r in ((1, reps), (0, host_reps), (1, reps)):
            eng.set_option("graph_geod_device", mode)
            res.setdefault(mode, []).append(timed(run, r)[0])
    finally:
        eng.set_option("graph_geod_device", 1)
    return {"case": "mesh_zoomout_refine(subsample=512), 50 -> 200", "N": 2048, "device_ms": [round(x, 2) for x in res[1]],
            "host_ms": round(res[0][0], 1)}


def case_sweeps(N, size):
    """sweeps per sample of the warm-started sampling, synchronous pull sweeps in NumPy (the kernel relaxes in place: it needs no
    more); the last sweep of every sample is the one that changes nothing"""
    import scipy.sparse as sparse
    m = meshes_of(N, 1)[0]
    G = sparse.csc_matrix(m._fps_edge_graph())
    n = G.shape[0]
    rl = np.diff(G.indptr)
    cols = np.full((int(rl.max()), n), -1, np.int64)
    w = np.zeros(cols.shape)
    pos = np.arange(G.nnz) - np.repeat(G.indptr[:-1], rl)
    v = np.repeat(np.arange(n), rl)
    cols[pos, v], w[pos, v] = G.indices, G.data
    d = np.full(n, np.inf)
    cur, sweeps = 0, []
    for _ in range(size):
        d[cur] = 0.0
        k = 0
        while True:
            new = np.minimum(d, np.where(cols >= 0, d[np.maximum(cols, 0)] + w, np.inf).min(axis=0))
            k += 1
            if np.array_equal(new, d):
                break
            d = new
        sweeps.append(k)
        cur = int(np.argmax(d))
    s = np.asarray(sweeps)
    return {"case": "sweeps per sample (synchronous restatement)", "N": N, "samples": size, "first_8": s[:8].tolist(),
            "samples_64_to_72": s[64:72].tolist(), "last_8": s[-8:].tolist(), "total": int(s.sum()), "mean": round(float(s.mean()), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["fps", "allpairs", "zoomout", "sweeps"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--big", type=int, default=1, help="0: skip the N = 8192 cases (their host route takes tens of seconds)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_geodesic_timing: no GPU")
    eng = default_engine()
    warnings.simplefilter("ignore")
    if "fps" in a.cases:
        for N, B in ((2048, 1), (2048, 64)) + (((8192, 1),) if a.big else ()):
            print(json.dumps(case_fps(eng, N, B, 512, a.reps, a.host_reps)), flush=True)
    if "allpairs" in a.cases:
        for N, B in ((2048, 1), (2048, 16)) + (((8192, 1),) if a.big else ()):
            print(json.dumps(case_allpairs(eng, N, B, min(a.reps, 3), a.host_reps)), flush=True)
            torch.cuda.empty_cache()
    if "zoomout" in a.cases:
        print(json.dumps(case_zoomout(eng, min(a.reps, 3), a.host_reps)), flush=True)
    if "sweeps" in a.cases:
        print(json.dumps(case_sweeps(2048, 512)), flush=True)


if __name__ == "__main__":
    main()

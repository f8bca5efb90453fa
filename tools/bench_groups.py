#!/usr/bin/env python
"""
Time the semantic group distances (MatchEngine.groups_dmtx -> dm_lsa_gather) against the reference's SciPy loop (the host route of
densematcher_amd.utils.get_groups_dmtx, what the package offered before) on one machine, in one process:

    python tools/bench_groups.py [--repeats 7] [--out FILE.json]

  * the 2048-vertex torus of tests/golden/fx_geod.npz, shortest-path distances along its edges, G in {8, 16, 32} Voronoi groups
    (tests/groups_restate.py: farthest-point seeds, argmin labels): groups_dmtx at B = 1 and B = 16 (the same mesh sixteen times)
    on a matrix that is already on the device, and the host loop on the same matrix in host memory;
  * end to end for 16 meshes with G = 16: TriMesh.get_groups_dmtx_many(robust=False) against get_geodesic_many(robust=False) followed by
    the host loop per mesh.
Every figure is the median of `repeats` runs after a warm-up run, a host clock around work that ends in a device synchronise (the
means are read back).  The host loop is run `host_repeats` times (it takes a third of a second or more per mesh).
Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import groups_restate as gr  # noqa: E402


def median_ms(fn, repeats, sync):
    fn()
    sync()
    ts = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import scipy.sparse.csgraph as csgraph
    from densematcher_amd import utils
    from densematcher_amd.engine import default_engine
    from densematcher_amd.pyFM.mesh import geometry
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    eng = default_engine()
    sync = eng.synchronize
    fx = dict(np.load(os.path.join(REPO, "tests", "golden", "fx_geod.npz")))
    V, F = fx["torus_V"], fx["torus_F"]
    D = csgraph.dijkstra(geometry.edge_graph(V, F))
    D1 = torch.as_tensor(D[None]).to(eng.device)
    D16 = D1.expand(16, -1, -1).contiguous()
    rows = []
    for G in (8, 16, 32):
        groups = gr.voronoi_groups(D, G)
        sizes = sorted(len(g) for g in groups)
        dev1 = median_ms(lambda: eng.groups_dmtx(D1, [groups]), a.repeats, sync)
        dev16 = median_ms(lambda: eng.groups_dmtx(D16, [groups] * 16), a.repeats, sync)
        host = median_ms(lambda: utils.get_groups_dmtx(D, groups, device=False), a.host_repeats, lambda: None)
        got, ref = eng.groups_dmtx(D1, [groups])[0], utils.get_groups_dmtx(D, groups, device=False)
        ok = bool(np.all(np.abs(got - ref) <= gr.mean_bound(groups, ref)))
        rows.append({"G": G, "problems": G * (G - 1) // 2, "group_sizes_min_med_max": [sizes[0], sizes[len(sizes) // 2], sizes[-1]],
                     "device_B1_ms": dev1, "device_B16_ms": dev16, "host_ms": host, "agrees_with_host": ok})
        print(json.dumps(rows[-1]), flush=True)
    # end to end, 16 meshes (the torus with sixteen different vertex perturbations would give the same sizes: the same mesh is used)
    meshes = [TriMesh(V, F) for _ in range(16)]
    Dh = TriMesh.get_geodesic_many(meshes[:1], robust=False)[0]
    groups = gr.voronoi_groups(np.maximum(Dh, Dh.T), 16)
    e2e_dev = median_ms(lambda: TriMesh.get_groups_dmtx_many(meshes, [groups] * 16, robust=False), max(3, a.repeats // 2), sync)

    def host_chain():
        mats = TriMesh.get_geodesic_many(meshes, robust=False)
        return [utils.get_groups_dmtx(Dm, groups, device=False) for Dm in mats]
    e2e_host = median_ms(host_chain, 1, sync)
    geod_only = median_ms(lambda: TriMesh.get_geodesic_many(meshes, robust=False), 3, sync)
    res = {"single_mesh": rows, "end_to_end_16_meshes_G16": {"device_ms": e2e_dev, "geodesic_many_plus_host_loop_ms": e2e_host,
                                                              "geodesic_many_alone_ms": geod_only},
           "device_below_host_at_every_G": all(r["device_B1_ms"][0] < r["host_ms"][0] for r in rows),
           "columns": "median, min, max in ms"}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""
Time per iteration of Consistent ZoomOut (densematcher_amd.pyFM.FMN.zoomout_iteration), device route against host route on the same
machine: 16 synthetic tori of 2 048 vertices, all 240 directed edges, 512 farthest point samples per mesh, M = 20 and M = 50 (one
iteration M -> M + 2 with a canonical basis of int(0.9 M)), weight_type 'adjacency' and 'icsm'.

    python tools/fmn_time.py [--meshes 16] [--reps 3] [--no-host]

Every timed iteration starts from the same initial maps (nearest-vertex maps with 10 % of the entries replaced at random); the device
time is the wall time between two stream synchronisations after one untimed iteration of the same shape, the median of --reps.  For each
case the script also prints MatchEngine.profile_report() of one device iteration (kernel name: launches, total ms).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Mesh:
    def __init__(self, verts, faces, lam, Phi, mass):
        self.vertlist, self.facelist = verts, faces
        self.eigenvalues, self.eigenvectors = lam, Phi
        self.A = sparse.diags(mass).tocsr()
        self.n_vertices = verts.shape[0]


def fps_euclid(V, size, start=0):
    inds = [start]
    d = np.linalg.norm(V - V[start], axis=1)
    for _ in range(size - 1):
        inds.append(int(np.argmax(d)))
        d = np.minimum(d, np.linalg.norm(V - V[inds[-1]], axis=1))
    return np.asarray(inds)


def build(n_meshes, K):
    from densematcher_amd import synth
    meshes = []
    for q in range(n_meshes):
        V, F = synth.torus_mesh(64, 32, perturb=0.0 if q == 0 else 0.1, seed=q)
        lam, Phi, mass = synth.eigenbasis(V, F, K, method="arpack")
        meshes.append(Mesh(V, F, lam, Phi, mass))
    samples = np.stack([fps_euclid(m.vertlist, 512) for m in meshes])
    return meshes, samples


def initial_maps(meshes, M, seed=0):
    rng = np.random.default_rng(seed)
    maps = {}
    for i, mi in enumerate(meshes):
        for j, mj in enumerate(meshes):
            if i == j:
                continue
            p2p = np.arange(mj.n_vertices)                      # (the tori share their grid)
            bad = rng.random(p2p.shape[0]) < 0.10
            p2p[bad] = rng.integers(mi.n_vertices, size=int(bad.sum()))
            maps[(i, j)] = mj.eigenvectors[:, :M].T @ (mj.A @ mi.eigenvectors[p2p, :M])
    return maps


def one_iteration(net, maps0, M, wt, sync):
    net.set_maps(maps0)
    net.M = M
    sync()
    t0 = time.perf_counter()
    net.zoomout_iteration(int(0.9 * M), M, M + 2, weight_type=wt, complete=False)
    sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    from densematcher_amd.engine import default_engine
    from densematcher_amd.pyFM import FMN
    eng = default_engine()
    meshes, samples = build(args.meshes, 52)
    for M in (20, 50):
        maps0 = initial_maps(meshes, M)
        for wt in ("adjacency", "icsm"):
            dev = FMN(meshes, maps_dict=None, device=True)
            dev.set_subsample(samples)
            one_iteration(dev, maps0, M, wt, torch.cuda.synchronize)
            times = sorted(one_iteration(dev, maps0, M, wt, torch.cuda.synchronize) for _ in range(args.reps))
            eng.profile_kernel("*")
            one_iteration(dev, maps0, M, wt, torch.cuda.synchronize)
            report = eng.profile_report()
            eng.profile_kernel(None)
            row = {"M": M, "weight_type": wt, "meshes": args.meshes, "edges": len(maps0), "device_ms": 1e3 * times[len(times) // 2]}
            if not args.no_host:
                host = FMN(meshes, maps_dict=None, device=False)
                host.set_subsample(samples)
                row["host_ms"] = 1e3 * one_iteration(host, maps0, M, wt, lambda: None)
            print(json.dumps(row), flush=True)
            top = sorted(report.items(), key=lambda kv: -kv[1][1])[:12]
            print("   profile (launches, ms): " + ", ".join(f"{k}: {v[0]}, {v[1]:.3f}" for k, v in top), flush=True)


if __name__ == "__main__":
    main()

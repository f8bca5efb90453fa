#!/usr/bin/env python
"""
Time get_all_operators (densematcher_amd.diffusion_net.geometry) on 16 perturbed tori of 2048 vertices, k_eig = 128: the device route
(one batched call of dm_dnet_rows / dm_dnet_ell + dm_eigenbasis) against the host route (vectorised NumPy + SciPy's eigsh, one mesh after
the other) in the same process.  Both arms: warm-up calls first, device synchronise, median of the repeats; one JSON line.

    python tools/dnet_ops_time.py [--meshes 16] [--repeats 5] [--host-repeats 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--k-eig", type=int, default=128)
    a = ap.parse_args()
    from densematcher_amd import synth
    from densematcher_amd.diffusion_net import geometry as geo
    meshes = [synth.torus_mesh(64, 32, perturb=0.08, seed=s) for s in range(a.meshes)]
    verts = [torch.from_numpy(v) for v, _ in meshes]
    faces = [torch.from_numpy(f) for _, f in meshes]

    def timed(route, repeats, warmup):
        times = []
        for it in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = geo.get_all_operators(verts, faces, a.k_eig, route=route)
            torch.cuda.synchronize()
            if it >= warmup:
                times.append(time.perf_counter() - t0)
        return statistics.median(times), out

    dev_s, dev = timed("device", a.repeats, 2)
    host_s, host = timed("host", a.host_repeats, 1)
    lam_dev = max(float((d - h).abs().max() / h[-1]) for d, h in zip(dev[3], host[3]))
    gx_dev = max(float((d.to_dense() - h.to_dense()).abs().max() / h.to_dense().abs().max()) for d, h in zip(dev[5], host[5]))
    print(json.dumps({"meshes": a.meshes, "n_verts": int(verts[0].shape[0]), "device_repeats": a.repeats, "device_warmup": 2, "host_repeats": a.host_repeats, "host_warmup": 1, "k_eig": a.k_eig, "device_s": round(dev_s, 4), "host_s": round(host_s, 4),
                      "device_s_per_mesh": round(dev_s / a.meshes, 5), "host_s_per_mesh": round(host_s / a.meshes, 5),
                      "speedup": round(host_s / dev_s, 1), "max_rel_evals_diff": lam_dev, "max_rel_gradX_diff": gx_dev}))


if __name__ == "__main__":
    main()

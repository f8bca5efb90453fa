#!/usr/bin/env python
"""
Timing of the shape difference operators, device route against host route on the same box (one process, the arms alternating, every
arm after a warm-up; the device arm is bracketed by HIP events on the engine's stream AND by a host clock -- it ends with the
operators on the device --, the host arm by the host clock: median and min - max are reported).

    python tools/shape_diff_time.py [--meshes 16] [--repeats 5] [--out profiles/shape_diff_time.txt]

Input: --meshes tori of 2 048 vertices (4 096 faces, seeded perturbations) against one base torus, one seeded vertex map per pair
(repeats, not surjective).  Stiffness rows and masses from the package's device assembly; the bases are seeded stand-ins
(synth.random_basis, 384 columns: throughput only, the arithmetic does not care).  k1 = 20 / 50 / 128 (k2 = 3 k1), SD_type spectral and
semican:
    device   pyFM.spectral.compute_SD_many(device=True): one call per kernel for all pairs, the meshes hand over the device rows
    host     compute_SD per pair (device=False): NumPy / SciPy products, the reference's arithmetic
and the same for ONE pair (compute_SD, device=True against device=False).
"""
import argparse
import copy
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
from densematcher_amd.pyFM.spectral import shape_difference as sd  # noqa: E402

KMAX = 384


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed_device(fn):
    """(HIP event time, host clock) of a call that leaves its results on the device"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms ({min(ts):.3f} - {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shape_diff_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shape_diff_time: no GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    dev_meshes = [TriMesh(*synth.torus_mesh(64, 32, perturb=0.0 if s == 0 else 0.1, seed=s)) for s in range(args.meshes + 1)]
    TriMesh._assemble_many(dev_meshes, robust=False)
    for s, m in enumerate(dev_meshes):
        m.eigenvalues, m.eigenvectors, _ = synth.random_basis(m.n_vertices, KMAX, seed=100 + s)
    host_meshes = [copy.copy(m) for m in dev_meshes]
    for m in host_meshes:
        m.W, m.A                                                 # (materialised on the host once, outside the clock)
    n = dev_meshes[0].n_vertices
    maps = [rng.integers(0, n, n) for _ in range(args.meshes)]
    maps_dev = [torch.as_tensor(p).cuda() for p in maps]
    say(f"# {torch.cuda.get_device_name(0)}; {args.meshes} meshes of {n} vertices against one base, one map each; repeats {args.repeats}")
    say("# columns: device route HIP events | device route host clock | host route host clock | host / device (host clocks)")
    for SD_type in ("spectral", "semican"):
        for k1 in (20, 50, 128):
            def device():
                return sd.compute_SD_many(dev_meshes[0], dev_meshes[1:], k1=k1, p2ps=maps_dev, SD_type=SD_type, device=True)

            def host():
                return sd.compute_SD_many(host_meshes[0], host_meshes[1:], k1=k1, p2ps=maps, SD_type=SD_type, device=False)

            def device1():
                return sd.compute_SD(dev_meshes[0], dev_meshes[1], k1=k1, p2p=maps_dev[0], SD_type=SD_type, device=True)

            def host1():
                return sd.compute_SD(host_meshes[0], host_meshes[1], k1=k1, p2p=maps[0], SD_type=SD_type, device=False)

            got, ref = device(), host()                          # warm-up of both arms, and the comparison
            worst = max(float(np.abs(got[q][b].cpu().numpy() - ref[q][b])[1:].max() / np.abs(ref[q][b])[1:].max())
                        for q in range(2) for b in range(args.meshes))
            device1(), host1()
            te, td, th, te1, td1, th1 = [], [], [], [], [], []
            for _ in range(args.repeats):                        # (the arms alternate)
                e, d = timed_device(device)
                te.append(e), td.append(d)
                th.append(timed_host(host))
                e, d = timed_device(device1)
                te1.append(e), td1.append(d)
                th1.append(timed_host(host1))
            say(f"{SD_type:8s} k1 {k1:3d}  {args.meshes:2d} pairs  {fmt(te)} | {fmt(td)} | {fmt(th)} | {statistics.median(th) / statistics.median(td):6.1f}"
                f"   (largest difference outside row 0, relative to the largest entry: {worst:.1e})")
            say(f"{SD_type:8s} k1 {k1:3d}   1 pair   {fmt(te1)} | {fmt(td1)} | {fmt(th1)} | {statistics.median(th1) / statistics.median(td1):6.1f}")
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

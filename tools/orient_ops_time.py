#!/usr/bin/env python
"""
Timing of the orientation operators of a fit with w_orient > 0, device route against host route on the same box (one process, the arms
alternating, every arm after a warm-up, bracketed by device synchronisation: median and min - max are reported).

    python tools/orient_ops_time.py [--pairs 8] [--repeats 3] [--out profiles/orient_ops_time.txt]

Both arms start from the meshes, bases and descriptors on the host and end with the two operator sets a fit needs (the rescaling
operators, rows divided by vertex_areas, and the optimisation operators, rows divided by diag(A)) of both meshes of a pair:
    host     FunctionalMapping.compute_orientation_op(area="vertex") + (area="mass"): per descriptor and mesh a sparse assembly and two
             sparse-dense products, twice (what fit(orient_route="host") runs, unchanged from the parent commit)
    device   what fit(orient_route="device") / compute_surface_map_batch run: MatchEngine.orientation_ops per mesh side, one call
             serving both forms (lumped masses); "batch": --pairs pairs stacked in one call per side, reported per pair
Cases: N = 2048 vertices (4096 faces), k = 15 / 50, D = 128 / 768 fp16 descriptors.  The host arm is timed on one pair (a batch of pairs
is that loop, pair after pair).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from densematcher_amd import synth  # noqa: E402
from densematcher_amd.engine import default_engine  # noqa: E402
from densematcher_amd.pyFM import FunctionalMapping, TriMesh  # noqa: E402
from densematcher_amd.pyFM.functional import _orientation_ops_device  # noqa: E402


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def fmt(ts):
    return f"{statistics.median(ts):10.3f} ms  ({min(ts):.3f} - {max(ts):.3f}, n = {len(ts)})"


def make_mesh(seed, k):
    verts, faces = synth.torus_mesh(64, 32, perturb=0.1, seed=seed)
    lam, phi, a = synth.random_basis(verts.shape[0], k, seed)
    m = TriMesh(verts, faces)
    m.A = sp.diags(a).tocsr()
    m.W = sp.identity(m.n_vertices).tocsr()
    m.eigenvalues, m.eigenvectors = lam, phi
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "orient_ops_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("orient_ops_time: no GPU")
    eng = default_engine()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N = 2048
    say(f"# {torch.cuda.get_device_name(0)}; N = {N}, 4096 faces, float64 basis, fp16 descriptors; repeats {args.repeats}, batch of {args.pairs} pairs")
    rng = np.random.default_rng(0)
    for k in (15, 50):
        meshes = [make_mesh(s, k) for s in range(2)]
        for D in (128, 768):
            F = [rng.standard_normal((N, D)).astype(np.float16) for _ in range(2)]
            model = FunctionalMapping(meshes[0], meshes[1])
            model.preprocess(n_ev=(k, k), n_descr=D, descr1=F[0], descr2=F[1], subsample_step=1)
            B = args.pairs
            stack = [(np.stack([m.vertlist] * B), np.stack([m.facelist] * B), np.stack([m.eigenvectors] * B), np.stack([f] * B))
                     for m, f in zip(meshes, F)]

            def host():
                return model.compute_orientation_op(), model.compute_orientation_op(area="mass")

            def device():
                return _orientation_ops_device(eng, [model], [m.eigenvectors[None] for m in meshes], [f[None] for f in F], "vertex")[0]

            def batch():
                return [eng.orientation_ops(v, f, P, Fd, k=k) for v, f, P, Fd in stack]
            th, td, tb = [], [], []
            for _ in range(2):                                   # (the arms alternate)
                th += timed(host, 1, warmup=0)
                td += timed(device, args.repeats)
                tb += timed(batch, args.repeats)
            tag = f"k = {k:2d}, D = {D:3d}"
            say(f"{tag}   host, one pair            {fmt(th)}")
            say(f"{tag}   device, one pair          {fmt(td)}")
            say(f"{tag}   device, per pair of {B:3d}   {fmt([t / B for t in tb])}")
            say(f"{tag}   host / device = {statistics.median(th) / statistics.median(td):.1f} (one pair), "
                f"{statistics.median(th) / (statistics.median(tb) / B):.1f} (batch)")
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

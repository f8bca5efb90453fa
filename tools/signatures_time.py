#!/usr/bin/env python
"""
Timing of the spectral signatures (HKS / WKS) as a descriptor source of the fit, device route against host route on the same box (one
process, the arms alternating, every arm after a warm-up, bracketed by device synchronisation: median and min - max are reported).

    python tools/signatures_time.py [--meshes 128] [--repeats 5] [--out profiles/signatures_time.txt]

Both arms start from the eigenpairs on the host (where TriMesh keeps them) and end with the fp32 descriptors of the fit on the device:
    host     pyFM.signatures.mesh_HKS / mesh_WKS per mesh (NumPy float64), converted to fp32, stacked and uploaded
    device   MatchEngine.signatures(..., out_dtype=float32): the parameter tables built on the host, the eigenvectors uploaded,
             dm_spectral_signatures_f64 (weights kernel + one float64 matrix-core product per mesh and block)
             "kernels": the same call with the eigenvectors already on the device
Cases: 1 mesh and --meshes meshes of 2048 vertices, k = 50; HKS-16 and WKS-2048 (compute_surface_map's sizes).
"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from densematcher_amd import synth  # noqa: E402
from densematcher_amd.engine import default_engine  # noqa: E402
from densematcher_amd.pyFM import signatures as sg  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "signatures_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("signatures_time: no GPU")
    eng = default_engine()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N, k = 2048, 50
    say(f"# {torch.cuda.get_device_name(0)}; N = {N}, k = {k}, float64 basis; repeats {args.repeats}")
    distinct = [synth.random_basis(N, k, seed) for seed in range(4)]
    for B in (1, args.meshes):
        meshes = [types.SimpleNamespace(eigenvalues=distinct[b % 4][0] * (1.0 + 0.01 * b), eigenvectors=distinct[b % 4][1]) for b in range(B)]
        Phi = np.stack([m.eigenvectors for m in meshes])
        lam = np.stack([m.eigenvalues for m in meshes])
        Phi_d = torch.as_tensor(Phi).to(eng.device)
        for kind, num in (("HKS", 16), ("WKS", 2048)):
            fn = sg.mesh_HKS if kind == "HKS" else sg.mesh_WKS

            def host():
                with np.errstate(all="ignore"):
                    F = np.stack([np.ascontiguousarray(fn(m, num, k=k), dtype=np.float32) for m in meshes])
                return torch.as_tensor(F).to(eng.device)

            def device():
                return eng.signatures(Phi, lam, kind, num, out_dtype=torch.float32)

            def kernels():
                return eng.signatures(Phi_d, lam, kind, num, out_dtype=torch.float32)
            reps = args.repeats if (B == 1 or kind == "HKS") else max(2, args.repeats // 2)
            th, td, tk = [], [], []
            for _ in range(2):                                   # (the arms alternate)
                th += timed(host, reps)
                td += timed(device, reps)
                tk += timed(kernels, reps)
            say(f"{kind}-{num:<5d} {B:4d} mesh(es)   host    {fmt(th)}")
            say(f"{kind}-{num:<5d} {B:4d} mesh(es)   device  {fmt(td)}")
            say(f"{kind}-{num:<5d} {B:4d} mesh(es)   kernels {fmt(tk)}")
            say(f"{kind}-{num:<5d} {B:4d} mesh(es)   host / device = {statistics.median(th) / statistics.median(td):.2f}")
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""
All-pairs heat-method geodesics on the device, timed per call: MatchEngine.heat_geodesic_factor + heat_geodesic for B meshes of
N vertices (perturbed tori, cotangent Laplacian), bracketed with HIP events after one untimed call of the same shape, profiler off.
The bracket holds the whole call: host checks, uploads, the kernels, the gaps between them; the meshes' W and A are built before it.
One JSON line per (N, B): factor / solve / total ms per mesh (median of --reps) and the f64 rate of the nominal 4.7 N^3 flops per
mesh (two Cholesky factorisations at N^3 / 3, 4 N^3 of substitutions) against the 78.6 TF f64 matrix peak.

    python tools/geodesic_timing.py                     # N = 512 / 2048 / 8192, B = 1 / 16 / 64 (shapes over --max-gb skipped)
    python tools/geodesic_timing.py --sizes 2048 --batches 1
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densematcher_amd import synth  # noqa: E402
from densematcher_amd.engine import default_engine  # noqa: E402
from densematcher_amd.pyFM.mesh import laplacian as lap  # noqa: E402

PEAK_F64 = 78.6e12
GRIDS = {512: (32, 16), 2048: (64, 32), 8192: (128, 64)}


def mesh(N, seed):
    nu, nv = GRIDS[N]
    V, F = synth.torus_mesh(nu, nv, perturb=0.05, seed=seed)
    W, mass = lap.cotangent_laplacian(V, F)
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    t = np.linalg.norm(V[e[:, 0]] - V[e[:, 1]], axis=1).mean() ** 2
    return (V, F, W, mass), t


def run(eng, N, B, reps):
    ms = [mesh(N, s) for s in range(min(B, 4))]
    ops = [ms[b % len(ms)][0] for b in range(B)]
    ts = [ms[b % len(ms)][1] for b in range(B)]
    fac = eng.heat_geodesic_factor(ops, ts)                              # warm-up of both phases
    D = eng.heat_geodesic(fac)
    del D, fac
    torch.cuda.synchronize()
    tf, tsol = [], []
    for _ in range(reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        fac = eng.heat_geodesic_factor(ops, ts)
        e1.record()
        D = eng.heat_geodesic(fac)
        e2.record()
        torch.cuda.synchronize()
        tf.append(e0.elapsed_time(e1))
        tsol.append(e1.elapsed_time(e2))
        del D, fac
    f, s = float(np.median(tf)) / B, float(np.median(tsol)) / B
    flops = 4.7 * float(N) ** 3
    return {"N": N, "B": B, "reps": reps, "factor_ms_per_mesh": round(f, 3), "solve_ms_per_mesh": round(s, 3),
            "total_ms_per_mesh": round(f + s, 3), "tflops": round(flops / ((f + s) * 1e-3) / 1e12, 2),
            "frac_f64_peak": round(flops / ((f + s) * 1e-3) / PEAK_F64, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048, 8192])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-gb", type=float, default=64.0, help="skip shapes whose factors + distances + work space exceed this")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geodesic_timing: no GPU")
    eng = default_engine()
    for N in a.sizes:
        for B in a.batches:
            need = B * 8.0 * N * N * 6 / 1e9                             # 2 factors + 2 work arrays + D rows + D transposed
            if need > a.max_gb:
                print(json.dumps({"N": N, "B": B, "skipped": f"needs {need:.0f} GB > --max-gb {a.max_gb:.0f}"}), flush=True)
                continue
            t0 = time.time()
            r = run(eng, N, B, a.reps)
            r["wall_s"] = round(time.time() - t0, 1)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

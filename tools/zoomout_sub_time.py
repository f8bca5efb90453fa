#!/usr/bin/env python
"""
Timing of subsampled ZoomOut and of farthest-point sampling (one process, the arms alternating, every arm after a warm-up, bracketed
by device synchronisation, several repeats: median and min - max are reported).

    python tools/zoomout_sub_time.py [--pairs 32] [--host-pairs 4] [--repeats 5] [--out profiles/zoomout_sub_time.txt]

ZoomOut (BASELINE config 4's shape: N = 2048, 50 -> 200 in 150 iterations, float64 basis), per sample count ns = 512 / 1024:
    sub_fused    MatchEngine.zoomout(subsample=...) = dm_zoomout_sub, all pairs in one call        ("zoomout_sub_fused" = 1)
    sub_host     refine.zoomout_refine(subsample=...) with "zoomout_sub_fused" = 0: the search and dm_p2p_to_fm_lstsq chained from
                 the host, pair by pair (its surface takes one pair); timed on --host-pairs pairs, reported per pair
    full         dm_zoomout on all vertices of the same pairs
and the launches per iteration of the new loop from profile_report(kernels=True).
Samplers (size 512, N = 2048, 1 and 64 meshes): dm_fps_euclid, dm_fps_heat by both routes (factorisation timed apart), against the
host loops they replace (NumPy Euclidean distances; SciPy Dijkstra = extract_fps()'s default), timed on one mesh.
"""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from densematcher_amd import synth  # noqa: E402
from densematcher_amd.engine import default_engine  # noqa: E402


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


def fmt(ts, div=1.0):
    ts = [t / div for t in ts]
    return f"{statistics.median(ts):10.3f} ms  ({min(ts):.3f} - {max(ts):.3f}, n = {len(ts)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--host-pairs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--fps-batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "zoomout_sub_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zoomout_sub_time: no GPU")
    from densematcher_amd.pyFM import refine
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    eng = default_engine()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, nit, k0 = args.pairs, args.nit, 50
    say(f"# {torch.cuda.get_device_name(0)}; {B} pairs, N = 2048, {k0} -> {k0 + nit}, float64 basis; repeats {args.repeats}")
    batch = synth.make_pair_batch(B, 64, 32, 8, k0 + nit, sigma=0.1, n_distinct_meshes=2, seed0=9, real_dtype=np.float64)
    rng = np.random.default_rng(4)
    C0 = np.stack([np.eye(k0) + 0.02 * rng.standard_normal((k0, k0)) for _ in range(B)])
    Phi1 = torch.as_tensor(np.asarray(batch["Phi1"], np.float64)).to(eng.device)
    Phi2 = torch.as_tensor(np.asarray(batch["Phi2"], np.float64)).to(eng.device)
    a2 = torch.as_tensor(np.asarray(batch["a2"], np.float64)).to(eng.device)
    C0d = torch.as_tensor(C0).to(eng.device)
    P1h, P2h = Phi1.cpu().numpy(), Phi2.cpu().numpy()

    full = lambda: eng.zoomout(Phi1, Phi2, a2, C0d, nit, 1, return_p2p=True)
    for ns in (512, 1024):
        subs = [(np.sort(np.random.default_rng(7 + b).choice(2048, ns, replace=False)),
                 np.sort(np.random.default_rng(107 + b).choice(2048, ns + 32, replace=False))) for b in range(B)]
        s1 = torch.as_tensor(np.stack([s[0] for s in subs]).astype(np.int32)).to(eng.device)
        s2 = torch.as_tensor(np.stack([s[1] for s in subs]).astype(np.int32)).to(eng.device)
        fused = lambda: eng.zoomout(Phi1, Phi2, None, C0d, nit, 1, return_p2p=True, subsample=(s1, s2))
        hp = min(args.host_pairs, B)

        def host():
            eng.set_option("zoomout_sub_fused", 0)
            try:
                return [refine.zoomout_refine(C0[b], P1h[b], P2h[b], nit=nit, step=1, subsample=subs[b], return_p2p=True) for b in range(hp)]
            finally:
                eng.set_option("zoomout_sub_fused", 1)

        # agreement of the two paths on the timed input (maps equal, C within 1e-9), before any number is trusted
        Cf, pf = fused()
        ref = host()
        same = all(np.array_equal(pf[b].cpu().numpy(), ref[b][1]) for b in range(hp))
        dC = max(np.abs(Cf[b].cpu().numpy() - ref[b][0]).max() for b in range(hp))
        tf, th, tl = [], [], []
        timed(fused, 1, 1), timed(full, 1, 1)
        for _ in range(args.repeats):                             # alternating arms
            tf += timed(fused, 1, 0)
            th += timed(host, 1, 0)
            tl += timed(full, 1, 0)
        say(f"ns = {ns}   (sub_fused against sub_host on the first {hp} pairs: vertex maps equal {same}, max |C - C| = {dC:.2e})")
        say(f"  sub_fused  {B:3d} pairs in one call   {fmt(tf)}    per pair {fmt(tf, B)}")
        say(f"  sub_host   {hp:3d} pairs, one by one   {fmt(th)}    per pair {fmt(th, hp)}")
        say(f"  full       {B:3d} pairs in one call   {fmt(tl)}    per pair {fmt(tl, B)}")
        say(f"  per pair: sub_host / sub_fused = {statistics.median(th) / hp / (statistics.median(tf) / B):.1f} x, "
            f"full / sub_fused = {statistics.median(tl) / statistics.median(tf):.2f} x")
        one = lambda: eng.zoomout(Phi1[:1], Phi2[:1], None, C0d[:1], nit, 1, return_p2p=True, subsample=(s1[:1], s2[:1]))
        t1 = timed(one, args.repeats)
        say(f"  sub_fused    1 pair                  {fmt(t1)}    sub_host / sub_fused at one pair = "
            f"{statistics.median(th) / hp / statistics.median(t1):.1f} x")
        eng.profile_kernel("*")
        eng.zoomout(Phi1, Phi2, None, C0d, nit, 1, subsample=(s1, s2))
        rep = eng.profile_report(kernels=True)
        eng.profile_kernel(None)
        per_it = {name: v[0] for name, v in rep.items() if v[0] >= nit}
        say(f"  launches of the new loop: {sum(per_it.values())} in {nit} iterations = {sum(per_it.values()) / nit:.2f} per iteration {per_it}; "
            f"once per call: { {name: v[0] for name, v in rep.items() if v[0] < nit} }")
        say("  device time by kernel (ms, all pairs): " + ", ".join(f"{name} {v[1]:.2f}" for name, v in rep.items()))

    # ---- samplers
    size, Bm = 512, args.fps_batch
    say()
    say(f"# farthest-point sampling, size {size}, N = 2048")
    meshes = []
    for b in range(Bm):
        V, F = synth.torus_mesh(64, 32, perturb=0.08, seed=b)
        meshes.append(TriMesh(V, F))
    starts = [int(np.random.default_rng(b).integers(2048)) for b in range(Bm)]
    for nb in (1, Bm):
        ms, st = meshes[:nb], starts[:nb]
        V = np.stack([m.vertlist for m in ms]).astype(np.float64)
        Vd = torch.as_tensor(V).to(eng.device)
        say(f"{nb} mesh(es)")
        say(f"  dm_fps_euclid                        {fmt(timed(lambda: eng.fps(Vd, size, st), args.repeats))}")
        t0 = time.perf_counter()
        fac = eng.heat_geodesic_factor([m._geod_operands() for m in ms], [m._heat_time() for m in ms])
        torch.cuda.synchronize()
        say(f"  heat factorisation (once per batch)  {(time.perf_counter() - t0) * 1e3:10.3f} ms")
        outs = {}
        for route, label in ((1, "all-pairs rows + one sampling launch"), (2, "one single-source solve per sample")):
            eng.set_option("fps_heat_route", route)
            try:
                ts = timed(lambda: outs.__setitem__(route, eng.fps_heat(fac, size, st)), max(2, args.repeats // 2))
            finally:
                eng.set_option("fps_heat_route", 0)
            say(f"  dm_fps_heat route {'(a)' if route == 1 else '(b)'} {label:36s} {fmt(ts)}")
        assert torch.equal(outs[1], outs[2])
        del fac
    m = meshes[0]

    def host_euclid():
        Vh = m.vertlist
        inds = [starts[0]]
        d = np.linalg.norm(Vh - Vh[inds[0], None, :], axis=1)
        for _ in range(size - 1):
            inds.append(int(np.argmax(d)))
            d = np.minimum(d, np.linalg.norm(Vh - Vh[inds[-1], None, :], axis=1))
        return np.asarray(inds)

    assert np.array_equal(host_euclid(), eng.fps(m.vertlist[None], size, starts[0])[0].cpu().numpy())
    say(f"host, one mesh: NumPy Euclidean loop     {fmt(timed(host_euclid, args.repeats))}")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        say(f"host, one mesh: extract_fps() default (SciPy Dijkstra)  {fmt(timed(lambda: m.extract_fps(size, start=starts[0]), 2))}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""
Heat-method geodesic fixture, produced by IMPORTING THE REFERENCE (/root/reference) in the build container (recipe and stubs:
tools/make_golden.py, which this script re-uses, like make_golden_r05.py).

    fx_geod.npz   the reference's TriMesh.get_geodesic(robust=False) (pyFM/mesh/trimesh.py:612-692 -> geometry.heat_geodmat,
                  geometry.py:673-740: SciPy SuperLU on A + tW and W) on three meshes, inputs included:
        torus_*   perturbed 64 x 32 torus (N = 2048): D[:, torus_cols] (16 stored columns of the full matrix)
        grid_*    open bumpy 40 x 30 grid (N = 1200, boundary): D[:, grid_cols]
        small_*   irregular planar-Delaunay mesh with obtuse triangles, lifted (N = 160): the full matrix D (sym=True is
                  0.5 D + (0.5 D)^T, the reference's own arithmetic on it, trimesh.py:677-679), the edges, and
                  geodesic_distmat_dijkstra rows for small_dijk_rows
        *_t       t = (mean edge length)^2 (trimesh.py:661-665);  torus_from_j / torus_from: geod_from(j, robust=False)
                  (trimesh.py:694-738; a fresh mesh per call: the reference's second call on one mesh names an unbound variable)
    One committed file must stay under 1 MiB, so the large meshes keep a few columns.
Run time here: about fifteen seconds.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
from densematcher.pyFM.mesh import geometry as ref_geom  # noqa: E402

OUT = mg.OUT


def bumpy_grid(nx=40, ny=30, seed=7):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(0.0, 2.0, nx), np.linspace(0.0, 1.5, ny), indexing="ij")
    z = 0.15 * np.sin(3.0 * x) * np.cos(4.0 * y) + 0.1 * np.exp(-((x - 1.0) ** 2 + (y - 0.7) ** 2) / 0.1)
    V = np.stack([x.ravel(), y.ravel(), z.ravel()], 1) + 0.004 * rng.standard_normal((nx * ny, 3))
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    v00, v10, v01, v11 = (i * ny + j).ravel(), ((i + 1) * ny + j).ravel(), (i * ny + j + 1).ravel(), ((i + 1) * ny + j + 1).ravel()
    F = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)])
    return V, F.astype(np.int64)


def irregular_mesh(n=160, seed=11):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1.0, (n, 2)) * np.array([2.5, 1.0])
    F = Delaunay(p).simplices.astype(np.int64)
    V = np.concatenate([p, (0.3 * np.sin(2.0 * p[:, :1]) * np.cos(3.0 * p[:, 1:]))], 1)
    a = 0.5 * np.linalg.norm(np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]), axis=1)
    F = F[a > 1e-4]                                   # (no sliver at the hull)
    used = np.unique(F)
    remap = np.full(n, -1)
    remap[used] = np.arange(len(used))
    return V[used], remap[F]


def ref_mesh(V, F):
    m = mg.TriMesh(V, F)
    m.process(k=0)
    return m


def main():
    out = {}
    for name, (V, F), cols in (("torus", mg.synth.torus_mesh(64, 32, perturb=0.08, seed=3), np.arange(0, 2048, 128)),
                               ("grid", bumpy_grid(), np.arange(0, 1200, 75)),
                               ("small", irregular_mesh(), None)):
        m = ref_mesh(V, F)
        D = m.get_geodesic(robust=False, force_compute=True)
        e = m.edges
        t = np.linalg.norm(m.vertlist[e[:, 1]] - m.vertlist[e[:, 0]], axis=1).mean() ** 2
        out[name + "_V"], out[name + "_F"], out[name + "_t"] = V, F.astype(np.int32), t
        if cols is None:
            out[name + "_D"] = D
            out[name + "_edges"] = e.astype(np.int32)
        else:
            out[name + "_cols"], out[name + "_D"] = cols, D[:, cols]
        print(name, V.shape[0], "vertices, max D", D.max(), flush=True)
    js = np.array([5, 777, 2047])
    V, F = out["torus_V"], out["torus_F"].astype(np.int64)
    out["torus_from_j"] = js
    out["torus_from"] = np.stack([ref_mesh(V, F).geod_from(int(j), robust=False) for j in js], 1)
    rows = np.arange(0, out["small_V"].shape[0], 5)
    out["small_dijk_rows"] = rows
    out["small_dijk"] = ref_geom.geodesic_distmat_dijkstra(out["small_V"], out["small_F"].astype(np.int64))[rows]
    path = os.path.join(OUT, "fx_geod.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

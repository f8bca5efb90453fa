#!/usr/bin/env python
"""
Farthest-point-sampling fixture, produced by IMPORTING THE REFERENCE in the build container (recipe and stubs: tools/make_golden.py,
which this script re-uses, like make_golden_geod.py).

    fx_fps.npz   the reference's geometry.farthest_point_sampling_call (pyFM/mesh/geometry.py:813-851) with the Euclidean distance
                 function of TriMesh.extract_fps(geodesic=False) (pyFM/mesh/trimesh.py:871-877) on
        cfg1_verts1, cfg1_verts2   the two meshes of fx_cfg1.npz, 200 samples each
        torus_V, grid_V, small_V   the three meshes of fx_geod.npz, 64 samples each
    One int32 index list per mesh; its first entry is the start vertex the reference drew (it draws from an unseeded generator,
    so a re-run writes other lists: the tests start from the recorded vertex).
Run time here: a few seconds.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
from densematcher.pyFM.mesh import geometry as ref_geom  # noqa: E402

OUT = mg.OUT


def ref_fps(V, size):
    V = np.asarray(V, np.float64)

    def dist_func(i):                                           # trimesh.py:872-873
        return np.linalg.norm(V - V[i, None, :], axis=1)

    return ref_geom.farthest_point_sampling_call(dist_func, size, n_points=V.shape[0])


def restated(V, size, start):
    V = np.asarray(V, np.float64)
    inds = [int(start)]
    d = np.linalg.norm(V - V[inds[0]], axis=1)
    ties = 0
    for _ in range(size - 1):
        ties += int(np.count_nonzero(d == d.max()) > 1)
        inds.append(int(np.argmax(d)))
        d = np.minimum(d, np.linalg.norm(V - V[inds[-1]], axis=1))
    return np.asarray(inds), ties


def main():
    cfg1 = np.load(os.path.join(OUT, "fx_cfg1.npz"))
    geod = np.load(os.path.join(OUT, "fx_geod.npz"))
    out = {}
    for name, V, size in (("cfg1_verts1", cfg1["verts1"], 200), ("cfg1_verts2", cfg1["verts2"], 200),
                          ("torus_V", geod["torus_V"], 64), ("grid_V", geod["grid_V"], 64), ("small_V", geod["small_V"], 64)):
        inds = np.asarray(ref_fps(V, size))
        again, ties = restated(V, size, inds[0])
        assert np.array_equal(inds, again), name
        out[name] = inds.astype(np.int32)
        print(name, V.shape[0], "vertices, start", int(inds[0]), "steps with tied maxima:", ties, flush=True)
    path = os.path.join(OUT, "fx_fps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

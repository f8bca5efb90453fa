#!/usr/bin/env python
"""
Precise-map fixture on designed inputs, produced by IMPORTING THE REFERENCE (/root/reference) in the build container (recipe and
stubs: tools/make_golden.py, which this script re-uses, like make_golden_geod.py).

    fx_precise_regions.npz   the reference's face choice and barycentric weights (pyFM/spectral/projection_utils.py:
                             compute_lmax, compute_Deltamin, compute_all_dmin, then project_to_mesh per point -- what
                             project_pc_to_triangles runs before it packs the result into a sparse matrix) on
        a_<shape>_k<k>   the four planar triangles of tests/precise_restate.py (every one of the 25 return statements of the
                         projection is the winner's somewhere), the triangle TWICE in the face list: several candidates with an
                         exact tie, k = 3 and k = 17
        b_corner, b_twin the open obtuse corner above a large far triangle (and the corner with its face turned, [0, 2, 1]): the
                         vectorised code's region-4 distances decide which face wins
        <name>_face (n,) int32, <name>_bary (n,3) float64;  inputs_sha256: the inputs are NOT stored, tests regenerate them
                         (precise_restate.fixture_inputs) and compare this hash
The script asserts what the fixture is for: in (b), per mesh, at least 5 points whose reference winner is farther than the truly
nearest face by more than 1e-9, every one of them with the corner's face in branch 4b or 4e.
Run time here: a few seconds.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
from densematcher.pyFM.spectral import projection_utils as ref_pu  # noqa: E402

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
import precise_restate as pr  # noqa: E402


def reference_projection(V, faces, P):
    lmax = ref_pu.compute_lmax(V, faces)
    Deltamin = ref_pu.compute_Deltamin(V, P)
    dmin = ref_pu.compute_all_dmin(V, faces, P)
    fm, bary = np.zeros(len(P), dtype=np.int32), np.zeros((len(P), 3))
    for i in range(len(P)):
        f, b = ref_pu.project_to_mesh(V, faces, P, i, lmax, Deltamin, dmin=dmin)
        fm[i], bary[i] = int(np.asarray(f).ravel()[0]), np.asarray(b).ravel()
    return fm, bary


def main():
    inputs = pr.fixture_inputs()
    out = {"inputs_sha256": np.array(pr.fixture_hash(inputs))}
    for name, (V, faces, P) in inputs.items():
        fm, bary = reference_projection(V, faces, P)
        out[name + "_face"], out[name + "_bary"] = fm, bary
        if name.startswith("a_"):
            assert not fm.any(), "the reference does not name the first of two equal faces"
        else:
            d_win = pr.face_distance(V, faces, P, fm)
            d_min, _ = pr.nearest_distance(V, faces, P)
            farther = np.where(d_win - d_min > 1e-9)[0]
            labels = {pr.branch(*pr.abcdef(V[faces[0]], P[i:i + 1])[0]) for i in farther}
            print(name, len(P), "points;", len(farther), "where the reference names the farther face; branches", sorted(labels))
            assert len(farther) >= 5 and labels <= {"4b", "4e"} and np.all(fm[farther] == 1)
    path = os.path.join(mg.OUT, "fx_precise_regions.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

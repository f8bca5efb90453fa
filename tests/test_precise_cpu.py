"""
CPU: the reference side of the precise map (oracle/dm_oracle.py: _point_triangle, project_pc_to_triangles) held against an
independent longdouble solver (tests/precise_restate.py) on inputs designed to leave through every one of the projection's 25
return statements, and against the reference itself on those inputs (tests/golden/fx_precise_regions.npz,
tools/make_golden_precise.py).  tests/test_gpu_precise.py holds the device against the same.
"""
import collections
import os

import numpy as np
import pytest

import precise_restate as pr
from oracle import dm_oracle as orc

TOL = 1e-9            # the project's precise-map tolerance (tests/test_gpu_parity.py: test_precise_map_and_its_assignment)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_precise_regions.npz")


@pytest.fixture(scope="module")
def fixture():
    fx = dict(np.load(GOLDEN, allow_pickle=False))
    inputs = pr.fixture_inputs()
    assert pr.fixture_hash(inputs) == str(fx["inputs_sha256"]), "regenerated inputs differ from the ones the reference was run on"
    return fx, inputs


def test_solver_on_hand_cases():
    """the independent solver itself: interior, edge, corner, and a point above the plane, worked by hand"""
    tri = np.array([(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)])
    P = np.array([(0.5, 0.5, 3.0), (1.0, -1.0, 0.0), (-1.0, -1.0, 0.0), (2.0, 2.0, 0.0), (5.0, -1.0, 1.0)])
    q, b, d = pr.closest_point(tri, P)
    assert np.abs(q - np.array([(0.5, 0.5, 0), (1, 0, 0), (0, 0, 0), (1, 1, 0), (2, 0, 0)])).max() < 1e-18
    assert np.abs(b - np.array([(0.5, 0.25, 0.25), (0.5, 0.5, 0), (1, 0, 0), (0, 0.5, 0.5), (0, 1, 0)])).max() < 1e-18
    assert np.abs(d - np.sqrt(np.array([9.0, 1.0, 2.0, 2.0, 11.0], dtype=pr.LD))).max() < 1e-18
    d_all, f_all = pr.nearest_distance(np.concatenate([tri, tri + (0, 0, 2.5)]), np.array([[0, 1, 2], [3, 4, 5]]), P)
    assert list(f_all) == [1, 0, 0, 0, 0] and abs(d_all[0] - 0.5) < 1e-18


@pytest.mark.parametrize("k", [3, 17])
def test_every_branch_against_the_solver(k):
    """Over the four designed triangles every one of the 25 return statements is taken at least 10 times, and at every point, for
    both values of `multi`, _point_triangle's (s, t) names the solver's closest point and its squared distance is the solver's --
    except in 4b / 4e with multi, where it is d * s + f / e * t + f on the UNCLAMPED s / t, as the vectorised reference codes it."""
    count = collections.Counter()
    for shape in pr.SHAPES:
        V, P = pr.designed_case(shape, k)
        args = pr.abcdef(V, P)
        labels = np.array([pr.branch(*row) for row in args])
        count.update(labels)
        q_ref, _, d_ref = pr.closest_point(V, P)
        for multi in (False, True):
            st = np.array([orc._point_triangle(*row, multi) for row in args])
            q = V[0] + st[:, :1] * (V[1] - V[0]) + st[:, 1:2] * (V[2] - V[0])
            assert np.abs(q - q_ref).max() <= TOL, (shape, multi)
            quirk = np.isin(labels, ("4b", "4e")) & multi
            assert np.abs(st[~quirk, 2] - (d_ref ** 2)[~quirk]).max() <= TOL, (shape, multi)
            a, b, c, d, e, f = args[quirk].T
            s_raw, t_raw = b * e - c * d, b * d - a * e
            coded = np.where(labels[quirk] == "4b", d * s_raw + f, e * t_raw + f)
            assert np.array_equal(st[quirk, 2], coded), (shape, multi)
            if multi and shape == "obtuse0":
                assert quirk.sum() >= 20 and np.abs(st[quirk, 2] - (d_ref ** 2)[quirk]).max() > 1e-3     # (the quirk is no rounding matter)
    print("return statements taken, k =", k, dict(sorted(count.items())))
    assert set(count) == set(pr.LABELS)
    assert min(count.values()) >= 10, count


def test_oracle_equals_the_reference_on_the_designed_inputs(fixture):
    """faces exactly, barycentric weights to 1e-9, on (a) the doubled triangles -- an exact tie, the first face is named -- and (b)
    the open corner and its twin"""
    fx, inputs = fixture
    for name, (V, faces, P) in inputs.items():
        fm, bary = orc.project_pc_to_triangles(V, faces, P)
        assert np.array_equal(fm, fx[name + "_face"]), name
        assert np.abs(bary - fx[name + "_bary"]).max() <= TOL, name
        if name.startswith("a_"):
            assert not fm.any()


@pytest.mark.parametrize("which", ["corner", "twin"])
def test_the_region4_quirk_decides_the_face(fixture, which):
    """On the open corner the reference names a face that is NOT the nearest at >= 5 points, each of them with the corner's face
    in 4b or 4e -- so the unclamped distances have to be reproduced, they are no dead code.  The triangles share no edge: no point's
    winner and runner-up are within 1e-9 (what the GPU test's margin rule relies on)."""
    fx, inputs = fixture
    V, faces, P = inputs["b_" + which]
    det = []
    fm, _ = orc.project_pc_to_triangles(V, faces, P, details=det)
    assert np.array_equal(fm, fx[f"b_{which}_face"])
    d_win = pr.face_distance(V, faces, P, fx[f"b_{which}_face"])
    d_min, f_min = pr.nearest_distance(V, faces, P)
    farther = np.where(d_win - d_min > TOL)[0]
    labels = collections.Counter(pr.branch(*det[i]["abcdef"][0]) for i in farther)
    print(which, ": the reference names the farther face at", len(farther), "of", len(P), "points;", dict(labels),
          "; by up to", float((d_win - d_min).max()))
    assert len(farther) >= 5 and set(labels) <= {"4b", "4e"}
    assert all(det[i]["multi"] and det[i]["cand"][0] == 0 for i in farther) and np.all(fm[farther] == 1) and np.all(f_min[farther] == 0)
    assert set(labels) == {"4b", "4e"}                         # both statements decide somewhere, on either mesh
    margin = np.array([np.diff(np.sort(x["dist"]))[0] if len(x["dist"]) > 1 else np.inf for x in det])
    assert (margin <= TOL).mean() == 0.0


def test_nan_candidates_are_passed_over():
    """a zero-area face (two corners on one vertex row) gives 0 * inf in region 0; the reference's argmin names that face and hands on
    NaN weights -- this project passes such a candidate over, oracle and device alike"""
    V, P = pr.designed_case("acute", 5)
    V = np.concatenate([V, V[:1]])
    faces = np.array([[0, 3, 2], [0, 1, 2], [3, 0, 0]])
    fm, bary = orc.project_pc_to_triangles(V, faces, P)
    fm1, bary1 = orc.project_pc_to_triangles(V, faces[1:2], P)
    assert np.all(fm == 1) and np.isfinite(bary).all()
    assert np.abs(bary - bary1).max() <= TOL                  # (4b / 4e: not on the acute triangle)
    fm0, bary0 = orc.project_pc_to_triangles(V, faces[[0, 2]], P[:7])       # nothing sound: face 0, its first corner
    assert not fm0.any() and np.array_equal(bary0, np.tile([1.0, 0.0, 0.0], (7, 1)))

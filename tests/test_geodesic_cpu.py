"""CPU: the heat-method contract (what dm_heat_geodesic_* compute) restated in NumPy and held against the reference's
TriMesh.get_geodesic(robust=False) (tests/golden/fx_geod.npz, tools/make_golden_geod.py); edges, t, Dijkstra, the fail-closed
robust routes and the map measures of pyFM.eval, none of which needs a GPU."""
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from densematcher_amd.pyFM.mesh import geometry
from densematcher_amd.pyFM.mesh import laplacian as lap
from densematcher_amd.pyFM.mesh.trimesh import TriMesh

from conftest import load_golden
from geod_restate import heat_restated


@pytest.fixture(scope="module")
def fx():
    return load_golden("fx_geod.npz")


@pytest.mark.parametrize("name", ["torus", "grid", "small"])
def test_restatement_matches_reference(fx, name):
    V, F, t = fx[name + "_V"], fx[name + "_F"].astype(np.int64), float(fx[name + "_t"])
    W, mass = lap.cotangent_laplacian(V, F)
    cols = fx[name + "_cols"] if name + "_cols" in fx else np.arange(len(V))
    D = heat_restated(V, F, W, mass, t, cols)
    ref = fx[name + "_D"]
    # (the obtuse mesh's systems are the worst conditioned: 2.6e-12 of the diameter between two LU pivot orders, measured)
    tol = 1e-11 if name == "small" else 1e-12
    assert np.abs(D - ref).max() <= tol * ref.max()


def test_restatement_geod_from(fx):
    V, F = fx["torus_V"], fx["torus_F"].astype(np.int64)
    W, mass = lap.cotangent_laplacian(V, F)
    D = heat_restated(V, F, W, mass, float(fx["torus_t"]), fx["torus_from_j"])
    assert np.abs(D - fx["torus_from"]).max() <= 1e-12 * fx["torus_from"].max()


@pytest.mark.parametrize("name", ["torus", "grid", "small"])
def test_heat_time_exact(fx, name):
    m = TriMesh(fx[name + "_V"], fx[name + "_F"])
    assert m._heat_time() == float(fx[name + "_t"])


def test_edges_exact(fx):
    m = TriMesh(fx["small_V"], fx["small_F"])
    np.testing.assert_array_equal(m.edges, fx["small_edges"])
    np.testing.assert_array_equal(geometry.edges_from_faces(fx["small_F"]), fx["small_edges"])


def test_dijkstra_exact(fx):
    D = geometry.geodesic_distmat_dijkstra(fx["small_V"], fx["small_F"])
    np.testing.assert_array_equal(D[fx["small_dijk_rows"]], fx["small_dijk"])
    m = TriMesh(fx["small_V"], fx["small_F"])
    np.testing.assert_array_equal(m.get_geodesic(dijkstra=True), D)


def test_robust_routes_fail_closed(fx, monkeypatch):
    monkeypatch.setitem(sys.modules, "potpourri3d", None)          # (import of it raises ImportError)
    V, F = fx["small_V"], fx["small_F"]
    with pytest.raises(ImportError, match="potpourri3d.*robust=False"):
        geometry.heat_geodmat_robust(V, F)
    m = TriMesh(V, F)
    with pytest.raises(ImportError, match="potpourri3d"):
        m.get_geodesic()
    with pytest.raises(ImportError, match="potpourri3d"):
        m.geod_from(0)
    with pytest.raises(ImportError, match="potpourri3d"):
        TriMesh.get_geodesic_many([m])


def test_argument_errors(fx):
    V, F = fx["small_V"], fx["small_F"]
    m = TriMesh(V, F)
    with pytest.raises(ValueError, match="No path specified"):
        m.get_geodesic(robust=False, save=True)
    W, mass = lap.cotangent_laplacian(V, F)
    with pytest.raises(TypeError, match="W"):
        geometry.heat_geodesic_from(0, V, F, geometry.compute_normals(V, F), sp.diags(mass))
    with pytest.raises(TypeError, match="solver"):
        geometry.heat_geodesic_from(0, V, F, None, sp.diags(mass), W=W, solver_heat=lambda b: b)


def test_eval_measures(fx):
    from densematcher_amd.pyFM import eval as ev
    D = fx["small_D"]
    n = D.shape[0]
    rng = np.random.default_rng(0)
    gt = np.arange(n)
    p2p = np.where(rng.random(n) < 0.3, rng.integers(0, n, n), gt)
    assert ev.accuracy(gt, gt, D) == 0.0
    acc, d = ev.accuracy(p2p, gt, D, return_all=True)
    np.testing.assert_array_equal(d, D[p2p, gt])
    assert acc == D[p2p, gt].mean()
    assert ev.accuracy(p2p, gt, D, sqrt_area=2.0) == (D[p2p, gt] / 2.0).mean()
    e = fx["small_edges"]
    Dd = geometry.geodesic_distmat_dijkstra(fx["small_V"], fx["small_F"])   # (the heat distance of a neighbour can be 0)
    assert ev.continuity(gt, Dd, Dd, e) == 1.0
    assert ev.continuity(p2p, D, Dd, e) == np.mean(D[p2p[e[:, 0]], p2p[e[:, 1]]] / Dd[e[:, 0], e[:, 1]])
    W, mass = lap.cotangent_laplacian(fx["small_V"], fx["small_F"])
    A = sp.diags(mass).tocsr()
    assert ev.coverage(gt, A) == pytest.approx(1.0, abs=1e-15)
    cov = mass[np.unique(p2p)].sum() / mass.sum()
    assert ev.coverage(p2p, A) == cov and ev.coverage(p2p, mass) == cov


def test_inconsistent_mass_fails_closed(fx):
    """A mass that is not one third of the adjacent face areas (the intrinsic Laplacian's) makes W phi = A div h inconsistent: the
    grounded answer then depends on the ground vertex (so the reference's depends on SuperLU's pivoting), and it is refused"""
    import warnings
    from densematcher_amd.engine import heat_geodesic_check
    V, F = fx["grid_V"], fx["grid_F"].astype(np.int64)
    W, mass = lap.cotangent_laplacian(V, F)
    heat_geodesic_check(V, F, mass)
    t = float(fx["grid_t"])
    src = np.arange(0, 1200, 150)
    D0, D1 = (heat_restated(V, F, W, mass, t, src, ground=g) for g in (0, 777))
    assert np.abs(D0 - D1).max() <= 1e-12 * D0.max()                   # consistent: the ground does not matter
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wr, Ar = lap.robust_mesh_laplacian(V, F, mollify_factor=1e-5)[:2]
    mr = np.asarray(Ar.diagonal())
    R0, R1 = (heat_restated(V, F, Wr, mr, t, src, ground=g) for g in (0, 777))
    assert np.abs(R0 - R1).max() > 0.1 * R0.max()                     # inconsistent: it does
    with pytest.raises(ValueError, match="one third"):
        heat_geodesic_check(V, F, mr)
    with pytest.raises(ValueError, match="one third"):
        geometry.heat_geodmat(V, F, None, sp.diags(mr), Wr, t=t)       # (refused before any device work)
    with pytest.raises(ValueError, match="one third"):
        geometry.heat_geodesic_from(0, V, F, None, sp.diags(mr), W=Wr, t=t)


def test_passed_geometry_must_be_the_meshes_own(fx):
    V, F = fx["small_V"], fx["small_F"].astype(np.int64)
    W, mass = lap.cotangent_laplacian(V, F)
    A = sp.diags(mass)
    area = 0.5 * np.linalg.norm(np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]), axis=1)
    va = np.zeros(len(V))
    np.add.at(va, F.ravel(), np.repeat(area / 3, 3))
    n = geometry.compute_normals(V, F)
    g = np.asarray([np.cross(n, e) / (2 * area[:, None]) for e in (V[F[:, 2]] - V[F[:, 1]], V[F[:, 0]] - V[F[:, 2]], V[F[:, 1]] - V[F[:, 0]])])
    geometry._check_inputs(V, F, n, A, area, va, g)                    # the mesh's own values pass
    geometry._check_inputs(V, F, -n, A, area, va, -g)                  # (orientation does not enter the result)
    for kw, match in (({"face_areas": area * 1.01}, "face_areas"), ({"vert_areas": mass * 1.2}, "vert_areas"),
                      ({"grads": g * 2}, "grads")):
        with pytest.raises(ValueError, match=match):
            geometry._check_inputs(V, F, None, A, **kw)
    with pytest.raises(ValueError, match="face_areas"):
        geometry.heat_geodmat(V, F, None, A, W, face_areas=area * 1.01)
    with pytest.raises(ValueError, match="diagonal"):
        geometry.heat_geodmat(V, F, None, A + sp.eye(len(V), k=1), W)
    m = TriMesh(V, F)
    m.W, m.A = W, (A + sp.eye(len(V), k=1)).tocsr()
    with pytest.raises(ValueError, match="diagonal"):
        m._geod_operands()


def test_source_indices_follow_numpy():
    np.testing.assert_array_equal(geometry._source_indices(-1, 10), [9])
    np.testing.assert_array_equal(geometry._source_indices([0, -10, 9], 10), [0, 0, 9])
    for bad in (10, -11, []):
        with pytest.raises(IndexError):
            geometry._source_indices(bad, 10)

"""GPU: heat-method geodesic distances (dm_heat_geodesic_factor / _solve) against the reference's get_geodesic(robust=False)
(tests/golden/fx_geod.npz) and against the contract's NumPy restatement; the bits of a source's distances do not depend on the
other sources or meshes of the call; the degenerate inputs fail closed."""
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden
from geod_restate import heat_restated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load_golden("fx_geod.npz")


@pytest.fixture(scope="module")
def meshes(fx):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    return {name: TriMesh(fx[name + "_V"], fx[name + "_F"]) for name in ("torus", "grid", "small")}


@pytest.fixture(scope="module")
def full(meshes):
    return {name: m.get_geodesic(robust=False) for name, m in meshes.items()}


@pytest.mark.parametrize("name", ["torus", "grid", "small"])
def test_all_pairs_match_reference(fx, full, name):
    D = full[name]
    ref = fx[name + "_D"]
    cols = fx[name + "_cols"] if name + "_cols" in fx else np.arange(D.shape[0])
    assert D.shape == (len(fx[name + "_V"]),) * 2
    assert np.abs(D[:, cols] - ref).max() <= 1e-9 * ref.max()


def test_geod_from_and_source_subsets_bitwise(fx, meshes, full):
    from densematcher_amd.engine import default_engine
    m, D = meshes["torus"], full["torus"]
    for j in (0, 5, 777, 2047):
        np.testing.assert_array_equal(m.geod_from(j, robust=False), D[:, j])
    ref = fx["torus_from"]
    assert np.abs(D[:, fx["torus_from_j"]] - ref).max() <= 1e-9 * ref.max()
    rng = np.random.default_rng(1)
    fac = m._geodesic_factors()
    for src in (rng.permutation(2048)[:37], np.array([2047, 3, 3, 1000, 64, 63]), rng.permutation(2048)):
        Ds = default_engine().heat_geodesic(fac, src)[0].cpu().numpy()
        np.testing.assert_array_equal(Ds, D[:, src])


def test_batch_of_different_sizes_bitwise(meshes, full):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    order = ["small", "torus", "grid"]
    Ds = TriMesh.get_geodesic_many([meshes[k] for k in order], robust=False)
    for k, D in zip(order, Ds):
        np.testing.assert_array_equal(D, full[k])


def test_sym(meshes, full):
    for name in ("small", "grid"):
        h = full[name] * 0.5
        np.testing.assert_array_equal(meshes[name].get_geodesic(robust=False, sym=True), h + h.T)


def test_robust_processed_mesh_fails_closed_and_uses_its_W(fx):
    from densematcher_amd.pyFM.mesh import laplacian as lap
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    m = TriMesh(fx["grid_V"], fx["grid_F"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.process(k=0, robust=True)                      # the restated robust Laplacian (the conftest opts in)
    # its A is not one third of the face areas: W phi = A div h is inconsistent, the answer would depend on the ground vertex
    with pytest.raises(ValueError, match="one third"):
        m.get_geodesic(robust=False)
    with pytest.raises(ValueError, match="one third"):
        m.geod_from(3, robust=False)
    # the same robust W with A = one third of the adjacent face areas is consistent: the mesh's own W is used, and the result
    # does not depend on where W is grounded
    W0, _ = lap.cotangent_laplacian(m.vertlist, m.facelist)
    assert abs(sp.csr_matrix(m.W) - W0).max() > 1e-6        # (it is not the cotangent W)
    V, F = m.vertlist, m.facelist
    area = 0.5 * np.linalg.norm(np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]), axis=1)
    va = np.zeros(len(V))
    np.add.at(va, F.ravel(), np.repeat(area / 3, 3))
    m.A = sp.diags(va).tocsr()
    src = np.arange(0, 1200, 40)
    Dall = m.get_geodesic(robust=False)
    np.testing.assert_array_equal(np.stack([m.geod_from(int(j), robust=False) for j in src[:3]], 1), Dall[:, src[:3]])
    for ground in (0, 777):
        ref = heat_restated(V, F, m.W, va, m._heat_time(), src, ground=ground)
        assert np.abs(Dall[:, src] - ref).max() <= 1e-9 * ref.max()


def test_negative_source_is_counted_from_the_end(fx, meshes, full):
    from densematcher_amd.pyFM.mesh import geometry
    m, D = meshes["small"], full["small"]
    n = D.shape[0]
    np.testing.assert_array_equal(m.geod_from(-1, robust=False), D[:, n - 1])
    Dj = geometry.heat_geodesic_from([-1, 2], m.vertlist, m.facelist, None, m.A, W=m.W, t=m._heat_time())
    np.testing.assert_array_equal(Dj, D[:, [n - 1, 2]])


def test_config5_torus_columns():
    from densematcher_amd import synth
    from densematcher_amd.engine import default_engine
    from densematcher_amd.pyFM.mesh import laplacian as lap
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    V, F = synth.torus_mesh(128, 64)
    m = TriMesh(V, F)
    W, mass = lap.cotangent_laplacian(V, F)
    t = m._heat_time()
    src = np.arange(0, 8192, 256)
    eng = default_engine()
    fac = eng.heat_geodesic_factor([(V, F, W, mass)], t)
    D = eng.heat_geodesic(fac, src)[0].cpu().numpy()
    ref = heat_restated(V, F, W, mass, t, src)
    assert np.abs(D - ref).max() <= 1e-9 * ref.max()
    del fac


def test_fail_closed(fx, monkeypatch):
    from densematcher_amd import synth
    from densematcher_amd.engine import default_engine
    from densematcher_amd.pyFM.mesh import geometry
    from densematcher_amd.pyFM.mesh import laplacian as lap
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    V, F = synth.torus_mesh(16, 8)
    two = TriMesh(np.concatenate([V, V + 5.0]), np.concatenate([F, F + len(V)]))
    with pytest.raises(ValueError, match="connected components"):
        two.get_geodesic(robust=False)
    W, mass = lap.cotangent_laplacian(V, F)
    Fz = np.concatenate([F, [[0, 1, 0]]])                 # a face of zero area
    with pytest.raises(ValueError, match="zero area"):
        geometry.heat_geodmat(V, Fz, None, sp.diags(mass), W, t=1e-3)
    V1 = np.concatenate([V, [[3.0, 3.0, 3.0]]])           # a vertex that no face references
    W1 = sp.block_diag([W, sp.csr_matrix((1, 1))]).tocsr()
    with pytest.raises(ValueError, match="connected components"):
        default_engine().heat_geodesic_factor([(V1, F, W1, np.append(mass, 1.0))], 1e-3)
    monkeypatch.setitem(sys.modules, "potpourri3d", None)
    with pytest.raises(ImportError, match="potpourri3d"):
        TriMesh(V, F).get_geodesic(robust=True)

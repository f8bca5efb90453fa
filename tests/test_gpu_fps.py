"""GPU: farthest-point sampling on the device (dm_fps_euclid / dm_fps_heat) against the reference's own index lists
(tests/golden/fx_fps.npz, tools/make_golden_fps.py) and against the reference's greedy loop restated in NumPy over distance
matrices; batches equal single calls; the default extract_fps() keeps its Dijkstra samples and its warning."""
import warnings

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FPS_MESHES = (("cfg1_verts1", "cfg1", "verts1"), ("cfg1_verts2", "cfg1", "verts2"), ("torus_V", "geod", "torus_V"),
              ("grid_V", "geod", "grid_V"), ("small_V", "geod", "small_V"))


@pytest.fixture(scope="module")
def fx():
    return {"cfg1": load_golden("fx_cfg1.npz"), "geod": load_golden("fx_geod.npz"), "fps": load_golden("fx_fps.npz")}


@pytest.fixture(scope="module")
def meshes(fx):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    g = fx["geod"]
    return {name: TriMesh(g[name + "_V"], g[name + "_F"]) for name in ("torus", "grid", "small")}


def greedy(D, size, start):
    """geometry.py:839-848 with d(i) = D[i]"""
    inds = [int(start)]
    d = D[inds[0]]
    gap = np.inf
    for _ in range(size - 1):
        top = np.sort(d)[-2:]
        gap = min(gap, top[1] - top[0])
        inds.append(int(np.argmax(d)))
        d = np.minimum(d, D[inds[-1]])
    return np.asarray(inds), gap


def euclid_greedy(V, size, start):
    V = np.asarray(V, np.float64)
    inds = [int(start)]
    d = np.linalg.norm(V - V[inds[0]], axis=1)
    ties = 0
    for _ in range(size - 1):
        ties += int(np.count_nonzero(d == d.max()) > 1)
        inds.append(int(np.argmax(d)))
        d = np.minimum(d, np.linalg.norm(V - V[inds[-1]], axis=1))
    return np.asarray(inds), ties


def test_euclidean_equals_the_reference_lists(fx):
    """index for index, from the recorded start, through MatchEngine.fps and through TriMesh.extract_fps(geodesic=False, start=);
    the first mesh has steps with more than one vertex at the maximum (the lowest index must win)"""
    from densematcher_amd.engine import default_engine
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    eng = default_engine()
    _, ties = euclid_greedy(fx["cfg1"]["verts1"], 200, fx["fps"]["cfg1_verts1"][0])
    assert ties > 0
    for key, src, vk in FPS_MESHES:
        V = np.asarray(fx[src][vk], np.float64)
        ref = fx["fps"][key]
        got = eng.fps(V[None], len(ref), int(ref[0]))[0].cpu().numpy()
        np.testing.assert_array_equal(got, ref, err_msg=key)
        faces = fx[src]["faces" + vk[-1]] if src == "cfg1" else fx[src][vk[:-2] + "_F"]
        m = TriMesh(V, faces)
        s = m.extract_fps(len(ref), geodesic=False, start=int(ref[0]))
        assert s.dtype == np.int64
        np.testing.assert_array_equal(s, ref, err_msg=key)


def test_euclidean_padded_batch_and_repeats(fx):
    """the five meshes padded to 2048 vertices in one call: each mesh its own list; size > n_verts repeats vertex 0 like np.argmax"""
    from densematcher_amd.engine import default_engine
    eng = default_engine()
    Vs = [np.asarray(fx[src][vk], np.float64) for _, src, vk in FPS_MESHES]
    refs = [fx["fps"][key] for key, _, _ in FPS_MESHES]
    batch = np.full((5, 2048, 3), 1e6)                         # far-away padding: it must never be chosen
    for b, V in enumerate(Vs):
        batch[b, :len(V)] = V
    out = eng.fps(batch, 200, [int(r[0]) for r in refs], n_verts=[len(V) for V in Vs]).cpu().numpy()
    for b, (V, ref) in enumerate(zip(Vs, refs)):
        np.testing.assert_array_equal(out[b, :len(ref)], ref)
        np.testing.assert_array_equal(out[b], euclid_greedy(V, 200, ref[0])[0])
    small = Vs[4]
    got = eng.fps(small[None], 170, 3)[0].cpu().numpy()
    np.testing.assert_array_equal(got, euclid_greedy(small, 170, 3)[0])
    assert len(set(got[:160].tolist())) == 160 and np.all(got[160:] == 0)


def test_heat_small_equals_greedy_on_the_reference_matrix(fx, meshes):
    """d(i) = geod_from(i) = COLUMN i of the reference's matrix (which is not symmetric); both routes"""
    from densematcher_amd.engine import default_engine
    eng = default_engine()
    D = fx["geod"]["small_D"]
    assert np.abs(D - D.T).max() > 0.1
    m = meshes["small"]
    for start in (0, 17, 159):
        ref, gap = greedy(np.ascontiguousarray(D.T), 80, start)
        print(f"small start {start}: smallest gap between the top two candidates {gap / D.max():.3e} max D")
        assert gap > 1e-7 * D.max()                             # (the device distances agree with D to 1e-9 max D)
        try:
            for route in (1, 2):
                eng.set_option("fps_heat_route", route)
                got = m.extract_fps(80, geodesic=True, robust=False, start=start)
                np.testing.assert_array_equal(got, ref, err_msg=f"start {start} route {route}")
        finally:
            eng.set_option("fps_heat_route", 0)


@pytest.mark.parametrize("name", ["torus", "grid"])
def test_heat_equals_greedy_on_get_geodesic(meshes, name):
    from densematcher_amd.engine import default_engine
    eng = default_engine()
    m = meshes[name]
    D = m.get_geodesic(robust=False)
    start = 11
    ref, _ = greedy(np.ascontiguousarray(D.T), 256, start)
    assert len(set(ref.tolist())) == 256
    try:
        eng.set_option("fps_heat_route", 1)
        a = m.extract_fps(256, geodesic=True, robust=False, start=start)
        eng.set_option("fps_heat_route", 2)
        b = eng.fps_heat(m._geodesic_factors(), 256, start)[0].cpu().numpy()
    finally:
        eng.set_option("fps_heat_route", 0)
    np.testing.assert_array_equal(a, ref)
    np.testing.assert_array_equal(b, ref)
    np.testing.assert_array_equal(m.extract_fps(256, geodesic=True, robust=False, start=start), ref)


def test_extract_fps_many_equals_single_calls(meshes):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    order = ["small", "torus", "grid"]
    ms = [meshes[k] for k in order]
    starts = [5, 1000, 77]
    for kw in (dict(geodesic=False), dict(geodesic=True, robust=False)):
        many = TriMesh.extract_fps_many(ms, 64, starts=starts, **kw)
        for m, s, got in zip(ms, starts, many):
            np.testing.assert_array_equal(got, m.extract_fps(64, start=s, **kw))
    a = TriMesh.extract_fps_many(ms, 16, geodesic=False, rng=np.random.default_rng(3))
    rng = np.random.default_rng(3)
    for m, got in zip(ms, a):
        np.testing.assert_array_equal(got, m.extract_fps(16, geodesic=False, rng=rng))


def test_default_extract_fps_keeps_dijkstra_and_warns(meshes):
    """extract_fps() with default arguments: today's samples (shortest paths along the edges), restated here, and the warning"""
    import scipy.sparse as sparse
    import scipy.sparse.csgraph as csgraph
    m = meshes["grid"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = m.extract_fps(40, rng=np.random.default_rng(6))
    assert any("potpourri3d" in str(w.message) for w in caught)
    n, f, V = m.n_vertices, m.facelist, m.vertlist
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    w = np.linalg.norm(V[e[:, 0]] - V[e[:, 1]], axis=1)
    G = sparse.coo_matrix((w, (e[:, 0], e[:, 1])), shape=(n, n)).tocsr()
    G = G.maximum(G.T)
    inds = [int(np.random.default_rng(6).integers(n))]
    d = csgraph.dijkstra(G, directed=False, indices=inds[0])
    for _ in range(39):
        inds.append(int(np.argmax(d)))
        d = np.minimum(d, csgraph.dijkstra(G, directed=False, indices=inds[-1]))
    np.testing.assert_array_equal(got, np.asarray(inds))


def test_bad_starts_raise(fx, meshes):
    from densematcher_amd.engine import default_engine
    eng = default_engine()
    V = np.asarray(fx["geod"]["small_V"], np.float64)
    with pytest.raises(ValueError):
        eng.fps(V[None], 8, 160)
    with pytest.raises(ValueError):
        meshes["small"].extract_fps(8, geodesic=True, robust=False, start=-1)
    with pytest.raises(ValueError):
        eng.fps_heat(meshes["small"]._geodesic_factors(), 8, 160)

"""GPU: shortest paths along mesh edges on the device (dm_graph_geodesic / dm_fps_graph) against scipy.sparse.csgraph.dijkstra at test
time -- the reference's route verbatim (geometry.py:524-556) -- with assert_array_equal throughout: all pairs, explicit sources,
padded batches, the default extract_fps / extract_fps_many against the host loop, a constructed mesh with two components, an
unreferenced vertex and a zero-length edge, the 16384-vertex limit, the routing option and the errors."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

import graphgeod_restate as gr
from conftest import load_golden

pytestmark = pytest.mark.gpu

NAMES = ("small", "grid", "torus")


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    e = default_engine()
    yield e
    e.reset_options()
    e.profile_kernel(None)


@pytest.fixture(scope="module")
def meshes():
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    g = load_golden("fx_geod.npz")
    out = {name: TriMesh(g[name + "_V"], g[name + "_F"]) for name in NAMES}
    out["constructed"] = TriMesh(*gr.constructed_mesh())
    return out


@pytest.fixture(scope="module")
def graphs(meshes):
    from densematcher_amd.pyFM.mesh import geometry
    return {name: geometry.edge_graph(m.vertlist, m.facelist) for name, m in meshes.items()}


@pytest.fixture(scope="module")
def scipy_all_pairs(graphs):
    """csgraph.dijkstra of every mesh, computed once and shared (read-only)"""
    out = {name: csgraph.dijkstra(G) for name, G in graphs.items()}
    for D in out.values():
        D.setflags(write=False)
    return out


def quiet_fps(mesh, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mesh.extract_fps(*a, **k)


@pytest.mark.parametrize("name", NAMES + ("constructed",))
def test_all_pairs_equal_scipy(eng, meshes, graphs, scipy_all_pairs, name):
    ref = scipy_all_pairs[name]
    D = meshes[name].get_geodesic(dijkstra=True)
    assert isinstance(D, np.ndarray) and D.shape == ref.shape
    np.testing.assert_array_equal(D, ref)
    np.testing.assert_array_equal(eng.graph_geodesic([graphs[name]])[0].cpu().numpy(), ref)
    if name == "constructed":
        assert np.isinf(ref).any() and ref[40, 41] == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_explicit_sources_equal_the_all_pairs_rows(eng, graphs, scipy_all_pairs, name):
    n = graphs[name].shape[0]
    src = [0, n - 1, n // 2, 7, 7, 63, 64]
    np.testing.assert_array_equal(eng.graph_geodesic([graphs[name]], src)[0].cpu().numpy(), scipy_all_pairs[name][src])
    # one list per mesh, -1 = none: a row of zeros
    got = eng.graph_geodesic([graphs[name]], [[5, -1, 3]])[0].cpu().numpy()
    np.testing.assert_array_equal(got[[0, 2]], scipy_all_pairs[name][[5, 3]])
    assert not got[1].any()


def test_a_padded_batch_gives_each_mesh_its_own_bits(eng, meshes, graphs, scipy_all_pairs):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    order = ("grid", "constructed", "torus", "small")
    D = eng.graph_geodesic([graphs[k] for k in order]).cpu().numpy()
    many = TriMesh.get_geodesic_many([meshes[k] for k in order], dijkstra=True)
    for b, k in enumerate(order):
        n = graphs[k].shape[0]
        np.testing.assert_array_equal(D[b, :n, :n], scipy_all_pairs[k])
        assert not D[b, n:].any() and not D[b, :, n:].any()                  # padding: zeros
        np.testing.assert_array_equal(many[b], scipy_all_pairs[k])
    src = [[3, 100, -1], [300, 156, 0], [2047, 5, 1], [-1, 159, 2]]         # one list per mesh
    got = eng.graph_geodesic([graphs[k] for k in order], src).cpu().numpy()
    for b, k in enumerate(order):
        n = graphs[k].shape[0]
        for q, s in enumerate(src[b]):
            np.testing.assert_array_equal(got[b, q, :n], scipy_all_pairs[k][s] if s >= 0 else np.zeros(n))


@pytest.mark.parametrize("name", NAMES)
def test_default_extract_fps_equals_the_host_loop(meshes, name):
    m = meshes[name]
    G = gr.fps_graph_of(m.vertlist, m.facelist)
    for start in (0, m.n_vertices - 1, m.n_vertices // 3):
        got = quiet_fps(m, 64, start=start)
        assert got.dtype == np.int64 and got.shape == (64,)
        np.testing.assert_array_equal(got, gr.host_fps(G, 64, start))


def test_extract_fps_many_equals_the_single_calls(eng, meshes):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    order = ("torus", "small", "constructed", "grid")
    starts = [17, 159, 200, 0]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = TriMesh.extract_fps_many([meshes[k] for k in order], 64, starts=starts)
    assert sum("potpourri3d" in str(w.message) for w in caught) == len(order)
    for k, s, g in zip(order, starts, got):
        np.testing.assert_array_equal(g, quiet_fps(meshes[k], 64, start=s))
        np.testing.assert_array_equal(g, gr.host_fps(gr.fps_graph_of(meshes[k].vertlist, meshes[k].facelist), 64, s))


def test_constructed_mesh_sampling(eng, meshes):
    """two components + an unreferenced vertex: +inf is a maximum and the lowest index among them is taken; size > n_verts repeats
    indices as the host loop does; the zero-length edge 40 -- 41"""
    m = meshes["constructed"]
    n = m.n_vertices
    G = gr.fps_graph_of(m.vertlist, m.facelist)
    got = quiet_fps(m, 12, start=5)
    assert got[1] == 156 and got[2] == 157
    for start, size in ((5, n + 9), (300, 40), (156, 40), (40, 40)):
        np.testing.assert_array_equal(quiet_fps(m, size, start=start), gr.host_fps(G, size, start))
    # the engine on a graph that stores the zero-length edge (the reference's all-pairs graph does)
    from densematcher_amd.pyFM.mesh import geometry
    E = geometry.edge_graph(m.vertlist, m.facelist)
    np.testing.assert_array_equal(eng.fps_graph([E], n + 9, 41)[0].cpu().numpy(), gr.host_fps(E, n + 9, 41))


def test_the_largest_mesh(eng):
    """128 x 128 torus, 16384 vertices: the running minimum fills 128 KiB of LDS; 48 samples against 48 host Dijkstra runs, and a
    few single sources (the sixteen-wave instance of the distance kernel)"""
    from densematcher_amd import synth
    V, F = synth.torus_mesh(128, 128, perturb=0.05, seed=3)[:2]
    assert len(V) == 16384
    G = gr.fps_graph_of(V, F)
    np.testing.assert_array_equal(eng.fps_graph([G], 48, 16383)[0].cpu().numpy(), gr.host_fps(G, 48, 16383))
    src = [0, 16383, 8191]
    np.testing.assert_array_equal(eng.graph_geodesic([G], src)[0].cpu().numpy(), csgraph.dijkstra(G, indices=src))


def test_more_than_4096_vertices_padded_with_a_small_mesh(eng, graphs):
    """a 75 x 67 torus (5025 vertices: sixteen waves, five vertices per thread, the last ones idle) in a batch with the smallest mesh"""
    from densematcher_amd import synth
    V, F = synth.torus_mesh(75, 67, perturb=0.05, seed=4)[:2]
    G = gr.fps_graph_of(V, F)
    src = [[0, 5024, 1234], [159, 0, -1]]
    got = eng.graph_geodesic([G, graphs["small"]], src).cpu().numpy()
    np.testing.assert_array_equal(got[0], csgraph.dijkstra(G, indices=src[0]))
    np.testing.assert_array_equal(got[1, :2, :160], csgraph.dijkstra(graphs["small"], indices=src[1][:2]))
    assert not got[1, 2].any() and not got[1, :, 160:].any()
    out = eng.fps_graph([G, graphs["small"]], 40, [5024, 3]).cpu().numpy()
    np.testing.assert_array_equal(out[0], gr.host_fps(G, 40, 5024))
    np.testing.assert_array_equal(out[1], gr.host_fps(graphs["small"], 40, 3))


# ---------------------------------------------------------------------------------------------------------------- routing
def test_the_option_switches_the_route_and_not_the_bits(eng, meshes):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    res = {}
    try:
        for mode in (0, 1):
            eng.set_option("graph_geod_device", mode)
            eng.profile_kernel("*")
            res[mode] = (quiet_fps(meshes["grid"], 40, start=11), meshes["small"].get_geodesic(dijkstra=True),
                         TriMesh.get_geodesic_many([meshes["small"], meshes["constructed"]], dijkstra=True))
            names = set(eng.profile_report())
            eng.profile_kernel(None)
            assert ({"fps_graph", "graph_geodesic"} <= names) == (mode == 1) and (mode == 1 or not names), names
    finally:
        eng.set_option("graph_geod_device", 1)
        eng.profile_kernel(None)
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    for a, b in zip(res[0][2], res[1][2]):
        np.testing.assert_array_equal(a, b)


def mesh_with_spectrum(fx, which):
    from densematcher_amd.pyFM.mesh import TriMesh
    m = TriMesh(fx[f"verts{which}"], fx[f"faces{which}"])
    m.A = sp.diags(fx[f"a{which}"].astype(np.float64)).tocsr()
    m.W = sp.identity(m.n_vertices).tocsr()
    m.eigenvalues = fx[f"lam{which}"].copy()
    m.eigenvectors = fx[f"Phi{which}"].astype(np.float64)
    return m


def test_the_default_routes_never_call_scipys_dijkstra(eng, meshes, fx_cfg1, monkeypatch):
    from densematcher_amd.pyFM import refine
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh

    def refuse(*a, **k):
        raise AssertionError("csgraph.dijkstra called on the host")
    assert eng.get_option("graph_geod_device") == 1
    want_fps = gr.host_fps(gr.fps_graph_of(meshes["small"].vertlist, meshes["small"].facelist), 20, 4)
    monkeypatch.setattr(csgraph, "dijkstra", refuse)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = meshes["grid"].extract_fps(30, rng=np.random.default_rng(2))
        assert got.shape == (30,) and len(set(got.tolist())) == 30
        np.testing.assert_array_equal(meshes["small"].extract_fps(20, start=4), want_fps)
        many = TriMesh.extract_fps_many([meshes["small"], meshes["grid"]], 20, starts=[4, 9])
        np.testing.assert_array_equal(many[0], want_fps)
        assert meshes["small"].get_geodesic(dijkstra=True).shape == (160, 160)
        m1, m2 = mesh_with_spectrum(fx_cfg1, 1), mesh_with_spectrum(fx_cfg1, 2)
        eng.profile_kernel("*")
        C0 = np.ascontiguousarray(fx_cfg1["C20"][:8, :8])                    # 8 -> 14 functions on 32 samples
        C, p = refine.mesh_zoomout_refine(C0, m1, m2, nit=3, step=2, subsample=32, return_p2p=True)
        rep = eng.profile_report()
        eng.profile_kernel(None)
    assert C.shape == (14, 14) and np.isfinite(C).all() and p.shape == (m2.n_vertices,)
    assert rep["fps_graph"][0] == 1, rep                                     # both meshes sampled by one launch


def test_sampling_is_one_launch_per_call_whatever_the_batch(eng, meshes):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    for batch in (["grid"], ["grid", "small", "torus", "constructed", "grid"]):
        eng.profile_kernel("*")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            TriMesh.extract_fps_many([meshes[k] for k in batch], 64, starts=[1] * len(batch))
        rep = eng.profile_report()
        eng.profile_kernel(None)
        assert rep == {"fps_graph": (1, rep["fps_graph"][1])}, rep


# ---------------------------------------------------------------------------------------------------------------- errors
def test_bad_sources_and_starts_raise(eng, meshes, graphs):
    G = graphs["small"]
    for bad in (160, -2):
        with pytest.raises(ValueError, match="source"):
            eng.graph_geodesic([G], [0, bad])
    for bad in (160, -1):
        with pytest.raises(ValueError, match="start"):
            eng.fps_graph([G], 8, bad)
        with pytest.raises(ValueError, match="start"):
            meshes["small"].extract_fps(8, start=bad)
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    with pytest.raises(ValueError, match="start"):
        TriMesh.extract_fps_many([meshes["small"], meshes["grid"]], 8, starts=[0, 1200])
    with pytest.raises(ValueError, match="sources must be"):
        eng.graph_geodesic([G, G], [[0, 1]])


def test_bad_graphs_are_refused(eng, graphs):
    from densematcher_amd.engine import GraphTooWide
    G = sp.csr_matrix(graphs["small"]).copy()
    G.data[7] = -G.data[7]
    with pytest.raises(ValueError, match="negative or NaN"):
        eng.graph_geodesic([graphs["small"], G], [0, 1])
    with pytest.raises(ValueError, match="mesh 0.*negative or NaN"):
        eng.fps_graph([G], 8, 0)
    G.data[7] = np.nan
    with pytest.raises(ValueError, match="negative or NaN"):
        eng.graph_geodesic([G])
    # a hub vertex above the ELL width cap: GraphTooWide from the engine, the host route (same bits) from the mesh layer
    n = 80
    star = sp.coo_matrix((np.arange(1.0, n), (np.zeros(n - 1, int), np.arange(1, n))), shape=(n, n)).tocsr()
    star = star.maximum(star.T)
    with pytest.raises(GraphTooWide):
        eng.graph_geodesic([star])
    with pytest.raises(GraphTooWide):
        eng.fps_graph([star], 4, 0)
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    ang = 2 * np.pi * np.arange(n - 1) / (n - 1)
    V = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)])
    F = np.stack([np.zeros(n - 1, int), 1 + np.arange(n - 1), 1 + (np.arange(n - 1) + 1) % (n - 1)], 1)
    fan = TriMesh(V, F)                                                      # vertex 0 has 79 neighbours
    eng.profile_kernel("*")
    D = fan.get_geodesic(dijkstra=True)
    got = quiet_fps(fan, 10, start=3)
    names = set(eng.profile_report())
    eng.profile_kernel(None)
    assert not names, names
    from densematcher_amd.pyFM.mesh import geometry
    np.testing.assert_array_equal(D, csgraph.dijkstra(geometry.edge_graph(V, F)))
    np.testing.assert_array_equal(got, gr.host_fps(gr.fps_graph_of(V, F), 10, 3))

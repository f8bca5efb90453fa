"""CPU: the argument behind dm_graph_geodesic / dm_fps_graph ("Edge-graph shortest paths"), independent of the
device code: relaxing every edge until a sweep changes nothing ends at the BITS of scipy.sparse.csgraph.dijkstra, and sampling that
relaxes from the running minimum takes the host loop's vertices.  Also pins what the GPU tests assume of SciPy: a stored weight 0 is
an edge, an unreachable vertex is at +inf."""
import numpy as np
import pytest
import scipy.sparse.csgraph as csgraph

import graphgeod_restate as gr
from conftest import load_golden
from densematcher_amd.pyFM.mesh import geometry


@pytest.fixture(scope="module")
def meshes():
    g = load_golden("fx_geod.npz")
    out = {name: (g[name + "_V"], g[name + "_F"]) for name in ("small", "grid")}
    out["constructed"] = gr.constructed_mesh()
    return out


@pytest.mark.parametrize("name", ["small", "grid", "constructed"])
def test_pull_sweeps_end_at_dijkstras_bits(meshes, name):
    V, F = meshes[name]
    for G in (geometry.edge_graph(V, F), gr.fps_graph_of(V, F)):
        n = G.shape[0]
        rows = np.arange(n) if n <= 400 else np.random.default_rng(1).choice(n, 48, replace=False)
        cols, w = gr.ell_of(G)
        ref = csgraph.dijkstra(G, indices=rows)
        for r, s in enumerate(rows):
            m = np.full(n, np.inf)
            m[s] = 0.0
            d, sweeps = gr.relax(m, cols, w)
            np.testing.assert_array_equal(d, ref[r])
            assert sweeps <= n + 1


@pytest.mark.parametrize("name", ["small", "grid", "constructed"])
def test_warm_started_sampling_takes_the_host_loops_vertices(meshes, name):
    V, F = meshes[name]
    G = gr.fps_graph_of(V, F)
    n = G.shape[0]
    size = 64 if name != "constructed" else n + 9                           # (size > n: the indices repeat)
    for start in (0, n - 1):
        inds, m, sweeps = gr.warm_fps(G, size, start)
        np.testing.assert_array_equal(inds, gr.host_fps(G, size, start))
        np.testing.assert_array_equal(m, csgraph.dijkstra(G, directed=False, indices=inds).min(axis=0))
        assert max(sweeps[8:]) <= max(sweeps[:2])                            # later samples only move their own region


def test_scipy_reads_a_stored_zero_as_an_edge_and_inf_for_no_path(meshes):
    V, F = meshes["constructed"]
    G = geometry.edge_graph(V, F)
    assert G[40, 41] == 0.0 and G[41, 40] == 0.0 and 41 in G[:, 40].indices   # stored, of weight exactly 0
    D = csgraph.dijkstra(G)
    assert D[40, 41] == 0.0 and D[41, 40] == 0.0
    H = G.copy()
    H.eliminate_zeros()
    assert csgraph.dijkstra(H, indices=40)[41] > 0.0                         # without the stored zero the way round is longer
    assert np.isinf(D[156, :156]).all() and np.isinf(D[:156, 157:]).all() and D[156, 156] == 0.0
    assert np.isfinite(D[:156, :156]).all() and np.isfinite(D[157:, 157:]).all()
    # the sampler's first arg-max from the first sheet is the lowest index at +inf
    assert gr.host_fps(gr.fps_graph_of(V, F), 3, 5).tolist()[1:] == [156, 157]


def test_geodesic_distmat_dijkstra_many(meshes):
    """the batch entry on whichever route this process takes (without a GPU: the host loop); SciPy's bits either way"""
    got = geometry.geodesic_distmat_dijkstra_many([meshes["small"], meshes["constructed"]])
    for D, (V, F) in zip(got, (meshes["small"], meshes["constructed"])):
        np.testing.assert_array_equal(D, csgraph.dijkstra(geometry.edge_graph(V, F)))

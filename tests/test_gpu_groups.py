"""GPU: many ragged assignments gathered from one matrix (dm_lsa_gather, MatchEngine.lsa_gather / groups_dmtx, densematcher_amd.utils,
TriMesh.get_groups_dmtx_many) against scipy.optimize.linear_sum_assignment at test time.

Assignments: assert_array_equal against SciPy.  Means: |got - ref| <= n 2^-52 |ref| with n = min(nr, nc) -- not a measured number:
two summation orders of the same n terms of one sign err by at most (n - 1) 2^-53 of the sum each, plus one rounding each for the
division (NumPy's mean adds pairwise, the kernel in row order, so bit equality is not asked)."""
import numpy as np
import pytest
import scipy.sparse.csgraph as csgraph
from scipy.optimize import linear_sum_assignment

import graphgeod_restate as ggr
import groups_restate as gr
from conftest import load_golden

pytestmark = pytest.mark.gpu

ONE_WAVE_CAP = 1024                      # columns of the widest one-wave search (dm_lsa_gather.hip: 64 LG_MAX_CPL)
CPL_BOUNDS = (64, 128, 256, 512, 1024)   # the longer side at which the search takes its next columns-per-lane body
PER_WORKGROUP = 4                        # problems per workgroup (LG_WPB)


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    e = default_engine()
    yield e
    e.reset_options()


@pytest.fixture(scope="module")
def geod():
    return load_golden("fx_geod.npz")


@pytest.fixture(scope="module")
def dijkstra_mats(geod):
    """csgraph.dijkstra on the edge graphs of the fixture's meshes and of the constructed two-component mesh: computed once, read-only"""
    from densematcher_amd.pyFM.mesh import geometry
    out = {}
    for name in ("grid", "torus"):
        out[name] = csgraph.dijkstra(geometry.edge_graph(geod[name + "_V"], geod[name + "_F"]))
    out["constructed"] = csgraph.dijkstra(geometry.edge_graph(*ggr.constructed_mesh()))
    for D in out.values():
        D.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def random_D():
    D = np.random.default_rng(5).uniform(0.0, 1.0, (1100, 1100))
    D.setflags(write=False)
    return D


def scipy_problem(block, maximize=False):
    r, c = linear_sum_assignment(block, maximize=maximize)
    col_of_row = np.full(block.shape[0], -1, np.int32)
    col_of_row[r] = c
    return col_of_row, block[r, c].mean()


def check(eng, D, rows, cols, mesh=None, maximize=False, Dd=None):
    """every problem of one lsa_gather call against SciPy; returns the means"""
    means, assign = eng.lsa_gather(D if Dd is None else Dd, rows, cols, mesh=mesh, maximize=maximize, return_assignment=True)
    assert means.shape == (len(rows),) and means.dtype == np.float64 and len(assign) == len(rows)
    for p, (r, c) in enumerate(zip(rows, cols)):
        Db = D if D.ndim == 2 else D[0 if mesh is None else mesh[p]]
        ref_assign, ref_mean = scipy_problem(Db[np.ix_(r, c)], maximize)
        np.testing.assert_array_equal(assign[p], ref_assign, err_msg=f"problem {p}: {len(r)} x {len(c)}")
        bound = min(len(r), len(c)) * 2.0 ** -52 * abs(ref_mean)
        print(f"problem {p}: {len(r)} x {len(c)}: |mean - ref| = {abs(means[p] - ref_mean):.3e}, bound {bound:.3e}")
        assert abs(means[p] - ref_mean) <= bound, (p, len(r), len(c), means[p], ref_mean)
    return means


def lists(rng, n, sizes):
    return [rng.permutation(n)[:s].tolist() for s in sizes]


def test_small_shapes_every_combination(eng, random_D):
    """nr, nc in {1, 2, 63, 64, 65}: square, wide and tall (the transposed, staged route), 25 problems in one call"""
    rng = np.random.default_rng(1)
    sizes = (1, 2, 63, 64, 65)
    rows = lists(rng, 1100, [a for a in sizes for _ in sizes])
    cols = lists(rng, 1100, [b for _ in sizes for b in sizes])
    check(eng, random_D, rows, cols)


@pytest.mark.parametrize("bound", CPL_BOUNDS)
def test_each_side_of_a_columns_per_lane_boundary(eng, random_D, bound):
    """the longer side at a boundary and one past it (past the last: the workgroup-per-matrix route), wide and tall"""
    rng = np.random.default_rng(bound)
    short = 5
    rows = lists(rng, 1100, [short, short, bound, bound + 1])
    cols = lists(rng, 1100, [bound, bound + 1, short, short])
    check(eng, random_D, rows, cols)


def test_just_past_the_one_wave_cap(eng, random_D):
    """the wide route on more than a sliver: 40 x 1030, its transpose, and a square 1025 x 1025 block, next to one-wave problems"""
    rng = np.random.default_rng(7)
    n = ONE_WAVE_CAP + 6
    rows = lists(rng, 1100, [40, n, 30, ONE_WAVE_CAP + 1])
    cols = lists(rng, 1100, [n, 40, 30, ONE_WAVE_CAP + 1])
    check(eng, random_D, rows, cols)


@pytest.mark.parametrize("P", [1, 3, 5, 2 * PER_WORKGROUP + 3])
def test_problem_counts(eng, random_D, P):
    rng = np.random.default_rng(100 + P)
    rows = lists(rng, 1100, rng.integers(1, 150, P))
    cols = lists(rng, 1100, rng.integers(1, 150, P))
    check(eng, random_D, rows, cols)


def test_no_problem_is_legal(eng, random_D):
    means, assign = eng.lsa_gather(random_D[:64, :64], [], [], return_assignment=True)
    assert means.shape == (0,) and assign == []


def test_ties_integer_fixture(eng):
    g = load_golden("fx_groups.npz")
    groups = gr.unpack_groups(g["b_flat"], g["b_off"])
    pairs = [(i, j) for i in range(len(groups)) for j in range(len(groups)) if i != j]
    check(eng, g["b_D"], [groups[i] for i, _ in pairs], [groups[j] for _, j in pairs])
    got = eng.groups_dmtx(g["b_D"], groups)
    assert np.all(np.abs(got - g["b_dmtx"]) <= gr.mean_bound(groups, g["b_dmtx"]))


def test_ties_grid_dijkstra_blocks(eng, dijkstra_mats):
    """the grid's shortest-path matrix: hundreds of thousands of tied entries, not bit-symmetric"""
    D = dijkstra_mats["grid"]
    rng = np.random.default_rng(3)
    sizes_r, sizes_c = (20, 200, 64, 131, 90, 1, 77, 150), (200, 20, 64, 45, 90, 33, 260, 150)
    check(eng, D, lists(rng, 1200, sizes_r), lists(rng, 1200, sizes_c))
    # contiguous index ranges: neighbouring vertices, where the ties are densest
    check(eng, D, [list(range(0, 90)), list(range(300, 420))], [list(range(600, 720)), list(range(35, 115))])


def test_infinities_and_errors(eng, dijkstra_mats):
    D = dijkstra_mats["constructed"]
    assert np.isinf(D).sum() == 45528
    A, Bs = (3, 50, 120), (160, 250)                                              # vertices of the first / the second sheet
    rows, cols = list(A) + list(Bs), [7, 60, 100, 140] + [170, 200, 290]
    assert np.isinf(D[np.ix_(rows, cols)]).sum() == 17
    check(eng, D, [rows, cols], [cols, rows])                                     # feasible across both components, wide and tall
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        eng.lsa_gather(D, [list(A), [1, 2]], [[170, 200, 290], [3, 4]])
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        eng.lsa_gather(D, [[170, 200, 290, 180]], [list(A)])
    finite = list(range(0, 150, 7))
    bad = D.copy()
    bad[finite[3], finite[5]] = np.nan
    for r, c in ((finite, finite[:9]), (finite[:9], finite)):
        with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
            eng.lsa_gather(bad, [r, [0, 1]], [c, [2, 3]])
    bad = D.copy()
    bad[finite[3], finite[5]] = -np.inf
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        eng.lsa_gather(bad, [finite], [finite])
    check(eng, D, [finite, finite[:8], finite], [finite, finite, finite[:8]], maximize=True)
    with pytest.raises(ValueError, match=r"indices must lie in \[0, 301\)"):
        eng.lsa_gather(D, [[0, 301]], [[1, 2]])
    with pytest.raises(ValueError, match="indices must lie"):
        eng.lsa_gather(D, [[0, 1]], [[-1, 2]])
    with pytest.raises(ValueError, match="empty index list"):
        eng.lsa_gather(D, [[0, 1], []], [[1, 2], [3]])


def test_strided_device_tensor_is_read_in_place(eng, random_D):
    import torch
    full = torch.as_tensor(random_D).to(eng.device)
    view = full[:700, :700]                                                       # row stride 1100
    rng = np.random.default_rng(11)
    rows, cols = lists(rng, 700, (30, 80, 100)), lists(rng, 700, (90, 80, 20))
    got = check(eng, random_D[:700, :700], rows, cols, Dd=view)
    np.testing.assert_array_equal(got, eng.lsa_gather(np.ascontiguousarray(random_D[:700, :700]), rows, cols))


@pytest.fixture(scope="module")
def padded_batch(geod, dijkstra_mats):
    """small (160, heat method), grid (1200) and torus (2048, shortest paths) with 3, 6 and 16 Voronoi groups, padded to 2048"""
    mats = [geod["small_D"], dijkstra_mats["grid"], dijkstra_mats["torus"]]
    groups = [gr.voronoi_groups(D, G) for D, G in zip(mats, (3, 6, 16))]
    pad = np.zeros((3, 2048, 2048))
    for b, D in enumerate(mats):
        pad[b, :len(D), :len(D)] = D
    ref = [gr.groups_dmtx(D, g) for D, g in zip(mats, groups)]
    return mats, groups, pad, ref


def test_padded_batch_of_three_meshes(eng, padded_batch):
    import torch
    mats, groups, pad, ref = padded_batch
    sizes = [len(D) for D in mats]
    got = eng.groups_dmtx(pad, groups, n_verts=sizes)
    Dd = torch.as_tensor(pad).to(eng.device)
    got_dev = eng.groups_dmtx(Dd, groups, n_verts=sizes)
    assert len(got) == 3
    for b in range(3):
        G = len(groups[b])
        assert got[b].shape == (G, G) and got[b].dtype == np.float64
        np.testing.assert_array_equal(got[b], got[b].T)
        np.testing.assert_array_equal(np.diag(got[b]), 0.0)
        bound = gr.mean_bound(groups[b], ref[b])
        print(f"mesh {b}: worst |got - ref| / bound = {np.max(np.abs(got[b] - ref[b])[bound > 0] / bound[bound > 0]):.3f}")
        assert np.all(np.abs(got[b] - ref[b]) <= bound)
        np.testing.assert_array_equal(got_dev[b], got[b])
        # a problem's bits do not depend on what else shares the call
        for i in range(G):
            for j in range(i + 1, G):
                alone = eng.lsa_gather(Dd, [groups[b][i]], [groups[b][j]], mesh=[b])
                np.testing.assert_array_equal(alone[0], got[b][i, j])
    with pytest.raises(ValueError, match="indices must lie"):
        eng.groups_dmtx(Dd, [[[0, 160]], [[0]], [[0]]], n_verts=sizes)


def test_few_groups(eng, geod):
    D = geod["small_D"]
    np.testing.assert_array_equal(eng.groups_dmtx(D, [[1, 2, 3]]), [[0.0]])
    np.testing.assert_array_equal(eng.groups_dmtx(D, [[1, 2, 3], []]), np.zeros((2, 2)))
    assert eng.groups_dmtx(D, []).shape == (0, 0)


def test_reference_fixture_through_utils(eng, geod, capsys, monkeypatch):
    from densematcher_amd import utils
    g = load_golden("fx_groups.npz")
    groups = gr.unpack_groups(g["a_flat"], g["a_off"])
    monkeypatch.setenv("VERBOSE", "1")
    got = utils.get_groups_dmtx(geod["small_D"], groups, device=True)
    assert capsys.readouterr().out.count("Warning: empty group") == 5
    assert got.shape == (6, 6) and np.all(np.abs(got - g["a_dmtx"]) <= gr.mean_bound(groups, g["a_dmtx"]))
    assert np.all(got[2] == 0) and np.all(got[:, 2] == 0)
    monkeypatch.delenv("VERBOSE")
    host = utils.get_groups_dmtx(geod["small_D"], groups, device=False)
    np.testing.assert_array_equal(host, g["a_dmtx"])
    many = utils.get_groups_dmtx_many([geod["small_D"], g["b_D"]], [groups, gr.unpack_groups(g["b_flat"], g["b_off"])], device=True)
    np.testing.assert_array_equal(many[0], got)
    assert np.all(np.abs(many[1] - g["b_dmtx"]) <= gr.mean_bound(gr.unpack_groups(g["b_flat"], g["b_off"]), g["b_dmtx"]))
    full = [x for x in groups if len(x)]
    d = utils.get_distance_between_groups(geod["small_D"], full[0], full[1], device=True)
    assert d == got[0, 1] and utils.get_distance_between_groups(geod["small_D"], [], full[1], device=True) == 0


@pytest.mark.parametrize("kw", [dict(dijkstra=True), dict(robust=False), dict(robust=False, sym=True)], ids=["dijkstra", "heat", "heat_sym"])
def test_trimesh_groups_dmtx_many(geod, kw):
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    meshes = [TriMesh(geod[name + "_V"], geod[name + "_F"]) for name in ("small", "grid")]
    mats = TriMesh.get_geodesic_many(meshes, **kw)
    groups = [gr.voronoi_groups(np.maximum(D, D.T), G) for D, G in zip(mats, (4, 7))]
    got = TriMesh.get_groups_dmtx_many(meshes, groups, **kw)
    for D, g, out in zip(mats, groups, got):
        ref = gr.groups_dmtx(D, g)
        assert np.all(np.abs(out - ref) <= gr.mean_bound(g, ref))
    np.testing.assert_array_equal(meshes[0].get_groups_dmtx(groups[0], **kw), got[0])


def test_trimesh_robust_needs_the_wheel(geod):
    from densematcher_amd.pyFM.mesh import geometry
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    try:
        geometry._pp3d()
    except ImportError:
        with pytest.raises(ImportError):
            TriMesh(geod["small_V"], geod["small_F"]).get_groups_dmtx([[0, 1], [2, 3]])

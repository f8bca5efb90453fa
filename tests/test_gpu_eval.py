"""GPU: map quality measures on the device (dm_map_metrics / dm_geodesic_diameter, MatchEngine.map_accuracy / map_continuity /
map_coverage / geodesic_diameter, the device route of pyFM.eval, evaluate_pairs) against the host functions of pyFM.eval on the same
matrix, computed at test time, and against the reference's numbers in tests/golden/fx_eval.npz.

Comparison rule -- a bound, not a measurement:
* per-element results (return_all) and the diameter are a gather, one division and a max: BIT-IDENTICAL;
* means and coverages: |got - ref| <= n 2^-52 |ref|, n the number of terms (coverage: the terms of both sums).  Two summation
  orders of the same n terms of one sign err by at most (n - 1) 2^-53 of the sum each; NumPy adds pairwise, the kernel 256 strided
  partial sums and a tree;
* inf / nan results must be the same inf / nan.
Every figure is printed before it is asserted."""
import warnings

import numpy as np
import pytest
import scipy.sparse.csgraph as csgraph

import graphgeod_restate as ggr
from conftest import load_golden
from densematcher_amd.pyFM import eval as ev

pytestmark = pytest.mark.gpu

WAVE, WORKGROUP = 64, 256                # dm_mapmetrics.hip: MM_T threads per problem, one term per thread and pass
LENGTHS = (1, WAVE - 1, WAVE, WAVE + 1, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, 1000)


@pytest.fixture(autouse=True)
def quiet():
    """x / 0, inf / inf and the mean of nothing are NumPy's own warnings on the reference side"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    e = default_engine()
    yield e
    e.reset_options()


@pytest.fixture(scope="module")
def fx():
    e, geod, groups = load_golden("fx_eval.npz"), load_golden("fx_geod.npz"), load_golden("fx_groups.npz")
    for k in ("small_D", "small_edges", "small_V", "small_F", "grid_V", "grid_F", "torus_V", "torus_F"):
        e[k] = geod[k]
    e["b_D"] = groups["b_D"]
    for v in e.values():
        v.setflags(write=False)
    return e


@pytest.fixture(scope="module")
def mats(fx):
    """the 160-vertex heat matrix of the fixture, csgraph.dijkstra of grid (1200) and torus (2048) and of the constructed
    two-component mesh: computed once, read-only; with each its edge list"""
    from densematcher_amd.pyFM.mesh import geometry
    out = {"small": (fx["small_D"], fx["small_edges"].astype(np.int64))}
    for name in ("grid", "torus"):
        V, F = fx[name + "_V"], fx[name + "_F"]
        out[name] = (csgraph.dijkstra(geometry.edge_graph(V, F)), geometry.edges_from_faces(F))
    V, F = ggr.constructed_mesh()
    out["constructed"] = (csgraph.dijkstra(geometry.edge_graph(V, F)), geometry.edges_from_faces(F))
    for D, E in out.values():
        D.setflags(write=False)
        E.setflags(write=False)
    return out


def close(got, ref, n, what):
    """the comparison rule for a mean or a coverage of n terms"""
    got, ref = float(got), float(ref)
    if not np.isfinite(ref):
        print(f"{what}: got {got}, ref {ref}")
        assert (np.isnan(got) and np.isnan(ref)) or got == ref, (what, got, ref)
        return
    bound = n * 2.0 ** -52 * abs(ref)
    print(f"{what}: n = {n}: |got - ref| = {abs(got - ref):.3e}, bound {bound:.3e}")
    assert abs(got - ref) <= bound, (what, got, ref, bound)


def seeded_maps(rng, n, lengths):
    """maps with repeats, of the given lengths, into [0, n)"""
    return [rng.integers(0, n, L) for L in lengths]


@pytest.mark.parametrize("name", ["small", "grid", "torus"])
def test_accuracy_every_length(eng, mats, name):
    """lengths below, at and above the wavefront, the workgroup (= one full pass) and N, in one call; plain, scaled per problem,
    and scaled by the diameter; the host matrix and the device tensor give the same bits"""
    import torch
    D = mats[name][0]
    n = len(D)
    lengths = LENGTHS + (n,)
    rng = np.random.default_rng(n)
    p2ps, gts = seeded_maps(rng, n, lengths), seeded_maps(rng, n, lengths)
    Dd = torch.as_tensor(D).to(eng.device)
    scales = rng.uniform(0.5, 3.0, len(lengths))
    diam = eng.geodesic_diameter(Dd)
    assert diam.shape == (1,) and diam.dtype == np.float64
    np.testing.assert_array_equal(diam, [np.max(D)])
    for scale, ref_scale in ((None, [None] * len(lengths)), (scales, list(scales)), ("diameter", [np.max(D)] * len(lengths))):
        means, dists = eng.map_accuracy(Dd, p2ps, gts, scale=scale, return_all=True)
        assert means.shape == (len(lengths),) and means.dtype == np.float64
        for p, L in enumerate(lengths):
            ref_mean, ref_d = ev.accuracy(p2ps[p], gts[p], D, return_all=True, sqrt_area=ref_scale[p])
            np.testing.assert_array_equal(dists[p], ref_d, err_msg=f"length {L}")
            close(means[p], ref_mean, L, f"{name}: accuracy, length {L}, scale {scale if isinstance(scale, str) else scale is not None}")
        np.testing.assert_array_equal(eng.map_accuracy(Dd, p2ps, gts, scale=scale), means)
        np.testing.assert_array_equal(eng.map_accuracy(D, p2ps, gts, scale=scale), means)


def test_continuity_edge_lists(eng, mats):
    """1, 465 (small_edges) and 6144 (torus) edges; both sides in one tensor (D2=None), and a second tensor of another N"""
    import torch
    rng = np.random.default_rng(6144)
    Ds, Es = mats["small"]
    Dg = mats["grid"][0]
    Dt, Et = mats["torus"]
    assert len(Es) == 465 and len(Et) == 6144
    dev = {k: torch.as_tensor(mats[k][0]).to(eng.device) for k in ("small", "grid", "torus")}
    # the source and the target in ONE padded tensor: torus (mesh 0) and small (mesh 1)
    pad = np.zeros((2, 2048, 2048))
    pad[0], pad[1, :160, :160] = Dt, Ds
    padd = torch.as_tensor(pad).to(eng.device)
    m_tt, m_ss, m_ts, m_st = rng.integers(0, 2048, 2048), rng.integers(0, 160, 160), rng.integers(0, 160, 2048), rng.integers(0, 2048, 160)
    cases = [(m_tt, Et, 0, 0), (m_tt, Et[:1], 0, 0), (m_ss, Es, 1, 1), (m_ts, Et, 1, 0), (m_st, Es, 0, 1), (m_st, Es[5:6], 0, 1)]
    got = eng.map_continuity(padd, None, [c[0] for c in cases], [c[1] for c in cases], mesh1=[c[2] for c in cases],
                             mesh2=[c[3] for c in cases], n_verts1=[2048, 160])
    assert got.shape == (len(cases),) and got.dtype == np.float64
    host = (Dt, Ds)
    for k, (m, E, b1, b2) in enumerate(cases):
        close(got[k], ev.continuity(m, host[b1], host[b2], E), len(E), f"continuity in one tensor, case {k}, {len(E)} edges")
    # a second tensor of another N: torus vertices mapped into the grid
    m_tg = rng.integers(0, 1200, 2048)
    got = eng.map_continuity(dev["grid"], dev["torus"], [m_tg, m_tg], [Et, Et[:1]])
    close(got[0], ev.continuity(m_tg, Dg, Dt, Et), 6144, "continuity, grid <- torus, 6144 edges")
    close(got[1], ev.continuity(m_tg, Dg, Dt, Et[:1]), 1, "continuity, grid <- torus, 1 edge")
    # the heat matrix has neighbours at distance 0: inf, as the host gives
    m = rng.integers(0, 160, 160)
    ref = ev.continuity(m, Ds, Ds, Es)
    assert not np.isfinite(ref)
    close(eng.map_continuity(dev["small"], None, [m], [Es])[0], ref, 465, "continuity, small_edges (zero lengths)")


def test_reference_fixture_on_the_device(eng, fx):
    """the numbers the reference's functions returned (tools/make_golden_eval.py), cases a and b"""
    import torch
    D, bD = fx["small_D"], fx["b_D"]
    Dd, bDd = torch.as_tensor(D).to(eng.device), torch.as_tensor(bD).to(eng.device)
    sa = float(fx["a_sqrt_area"])
    means, dists = eng.map_accuracy(Dd, [fx["a_p2p"], fx["a_p2p_long"]] * 2, [fx["a_gt"], fx["a_gt_long"]] * 2, return_all=True,
                                    scale=[1.0, 1.0, sa, sa])
    for k, name in enumerate(("", "_long", "_scaled", "_long_scaled")):
        np.testing.assert_array_equal(dists[k], fx["a_dists" + name])
        close(means[k], fx["a_acc" + name], len(dists[k]), "fixture a_acc" + name)
    means, dists = eng.map_accuracy(bDd, [fx["b_acc_p2p"]], [fx["b_acc_gt"]], return_all=True)
    np.testing.assert_array_equal(dists[0], fx["b_dists"])
    close(means[0], fx["b_acc"], 130, "fixture b_acc (ties)")
    got = eng.map_continuity(Dd, None, [fx["a_p2p"]] * 2, [fx["small_edges"], fx["a_edges_pos"]])
    close(got[0], fx["a_cont"], 465, "fixture a_cont")
    close(got[1], fx["a_cont_pos"], len(fx["a_edges_pos"]), "fixture a_cont_pos")
    got = eng.map_continuity(bDd, None, [fx["b_p2p"]] * 2, [fx["b_edges_inf"], fx["b_edges_nan"]])
    assert np.isposinf(got[0]) and np.isposinf(fx["b_cont_inf"]) and np.isnan(got[1]) and np.isnan(fx["b_cont_nan"])
    got = eng.map_coverage(fx["a_area"], [fx["a_p2p"], fx["a_p2p_long"]])
    close(got[0], fx["a_cov"], len(np.unique(fx["a_p2p"])) + 160, "fixture a_cov")
    close(got[1], fx["a_cov_long"], len(np.unique(fx["a_p2p_long"])) + 160, "fixture a_cov_long")


def test_two_components_infinite_distances(eng, mats):
    """accuracy inf, "diameter" scale inf, elements inf / inf = nan as NumPy gives them"""
    D = mats["constructed"][0]
    n = len(D)
    assert np.isinf(D).sum() == 45528
    rng = np.random.default_rng(301)
    p2p, gt = rng.integers(0, n, 400), rng.integers(0, n, 400)
    assert np.isinf(D[p2p, gt]).any()
    inside = np.flatnonzero(np.isfinite(D[0]))
    same_p, same_g = inside[rng.integers(0, len(inside), 100)], inside[rng.integers(0, len(inside), 100)]
    np.testing.assert_array_equal(eng.geodesic_diameter(D), [np.inf])
    for scale, ref_scale in ((None, None), ("diameter", np.inf)):
        means, dists = eng.map_accuracy(D, [p2p, same_p], [gt, same_g], scale=scale, return_all=True)
        for k, (a, b) in enumerate(((p2p, gt), (same_p, same_g))):
            ref_mean, ref_d = ev.accuracy(a, b, D, return_all=True, sqrt_area=ref_scale)
            np.testing.assert_array_equal(dists[k], ref_d)
            close(means[k], ref_mean, len(a), f"two components, problem {k}, scale {scale}")
    assert np.isposinf(eng.map_accuracy(D, [p2p], [gt])[0]) and np.isnan(eng.map_accuracy(D, [p2p], [gt], scale="diameter")[0])
    bad = D.copy()
    bad[17, 5] = np.nan
    assert np.isnan(eng.geodesic_diameter(bad)[0])


@pytest.fixture(scope="module")
def padded(mats):
    """960, 640 and 6 vertices in one (3, 960, ld = 1000) tensor; everything past n_verts[b] and the columns 960..ld hold 1e300, and
    so does the same region of the areas"""
    sizes = (960, 640, 6)
    blocks = [np.ascontiguousarray(mats[k][0][:s, :s]) for k, s in zip(("grid", "torus", "small"), sizes)]
    full = np.full((3, 960, 1000), 1e300)
    rng = np.random.default_rng(960)
    areas = [rng.uniform(0.1, 1.0, s) for s in sizes]
    area = np.full((3, 960), 1e300)
    for b, (D, a) in enumerate(zip(blocks, areas)):
        full[b, :len(D), :len(D)] = D
        area[b, :len(a)] = a
    lengths = (1, 5, 100, 700)
    mesh = np.repeat(np.arange(3), len(lengths))
    maps = [rng.integers(0, s, L) for s in sizes for L in lengths]
    gts = [rng.integers(0, sizes[b], len(m)) for b, m in zip(mesh, maps)]
    # edges between DIFFERENT entries of a map (a shortest-path matrix is zero on its diagonal only); a map of one entry has none
    edges = []
    for m in maps:
        e0 = rng.integers(0, len(m), 300)
        edges.append(np.stack([e0, (e0 + 1 + rng.integers(0, max(1, len(m) - 1), 300)) % len(m)], 1))
    # continuity needs every edge end below the map's length AND the vertex count of the target (here: the map's own mesh)
    ok = [k for k in range(len(maps)) if 1 < len(maps[k]) <= sizes[mesh[k]]]
    return sizes, blocks, full, areas, area, maps, gts, edges, mesh, ok


def test_padded_batch_masks_the_padding(eng, padded):
    import torch
    sizes, blocks, full, areas, area, maps, gts, edges, mesh, ok = padded
    view = torch.as_tensor(full).to(eng.device)[:, :, :960]
    assert view.stride() == (960000, 1000, 1) and len(ok) == 6
    np.testing.assert_array_equal(eng.geodesic_diameter(view, n_verts=sizes), [np.max(D) for D in blocks])
    acc, dists = eng.map_accuracy(view, maps, gts, mesh=mesh, n_verts=sizes, scale="diameter", return_all=True)
    cont = eng.map_continuity(view, None, [maps[k] for k in ok], [edges[k] for k in ok], mesh1=mesh[ok], mesh2=mesh[ok], n_verts1=sizes)
    cov = eng.map_coverage(torch.as_tensor(area).to(eng.device), maps, mesh=mesh, n_verts=sizes)
    for k, b in enumerate(mesh):
        alone_acc, alone_d = eng.map_accuracy(blocks[b], [maps[k]], [gts[k]], scale="diameter", return_all=True)
        np.testing.assert_array_equal(acc[k], alone_acc[0])
        np.testing.assert_array_equal(dists[k], alone_d[0])
        ref_mean, ref_d = ev.accuracy(maps[k], gts[k], blocks[b], return_all=True, sqrt_area=np.max(blocks[b]))
        np.testing.assert_array_equal(dists[k], ref_d)
        close(acc[k], ref_mean, len(maps[k]), f"padded accuracy {k}")
        np.testing.assert_array_equal(cov[k], eng.map_coverage(areas[b], [maps[k]])[0])
        close(cov[k], ev.coverage(maps[k], areas[b]), len(np.unique(maps[k])) + sizes[b], f"padded coverage {k}")
    for j, k in enumerate(ok):
        b = mesh[k]
        np.testing.assert_array_equal(cont[j], eng.map_continuity(blocks[b], None, [maps[k]], [edges[k]])[0])
        close(cont[j], ev.continuity(maps[k], blocks[b], blocks[b], edges[k]), len(edges[k]), f"padded continuity {k}")
    with pytest.raises(IndexError):
        eng.map_accuracy(view, [[0, 6]], [[0, 1]], mesh=[2], n_verts=sizes)
    with pytest.raises(IndexError):
        eng.map_coverage(area, [[640]], mesh=[1], n_verts=sizes)


def test_three_hundred_mixed_problems_one_call(eng, padded):
    """accuracy, continuity and coverage problems in ONE launch, many sharing index lists: every value is bit-identical to the
    same problem in a call of its own and in a call with the problems in reverse order"""
    import torch
    sizes, blocks, full, areas, area, maps, gts, edges, mesh, ok = padded
    view = torch.as_tensor(full).to(eng.device)[:, :, :960]
    aread = torch.as_tensor(area).to(eng.device)
    parts, off = [], 0

    def put(a):
        nonlocal off
        parts.append(np.asarray(a, np.int32))
        off += len(a)
        return off - len(a)
    o_map = [put(m) for m in maps]                                                # every list once, whatever the number of its problems
    o_gt = [put(g) for g in gts]
    edge_counts = (1, 65, 300)
    o_edge = {(k, E): put(edges[k][:E].T.reshape(-1)) for k in ok for E in edge_counts}      # every e0, then every e1
    rows, scale, n_all = [], [], 0
    rng = np.random.default_rng(300)
    for p in range(300):
        kind = p % 3
        k = ok[int(rng.integers(0, len(ok)))] if kind == 1 else int(rng.integers(0, len(maps)))
        b, L = int(mesh[k]), len(maps[k])
        if kind == 0:
            flags = int(rng.integers(0, 4))                                       # 1: scaled, 2: the elements are kept
            rows.append((0, b, 0, o_map[k], o_gt[k], L, n_all, flags))
            n_all += L if flags & 2 else 0
        elif kind == 1:
            E = edge_counts[int(rng.integers(0, 3))]
            rows.append((1, b, b, o_map[k], o_edge[k, E], E, L, 0))
        else:
            rows.append((2, b, 0, o_map[k], 0, int(rng.integers(0, L + 1)), 0, 0))     # a prefix of the map, the empty one included
        scale.append(float(rng.uniform(0.5, 2.0)))
    table, idx, scale = np.asarray(rows, np.int32), np.concatenate(parts), np.asarray(scale)
    assert table.shape == (300, 8) and {0, 1, 2} <= set(table[:, 0].tolist())
    kw = dict(D=view, area=aread, n_verts=sizes)
    values, every = eng.map_metrics_table(idx, table, scale=scale, n_all=n_all, **kw)
    assert values.shape == (300,) and every.shape == (n_all,) and np.isfinite(values).sum() >= 290
    rev, rev_every = eng.map_metrics_table(idx, table[::-1], scale=scale[::-1], n_all=n_all, **kw)
    np.testing.assert_array_equal(rev[::-1], values)
    np.testing.assert_array_equal(rev_every, every)
    for p in range(300):
        row = table[p].copy()
        keep = bool(row[0] == 0 and row[7] & 2)
        first = row[6]
        if keep:
            row[6] = 0
        one, one_every = eng.map_metrics_table(idx, row[None], scale=scale[p:p + 1], n_all=int(row[5]) if keep else 0, **kw)
        np.testing.assert_array_equal(one[0], values[p], err_msg=f"problem {p}: {table[p]}")
        if keep:
            np.testing.assert_array_equal(one_every, every[first:first + row[5]])


def test_table_errors(eng, fx):
    D = fx["small_D"]
    idx = np.arange(10, dtype=np.int32)
    for row in ((3, 0, 0, 0, 0, 5, 0, 0), (0, 1, 0, 0, 0, 5, 0, 0), (0, 0, 0, 6, 0, 5, 0, 0), (0, 0, 0, 0, 0, 5, 0, 2),
                (1, 0, 1, 0, 0, 5, 10, 0), (1, 0, 0, 0, 1, 5, 10, 0), (2, 0, 0, 0, 0, 5, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, -1, 0, 5, 0, 0)):
        with pytest.raises(ValueError):
            eng.map_metrics_table(idx, [row], D=D)
    with pytest.raises(IndexError):                                               # the kernel refuses an index outside its mesh
        eng.map_metrics_table(np.asarray([0, 160], np.int32), [(0, 0, 0, 0, 0, 2, 0, 0)], D=D)
    with pytest.raises(IndexError):
        eng.map_metrics_table(np.asarray([0, 3], np.int32), [(2, 0, 0, 0, 0, 2, 0, 0)], area=np.ones(3))


def test_no_problem_and_empty_lists(eng, fx):
    D = fx["small_D"]
    assert eng.map_accuracy(D, [], []).shape == (0,)
    means, dists = eng.map_accuracy(D, [], [], return_all=True)
    assert means.shape == (0,) and dists == []
    assert eng.map_continuity(D, None, [], []).shape == (0,) and eng.map_coverage(fx["a_area"], []).shape == (0,)
    empty = np.zeros(0, np.int64)
    means, dists = eng.map_accuracy(D, [empty, fx["a_p2p"]], [empty, fx["a_gt"]], return_all=True)
    assert np.isnan(means[0]) and dists[0].shape == (0,)
    np.testing.assert_array_equal(dists[1], fx["a_dists"])
    got = eng.map_continuity(D, None, [fx["a_p2p"], fx["a_p2p"]], [np.zeros((0, 2), np.int64), fx["a_edges_pos"]])
    assert np.isnan(got[0])
    close(got[1], fx["a_cont_pos"], len(fx["a_edges_pos"]), "continuity next to an empty edge list")
    np.testing.assert_array_equal(eng.map_coverage(fx["a_area"], [empty]), [ev.coverage(empty, fx["a_area"])])


def test_coverage_one_vertex_and_permutation(eng, fx, mats):
    rng = np.random.default_rng(2048)
    for n in (160, 1200, 2048):
        area = rng.uniform(0.1, 1.0, n)
        one, perm, twice = np.full(300, n - 1), rng.permutation(n), np.concatenate([rng.permutation(n), rng.permutation(n)[:77]])
        part = rng.integers(0, n, n)
        got = eng.map_coverage(area, [one, perm, twice, part, [0]])
        close(got[0], ev.coverage(one, area), 1 + n, f"coverage, one vertex of {n}")
        assert got[1] == 1.0 and got[2] == 1.0
        close(got[3], ev.coverage(part, area), len(np.unique(part)) + n, f"coverage, seeded map on {n}")
        close(got[4], area[0] / area.sum(), 1 + n, f"coverage, vertex 0 of {n}")


def test_pyfm_eval_routes(eng, fx, mats):
    """a device tensor takes the device route and equals the host call on the same matrix under the rule; NumPy inputs return the
    host route's bits: the same values as before the device route existed (the fixture's)"""
    import torch
    D, E = mats["grid"]
    n = len(D)
    Dd = torch.as_tensor(D).to(eng.device)
    rng = np.random.default_rng(12)
    p2p, gt = rng.integers(0, n, n), rng.integers(0, n, n)
    acc, dists = ev.accuracy(p2p, gt, Dd, return_all=True, sqrt_area=1.75)
    ref_acc, ref_d = ev.accuracy(p2p, gt, Dd.cpu().numpy(), return_all=True, sqrt_area=1.75)
    np.testing.assert_array_equal(dists, ref_d)
    close(acc, ref_acc, n, "pyFM.eval.accuracy")
    assert ev.accuracy(p2p, gt, Dd, sqrt_area=1.75) == acc
    close(ev.continuity(p2p, Dd, Dd, E), ev.continuity(p2p, D, D, E), len(E), "pyFM.eval.continuity")
    area = rng.uniform(0.1, 1.0, n)
    close(ev.coverage(p2p, torch.as_tensor(area).to(eng.device)), ev.coverage(p2p, area), len(np.unique(p2p)) + n, "pyFM.eval.coverage")
    np.testing.assert_array_equal(ev.geodesic_label_errors(Dd, p2p, gt), D[p2p, gt] / D.max())
    np.testing.assert_array_equal(ev.geodesic_label_errors(Dd, p2p, gt, normalization="area", area=2.5), D[p2p, gt] / np.sqrt(2.5))
    many = ev.accuracy_many([p2p, p2p[:100]], [gt, gt[:100]], Dd, sqrt_area=[1.75, 1.0])
    assert many[0] == acc
    close(many[1], ev.accuracy(p2p[:100], gt[:100], D), 100, "accuracy_many on the device")
    close(ev.continuity_many([p2p], Dd, None, [E])[0], ev.continuity(p2p, D, D, E), len(E), "continuity_many on the device")
    close(ev.coverage_many([p2p], torch.as_tensor(area).to(eng.device))[0], ev.coverage(p2p, area), len(np.unique(p2p)) + n, "coverage_many")
    # NumPy in: the host route, bit for bit
    sD = fx["small_D"]
    acc, dists = ev.accuracy(fx["a_p2p"], fx["a_gt"], sD, return_all=True, sqrt_area=float(fx["a_sqrt_area"]))
    np.testing.assert_array_equal(acc, fx["a_acc_scaled"])
    np.testing.assert_array_equal(dists, fx["a_dists_scaled"])
    np.testing.assert_array_equal(ev.continuity(fx["a_p2p"], sD, sD, fx["a_edges_pos"]), fx["a_cont_pos"])
    np.testing.assert_array_equal(ev.coverage(fx["a_p2p"], fx["a_area"]), fx["a_cov"])
    np.testing.assert_array_equal(ev.accuracy_many([fx["a_p2p"]], [fx["a_gt"]], sD), [fx["a_acc"]])


@pytest.mark.parametrize("kw", [dict(dijkstra=True), dict(robust=False)], ids=["dijkstra", "heat"])
def test_evaluate_pairs(eng, fx, mats, kw, monkeypatch):
    """3 meshes (small, and grid twice), 4 pairs: the host functions on the host matrices; the distinct meshes' matrices are
    computed ONCE (one graph_geodesic call, two matrices).  The heat method on small alone."""
    from densematcher_amd.engine import MatchEngine
    from densematcher_amd.pyFM.mesh.trimesh import TriMesh
    small, grid = TriMesh(fx["small_V"], fx["small_F"]), TriMesh(fx["grid_V"], fx["grid_F"])
    if "dijkstra" in kw:
        meshes, pairs = [small, grid, grid], [(0, 1), (1, 0), (1, 2), (2, 2)]
        from densematcher_amd.pyFM.mesh import geometry
        host = [csgraph.dijkstra(geometry.edge_graph(fx["small_V"], fx["small_F"])), mats["grid"][0], mats["grid"][0]]
    else:
        meshes, pairs = [small], [(0, 0), (0, 0)]
        host = TriMesh.get_geodesic_many(meshes, robust=False)
    rng = np.random.default_rng(4)
    maps, gts = [], []
    for q, (i, j) in enumerate(pairs):
        ns, nt = meshes[i].n_vertices, meshes[j].n_vertices
        one = rng.integers(0, ns, nt)
        maps.append(one if q == 0 else {"p2p21": one, "p2p21_zo": rng.permutation(max(ns, nt))[:nt] % ns})
        gts.append(rng.integers(0, ns, nt))
    calls = []
    real = MatchEngine.graph_geodesic
    monkeypatch.setattr(MatchEngine, "graph_geodesic", lambda self, graphs, *a, **k: (calls.append(len(graphs)), real(self, graphs, *a, **k))[1])
    out = ev.evaluate_pairs(meshes, pairs, maps, gts, normalization="diameter", **kw)
    assert calls == ([2] if "dijkstra" in kw else [])
    assert len(out) == len(pairs) and set(out[0]) == {"accuracy", "continuity", "coverage"} and set(out[1]) == {"p2p21", "p2p21_zo"}
    for q, (i, j) in enumerate(pairs):
        for name, m in (maps[q].items() if isinstance(maps[q], dict) else [(None, maps[q])]):
            res = out[q] if name is None else out[q][name]
            what = f"evaluate_pairs {kw}: pair {q} {name}"
            close(res["accuracy"], ev.accuracy(m, gts[q], host[i], sqrt_area=np.max(host[i])), len(m), what + " accuracy")
            E = meshes[j].edges
            close(res["continuity"], ev.continuity(m, host[i], host[j], E), len(E), what + " continuity")
            va = meshes[i].vertex_areas
            close(res["coverage"], ev.coverage(m, va), len(np.unique(m)) + len(va), what + " coverage")
    only = ev.evaluate_pairs(meshes, pairs[:1], maps[:1], gts[:1], continuity=False, coverage=False, **kw)
    assert set(only[0]) == {"accuracy"}
    close(only[0]["accuracy"], ev.accuracy(maps[0], gts[0], host[pairs[0][0]]), len(maps[0]), "evaluate_pairs, accuracy alone, no scale")

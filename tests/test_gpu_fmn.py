"""GPU: functional map networks on the device (dm_fmn_*, dm_eigh_smallest, densematcher_amd.pyFM.FMN with device=True) against the host
route, which tests/test_fmn_cpu.py pins to the recorded reference (tests/golden/fx_fmn.npz), and against NumPy.  Every bound is stated in
units of u2 = 2^-52 from the lengths of the sums involved, or from the residual the eigensolver itself returns (Davis-Kahan)."""
import numpy as np
import pytest
import scipy.sparse as sparse

import fmn_fixture as ff

pytestmark = pytest.mark.gpu
U2 = 2.0 ** -52
M_SET = (4, 13, 22, 65)
PAD = 3


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    e = default_engine()
    yield e
    e.set_option("fmn_eig_route", 0)


def _consistent_maps(E_edges, M, seed, noise=0.05):
    """seeded maps of a nearly consistent network: C_ij = R_i^T R_j + noise (R_i random orthogonal), stored (E, M + PAD, M + PAD) inside
    random padding that the crop must ignore"""
    rng = np.random.default_rng(seed)
    R = [np.linalg.qr(rng.standard_normal((M, M)))[0] for _ in range(5)]
    out = rng.standard_normal((len(E_edges), M + PAD, M + PAD))
    for q, (i, j) in enumerate(E_edges):
        out[q, :M, :M] = R[i].T @ R[j] + noise * rng.standard_normal((M, M)) / np.sqrt(M)
    return out


@pytest.fixture(scope="module")
def cases():
    """per M: maps (E, M + 3, M + 3), weights (E,), the host quadratic form, the same on absolute values"""
    from densematcher_amd.pyFM import CLB_quad_form
    fx, meshes, edges, maps0, samples = ff.load()
    out = {}
    for M in M_SET:
        if M == 4:
            maps = np.ascontiguousarray(fx["maps0"][:, :M + PAD, :M + PAD])
        elif M == 22:
            maps = np.random.default_rng(5).standard_normal((len(edges), M + PAD, M + PAD))
            maps[:, :M, :M] = fx["adjacency_sub_maps"]
        else:
            maps = _consistent_maps(edges, M, seed=M)
        w = np.random.default_rng(100 + M).uniform(0.2, 1.7, len(edges))
        w[0], w[1] = 0.0, 1.0
        I, J = [e[0] for e in edges], [e[1] for e in edges]
        wm = sparse.csr_matrix((w, (I, J)), shape=(5, 5))
        md = {e: maps[q] for q, e in enumerate(edges)}
        W = CLB_quad_form(md, wm, M=M).toarray()
        Wabs = CLB_quad_form({e: np.abs(maps[q]) for q, e in enumerate(edges)}, wm, M=M).toarray()
        out[M] = dict(maps=maps, w=w, W=W, Wabs=np.abs(Wabs), edges=edges)
    return out


@pytest.fixture(scope="module")
def device_W(eng, cases):
    import torch
    out = {}
    for M, c in cases.items():
        e = torch.as_tensor(np.asarray(c["edges"], np.int32))
        out[M] = eng.fmn_quad_form(5, M, c["maps"], e, c["w"])
    return out


# ---------------------------------------------------------------------------------------------------------------- quadratic form
@pytest.mark.parametrize("M", M_SET)
def test_quad_form(cases, device_W, M):
    c = cases[M]
    W = device_W[M].cpu().numpy()
    assert W.shape == (5 * M, 5 * M)
    assert np.array_equal(W, W.T)
    deg = np.zeros(5, int)
    for (i, j) in c["edges"]:
        deg[i] += 1
        deg[j] += 1
    for bi in range(5):
        for bj in range(5):
            blk = W[bi * M:(bi + 1) * M, bj * M:(bj + 1) * M]
            ref = c["W"][bi * M:(bi + 1) * M, bj * M:(bj + 1) * M]
            if bi != bj:
                assert np.array_equal(blk, ref), (bi, bj)            # one product or a two-term sum: the host's bits
            else:
                bound = (M + deg[bi]) * U2 * c["Wabs"][bi * M:(bi + 1) * M, bj * M:(bj + 1) * M]
                err = np.abs(blk - ref)
                print(f"M={M} block {bi}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
                assert np.all(err <= bound), (bi, float((err - bound).max()))


# ------------------------------------------------------------------------------------------------ orthogonality defect, cycle costs
def _cycles(edges):
    from densematcher_amd.pyFM import FMN
    net = FMN([None] * 5, device=False)
    net.edges, net.edge2ind = list(edges), {e: q for q, e in enumerate(edges)}
    net.extract_3_cycles()
    return net.cycles, net._cycle_edge_indices()


@pytest.mark.parametrize("M", M_SET)
def test_orth_defect_and_cycle_costs(eng, cases, M):
    c = cases[M]
    maps = c["maps"]
    C = maps[:, :M, :M]
    d = eng.fmn_orth_defect(maps, M).cpu().numpy()
    ref = np.asarray([np.linalg.norm(C[q].T @ C[q] - np.eye(M)) for q in range(len(C))])
    bound = np.asarray([M * U2 * np.linalg.norm(np.abs(C[q]).T @ np.abs(C[q])) for q in range(len(C))])
    print(f"M={M} defect: max err / bound = {(np.abs(d - ref) / bound).max():.3f}")
    assert np.all(np.abs(d - ref) <= bound)
    cycles, ce = _cycles(c["edges"])
    assert len(cycles) > 10
    cost = eng.fmn_cycle_costs(maps, M, ce).cpu().numpy()
    eye = np.eye(M)
    for q, (a, b, cc) in enumerate(ce):
        rots = [(a, b, cc), (b, cc, a), (cc, a, b)]
        host = max(np.linalg.norm(C[x] @ C[y] @ C[z] - eye) for x, y, z in rots)
        bnd = max(2 * M * U2 * np.linalg.norm(np.abs(C[x]) @ np.abs(C[y]) @ np.abs(C[z])) for x, y, z in rots)
        assert abs(cost[q] - host) <= bnd, (q, cost[q], host, bnd)
    # an edge's / a cycle's result does not depend on what else is in the call
    assert np.array_equal(eng.fmn_orth_defect(maps[:3], M).cpu().numpy(), d[:3])
    assert np.array_equal(eng.fmn_cycle_costs(maps, M, ce[3:5]).cpu().numpy(), cost[3:5])


def test_independence_of_the_quadratic_form_of_absent_edges(eng, cases, device_W):
    """3 of the 18 edges: the blocks they alone touch are the bits of the 18-edge call's"""
    import torch
    c = cases[13]
    sel = [q for q, e in enumerate(c["edges"]) if e in ((0, 1), (1, 0), (3, 0))]             # ((0, 3) is no edge of the graph)
    assert len(sel) == 3
    e3 = torch.as_tensor(np.asarray([c["edges"][q] for q in sel], np.int32))
    W3 = eng.fmn_quad_form(5, 13, c["maps"][sel], e3, c["w"][sel]).cpu().numpy()
    W18 = device_W[13].cpu().numpy()
    for (bi, bj) in ((0, 1), (1, 0), (3, 0), (0, 3)):
        assert np.array_equal(W3[bi * 13:(bi + 1) * 13, bj * 13:(bj + 1) * 13], W18[bi * 13:(bi + 1) * 13, bj * 13:(bj + 1) * 13])
    assert not W3[4 * 13:].any() and not W3[:, 4 * 13:].any() and not W3[2 * 13:3 * 13].any()                      # every block is written, zeros included


def test_set_isometries_makes_the_fixture_choices():
    from densematcher_amd.pyFM import FMN
    fx, meshes, edges, maps0, samples = ff.load()
    net = FMN(meshes, maps_dict=maps0, device=True)
    net.set_isometries(M=ff.M0)
    got = net.maps
    assert all(np.array_equal(got[e], fx["adjacency_sub_it1_iso_maps"][q]) for q, e in enumerate(edges))


# ------------------------------------------------------------------------------------------------------------------ eigen-solver
def _double_eigenvalue_matrix():
    rng = np.random.default_rng(77)
    lam = np.concatenate([[0.1, 0.2, 0.3, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1], rng.uniform(3.0, 10.0, 188)])
    Q = np.linalg.qr(rng.standard_normal((200, 200)))[0]
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T), 12


@pytest.mark.parametrize("route", (1, 2))
@pytest.mark.parametrize("which", (13, 22, 65, "double"))
def test_eigh_smallest(eng, device_W, route, which):
    if which == "double":
        A, k = _double_eigenvalue_matrix()
    else:
        A, k = device_W[which].cpu().numpy(), which
    n = A.shape[0]
    eng.set_option("fmn_eig_route", route)
    try:
        lam, V, resid, rounds = eng.eigh_smallest(A, k)
    finally:
        eng.set_option("fmn_eig_route", 0)
    lam, V, resid = lam.cpu().numpy(), V.cpu().numpy(), float(resid)
    ref, Vr = np.linalg.eigh(A)
    lmax = np.abs(ref).max()
    print(f"n={n} k={k} route={route}: rounds={rounds} resid={resid:.3e} max|dlam|={np.abs(lam - ref[:k]).max():.3e}")
    assert resid <= 1e-9 * np.abs(np.diag(A)).max() <= 1e-9 * lmax                    # (the engine's test: max |A_ii| <= lambda_max)
    assert np.all(np.abs(lam - ref[:k]) <= np.sqrt(n) * resid + n * U2 * lmax)
    assert np.abs(V.T @ V - np.eye(k)).max() <= 1e-12
    gap = ref[k] - ref[k - 1]
    defect = np.linalg.norm(V @ V.T - Vr[:, :k] @ Vr[:, :k].T, 2)
    assert defect <= 2 * np.sqrt(n * k) * resid / gap, (defect, resid, gap)
    assert np.all(V[np.abs(V).argmax(axis=0), np.arange(k)] > 0)                     # the sign rule


# -------------------------------------------------------------------------------------------------------------------------- CCLB
@pytest.mark.parametrize("m", (9, 19))
def test_cclb(eng, m):
    """Eigenvalues within m 2^-52 |E|_2 of NumPy's on NumPy's own E, vectors (up to sign) within that over the smallest gap.  (NumPy's
    own eigenvalues are within 0.1 of the bound of an extended-precision evaluation; the diagonal a Jacobi solve leaves is not -- 1.0 to
    1.5 of it at m = 19 -- which is why dm_fmn_cclb returns Rayleigh quotients.)"""
    from densematcher_amd.pyFM import FMN
    fx, meshes, edges, maps0, samples = ff.load()
    M = 10 if m == 9 else 22
    maps = maps0 if M == 10 else {e: fx["adjacency_sub_maps"][q] for q, e in enumerate(edges)}
    host = FMN(meshes, maps_dict=maps, device=False)
    host.set_weights(weight_type="adjacency")
    host.compute_CLB()
    host.compute_CCLB(m)
    CLB = host.CLB
    lam = np.stack([mesh.eigenvalues for mesh in meshes])
    cclb, ev = eng.fmn_cclb(CLB, lam, m)
    cclb, ev = cclb.cpu().numpy(), ev.cpu().numpy()
    E = sum(CLB[i][:, :m].T @ (lam[i, :M, None] * CLB[i][:, :m]) for i in range(5)) / 5
    E = 0.5 * (E + E.T)
    ref = np.linalg.eigvalsh(E)
    bound = m * U2 * np.linalg.norm(E, 2)
    print(f"m={m}: max |d theta| / bound = {np.abs(ev - ref).max() / bound:.3f}")
    assert np.all(np.abs(ev - ref) <= bound)
    gap = np.diff(ref).min()
    hc = host.CCLB
    for i in range(5):
        s = np.sign(np.sum(cclb[i] * hc[i], axis=0))
        assert np.abs(cclb[i] * s - hc[i]).max() <= bound / gap, (i, np.abs(cclb[i] * s - hc[i]).max(), bound / gap)


# ------------------------------------------------------------------------------------------------------------------ one iteration
def _near_tie_check(host, p_dev, p_ref, edges, complete, tau):
    """every entry where the device's vertex map differs from the reference's is a near tie in the host route's embedding"""
    n_diff = n_all = 0
    clean = []
    for (i, j) in edges:
        a, b = p_dev[(i, j)], p_ref[(i, j)]
        n_all += a.size
        bad = np.nonzero(a != b)[0]
        n_diff += bad.size
        if bad.size == 0:
            clean.append((i, j))
            continue
        tree, query = host.get_LB(i, complete=False), host.get_LB(j, complete=complete)
        da = ((query[bad] - tree[a[bad]]) ** 2).sum(-1)
        db = ((query[bad] - tree[b[bad]]) ** 2).sum(-1)
        assert np.all(np.abs(da - db) <= tau * np.maximum(da, db)), ((i, j), float((np.abs(da - db) / np.maximum(da, db)).max()), tau)
    return n_diff, n_all, clean


@pytest.mark.parametrize("wt,use_sub", ff.CONFIGS)
def test_one_iteration(wt, use_sub):
    from densematcher_amd.pyFM import FMN
    fx, meshes, edges, maps0, samples = ff.load()
    pre = ff.prefix(wt, use_sub) + "it1_"
    nets = []
    for device in (False, True):
        net = FMN(meshes, maps_dict=maps0, device=device)
        net.set_subsample(samples if use_sub else None)
        net.M = ff.M0
        net.set_isometries(M=ff.M0)
        if wt == "icsm":
            net.extract_3_cycles()
            net.compute_Amat()
            x = net.optimize_icsm()
            if device:                                                               # feasible, and the fixture's optimum (the vertex may differ)
                assert np.all(x >= 0) and np.all(net.A @ x >= net.cycle_weight * (1 - 1e-9))
                assert abs(net.icsm_objective - fx[pre + "lp_objective"]) <= 1e-10 * abs(fx[pre + "lp_objective"])
                assert np.abs(net.cycle_weight - fx[pre + "cycle_costs"]).max() <= 1e-12 * fx[pre + "cycle_costs"].max()
        net.set_weights(weight_type=wt)
        net.compute_W(M=ff.M0)
        net.compute_CLB()
        net.compute_CCLB(9)
        net.compute_p2p(complete=not use_sub)
        nets.append(net)
    host, dev = nets
    assert np.abs(np.asarray(dev.W) - host.W.toarray()).max() <= 64 * U2 * np.abs(host.W.toarray()).max()
    lam = host.clb_eigenvalues
    resid = float(dev.clb_resid)
    tau = 8 * np.sqrt(5 * ff.M0 * 9) * resid / (lam[9] - lam[8])
    p_ref = {e: fx[pre + f"p2p_{e[0]}{e[1]}"].astype(np.int64) for e in edges}
    n_diff, n_all, clean = _near_tie_check(host, dev.p2p, p_ref, edges, not use_sub, tau)
    print(f"{pre}: resid={resid:.3e} tau={tau:.3e} differing entries {n_diff} of {n_all}")
    assert n_diff <= 0.005 * n_all
    dev.compute_maps(ff.M0 + ff.STEP, complete=not use_sub)
    got = dev.maps
    for e in clean:
        q = edges.index(e)
        assert np.abs(got[e] - fx[pre + "maps"][q]).max() <= 1e-9, e


# --------------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("wt,use_sub", ff.CONFIGS)
def test_zoomout_refine(wt, use_sub):
    from densematcher_amd.pyFM import FMN
    fx, meshes, edges, maps0, samples = ff.load()
    pre = ff.prefix(wt, use_sub)
    net = FMN(meshes, maps_dict=maps0, device=True)
    kept = ff.keep_last_iteration(net)
    net.zoomout_refine(nit=ff.NIT, step=ff.STEP, subsample=samples if use_sub else None, weight_type=wt, M_init=ff.M0)
    assert net.M == 22
    ref = ff.fixture_p2p(fx, pre, edges)
    n_all = sum(v.size for v in ref.values())
    n_diff = sum(int(np.count_nonzero(kept["p2p"][e] != ref[e])) for e in edges)
    print(f"{pre}: differing final entries {n_diff} of {n_all}")
    assert n_diff <= 0.01 * n_all
    if n_diff == 0:
        assert np.abs(kept["cclb_eigenvalues"] - fx[pre + "cclb_eigenvalues"]).max() <= 1e-6 * np.abs(fx[pre + "cclb_eigenvalues"]).max()
    assert set(net.maps) == set(edges) and net.maps[edges[0]].shape == (22, 22)


# ----------------------------------------------------------------------------------------------------------------------- sampling
def test_integer_subsample_on_trimesh_objects():
    """zoomout_refine(subsample=<int>), the default usage: the samples come from TriMesh.extract_fps_many (ONE device call)"""
    from densematcher_amd.pyFM import FMN, TriMesh
    fx, meshes, edges, maps0, samples = ff.load()
    tms = []
    for mesh in meshes:
        tm = TriMesh(mesh.vertlist, mesh.facelist)
        tm.A, tm.eigenvalues, tm.eigenvectors = mesh.A, mesh.eigenvalues, mesh.eigenvectors
        tms.append(tm)
    net = FMN(tms, maps_dict=maps0, device=True)
    net.compute_subsample(size=96, geodesic=False, starts=[0] * 5)
    assert np.array_equal(net.subsample, samples)                                    # the fixture's Euclidean samples from vertex 0
    net.zoomout_refine(nit=3, step=2, subsample=96, weight_type="adjacency", M_init=ff.M0)
    assert net.subsample.shape == (5, 96) and all(len(set(row)) == 96 for row in net.subsample.tolist())
    got = net.maps
    assert net.M == 14 and all(got[e].shape == (14, 14) and np.isfinite(got[e]).all() for e in edges)


# ------------------------------------------------------------------------------------------------------------------------- limits
def test_device_limits():
    from densematcher_amd.pyFM import FMN
    fx, meshes, edges, maps0, samples = ff.load()
    chain = {(i, i + 1): np.eye(241) for i in range(16)}
    net = FMN([meshes[0]] * 17, maps_dict=chain, device=True)
    net.set_weights(weight_type="adjacency")
    with pytest.raises(ValueError, match="4096"):
        net.compute_W()                                                              # n M = 17 * 241 = 4097
    net = FMN([meshes[0]] * 2, maps_dict={(0, 1): np.eye(257)}, device=True)
    net.set_weights(weight_type="adjacency")
    with pytest.raises(ValueError, match="256"):
        net.compute_W()
    eng = net._eng
    with pytest.raises(ValueError, match="edge ends"):
        eng.fmn_quad_form(2, 4, np.zeros((1, 4, 4)), np.asarray([[0, 2]], np.int32), np.ones(1))
    with pytest.raises(ValueError, match="cycle edge indices"):
        eng.fmn_cycle_costs(np.zeros((3, 4, 4)), 4, np.asarray([[0, 1, 3]], np.int32))
    host = FMN([meshes[0]] * 2, maps_dict={(0, 1): np.eye(257)}, device=False)
    host.set_weights(weight_type="adjacency")
    host.compute_W()
    assert host.W.shape == (514, 514)

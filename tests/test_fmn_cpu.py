"""CPU: the host route of the functional map network (densematcher_amd.pyFM.FMN, device=False) against the recorded run of the
reference's FMN class (tests/golden/fx_fmn.npz), the reference's quirks that are kept, and the C ABI of the device route."""
import os
import re

import numpy as np
import pytest

import fmn_fixture as ff

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dm_fmn_orth_defect", "dm_fmn_cycle_costs", "dm_fmn_quad_form", "dm_eigh_smallest", "dm_fmn_cclb")


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _host_net(use_sub):
    from densematcher_amd.pyFM import FMN
    fx, meshes, edges, maps0, samples = ff.load()
    net = FMN(meshes, maps_dict=maps0, device=False)
    net.set_subsample(samples if use_sub else None)
    net.M = ff.M0
    return net


@pytest.mark.parametrize("wt,use_sub", ff.CONFIGS)
def test_first_iteration_matches_reference(wt, use_sub):
    fx, meshes, edges, maps0, samples = ff.load()
    pre = ff.prefix(wt, use_sub) + "it1_"
    net = _host_net(use_sub)
    net.set_isometries(M=ff.M0)
    assert all(np.array_equal(net.maps[e], fx[pre + "iso_maps"][q]) for q, e in enumerate(edges))      # the same choices, exact transposes
    net.set_weights(weight_type=wt)
    w = np.asarray([net.weights[i, j] for (i, j) in edges])
    assert _rel(w, fx[pre + "weights"]) <= 1e-12
    if wt == "icsm":
        assert [tuple(c) for c in fx[pre + "cycles"]] == list(net.cycles)
        assert _rel(net.cycle_weight, fx[pre + "cycle_costs"]) <= 1e-12
        assert abs(net.icsm_objective - fx[pre + "lp_objective"]) <= 1e-12 * abs(fx[pre + "lp_objective"])
    net.compute_W(M=ff.M0)
    assert _rel(net.W.toarray(), fx[pre + "W"]) <= 1e-12
    net.compute_CLB()
    lmax = fx[pre + "W_evals"][-1]
    assert np.abs(net.clb_eigenvalues - fx[pre + "W_evals"][:ff.M0]).max() <= 1e-10 * lmax
    assert net.CLB.shape == (5, ff.M0, ff.M0)
    gram = sum(net.CLB[i].T @ net.CLB[i] for i in range(5))
    assert np.abs(gram - 5 * np.eye(ff.M0)).max() <= 1e-12 * 5                                          # sum Y_i^T Y_i = n I
    net.compute_CCLB(int(0.9 * ff.M0))
    assert net.m_cclb == 9
    assert np.abs(net.cclb_eigenvalues - fx[pre + "cclb_eigenvalues"]).max() <= 1e-10 * np.abs(fx[pre + "cclb_eigenvalues"]).max()
    net.compute_p2p(complete=not use_sub)
    for e in edges:
        assert np.array_equal(net.p2p[e], fx[pre + f"p2p_{e[0]}{e[1]}"]), e
    net.compute_maps(ff.M0 + ff.STEP, complete=not use_sub)
    assert net.M == 12 and net.p2p is None and net.W is None and net.CCLB is None
    assert _rel(np.stack([net.maps[e] for e in edges]), fx[pre + "maps"]) <= 1e-12


@pytest.mark.parametrize("wt,use_sub", ff.CONFIGS)
def test_refine_matches_reference_and_runs_nit_minus_one_iterations(wt, use_sub):
    from densematcher_amd.pyFM import FMN
    fx, meshes, edges, maps0, samples = ff.load()
    pre = ff.prefix(wt, use_sub)
    net = FMN(meshes, maps_dict=maps0, device=False)
    kept = ff.keep_last_iteration(net)
    calls, inner = [], net.zoomout_iteration

    def counted(*a, **k):
        calls.append((a, k))
        return inner(*a, **k)
    net.zoomout_iteration = counted
    net.zoomout_refine(nit=ff.NIT, step=ff.STEP, subsample=samples if use_sub else None, weight_type=wt, M_init=ff.M0)
    assert len(calls) == ff.NIT - 1 == 6
    assert all(c[1]["complete"] == (not use_sub) for c in calls)
    assert [c[0][0] for c in calls] == [int(0.9 * M) for M in range(10, 22, 2)]                          # m_cclb = int(cclb_ratio * M)
    assert net.M == 22
    ref = ff.fixture_p2p(fx, pre, edges)
    for e in edges:
        assert np.array_equal(kept["p2p"][e], ref[e]), e
    assert _rel(np.stack([net.maps[e] for e in edges]), fx[pre + "maps"]) <= 1e-12
    assert np.abs(kept["cclb_eigenvalues"] - fx[pre + "cclb_eigenvalues"]).max() <= 1e-10 * np.abs(fx[pre + "cclb_eigenvalues"]).max()
    assert np.abs(kept["clb_eigenvalues"] - fx[pre + "W_evals"][:20]).max() <= 1e-10 * fx[pre + "W_evals"][-1]


def test_p2p_tree_is_always_on_the_samples():
    """the reference's quirk: with a subsample and complete=True the tree of edge (i, j) holds the SAMPLED rows of mesh i"""
    fx, meshes, edges, maps0, samples = ff.load()
    net = _host_net(True)
    net.set_weights(weight_type="adjacency")
    net.compute_CCLB(9)
    net.compute_p2p(complete=True)
    for (i, j) in edges:
        p = net.p2p[(i, j)]
        assert p.shape == (meshes[j].n_vertices,) and p.max() < samples.shape[1]
        tree, query = net.get_LB(i, complete=False), net.get_LB(j, complete=True)
        assert tree.shape[0] == samples.shape[1]
        d2 = ((query[:, None, :] - tree[None, :, :]) ** 2).sum(-1)
        assert np.array_equal(p, d2.argmin(axis=1))


def test_host_subsample_and_shape_differences():
    fx, meshes, edges, maps0, samples = ff.load()
    net = _host_net(False)
    net.compute_subsample(size=96, geodesic=False, starts=[0] * 5)
    assert np.array_equal(net.subsample, samples)
    net.set_weights(weight_type="adjacency")
    net.compute_CCLB(9)
    area, conf = zip(*(net.get_CSD(i) for i in range(5)))
    Y = net.CCLB
    assert all(np.array_equal(area[i], Y[i].T @ Y[i]) for i in range(5))
    assert np.abs(sum(area) - 5 * np.eye(9)).max() <= 1e-12 * 5                       # sum_i Y_i^T Y_i = n I: Q is orthogonal
    # sum_i Y_i^T diag(lambda_i) Y_i = n diag(theta); theta_0 = 0 (the constant functions) is cut by the pseudo-inverse
    assert np.abs(sum(conf)[1:, 1:] - 5 * np.eye(8)).max() <= 1e-9 and np.abs(sum(conf)[0]).max() <= 1e-9


def test_last_mesh_without_an_edge_is_refused():
    from densematcher_amd.pyFM import FMN
    fx, meshes, edges, maps0, samples = ff.load()
    net = FMN(list(meshes) + [meshes[0]], maps_dict=maps0, device=False)
    net.set_weights(weight_type="adjacency")
    with pytest.raises(ValueError, match="max\\(edges\\)"):
        net.compute_W(M=ff.M0)


def test_unknown_weight_type_and_exports():
    import densematcher_amd.pyFM as pyFM
    assert isinstance(pyFM.FMN, type) and callable(pyFM.CLB_quad_form)
    with pytest.raises(ValueError):
        _host_net(False).set_weights(weight_type="other")


# ---- the C ABI of the device route (in the manner of test_fps_abi_cpu.py)
@pytest.fixture(scope="module")
def lib():
    from densematcher_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_new_symbols_declared_bound_and_exported(lib):
    from densematcher_amd import _lib
    hdr = open(os.path.join(REPO, "include", "densematch.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert name in declared, name
        assert hasattr(lib, name), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [6, 8, 9, 14, 9]


def test_option_exists():
    from densematcher_amd.engine import MatchEngine
    assert MatchEngine.OPTION_DEFAULTS["fmn_eig_route"] == 0
    assert '"fmn_eig_route"' in open(os.path.join(REPO, "include", "densematch.h")).read()
    assert "fmn_eig_route" in MatchEngine.set_option.__doc__
    assert all(hasattr(MatchEngine, n) for n in ("eigh_smallest", "fmn_orth_defect", "fmn_cycle_costs", "fmn_quad_form", "fmn_cclb"))


def test_null_context_is_refused(lib):
    assert lib.dm_fmn_orth_defect(None, 1, 4, None, 4, None) != 0
    assert lib.dm_fmn_cycle_costs(None, 3, 4, None, 4, 1, None, None) != 0
    assert lib.dm_fmn_quad_form(None, 2, 1, 4, None, 4, None, None, None) != 0
    assert lib.dm_eigh_smallest(None, 1, 8, None, 8, 2, 2, 1, 8, 0, None, None, None, None) != 0
    assert lib.dm_fmn_cclb(None, 2, 4, 3, None, None, 4, None, None) != 0

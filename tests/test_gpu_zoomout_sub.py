"""GPU: subsampled ZoomOut as one device loop (dm_zoomout_sub: one Cholesky factor of Phi2[sub2]^T Phi2[sub2] for all iterations)
against the oracle's scipy.linalg.lstsq trajectory (oracle.dm_oracle.zoomout_refine(subsample=...)) at full length, in batches,
against the host-chained path it replaces, through the pyFM-shaped surface, and failing closed."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import dm_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    e = default_engine()
    yield e
    e.reset_options()


def samples(seed, ns, n=2048):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n, ns)), np.sort(rng.choice(n, ns + 32))


_ORACLE = {}


def oracle_cfg4(fx, seed, ns):
    """the oracle's run on fx_cfg4 with the samples of `seed` (cached: every test compares against the same trajectory)"""
    if (seed, ns) not in _ORACLE:
        sub = samples(seed, ns)
        _ORACLE[(seed, ns)] = orc.zoomout_refine(fx["C0"], fx["Phi1"].astype(np.float64), fx["Phi2"].astype(np.float64), nit=int(fx["nit"]),
                                                 step=1, subsample=sub, return_p2p=True)
    return _ORACLE[(seed, ns)]


def mesh_of(fx, which, k=None):
    from densematcher_amd.pyFM.mesh import TriMesh
    m = TriMesh(fx[f"verts{which}"], fx[f"faces{which}"])
    kk = fx[f"Phi{which}"].shape[1] if k is None else k
    m.A = sp.diags(fx[f"a{which}"].astype(np.float64)).tocsr()
    m.W = sp.identity(m.n_vertices).tocsr()
    m.eigenvalues = fx[f"lam{which}"][:kk].copy()
    m.eigenvectors = fx[f"Phi{which}"][:, :kk].astype(np.float64)
    return m


@pytest.mark.parametrize("ns", [512, 1024])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_full_length_against_the_oracle(eng, fx_cfg4, ns, dtype):
    """fx_cfg4, 50 -> 200 in 150 iterations on the samples of seed 7: the full-vertex map identical (every vertex compared),
    max |C - C_oracle| <= 1e-9 (the tolerance of test_config4_zoomout_full_length_against_reference).  Measured on MI355X without
    any refinement step: 5.6e-15 (ns = 512) and 2.3e-15 (ns = 1024) for both dtypes, 0 of 2048 vertices differ."""
    fx = fx_cfg4
    sub = samples(7, ns)
    Co, po = oracle_cfg4(fx, 7, ns)
    C, p = eng.zoomout(fx["Phi1"].astype(dtype)[None], fx["Phi2"].astype(dtype)[None], None, fx["C0"][None], nit=int(fx["nit"]), step=1,
                       return_p2p=True, subsample=sub)
    C, p = C[0].cpu().numpy(), p[0].cpu().numpy()
    err = np.abs(C - Co).max()
    print(f"ns {ns} {np.dtype(dtype).name}: max |C - C_oracle| = {err:.3e}, vertices that differ: {int(np.count_nonzero(p != po))} of {len(po)}")
    assert p.shape == po.shape == (2048,)
    assert np.array_equal(p, po)
    assert err <= 1e-9


def test_batch_of_eight_sample_sets_bitwise(eng, fx_cfg4):
    """8 copies of the pair with 8 sample seeds in one call: every pair equals its own single-pair call bit for bit, pair 0 the oracle"""
    fx = fx_cfg4
    B, ns = 8, 512
    subs = [samples(7 + q, ns) for q in range(B)]
    sub1 = np.stack([s[0] for s in subs])
    sub2 = np.stack([s[1] for s in subs])
    Phi1 = np.repeat(fx["Phi1"].astype(np.float64)[None], B, 0)
    Phi2 = np.repeat(fx["Phi2"].astype(np.float64)[None], B, 0)
    C0 = np.repeat(fx["C0"][None], B, 0)
    Cb, pb = eng.zoomout(Phi1, Phi2, None, C0, nit=int(fx["nit"]), step=1, return_p2p=True, subsample=(sub1, sub2))
    for q in range(B):
        C1, p1 = eng.zoomout(Phi1[:1], Phi2[:1], None, C0[:1], nit=int(fx["nit"]), step=1, return_p2p=True, subsample=subs[q])
        assert torch.equal(C1[0], Cb[q]) and torch.equal(p1[0], pb[q]), q
    Co, po = oracle_cfg4(fx, 7, ns)
    assert np.array_equal(pb[0].cpu().numpy(), po)
    assert np.abs(Cb[0].cpu().numpy() - Co).max() <= 1e-9
    assert not torch.equal(Cb[0], Cb[1])                       # (other samples, another map)


def test_device_loop_against_host_chained_path(eng, fx_cfg1, fx_cfg4):
    """zoomout_sub_fused = 0 (the search and dm_p2p_to_fm_lstsq chained from the host) against 1: maps equal, C within 1e-9"""
    from densematcher_amd.pyFM import refine
    fx = fx_cfg1
    e1, e2 = fx["Phi1"].astype(np.float64), fx["Phi2"].astype(np.float64)
    rng = np.random.default_rng(3)
    cases = [(fx["C20"], e1, e2, 6, 2, (np.sort(rng.choice(500, 300, replace=False)), np.sort(rng.choice(500, 320, replace=False)))),
             (fx_cfg4["C0"], fx_cfg4["Phi1"].astype(np.float64), fx_cfg4["Phi2"].astype(np.float64), int(fx_cfg4["nit"]), 1, samples(7, 512))]
    for C0, p1, p2, nit, step, sub in cases:
        res = {}
        try:
            for mode in (0, 1):
                eng.set_option("zoomout_sub_fused", mode)
                eng.profile_kernel("*")
                res[mode] = refine.zoomout_refine(C0, p1, p2, nit=nit, step=step, subsample=sub, return_p2p=True)
                names = set(eng.profile_report())
                eng.profile_kernel(None)
                assert ("zo_sub_solve" in names) == (mode == 1), names         # (the option really switches the path)
        finally:
            eng.set_option("zoomout_sub_fused", 1)
            eng.profile_kernel(None)
        assert np.array_equal(res[0][1], res[1][1])
        assert np.abs(res[0][0] - res[1][0]).max() <= 1e-9


def test_rectangular_and_two_step_calls_stay_host_chained(eng, fx_cfg1):
    from densematcher_amd.pyFM import refine
    fx = fx_cfg1
    e1, e2 = fx["Phi1"].astype(np.float64), fx["Phi2"].astype(np.float64)
    rng = np.random.default_rng(4)
    sub = (np.sort(rng.choice(500, 300, replace=False)), np.sort(rng.choice(500, 320, replace=False)))
    for C0, step in ((fx["C20"], (2, 3)), (fx["C20"][:, :16], 2)):
        eng.profile_kernel("*")
        C, p = refine.zoomout_refine(C0, e1, e2, nit=4, step=step, subsample=sub, return_p2p=True)
        names = set(eng.profile_report())
        eng.profile_kernel(None)
        assert "zo_sub_solve" not in names
        Co, po = orc.zoomout_refine(C0, e1, e2, nit=4, step=step, subsample=sub, return_p2p=True)
        assert C.shape == Co.shape and np.abs(C - Co).max() < 1e-8 and np.array_equal(p, po)


def test_launches_per_iteration(eng, fx_cfg4):
    """the loop's launch count, from the library's own profile: at most 8 per iteration (5 search, 1 product, 1 solve here)"""
    fx = fx_cfg4
    nit = 40
    eng.profile_kernel("*")
    eng.zoomout(fx["Phi1"].astype(np.float64)[None], fx["Phi2"].astype(np.float64)[None], None, fx["C0"][None], nit=nit, step=1,
                subsample=samples(7, 512))
    rep = eng.profile_report(kernels=True)
    eng.profile_kernel(None)
    once = {"zo_sub_gather", "zo_sub_iota_ones", "zo_sub_factor", "p2pfm_prescale", "zo_copy_mat"}
    per_it = sum(n for name, (n, _, _) in rep.items() if n >= nit)
    print({name: v[0] for name, v in rep.items()})
    assert rep["zo_sub_solve"][0] == nit and rep["zo_sub_factor"][0] == 1
    assert per_it <= 8 * nit + 8
    assert all(rep[name][0] <= 3 for name in once if name in rep)


def test_mesh_zoomout_refine_p2p_with_subsamples(eng, fx_cfg1):
    from densematcher_amd.pyFM import refine
    fx = fx_cfg1
    m1, m2 = mesh_of(fx, 1), mesh_of(fx, 2)
    e1, e2 = m1.eigenvectors, m2.eigenvectors
    rng = np.random.default_rng(8)
    sub = (np.sort(rng.choice(500, 300, replace=False)), np.sort(rng.choice(500, 320, replace=False)))
    # subsample = (sub1, sub2): the initial map from the full vertex map with the mass (zoomout.py:211), the loop on the samples
    C, p = refine.mesh_zoomout_refine_p2p(fx["knn21"], m1, m2, 20, nit=6, step=2, subsample=sub, return_p2p=True)
    C0 = orc.p2p_to_fm(fx["knn21"], e1[:, :20], e2[:, :20], fx["a2"])
    Co, po = orc.zoomout_refine(C0, e1, e2, nit=6, step=2, subsample=sub, return_p2p=True)
    assert np.abs(C - Co).max() < 1e-8 and np.array_equal(p, po)
    # p2p_on_sub: a map between the samples, the initial map by least squares on the sampled rows (zoomout.py:209)
    p_sub = orc.knn_query(e1[sub[0]][:, :20] @ fx["C20"].T, e2[sub[1]][:, :20])
    C, p = refine.mesh_zoomout_refine_p2p(p_sub, m1, m2, 20, nit=6, step=2, subsample=sub, return_p2p=True, p2p_on_sub=True)
    C0 = orc.p2p_to_fm(p_sub, e1[sub[0]][:, :20], e2[sub[1]][:, :20], None)
    Co, po = orc.zoomout_refine(C0, e1, e2, nit=6, step=2, subsample=sub, return_p2p=True)
    assert np.abs(C - Co).max() < 1e-8 and np.array_equal(p, po)
    # subsample = int: farthest-point samples of both meshes (the default sampler warns about its distance)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        C, p = refine.mesh_zoomout_refine_p2p(fx["knn21"], m1, m2, 20, nit=3, step=2, subsample=120, return_p2p=True)
    assert C.shape == (26, 26) and p.shape == (500,) and np.isfinite(C).all() and p.min() >= 0 and p.max() < 500
    with pytest.raises(ValueError, match="undefined subsample"):
        refine.mesh_zoomout_refine_p2p(fx["knn21"], m1, m2, 20, nit=3, step=2, subsample=120, p2p_on_sub=True)


def test_fails_closed(eng, fx_cfg1):
    from densematcher_amd._lib import DenseMatchError
    fx = fx_cfg1
    P1, P2 = fx["Phi1"].astype(np.float64)[None], fx["Phi2"].astype(np.float64)[None]
    C0 = fx["C20"][None]
    good1 = np.arange(0, 500, 2)
    with pytest.raises(DenseMatchError):                       # duplicated samples: Phi2[sub2] has rank 3
        eng.zoomout(P1, P2, None, C0, nit=6, step=2, subsample=(good1, np.repeat(np.array([4, 9, 200]), 100)))
    with pytest.raises(DenseMatchError):                       # fewer samples than kf = 32
        eng.zoomout(P1, P2, None, C0, nit=6, step=2, subsample=(good1, np.arange(25) * 7))
    for bad in (np.array([0, 1, 500]), np.array([-1, 3, 4])):
        with pytest.raises(ValueError):
            eng.zoomout(P1, P2, None, C0, nit=6, step=2, subsample=(np.concatenate([good1, bad]), good1))
        with pytest.raises(ValueError):
            eng.zoomout(P1, P2, None, C0, nit=6, step=2, subsample=(good1, np.concatenate([good1, bad])))
    # the device is still healthy, and a good pair beside a bad one in the same call is reported per pair
    C = eng.zoomout(P1, P2, None, C0, nit=6, step=2, subsample=(good1, good1))
    Co = orc.zoomout_refine(fx["C20"], P1[0], P2[0], nit=6, step=2, subsample=(good1, good1))
    assert np.abs(C[0].cpu().numpy() - Co).max() < 1e-8

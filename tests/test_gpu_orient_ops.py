"""
GPU (-m gpu): the orientation operators on the device (dm_fmap_orient_ops -> MatchEngine.orientation_ops) and the layers above:
FunctionalMapping.compute_orientation_op(route="device"), fit(orient_route="device"), w_orient in compute_surface_map_batch.

References: the reference's own operators and fit (tests/golden/fx_cfg1_shape_terms.npz) and the oracle's restatement
(orc.orientation_ops, pinned to them in test_oracle_golden.py).  Bound on the operators: 1e-11 max|op|, the bound the oracle itself is
held to there -- a float64 sum in another order lands within about 1e-14 max|op| (sum |terms| / max|op| ~ 40 on the fixture).
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import dm_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-11
NOTEBOOK = dict(w_descr=1e4, w_lap=1e3, w_dcomm=0, w_ent=1e-1, w_sumto1=1e1, optinit="zeros", maxiter=5000)   # example.ipynb cell 11


class _Duck:
    """what compute_surface_map needs from a pytorch3d Meshes (reference functional_map.py:17-18)"""
    def __init__(self, v, f):
        import torch
        self.v, self.f = torch.tensor(v), torch.tensor(f)

    def verts_list(self):
        return [self.v]

    def faces_list(self):
        return [self.f]


def _mesh(fx, which, k=None):
    from densematcher_amd.pyFM.mesh import TriMesh
    m = TriMesh(fx[f"verts{which}"], fx[f"faces{which}"])
    kk = fx[f"Phi{which}"].shape[1] if k is None else k
    m.A = sp.diags(fx[f"a{which}"].astype(np.float64)).tocsr()
    m.W = sp.identity(m.n_vertices).tocsr()            # not used by the matching path
    m.eigenvalues = fx[f"lam{which}"][:kk].copy()
    m.eigenvectors = fx[f"Phi{which}"][:, :kk].astype(np.float64)
    return m


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def _device_ops(eng, verts, faces, Phi, F, k, row_scale=None):
    return eng.orientation_ops(verts[None], faces[None], Phi[None], F[None], k=k, row_scale=None if row_scale is None else row_scale[None])[0]


def _oracle_ops(verts, faces, Phi, F, k, row_scale=None):
    """orc.orientation_ops on the values the kernel reads; its left factor is phi * (mass / vertex_areas): row_scale goes in as mass / 1"""
    n = Phi.shape[0]
    mass = np.ones(n) if row_scale is None else np.asarray(row_scale, np.float64)
    return orc.orientation_ops(Phi[:, :k].astype(np.float64), mass, verts, faces, F.astype(np.float64), vertex_areas=None if row_scale is None else np.ones(n))


def _close(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    err, sc = np.abs(got - want).max(), np.abs(want).max()
    print("max |op - ref| = %.2e of max |op| = %.2e" % (err, sc))
    return err <= TOL * sc


# --------------------------------------------------------------------------- 1. the kernel against the reference's operators
@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("which", [1, 2])
def test_kernel_against_reference_operators(eng, fx_cfg1, fx_cfg1_shape_terms, which, real):
    """fixture meshes (N = 500, m = 1000), k = 30 of the 48 stored columns (row stride != k), the fixture's 6 descriptors: the "vertex" form
    against the reference's compute_orientation_op output, the "mass" form against the oracle and the reference's float32 operators"""
    fx, ft = fx_cfg1, fx_cfg1_shape_terms
    k, nd = int(fx["k"]), int(ft["ndesc"])
    assert k == 30 and fx[f"Phi{which}"].shape[1] == 48 and nd == 6
    verts, faces = fx[f"verts{which}"], fx[f"faces{which}"]
    Phi = fx[f"Phi{which}"].astype(real)
    F = fx[f"F{which}"][:, :nd].astype(np.float32)
    a = fx[f"a{which}"].astype(np.float64)
    o_np = _device_ops(eng, verts, faces, Phi, F, k, row_scale=a / ft[f"vertex_areas{which}"])
    assert _close(o_np, ft[f"orient_np_op{which}"])
    o_t = _device_ops(eng, verts, faces, Phi, F, k).cpu().numpy()
    assert _close(o_t, orc.orientation_ops(Phi[:, :k].astype(np.float64), a, verts, faces, F.astype(np.float64)))
    assert np.abs(o_t - ft[f"orient_t_op{which}"]).max() <= 5e-6 * np.abs(ft[f"orient_np_op{which}"]).max()   # (the reference's float32 side)


# --------------------------------------------------------------------------- 2. shapes at which it can go wrong
@pytest.mark.parametrize("k,D,fdt", [(15, 6, np.float32), (1, 6, np.float32), (30, 1, np.float32), (30, 128, np.float16), (48, 128, np.float16)])
def test_kernel_shapes_on_fixture(eng, fx_cfg1, k, D, fdt):
    """k = 15 (four descriptors per 64-row tile), k = 1; D = 1, D = 128 (every fixture column, fp16 as staged for the fit; with k = 48 the
    K chunk is three times the smallest one)"""
    fx = fx_cfg1
    verts, faces = fx["verts1"], fx["faces1"]
    Phi = np.ascontiguousarray(fx["Phi1"][:, 1:]) if k == 1 else fx["Phi1"]      # (column 0 is constant: its operators are zero)
    F = fx["F1"][:, :D].astype(fdt)
    rs = 0.5 + np.random.default_rng(3).random(Phi.shape[0])
    assert _close(_device_ops(eng, verts, faces, Phi, F, k, row_scale=rs), _oracle_ops(verts, faces, Phi, F, k, row_scale=rs))


def _closed_mesh(n, seed):
    """convex hull of n points on the sphere: a closed mesh of 2 n - 4 faces"""
    from scipy.spatial import ConvexHull
    p = np.random.default_rng(seed).standard_normal((n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    f = ConvexHull(p).simplices.astype(np.int64)
    flip = np.einsum("ij,ij->i", np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), p[f[:, 0]]) < 0
    f[flip] = f[flip][:, ::-1]
    return p, f


@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_kernel_small_closed_mesh(eng, real):
    """37 vertices, 70 faces: 210 K rows, no multiple of the 16-row stage; one K split (the product writes the operators itself)"""
    verts, faces = _closed_mesh(37, 0)
    assert faces.shape == (70, 3)
    rng = np.random.default_rng(1)
    Phi = rng.standard_normal((37, 9)).astype(real)
    F = rng.standard_normal((37, 5)).astype(np.float32)
    assert _close(_device_ops(eng, verts, faces, Phi, F, 7), _oracle_ops(verts, faces, Phi, F, 7))


def test_kernel_many_k_splits(eng):
    """a torus of 1200 vertices, 2400 faces: 7200 K rows in 15 chunks of 512 whose partials the fixed-order reduction adds"""
    from densematcher_amd import synth
    verts, faces = synth.torus_mesh(40, 30, perturb=0.1, seed=2)
    rng = np.random.default_rng(2)
    Phi = rng.standard_normal((1200, 20)).astype(np.float32)
    F = rng.standard_normal((1200, 3)).astype(np.float16)
    assert _close(_device_ops(eng, verts, faces, Phi, F, 20), _oracle_ops(verts, faces, Phi, F, 20))


@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_batch_of_padded_meshes_equals_solo_calls(eng, real):
    """three meshes of 120 vertices with 240 / 233 / 140 faces in one call, padded to 240 rows: each equals its solo call bit for bit
    (what the batched fit's equality with the single call rests on) and the oracle; the padding rows hold a valid triangle that would
    change the sums if it were read"""
    import torch
    from densematcher_amd import synth
    N, k, D = 120, 11, 7
    rng = np.random.default_rng(5)
    meshes = []
    for q, nf in enumerate((240, 233, 140)):
        verts, faces = synth.torus_mesh(12, 10, perturb=0.05 * (q + 1), seed=q)
        meshes.append((verts, faces[rng.permutation(240)[:nf]]))
    Phi = rng.standard_normal((3, N, k + 2)).astype(real)
    F = rng.standard_normal((3, N, D)).astype(np.float16)
    rs = 0.5 + rng.random((3, N))
    faces = np.empty((3, 240, 3), dtype=np.int64)
    faces[:] = np.array([5, 6, 17])
    for q, (_, f) in enumerate(meshes):
        faces[q, :len(f)] = f
    nf = [len(f) for _, f in meshes]
    got = eng.orientation_ops(np.stack([v for v, _ in meshes]), faces, Phi, F, k=k, row_scale=rs, n_faces=nf)
    for q, (v, f) in enumerate(meshes):
        solo = eng.orientation_ops(v[None], f[None], Phi[q:q + 1], F[q:q + 1], k=k, row_scale=rs[q:q + 1])
        assert torch.equal(got[q], solo[0]), q
        assert _close(got[q], _oracle_ops(v, f, Phi[q], F[q], k, row_scale=rs[q]))


# --------------------------------------------------------------------------- 3. input errors never launch
def test_input_errors(eng, fx_cfg1):
    from densematcher_amd.pyFM.functional import FunctionalMapping
    fx = fx_cfg1
    verts, faces, Phi = fx["verts1"], fx["faces1"].copy(), fx["Phi1"]
    F = fx["F1"][:, :2]
    faces[17, 1] = Phi.shape[0]
    with pytest.raises(ValueError, match="face index"):
        _device_ops(eng, verts, faces, Phi, F, 30)
    faces[17, 1] = -1
    with pytest.raises(ValueError, match="face index"):
        _device_ops(eng, verts, faces, Phi, F, 30)
    with pytest.raises(ValueError, match="row stride"):
        _device_ops(eng, verts, fx["faces1"], Phi, F, Phi.shape[1] + 1)
    model = FunctionalMapping(_mesh(fx, 1, 30), _mesh(fx, 2, 30), partial=False, optimizer="L-BFGS-B")
    model.preprocess(n_ev=(30, 30), n_descr=2, descr1=fx["F1"][:, :2], descr2=fx["F2"][:, :2], subsample_step=1)
    with pytest.raises(NotImplementedError):
        model.compute_orientation_op(route="device", normalize=True)
    with pytest.raises(ValueError, match="route"):
        model.compute_orientation_op(route="x")
    with pytest.raises(ValueError, match="orient_route"):
        model.fit(w_descr=1e4, w_lap=1e3, w_dcomm=0, w_orient=1, orient_route="x")


# --------------------------------------------------------------------------- 4. compute_orientation_op(route="device")
def _model(fx, ft):
    from densematcher_amd.pyFM.functional import FunctionalMapping
    k, nd = int(fx["k"]), int(ft["ndesc"])
    model = FunctionalMapping(_mesh(fx, 1, k), _mesh(fx, 2, k), partial=False, optimizer="L-BFGS-B")
    model.preprocess(n_ev=(k, k), n_descr=nd, descr1=fx["F1"][:, :nd].astype(np.float64), descr2=fx["F2"][:, :nd].astype(np.float64), subsample_step=1)
    return model


@pytest.mark.parametrize("area", ["vertex", "mass"])
def test_compute_orientation_op_device_route(fx_cfg1, fx_cfg1_shape_terms, area):
    model = _model(fx_cfg1, fx_cfg1_shape_terms)
    host = model.compute_orientation_op(area=area)
    dev = model.compute_orientation_op(area=area, route="device")
    assert len(dev) == len(host) == int(fx_cfg1_shape_terms["ndesc"])
    for side in (0, 1):
        assert dev[0][side].shape == host[0][side].shape
        assert _close(np.stack([o[side] for o in dev]), np.stack([o[side] for o in host]))
    rev = model.compute_orientation_op(area=area, route="device", reversing=True)
    for (a, b), (ar, br) in zip(dev, rev):
        assert np.array_equal(ar, a) and np.array_equal(br, -b)


# --------------------------------------------------------------------------- 5. fit(orient_route="device")
def test_fit_device_route_against_reference_fit(fx_cfg1, fx_cfg1_shape_terms):
    """the reference's fit with w_orient / w_area / w_conformal (the call of test_gpu_api.py's orientation test) with the operators from the
    device: within the reference fit's float32 noise floor of its map.  The distance to the host route's map is printed, not asserted:
    it depends on where two L-BFGS runs on last-bit different operators stop."""
    ft = fx_cfg1_shape_terms
    model = _model(fx_cfg1, ft)
    call = dict(w_descr=1e4, w_lap=1e3, w_dcomm=0, w_orient=1, w_area=1e2, w_conformal=1e2, optinit="zeros", stopping="tight")
    model.fit(**call, orient_route="device")
    C_dev, w_dev = model.FM.copy(), model.w_orient_rescaled
    d = np.abs(C_dev - ft["fit_orient_C"]).max()
    model.fit(**call)
    print("fit, orient_route='device': |C - C_reference| = %.2e; |C_device - C_host| = %.2e; rescaled w_orient device %.17g, host %.17g"
          % (d, np.abs(C_dev - model.FM).max(), w_dev, model.w_orient_rescaled))
    assert d <= 5e-3


# --------------------------------------------------------------------------- 6. w_orient in compute_surface_map_batch
@pytest.mark.parametrize("route,reversing", [("device", False), ("device", True), ("host", False)])
def test_surface_map_batch_with_orientation_term(fx_cfg1, monkeypatch, route, reversing):
    """four pairs of the fixture meshes (the pair, the swapped pair, the pair with other descriptor columns, and the pair with one face of
    mesh 2 dropped: the same group, so mesh 2's faces are padded and n_faces differs inside it), n_ev = 15, w_orient = 1 with
    the notebook's other weights: every integer map and both functional maps of the batched call equal the single call's -- with
    orient_route="device" the single call on the same route, with "host" today's default single call.  Equal operators enter kernels
    whose per-pair results do not depend on the batch; nothing is compared across routes."""
    from densematcher_amd.functional_map import compute_surface_map, compute_surface_map_batch
    from densematcher_amd.pyFM.mesh import TriMesh
    fx = fx_cfg1
    k = 15
    by_verts = [(fx["verts1"], 1), (fx["verts2"], 2)]

    def process(self, k=200, **kw):
        for vv, which in by_verts:
            if np.array_equal(self.vertlist, vv):
                src = _mesh(fx, which, k)
                self.W, self.A, self.eigenvalues, self.eigenvectors = src.W, src.A, src.eigenvalues, src.eigenvectors
                return self
        raise RuntimeError("unknown mesh")

    monkeypatch.setattr(TriMesh, "process", process)
    m1, m2 = (fx["verts1"], fx["faces1"]), (fx["verts2"], fx["faces2"])
    pairs = [(_Duck(*m1), _Duck(*m2), fx["F1"][:, :16], fx["F2"][:, :16]),
             (_Duck(*m2), _Duck(*m1), fx["F2"][:, :16], fx["F1"][:, :16]),
             (_Duck(*m1), _Duck(*m2), fx["F1"][:, 16:32], fx["F2"][:, 16:32]),
             (_Duck(*m1), _Duck(m2[0], m2[1][:-1]), fx["F1"][:, :16], fx["F2"][:, :16])]
    fit = dict(NOTEBOOK, w_orient=1, orient_reversing=reversing)
    kw = dict(n_ev=k, compute_extra=True, optimizer="L-BFGS-B")
    got = compute_surface_map_batch([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], [p[3] for p in pairs],
                                    fit_params=dict(fit, orient_route=route), **kw)
    for q, p in enumerate(pairs):
        want = compute_surface_map(*p, fit_params=dict(fit, orient_route="device") if route == "device" else fit, **kw)
        assert got[q][7].w_orient_rescaled == want[7].w_orient_rescaled, q
        assert np.array_equal(got[q][7]._FM_base, want[7]._FM_base), q
        assert np.array_equal(got[q][7].FM, want[7].FM), q                    # (the ICP map)
        for slot in (0, 1, 4, 5, 10, 11, 12, 13):
            assert np.array_equal(got[q][slot], want[slot]), (q, slot)
        for slot in (2, 3, 6):
            assert np.array_equal(got[q][slot][0], want[slot][0]) and np.array_equal(got[q][slot][1], want[slot][1]), (q, slot)

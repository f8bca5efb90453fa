"""
CPU: the DiffusionNet operators (densematcher_amd.diffusion_net.geometry, reference diffusion_net/geometry.py:151-570) on the host route
against the reference's own frames and gradients (tests/golden/fx_dnet.npz, tools/make_golden_dnet.py), the cache's file format in
both directions, and the plain torch helpers.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import dnet_checks as dc
from densematcher_amd.diffusion_net import geometry as geo
from densematcher_amd.diffusion_net import _host


@pytest.mark.parametrize("key", ["t", "f", "u", "r", "g"])
def test_host_route_against_the_golden(key):
    """frames, gradX, gradY, L, massvec of every mesh, float64; u takes the normal-repair path (one unreferenced vertex), g has exact
    zero cotangents whose neighbours stay in the gradient rows"""
    verts, faces = dc.mesh(key)
    k = 0 if key in ("u", "g") else int(dc.golden()["k_eig"])
    ops = geo.compute_operators(verts, faces, k, route="host")
    assert all(o.dtype == torch.float64 for o in ops)
    assert ops[2].is_sparse and ops[2].is_coalesced() and ops[5].is_coalesced() and ops[6].is_coalesced()
    dc.check_against_golden(ops, key, tag="host")
    if k == 0:
        assert ops[3].shape == (0,) and ops[4].shape == (verts.shape[0], 0)


@pytest.mark.parametrize("key", ["t", "f", "r"])
def test_host_spectrum(key):
    verts, faces = dc.mesh(key)
    ops = geo.compute_operators(verts, faces, int(dc.golden()["k_eig"]), route="host")
    dc.check_spectrum(ops, dc.golden()[f"evals_{key}"], tag=f"host {key}")


def test_given_normals_and_float32_input():
    """normals= replaces the computed ones; float32 input is widened, computed in float64 and rounded once"""
    verts, faces = dc.mesh("t")
    n = torch.from_numpy(dc.ref_array("t", "frames")[:, 2, :].copy())
    a = geo.compute_operators(verts, faces, 0, normals=n, route="host")
    dc.check_against_golden(a, "t", tag="given normals")
    v32 = verts.float()
    b = geo.compute_operators(v32, faces, 4, route="host")
    assert all(o.dtype == torch.float32 for o in b)
    c = geo.compute_operators(v32.double(), faces, 4, route="host")
    for x, y, name in zip(b, c, dc.NAMES):
        if name not in ("evals", "evecs"):
            assert np.array_equal(dc.dense(x), dc.dense(y).astype(np.float32).astype(np.float64)), name


def test_named_pieces_match_the_operators():
    """build_tangent_frames, edge_tangent_vectors and build_grad chained as compute_operators chains them in the reference"""
    verts, faces = dc.mesh("f")
    frames = geo.build_tangent_frames(verts, faces)
    assert np.abs(frames.numpy() - dc.ref_array("f", "frames")).max() <= 1e-13
    fx = dc.golden()
    edges = torch.from_numpy(np.stack((fx["L_row_f"], fx["L_col_f"])).astype(np.int64))
    G = geo.build_grad(verts, edges, geo.edge_tangent_vectors(verts, frames, edges))
    for part, name in ((G.real, "gradX"), (G.imag, "gradY")):
        ref = dc.ref_array("f", name)
        assert np.abs(part.toarray() - ref).max() <= 1e-11 * np.abs(ref).max()
    assert np.abs(geo.vertex_normals(verts, faces).numpy() - dc.ref_array("f", "frames")[:, 2]).max() <= 1e-13


def test_errors_keep_the_reference_wording():
    verts, faces = dc.mesh("g")
    with pytest.raises(NotImplementedError):
        geo.compute_operators(verts, faces[:0], 0, route="host")
    bad = torch.full((verts.shape[0], 3), float("nan"), dtype=torch.float64)
    with pytest.raises(ValueError, match="NaN coordinate frame! Must be very degenerate"):
        geo.compute_operators(verts, faces, 0, normals=bad, route="host")
    with pytest.raises(RuntimeError, match="NaN verts"):
        geo.get_operators(verts * float("nan"), faces, 0)
    with pytest.raises(ValueError, match="route"):
        geo.compute_operators(verts, faces, 0, route="fast")


def _same(a, b):
    return all(np.array_equal(dc.dense(x), dc.dense(y)) for x, y in zip(a, b))


def test_cache_round_trip(tmp_path, monkeypatch):
    """a file written by get_operators loads back equal to what was computed, after the float32 store (float32 vertices, the
    reference's usual input: it compares the input with the stored float32 vertices, so other float64 inputs never hit)"""
    monkeypatch.setattr(geo, "compute_operators", lambda v, f, k, normals=None: geo._compute_many([v], [f], k, None, "host")[0])
    verts, faces = dc.mesh("t", dtype=torch.float32)
    first = geo.get_operators(verts, faces, k_eig=8, op_cache_dir=str(tmp_path))
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == [geo.utils.hash_arrays((verts.numpy(), faces.numpy())) + "_0.npz"]
    monkeypatch.setattr(geo, "compute_operators", lambda *a, **k: (_ for _ in ()).throw(AssertionError("computed again")))
    again = geo.get_operators(verts, faces, k_eig=8, op_cache_dir=str(tmp_path))
    assert all(o.dtype == torch.float32 for o in again)
    for x, y, name in zip(again, first, dc.NAMES):
        assert np.array_equal(dc.dense(x), dc.dense(y)), name
    fewer = geo.get_operators(verts, faces, k_eig=5, op_cache_dir=str(tmp_path))          # enough pairs in the file: the first five
    assert np.array_equal(dc.dense(fewer[3]), dc.dense(again[3])[:5]) and fewer[4].shape == (160, 5)
    with pytest.raises(AssertionError, match="computed again"):                             # cache_k_eig < k_eig: computed anew
        geo.get_operators(verts, faces, k_eig=9, op_cache_dir=str(tmp_path))
    assert list(tmp_path.iterdir()) == []                                                   # (and the stale entry is gone)


def test_cache_file_in_the_reference_layout_is_returned(tmp_path, monkeypatch):
    """a file assembled here in the reference's layout (geometry.py:548-568: name, keys, dtypes) from fixture arrays is returned without
    computing anything; a colliding file of another mesh in bucket 0 sends the search to bucket 1"""
    monkeypatch.setattr(geo, "compute_operators", lambda *a, **k: (_ for _ in ()).throw(AssertionError("computed")))
    fx = dc.golden()
    verts, faces = dc.mesh("r")
    verts_np, faces_np = verts.numpy(), faces.numpy()
    key = geo.utils.hash_arrays((verts_np, faces_np))
    n, k = verts_np.shape[0], 6
    rng = np.random.default_rng(0)
    evecs = rng.standard_normal((n, k))
    entries = {}
    mats = {}
    for name in ("L", "gradX", "gradY"):
        A = sp.coo_matrix((fx[f"{name}_val_r"], (fx[f"{name}_row_r"], fx[f"{name}_col_r"])), shape=(n, n)).tocsc().astype(np.float32)
        mats[name] = A
        entries.update({f"{name}_data": A.data, f"{name}_indices": A.indices, f"{name}_indptr": A.indptr, f"{name}_shape": A.shape})
    np.savez(str(tmp_path / f"{key}_1.npz"), verts=verts_np.astype(np.float32), frames=fx["frames_r"].astype(np.float32), faces=faces_np, k_eig=k,
             mass=fx["mass_r"].astype(np.float32), evals=fx["evals_r"][:k].astype(np.float32), evecs=evecs.astype(np.float32), **entries)
    np.savez(str(tmp_path / f"{key}_0.npz"), verts=verts_np[::-1].astype(np.float32), faces=faces_np, k_eig=k)       # a hash collision
    # (the reference compares the float64 input with the stored float32 vertices: equal only when the input is float32-exact)
    v32 = torch.from_numpy(verts_np.astype(np.float32))
    np.savez(str(tmp_path / f"{geo.utils.hash_arrays((v32.numpy(), faces_np))}_0.npz"), verts=v32.numpy(), frames=fx["frames_r"].astype(np.float32),
             faces=faces_np, k_eig=k, mass=fx["mass_r"].astype(np.float32), evals=fx["evals_r"][:k].astype(np.float32), evecs=evecs.astype(np.float32), **entries)
    out = geo.get_operators(v32, faces, k_eig=4, op_cache_dir=str(tmp_path))
    assert all(o.dtype == torch.float32 for o in out)
    assert np.array_equal(out[0].numpy(), fx["frames_r"].astype(np.float32)) and np.array_equal(out[1].numpy(), fx["mass_r"].astype(np.float32))
    assert np.array_equal(out[3].numpy(), fx["evals_r"][:4].astype(np.float32)) and np.array_equal(out[4].numpy(), evecs.astype(np.float32)[:, :4])
    for q, name in ((2, "L"), (5, "gradX"), (6, "gradY")):
        assert np.array_equal(dc.dense(out[q]), mats[name].toarray().astype(np.float64)), name
    with pytest.raises(AssertionError, match="computed"):          # float64 input: bucket 0 holds other vertices, bucket 1 float32-rounded ones
        geo.get_operators(verts, faces, k_eig=4, op_cache_dir=str(tmp_path))


def test_get_all_operators_lists_and_cache(tmp_path):
    vs, fs = zip(*(dc.mesh(k) for k in ("t", "r", "f")))
    out = geo.get_all_operators(list(vs), list(fs), 3, op_cache_dir=str(tmp_path), route="host")
    assert len(out) == 7 and all(isinstance(o, list) and len(o) == 3 for o in out)
    assert len(list(tmp_path.iterdir())) == 3
    for i, key in enumerate(("t", "r", "f")):
        dc.check_against_golden([o[i] for o in out], key, tag="get_all")
        single = geo.compute_operators(vs[i], fs[i], 3, route="host")
        assert _same([o[i] for o in out][:3], single[:3])


def test_hks_and_basis_helpers():
    g = torch.Generator().manual_seed(1)
    evals = torch.rand(12, generator=g, dtype=torch.float64).sort().values * 5
    evecs = torch.randn(30, 12, generator=g, dtype=torch.float64)
    got = geo.compute_hks_autoscale(evals, evecs, 7)
    scales = torch.logspace(-2, 0.0, steps=7, dtype=torch.float64)
    want = ((evecs * evecs)[:, None, :] * torch.exp(-evals[None, None, :] * scales[None, :, None])).sum(-1)
    assert got.shape == (30, 7) and torch.allclose(got, want, rtol=1e-14, atol=0)
    assert torch.equal(geo.compute_hks(evals[None], evecs[None], scales[None])[0], geo.compute_hks(evals, evecs, scales))
    mass = torch.rand(30, generator=g, dtype=torch.float64)
    vals = torch.randn(30, 4, generator=g, dtype=torch.float64)
    assert torch.equal(geo.to_basis(vals[None], evecs[None], mass[None])[0], evecs.T @ (vals * mass[:, None]))
    assert torch.equal(geo.from_basis(vals[:12], evecs), evecs @ vals[:12])


def test_formulas_against_the_wheel():
    """parity of the closed formulas with potpourri3d itself: unpinned where the wheel is not installed"""
    pp3d = pytest.importorskip("potpourri3d")
    for key in ("t", "f", "r"):
        verts, faces = dc.mesh(key)
        V, F = verts.numpy(), faces.numpy()
        L = pp3d.cotan_laplacian(V, F, denom_eps=1e-10)
        assert np.abs(_host.cotan_laplacian(V, F).toarray() - L.toarray()).max() <= 1e-11 * abs(L).max()
        A = pp3d.vertex_areas(V, F)
        assert np.abs(_host.vertex_areas(V, F) - A).max() <= 1e-13 * A.max()

"""
GPU (-m gpu): the DiffusionNet operators on the device route (dm_dnet_rows / dm_dnet_ell + dm_eigenbasis behind
densematcher_amd.diffusion_net.geometry) against the reference's own frames and gradients (tests/golden/fx_dnet.npz), with the bounds
of the CPU test; batches against single calls; the repair path; the row limit.
"""
import functools

import numpy as np
import pytest
import torch

import dnet_checks as dc
from densematcher_amd.diffusion_net import geometry as geo
from densematcher_amd.diffusion_net import _host

pytestmark = pytest.mark.gpu
K = 16


@functools.lru_cache(maxsize=None)
def single(key, k=K):
    """compute_operators(route="device") of one fixture mesh, computed once and shared"""
    verts, faces = dc.mesh(key)
    return geo.compute_operators(verts, faces, k, route="device")


@pytest.mark.parametrize("key", ["t", "f", "r", "g"])
def test_device_route_against_the_golden(key):
    """f: the valence-40 apex and the boundary vertices are the rows that catch a wrong neighbour loop; r, g: neighbours of (near) zero
    weight stay in the gradient rows"""
    ops = single(key, 0 if key == "g" else K)
    assert all(o.dtype == torch.float64 and o.device.type == "cpu" for o in ops)
    assert ops[2].is_coalesced() and ops[5].is_coalesced() and ops[6].is_coalesced()
    dc.check_against_golden(ops, key, tag="device")


def test_float32_input_against_the_reference_float32_run():
    """|got - ref32| <= (4 f32_floor + 2^-23) max |ref32| per array: the floor is the fixture's measured distance between the reference's
    mixed float32 / float64 arithmetic and float64 arithmetic on the widened input, 2^-23 the final rounding"""
    verts, faces = dc.mesh("t32", dtype=torch.float32)
    ops = geo.compute_operators(verts, faces, K, route="device")
    assert all(o.dtype == torch.float32 for o in ops)
    fx = dc.golden()
    bounds = {name: 4.0 * float(fx["f32_floor_" + {"massvec": "mass"}.get(name, name)]) + 2.0 ** -23 for name in dc.BOUNDS}
    dc.check_against_golden(ops, "t32", bounds=bounds, tag="float32")


def test_repair_path_and_padding(monkeypatch):
    """mesh u (one unreferenced vertex): the device raises the info bit, the host repair is taken, frames equal the golden's; batched with a
    larger partner, no padding row appears in any returned tensor"""
    from densematcher_amd.engine import default_engine
    calls = []
    real = _host.vertex_normals
    monkeypatch.setattr(_host, "vertex_normals", lambda V, F: calls.append(V.shape[0]) or real(V, F))
    verts, faces = dc.mesh("u")
    raw = default_engine().diffusion_operators([verts], [faces], 0)
    assert raw[0]["info"] & 1 and calls == [161]
    assert not torch.isnan(raw[0]["frames"]).any() and not torch.isnan(raw[0]["gx"]).any()
    ops = geo.compute_operators(verts, faces, 0, route="device")
    dc.check_against_golden(ops, "u", tag="device, repaired")
    assert ops[3].shape == (0,) and ops[4].shape == (161, 0)
    assert calls == [161, 161]
    keys = ("g", "u", "f")                                   # 20 / 161 / 81 vertices: g and f ride along padded
    vs, fs = zip(*(dc.mesh(k) for k in keys))
    out = geo.get_all_operators(list(vs), list(fs), 0, route="device")
    assert calls == [161, 161, 161]                          # (only u is repaired)
    for i, key in enumerate(keys):
        n = vs[i].shape[0]
        ops_i = [o[i] for o in out]
        assert ops_i[0].shape == (n, 3, 3) and ops_i[1].shape == (n,) and ops_i[4].shape == (n, 0)
        for q in (2, 5, 6):
            assert tuple(ops_i[q].shape) == (n, n) and int(ops_i[q].indices().max()) < n
        assert sorted(set(ops_i[5].indices()[0].tolist())) == list(range(n))         # every vertex has its g_self entry
        dc.check_against_golden(ops_i, key, tag="device, batched")


def test_batched_call_equals_the_single_calls():
    """get_all_operators on [t, r, f] (160 / 96 / 81 vertices in one call): bit for bit on frames, massvec and the values of L, gradX,
    gradY; eigenvalues to 1e-12 of the largest (what the eigensolver's own tests state across batches)"""
    keys = ("t", "r", "f")
    vs, fs = zip(*(dc.mesh(k) for k in keys))
    out = geo.get_all_operators(list(vs), list(fs), K, route="device")
    for i, key in enumerate(keys):
        one, many = single(key), [o[i] for o in out]
        for q in (0, 1):
            assert torch.equal(one[q], many[q]), (key, dc.NAMES[q])
        for q in (2, 5, 6):
            assert torch.equal(one[q].indices(), many[q].indices()) and torch.equal(one[q].values(), many[q].values()), (key, dc.NAMES[q])
        dev = float((one[3] - many[3]).abs().max() / one[3][-1])
        print(f"mesh {key}: batched against single eigenvalues: {dev:.3e} of the largest (1e-12)")
        assert dev <= 1e-12
        dc.check_spectrum(many, dc.golden()[f"evals_{key}"], tag=f"device, batched {key}")


def test_spectrum_filtered_route():
    """k_eig = 16 at 160 vertices: 2 (k + guard) <= N, the filtered subspace iteration"""
    dc.check_spectrum(single("t"), dc.golden()["evals_t"], tag="device t")
    dc.check_spectrum(single("f"), dc.golden()["evals_f"], tag="device f")


def test_spectrum_dense_route():
    """k_eig = 60 on r (96 vertices): 2 (k + guard) > N, the dense route; eigenvalues against SciPy's dense generalised eigensolver on the
    reference arrays, whose first 16 are the fixture's"""
    import scipy.linalg
    ops = single("r", 60)
    L, mass = dc.ref_array("r", "L"), dc.ref_array("r", "massvec")
    lam = scipy.linalg.eigh(L + 1e-8 * np.eye(96), np.diag(mass), eigvals_only=True)[:60]
    assert np.abs(lam[:K] - dc.golden()["evals_r"]).max() <= 1e-7 * lam[K - 1]
    dc.check_spectrum(ops, lam, tag="device r, dense")


def test_mixed_routes_in_one_batch():
    """k_eig = 16 on [g, t] (20 / 160 vertices): g is too small for the filtered iteration (2 (k + guard) = 64 > 20), t is not.  The
    eigensolver takes each with its own route, so t has the eigenvalues it has alone and g those of SciPy's dense generalised solver"""
    import scipy.linalg
    keys = ("g", "t")
    vs, fs = zip(*(dc.mesh(k) for k in keys))
    out = geo.get_all_operators(list(vs), list(fs), K, route="device")
    t_many, t_one = [o[1] for o in out], single("t")
    dev = float((t_many[3] - t_one[3]).abs().max() / t_one[3][-1])
    print(f"mesh t beside a dense-route mesh: eigenvalues against the single call: {dev:.3e} of the largest (1e-12)")
    assert dev <= 1e-12
    dc.check_spectrum(t_many, dc.golden()["evals_t"], tag="device t, mixed batch")
    L, mass = dc.ref_array("g", "L"), dc.ref_array("g", "massvec")
    lam = scipy.linalg.eigh(L + 1e-8 * np.eye(20), np.diag(mass), eigvals_only=True)[:K]
    dc.check_spectrum([o[0] for o in out], lam, tag="device g, dense in a mixed batch")
    dc.check_against_golden([o[0] for o in out], "g", tag="device g, mixed batch")


def test_abi_refuses_a_width_below_the_longest_row():
    """dm_dnet_ell with nnz < max_row of dm_dnet_rows would drop entries: DM_EINVAL (ValueError), and the context stays usable"""
    import ctypes as C
    from densematcher_amd.engine import default_engine, _ptr
    eng = default_engine()
    verts, faces = dc.mesh("g")
    B, N, nt = 1, verts.shape[0], faces.shape[0]
    tri = faces.to(torch.int32).to(eng.device).contiguous()
    vd = verts.to(eng.device).contiguous()
    rows = torch.empty(int(eng.lib.dm_dnet_rows_bytes(B, N, nt)), dtype=torch.uint8, device=eng.device)
    frames = torch.empty((B, N, 3, 3), dtype=torch.float64, device=eng.device)
    info = torch.empty((B,), dtype=torch.int32, device=eng.device)
    mx = C.c_int(0)
    eng._chk(eng.lib.dm_dnet_rows(eng.ctx, B, N, nt, _ptr(tri), _ptr(vd), None, None, 1e-10, 1e-5, _ptr(rows), _ptr(frames), _ptr(info), C.byref(mx)))
    assert mx.value == 7                                     # an interior grid vertex: six neighbours and itself
    nnz = mx.value - 1
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=eng.device)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=eng.device)
    args = (_ptr(i32(B, N)), _ptr(i32(B, N, nnz)), _ptr(f64(B, N, nnz)), _ptr(f64(B, N, nnz)), _ptr(f64(B, N, nnz)), _ptr(f64(B, N, nnz)),
            _ptr(f64(B, N)), _ptr(torch.empty((B, N), dtype=torch.float32, device=eng.device)))
    with pytest.raises(ValueError, match="narrower than the longest row"):
        eng._chk(eng.lib.dm_dnet_ell(eng.ctx, B, N, nt, _ptr(rows), nnz, None, 1e-8, 1e-8, *args))
    bad_nv = torch.zeros((B,), dtype=torch.int32, device=eng.device)
    with pytest.raises(ValueError, match="n_verts"):
        eng._chk(eng.lib.dm_dnet_rows(eng.ctx, B, N, nt, _ptr(tri), _ptr(vd), None, _ptr(bad_nv), 1e-10, 1e-5, _ptr(rows), _ptr(frames), _ptr(info), C.byref(mx)))
    dc.check_against_golden(geo.compute_operators(verts, faces, 0, route="device"), "g", tag="after the refusals")


def test_row_limit_is_an_error_and_the_context_survives():
    """a vertex of valence above LAP_MAXROW - 1 = 63: ValueError naming the limit; the next call works"""
    m = 70
    az = 2.0 * np.pi * np.arange(m) / m
    V = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(az), np.sin(az), np.zeros(m)], axis=1)])
    F = np.array([[0, 1 + i, 1 + (i + 1) % m] for i in range(m)])
    with pytest.raises(ValueError, match="more than 63 neighbours"):
        geo.compute_operators(torch.from_numpy(V), torch.from_numpy(F), 0, route="device")
    verts, faces = dc.mesh("g")
    dc.check_against_golden(geo.compute_operators(verts, faces, 0, route="device"), "g", tag="after the error")

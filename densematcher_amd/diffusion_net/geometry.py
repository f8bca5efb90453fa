"""
diffusion_net.geometry of the reference: the operator precomputation every DiffusionNet forward needs, with the reference's names
and argument orders -- get_operators / get_all_operators / compute_operators -> (frames, massvec, L, evals, evecs, gradX, gradY).

Two routes compute the same definitions:
  device   MatchEngine.diffusion_operators: one batched call of dm_dnet_rows / dm_dnet_ell (normals, frames, cotangent Laplacian, masses,
           gradient rows, one thread per vertex) and dm_eigenbasis for the spectra; get_all_operators hands it all cache misses at once.
  host     the same definitions in vectorised NumPy with SciPy's eigsh(L + 1e-8 I, k, M, sigma=1e-8) (_host.py): what runs without a GPU.
route="auto" takes the device when a GPU is present.  Values are computed in float64 from the widened input and rounded once to
verts.dtype.

The reference takes L and the masses from the potpourri3d wheel (cotan_laplacian(V, F, denom_eps=1e-10), vertex_areas).  Here they are
the closed formulas those calls name: 1/2 dot / (|cross| + denom_eps) per corner, a third of the incident face areas.  PARITY WITH THE
WHEEL IS UNPINNED: it is not installed where the fixtures were made; tests/test_dnet_operators_cpu.py compares with it when it imports.
Frames and gradients are pinned to the reference's own functions (tests/golden/fx_dnet.npz).

Not built: point clouds (faces.numel() == 0 raises NotImplementedError), find_knn, farthest_point_sampling, normalize_positions and the
geodesic helpers of the reference's file.
"""
import os

import numpy as np
import scipy.sparse
import torch

from . import _host, utils
from .. import _routes
from .utils import toNP


# ---------------------------------------------------------------------------------------------------------------------
# the reference's named pieces, on the host route's definitions (_host.py): float64 from the widened input, rounded once
def _no_clouds(faces):
    if faces.numel() == 0:
        raise NotImplementedError("point clouds (no faces) are not built: diffusion_net operators need a triangle mesh here")


def _f64(t):
    return toNP(t).astype(np.float64)


def _like(array, verts):
    return torch.from_numpy(np.ascontiguousarray(array)).to(device=verts.device, dtype=verts.dtype)


def vertex_normals(verts, faces, n_neighbors_cloud=30):
    """vertex normals of a mesh, undefined ones repaired as the reference repairs them (_host.vertex_normals)"""
    _no_clouds(faces)
    return _like(_host.vertex_normals(_f64(verts), toNP(faces).astype(np.int64)), verts)


def build_tangent_frames(verts, faces, normals=None):
    """(V, 3, 3) frames with rows (bx, by, n); `normals` replaces the computed vertex normals"""
    if normals is None:
        _no_clouds(faces)
        n = _host.vertex_normals(_f64(verts), toNP(faces).astype(np.int64))
    else:
        n = _f64(normals)
    return _like(_host.tangent_frames(n), verts)


def edge_tangent_vectors(verts, frames, edges):
    """(E, 2) components of the edge vectors verts[edges[1]] - verts[edges[0]] in the frame of the tail vertex"""
    e = np.asarray(toNP(edges) if isinstance(edges, torch.Tensor) else edges).astype(np.int64)
    return _like(_host.edge_tangents(_f64(verts), _f64(frames), e[0], e[1]), verts)


def build_grad(verts, edges, edge_tangent_vectors):
    """(V, V) complex sparse gradient operator from the edges (2, E) and their tangent vectors: the reference's loops, vectorised"""
    edges_np = np.asarray(toNP(edges) if isinstance(edges, torch.Tensor) else edges).astype(np.int64)
    tang = toNP(edge_tangent_vectors) if isinstance(edge_tangent_vectors, torch.Tensor) else np.asarray(edge_tangent_vectors)
    return _host.grad_rows(verts.shape[0], edges_np[0], edges_np[1], tang)


# ---------------------------------------------------------------------------------------------------------------------
def _ell_to_coo(n, row_len, cols, vals, device, dtype):
    """rows in ELL (entries q < row_len[i] of row i, sorted by column) -> coalesced torch COO, rounded once to dtype"""
    keep = torch.arange(cols.shape[1], device=cols.device)[None, :] < row_len[:, None]
    rows = torch.arange(n, device=cols.device)[:, None].expand_as(cols)[keep]
    idx = torch.stack((rows, cols[keep].long()))
    return torch.sparse_coo_tensor(idx.to(device), vals[keep].to(device=device, dtype=dtype), (n, n)).coalesce()


def _check_frames(frames):
    if torch.any(torch.isnan(frames)):
        raise ValueError("NaN coordinate frame! Must be very degenerate")


def _from_device(op, device, dtype):
    n = op["frames"].shape[0]
    _check_frames(op["frames"])
    to = lambda t: t.to(device=device, dtype=dtype)
    sp3 = [_ell_to_coo(n, op["row_len"], op["cols"], op[key], device, dtype) for key in ("l", "gx", "gy")]
    return to(op["frames"]), to(op["mass"]), sp3[0], to(op["evals"]), to(op["evecs"]), sp3[1], sp3[2]


def _from_host(verts, faces, k_eig, normals):
    device, dtype = verts.device, verts.dtype
    nrm = None if normals is None else toNP(normals).astype(np.float64)
    frames, mass, L, evals, evecs, gX, gY = _host.operators(toNP(verts).astype(np.float64), toNP(faces).astype(np.int64), k_eig, nrm)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    sp_ = lambda A: utils.sparse_np_to_torch(A, torch.float64).to(device=device, dtype=dtype)
    return to(frames), to(mass), sp_(L), to(evals), to(evecs), sp_(gX), sp_(gY)


def _compute_many(verts_list, faces_list, k_eig, normals, route):
    for f in faces_list:
        _no_clouds(f)
    picked = _routes.pick_host(route)                  # "auto": the device when a GPU is present
    nrm = [None] * len(verts_list) if normals is None else list(normals)
    if picked != "device":
        return [_from_host(v, f, k_eig, g) for v, f, g in zip(verts_list, faces_list, nrm)]
    ops = _routes.engine_or_none().diffusion_operators(verts_list, faces_list, k_eig, normals=None if normals is None else nrm)
    return [_from_device(op, v.device, v.dtype) for op, v in zip(ops, verts_list)]


def compute_operators(verts, faces, k_eig, normals=None, route="auto"):
    """Spectral operators of a mesh, torch in / torch out on verts.device in verts.dtype:
      frames (V,3,3), massvec (V), L (VxV sparse), evals (k), evecs (V,k), gradX, gradY (VxV sparse).
    See get_operators() for the same behind the reference's cache."""
    return _compute_many([verts], [faces], k_eig, None if normals is None else [normals], route)[0]


# ---------------------------------------------------------------------------------------------------------------------
# the reference's .npz cache (geometry.py:425-570): <sha1 of verts and faces>_<bucket>.npz, float32 arrays, CSC triplets
_SPARSE = ("L", "gradX", "gradY")


def _cache_path(op_cache_dir, digest, bucket):
    return os.path.join(op_cache_dir, f"{digest}_{bucket}.npz")


def _cache_lookup(verts, faces, k_eig, op_cache_dir, overwrite_cache):
    """(operators or None, the path a new entry goes to).  Files are named <sha1 of the vertex and face bytes>_<bucket>.npz; buckets
    0, 1, ... are tried until one holds exactly these vertices and faces (a hit), or is missing or unreadable (the slot for a new
    entry).  A hit that is to be overwritten, holds fewer than k_eig eigenpairs or lacks the matrices is deleted and its slot reused."""
    V, F = toNP(verts), toNP(faces)
    utils.ensure_dir_exists(op_cache_dir)
    digest = utils.hash_arrays((V, F))
    bucket = 0
    while True:
        path = _cache_path(op_cache_dir, digest, bucket)
        try:
            with np.load(path, allow_pickle=True) as z:
                if not (np.array_equal(V, z["verts"]) and np.array_equal(F, z["faces"])):
                    bucket += 1                      # another mesh with the same digest
                    continue
                stale = overwrite_cache or int(z["k_eig"]) < k_eig or "L_data" not in z.files
                if not stale:
                    dense = {key: z[key] for key in ("frames", "mass", "evals", "evecs")}
                    mats = {m: scipy.sparse.csc_matrix((z[m + "_data"], z[m + "_indices"], z[m + "_indptr"]), shape=tuple(z[m + "_shape"])) for m in _SPARSE}
        except FileNotFoundError:
            return None, path
        except Exception as err:                     # an unreadable file: compute, and write over it
            print(f"operator cache: could not read {path}: {err}")
            return None, path
        if stale:
            os.remove(path)
            return None, path
        t = lambda a: _like(a, verts)
        m = {k: utils.sparse_np_to_torch(A).to(device=verts.device, dtype=verts.dtype) for k, A in mats.items()}
        return (t(dense["frames"]), t(dense["mass"]), m["L"], t(dense["evals"][:k_eig]), t(dense["evecs"][:, :k_eig]), m["gradX"], m["gradY"]), path


def _cache_store(path, verts, faces, k_eig, ops):
    """one entry in the reference's layout: float32 arrays, the three matrices as CSC triplets + shape, faces and k_eig as they are"""
    frames, mass, L, evals, evecs, gradX, gradY = ops
    f32 = lambda t: toNP(t).astype(np.float32)
    entry = {"verts": f32(verts), "faces": toNP(faces), "k_eig": k_eig, "frames": f32(frames), "mass": f32(mass), "evals": f32(evals), "evecs": f32(evecs)}
    for name, A in zip(_SPARSE, (L, gradX, gradY)):
        A = utils.sparse_torch_to_np(A).astype(np.float32)
        entry.update({name + "_data": A.data, name + "_indices": A.indices, name + "_indptr": A.indptr, name + "_shape": A.shape})
    np.savez(path, **entry)


def _check_verts(verts):
    if np.isnan(toNP(verts)).any():
        raise RuntimeError("tried to construct operators from NaN verts")


def get_operators(verts, faces, k_eig=128, op_cache_dir=None, normals=None, overwrite_cache=False):
    """compute_operators() behind the reference's cache: arrays are computed in double precision, stored on disk as single precision,
    and returned as tensors with the dtype / device of `verts`.  A directory written by the reference is readable here and back."""
    _check_verts(verts)
    found, search_path = (None, None) if op_cache_dir is None else _cache_lookup(verts, faces, k_eig, op_cache_dir, overwrite_cache)
    if found is not None:
        return found
    ops = compute_operators(verts, faces, k_eig, normals=normals)
    if op_cache_dir is not None:
        _cache_store(search_path, verts, faces, k_eig, ops)
    return ops


def get_all_operators(verts_list, faces_list, k_eig, op_cache_dir=None, normals=None, route="auto"):
    """get_operators for every mesh, lists out as in the reference; the cache misses share ONE batched device call (the reference
    loops over the meshes).  Inside it the eigensolver takes the meshes in up to two groups: those too small for the filtered iteration
    (2 (k_eig + guard) > vertices, e.g. fewer than 320 vertices at k_eig = 128) go down the dense route together, the others share the
    filtered iteration, so every mesh is solved by the route it takes alone."""
    N = len(verts_list)
    out, paths = [None] * N, [None] * N
    for i in range(N):
        _check_verts(verts_list[i])
        if op_cache_dir is not None:
            out[i], paths[i] = _cache_lookup(verts_list[i], faces_list[i], k_eig, op_cache_dir, False)
    miss = [i for i in range(N) if out[i] is None]
    if miss:
        ops = _compute_many([verts_list[i] for i in miss], [faces_list[i] for i in miss], k_eig,
                            None if normals is None else [normals[i] for i in miss], route)
        for i, op in zip(miss, ops):
            out[i] = op
            if op_cache_dir is not None:
                _cache_store(paths[i], verts_list[i], faces_list[i], k_eig, op)
    return tuple([o[q] for o in out] for q in range(7))


# ---------------------------------------------------------------------------------------------------------------------
# plain torch expressions (plumbing for the network's code, no kernels)
def to_basis(values, basis, massvec):
    """spectral coefficients basis^T diag(massvec) values: (B,V,D), (B,V,K), (B,V) -> (B,K,D)"""
    return basis.transpose(-2, -1) @ (massvec.unsqueeze(-1) * values)


def from_basis(values, basis):
    """basis @ values: (K,D) coefficients -> (V,D) vertex values; a real operand is promoted when the other is complex"""
    if values.is_complex() != basis.is_complex():
        ctype = values.dtype if values.is_complex() else basis.dtype
        values, basis = values.to(ctype), basis.to(ctype)
    return basis @ values


def compute_hks(evals, evecs, scales):
    """heat kernel signatures sum_k exp(-lambda_k t_s) phi_k(v)^2: evals (K), evecs (V,K), scales (S) -> (V,S), or all three with a
    leading batch dimension -> (B,V,S)"""
    weights = torch.exp(-scales.unsqueeze(-1) * evals.unsqueeze(-2))           # (..., S, K)
    return torch.einsum("...vk,...sk->...vs", evecs * evecs, weights)


def compute_hks_autoscale(evals, evecs, count):
    """compute_hks at `count` log-spaced times between 1e-2 and 1"""
    return compute_hks(evals, evecs, torch.logspace(-2, 0.0, steps=count, device=evals.device, dtype=evals.dtype))

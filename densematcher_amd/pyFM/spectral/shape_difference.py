"""
Shape difference operators with the reference's names (densematcher/pyFM/spectral/shape_difference.py:6-98): area_SD, conformal_SD,
compute_SD -- and compute_SD_many for collections (every shape against a base shape, several candidate maps per pair).

Two routes, chosen by what the caller passes:
* NumPy in: host NumPy / SciPy, the reference's products in the reference's order -- its bits, the noise row included: row 0 of
  the conformal operator is rounding noise divided by lambda_0 whenever np.linalg.pinv's cut-off keeps lambda_0.
* a GPU tensor in (a map, a vertex map), a leading batch dimension, or device=True: dm_shape_diff_f64 / dm_pullback_forms_f64
  (MatchEngine.shape_difference / pullback_forms), one call per kernel for all pairs, tensors out.  The sums run in another (fixed)
  order than the host's: entries agree to the error bound of two summation orders, (n + 2) 2^-52 |X|^T |A| |X| with n the length
  of the contraction; a pair's bits do not depend on what shares the call.

A single compute_SD call on NumPy inputs stays on the host: one pair is a few small products, less than a launch chain and the
transfers (tools/shape_diff_time.py).
"""
import numpy as np

__all__ = ["area_SD", "conformal_SD", "compute_SD", "compute_SD_many"]


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _on_device(*arrays):
    """is one of the arrays a torch tensor on a GPU?  (torch is not imported for NumPy callers)"""
    return any(_is_torch(a) and getattr(a, "is_cuda", False) for a in arrays)


def _engine():
    from ...engine import default_engine
    return default_engine()


def _batched(FM):
    """(the map with a batch axis, did it have one) for the device route"""
    nd = FM.dim() if _is_torch(FM) else np.ndim(FM)
    if nd not in (2, 3):
        raise ValueError("a functional map is (k2,k1), a batch of maps (B,k2,k1)")
    return (FM if nd == 3 else FM[None]), nd == 3


def _evals_rows(ev, B, k):
    """eigenvalues (>= k,) shared by the maps of a batch, or (B, >= k), cut to k columns"""
    ev = ev if _is_torch(ev) else np.asarray(ev, dtype=np.float64)
    if ev.ndim == 1:
        ev = ev[None].expand(B, -1) if _is_torch(ev) else np.broadcast_to(ev[None], (B, ev.shape[0]))
    return ev[:, :k]


def area_SD(FM):
    """FM^T FM, the area based shape difference operator of a (k2,k1) functional map (shape_difference.py:6-21).
    NumPy (k2,k1): NumPy out.  A GPU tensor or a batch (B,k2,k1): dm_shape_diff_f64, a tensor of the same rank out."""
    if not _on_device(FM) and np.ndim(FM) == 2:
        return FM.T @ FM
    maps, had = _batched(FM)
    out = _engine().shape_difference(maps)[0]
    return out if had else out[0]


def conformal_SD(FM, evals1, evals2):
    """pinv(diag(evals1[:k1])) FM^T (evals2[:k2, None] * FM), the conformal shape difference operator (shape_difference.py:24-45).
    NumPy (k2,k1): NumPy out, the products left to right as the reference takes them.  A GPU tensor or a batch (B,k2,k1), with
    eigenvalues (k,) shared or (B,k): dm_shape_diff_f64, a tensor of the same rank out."""
    if not _on_device(FM, evals1, evals2) and np.ndim(FM) == 2:
        k2, k1 = FM.shape
        inv1 = np.linalg.pinv(np.diag(evals1[:k1]))
        return inv1 @ FM.T @ (evals2[:k2, None] * FM)
    maps, had = _batched(FM)
    B, k2, k1 = maps.shape
    out = _engine().shape_difference(maps, _evals_rows(evals1, B, k1), _evals_rows(evals2, B, k2))[1]
    return out if had else out[0]


def _host_FM(p2p, mesh1, mesh2, k1, k2):
    """convert.mesh_p2p_to_FM on the host (convert.py:39-48, :90): Phi2[:, :k2]^T (A2 Phi1[p2p, :k1]), the slices clipping
    silently to the eigenpairs the meshes hold"""
    pulled = mesh1.eigenvectors[:, :k1][p2p, :]
    A2 = mesh2.A
    if A2.shape[0] != mesh2.eigenvectors.shape[0]:
        raise ValueError("Can't compute exact pseudo inverse with subsampled eigenvectors")
    if A2.ndim == 1:
        return mesh2.eigenvectors[:, :k2].T @ (A2[:, None] * pulled)
    return mesh2.eigenvectors[:, :k2].T @ (A2 @ pulled)


def _host_SD(mesh1, mesh2, k1, k2, p2p, SD_type):
    if SD_type == 'spectral':
        FM = _host_FM(p2p, mesh1, mesh2, k1, k2)
        return area_SD(FM), conformal_SD(FM, mesh1.eigenvalues, mesh2.eigenvalues)
    X = mesh1.eigenvectors[p2p, :k1]
    SD_a = X.T @ mesh2.A @ X
    SD_c = np.linalg.pinv(np.diag(mesh1.eigenvalues[:k1])) @ X.T @ mesh2.W @ X
    return SD_a, SD_c


def _defaults(mesh1, mesh2, k1, k2, p2p):
    if k1 is None:
        k1 = len(mesh1.eigenvalues)
    if k2 is None:
        k2 = 3 * k1
    if p2p is None:
        p2p = np.arange(mesh2.n_vertices)
    return k1, k2, p2p


def compute_SD(mesh1, mesh2, k1=None, k2=None, p2p=None, SD_type='spectral', device=None):
    """(SD_a, SD_c), both (k1,k1), from a vertex to vertex map p2p (n2,) of mesh2 into mesh1 (shape_difference.py:48-98).
    'spectral': through the (k2,k1) functional map of p2p in the two eigenbases; 'semican': the canonical basis on mesh2, i.e. its
    mass and stiffness matrices pulled back through p2p.  Defaults as in the reference: k1 all of mesh1's eigenpairs, k2 = 3 k1
    (clipped silently to what mesh2 holds), p2p the identity.
    device (not in the reference): None = the device route when p2p is a GPU tensor, else the host's NumPy (the reference's bits);
    True / False force a route.  The device route returns tensors."""
    assert SD_type in ['spectral', 'semican'], f"Problem with type of SD type : {SD_type}"
    if device is None:
        device = _on_device(p2p)
    if not device:
        k1, k2, p2p = _defaults(mesh1, mesh2, k1, k2, p2p)
        if _is_torch(p2p):
            p2p = p2p.cpu().numpy()
        return _host_SD(mesh1, mesh2, k1, k2, p2p, SD_type)
    SD_a, SD_c = compute_SD_many([mesh1], [mesh2], k1=k1, k2=k2, p2ps=[p2p], SD_type=SD_type, device=True)
    return SD_a[0], SD_c[0]


def _stiffness_operand(mesh):
    """W of a mesh as MatchEngine.pullback_forms takes it: the device rows of the last assembly when they are still there (no host
    round trip), else the SciPy matrix"""
    if getattr(mesh, "_W", True) is None and getattr(mesh, "_W_dev", None) is not None:
        return mesh._W_dev
    return mesh.W


def _pad_rows(arrays, n, dtype):
    out = np.zeros((len(arrays), n) + arrays[0].shape[1:], dtype=dtype)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0]] = a
    return out


def compute_SD_many(meshes1, meshes2, k1=None, k2=None, p2ps=None, SD_type='spectral', device=None):
    """compute_SD for P pairs (meshes1[p], meshes2[p], p2ps[p]); a single mesh in place of a list is shared by all pairs, and a
    mesh may appear in any number of pairs.  k1 / k2: one value, or one per pair.
    device: None = the device route when a GPU is present, True / False force a route.
    Host route: the loop of compute_SD, two lists of NumPy arrays.
    Device route: ONE call per kernel for all the pairs of a group -- pairs are grouped by k1 ('semican': meshes of different
    vertex counts ride along padded; 'spectral': also by k2 and by the target's vertex count, which fixes the summation order of
    dm_p2p_to_fm_f64) -- so that every pair has the bits it has alone.  Meshes that still hold the device stiffness rows of their
    assembly hand them over as they are.  Returns two stacked (P,k1,k1) tensors, or two lists of tensors when k1 varies."""
    assert SD_type in ['spectral', 'semican'], f"Problem with type of SD type : {SD_type}"
    lists = [x for x in (meshes1, meshes2, p2ps) if isinstance(x, (list, tuple))]
    if not lists:
        raise ValueError("compute_SD_many: pass a list of meshes or of maps")
    P = len(lists[0])
    spread = lambda x: list(x) if isinstance(x, (list, tuple)) else [x] * P
    meshes1, meshes2, p2ps = spread(meshes1), spread(meshes2), spread(p2ps)
    k1s = list(k1) if isinstance(k1, (list, tuple, np.ndarray)) else [k1] * P
    k2s = list(k2) if isinstance(k2, (list, tuple, np.ndarray)) else [k2] * P
    if not (len(meshes1) == len(meshes2) == len(p2ps) == len(k1s) == len(k2s) == P):
        raise ValueError("compute_SD_many: lists of different lengths")
    if device is None:
        import torch
        device = _on_device(*p2ps) or torch.cuda.is_available()
    if not device:
        out = [compute_SD(meshes1[p], meshes2[p], k1=k1s[p], k2=k2s[p], p2p=p2ps[p], SD_type=SD_type, device=False) for p in range(P)]
        return [o[0] for o in out], [o[1] for o in out]

    import torch
    eng = _engine()
    groups = {}
    for p in range(P):
        m1, m2 = meshes1[p], meshes2[p]
        ka, kb, _ = _defaults(m1, m2, k1s[p], k2s[p], 0)
        ka, kb = min(ka, m1.eigenvectors.shape[1]), min(kb, m2.eigenvectors.shape[1])       # (the reference's slices clip silently)
        if len(m1.eigenvalues) < ka or len(m2.eigenvalues) < kb:
            raise ValueError(f"compute_SD_many: pair {p}: fewer eigenvalues than eigenvectors")
        key = (ka, kb, m2.eigenvectors.shape[0]) if SD_type == 'spectral' else (ka,)
        groups.setdefault(key, []).append((p, ka, kb))
    res_a, res_c = [None] * P, [None] * P
    for members in groups.values():
        idx = [m[0] for m in members]
        ka, kb = members[0][1], members[0][2]
        G = len(idx)
        g1, g2 = [meshes1[p] for p in idx], [meshes2[p] for p in idx]
        nv1 = np.asarray([m.eigenvectors.shape[0] for m in g1], np.int32)
        nv2 = np.asarray([m.eigenvectors.shape[0] for m in g2], np.int32)
        N1, N2 = int(nv1.max()), int(nv2.max())
        Phi1 = _pad_rows([np.asarray(m.eigenvectors, np.float64)[:, :ka] for m in g1], N1, np.float64)
        lam1 = np.stack([np.asarray(m.eigenvalues, np.float64)[:ka] for m in g1])
        mass2 = _pad_rows([np.asarray(m.A.diagonal(), np.float64) for m in g2], N2, np.float64)
        maps = torch.zeros((G, N2), dtype=torch.int64, device=eng.device)
        for q, p in enumerate(idx):
            if p2ps[p] is None:
                maps[q, :nv2[q]] = torch.arange(int(nv2[q]), device=eng.device)
            else:
                m = p2ps[p] if _is_torch(p2ps[p]) else torch.as_tensor(np.asarray(p2ps[p]))
                if m.dtype.is_floating_point or m.dtype == torch.bool:
                    raise IndexError("arrays used as indices must be of integer type")
                if m.dim() != 1 or m.shape[0] != nv2[q]:
                    raise ValueError(f"compute_SD_many: pair {p}: a map of {tuple(m.shape)} entries for {int(nv2[q])} target vertices")
                maps[q, :nv2[q]] = m.to(eng.device)
        r1 = None if int(nv1.min()) == N1 else nv1
        r2 = None if int(nv2.min()) == N2 else nv2
        if SD_type == 'spectral':
            p21 = eng._vertex_maps(maps, G, N2, N1, r1, r2, "compute_SD")
            Phi2 = np.stack([np.asarray(m.eigenvectors, np.float64)[:, :kb] for m in g2])
            lam2 = np.stack([np.asarray(m.eigenvalues, np.float64)[:kb] for m in g2])
            FM = eng.p2p_to_fm(p21, Phi1, Phi2, mass2, ka, kb)
            SD_a, SD_c = eng.shape_difference(FM, lam1, lam2)
        else:
            SD_a, SD_c = eng.pullback_forms(maps, Phi1, [_stiffness_operand(m) for m in g2], mass2, ka, lam1=lam1, n_verts1=r1, n_verts2=r2)
        for q, p in enumerate(idx):
            res_a[p], res_c[p] = SD_a[q], SD_c[q]
    if len({tuple(t.shape) for t in res_a}) == 1:
        return torch.stack(res_a), torch.stack(res_c)
    return res_a, res_c

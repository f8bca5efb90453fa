"""
Host-side operand handling of MatchEngine, once: the stride rule of the C ABI, vertex counts and index tables of padded batches,
CSR -> ELL rows, info words -> errors.  Plain functions of tensors and NumPy arrays: no engine, no stream, no library call.
"""
import ctypes as C

import numpy as np
import torch


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def host_ptr(a):
    """a NumPy array as a pointer argument of the library (None or no elements: NULL)"""
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


def fits_strides(shape, strides, min_ld=None):
    """fits_abi on the sizes and strides of a 2-D (R, W) or 3-D (B, N, W) operand"""
    if len(shape) == 2:
        B, (N, W), s0, (s1, s2) = 1, shape, 0, strides
    else:
        (B, N, W), (s0, s1, s2) = shape, strides
    ld = s1 if N > 1 else (s0 if B > 1 else W)
    if (W == 1 or s2 == 1) and (W if min_ld is None else max(W, min_ld)) <= ld < 2 ** 31 and (B == 1 or s0 == N * ld):
        return int(ld)
    return None


def fits_abi(t, min_ld=None):
    """The row stride ld with which the library reads the matrix t, (R, W) or (B, N, W), where it lies (a parameter, a column slice, a
    padded view): the elements of a row adjacent, W <= ld < 2^31 (the ABI's int), meshes N ld apart.  None: t has to be copied."""
    return fits_strides(t.shape, t.stride(), min_ld)


def counts(n_verts, B, N, lo, who, name="n_verts", hi="N"):
    """the vertex counts of a batch padded to N as a (B,) int32 array (None: N for every mesh; one number: every mesh's), each in
    [lo, N]; `hi` is how the message writes the upper bound"""
    nv = np.full(B, N, np.int64) if n_verts is None else np.broadcast_to(np.asarray(n_verts, np.int64).reshape(-1), (B,))
    if nv.min() < lo or nv.max() > N:
        raise ValueError(f"{who}: {name} must lie in [{lo}, {hi}]")
    return np.ascontiguousarray(nv, np.int32)


def problem_meshes(mesh, P, B, who):
    """the mesh of every problem of a call as a (P,) int64 array (None: mesh 0), each in [0, B)"""
    mesh = np.zeros(P, np.int64) if mesh is None else np.broadcast_to(np.asarray(mesh, np.int64), (P,))
    if P and (mesh.min() < 0 or mesh.max() >= B):
        raise ValueError(f"{who}: mesh indices must lie in [0, {B})")
    return mesh


def csr_to_ell(indptr, indices, data, n_rows, width=None, pad_col=-1):
    """The rows of a CSR matrix (the columns of a CSC one) as ELL rows (cols (n_rows, w) int32, vals (n_rows, w) float64): a row's entries in
    stored order, explicit zeros kept, then col = pad_col (a number, or (n_rows, 1) values), val = 0.  width None: the longest row, at least 1."""
    rl = np.diff(indptr)
    w = max(1, int(rl.max()) if n_rows else 0) if width is None else width
    cols = np.full((n_rows, w), pad_col, np.int32)
    vals = np.zeros((n_rows, w), np.float64)
    r = np.repeat(np.arange(n_rows), rl)
    pos = np.arange(len(r)) - np.repeat(indptr[:-1], rl)
    cols[r, pos] = indices
    vals[r, pos] = data
    return cols, vals


def stack_ell(rows, N, device):
    """per-mesh ELL rows [(cols (n_b, w_b), w (n_b, w_b))] as one batch (cols (B, N, nnz) int32, w (B, N, nnz) float64) on
    `device`, nnz the widest; the padding is col = -1, w = 0"""
    nnz = max(int(c.shape[1]) for c, _ in rows)
    cols = torch.full((len(rows), N, nnz), -1, dtype=torch.int32, device=device)
    wv = torch.zeros((len(rows), N, nnz), dtype=torch.float64, device=device)
    for b, (c, w) in enumerate(rows):
        cols[b, :c.shape[0], :c.shape[1]] = c.to(device, torch.int32)
        wv[b, :w.shape[0], :w.shape[1]] = w.to(device, torch.float64)
    return cols, wv


def pad_stack(arrays, shape, fill, dtype):
    """per-mesh arrays (n_b, ...) as one (B,) + shape array: the rows of mesh b, then `fill`"""
    out = np.full((len(arrays),) + shape, fill, dtype)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out


def source_table(sources, n_verts, N, who):
    """the (B, ns) int32 source table of a geodesic call on meshes of n_verts vertices padded to N: None = all pairs (every vertex of
    a mesh, then -1), a 1-D list shared by every mesh, or one list per mesh (the same length, -1 = none)"""
    Bn = len(n_verts)
    if sources is None:
        src = np.full((Bn, N), -1, np.int32)
        for b, n in enumerate(n_verts):
            src[b, :n] = np.arange(n)
        return src
    src = np.asarray(sources)
    src = np.broadcast_to(src, (Bn, src.shape[-1])) if src.ndim == 1 else src
    if src.ndim != 2 or src.shape[0] != Bn or src.shape[1] == 0:
        raise ValueError(f"{who}: sources must be (ns,) or ({Bn}, ns)")
    for b, n in enumerate(n_verts):
        if src[b].min() < -1 or src[b].max() >= n:
            raise ValueError(f"{who}: mesh {b}: source indices must lie in [0, {n})")
    return np.ascontiguousarray(src, np.int32)


def start_vertices(start, n_verts, who):
    """the start vertices of a sampling call as a (B,) int32 array: one index or one per mesh, each in its mesh"""
    st = np.broadcast_to(np.asarray(start, np.int64), (len(n_verts),))
    for b, n in enumerate(n_verts):
        if st[b] < 0 or st[b] >= n:
            raise ValueError(f"{who}: mesh {b}: the start vertex must lie in [0, {n})")
    return np.ascontiguousarray(st, np.int32)


def raise_info(info_host, table, who, what="mesh"):
    """ValueError for the first nonzero word of a per-mesh info array: the texts of its bits in `table` ((bit, text), ...)"""
    for b in np.flatnonzero(info_host):
        raise ValueError(f"{who}: {what} {int(b)}: " + "; ".join(msg for bit, msg in table if info_host[b] & bit))


def index_list(lst, n, who):
    a = np.asarray(lst)
    if a.ndim != 1:
        raise ValueError(f"{who}: an index list must be one-dimensional")
    if a.size and not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.bool_)):
        raise ValueError(f"{who}: an index list must hold integers")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= n):
        raise ValueError(f"{who}: vertex indices must lie in [0, {n})")
    return a.astype(np.int32)


def numpy_index(lst, n, who):
    """an index list with NumPy's rules against an axis of length n: integers in [-n, n), negatives counted from the end
    (IndexError otherwise, NumPy's text); returned as non-negative int32"""
    a = np.asarray(lst.cpu() if isinstance(lst, torch.Tensor) else lst)
    if a.ndim != 1:
        raise ValueError(f"{who}: an index list must be one-dimensional")
    if a.size == 0:
        return np.zeros(0, np.int32)
    if not np.issubdtype(a.dtype, np.integer):
        raise IndexError(f"{who}: arrays used as indices must be of integer type")
    lo, hi = int(a.min()), int(a.max())
    if lo < -n or hi >= n:
        raise IndexError(f"{who}: index {lo if lo < -n else hi} is out of bounds for axis 0 with size {n}")
    return np.where(a < 0, a + n, a).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# multi-view feature lifting: the one place where its meshes, cameras and given pix2face images are checked (MatchEngine on the
# device route, projection.py on the host route)
def to_numpy(a, dtype=None):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


def image_frame(H, W, focal_length, who):
    """(H, W) as ints of a square, non-empty image; focal_length (None: the caller has none to check) positive and finite"""
    if int(H) != int(W):
        raise ValueError(f"{who}: square images only (H = {H}, W = {W})")
    if int(H) <= 0:
        raise ValueError(f"{who}: H and W must be positive")
    if focal_length is not None and not (float(focal_length) > 0.0 and np.isfinite(float(focal_length))):
        raise ValueError(f"{who}: the focal length must be positive and finite")
    return int(H), int(W)


def lift_mesh(verts, faces, who):
    """(verts (n, 3) float64, faces (m, 3) int64) as NumPy arrays, every face index inside the mesh"""
    V, F = to_numpy(verts, np.float64), to_numpy(faces)
    if V.ndim != 2 or V.shape[1] != 3 or V.shape[0] == 0:
        raise ValueError(f"{who}: vertices must be (n, 3)")
    if F.ndim != 2 or F.shape[1] != 3 or F.shape[0] == 0 or not np.issubdtype(F.dtype, np.integer):
        raise ValueError(f"{who}: faces must be (m, 3) integers")
    if F.min() < 0 or F.max() >= V.shape[0]:
        raise ValueError(f"{who}: faces must be (m, 3) indices into the {V.shape[0]} vertices")
    return V, F.astype(np.int64)


def lift_cameras(cameras, who, max_views=None):
    """(R (views, 3, 3), T (views, 3)) float64 NumPy arrays"""
    if cameras is None:
        raise ValueError(f"{who}: cameras=(R, T) is required: the feature maps were rendered with some cameras, and the caller has them")
    if len(cameras) != 2:
        raise ValueError(f"{who}: cameras must be a pair (R (views, 3, 3), T (views, 3))")
    R, T = to_numpy(cameras[0], np.float64), to_numpy(cameras[1], np.float64)
    if R.ndim != 3 or R.shape[1:] != (3, 3) or T.shape != (R.shape[0], 3) or R.shape[0] == 0:
        raise ValueError(f"{who}: cameras must be a pair (R (views, 3, 3), T (views, 3))")
    if max_views is not None and R.shape[0] > max_views:
        raise ValueError(f"{who}: at most {max_views} views per mesh")
    return R, T


def lift_pix2face(pix2face, views, n_faces, who):
    """a given pix2face as an integer (views, H, H) tensor where it lies ((views, H, H, 1), pytorch3d's shape, is accepted), every
    entry in [-1, n_faces): one read of (min, max), a single host round trip for a device tensor"""
    g = pix2face if isinstance(pix2face, torch.Tensor) else torch.as_tensor(np.asarray(pix2face))
    if g.dim() == 4 and g.shape[-1] == 1:
        g = g[..., 0]
    if g.dtype.is_floating_point or g.dtype == torch.bool or g.dim() != 3 or g.shape[0] != views or g.shape[1] != g.shape[2] or g.numel() == 0:
        raise ValueError(f"{who}: pix2face must be ({views}, H, H) integers")
    lo, hi = torch.stack(torch.aminmax(g)).tolist()
    if lo < -1 or hi >= n_faces:
        raise ValueError(f"{who}: pix2face holds {lo if lo < -1 else hi}: face indices must lie in [-1, {n_faces})")
    return g


# ---------------------------------------------------------------------------------------------------------------------
# textured-mesh rendering: the one place where its textures, colours and lights are checked (MatchEngine.render_phong on the device
# route, render.py on the host route)
def _tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


def render_texture(tex, n_verts, n_faces, who):
    """A mesh's texture: None (white), ("vertex", colours (n, 3)) or ("uv", map (Ht, Wt, 3), verts_uvs (n_uv, 2), faces_uvs (m, 3)).
    Returns (0,), (1, colours fp32 tensor) or (2, map fp32 tensor, verts_uvs fp32 tensor, faces_uvs int32 array), the tensors where
    they lie; every UV index inside verts_uvs."""
    if tex is None:
        return (0,)
    if not isinstance(tex, (tuple, list)) or not tex or tex[0] not in ("vertex", "uv"):
        raise ValueError(f"{who}: a texture is None, ('vertex', colours) or ('uv', map, verts_uvs, faces_uvs)")
    if tex[0] == "vertex":
        if len(tex) != 2:
            raise ValueError(f"{who}: a vertex texture is ('vertex', colours)")
        col = _tensor(tex[1])
        if col.dim() != 2 or tuple(col.shape) != (n_verts, 3):
            raise ValueError(f"{who}: vertex colours must be ({n_verts}, 3): one RGB row per vertex")
        return 1, col.to(torch.float32).contiguous()
    if len(tex) != 4:
        raise ValueError(f"{who}: a UV texture is ('uv', map, verts_uvs, faces_uvs)")
    tmap, uvs, fuv = _tensor(tex[1]), _tensor(tex[2]), to_numpy(tex[3])
    if tmap.dim() != 3 or tmap.shape[2] != 3 or tmap.shape[0] == 0 or tmap.shape[1] == 0 or max(tmap.shape[:2]) > 32768:
        raise ValueError(f"{who}: a texture map must be (Ht, Wt, 3), at most 32768 x 32768")
    if uvs.dim() != 2 or uvs.shape[1] != 2 or uvs.shape[0] == 0:
        raise ValueError(f"{who}: verts_uvs must be (n_uv, 2)")
    if fuv.shape != (n_faces, 3) or not np.issubdtype(fuv.dtype, np.integer):
        raise ValueError(f"{who}: faces_uvs must be ({n_faces}, 3) integers: one row per face")
    if fuv.min() < 0 or fuv.max() >= uvs.shape[0]:
        raise ValueError(f"{who}: faces_uvs must be ({n_faces}, 3) indices into the {uvs.shape[0]} rows of verts_uvs")
    return 2, tmap.to(torch.float32).contiguous(), uvs.to(torch.float32).contiguous(), np.ascontiguousarray(fuv, np.int32)


def render_corners(F, n):
    """the faces incident to every vertex as a CSR (ptr (n + 1,), face (3 m,)) int32: one entry per corner, ascending face index"""
    flat = np.asarray(F, np.int64).ravel()
    face = (np.argsort(flat, kind="stable") // 3).astype(np.int32)
    ptr = np.concatenate(([0], np.cumsum(np.bincount(flat, minlength=n)))).astype(np.int32)
    return ptr, face


def render_colour(c, who, name):
    a = np.asarray(to_numpy(c), np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{who}: {name} must be three finite numbers")
    return a.astype(np.float32)


def render_points(p, views, who, name):
    """optional per-view points (views, 3) (or one (3,) / (1, 3) point for every view) as float64"""
    if p is None:
        return None
    a = to_numpy(p, np.float64)
    a = np.broadcast_to(a.reshape(-1, 3), (views, 3)) if a.size == 3 else a
    if a.shape != (views, 3) or not np.isfinite(a).all():
        raise ValueError(f"{who}: {name} must be ({views}, 3) finite numbers")
    return np.ascontiguousarray(a)


def render_normals(nrm, n_verts, who):
    if nrm is None:
        return None
    a = to_numpy(nrm, np.float64)
    if a.shape != (n_verts, 3) or not np.isfinite(a).all():
        raise ValueError(f"{who}: vertex normals must be ({n_verts}, 3) finite numbers")
    return a

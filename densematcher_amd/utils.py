"""
The semantic group distances of the reference's driver (densematcher/utils.py:115-143), under its names:

    from densematcher_amd.utils import get_distance_between_groups, get_groups_dmtx

These two functions (and a batched form of the second), the camera generator get_uniform_SO3_RT with its look_at_view_transform
(end of this file) and recenter are what is mirrored of that module; nothing here imports its rendering or plotting dependencies.  For every pair of vertex groups the reference solves a rectangular min-cost assignment on
D[np.ix_(g_i, g_j)] with SciPy and takes the mean matched distance.  On the device all pairs of all meshes are ONE call
(MatchEngine.groups_dmtx -> dm_lsa_gather): the same assignments, ties included; the means agree with the reference's to the
rounding of a sum of min(|g_i|, |g_j|) terms (NumPy adds them pairwise, the kernel in row order).

Routing (_routes.engine_for): `device=None` takes the device when the process has a GPU and
DEVICE_DEFAULT is set, else the reference's SciPy loop on the host; `device=True` / `device=False` force a route
(device=True without a GPU fails as MatchEngine() does: there is no silent fall-back).
"""
import os

import numpy as np

from . import _routes

# Whether device=None means the device in a process with a GPU.  Set from the measurement in DESIGN.md ("Semantic group
# distances"): the device route is the default only because its single-mesh time was below the host loop's at every
# group count measured.
DEVICE_DEFAULT = True


def _host_pair(D, group1, group2):
    from scipy.optimize import linear_sum_assignment
    block = D[np.asarray(group1)[:, None], np.asarray(group2)[None, :]]
    rows, cols = linear_sum_assignment(block)
    return block[rows, cols].mean()


def _empty_pair():
    if os.environ.get('VERBOSE', False):
        print("Warning: empty group when computing distance between groups")
    return 0


def get_distance_between_groups(geodesic_distmat, group1, group2, device=None):
    """Mean matched distance of the min-cost assignment between two vertex groups on the (V, V) matrix geodesic_distmat: rows
    group1, columns group2 (utils.py:115-127).  An empty group gives 0 (and the reference's warning when VERBOSE is set in
    the environment)."""
    if len(group1) == 0 or len(group2) == 0:
        return _empty_pair()
    eng = _routes.engine_for(device, DEVICE_DEFAULT)
    if eng is None:
        return _host_pair(np.asarray(geodesic_distmat), group1, group2)
    return eng.lsa_gather(geodesic_distmat, [group1], [group2])[0]


def _host_dmtx(D, groups):
    D = np.asarray(D)
    G = len(groups)
    out = np.zeros((G, G))
    for i in range(G):
        for j in range(i + 1, G):
            if len(groups[i]) == 0 or len(groups[j]) == 0:
                out[i, j] = _empty_pair()
            else:
                out[i, j] = _host_pair(D, groups[i], groups[j])
            out[j, i] = out[i, j]
    return out


def _warn_empty(groups):
    G = len(groups)
    for i in range(G):
        for j in range(i + 1, G):
            if len(groups[i]) == 0 or len(groups[j]) == 0:
                _empty_pair()


def get_groups_dmtx(geodesic_distmat, groups, device=None):
    """(G, G) distance matrix between vertex groups (utils.py:129-143): 0 on the diagonal; entry [i, j] for i < j is
    get_distance_between_groups(D, groups[i], groups[j]) -- rows g_i, columns g_j: D is not symmetric (the heat method's is
    not, Dijkstra's not in the last bit), so the orientation is part of the result -- and [j, i] is a copy of it.
    The reference marks entries that are not computed yet with -1 and therefore computes [j, i] afresh when a mean is
    exactly -1; that cannot happen for distances and is NOT mirrored: [j, i] is always the copy."""
    eng = _routes.engine_for(device, DEVICE_DEFAULT)
    if eng is None:
        return _host_dmtx(geodesic_distmat, groups)
    _warn_empty(groups)
    return eng.groups_dmtx(geodesic_distmat if _is_tensor(geodesic_distmat) else np.asarray(geodesic_distmat), list(groups))


def _is_tensor(x):
    import torch
    return isinstance(x, torch.Tensor)


def get_groups_dmtx_many(geodesic_distmats, groups_list, device=None):
    """get_groups_dmtx for several meshes: a list of (n_b, n_b) matrices (any sizes) or one padded (B, N, N) array / device
    tensor, and one list of groups per mesh.  ONE device call for the batch.  Returns a list of (G_b, G_b) arrays."""
    groups_list = [list(g) for g in groups_list]
    eng = _routes.engine_for(device, DEVICE_DEFAULT)
    stacked = _is_tensor(geodesic_distmats) or (isinstance(geodesic_distmats, np.ndarray) and geodesic_distmats.ndim == 3)
    if len(geodesic_distmats) != len(groups_list):
        raise ValueError(f"get_groups_dmtx_many: {len(groups_list)} lists of groups for {len(geodesic_distmats)} matrices")
    if eng is None:
        return [_host_dmtx(D.cpu().numpy() if _is_tensor(D) else D, g) for D, g in zip(geodesic_distmats, groups_list)]
    if len(groups_list) == 0:
        return []
    for g in groups_list:
        _warn_empty(g)
    if stacked:
        return eng.groups_dmtx(geodesic_distmats, groups_list)
    mats = [np.asarray(D, np.float64) for D in geodesic_distmats]
    sizes = [D.shape[0] for D in mats]
    N = max(sizes)
    pad = np.zeros((len(mats), N, N))
    for b, D in enumerate(mats):
        if D.ndim != 2 or D.shape[0] != D.shape[1]:
            raise ValueError(f"get_groups_dmtx_many: matrix {b} must be square")
        pad[b, :sizes[b], :sizes[b]] = D
    return eng.groups_dmtx(pad, groups_list, n_verts=sizes)


# ---------------------------------------------------------------------------------------------------------------------
# cameras (utils.py:73-113).  pytorch3d's look_at_view_transform is restated, NOT pinned against pytorch3d: row vectors,
# X_view = X_world R + T, the columns of R are the camera's x (left), y (up), z (forward) axes in world coordinates.
POLE_EPS = 1e-8


def look_at_view_transform(dist=1.0, elev=0.0, azim=0.0, at=((0.0, 0.0, 0.0),), up=((0.0, 1.0, 0.0),), device="cpu"):
    """(R (views, 3, 3), T (views, 3)) fp32 tensors of cameras at eye = at + dist (cos e sin a, sin e, cos e cos a) (degrees) that look
    at `at`: z = unit(at - eye), x = unit(up x z), y = unit(z x x), R = [x | y | z], T = -eye R; computed in float64.
    Where up is parallel to the view direction (|up x z| < 1e-8: the pole views of get_uniform_SO3_RT) pytorch3d's fallback depends on
    fp32 rounding; HERE the x axis is the limit of azimuth a as |e| -> 90 degrees, x = (-cos a, 0, sin a) (for the default up = +y).
    This is a stated deviation from pytorch3d."""
    import torch
    num = lambda v: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float64)
    e, a, d = np.deg2rad(num(elev)).reshape(-1), np.deg2rad(num(azim)).reshape(-1), num(dist).reshape(-1)
    views = max(len(e), len(a), len(d))
    e, a, d = (np.broadcast_to(t, (views,)) for t in (e, a, d))
    at, up = np.broadcast_to(num(at).reshape(-1, 3), (views, 3)), np.broadcast_to(num(up).reshape(-1, 3), (views, 3))
    eye = at + d[:, None] * np.stack((np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)), axis=1)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    z = unit(at - eye)
    x = np.cross(up, z)
    pole = np.linalg.norm(x, axis=1) < POLE_EPS
    x[pole] = np.stack((-np.cos(a), np.zeros(views), np.sin(a)), axis=1)[pole]
    x = unit(x)
    y = unit(np.cross(z, x))
    R = np.stack((x, y, z), axis=2)
    T = -np.einsum("vj,vjk->vk", eye, R)
    return torch.from_numpy(R.astype(np.float32)).to(device), torch.from_numpy(T.astype(np.float32)).to(device)


def get_uniform_SO3_RT(num_azimuth, num_elevation, distance, center, device="cpu", add_angle_azi=0, add_angle_ele=0):
    """The reference's camera placement (utils.py:85-113): num_azimuth * num_elevation views on a grid of azimuths
    linspace(0, 360, num_azimuth + 1)[:-1] and elevations linspace(-90, 90, num_elevation + 2)[1:-1] (elevation-major), then the two
    pole views (azimuth 0, elevation -90 and +90); add_angle_azi / add_angle_ele are added to every view.  All cameras look at
    `center` ((1, 3) or (3,)) from `distance`.  Returns (rotation (views, 3, 3), translation (views, 3), azimuth, elevation) fp32."""
    import torch
    num = lambda v: float(v.detach().cpu().reshape(-1)[0]) if isinstance(v, torch.Tensor) else float(np.asarray(v).reshape(-1)[0])
    azi = np.linspace(0.0, 360.0, int(num_azimuth) + 1)[:-1]
    ele = np.linspace(-90.0, 90.0, int(num_elevation) + 2)[1:-1]
    grid = np.stack(np.broadcast_arrays(azi[None, :], ele[:, None]), axis=-1).reshape(-1, 2)
    grid = np.concatenate((grid, np.array([[0.0, -90.0], [0.0, 90.0]])), axis=0)
    azimuth, elevation = grid[:, 0] + num(add_angle_azi), grid[:, 1] + num(add_angle_ele)
    rotation, translation = look_at_view_transform(dist=num(distance), elev=elevation, azim=azimuth, at=center, device=device)
    return rotation, translation, torch.from_numpy(azimuth.astype(np.float32)), torch.from_numpy(elevation.astype(np.float32))


def recenter(mesh, mesh_simp):
    """Move a pair of meshes to the centre of the SIMPLIFIED mesh's bounding box (utils.py:73-83).  Mesh objects that offer
    offset_verts_ (pytorch3d's Meshes) are moved in place; otherwise the arguments are (verts, verts_simp) arrays or tensors and the
    moved pair is returned."""
    if hasattr(mesh_simp, "offset_verts_"):
        vs = mesh_simp.verts_list()[0]
        center = (vs.min(dim=0).values + vs.max(dim=0).values)[None] / 2
        mesh.offset_verts_(-center.repeat(mesh.verts_list()[0].shape[0], 1))
        mesh_simp.offset_verts_(-center.repeat(vs.shape[0], 1))
        return None
    center = (mesh_simp.min(0) + mesh_simp.max(0)) / 2 if isinstance(mesh_simp, np.ndarray) else (mesh_simp.min(dim=0).values + mesh_simp.max(dim=0).values) / 2
    return mesh - center, mesh_simp - center

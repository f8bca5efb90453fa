"""
The semantic group distances of the reference's driver (densematcher/utils.py:115-143), under its names:

    from densematcher_amd.utils import get_distance_between_groups, get_groups_dmtx

Only these two functions of that module are mirrored (and a batched form of the second); nothing here imports its rendering
or plotting dependencies.  For every pair of vertex groups the reference solves a rectangular min-cost assignment on
D[np.ix_(g_i, g_j)] with SciPy and takes the mean matched distance.  On the device all pairs of all meshes are ONE call
(MatchEngine.groups_dmtx -> dm_lsa_gather): the same assignments, ties included; the means agree with the reference's to the
rounding of a sum of min(|g_i|, |g_j|) terms (NumPy adds them pairwise, the kernel in row order).

Routing (the pattern of pyFM.mesh.geometry.graph_engine): `device=None` takes the device when the process has a GPU and
DEVICE_DEFAULT is set, else the reference's SciPy loop on the host; `device=True` / `device=False` force a route
(device=True without a GPU fails as MatchEngine() does: there is no silent fall-back).
"""
import os

import numpy as np

# Whether device=None means the device in a process with a GPU.  Set from the measurement in DESIGN.md ("Semantic group
# distances"): the device route is the default only because its single-mesh time was below the host loop's at every
# group count measured.
DEVICE_DEFAULT = True


def _engine(device):
    """the engine of the device route, or None for the host route"""
    if device is None:
        import torch
        device = DEVICE_DEFAULT and torch.cuda.is_available()
    if not device:
        return None
    from .engine import default_engine
    return default_engine()


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
    eng = _engine(device)
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
    eng = _engine(device)
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
    eng = _engine(device)
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

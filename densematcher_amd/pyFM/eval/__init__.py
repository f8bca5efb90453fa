"""
Map quality measures that consume a geodesic distance matrix (reference: densematcher/pyFM/eval/evaluate.py:4-100): host NumPy,
the reference's arithmetic.  D1_geod / D2_geod come from TriMesh.get_geodesic (the heat method on the device, or Dijkstra).
"""
import numpy as np

__all__ = ["accuracy", "continuity", "coverage"]


def accuracy(p2p, gt_p2p, D1_geod, return_all=False, sqrt_area=None):
    """mean geodesic distance on the source shape between matched and ground-truth vertices (evaluate.py:4-35)"""
    dists = D1_geod[(p2p, gt_p2p)]
    if sqrt_area is not None:
        dists /= sqrt_area
    if return_all:
        return dists.mean(), dists
    return dists.mean()


def continuity(p2p, D1_geod, D2_geod, edges):
    """mean ratio of mapped edge length (source geodesics) to edge length (target geodesics) (evaluate.py:38-70)"""
    source_len = D2_geod[(edges[:, 0], edges[:, 1])]
    target_len = D1_geod[(p2p[edges[:, 0]], p2p[edges[:, 1]])]
    return np.mean(target_len / source_len)


def coverage(p2p, A):
    """area fraction of the source shape that the map reaches (evaluate.py:73-100); A: (n1, n1) area matrix or (n1,) vertex
    areas (the reference reads only the matrix form: its 1-D branch names an undefined variable)"""
    vert_area = np.asarray(A.sum(1)).flatten() if len(A.shape) == 2 else np.asarray(A)
    return vert_area[np.unique(p2p)].sum() / vert_area.sum()

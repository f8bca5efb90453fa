"""The reference's semantic group distances (densematcher/utils.py:115-143) restated over scipy.optimize.linear_sum_assignment, and
helpers the group tests share: Voronoi groups on a distance matrix and the bound on a mean's rounding."""
import numpy as np
from scipy.optimize import linear_sum_assignment


def pair_distance(D, g1, g2):
    """mean matched distance of the min-cost assignment on the block rows g1, columns g2; 0 when a group is empty"""
    if len(g1) == 0 or len(g2) == 0:
        return 0
    block = D[np.ix_(np.asarray(g1), np.asarray(g2))]
    r, c = linear_sum_assignment(block)
    return block[r, c].mean()


def groups_dmtx(D, groups):
    """(G, G): zero diagonal, the upper triangle from rows g_i / columns g_j (i < j), the lower triangle its mirror"""
    G = len(groups)
    out = np.zeros((G, G))
    for i in range(G):
        for j in range(i + 1, G):
            out[i, j] = out[j, i] = pair_distance(D, groups[i], groups[j])
    return out


def mean_bound(groups, ref):
    """(G, G) bounds n 2^-52 |ref| with n = min(|g_i|, |g_j|): two summation orders of the same n terms of one sign differ by at most
    (n - 1) 2^-53 of the sum each, plus a rounding of the division each"""
    n = np.asarray([[min(len(a), len(b)) for b in groups] for a in groups], np.float64)
    return n * 2.0 ** -52 * np.abs(ref)


def voronoi_groups(D, G, start=0):
    """G groups on the distance matrix D: farthest-point seeds from `start` (np.argmax of the running minimum of the seeds' rows),
    then every vertex to the seed whose row is smallest there (np.argmin: the first seed on ties).  Lists of int vertex indices."""
    seeds = [start]
    m = D[start].copy()
    for _ in range(G - 1):
        s = int(np.argmax(m))
        seeds.append(s)
        m = np.minimum(m, D[s])
    label = np.argmin(D[seeds], axis=0)
    return [np.flatnonzero(label == g).tolist() for g in range(G)]


def unpack_groups(flat, offsets):
    return [flat[offsets[g]:offsets[g + 1]].tolist() for g in range(len(offsets) - 1)]

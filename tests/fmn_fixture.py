"""Shared by test_fmn_cpu.py and test_gpu_fmn.py: the recorded run of the reference's functional map network (tests/golden/fx_fmn.npz,
written by tools/make_golden_fmn.py) as the objects the FMN class takes."""
import functools
import os

import numpy as np
import scipy.sparse as sparse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_fmn.npz")
CONFIGS = [("adjacency", True), ("adjacency", False), ("icsm", True), ("icsm", False)]
M0, STEP, NIT = 10, 2, 7


class Mesh:
    """what FMN reads of a mesh"""
    def __init__(self, verts, faces, lam, Phi, mass):
        self.vertlist, self.facelist = verts, faces
        self.eigenvalues, self.eigenvectors = lam, Phi
        self.A = sparse.diags(mass).tocsr()
        self.n_vertices = verts.shape[0]


@functools.lru_cache(maxsize=1)
def load():
    """(fx dict, meshes, edges, maps0 dict, samples) -- shared, never modified (FMN copies its meshes and maps)"""
    fx = dict(np.load(GOLDEN))
    meshes = [Mesh(fx[f"verts_{q}"], fx[f"faces_{q}"], fx[f"lam_{q}"], fx[f"Phi_{q}"], fx[f"mass_{q}"]) for q in range(5)]
    edges = [tuple(int(x) for x in e) for e in fx["edges"]]
    maps0 = {e: fx["maps0"][q] for q, e in enumerate(edges)}
    return fx, meshes, edges, maps0, fx["samples"].astype(np.int64)


def prefix(wt, use_sub):
    return f"{wt}_{'sub' if use_sub else 'full'}_"


def fixture_p2p(fx, pre, edges):
    return {e: fx[pre + f"p2p_{e[0]}{e[1]}"].astype(np.int64) for e in edges}


def keep_last_iteration(net):
    """compute_maps resets p2p, cclb_eigenvalues and the eigen-solver's residual (as the reference does): keep those of the last
    iteration in the returned dict"""
    kept, inner = {}, net.compute_maps

    def compute_maps(*a, **k):
        kept.update(p2p=dict(net.p2p), cclb_eigenvalues=np.array(net.cclb_eigenvalues), clb_eigenvalues=np.array(net.clb_eigenvalues))
        return inner(*a, **k)
    net.compute_maps = compute_maps
    return kept

#!/usr/bin/env python
"""
Functional-map-network fixture, produced by RUNNING THE REFERENCE's FMN class on the CPU.

    python tools/make_golden_fmn.py <reference checkout>        -> tests/golden/fx_fmn.npz

The reference's pyFM is imported WITHOUT its package __init__ (which pulls in plotting and mesh-IO dependencies): an empty module named
pyFM whose __path__ is the reference's pyFM directory is registered, then pyFM.spectral and pyFM.FMN.FMN are imported from it.

Collection: five tori on grids 20x12, 18x14, 22x11, 20x12, 16x15 (240, 252, 242, 240, 240 vertices), mesh 0 unperturbed, the others
radially perturbed; k = 40 eigenpairs of this package's host cotangent Laplacian (densematcher_amd.synth.eigenbasis).  All 20 directed
edges except (0, 3) and (4, 1).  Initial maps at M = 10 from nearest-vertex maps with 10 % of the entries replaced at random (seeded).
Euclidean farthest point samples of 96 from vertex 0.

Stored: the inputs (verts_i, faces_i, Phi_i, lam_i, mass_i, samples, edges, maps0), and for weight_type in {adjacency, icsm} x
{sub, full} (prefix e.g. "icsm_sub_"):
    after zoomout_refine(nit=7, step=2, M_init=10):  maps, and of its last iteration (compute_maps resets them) p2p_<e> per edge,
                                                     cclb_eigenvalues, W_evals (all eigenvalues of W)
    of the first iteration:  it1_iso_maps (the maps after set_isometries), it1_weights (E,), it1_cycle_costs, it1_lp_objective (icsm),
                             it1_W (dense), it1_W_evals, it1_cclb_eigenvalues, it1_p2p_<e>, it1_maps
The script also runs this package's host route on the same inputs, prints how many vertex-map entries differ from the reference's (0 when
the fixture is well posed) and the smallest relative gap lambda_m - lambda_{m-1} of W at the canonical basis' size m along the runs (a regenerated fixture must not be
near-degenerate there).
"""
import os
import sys
import types

import numpy as np
import scipy.sparse as sparse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "fx_fmn.npz")

GRIDS = [(20, 12), (18, 14), (22, 11), (20, 12), (16, 15)]
K, M0, NSUB, NIT, STEP = 40, 10, 96, 7, 2
SKIP = {(0, 3), (4, 1)}


class Mesh:
    """what FMN reads of a mesh"""
    def __init__(self, verts, faces, lam, Phi, mass):
        self.vertlist, self.facelist = verts, faces
        self.eigenvalues, self.eigenvectors = lam, Phi
        self.A = sparse.diags(mass).tocsr()
        self.n_vertices = verts.shape[0]


def import_reference(checkout):
    root = os.path.join(checkout, "densematcher", "pyFM")
    if not os.path.isdir(root):
        root = os.path.join(checkout, "pyFM")
    pkg = types.ModuleType("pyFM")
    pkg.__path__ = [root]
    sys.modules["pyFM"] = pkg
    import pyFM.spectral  # noqa: F401
    from pyFM.FMN.FMN import FMN
    return FMN


def fps_euclid(V, size, start=0):
    inds = [start]
    d = np.linalg.norm(V - V[start], axis=1)
    for _ in range(size - 1):
        inds.append(int(np.argmax(d)))
        d = np.minimum(d, np.linalg.norm(V - V[inds[-1]], axis=1))
    return np.asarray(inds)


def build_inputs():
    from densematcher_amd import synth
    meshes = []
    for q, (nu, nv) in enumerate(GRIDS):
        V, F = synth.torus_mesh(nu, nv, perturb=0.0 if q == 0 else 0.12, seed=10 + q)
        lam, Phi, mass = synth.eigenbasis(V, F, K, method="dense")
        meshes.append(Mesh(V, F, lam, Phi, mass))
    edges = sorted((i, j) for i in range(5) for j in range(5) if i != j and (i, j) not in SKIP)
    rng = np.random.default_rng(2024)
    maps0 = {}
    for (i, j) in edges:
        mi, mj = meshes[i], meshes[j]
        d2 = ((mj.vertlist[:, None, :] - mi.vertlist[None, :, :]) ** 2).sum(-1)
        p2p = d2.argmin(axis=1)                                             # vertex of mesh i nearest to each vertex of mesh j
        bad = rng.random(p2p.shape[0]) < 0.10
        p2p[bad] = rng.integers(mi.n_vertices, size=int(bad.sum()))
        maps0[(i, j)] = mj.eigenvectors[:, :M0].T @ (mj.A @ mi.eigenvectors[p2p, :M0])
    samples = np.stack([fps_euclid(m.vertlist, NSUB) for m in meshes])
    return meshes, edges, maps0, samples


def main():
    RefFMN = import_reference(sys.argv[1])
    from densematcher_amd.pyFM import FMN as OurFMN
    meshes, edges, maps0, samples = build_inputs()
    gaps = []

    class Rec(RefFMN):
        def compute_CLB(self, *a, **k):
            if self.W is None:
                self.compute_W()
            self.W_evals = np.linalg.eigvalsh(self.W.toarray())
            return super().compute_CLB(*a, **k)

        def compute_CCLB(self, m, *a, **k):         # (the gap at the size of the canonical basis conditions the vertex maps)
            ev = self.W_evals
            gaps.append((ev[m] - ev[m - 1]) / ev[-1])
            return super().compute_CCLB(m, *a, **k)

        def compute_maps(self, *a, **k):            # (compute_maps resets p2p and cclb_eigenvalues: keep the last iteration's)
            self.last_p2p, self.last_cclb_eigenvalues = dict(self.p2p), self.cclb_eigenvalues.copy()
            return super().compute_maps(*a, **k)

    out = {"edges": np.asarray(edges, np.int32), "samples": samples.astype(np.int32),
           "maps0": np.stack([maps0[e] for e in edges])}
    for q, m in enumerate(meshes):
        out[f"verts_{q}"], out[f"faces_{q}"] = m.vertlist, m.facelist.astype(np.int32)
        out[f"Phi_{q}"], out[f"lam_{q}"], out[f"mass_{q}"] = m.eigenvectors, m.eigenvalues, np.asarray(m.A.diagonal())

    total_diff = 0
    for wt in ("adjacency", "icsm"):
        for use_sub in (True, False):
            pre = f"{wt}_{'sub' if use_sub else 'full'}_"
            sub = samples if use_sub else None
            # ---- first iteration, step by step (the body of zoomout_iteration)
            net = Rec(meshes, maps_dict=maps0)
            net.subsample = sub
            net.M = M0
            net.set_isometries(M=M0)
            out[pre + "it1_iso_maps"] = np.stack([net.maps[e] for e in edges])
            net.set_weights(weight_type=wt)
            out[pre + "it1_weights"] = np.asarray([net.weights[i, j] for (i, j) in edges], dtype=np.float64)
            if wt == "icsm":
                out[pre + "it1_cycle_costs"] = net.cycle_weight.copy()
                out[pre + "it1_cycles"] = np.asarray(net.cycles, np.int32)
                from scipy.optimize import linprog
                res = linprog(net.edge_weights, A_ub=-net.A, b_ub=-net.cycle_weight, bounds=(0, float("inf")), method="highs-ds")
                out[pre + "it1_lp_objective"] = np.float64(res.fun)
            net.compute_W(M=M0)
            out[pre + "it1_W"] = net.W.toarray()
            net.compute_CLB()
            out[pre + "it1_W_evals"] = net.W_evals
            net.compute_CCLB(int(0.9 * M0))
            out[pre + "it1_cclb_eigenvalues"] = net.cclb_eigenvalues
            net.compute_p2p(complete=not use_sub)
            for e in edges:
                out[pre + f"it1_p2p_{e[0]}{e[1]}"] = net.p2p[e].astype(np.int16)
            net.compute_maps(M0 + STEP, complete=not use_sub)
            out[pre + "it1_maps"] = np.stack([net.maps[e] for e in edges])
            # ---- the whole refinement
            net = Rec(meshes, maps_dict=maps0)
            net.zoomout_refine(nit=NIT, step=STEP, subsample=sub, weight_type=wt, M_init=M0)
            out[pre + "maps"] = np.stack([net.maps[e] for e in edges])
            out[pre + "cclb_eigenvalues"] = net.last_cclb_eigenvalues
            out[pre + "W_evals"] = net.W_evals
            for e in edges:
                out[pre + f"p2p_{e[0]}{e[1]}"] = net.last_p2p[e].astype(np.int16)
            # ---- this package's host route on the same inputs
            ours = OurFMN(meshes, maps_dict=maps0, device=False)
            keep, inner = {}, ours.compute_maps
            ours.compute_maps = lambda *a, **k: (keep.update(ours.p2p), inner(*a, **k))[1]
            ours.zoomout_refine(nit=NIT, step=STEP, subsample=sub, weight_type=wt, M_init=M0)
            nd = sum(int(np.count_nonzero(keep[e] != net.last_p2p[e])) for e in edges)
            ne = sum(net.last_p2p[e].size for e in edges)
            md = max(float(np.abs(ours.maps[e] - net.maps[e]).max()) for e in edges)
            total_diff += nd
            print(f"{pre[:-1]}: final M = {net.M}, host route vs reference: {nd} of {ne} vertex-map entries differ, max |map difference| = {md:.3e}",
                  flush=True)
    print(f"smallest relative gap (lambda_m - lambda_(m-1)) / lambda_max of W at the canonical size m = int(0.9 M) along the runs: {min(gaps):.3e}")
    if min(gaps) < 1e-5 or total_diff:
        print("WARNING: the fixture is near-degenerate or the host route differs from the reference: do not commit it as it is")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""
Shape-difference fixture, produced by RUNNING THE REFERENCE's pyFM.spectral.shape_difference on the CPU.

    python tools/make_golden_sd.py <reference checkout>        -> tests/golden/fx_sd.npz

The reference's pyFM is imported WITHOUT its package __init__ (as tools/make_golden_fmn.py does): an empty module named pyFM whose
__path__ is the reference's pyFM directory is registered, then pyFM.spectral is imported from it.

Meshes: torus 20x12 (240 vertices, unperturbed, "0"), torus 18x14 (252 vertices, radially perturbed 0.12, seed 11, "1") and the 20x12
torus perturbed the same way ("2"); k = 40 eigenpairs of this package's host cotangent Laplacian (densematcher_amd.synth.eigenbasis,
method="dense"), W from synth.cotan_laplacian stored as COO.  Pair "m": mesh1 = 0, mesh2 = 1 with the nearest-vertex map, 10 % of its
entries replaced at random (seeded): it has repeats and is not surjective.  Pair "i": mesh1 = 0, mesh2 = 2 with p2p = None (the identity).

Stored: the inputs (verts_q, faces_q, Phi_q, lam_q, mass_q, W_row_q / W_col_q / W_val_q, p2p), and per pair, SD_type and
(k1, k2) in (5, None), (12, None), (17, 8), (40, 40) -- key "<pair>_<type>_<k1>_<k2 or N>_" + "a" / "c" -- the reference's compute_SD;
per pair and (k1, k2) the reference's mesh_p2p_to_FM map ("<pair>_FM_<k1>_<k2>") and area_SD / conformal_SD of it ("..._a", "..._c").

The script asserts that both branches of np.linalg.pinv's cut-off occur on these inputs (lambda_0 of mesh 0 is rounding noise: kept at
k1 = 5, cut at k1 = 12), that this package's host route reproduces every stored array bit for bit, and that a NumPy restatement of the
device's summation order stays inside the bounds the GPU tests use (tests/sd_restate.py), printing the share it uses.
"""
import os
import sys
import types

import numpy as np
import scipy.sparse as sparse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "fx_sd.npz")

K = 40
DIMS = [(5, None), (12, None), (17, 8), (40, 40)]


class Mesh:
    """what compute_SD reads of a mesh"""
    def __init__(self, verts, faces, lam, Phi, mass, W):
        self.vertlist, self.facelist = verts, faces
        self.eigenvalues, self.eigenvectors = lam, Phi
        self.A = sparse.diags(mass).tocsr()
        self.W = W
        self.n_vertices = verts.shape[0]


def import_reference(checkout):
    root = os.path.join(checkout, "densematcher", "pyFM")
    if not os.path.isdir(root):
        root = os.path.join(checkout, "pyFM")
    pkg = types.ModuleType("pyFM")
    pkg.__path__ = [root]
    sys.modules["pyFM"] = pkg
    import pyFM.spectral as ref_spectral
    return ref_spectral


def mesh_from_arrays(fx, q):
    """the mesh as the tests rebuild it from the stored arrays (W from its COO triplets)"""
    n = fx[f"verts_{q}"].shape[0]
    W = sparse.coo_matrix((fx[f"W_val_{q}"], (fx[f"W_row_{q}"], fx[f"W_col_{q}"])), shape=(n, n)).tocsr()
    return Mesh(fx[f"verts_{q}"], fx[f"faces_{q}"], fx[f"lam_{q}"], fx[f"Phi_{q}"], fx[f"mass_{q}"], W)


def build_inputs():
    from densematcher_amd import synth
    out = {}
    for q, (nu, nv, perturb) in enumerate([(20, 12, 0.0), (18, 14, 0.12), (20, 12, 0.12)]):
        V, F = synth.torus_mesh(nu, nv, perturb=perturb, seed=11)
        lam, Phi, mass = synth.eigenbasis(V, F, K, method="dense")
        W = synth.cotan_laplacian(V, F)[0].tocoo()
        out[f"verts_{q}"], out[f"faces_{q}"] = V, F.astype(np.int32)
        out[f"lam_{q}"], out[f"Phi_{q}"], out[f"mass_{q}"] = lam, np.ascontiguousarray(Phi), mass
        out[f"W_row_{q}"], out[f"W_col_{q}"], out[f"W_val_{q}"] = W.row.astype(np.int32), W.col.astype(np.int32), W.data
    d2 = ((out["verts_1"][:, None, :] - out["verts_0"][None, :, :]) ** 2).sum(-1)
    p2p = d2.argmin(axis=1)                                                  # vertex of mesh 0 nearest to each vertex of mesh 1
    rng = np.random.default_rng(2025)
    bad = rng.random(p2p.shape[0]) < 0.10
    p2p[bad] = rng.integers(out["verts_0"].shape[0], size=int(bad.sum()))
    assert len(np.unique(p2p)) < len(p2p) and len(np.unique(p2p)) < out["verts_0"].shape[0]
    out["p2p"] = p2p.astype(np.int32)
    return out


def main():
    ref = import_reference(sys.argv[1])
    import sd_restate as sdr
    from densematcher_amd.pyFM.spectral import shape_difference as ours
    fx = build_inputs()
    meshes = [mesh_from_arrays(fx, q) for q in range(3)]
    pairs = {"m": (meshes[0], meshes[1], fx["p2p"].astype(np.int64)), "i": (meshes[0], meshes[2], None)}
    out = dict(fx)
    for pn, (m1, m2, p2p) in pairs.items():
        for k1, k2 in DIMS:
            tag = f"{k1}_{'N' if k2 is None else k2}"
            for SD_type in ("spectral", "semican"):
                a, c = ref.compute_SD(m1, m2, k1=k1, k2=k2, p2p=p2p, SD_type=SD_type)
                out[f"{pn}_{SD_type}_{tag}_a"], out[f"{pn}_{SD_type}_{tag}_c"] = a, c
                a2, c2 = ours.compute_SD(m1, m2, k1=k1, k2=k2, p2p=p2p, SD_type=SD_type, device=False)
                assert np.array_equal(a, a2) and np.array_equal(c, c2), f"host route differs from the reference: {pn} {SD_type} {tag}"
            k2e = 3 * k1 if k2 is None else k2
            FM = ref.mesh_p2p_to_FM(np.arange(m2.n_vertices) if p2p is None else p2p, m1, m2, dims=(k1, k2e))
            out[f"{pn}_FM_{tag}"] = FM
            out[f"{pn}_FM_{tag}_a"] = ref.area_SD(FM)
            out[f"{pn}_FM_{tag}_c"] = ref.conformal_SD(FM, m1.eigenvalues, m2.eigenvalues)
            assert np.array_equal(out[f"{pn}_FM_{tag}_a"], ours.area_SD(FM))
            assert np.array_equal(out[f"{pn}_FM_{tag}_c"], ours.conformal_SD(FM, m1.eigenvalues, m2.eigenvalues))
    # ---- both branches of the cut-off
    lam = meshes[0].eigenvalues
    print(f"lambda_0 = {lam[0]:.3e}, 1e-15 lambda_4 = {1e-15 * lam[4]:.3e}, 1e-15 lambda_11 = {1e-15 * lam[11]:.3e}")
    assert np.linalg.pinv(np.diag(lam[:5]))[0, 0] != 0.0, "row 0 is not kept at k1 = 5: regenerate with other inputs"
    assert np.linalg.pinv(np.diag(lam[:12]))[0, 0] == 0.0, "row 0 is not cut at k1 = 12: regenerate with other inputs"
    for k1 in (5, 12, 17, 40):
        host, rule = np.diag(np.linalg.pinv(np.diag(lam[:k1]))), sdr.inv_rule(lam, k1)
        # (the same cut decisions; a kept entry is 1 / lambda to two ulps -- LAPACK's singular values of a diagonal matrix are its entries
        #  up to a rounding: equal bits at k1 = 5, 12, 17, one ulp apart on 11 of the 40 entries at k1 = 40)
        assert np.array_equal(host == 0.0, rule == 0.0) and (np.abs(host - rule) <= 2 * sdr.U * np.abs(rule)).all(), k1
        print(f"k1 = {k1}: pinv(diag(lambda)) against the rule: {int((host != rule).sum())} of {k1} entries differ (by at most two ulps)")
    for pn in pairs:
        for SD_type in ("spectral", "semican"):
            assert np.any(out[f"{pn}_{SD_type}_5_N_c"][0] != 0.0) and not np.any(out[f"{pn}_{SD_type}_12_N_c"][0] != 0.0)
    # ---- the device's summation order, restated, against the reference with the GPU tests' bounds
    worst = 0.0
    for pn, (m1, m2, p2p) in pairs.items():
        for k1, _ in DIMS:
            X = m1.eigenvectors[np.arange(m2.n_vertices) if p2p is None else p2p, :k1]
            mass = np.asarray(m2.A.diagonal())
            Ga, Gw = sdr.slab_restate(X, mass, m2.W)
            ra, rc = ref.compute_SD(m1, m2, k1=k1, p2p=p2p, SD_type="semican")
            Gc = sdr.inv_rule(lam, k1)[:, None] * Gw
            ba, bc = sdr.forms_bounds(X, mass, m2.W, lam1=lam, ref_w=rc)
            for got, r, bd in ((Ga, ra, ba), (Gc, rc, bc)):
                err = np.abs(got - r)
                assert (err <= bd).all(), (pn, k1)
                worst = max(worst, float((err[bd > 0] / bd[bd > 0]).max()))
    print(f"slab-ordered restatement against the reference: largest share of the bounds {worst:.3f}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

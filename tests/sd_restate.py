"""
Shape difference operators, test side: the reference's formulas in NumPy, the entrywise bounds the device route is held to, and a
restatement of the device's summation order (slabs of 16 vertices, 32 slabs per partial, partials added in order).

The bounds are the standard error bounds of two summation orders of the same products (u = 2^-52, fused multiply-add or not):

    Ga                        (N2 + 2) u |X|^T diag(a2) |X|
    Gw                        (N2 + nnz + 2) u |X|^T |W| |X|            nnz: the longest row of W
    SD_a from a given FM      (k2 + 2) u |FM|^T |FM|
    SD_c                      |inv1[i]| (bound of its plain form) + u |ref|     (the last multiplication)

inv1[i] = 1 / lam1[i] where |lam1[i]| > 1e-15 max_j |lam1[j]|, else exactly 0: np.linalg.pinv(np.diag(lam1)) -- the same cut
decisions, the kept entries equal to two ulps (LAPACK's SVD returns the entries of a diagonal matrix as singular values that are a
rounding off in places, the division adds one); the plain form's bound, at least 3 u |ref|, has room for it.  Where inv1[0] is not cut
(lam_0 is rounding noise that happens to exceed the cut-off) the bound on row 0 is of order one: the check is vacuous there BY
CONSTRUCTION -- the reference's own row 0 is noise divided by lam_0; where it is cut, row 0 must be exactly 0.
"""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -52
SLAB = 16          # PB_SLAB of dm_shapediff.hip: target vertices per staged slab
SLABS = 32         # PB_SLABS: slabs per workgroup (one partial per SLAB * SLABS vertices)


def inv_rule(lam1, k1):
    """the diagonal of np.linalg.pinv(np.diag(lam1[:k1])), by the rule"""
    l = np.asarray(lam1, np.float64)[:k1]
    keep = np.abs(l) > 1e-15 * np.abs(l).max()
    out = np.zeros(k1)
    out[keep] = 1.0 / l[keep]
    return out


def forms_ref(X, mass, W, lam1=None):
    """(Ga, Gw) of the host route (shape_difference.py:95-96)"""
    Ga = X.T @ sp.diags(mass).tocsr() @ X
    if lam1 is None:
        return Ga, X.T @ W @ X
    return Ga, np.linalg.pinv(np.diag(lam1[:X.shape[1]])) @ X.T @ W @ X


def forms_bounds(X, mass, W, lam1=None, ref_w=None):
    """entrywise bounds on (Ga, Gw); with lam1 the bound on diag(inv1) Gw (ref_w: the reference's conformal operator)"""
    n2 = X.shape[0]
    Wc = sp.csr_matrix(W)
    nnz = int(np.diff(Wc.indptr).max())
    aX = np.abs(X)
    ba = (n2 + 2) * U * (aX.T @ (np.abs(mass)[:, None] * aX))
    bw = (n2 + nnz + 2) * U * (aX.T @ (abs(Wc) @ aX))
    if lam1 is not None:
        bw = np.abs(inv_rule(lam1, X.shape[1]))[:, None] * bw + U * np.abs(ref_w)
    return ba, bw


def sd_ref(FM, lam1, lam2):
    """(SD_a, SD_c) of the host route (shape_difference.py:20, :44)"""
    k2, k1 = FM.shape
    return FM.T @ FM, np.linalg.pinv(np.diag(lam1[:k1])) @ FM.T @ (lam2[:k2, None] * FM)


def sd_bounds(FM, lam1, lam2, ref_c, dFM=None):
    """entrywise bounds on (SD_a, SD_c) from a given map; dFM: an entrywise bound on the perturbation of the map itself (the
    end-to-end spectral route), which adds |FM|^T |dFM| + |dFM|^T |FM| (lam2-weighted for the conformal operator)"""
    k2, k1 = FM.shape
    aF, l2 = np.abs(FM), np.abs(np.asarray(lam2, np.float64)[:k2])[:, None]
    ba = (k2 + 2) * U * (aF.T @ aF)
    bc = (k2 + 2) * U * (aF.T @ (l2 * aF))
    if dFM is not None:
        ba = ba + aF.T @ dFM + dFM.T @ aF
        bc = bc + aF.T @ (l2 * dFM) + dFM.T @ (l2 * aF)
    return ba, np.abs(inv_rule(lam1, k1))[:, None] * bc + U * np.abs(ref_c)


def fm_perturbation(X, Phi2, mass2):
    """entrywise bound on the error of dm_p2p_to_fm_f64's map Phi2^T (a2 * X): (N2 + 2) u |Phi2|^T (a2 |X|)"""
    return (X.shape[0] + 2) * U * (np.abs(Phi2).T @ (np.abs(mass2)[:, None] * np.abs(X)))


def slab_restate(X, mass, W):
    """(Ga, Gw) in the device's order: a row of W X adds its stored entries in CSR order, a slab of 16 vertices adds them in index
    order, a partial its 32 slabs in order, the result the partials in order (NumPy products, not fused)"""
    n2, k1 = X.shape
    Wc = sp.csr_matrix(W)
    Y = np.zeros((n2, k1))
    for i in range(n2):
        for q in range(Wc.indptr[i], Wc.indptr[i + 1]):
            Y[i] += Wc.data[q] * X[Wc.indices[q]]
    Ga, Gw = np.zeros((k1, k1)), np.zeros((k1, k1))
    for c0 in range(0, n2, SLAB * SLABS):
        pa, pw = np.zeros((k1, k1)), np.zeros((k1, k1))
        for s0 in range(c0, min(n2, c0 + SLAB * SLABS), SLAB):
            for i in range(s0, min(n2, s0 + SLAB)):
                pa += np.outer(X[i], mass[i] * X[i])
                pw += np.outer(X[i], Y[i])
        Ga += pa
        Gw += pw
    return Ga, Gw


def report(name, got, ref, bound):
    """print the largest used share of the bound, then hold every entry to it"""
    err = np.abs(np.asarray(got) - np.asarray(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    print(f"{name}: max |got - ref| = {err.max():.3e}, largest share of the bound = {share.max():.3f}")
    assert np.isfinite(np.asarray(got)).all(), name
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} entries beyond the bound, worst share {share.max():.3f}"


def check_cut_rows(name, got, lam1, k1):
    """the cut decision is the host's: a row whose inv1 is 0 is exactly 0 (and reported: is the check on row 0 vacuous?)"""
    inv = inv_rule(lam1, k1)
    host = np.diag(np.linalg.pinv(np.diag(np.asarray(lam1, np.float64)[:k1])))
    # (kept entries: 1 / lambda to two ulps -- LAPACK returns the singular values of a diagonal matrix a rounding off in places)
    assert np.array_equal(inv == 0.0, host == 0.0) and (np.abs(inv - host) <= 2 * U * np.abs(inv)).all(), f"{name}: the rule and np.linalg.pinv disagree"
    got = np.asarray(got)
    for i in np.flatnonzero(inv == 0.0):
        assert (got[i] == 0.0).all(), f"{name}: row {i} is cut on the host and not exactly 0 here"
    if inv[0] != 0.0 and abs(lam1[0]) < 1e-9 * np.abs(lam1[:k1]).max():
        print(f"{name}: lam_0 = {lam1[0]:.3e} is kept by the cut-off: row 0 is held to {abs(inv[0]):.1e} x the plain form's bound "
              "(vacuous where the plain row is itself rounding noise: the constant eigenvector of a mesh)")

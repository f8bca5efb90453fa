"""The heat method of pyFM (mesh/geometry.py:587-670) restated with SciPy: what tests/test_geodesic_cpu.py holds against the reference's
fixture and tests/test_gpu_geodesic.py holds the device against.  A helper module, not a test file."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def heat_restated(V, F, W, mass, t, sources, ground=0):
    """Contract steps 1-5: LU of A + tW and of W grounded at vertex `ground` (its row and column -> identity, its rhs -> 0);
    columns = sources."""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    n, ns = len(V), len(sources)
    W = sp.csr_matrix(W)
    K = (sp.diags(mass) + t * W).tocsc()
    keep = np.ones(n)
    keep[ground] = 0.0
    Dk = sp.diags(keep)
    Wg = (Dk @ W @ Dk + sp.diags(1.0 - keep)).tocsc()
    E = np.zeros((n, ns))
    E[sources, np.arange(ns)] = 1.0
    U = spla.splu(K).solve(E)
    v1, v2, v3 = (V[F[:, c]] for c in range(3))
    cr = np.cross(v2 - v1, v3 - v1)
    area = 0.5 * np.linalg.norm(cr, axis=1)
    nrm = cr / np.linalg.norm(cr, axis=1, keepdims=True)
    G = [np.cross(nrm, e) / (2 * area[:, None]) for e in (v3 - v2, v1 - v3, v2 - v1)]
    u1, u2, u3 = (U[F[:, c]] for c in range(3))
    g = (u2 - u1)[:, :, None] * G[1][:, None, :] + (u3 - u1)[:, :, None] * G[2][:, None, :]
    h = -g / np.linalg.norm(g, axis=-1, keepdims=True)
    div = np.zeros((n, ns))
    for c in range(3):
        np.add.at(div, F[:, c], np.einsum('ij,ipj->ip', area[:, None] * G[c], h))
    va = np.zeros(n)
    np.add.at(va, F.ravel(), np.repeat(area / 3, 3))
    rhs = mass[:, None] * (div / va[:, None])
    rhs[ground] = 0.0
    phi = spla.splu(Wg).solve(rhs)
    phi -= phi.min(0, keepdims=True)
    phi[sources, np.arange(ns)] = 0.0
    return phi

"""
Host route of the DiffusionNet operators: the definitions of diffusion_net.geometry.compute_operators in vectorised NumPy / SciPy,
float64 throughout.  It is what runs on a machine without a GPU, what the CPU tests pin to the reference's own functions
(tests/golden/fx_dnet.npz), and where the normals of a mesh come from when the device reports one it cannot define.

The Laplacian and the lumped masses are the closed formulas the reference's calls name (potpourri3d.cotan_laplacian(V, F, denom_eps),
potpourri3d.vertex_areas); parity with that wheel itself is unpinned (see the docstring of geometry.py).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

DENOM_EPS = 1e-10      # compute_operators: cotan_laplacian(..., denom_eps=1e-10)
MASS_EPS = 1e-8        # massvec += eps * mean(massvec); also the shift of the eigenproblem, L + eps I, sigma = eps
GRAD_EPS = 1e-5        # build_grad: eps_reg
DIVIDE_EPS = 1e-6      # normalize(): x / (|x| + 1e-6)


def face_normals(V, F):
    """unit face normals raw / (|raw| + 1e-6) and the norms |raw| (twice the areas)"""
    raw = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    nrm = np.linalg.norm(raw, axis=1)
    return raw / (nrm + DIVIDE_EPS)[:, None], nrm


def mesh_vertex_normals(V, F):
    """the sum of the unit face normals over the incident corners, divided by its plain norm (not a number where that is zero)"""
    fn = face_normals(V, F)[0]
    out = np.zeros(V.shape)
    for i in range(3):
        np.add.at(out, F[:, i], fn)
    with np.errstate(invalid="ignore", divide="ignore"):
        return out / np.linalg.norm(out, axis=-1, keepdims=True)


def vertex_normals(V, F):
    """mesh_vertex_normals with the reference's repair sequence for undefined normals (geometry.py:128-141): the bad vertices are
    moved by a seeded wiggle and all normals recomputed; those still undefined (unreferenced vertices) get seeded random normals"""
    normals = mesh_vertex_normals(V, F)
    bad = np.isnan(normals).any(axis=1, keepdims=True)
    if bad.any():
        bbox = np.amax(V, axis=0) - np.amin(V, axis=0)
        scale = np.linalg.norm(bbox) * 1e-4
        wiggle = (np.random.RandomState(seed=777).rand(*V.shape) - 0.5) * scale
        normals = mesh_vertex_normals(V + bad * wiggle, F)
    bad = np.isnan(normals).any(axis=1)
    if bad.any():
        normals[bad, :] = (np.random.RandomState(seed=777).rand(*V.shape) - 0.5)[bad, :]
        normals = normals / np.linalg.norm(normals, axis=-1)[:, np.newaxis]
    if np.isnan(normals).any():
        raise ValueError("NaN normals :(")
    return normals


def tangent_frames(normals):
    """(V, 3, 3) rows bx, by, n (geometry.py:151-177)"""
    n = np.asarray(normals, np.float64)
    use_x = np.abs(n[:, 0]) < 0.9
    cand = np.where(use_x[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    bx = cand - n * np.sum(cand * n, axis=-1)[:, None]
    bx = bx / (np.linalg.norm(bx, axis=-1) + DIVIDE_EPS)[:, None]
    by = np.cross(n, bx)
    frames = np.stack((bx, by, n), axis=-2)
    if np.isnan(frames).any():
        raise ValueError("NaN coordinate frame! Must be very degenerate")
    return frames


def cotan_laplacian(V, F, denom_eps=DENOM_EPS):
    """weak cotangent Laplacian (CSR, sorted columns): per corner k opposite the edge (i, j), cot = dot / (|cross| + denom_eps),
    L_ii, L_jj += cot / 2, L_ij, L_ji -= cot / 2.  Every pair of vertices that share a face has an entry, zeros included."""
    n = V.shape[0]
    I, J, S = [], [], []
    for k in range(3):
        i, j = F[:, (k + 1) % 3], F[:, (k + 2) % 3]
        u, w = V[i] - V[F[:, k]], V[j] - V[F[:, k]]
        half = 0.5 * (np.sum(u * w, axis=1) / (np.linalg.norm(np.cross(u, w), axis=1) + denom_eps))
        I += [i, j, i, j]
        J += [i, j, j, i]
        S += [half, half, -half, -half]
    L = sp.coo_matrix((np.concatenate(S), (np.concatenate(I), np.concatenate(J))), shape=(n, n)).tocsr()
    L.sort_indices()
    return L


def vertex_areas(V, F):
    """a third of the incident face areas"""
    area = 0.5 * face_normals(V, F)[1]
    return np.bincount(F.ravel(), weights=np.repeat(area / 3.0, 3), minlength=V.shape[0])


def grad_rows(n, rows, cols, tangent, grad_eps=GRAD_EPS):
    """build_grad (geometry.py:209-272) without its loops: edges (rows -> cols) with their tangent vectors (E, 2); per vertex
    M = sum t t^T + grad_eps I, g = M^-1 t, g_self = -sum g.  Returns the complex (n, n) CSC matrix gradX + i gradY."""
    keep = rows != cols
    r, c, t = rows[keep], cols[keep], np.asarray(tangent, np.float64)[keep]
    a = np.bincount(r, weights=t[:, 0] * t[:, 0], minlength=n) + grad_eps
    b = np.bincount(r, weights=t[:, 0] * t[:, 1], minlength=n)
    d = np.bincount(r, weights=t[:, 1] * t[:, 1], minlength=n) + grad_eps
    det = a * d - b * b
    gx = (d[r] * t[:, 0] - b[r] * t[:, 1]) / det[r]
    gy = (a[r] * t[:, 1] - b[r] * t[:, 0]) / det[r]
    sx, sy = np.bincount(r, weights=gx, minlength=n), np.bincount(r, weights=gy, minlength=n)
    me = np.arange(n)
    data = np.concatenate([-(sx + 1j * sy), gx + 1j * gy])
    return sp.coo_matrix((data, (np.concatenate([me, r]), np.concatenate([me, c]))), shape=(n, n)).tocsc()


def edge_tangents(V, frames, rows, cols):
    d = V[cols] - V[rows]
    return np.stack((np.sum(d * frames[rows, 0], axis=-1), np.sum(d * frames[rows, 1], axis=-1)), axis=-1)


def eigenbasis(L, mass, k_eig, eps=MASS_EPS):
    """geometry.py:336-365: eigsh(L + eps I, k, M, sigma = eps) with its retry ladder, eigenvalues clipped at 0"""
    n = L.shape[0]
    if k_eig <= 0:
        return np.zeros((0,)), np.zeros((n, 0))
    L_eigsh = (L + sp.identity(n) * eps).tocsc()
    Mmat = sp.diags(mass)
    fail = 0
    while True:
        try:
            evals, evecs = sla.eigsh(L_eigsh, k=k_eig, M=Mmat, sigma=eps)
            return np.clip(evals, a_min=0.0, a_max=float("inf")), evecs
        except Exception as e:
            if fail > 3:
                raise ValueError("failed to compute eigendecomp") from e
            fail += 1
            L_eigsh = L_eigsh + sp.identity(n) * (eps * 10 ** fail)


def operators(V, F, k_eig, normals=None):
    """(frames, mass, L, evals, evecs, gradX, gradY) of one mesh: float64 arrays and SciPy matrices"""
    V = np.ascontiguousarray(V, np.float64)
    F = np.asarray(F, np.int64)
    n = V.shape[0]
    frames = tangent_frames(vertex_normals(V, F) if normals is None else normals)
    L = cotan_laplacian(V, F)
    mass = vertex_areas(V, F)
    mass = mass + MASS_EPS * np.mean(mass)
    if np.isnan(L.data).any():
        raise RuntimeError("NaN Laplace matrix")
    if np.isnan(mass).any():
        raise RuntimeError("NaN mass matrix")
    evals, evecs = eigenbasis(L, mass, k_eig)
    Lc = L.tocoo()
    G = grad_rows(n, Lc.row, Lc.col, edge_tangents(V, frames, Lc.row, Lc.col))
    return frames, mass, L, evals, evecs, G.real.tocsc(), G.imag.tocsc()

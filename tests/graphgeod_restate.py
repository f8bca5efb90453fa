"""Shortest paths along mesh edges, restated for the tests: the graphs as the package builds them, the kernel's scheme in NumPy
(pull sweeps to a fixed point, warm-started sampling), the host sampling loop on SciPy's Dijkstra, and one constructed mesh."""
import numpy as np
import scipy.sparse as sparse
import scipy.sparse.csgraph as csgraph


def fps_graph_of(V, F):
    """the graph of the default TriMesh.extract_fps: directed face edges summed into CSR, then the larger direction"""
    V, F = np.asarray(V, np.float64), np.asarray(F)
    n = len(V)
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    w = np.linalg.norm(V[e[:, 0]] - V[e[:, 1]], axis=1)
    G = sparse.coo_matrix((w, (e[:, 0], e[:, 1])), shape=(n, n)).tocsr()
    return G.maximum(G.T)


def host_fps(G, size, start):
    """geometry.py:839-848 with d(i) = csgraph.dijkstra(G, directed=False, indices=i): the host loop of extract_fps"""
    inds = [int(start)]
    d = csgraph.dijkstra(G, directed=False, indices=inds[0])
    for _ in range(size - 1):
        inds.append(int(np.argmax(d)))
        d = np.minimum(d, csgraph.dijkstra(G, directed=False, indices=inds[-1]))
    return np.asarray(inds)


def ell_of(G):
    """in-edges of every vertex as (cols (nnz, n), w (nnz, n)), -1 pads: the layout of dm_graph_geodesic for one mesh"""
    Gi = sparse.csc_matrix(G)
    n = Gi.shape[0]
    rl = np.diff(Gi.indptr)
    nnz = max(1, int(rl.max()))
    cols = np.full((nnz, n), -1, np.int64)
    w = np.zeros((nnz, n))
    pos = np.arange(Gi.nnz) - np.repeat(Gi.indptr[:-1], rl)
    v = np.repeat(np.arange(n), rl)
    cols[pos, v] = Gi.indices
    w[pos, v] = Gi.data
    return cols, w


def relax(m, cols, w):
    """synchronous pull sweeps from m until one changes nothing; returns (fixed point, sweeps run)"""
    sweeps = 0
    while True:
        cand = np.where(cols >= 0, m[np.maximum(cols, 0)] + w, np.inf).min(axis=0)
        new = np.minimum(m, cand)
        sweeps += 1
        if np.array_equal(new, m):
            return m, sweeps
        m = new


def relax_all_pairs(G):
    cols, w = ell_of(G)
    n = G.shape[0]
    D = np.empty((n, n))
    most = 0
    for s in range(n):
        m = np.full(n, np.inf)
        m[s] = 0.0
        D[s], k = relax(m, cols, w)
        most = max(most, k)
    return D, most


def warm_fps(G, size, start):
    """the sampler's scheme: arg-max of the running minimum, m[new] = 0, relax from m.  Returns (indices, final m, sweeps per sample)"""
    cols, w = ell_of(G)
    m = np.full(G.shape[0], np.inf)
    inds, sweeps = [int(start)], []
    for s in range(size):
        m = m.copy()
        m[inds[-1]] = 0.0
        m, k = relax(m, cols, w)
        sweeps.append(k)
        if s + 1 < size:
            inds.append(int(np.argmax(m)))
    return np.asarray(inds), m, sweeps


def grid_faces(nx, ny, off=0):
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).ravel() + off
    return np.concatenate([np.stack([a, a + ny, a + 1], 1), np.stack([a + 1, a + ny, a + ny + 1], 1)])


def constructed_mesh():
    """301 vertices (a multiple of neither 64 nor 1024): a jittered 13 x 12 sheet (vertices 0..155), ONE vertex no face references
    (156: every distance to and from it is inf), a second 12 x 12 sheet (157..300) far away; vertices 40 and 41 coincide (an edge of
    length exactly 0).  From a start on the first sheet the first arg-max is 156, the lowest index among the inf entries."""
    rng = np.random.default_rng(20)
    def sheet(nx, ny, z):
        x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
        P = np.stack([x.ravel(), y.ravel(), np.full(nx * ny, z)], 1)
        return P + rng.uniform(-0.2, 0.2, P.shape)
    V = np.concatenate([sheet(13, 12, 0.0), [[50.0, 50.0, 50.0]], sheet(12, 12, 30.0)])
    F = np.concatenate([grid_faces(13, 12), grid_faces(12, 12, off=157)]).astype(np.int32)
    V[41] = V[40]
    assert len(V) == 301 and 156 not in F
    return V, F

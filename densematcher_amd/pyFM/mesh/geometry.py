"""
Geodesic distances on triangle meshes (reference: densematcher/pyFM/mesh/geometry.py), what the DenseMatcher notebook imports from
`pyFM.mesh.geometry` (`heat_geodmat_robust`, `geodesic_distmat_dijkstra`) and what TriMesh.get_geodesic / geod_from call.

The heat method (Crane et al. 2013) with the reference's own arithmetic -- heat_geodmat / heat_geodesic_from, geometry.py:587-740:
u = (A + tW)^-1 e_j, h = -grad u / |grad u| per face, phi = W^-1 (A div h), phi -= min phi, phi[j] = 0 -- runs ON THE DEVICE
(MatchEngine.heat_geodesic_factor / heat_geodesic: dense float64 Cholesky of both systems, W grounded at one vertex, where the
reference uses SciPy's SuperLU).  Column j of a matrix holds the distances FROM vertex j, as in the reference.

The reference's robust routes (`heat_geodmat_robust`, `robust=True` of the TriMesh methods) call the external potpourri3d wheel
(intrinsic Delaunay heat method).  When the wheel is importable it is used, as the reference does; when it is not, they FAIL
(ImportError): this package does not substitute another operator silently.  robust=False is the pinned route.
"""
import numpy as np
import scipy.sparse as sparse

_NO_PP3D = ("the robust heat method (potpourri3d.MeshHeatMethodDistanceSolver, what the reference calls in "
            "pyFM/mesh/geometry.py:559-584 and pyFM/mesh/trimesh.py:700-705) needs the `potpourri3d` package, which is not installed.  "
            "This package computes the reference's own heat method on the device: pass robust=False "
            "(TriMesh.get_geodesic(robust=False), TriMesh.geod_from(i, robust=False)) or call geometry.heat_geodmat")


def _pp3d():
    try:
        import potpourri3d
    except ImportError:
        raise ImportError(_NO_PP3D) from None
    return potpourri3d


def edges_from_faces(faces):
    """(p, 2) unique undirected edges, smaller index first, in the reference's order (geometry.py:9-45)"""
    faces = np.asarray(faces)
    N = 1 + np.max(faces)
    I = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]])
    J = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]])
    In = np.concatenate([I, J])
    Jn = np.concatenate([J, I])
    Vn = np.ones_like(In)
    M = sparse.csr_matrix((Vn, (In, Jn)), shape=(N, N)).tocoo()
    indices = M.col > M.row
    return np.concatenate([M.row[indices, None], M.col[indices, None]], axis=1)


def compute_normals(vertices, faces):
    """unit face normals (geometry.py:110-133)"""
    v1, v2, v3 = (vertices[faces[:, c]] for c in range(3))
    normals = np.cross(v2 - v1, v3 - v1)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return normals


def graph_engine():
    """the engine whose kernels compute the shortest paths along mesh edges (dm_graph_geodesic / dm_fps_graph), or None where SciPy's
    Dijkstra runs on the host instead: the option "graph_geod_device" = 0, or a process without a GPU (the host-only tools and
    tests).  The two routes return the same bits."""
    import torch
    if not torch.cuda.is_available():
        return None
    from ...engine import default_engine
    eng = default_engine()
    return eng if eng.get_option("graph_geod_device") else None


def edge_graph(vertices, faces):
    """the weighted edge graph of geometry.py:524-556: every unique undirected edge stored in both directions, Euclidean lengths"""
    vertices = np.asarray(vertices)
    N = vertices.shape[0]
    edges = edges_from_faces(faces)
    I, J = edges[:, 0], edges[:, 1]
    V = np.linalg.norm(vertices[J] - vertices[I], axis=1)
    return sparse.coo_matrix((np.concatenate([V, V]), (np.concatenate([I, J]), np.concatenate([J, I]))), shape=(N, N)).tocsc()


def geodesic_distmat_dijkstra_many(meshes):
    """geodesic_distmat_dijkstra for a list of (vertices, faces): ONE device call for the batch (meshes padded to the largest, each
    matrix bit-identical to its own call); the host loop where the device route does not apply.  Returns a list of (n, n) arrays."""
    graphs = [edge_graph(V, F) for V, F in meshes]
    D = _dijkstra_many_device(graphs)
    if D is not None:
        D = D.cpu().numpy()
        return [np.ascontiguousarray(D[b, :g.shape[0], :g.shape[0]]) for b, g in enumerate(graphs)]
    from scipy.sparse import csgraph
    return [csgraph.dijkstra(g) for g in graphs]


def _dijkstra_many_device(graphs):
    """the padded (B, N, N) device tensor of the all-pairs shortest paths of the edge graphs, or None where the device route does not
    apply (graph_engine; more than 16384 vertices or a hub vertex)"""
    from ...engine import GraphTooWide
    eng = graph_engine()
    if eng is None:
        return None
    try:
        return eng.graph_geodesic(graphs)
    except GraphTooWide:
        return None


def geodesic_distmat_dijkstra(vertices, faces):
    """all-pairs shortest paths along the mesh edges (geometry.py:524-556): row i = the distances from vertex i, the bits of the
    reference's csgraph.dijkstra.  On the device (dm_graph_geodesic) for meshes of up to 16384 vertices; SciPy on the host otherwise
    (see graph_engine)."""
    return geodesic_distmat_dijkstra_many([(vertices, faces)])[0]


def heat_geodmat_robust(vertices, faces, verbose=False):
    """the reference's potpourri3d route (geometry.py:559-584): used when the wheel is installed, ImportError otherwise"""
    pp3d = _pp3d()
    n_vertices = vertices.shape[0]
    distmat = np.zeros((n_vertices, n_vertices))
    solver = pp3d.MeshHeatMethodDistanceSolver(vertices, faces)
    for vertind in range(n_vertices):
        distmat[vertind] = np.maximum(solver.compute_distance(vertind), 0)
    return distmat


def lumped_mass(A):
    """diag(A) of a lumped (diagonal) mass matrix; ValueError for any other A (the device route takes the diagonal only)"""
    A = sparse.csr_matrix(A)
    mass = np.asarray(A.diagonal(), dtype=np.float64)
    if (A - sparse.diags(mass)).count_nonzero():
        raise ValueError("A: the lumped (diagonal) mass matrix is expected")
    return mass


def _same(given, mine):
    given = np.asarray(given, dtype=np.float64)
    return given.shape == mine.shape and np.allclose(given, mine, rtol=1e-10, atol=1e-14 * max(1.0, np.abs(mine).max()))


def _check_inputs(vertices, faces, normals, A, face_areas=None, vert_areas=None, grads=None):
    """The device recomputes the unit face normals, the face and vertex areas and the hat gradients from the vertices (what the
    reference does when they are not passed).  Passed values must be those (the sign of the normals does not enter the result: it
    flips every gradient and h together); anything else is refused rather than ignored."""
    vertices = np.asarray(vertices, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    v1, v2, v3 = (vertices[faces[:, c]] for c in range(3))
    mine_n = compute_normals(vertices, faces) if (normals is not None or grads is not None) else None
    if normals is not None:
        nrm = np.asarray(normals, dtype=np.float64)
        if nrm.shape != mine_n.shape or not np.allclose(np.abs(np.einsum('ij,ij->i', nrm, mine_n)), 1.0, rtol=0, atol=1e-6):
            raise ValueError("normals: the heat method runs on the unit face normals of the mesh (geometry.compute_normals)")
    area = 0.5 * np.linalg.norm(np.cross(v2 - v1, v3 - v1), axis=1)
    if face_areas is not None and not _same(face_areas, area):
        raise ValueError("face_areas: the heat method runs on the mesh's own face areas (compute_faces_areas, geometry.py:48-70)")
    if vert_areas is not None:
        va = np.zeros(len(vertices))
        np.add.at(va, faces.ravel(), np.repeat(area / 3, 3))
        if not _same(vert_areas, va):
            raise ValueError("vert_areas: the heat method runs on one third of the adjacent face areas (compute_vertex_areas, "
                             "geometry.py:73-107)")
    if grads is not None:
        g = np.asarray([np.cross(mine_n, e) / (2 * area[:, None]) for e in (v3 - v2, v1 - v3, v2 - v1)])
        gg = np.asarray(grads, dtype=np.float64)
        if not (_same(gg, g) or _same(-gg, g)):
            raise ValueError("grads: the heat method runs on the hat gradients of the mesh (_get_grad_dir, geometry.py:284-316)")
    return vertices, faces, lumped_mass(A)


def _source_indices(inds, n):
    """NumPy's indexing of the reference (delta[inds] = 1): -n <= i < n, negative counted from the end"""
    src = np.atleast_1d(np.asarray(inds, dtype=np.int64))
    if src.ndim != 1 or src.size == 0 or src.min() < -n or src.max() >= n:
        raise IndexError(f"source indices must lie in [-{n}, {n})")
    return np.where(src < 0, src + n, src)


def heat_geodmat(vertices, faces, normals, A, W, t=1e-3, face_areas=None, vert_areas=None, batch_size=None, verbose=False):
    """(n, n) heat-method distance matrix, column j = distances from vertex j (geometry.py:673-740), computed on the device.
    normals / face_areas / vert_areas, when given, must be the mesh's own (ValueError otherwise: _check_inputs); A must be a lumped
    mass equal to one third of the adjacent face areas (engine.heat_geodesic_check); batch_size is accepted and does not change
    the result."""
    from ...engine import default_engine, heat_geodesic_check
    vertices, faces, mass = _check_inputs(vertices, faces, normals, A, face_areas, vert_areas)
    heat_geodesic_check(vertices, faces, mass)
    eng = default_engine()
    fac = eng.heat_geodesic_factor([(vertices, faces, sparse.csr_matrix(W), mass)], float(t))
    return eng.heat_geodesic(fac)[0].cpu().numpy()


def heat_geodesic_from(inds, vertices, faces, normals, A, W=None, t=1e-3, face_areas=None, vert_areas=None, grads=None,
                       solver_heat=None, solver_lap=None):
    """heat-method distances from the vertices `inds` (geometry.py:587-670): (n,) for one index, (n, p) for p of them.
    W is required: the reference's optional host solver callables cannot run on the device."""
    if W is None or solver_heat is not None or solver_lap is not None:
        raise TypeError("heat_geodesic_from: pass the stiffness matrix W; host solver callables (solver_heat / solver_lap) cannot "
                        "run on the device")
    from ...engine import default_engine, heat_geodesic_check
    vertices, faces, mass = _check_inputs(vertices, faces, normals, A, face_areas, vert_areas, grads)
    heat_geodesic_check(vertices, faces, mass)
    scalar = not isinstance(inds, (list, np.ndarray))
    src = _source_indices(inds, len(vertices))
    eng = default_engine()
    fac = eng.heat_geodesic_factor([(vertices, faces, sparse.csr_matrix(W), mass)], float(t))
    D = eng.heat_geodesic(fac, src)[0].cpu().numpy()
    return D[:, 0] if scalar or D.shape[1] == 1 else D

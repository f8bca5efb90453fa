"""
MatchEngine, distances on meshes: heat-method geodesics, shortest paths along edges, farthest-point sampling.
"""
import numpy as np
import torch

from ._operands import counts, csr_to_ell, pad_stack, ptr as _ptr, raise_info, source_table, stack_ell, start_vertices


def heat_geodesic_check(V, F, mass, b=0):
    """Host checks of one mesh of MatchEngine.heat_geodesic_factor; ValueError where the reference's SuperLU fails or returns
    numbers that depend on its pivoting:
    * more than one connected component (vertices that no face references included): W is singular beyond its constant;
    * lumped masses that are not one third of the adjacent face areas (e.g. those of process(robust=True), the intrinsic
      Laplacian's): W phi = A div h is then inconsistent -- sum_i A_i div_i = 0 holds only for A_i = va_i, since
      sum_i va_i div_i = sum_f area_f (sum_c grad phi_c) . h_f = 0 -- and its solution depends on where W is grounded."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    n = V.shape[0]
    if V.ndim != 2 or V.shape[1] != 3:
        raise ValueError(f"heat_geodesic_factor: mesh {b}: vertices must be (n, 3)")
    if F.ndim != 2 or F.shape[1] != 3 or F.size == 0 or F.min() < 0 or F.max() >= n:
        raise ValueError(f"heat_geodesic_factor: mesh {b}: faces must be (m, 3) indices into the {n} vertices")
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]]])
    G = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    ncomp = connected_components(G, directed=False)[0]
    if ncomp != 1:
        raise ValueError(f"heat_geodesic_factor: mesh {b} has {ncomp} connected components (vertices that no face references "
                         "count as components of their own): the heat method's W is singular beyond its constant there "
                         "(the reference's SuperLU fails or returns pivot-dependent numbers)")
    mass = np.asarray(mass, np.float64).ravel()
    if len(mass) != n:
        raise ValueError(f"heat_geodesic_factor: mesh {b}: {len(mass)} masses for {n} vertices")
    area = 0.5 * np.linalg.norm(np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]), axis=1)
    va = np.zeros(n)
    np.add.at(va, F.ravel(), np.repeat(area / 3.0, 3))
    dev = np.abs(mass - va)
    if not np.all(dev <= 1e-8 * va):
        i = int(np.argmax(np.where(va > 0, dev / np.maximum(va, 1e-300), np.inf)))
        raise ValueError(f"heat_geodesic_factor: mesh {b}: the lumped mass A is not one third of the adjacent face areas (vertex {i}: "
                         f"{mass[i]:.6g} against {va[i]:.6g}), as after process(robust=True): W phi = A div h is then inconsistent, "
                         "and its solution depends on the solver's pivoting (the reference's SuperLU) or on the ground vertex.  Use "
                         "the cotangent Laplacian's W and A (process(robust=False) on a fresh mesh)")


class GraphTooWide(ValueError):
    """a graph outside what dm_graph_geodesic / dm_fps_graph take (more than 16384 vertices, a degree above
    MatchEngine.GRAPH_MAX_DEGREE): the mesh layer answers it with SciPy's Dijkstra on the host, the same bits"""


class _GeodesicOps:
    # ------------------------------------------------------------- heat-method geodesics (dm_heat_geodesic_*)
    _GEOD_INFO = ((1, "A + tW is not positive definite"),
                  (2, "the grounded stiffness matrix W is not positive definite (more than one connected component?)"),
                  (4, "the mesh has a face of zero area"),
                  (8, "a face index or a column of W lies outside the mesh's vertices"),
                  (16, "a vertex that no face references"))

    def _stiffness_rows(self, W, n, who, b):
        """the stiffness matrix of mesh b (n vertices) as ELL rows (cols (n, nnz) int32, w (n, nnz) float64) on the device: a SciPy
        sparse matrix is converted row by row in CSR order and padded with col = -1, val = 0; (cols, w) device rows (those of
        laplacian_ell) pass through"""
        import scipy.sparse as sp
        if sp.issparse(W):
            Wc = sp.csr_matrix(W)
            if Wc.shape != (n, n):
                raise ValueError(f"{who}: mesh {b}: W is {Wc.shape}, expected {(n, n)}")
            cols_h, vals_h = csr_to_ell(Wc.indptr, Wc.indices, Wc.data, n)
            return torch.as_tensor(cols_h).to(self.device), torch.as_tensor(vals_h).to(self.device)
        cols_d, w_d = W
        if cols_d.shape[0] != n or w_d.shape != cols_d.shape:
            raise ValueError(f"{who}: mesh {b}: device rows of shape {tuple(cols_d.shape)} for {n} vertices")
        return cols_d, w_d

    def heat_geodesic_factor(self, meshes, t):
        """Factor the two systems of the heat method (pyFM geometry.heat_geodmat: A + tW and W, geometry.py:716-718) for a batch
        of meshes, on the device (dm_heat_geodesic_factor: dense float64 Cholesky, W grounded at vertex 0).
        meshes: list of (verts (n,3), faces (m,3), W, mass (n,)) with W the stiffness matrix as a SciPy sparse matrix or as the
        (cols, w) device rows (n, nnz) of laplacian_ell; t: the heat time, one float or one per mesh.  Fails closed (ValueError)
        on a mesh of more than one connected component (vertices that no face references included), masses that are not one
        third of the adjacent face areas (heat_geodesic_check), a face of zero area or a system that is not positive definite.  Returns the factors (a dict holding the device buffer) for heat_geodesic."""
        Bn = len(meshes)
        if Bn == 0:
            raise ValueError("heat_geodesic_factor: no meshes")
        ts = np.broadcast_to(np.asarray(t, np.float64), (Bn,)).copy()
        n_verts, rows = [], []
        for b, (V, F, W, mass) in enumerate(meshes):
            heat_geodesic_check(V, F, mass, b)
            n = len(V)
            rows.append(self._stiffness_rows(W, n, "heat_geodesic_factor", b))
            n_verts.append(n)
        N = max(n_verts)
        nt = max(len(m[1]) for m in meshes)
        tri_h = pad_stack([m[1] for m in meshes], (nt, 3), -1, np.int32)
        vert_h = pad_stack([m[0] for m in meshes], (N, 3), 0.0, np.float64)
        mass_h = pad_stack([np.asarray(m[3], np.float64).ravel() for m in meshes], (N,), 0.0, np.float64)
        cols, wv = stack_ell(rows, N, self.device)
        tri_d, vert_d, mass_d = (torch.as_tensor(x).to(self.device) for x in (tri_h, vert_h, mass_h))
        t_d = torch.as_tensor(ts).to(self.device)
        nv_d = torch.as_tensor(np.asarray(n_verts, np.int32)).to(self.device)
        nbytes = int(self.lib.dm_heat_geodesic_bytes(Bn, N, nt))
        if nbytes == 0:
            raise ValueError(f"heat_geodesic_factor: meshes of up to 16384 vertices (got {N})")
        buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_heat_geodesic_factor(self.ctx, Bn, N, nt, _ptr(tri_d), _ptr(vert_d), _ptr(cols), _ptr(wv), cols.shape[2], _ptr(mass_d),
                                                   _ptr(t_d), _ptr(nv_d), _ptr(buf), _ptr(info)))
        raise_info(info.cpu().numpy(), self._GEOD_INFO, "heat_geodesic_factor")
        return {"buf": buf, "B": Bn, "N": N, "nt": nt, "n_verts": n_verts, "t": ts}

    def heat_geodesic(self, factors, sources=None, sym=False):
        """Heat-method geodesic distances from the factors of heat_geodesic_factor (dm_heat_geodesic_solve): the reference's
        heat_geodesic_from / heat_geodmat (geometry.py:587-740) for robust=False.
        sources: None = all pairs; a 1-D list of vertex indices shared by every mesh; or one list per mesh (the same length, -1 = none).
        Returns a device tensor D (B, N, ns) float64 with D[b, :, s] = the distances FROM sources[s] (a column of the reference's
        matrix; rows past a mesh's vertex count are 0).  sym=True (all pairs only): (D + D^T) / 2 as the reference forms it
        (trimesh.py:677-679).  A column's bits do not depend on the other sources or meshes of the call."""
        Bn, N = factors["B"], factors["N"]
        if sym and sources is not None:
            raise ValueError("heat_geodesic: sym=True needs all pairs (sources=None)")
        src = source_table(sources, factors["n_verts"], N, "heat_geodesic")
        ns = src.shape[1]
        src_d = torch.as_tensor(src).to(self.device)
        rows = torch.empty((Bn, ns, N), dtype=torch.float64, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_heat_geodesic_solve(self.ctx, Bn, N, factors["nt"], _ptr(factors["buf"]), ns, _ptr(src_d), _ptr(rows),
                                                  _ptr(info)))
        raise_info(info.cpu().numpy(), ((~0, "a source lies outside [-1, n_verts)"),), "heat_geodesic")
        D = rows.transpose(1, 2)
        if sym:
            D = D * 0.5
            D = D + D.transpose(1, 2)
        return D.contiguous()

    # ------------------------------------------------------------- farthest-point sampling (dm_fps_*)
    def fps(self, verts, size, start, n_verts=None):
        """Farthest-point sampling on Euclidean distances (geometry.py:839-848 with the distance of trimesh.py:872-873), the
        reference's indices.  verts (B,N,3) or (N,3) float64; start: one index or (B,); n_verts (B,) for padded batches.
        Returns (B,size) int32 on the device."""
        verts = self._dev(verts, torch.float64, "verts")
        if verts.dim() == 2:
            verts = verts[None]
        if verts.dim() != 3 or verts.shape[2] != 3:
            raise ValueError("fps: verts must be (B,N,3)")
        Bn, N = int(verts.shape[0]), int(verts.shape[1])
        if N > 16384:
            raise ValueError(f"fps: meshes of up to 16384 vertices (got {N})")
        try:
            nv = counts(n_verts, Bn, N, 1, "fps")
            st = start_vertices(start, nv, "fps")
        except ValueError:
            raise ValueError("fps: start indices must lie in [0, n_verts), n_verts in [1, N]") from None
        st_d = torch.as_tensor(st).to(self.device)
        nv_d = torch.as_tensor(nv).to(self.device)
        out = torch.empty((Bn, int(size)), dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_fps_euclid(self.ctx, Bn, N, _ptr(verts), _ptr(nv_d), int(size), _ptr(st_d), _ptr(out)))
        return out

    def fps_heat(self, factors, size, start):
        """Farthest-point sampling on the heat-method distances of heat_geodesic_factor's factors: d(i) = geod_from(i, robust=False).
        start: one index or one per mesh.  Returns (B,size) int32 on the device.  The whole sampling is one call without host
        synchronisation ("fps_heat_route": all-pairs rows + one sampling launch, or one single-source solve per sample)."""
        Bn, N = factors["B"], factors["N"]
        st_d = torch.as_tensor(start_vertices(start, factors["n_verts"], "fps_heat")).to(self.device)
        out = torch.empty((Bn, int(size)), dtype=torch.int32, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_fps_heat(self.ctx, Bn, N, factors["nt"], _ptr(factors["buf"]), int(size), _ptr(st_d), _ptr(out), _ptr(info)))
        raise_info(info.cpu().numpy(), ((1, "a start vertex outside the mesh"), (2, "a distance that is not finite")), "fps_heat")
        return out

    # ------------------------------------------------------------- shortest paths along mesh edges (dm_graph_geodesic / dm_fps_graph)
    GRAPH_MAX_DEGREE = 64
    _GRAPH_INFO = ((1, "a source or start vertex outside the mesh"),
                   (2, "an edge weight that is negative or NaN (shortest paths by relaxation need weights >= 0)"),
                   (4, "a column outside the mesh's vertices"))

    def _graph_ell(self, graphs, who):
        """the ELL operands of dm_graph_geodesic / dm_fps_graph for a list of SciPy sparse matrices: G[i, j] stored = an edge i -> j
        of that weight (explicit zeros included, as csgraph reads a sparse matrix).  Vertex-minor layout (B, nnz, N), vertex v's
        entries = the edges INTO v, meshes padded to the largest, the width = the largest in-degree of the batch.  A degree above
        GRAPH_MAX_DEGREE = 64 raises GraphTooWide (a ValueError): every vertex of every mesh walks the padded width in every sweep, so
        one hub vertex would set the cost of the whole batch; mesh edge graphs stay far below (valence 6 on average)."""
        import scipy.sparse as sp
        Bn = len(graphs)
        if Bn == 0:
            raise ValueError(f"{who}: no graphs")
        ins, n_verts = [], []
        for b, G in enumerate(graphs):
            if not sp.issparse(G) or G.shape[0] != G.shape[1] or G.shape[0] < 1:
                raise ValueError(f"{who}: mesh {b}: a square SciPy sparse matrix is expected")
            Gi = sp.csc_matrix(G)                                                # column v = the edges into v (no entry is dropped or summed)
            ins.append(Gi)
            n_verts.append(Gi.shape[0])
        N = max(n_verts)
        if N > 16384:
            raise GraphTooWide(f"{who}: meshes of up to 16384 vertices (got {N})")
        nnz = max(1, max(int(np.diff(Gi.indptr).max()) for Gi in ins))
        if nnz > self.GRAPH_MAX_DEGREE:
            raise GraphTooWide(f"{who}: a vertex of degree {nnz}: the device route takes degrees up to {self.GRAPH_MAX_DEGREE}")
        cols_h = np.full((Bn, nnz, N), -1, np.int32)
        w_h = np.zeros((Bn, nnz, N), np.float64)
        for b, Gi in enumerate(ins):
            c, w = csr_to_ell(Gi.indptr, Gi.indices, Gi.data, n_verts[b], nnz)
            cols_h[b, :, :n_verts[b]], w_h[b, :, :n_verts[b]] = c.T, w.T
        nv_d = torch.as_tensor(np.asarray(n_verts, np.int32)).to(self.device)
        return {"B": Bn, "N": N, "nnz": nnz, "n_verts": n_verts, "nv_d": nv_d,
                "cols": torch.as_tensor(cols_h).to(self.device), "w": torch.as_tensor(w_h).to(self.device)}

    def graph_geodesic(self, graphs, sources=None):
        """Shortest-path distances on weighted graphs (dm_graph_geodesic): scipy.sparse.csgraph.dijkstra(G, indices=sources) BIT FOR
        BIT, the reference's geodesic_distmat_dijkstra (geometry.py:524-556) when G is the edge graph of a mesh.
        graphs: list of square SciPy sparse matrices, G[i, j] stored = an edge i -> j (store both directions of an undirected edge;
        explicit zeros are edges), weights >= 0 (negative or NaN: ValueError); up to 16384 vertices, degrees up to GRAPH_MAX_DEGREE
        (GraphTooWide, a ValueError, beyond either).
        sources: None = all pairs; a 1-D list of vertex indices shared by every mesh; or one list per mesh (the same length, -1 = none).
        Returns a device tensor D (B, ns, N) float64 with D[b, s] = the distances FROM sources[s] (row s of csgraph.dijkstra's
        matrix; +inf where no path leads; columns past a mesh's vertex count and rows without a source are 0).  A row's bits do not
        depend on the other sources or meshes of the call."""
        ell = self._graph_ell(graphs, "graph_geodesic")
        Bn, N = ell["B"], ell["N"]
        src = source_table(sources, ell["n_verts"], N, "graph_geodesic")
        ns = src.shape[1]
        src_d = torch.as_tensor(src).to(self.device)
        D = torch.empty((Bn, ns, N), dtype=torch.float64, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_graph_geodesic(self.ctx, Bn, N, ell["nnz"], _ptr(ell["cols"]), _ptr(ell["w"]), _ptr(ell["nv_d"]), ns,
                                             _ptr(src_d), _ptr(D), _ptr(info)))
        raise_info(info.cpu().numpy(), self._GRAPH_INFO, "graph_geodesic")
        return D

    def fps_graph(self, graphs, size, start):
        """Farthest-point sampling on the shortest-path distances of graph_geodesic (dm_fps_graph): the loop of geometry.py:839-848 with
        d(i) = csgraph.dijkstra(G, indices=i), the same indices (+inf is a maximum, the lowest index among equal maxima).
        graphs as for graph_geodesic; start: one index or one per mesh.  Returns (B,size) int32 on the device.  The whole sampling
        of the batch is ONE launch without host synchronisation."""
        ell = self._graph_ell(graphs, "fps_graph")
        Bn = ell["B"]
        if int(size) < 1:
            raise ValueError("fps_graph: size must be positive")
        st_d = torch.as_tensor(start_vertices(start, ell["n_verts"], "fps_graph")).to(self.device)
        out = torch.empty((Bn, int(size)), dtype=torch.int32, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_fps_graph(self.ctx, Bn, ell["N"], ell["nnz"], _ptr(ell["cols"]), _ptr(ell["w"]), _ptr(ell["nv_d"]), int(size),
                                        _ptr(st_d), _ptr(out), _ptr(info)))
        raise_info(info.cpu().numpy(), self._GRAPH_INFO, "fps_graph")
        return out

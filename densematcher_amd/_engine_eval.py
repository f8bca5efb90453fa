"""
MatchEngine, evaluation: ragged assignments gathered from one distance matrix, group distances, map quality measures.
"""
import numpy as np
import torch

from ._operands import counts, host_ptr, index_list, numpy_index, problem_meshes, ptr as _ptr


class _EvalOps:
    # ------------------------------------------------------------- ragged assignments gathered from one matrix (dm_lsa_gather)
    def _lsa_gather_D(self, D, who):
        """D as the (B, N, ld) float64 device operand of dm_lsa_gather: a device tensor is used where it is when its strides fit the
        ABI (unit stride along a row, one row stride ld >= N, meshes N ld apart); anything else is copied.  Returns (tensor, B, N, ld)."""
        if not isinstance(D, torch.Tensor):
            import warnings
            with warnings.catch_warnings():                  # (a read-only array is only read)
                warnings.simplefilter("ignore", UserWarning)
                D = torch.as_tensor(D)
        if D.dim() == 2:
            D = D[None]
        if D.dim() != 3 or D.shape[1] != D.shape[2] or D.shape[1] < 1:
            raise ValueError(f"{who}: D must be (N, N) or (B, N, N)")
        D, ld = self._strided(D, torch.float64, "D")
        return D, int(D.shape[0]), int(D.shape[1]), ld

    def _lsa_gather_run(self, D, idx, table, maximize, return_assignment, n_out):
        """dm_lsa_gather on a prepared index array (n_idx,) and problem table (P, 6), both int32 NumPy; the means (P,) float64 and,
        on request, the packed col_of_row (n_out,) int32, as NumPy arrays.  Raises SciPy's errors."""
        Dd, B, N, ld = D
        P = int(table.shape[0])
        if P == 0:
            return np.zeros(0, np.float64), (np.zeros(0, np.int32) if return_assignment else None)
        idx_d = torch.as_tensor(np.ascontiguousarray(idx, np.int32)).to(self.device)
        table = np.ascontiguousarray(table, np.int32)
        mean = torch.empty((P,), dtype=torch.float64, device=self.device)
        info = torch.empty((P,), dtype=torch.int32, device=self.device)
        out = torch.empty((max(1, n_out),), dtype=torch.int32, device=self.device) if return_assignment else None
        self._chk(self.lib.dm_lsa_gather(self.ctx, B, N, ld, _ptr(Dd), int(idx_d.numel()), _ptr(idx_d), P,
                                         host_ptr(table), 1 if maximize else 0, _ptr(out), _ptr(mean), _ptr(info)))
        self._raise_lsa(info)
        return mean.cpu().numpy(), (out.cpu().numpy() if return_assignment else None)

    def lsa_gather(self, D, row_lists, col_lists, mesh=None, maximize=False, return_assignment=False, n_verts=None):
        """Many assignments on sub-blocks of one matrix in ONE device call (dm_lsa_gather): problem p is
        scipy.optimize.linear_sum_assignment(D[mesh[p]][np.ix_(row_lists[p], col_lists[p])], maximize) -- the same assignment, ties
        included -- and the mean of its matched entries (the reference's get_distance_between_groups, densematcher/utils.py:115-127).
        D: (N, N) or (B, N, N), NumPy or torch; a float64 device tensor is read in place (a padded batch as heat_geodesic /
        graph_geodesic return it, or a view of one with a row stride).  row_lists / col_lists: P sequences of vertex indices
        (repeats and overlaps allowed, none empty); mesh: the mesh of every problem (default 0); n_verts (B,): the vertex counts of a
        padded batch, for the index check (default N).
        Returns the means (P,) float64 (NumPy); with return_assignment=True also the list of col_of_row arrays (int32, -1 for an
        unassigned row when a problem has more rows than columns).  ValueError with SciPy's texts for an infeasible problem and for
        NaN / the rejected infinity; ValueError for an index outside its mesh and for an empty list."""
        Dt = self._lsa_gather_D(D, "lsa_gather")
        B, N = Dt[1], Dt[2]
        P = len(row_lists)
        if len(col_lists) != P:
            raise ValueError("lsa_gather: as many column lists as row lists")
        mesh, nv = problem_meshes(mesh, P, B, "lsa_gather"), counts(n_verts, B, N, 1, "lsa_gather")
        parts, table, off, ooff = [], np.zeros((P, 6), np.int32), 0, 0
        for p in range(P):
            r = index_list(row_lists[p], int(nv[mesh[p]]), "lsa_gather")
            c = index_list(col_lists[p], int(nv[mesh[p]]), "lsa_gather")
            if r.size == 0 or c.size == 0:
                raise ValueError(f"lsa_gather: problem {p}: an empty index list")
            table[p] = (mesh[p], off, r.size, off + r.size, c.size, ooff)
            parts += [r, c]
            off += r.size + c.size
            ooff += r.size
        idx = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        means, packed = self._lsa_gather_run(Dt, idx, table, maximize, return_assignment, ooff)
        if not return_assignment:
            return means
        return means, [packed[table[p, 5]:table[p, 5] + table[p, 2]] for p in range(P)]

    def groups_dmtx(self, D, groups, n_verts=None):
        """The semantic distance matrices between vertex groups (the reference's get_groups_dmtx, densematcher/utils.py:129-143) of
        a batch of meshes in ONE lsa_gather call: out[i, j] = out[j, i] (i < j) = the mean matched distance of the assignment on
        D[np.ix_(groups[i], groups[j])], 0 on the diagonal and for a pair with an empty group.
        D (N, N) with one list of groups -> one (G, G) float64 NumPy array; D (B, N, N) (meshes padded to the largest, n_verts (B,)
        their vertex counts) with one list of groups per mesh (any numbers of groups) -> a list of B arrays."""
        single = (D.dim() if isinstance(D, torch.Tensor) else np.ndim(D)) == 2
        Dt = self._lsa_gather_D(D, "groups_dmtx")
        B, N = Dt[1], Dt[2]
        per_mesh = [groups] if single else list(groups)
        if len(per_mesh) != B:
            raise ValueError(f"groups_dmtx: {len(per_mesh)} lists of groups for {B} meshes")
        nv = counts(n_verts, B, N, 1, "groups_dmtx")
        parts, off, rows, where = [], 0, [], []
        for b, gs in enumerate(per_mesh):
            lists = [index_list(g, int(nv[b]), f"groups_dmtx: mesh {b}") for g in gs]
            offs = []
            for g in lists:                                  # every group once in the index array, whatever the number of its pairs
                offs.append(off)
                parts.append(g)
                off += g.size
            for i in range(len(lists)):
                for j in range(i + 1, len(lists)):
                    if lists[i].size and lists[j].size:
                        rows.append((b, offs[i], lists[i].size, offs[j], lists[j].size, 0))
                        where.append((b, i, j))
        table = np.asarray(rows, np.int32).reshape(-1, 6)
        idx = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        means, _ = self._lsa_gather_run(Dt, idx, table, False, False, 0)
        out = [np.zeros((len(gs), len(gs)), np.float64) for gs in per_mesh]
        for (b, i, j), m in zip(where, means):
            out[b][i, j] = out[b][j, i] = m
        return out[0] if single else out

    # ------------------------------------------------------------- map quality measures on the geodesic matrices (dm_map_metrics)
    MM_ACCURACY, MM_CONTINUITY, MM_COVERAGE = 0, 1, 2

    class _IndexPool:
        """the index array of one call: a list object that several problems pass is stored once"""

        def __init__(self):
            self.parts, self.off, self.seen = [], 0, {}

        def add(self, obj, extra, make):
            key = (id(obj),) + extra
            if key not in self.seen:
                a = make()
                self.seen[key] = (self.off, a, obj)          # (obj is held: its id stays its own for the call)
                self.parts.append(a)
                self.off += a.size
            return self.seen[key][:2]

        def array(self):
            return np.concatenate(self.parts) if self.parts else np.zeros(0, np.int32)

    def _map_metrics_run(self, D, D2, nv, nv2, area, idx, table, scale, n_all):
        """ONE dm_map_metrics launch on a prepared index array and table (P, 8); the values (P,) and `all` (n_all,) as NumPy arrays.
        D / D2: the tuples of _lsa_gather_D or None; area: (B, N) float64 device or None."""
        P = int(table.shape[0])
        if P == 0:
            return np.zeros(0, np.float64), np.zeros(0, np.float64)
        if D is not None:
            Dd, B, N, ld = D
        else:
            Dd, B, N, ld = None, int(area.shape[0]), int(area.shape[1]), int(area.shape[1])
        D2d, B2, N2, ld2 = D2 if D2 is not None else (None, 0, 0, 0)
        idx_d = torch.as_tensor(np.ascontiguousarray(idx, np.int32)).to(self.device) if len(idx) else torch.zeros(1, dtype=torch.int32, device=self.device)
        table = np.ascontiguousarray(table, np.int32)
        scale = None if scale is None else np.ascontiguousarray(scale, np.float64)
        value = torch.empty((P,), dtype=torch.float64, device=self.device)
        info = torch.empty((P,), dtype=torch.int32, device=self.device)
        every = torch.empty((n_all,), dtype=torch.float64, device=self.device) if n_all else None
        self._chk(self.lib.dm_map_metrics(self.ctx, B, N, ld, _ptr(Dd), B2, N2, ld2, _ptr(D2d), host_ptr(nv), host_ptr(nv2), _ptr(area),
                                          int(len(idx)), _ptr(idx_d), P, host_ptr(table), host_ptr(scale), int(n_all),
                                          _ptr(value), _ptr(every), _ptr(info)))
        if int(info.max()) != 0:                             # (the lists were checked here: not reached through this class)
            raise IndexError("map metrics: an index outside its mesh")
        return value.cpu().numpy(), (every.cpu().numpy() if n_all else np.zeros(0, np.float64))

    def map_metrics_table(self, idx, table, D=None, D2=None, area=None, scale=None, n_verts=None, n_verts2=None, n_all=0):
        """dm_map_metrics as the header states it, for callers that build the table themselves (problems of all three kinds in one
        launch): idx (n_idx,) int32 non-negative indices, table (P, 8) int32 rows (kind, mesh, mesh2, offset a, offset b, length,
        aux, flags), scale (P,) or None; D / D2 as in lsa_gather, area (B, N).  Returns (values (P,), all (n_all,)) as NumPy arrays;
        ValueError for a table the library refuses, IndexError for an index outside its mesh."""
        Dt = None if D is None else self._lsa_gather_D(D, "map_metrics_table")
        D2t = None if D2 is None else self._lsa_gather_D(D2, "map_metrics_table")
        if area is not None:
            area = self._dev(area if isinstance(area, torch.Tensor) else torch.as_tensor(np.asarray(area, np.float64)), torch.float64, "area")
            area = area[None] if area.dim() == 1 else area
        if Dt is None and area is None:
            raise ValueError("map_metrics_table: D or area is needed")
        if Dt is not None and area is not None and tuple(area.shape) != (Dt[1], Dt[2]):
            raise ValueError("map_metrics_table: area must be (B, N) like D")
        B, N = (Dt[1], Dt[2]) if Dt is not None else (int(area.shape[0]), int(area.shape[1]))
        nv = counts(n_verts, B, N, 1, "map_metrics_table")
        nv2 = None if (D2t is None or n_verts2 is None) else counts(n_verts2, D2t[1], D2t[2], 1, "map_metrics_table")
        table = np.asarray(table, np.int32).reshape(-1, 8)
        return self._map_metrics_run(Dt, D2t, nv, nv2, area, np.asarray(idx, np.int32).reshape(-1), table, scale, int(n_all))

    def geodesic_diameter(self, D, n_verts=None):
        """np.max(D[b, :n_verts[b], :n_verts[b]]) of every mesh of a padded batch (dm_geodesic_diameter; the diameter that the
        reference's geodesic_label_errors normalises by, diffusion_net/geometry.py:773): (B,) float64 NumPy, NaN where an entry is
        NaN.  D: (N, N) or (B, N, N), NumPy or torch; a float64 device tensor is read in place."""
        Dd, B, N, ld = self._lsa_gather_D(D, "geodesic_diameter")
        nv = counts(n_verts, B, N, 1, "geodesic_diameter")
        out = torch.empty((B,), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_geodesic_diameter(self.ctx, B, N, ld, _ptr(Dd), host_ptr(nv), _ptr(out)))
        return out.cpu().numpy()

    def map_accuracy(self, D, p2p_list, gt_list, mesh=None, scale=None, return_all=False, n_verts=None):
        """The reference's accuracy (pyFM/eval/evaluate.py:29-36) for P maps in ONE device call: problem p is
        d = D[mesh[p]][(p2p_list[p], gt_list[p])] -- the row from the map, the column from the ground truth --, d /= scale[p] element
        by element where a scale is given, and d.mean().  D as in lsa_gather (a float64 device tensor is read in place); index lists
        with NumPy's rules (-n <= i < n, IndexError otherwise); a list object passed for several problems is uploaded once.
        scale: None, one number, one number per problem, or "diameter" (geodesic_diameter, once for the batch).  An empty list gives
        NumPy's nan without a launch.  Returns the means (P,) float64 NumPy; with return_all=True also the list of the d arrays."""
        Dt = self._lsa_gather_D(D, "map_accuracy")
        B, N = Dt[1], Dt[2]
        p2p_list, gt_list = list(p2p_list), list(gt_list)
        P = len(p2p_list)
        if len(gt_list) != P:
            raise ValueError("map_accuracy: as many ground-truth lists as maps")
        mesh, nv = problem_meshes(mesh, P, B, "map_accuracy"), counts(n_verts, B, N, 1, "map_accuracy")
        if isinstance(scale, str):
            if scale != "diameter":
                raise ValueError("map_accuracy: scale must be None, numbers or 'diameter'")
            sc = self.geodesic_diameter(Dt[0], nv)[mesh]
        elif scale is not None:
            sc = np.array(np.broadcast_to(np.asarray(scale, np.float64), (P,)))
        else:
            sc = None
        pool, rows, where, n_all = self._IndexPool(), [], [], 0
        values = np.full(P, np.nan)
        for p in range(P):
            n = int(nv[mesh[p]])
            oa, a = pool.add(p2p_list[p], (n,), lambda: numpy_index(p2p_list[p], n, "map_accuracy"))
            ob, b = pool.add(gt_list[p], (n,), lambda: numpy_index(gt_list[p], n, "map_accuracy"))
            if a.size != b.size:
                raise ValueError(f"map_accuracy: problem {p}: a map of {a.size} and a ground truth of {b.size} entries")
            if a.size == 0:
                values[p] = np.zeros(0).mean()               # (NumPy's nan and its warning)
                continue
            flags = (1 if sc is not None else 0) | (2 if return_all else 0)
            rows.append((self.MM_ACCURACY, mesh[p], 0, oa, ob, a.size, n_all, flags))
            where.append(p)
            n_all += a.size if return_all else 0
        table = np.asarray(rows, np.int32).reshape(-1, 8)
        where = np.asarray(where, np.int64)
        got, every = self._map_metrics_run(Dt, None, nv, None, None, pool.array(), table, None if sc is None else sc[where], n_all)
        values[where] = got
        if not return_all:
            return values
        dists = [np.zeros(0) for _ in range(P)]
        for row, p in zip(table, where):
            dists[p] = every[row[6]:row[6] + row[5]].copy()
        return values, dists

    def map_continuity(self, D1, D2, p2p_list, edges_list, mesh1=None, mesh2=None, n_verts1=None, n_verts2=None):
        """The reference's continuity (pyFM/eval/evaluate.py:63-66) for P maps in ONE device call: problem p is
        np.mean(D1[mesh1[p]][(p2p[e0], p2p[e1])] / D2[mesh2[p]][(e0, e1)]) over the edges (e0, e1) = edges_list[p] (E, 2) of the
        target mesh, p2p = p2p_list[p] its map into the source mesh.  D2=None: both sides are meshes of D1.  IEEE division without
        guards: an edge of length zero gives inf or nan and the mean carries it, as NumPy's does.  Index rules, sharing of list
        objects, empty lists and the return as in map_accuracy."""
        D1t = self._lsa_gather_D(D1, "map_continuity")
        D2t = D1t if D2 is None else self._lsa_gather_D(D2, "map_continuity")
        p2p_list, edges_list = list(p2p_list), list(edges_list)
        P = len(p2p_list)
        if len(edges_list) != P:
            raise ValueError("map_continuity: as many edge lists as maps")
        mesh1, nv1 = problem_meshes(mesh1, P, D1t[1], "map_continuity"), counts(n_verts1, D1t[1], D1t[2], 1, "map_continuity")
        mesh2, nv2 = problem_meshes(mesh2, P, D2t[1], "map_continuity"), counts(n_verts1 if (D2 is None and n_verts2 is None) else n_verts2, D2t[1], D2t[2], 1, "map_continuity")
        pool, rows, where = self._IndexPool(), [], []
        values = np.full(P, np.nan)

        def edge_lists(edges, n_map, n2):
            e = np.asarray(edges.cpu() if isinstance(edges, torch.Tensor) else edges)
            if e.ndim != 2 or e.shape[1] != 2:
                raise ValueError("map_continuity: edges must be (E, 2)")
            flat = e.T.reshape(-1)                           # every e0, then every e1
            in_map = numpy_index(flat, n_map, "map_continuity")
            if n_map != n2 and not np.array_equal(in_map, numpy_index(flat, n2, "map_continuity")):
                raise ValueError("map_continuity: negative edge indices need a map with one entry per target vertex")
            return in_map

        for p in range(P):
            n1, n2 = int(nv1[mesh1[p]]), int(nv2[mesh2[p]])
            oa, a = pool.add(p2p_list[p], (n1,), lambda: numpy_index(p2p_list[p], n1, "map_continuity"))
            if a.size == 0 and np.size(edges_list[p]):
                raise IndexError("map_continuity: index 0 is out of bounds for axis 0 with size 0")
            ob, e = pool.add(edges_list[p], (a.size, n2), lambda: edge_lists(edges_list[p], a.size, n2))
            if e.size == 0:
                values[p] = np.zeros(0).mean()
                continue
            rows.append((self.MM_CONTINUITY, mesh1[p], mesh2[p], oa, ob, e.size // 2, a.size, 0))
            where.append(p)
        table = np.asarray(rows, np.int32).reshape(-1, 8)
        got, _ = self._map_metrics_run(D1t, D2t, nv1, nv2, None, pool.array(), table, None, 0)
        values[np.asarray(where, np.int64)] = got
        return values

    def map_coverage(self, area, p2p_list, mesh=None, n_verts=None):
        """The reference's coverage (pyFM/eval/evaluate.py:89-91) for P maps in ONE device call: problem p is
        area[mesh[p]][np.unique(p2p_list[p])].sum() / area[mesh[p]][:n].sum().  area: (N,) or (B, N) vertex areas, NumPy or torch.
        Index rules, sharing of list objects and the return as in map_accuracy; an empty map covers nothing (0.0, as NumPy gives)."""
        if not isinstance(area, torch.Tensor):
            area = torch.as_tensor(np.asarray(area, np.float64))
        if area.dim() == 1:
            area = area[None]
        if area.dim() != 2 or area.shape[1] < 1:
            raise ValueError("map_coverage: area must be (N,) or (B, N)")
        area = self._dev(area, torch.float64, "area")
        B, N = int(area.shape[0]), int(area.shape[1])
        p2p_list = list(p2p_list)
        P = len(p2p_list)
        mesh, nv = problem_meshes(mesh, P, B, "map_coverage"), counts(n_verts, B, N, 1, "map_coverage")
        pool, rows = self._IndexPool(), []
        for p in range(P):
            n = int(nv[mesh[p]])
            oa, a = pool.add(p2p_list[p], (n,), lambda: numpy_index(p2p_list[p], n, "map_coverage"))
            rows.append((self.MM_COVERAGE, mesh[p], 0, oa, 0, a.size, 0, 0))
        table = np.asarray(rows, np.int32).reshape(-1, 8)
        return self._map_metrics_run(None, None, nv, None, area, pool.array(), table, None, 0)[0]

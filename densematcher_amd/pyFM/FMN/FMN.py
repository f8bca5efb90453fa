"""
Functional map networks: consistent latent bases and Consistent ZoomOut, with the reference's names (densematcher/pyFM/FMN/FMN.py).

    from densematcher_amd.pyFM import FMN, CLB_quad_form
    net = FMN(meshes, maps_dict)                  # meshes: processed TriMesh objects, maps_dict[(i, j)] = FM_ij (basis i -> basis j)
    net.zoomout_refine(nit=10, step=2, subsample=500, weight_type='icsm')
    net.maps[(i, j)], net.p2p[(i, j)], net.CCLB

Routing (densematcher_amd._routes.engine_for): `device=None` takes the device when the process has a GPU and DEVICE_DEFAULT is
set, `device=True` / `device=False` force a route (True without a GPU fails as MatchEngine() does: there is no silent fall-back).

Host route: the reference's computation in NumPy / SciPy -- the restatement the tests pin to the recorded reference -- with three
replacements that leave the result where the reference's is defined: the M smallest eigenpairs of W by scipy.linalg.eigh on the dense
matrix instead of ARPACK's shift-invert, the eigenpairs of E / n by the symmetric solver instead of the general one, and the nearest
neighbours by scipy.spatial.cKDTree instead of scikit-learn's kd-tree.

Device route: the maps of all edges live in ONE (E, L, L) device tensor (they must share one square size), and an iteration is
    dm_fmn_orth_defect (set_isometries) -> [dm_fmn_cycle_costs -> host LP] -> dm_fmn_quad_form -> dm_eigh_smallest -> dm_fmn_cclb
    -> one batched product for the latent bases -> dm_knn_query_f64 per group of edges -> dm_p2p_to_fm_lstsq_f64 / dm_p2p_to_fm_f64.
Limits: n M <= 4096 and M <= 256 (ValueError beyond; device=False still works).  Attributes read by users (`maps`, `p2p`, `CLB`,
`CCLB`, `cclb_eigenvalues`, `weights`) come back as NumPy; `W` is a SciPy CSR matrix on the host route and a dense device tensor behind
a wrapper (np.asarray / .toarray() / .device_tensor()) on the device route.

Signs: ARPACK returns eigenvectors with arbitrary signs and an arbitrary basis inside a multiple eigenvalue.  Both routes here fix the
sign of every eigenvector (of W, and of E) so that its entry of largest magnitude is positive (the lowest index on ties), the rule of
dm_eigenbasis.  Results that depend on the basis inside a multiple eigenvalue are not comparable between routes, as in the reference.

Synchronisation: a device iteration reads back the eigensolver's residual (once on the Jacobi route, once per round on the filtered
route: MatchEngine.eigh_smallest raises when it does not converge) and, with a subsample, the status word of the least-squares maps
(MatchEngine.p2p_to_fm_lstsq, once per group of edges); everything else of an adjacency iteration is enqueued without a read-back.  With
weight_type='icsm' the linear program of the weights (E variables, scipy.optimize.linprog(method='highs-ds')) stays on the host in both
routes: one more synchronisation per iteration for the cycle costs.
"""
import copy

import numpy as np
import scipy.linalg
import scipy.sparse as sparse

from ... import _routes

# Whether device=None means the device in a process with a GPU.  Set from the measurement in DESIGN.md ("Functional map networks").
DEVICE_DEFAULT = True

MAX_DIM, MAX_M = 4096, 256          # limits of the device route: n M and M (MatchEngine.FMN_MAX_DIM / FMN_MAX_M)


def _is_tensor(x):
    if type(x).__module__.split(".")[0] != "torch":
        return False
    import torch
    return isinstance(x, torch.Tensor)


def _to_numpy(x):
    return x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)


def _fix_signs(V):
    """columns of V with their entry of largest magnitude positive (the lowest row on ties)"""
    V = np.array(V, dtype=np.float64)
    rows = np.argmax(np.abs(V), axis=0)
    V[:, V[rows, np.arange(V.shape[1])] < 0] *= -1.0
    return V


def _fps_euclid_host(V, size, start):
    """farthest point sampling on Euclidean distances from vertex `start` (the reference's loop, geometry.py:839-848)"""
    V = np.asarray(V, dtype=np.float64)
    inds = [int(start)]
    dists = np.linalg.norm(V - V[inds[0], None, :], axis=1)
    for _ in range(size - 1):
        inds.append(int(np.argmax(dists)))
        dists = np.minimum(dists, np.linalg.norm(V - V[inds[-1], None, :], axis=1))
    return np.asarray(inds)


class DeviceMatrix:
    """A dense float64 matrix that lives on the device (the quadratic form W of the device route): np.asarray(x) / x.toarray() copy it
    to the host once, x.device_tensor() is the tensor itself."""
    def __init__(self, tensor):
        self._t = tensor
        self._host = None
        self.shape = tuple(tensor.shape)
        self.ndim = 2
        self.dtype = np.dtype(np.float64)

    def device_tensor(self):
        return self._t

    def __array__(self, dtype=None, copy=None):
        if self._host is None:
            self._host = self._t.cpu().numpy()
        return self._host if dtype is None else self._host.astype(dtype)

    def toarray(self):
        return np.asarray(self)


class _HostView:
    """attribute kept as a device tensor (or a structure of them) by the device route and read by users as NumPy"""
    def __init__(self, name, convert=_to_numpy):
        self.slot, self.convert = "_" + name, convert

    def __get__(self, obj, cls=None):
        if obj is None:
            return self
        v = getattr(obj, self.slot, None)
        return None if v is None else self.convert(v)

    def __set__(self, obj, value):
        setattr(obj, self.slot, value)


def _p2p_view(v):
    if isinstance(v, dict):
        return v
    out = {}
    for edges, t in v:                      # device route: groups of edges that shared a search call
        h = t.cpu().numpy().astype(np.int64)
        for r, e in enumerate(edges):
            out[e] = h[r]
    return out


class FMN:
    """Functional map network (reference FMN.py:18-687): n shapes, a functional map on every directed edge (i, j) of a graph, taking
    basis i to basis j.

    meshlist  : list of TriMesh with `eigenvectors`, `eigenvalues`, `A` (TriMesh.process / process_many)
    maps_dict : {(i, j): FM_ij}, NumPy arrays or device tensors
    device    : None | True | False, see the module docstring
    """
    CLB = _HostView("CLB")
    CCLB = _HostView("CCLB")
    cclb_eigenvalues = _HostView("cclb_eigenvalues")
    clb_eigenvalues = _HostView("clb_eigenvalues")
    p2p = _HostView("p2p", _p2p_view)

    def __init__(self, meshlist, maps_dict=None, device=None):
        self.meshlist = copy.deepcopy(meshlist)
        self._eng = _routes.engine_for(device, DEVICE_DEFAULT)

        self.edges = None           # sorted list of (i, j)
        self._maps = None           # host route: dict; device route: (E, L, L) tensor in the order of `edges`
        self.weights = None         # (n, n) sparse matrix of edge weights
        self.edge2ind = None

        self.subsample = None       # (n, K) vertex indices per shape

        self.cycles = None          # list of three-cycles (i, j, k)
        self.A = None               # (n_cycles, n_edges) 0/1: edge in cycle
        self.A_sub = None           # indices of the edges that lie in a cycle
        self.use_icsm = False
        self.cycle_weight = None    # cost of every cycle (map dependent)
        self.edge_weights = None    # cost of every edge in the linear program (map dependent)
        self.icsm_objective = None  # optimum of the linear program of the last ICSM weights

        self.W = None               # (n M, n M) quadratic form
        self._CLB = None            # (n, M, M)
        self._clb_eigenvalues = None   # (M,) eigenvalues of W that go with the CLB
        self.clb_resid = None       # device route: max |W x - lam x| of the CLB's eigenpairs
        self._CCLB = None           # (n, M, m)
        self._cclb_eigenvalues = None
        self._p2p = None
        self._M = None
        self._dev_cache = {}

        if maps_dict is not None:
            self.set_maps(maps_dict=maps_dict, verbose=True)

    # ------------------------------------------------------------------ sizes
    @property
    def n_meshes(self):
        return len(self.meshlist)

    @property
    def M(self):
        """the shared size of the (square) functional maps in use: the one set, else the size of the first map"""
        if self._M is not None:
            return self._M
        if self._eng is not None:
            return int(self._maps.shape[1])
        return self._maps[self.edges[0]].shape[0]

    @M.setter
    def M(self, M):
        self._M = M

    @property
    def m_cclb(self):
        return self._CCLB.shape[2]

    # ------------------------------------------------------------------ maps
    @property
    def maps(self):
        """{(i, j): FM_ij} as NumPy.  On the device route this is a COPY of the device tensor: change maps with set_maps."""
        if self._maps is None or isinstance(self._maps, dict):
            return self._maps
        h = self._maps.cpu().numpy()
        return {e: h[q] for q, e in enumerate(self.edges)}

    @maps.setter
    def maps(self, value):
        if value is None:
            self._maps = None
        else:
            self.set_maps(value)

    def _reset_map_attributes(self):
        """forget what was computed from the maps (ICSM weights included: they are a function of the maps; given or adjacency weights stay)"""
        if self.use_icsm:
            self.use_icsm, self.weights, self.cycle_weight, self.edge_weights = False, None, None, None
        self.W = self.clb_resid = None
        for slot in ("_CLB", "_clb_eigenvalues", "_CCLB", "_cclb_eigenvalues", "_p2p"):
            setattr(self, slot, None)

    def set_maps(self, maps_dict, verbose=False):
        """Set the edges of the graph and their maps (:126-149).  FM may be NumPy arrays or device tensors; the device route needs
        them all of one square size."""
        self.edges = sorted(maps_dict)
        self.edge2ind = {edge: q for q, edge in enumerate(self.edges)}
        if self._eng is None:
            self._maps = {e: np.array(_to_numpy(maps_dict[e]), dtype=np.float64) for e in maps_dict}     # (the caller's key order)
        else:
            import torch
            shapes = {tuple(maps_dict[e].shape) for e in self.edges}
            if len(shapes) != 1 or len(next(iter(shapes))) != 2 or next(iter(shapes))[0] != next(iter(shapes))[1]:
                raise ValueError(f"FMN (device route): the maps must share one square size, got {sorted(shapes)}")
            dev = self._eng.device
            self._maps = torch.stack([maps_dict[e].to(device=dev, dtype=torch.float64) if _is_tensor(maps_dict[e])
                                      else torch.as_tensor(np.asarray(maps_dict[e], dtype=np.float64)).to(dev) for e in self.edges]).contiguous()
        if verbose:
            print(f"FMN: {len(self.edges)} directed edges between {self.n_meshes} meshes")
        return self

    # ------------------------------------------------------------------ samples
    def set_subsample(self, subsample):
        """(n, size) vertex indices per shape (:151-162)"""
        self.subsample = subsample
        self._dev_cache.pop("sub", None)
        return self

    def compute_subsample(self, size=1000, geodesic=False, verbose=False, rng=None, starts=None):
        """Farthest point samples of `size` vertices on every shape (:164-178: extract_fps(size, geodesic=geodesic, random_init=False) per
        mesh; the reference's start vertex is random all the same).  `rng` / `starts`: the generator of the start vertices or the start
        vertices themselves.  Device route: ONE sampling call for the collection (TriMesh.extract_fps_many)."""
        if verbose:
            print(f"FMN: farthest point sampling, {size} vertices per mesh")
        rng = np.random.default_rng() if rng is None else rng
        if starts is None:
            starts = [int(rng.integers(mesh.n_vertices)) for mesh in self.meshlist]
        if self._eng is not None:
            got = type(self.meshlist[0]).extract_fps_many(self.meshlist, size, geodesic=geodesic, starts=starts)
            sub = np.stack([np.asarray(g) for g in got]).astype(int)
        else:
            sub = np.zeros((self.n_meshes, size), dtype=int)
            for i, mesh in enumerate(self.meshlist):
                if geodesic:
                    sub[i] = mesh.extract_fps(size, geodesic=True, random_init=False, start=starts[i])
                else:
                    sub[i] = _fps_euclid_host(mesh.vertlist, size, starts[i])
        self.set_subsample(sub)

    # ------------------------------------------------------------------ weights
    def _weights_matrix(self, values):
        """(n, n) CSR matrix with values[e] at the position (i, j) of edge e"""
        rows, cols = zip(*self.edges)
        return sparse.csr_matrix((np.asarray(values, dtype=np.float64), (rows, cols)), shape=(self.n_meshes, self.n_meshes))

    def _icsm_edge_weights(self, verbose=False):
        """exp(-(d / sigma)^2 / 2) per edge: d solves the cycle-consistency linear program (optimize_icsm), sigma is the median of d over
        the edges that lie in a three-cycle, or their mean when that median is within 1e-4 of zero"""
        if self.cycles is None:
            if verbose:
                print("FMN: listing the three-cycles of the graph")
            self.extract_3_cycles()
            self.compute_Amat()
        d = self.optimize_icsm(verbose=verbose)
        in_cycles = d[self.A_sub]
        sigma = np.median(in_cycles)
        if np.isclose(sigma, 0, atol=1e-4):
            sigma = in_cycles.mean()
        return np.exp(-0.5 * np.square(d / sigma))

    def set_weights(self, weights=None, weight_type='icsm', verbose=False):
        """Edge weights (:180-232): a given (n, n) sparse matrix (copied), else by weight_type: 'adjacency' = 1 on every edge, 'icsm' = the
        cycle-consistency weights of _icsm_edge_weights (map dependent: forgotten again when the maps change)."""
        if weights is None and weight_type not in ('icsm', 'adjacency'):
            raise ValueError(f"FMN.set_weights: weight_type is 'icsm' or 'adjacency', got {weight_type!r}")
        self.use_icsm = weights is None and weight_type == 'icsm'
        if weights is not None:
            self.weights = copy.deepcopy(weights)
        elif self.use_icsm:
            self.weights = self._weights_matrix(self._icsm_edge_weights(verbose=verbose))
        else:
            self.weights = self._weights_matrix(np.ones(len(self.edges)))
        return self

    def _edge_weight_vector(self):
        """(E,) weights of the edges in the order of `edges`"""
        rows, cols = zip(*self.edges)
        return np.asarray(sparse.csr_matrix(self.weights)[list(rows), list(cols)], dtype=np.float64).ravel()

    def set_isometries(self, M=None):
        """For every pair of opposite edges keep the map whose leading M x M block is closer to orthogonal (the smaller
        |FM^T FM - I|_F; a tie keeps (i, j) with i < j) and replace the other one by its transpose -- of the whole stored map, not of
        the block (:234-270).  Resets what depends on the maps."""
        if M is None:
            M = self.M
        pairs = []
        visited = set()
        for (i, j) in self.edges:
            if (i, j) not in visited and (j, i) in self.edge2ind:
                pairs.append(((i, j), (j, i)))
                visited.add((j, i))
        if self._eng is None:
            def defect(edge):
                block = self._maps[edge][:M, :M]
                gram = block.T @ block
                return np.linalg.norm(gram - np.eye(gram.shape[0]))
            for forward, backward in pairs:                                  # (every edge lies in at most one pair)
                keep, replace = (forward, backward) if defect(forward) <= defect(backward) else (backward, forward)
                self._maps[replace] = self._maps[keep].T.copy()
        elif pairs:
            import torch
            self._check_device_sizes(M)
            d = self._eng.fmn_orth_defect(self._maps, M)
            e1 = torch.as_tensor([self.edge2ind[p[0]] for p in pairs], device=d.device)
            e2 = torch.as_tensor([self.edge2ind[p[1]] for p in pairs], device=d.device)
            keep1 = (d[e1] <= d[e2])[:, None, None]
            m1, m2 = self._maps[e1], self._maps[e2]
            new1 = torch.where(keep1, m1, m2.transpose(1, 2))
            new2 = torch.where(keep1, m1.transpose(1, 2), m2)
            maps = self._maps.clone()
            maps[e1] = new1
            maps[e2] = new2
            self._maps = maps
        self._reset_map_attributes()

    # ------------------------------------------------------------------ consistent latent basis
    def _check_device_sizes(self, M):
        if self.n_meshes * M > MAX_DIM:
            raise ValueError(f"FMN (device route): n M = {self.n_meshes} x {M} = {self.n_meshes * M} is above the limit of {MAX_DIM}; device=False has none")
        if M > MAX_M:
            raise ValueError(f"FMN (device route): M = {M} is above the limit of {MAX_M}; device=False has none")

    def compute_W(self, M=None, verbose=False):
        """The quadratic form of the consistent latent basis (:272-291): a SciPy CSR matrix on the host route, a DeviceMatrix on the
        device route.  ValueError when the last meshes have no edge: the form's size follows 1 + max(edges), and the reference then
        fails in compute_CLB's reshape."""
        if self._maps is None:
            raise ValueError("FMN.compute_W: the network has no maps yet (set_maps)")
        if self.weights is None:
            self.set_weights(verbose=verbose)
        if M is not None:
            self.M = M
        n_form = 1 + int(np.max(self.edges))
        if n_form != self.n_meshes:
            raise ValueError(f"the edges reach {n_form} meshes but the network has {self.n_meshes}: the quadratic form has "
                             f"1 + max(edges) blocks, and the consistent latent basis cannot be reshaped to (n_meshes, M, M)")
        if self._eng is None:
            self.W = CLB_quad_form(self._maps, self.weights, M=self.M)
        else:
            import torch
            self._check_device_sizes(self.M)
            dev = self._eng.device
            edges = np.asarray(self.edges, dtype=np.int32).reshape(-1, 2)
            w = torch.as_tensor(self._edge_weight_vector()).to(dev)
            self.W = DeviceMatrix(self._eng.fmn_quad_form(self.n_meshes, self.M, self._maps, edges, w))

    def compute_CLB(self, equals_id=False, verbose=False):
        """Consistent latent basis (:293-334): the M smallest eigenpairs of W; CLB = vectors.reshape(n, M, M).  equals_id=False: the
        vectors are scaled so that sum_i Y_i^T Y_i = n I (what eigsh's M = I / n gives), True: unit norm.  Signs: see the module."""
        if self.W is None:
            self.compute_W(verbose=verbose)
        M, n = self.M, self.n_meshes
        scale = 1.0 if equals_id else np.sqrt(n)
        if self._eng is None:
            lam, V = scipy.linalg.eigh(self.W.toarray(), subset_by_index=[0, M - 1])
            self._clb_eigenvalues = lam
            self._CLB = (scale * _fix_signs(V)).reshape((n, M, M))
        else:
            lam, V, resid, _ = self._eng.eigh_smallest(self.W.device_tensor(), M)
            self._clb_eigenvalues = lam
            self.clb_resid = resid
            self._CLB = (scale * V).reshape(n, M, M)

    def _device_meshes(self):
        """the meshes' eigenvectors (n, Nmax, K), eigenvalues (n, K) and lumped masses (n, Nmax) on the device, padded with zeros"""
        if "meshes" not in self._dev_cache:
            import torch
            dev = self._eng.device
            nv = [mesh.eigenvectors.shape[0] for mesh in self.meshlist]
            K = min(mesh.eigenvectors.shape[1] for mesh in self.meshlist)
            Phi = np.zeros((self.n_meshes, max(nv), K))
            mass = np.zeros((self.n_meshes, max(nv)))
            lam = np.zeros((self.n_meshes, K))
            for i, mesh in enumerate(self.meshlist):
                Phi[i, :nv[i]] = mesh.eigenvectors[:, :K]
                mass[i, :nv[i]] = np.asarray(mesh.A.diagonal())
                lam[i] = mesh.eigenvalues[:K]
            self._dev_cache["meshes"] = (torch.as_tensor(Phi).to(dev), torch.as_tensor(lam).to(dev), torch.as_tensor(mass).to(dev), nv, K)
        return self._dev_cache["meshes"]

    def _device_samples(self):
        """(sub (n, S) int64, Phi[sub] (n, S, K)) on the device"""
        if "sub" not in self._dev_cache:
            import torch
            Phi, _, _, nv, _ = self._device_meshes()
            sub = np.asarray(self.subsample, dtype=np.int64)
            if sub.ndim != 2 or sub.shape[0] != self.n_meshes or sub.min() < 0 or np.any(sub.max(axis=1) >= np.asarray(nv)):
                raise ValueError("FMN: subsample must be (n_meshes, size) vertex indices inside their meshes")
            sub_d = torch.as_tensor(sub).to(Phi.device)
            self._dev_cache["sub"] = (sub_d, torch.gather(Phi, 1, sub_d[:, :, None].expand(-1, -1, Phi.shape[2])).contiguous())
        return self._dev_cache["sub"]

    def compute_CCLB(self, m, verbose=True):
        """Canonical consistent latent basis (:336-369): E = sum_i Y_i^T diag(lambda_i[:M]) Y_i with Y_i = CLB[i][:, :m]; (theta, Q) =
        eigenpairs of E / n in ascending order from a symmetric solver; CCLB[i] = Y_i Q, cclb_eigenvalues = theta."""
        if self._CLB is None:
            self.compute_CLB(verbose=verbose)
        n, M = self.n_meshes, self.M
        if self._eng is None:
            stacked = self._CLB[:, :, :m].reshape(n * M, m)                  # the n blocks Y_i on top of each other
            lam = np.concatenate([mesh.eigenvalues[:M] for mesh in self.meshlist])
            energy = stacked.T @ (lam[:, None] * stacked) / n
            theta, Q = scipy.linalg.eigh(0.5 * (energy + energy.T))
            self._cclb_eigenvalues = theta
            self._CCLB = (stacked @ _fix_signs(Q)).reshape(n, M, m)
        else:
            _, lam, _, _, K = self._device_meshes()
            if M > K:
                raise ValueError(f"FMN: maps of size {M} need {M} eigenpairs per mesh, only {K} are there")
            self._CCLB, self._cclb_eigenvalues = self._eng.fmn_cclb(self._CLB, lam, m)
        return self

    def get_CSD(self, i):
        """(area, conformal) characteristic shape difference operators of mesh i in the latent space (:371-393): with Y = CCLB[i],
        Y^T Y and pinv(diag(cclb_eigenvalues)) Y^T diag(lambda_i[:M]) Y"""
        Y = self.CCLB[i]
        stiffness = self.meshlist[i].eigenvalues[:self.M, None] * Y
        inv_theta = np.linalg.pinv(np.diag(self.cclb_eigenvalues))
        return Y.T @ Y, (inv_theta @ Y.T) @ stiffness

    def get_LB(self, i, complete=True):
        """Latent basis of mesh i (:395-417): eigenvectors[:, :M] @ CCLB[i], on the sampled vertices only when complete=False and a
        subsample is set."""
        rows = slice(None) if (complete or self.subsample is None) else self.subsample[i]
        return self.meshlist[i].eigenvectors[rows, :self.M] @ self.CCLB[i]

    # ------------------------------------------------------------------ vertex maps and new functional maps
    def _edge_groups(self, complete):
        """the edges grouped by (rows of the search tree, query rows): one search call per group"""
        nv = [mesh.eigenvectors.shape[0] for mesh in self.meshlist]
        has_sub = self.subsample is not None
        size = None if not has_sub else int(np.asarray(self.subsample).shape[1])
        groups = {}
        for (i, j) in self.edges:
            nx = size if has_sub else nv[i]
            ny = size if (has_sub and not complete) else nv[j]
            groups.setdefault((nx, ny), []).append((i, j))
        return groups

    def compute_p2p(self, complete=True, n_jobs=1):
        """Vertex maps of all edges from the latent bases (:419-451): p2p[(i, j)][q] = the row of mesh i's search tree nearest to row q
        of mesh j's latent basis.  A quirk of the reference that is kept: the tree of edge (i, j) is ALWAYS built on
        get_LB(i, complete=False) -- the sampled rows whenever a subsample is set, also with complete=True -- while the queries are
        get_LB(j, complete=complete); with a subsample and complete=True the result therefore has one entry per vertex of mesh j, and
        each is an index into the SAMPLES of mesh i.  (`n_jobs` is accepted and ignored.)"""
        if self._eng is None:
            from scipy.spatial import cKDTree
            trees = {i: cKDTree(self.get_LB(i, complete=False), leafsize=40) for i in sorted({e[0] for e in self.edges})}
            queries = {j: self.get_LB(j, complete=complete) for j in sorted({e[1] for e in self.edges})}
            self._p2p = {(i, j): trees[i].query(queries[j])[1].ravel() for (i, j) in self.edges}
            return
        import torch
        Phi, _, _, nv, _ = self._device_meshes()
        M = self.M
        has_sub = self.subsample is not None
        LB_full = LB_sub = None
        if has_sub:
            LB_sub = torch.bmm(self._device_samples()[1][:, :, :M], self._CCLB)
        if (not has_sub) or complete:
            LB_full = torch.bmm(Phi[:, :, :M], self._CCLB)
        out = []
        for (nx, ny), edges in self._edge_groups(complete).items():
            ii = torch.as_tensor([e[0] for e in edges], device=Phi.device)
            jj = torch.as_tensor([e[1] for e in edges], device=Phi.device)
            X = (LB_sub if has_sub else LB_full).index_select(0, ii)[:, :nx]
            Y = (LB_sub if (has_sub and not complete) else LB_full).index_select(0, jj)[:, :ny]
            out.append((edges, self._eng.knn_query(X, Y)))
        self._p2p = out

    def compute_maps(self, M, complete=True):
        """Functional maps of size M from the vertex maps (:453-474): mesh_p2p_to_FM(p2p[(i, j)], mesh_i, mesh_j, dims=M,
        subsample=(sub_i, sub_j) when complete=False and a subsample is set, else None).  Resets what depends on the maps."""
        self.M = M
        use_sub = (not complete) and self.subsample is not None
        if self._eng is None:
            p2p = self._p2p
            for (i, j) in self.edges:
                m1, m2 = self.meshlist[i], self.meshlist[j]
                if use_sub:
                    pulled = m1.eigenvectors[self.subsample[i], :M][p2p[(i, j)], :]
                    FM = scipy.linalg.lstsq(m2.eigenvectors[self.subsample[j], :M], pulled)[0]
                else:
                    FM = m2.eigenvectors[:, :M].T @ (m2.A @ m1.eigenvectors[:, :M][p2p[(i, j)], :])
                self._maps[(i, j)] = FM
        else:
            import torch
            self._check_device_sizes(M)
            Phi, _, mass, nv, K = self._device_meshes()
            if M > K:
                raise ValueError(f"FMN: maps of size {M} need {M} eigenpairs per mesh, only {K} are there")
            new = torch.empty((len(self.edges), M, M), dtype=torch.float64, device=Phi.device)
            for edges, p in self._p2p:
                ii = torch.as_tensor([e[0] for e in edges], device=Phi.device)
                jj = torch.as_tensor([e[1] for e in edges], device=Phi.device)
                if use_sub:
                    Ps = self._device_samples()[1]
                    if p.shape[1] != Ps.shape[1]:
                        raise ValueError("FMN.compute_maps(complete=False): the vertex maps were computed with complete=True")
                    C = self._eng.p2p_to_fm_lstsq(p, Ps.index_select(0, ii), Ps.index_select(0, jj), M, M)
                else:
                    ni, nj = nv[edges[0][0]], nv[edges[0][1]]
                    if p.shape[1] != nj:
                        raise ValueError("FMN.compute_maps(complete=True): the vertex maps were computed with complete=False")
                    C = self._eng.p2p_to_fm(p, Phi.index_select(0, ii)[:, :ni], Phi.index_select(0, jj)[:, :nj], mass.index_select(0, jj)[:, :nj], M, M)
                new[torch.as_tensor([self.edge2ind[e] for e in edges], device=Phi.device)] = C
            self._maps = new
        self._reset_map_attributes()

    # ------------------------------------------------------------------ cycles and ICSM weights
    def extract_3_cycles(self):
        """All three-cycles (i, j, k) of the graph -- edges (i, j), (j, k), (k, i) -- with i > j > k or i < j < k, in the reference's order
        (:476-493): by i, the descending triples before the ascending ones"""
        n = self.n_meshes

        def closed(t):
            return all(e in self.edge2ind for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])))
        self.cycles = []
        for i in range(n):
            descending = [(i, j, k) for j in range(i) for k in range(j)]
            ascending = [(i, j, k) for j in range(i + 1, n) for k in range(j + 1, n)]
            self.cycles.extend(t for t in descending + ascending if closed(t))

    def _cycle_edge_indices(self):
        return np.asarray([[self.edge2ind[(i, j)], self.edge2ind[(j, k)], self.edge2ind[(k, i)]] for (i, j, k) in self.cycles],
                          dtype=np.int32).reshape(-1, 3)

    def compute_Amat(self):
        """A[c, e] = 1 when edge e (in the order of `edges`) lies in cycle c (:495-508)"""
        self.A = np.zeros((len(self.cycles), len(self.edges)))
        ce = self._cycle_edge_indices()
        for c in range(ce.shape[0]):
            self.A[c, ce[c]] = 1
        self.A_sub = np.where(self.A.sum(0) > 0)[0]

    def compute_3cycle_weights(self, M=None):
        """Cycle costs (get_cycle_weight) and the edge costs of the linear program, 1 / (sum of the costs of the cycles through the edge),
        0 for an edge in no cycle (:510-529)"""
        M = self.M if M is None else M
        if self._eng is None:
            self.cycle_weight = np.asarray([self.get_cycle_weight(cycle, M=M) for cycle in self.cycles], dtype=np.float64)
        else:
            self._check_device_sizes(M)
            self.cycle_weight = self._eng.fmn_cycle_costs(self._maps, M, self._cycle_edge_indices()).cpu().numpy()
        through = self.A.T @ self.cycle_weight
        self.edge_weights = np.zeros(len(self.edges))
        self.edge_weights[self.A_sub] = 1.0 / through[self.A_sub]

    def optimize_icsm(self, verbose=False):
        """The linear program of the ICSM weights (:531-557): min edge_weights^T x subject to A x >= cycle_weight, x >= 0; edges outside
        every cycle get 0.  Solved on the HOST in both routes (scipy.optimize.linprog, method='highs-ds', E variables): on the device
        route the cycle costs are read back for it, one synchronisation per iteration."""
        from scipy.optimize import linprog
        self.compute_3cycle_weights(M=self.M)
        lp = linprog(c=self.edge_weights, A_ub=-self.A, b_ub=-self.cycle_weight, bounds=(0, None), method='highs-ds')
        self.icsm_objective = float(lp.fun)
        in_cycle = np.zeros(len(self.edges), dtype=bool)
        in_cycle[self.A_sub] = True
        return np.where(in_cycle, lp.x, 0.0)

    def get_cycle_weight(self, cycle, M=None):
        """Cost of the cycle (i, j, k): the largest of the three |C C C - I|_F going once around from i, j and k (:559-594)"""
        M = self.M if M is None else M
        i, j, k = cycle
        around = ((i, j), (j, k), (k, i))
        if self._eng is not None:
            ce = np.asarray([[self.edge2ind[e] for e in around]], dtype=np.int32)
            return float(self._eng.fmn_cycle_costs(self._maps, M, ce)[0])
        C = [self._maps[e][:M, :M] for e in around]
        eye = np.eye(M)
        return max(np.linalg.norm(C[r] @ C[(r + 1) % 3] @ C[(r + 2) % 3] - eye) for r in range(3))

    # ------------------------------------------------------------------ Consistent ZoomOut
    def zoomout_iteration(self, cclb_size, M_init, M_final, isometric=True, weight_type='icsm', n_jobs=1, equals_id=False, complete=False):
        """One iteration of Consistent ZoomOut (:596-632): isometries (at size M_init), weights, W, CLB, CCLB of size cclb_size, vertex
        maps, maps of size M_final.  ICSM weights are recomputed every time; any other weight_type only sets adjacency weights when the
        network has no weights yet."""
        if isometric:
            self.set_isometries(M=M_init)
        if weight_type == 'icsm' or self.weights is None:
            self.set_weights(weight_type='icsm' if weight_type == 'icsm' else 'adjacency')
        self.compute_W(M=M_init)
        self.compute_CLB(equals_id=equals_id)
        self.compute_CCLB(cclb_size)
        self.compute_p2p(complete=complete, n_jobs=n_jobs)
        self.compute_maps(M_final, complete=complete)

    def zoomout_refine(self, nit=10, step=1, subsample=1000, isometric=True, weight_type='icsm', M_init=None, cclb_ratio=.9, n_jobs=1,
                       equals_id=False, verbose=False):
        """Consistent ZoomOut (:634-687).  Kept from the reference: nit - 1 iterations are performed (range(nit - 1); its "last
        iteration" branch is dead), `complete = not use_sub` in every one of them, m_cclb = int(cclb_ratio * M), and `isometric` is
        not passed on (every iteration runs set_isometries).  subsample: a size (farthest point samples are drawn), an (n, size) array
        of vertex indices, or 0 / None for all vertices."""
        is_size = np.issubdtype(type(subsample), np.integer)
        use_sub = subsample is not None and not (is_size and subsample == 0)
        if not use_sub:
            self.set_subsample(None)
        elif is_size:
            self.compute_subsample(size=subsample, verbose=verbose)
        else:
            self.set_subsample(subsample)
        if M_init is not None:
            self.M = M_init
        for it in range(nit - 1):
            M_now = self.M
            if verbose:
                print(f"FMN: iteration {it + 1} of {nit - 1}, maps {M_now} -> {M_now + step}")
            self.zoomout_iteration(int(cclb_ratio * M_now), M_now, M_now + step, weight_type=weight_type, equals_id=equals_id, n_jobs=n_jobs,
                                   complete=not use_sub)

def CLB_quad_form(maps, weights, M=None):
    """The quadratic form of a functional map network for the consistent latent basis (:690-738), host route: per edge (i, j) of the
    dict `maps` (in its own key order) with weight w = weights[i, j] and FM = maps[(i, j)][:M, :M],
        block (i, i) += w FM^T FM,   block (j, j) += w I,   block (i, j) -= w FM^T,   block (j, i) -= w FM.
    The number of blocks is 1 + max(edges).  Returns a scipy.sparse.csr_matrix (N M, N M).  (The device form is
    MatchEngine.fmn_quad_form / FMN.compute_W.)"""
    edges = list(maps.keys())
    N = 1 + int(np.max(edges))
    if M is None:
        M = maps[edges[0]].shape[0]
    W = np.zeros((N, M, N, M))
    eye = np.eye(M)
    for (i, j) in edges:
        FM = _to_numpy(maps[(i, j)])[:M, :M]
        w = weights[i, j]
        W[i, :, i, :] += w * (FM.T @ FM)
        W[j, :, j, :] += w * eye
        W[i, :, j, :] -= w * FM.T
        W[j, :, i, :] -= w * FM
    return sparse.csr_matrix(W.reshape(N * M, N * M))

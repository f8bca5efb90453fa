"""
Map quality measures that consume a geodesic distance matrix (reference: densematcher/pyFM/eval/evaluate.py:4-100, and
densematcher/diffusion_net/geometry.py:754-781 for geodesic_label_errors).  D1_geod / D2_geod come from TriMesh.get_geodesic (the
heat method on the device, or Dijkstra).

Two routes, chosen by what the caller passes:
* NumPy matrices: host NumPy, the reference's arithmetic and its bits.
* a torch tensor on the GPU (the padded batches that MatchEngine.heat_geodesic / graph_geodesic return, or one matrix): the
  measures are gathered and summed on the device (MatchEngine.map_accuracy / map_continuity / map_coverage, one dm_map_metrics
  launch per call) and no N x N matrix crosses to the host.  Per-element results are the host route's bits; means and coverages
  agree with it to n 2^-52 relative (another summation order of the same terms).

`*_many` evaluate lists of problems at once, `evaluate_pairs` everything for a set of mesh pairs, computing the geodesic matrices
of the distinct meshes once on the device.
"""
import numpy as np

__all__ = ["accuracy", "continuity", "coverage", "accuracy_many", "continuity_many", "coverage_many", "geodesic_label_errors",
           "evaluate_pairs"]


def _on_device(*arrays):
    """is one of the arrays a torch tensor on a GPU?  (torch is not imported for NumPy callers)"""
    return any(type(a).__module__.split(".")[0] == "torch" and getattr(a, "is_cuda", False) for a in arrays)


def _engine():
    from ...engine import default_engine
    return default_engine()


def _host(a):
    return a.cpu().numpy() if type(a).__module__.split(".")[0] == "torch" else a


def accuracy(p2p, gt_p2p, D1_geod, return_all=False, sqrt_area=None):
    """mean geodesic distance on the source shape between matched and ground-truth vertices (evaluate.py:4-35)"""
    if _on_device(D1_geod):
        out = _engine().map_accuracy(D1_geod, [p2p], [gt_p2p], scale=sqrt_area, return_all=return_all)
        return (out[0][0], out[1][0]) if return_all else out[0]
    dists = D1_geod[(p2p, gt_p2p)]
    if sqrt_area is not None:
        dists /= sqrt_area
    if return_all:
        return dists.mean(), dists
    return dists.mean()


def continuity(p2p, D1_geod, D2_geod, edges):
    """mean ratio of mapped edge length (source geodesics) to edge length (target geodesics) (evaluate.py:38-70)"""
    if _on_device(D1_geod, D2_geod):
        return _engine().map_continuity(D1_geod, D2_geod, [p2p], [edges])[0]
    source_len = D2_geod[(edges[:, 0], edges[:, 1])]
    target_len = D1_geod[(p2p[edges[:, 0]], p2p[edges[:, 1]])]
    return np.mean(target_len / source_len)


def coverage(p2p, A):
    """area fraction of the source shape that the map reaches (evaluate.py:73-100); A: (n1, n1) area matrix or (n1,) vertex
    areas (the reference reads only the matrix form: its 1-D branch names an undefined variable)"""
    if _on_device(A):
        return _engine().map_coverage(A.sum(1) if A.dim() == 2 else A, [p2p])[0]
    vert_area = np.asarray(A.sum(1)).flatten() if len(A.shape) == 2 else np.asarray(A)
    return vert_area[np.unique(p2p)].sum() / vert_area.sum()


def _meshes_of(P, mesh):
    return np.zeros(P, np.int64) if mesh is None else np.broadcast_to(np.asarray(mesh, np.int64), (P,))


def _host_matrix(D, b, n_verts):
    """matrix b of a list of matrices, of a (B, N, N) batch (cut to its n_verts[b] vertices) or of one (N, N) matrix"""
    if isinstance(D, (list, tuple)):
        return np.asarray(_host(D[b]))
    D = _host(D)
    if D.ndim == 2:
        if b != 0:
            raise ValueError("mesh indices must lie in [0, 1)")
        D = D[None]
    if not 0 <= b < D.shape[0]:
        raise ValueError(f"mesh indices must lie in [0, {D.shape[0]})")
    n = D.shape[1] if n_verts is None else int(np.broadcast_to(np.asarray(n_verts), (D.shape[0],))[b])
    return D[b, :n, :n]


def accuracy_many(p2p_list, gt_list, D1_geod, mesh=None, return_all=False, sqrt_area=None, n_verts=None):
    """accuracy for P maps: problem p on matrix mesh[p] (default 0) of D1_geod -- one (N, N) matrix, a (B, N, N) batch padded to
    the largest mesh (n_verts (B,): the vertex counts), or a list of matrices.  sqrt_area: None, one number, or one per problem.
    A GPU tensor: ONE device call for all of them; NumPy matrices (or a list): the loop of `accuracy`, its bits.
    Returns the means (P,) float64; with return_all=True also the list of the per-vertex distances."""
    P = len(p2p_list)
    if len(gt_list) != P:
        raise ValueError("accuracy_many: as many ground-truth lists as maps")
    if _on_device(D1_geod):
        return _engine().map_accuracy(D1_geod, p2p_list, gt_list, mesh=mesh, scale=sqrt_area, return_all=return_all, n_verts=n_verts)
    mesh = _meshes_of(P, mesh)
    sc = None if sqrt_area is None else np.broadcast_to(np.asarray(sqrt_area, np.float64), (P,))
    out = [accuracy(np.asarray(p2p_list[p]), np.asarray(gt_list[p]), _host_matrix(D1_geod, int(mesh[p]), n_verts), return_all=True,
                    sqrt_area=None if sc is None else sc[p]) for p in range(P)]
    means = np.asarray([o[0] for o in out], np.float64).reshape(P)
    return (means, [o[1] for o in out]) if return_all else means


def continuity_many(p2p_list, D1_geod, D2_geod, edges_list, mesh1=None, mesh2=None, n_verts1=None, n_verts2=None):
    """continuity for P maps: problem p maps the target mesh mesh2[p] of D2_geod into the source mesh mesh1[p] of D1_geod
    (D2_geod=None: both are meshes of D1_geod); matrices as in accuracy_many.  Returns (P,) float64."""
    P = len(p2p_list)
    if len(edges_list) != P:
        raise ValueError("continuity_many: as many edge lists as maps")
    if _on_device(D1_geod, D2_geod):
        return _engine().map_continuity(D1_geod, D2_geod, p2p_list, edges_list, mesh1=mesh1, mesh2=mesh2, n_verts1=n_verts1, n_verts2=n_verts2)
    mesh1, mesh2 = _meshes_of(P, mesh1), _meshes_of(P, mesh2)
    if D2_geod is None:
        D2_geod, n_verts2 = D1_geod, (n_verts1 if n_verts2 is None else n_verts2)
    return np.asarray([continuity(np.asarray(p2p_list[p]), _host_matrix(D1_geod, int(mesh1[p]), n_verts1),
                                  _host_matrix(D2_geod, int(mesh2[p]), n_verts2), np.asarray(edges_list[p]).reshape(-1, 2))
                       for p in range(P)], np.float64).reshape(P)


def coverage_many(p2p_list, A, mesh=None, n_verts=None):
    """coverage for P maps: problem p on the vertex areas A[mesh[p]]; A: (N,) or (B, N) vertex areas (n_verts (B,): the vertex counts
    of a padded batch), or a list of (n,) vectors / (n, n) area matrices.  Returns (P,) float64."""
    P = len(p2p_list)
    if _on_device(A):
        return _engine().map_coverage(A, p2p_list, mesh=mesh, n_verts=n_verts)
    mesh = _meshes_of(P, mesh)

    def areas(b):
        if isinstance(A, (list, tuple)):
            return A[b] if len(A[b].shape) == 2 else np.asarray(_host(A[b]))
        a = np.asarray(A)
        a = a[None] if a.ndim == 1 else a
        if not 0 <= b < a.shape[0]:
            raise ValueError(f"mesh indices must lie in [0, {a.shape[0]})")
        n = a.shape[1] if n_verts is None else int(np.broadcast_to(np.asarray(n_verts), (a.shape[0],))[b])
        return a[b, :n]
    return np.asarray([coverage(np.asarray(p2p_list[p], dtype=np.int64), areas(int(mesh[p]))) for p in range(P)], np.float64).reshape(P)


def geodesic_label_errors(D, pred, gt, normalization="diameter", area=None):
    """(n,) geodesic distances between predicted and ground-truth labels on a given all-pairs matrix, normalised by the geodesic
    diameter np.max(D) or by the square root of the total surface area `area` (diffusion_net/geometry.py:770-781; the reference
    computes D itself, with libigl).  D on the GPU: gathered and divided on the device, the same bits."""
    if normalization not in ("diameter", "area"):
        raise ValueError('unrecognized normalization')
    if normalization == "area" and area is None:
        raise ValueError("geodesic_label_errors: normalization='area' needs the total surface area")
    if _on_device(D):
        scale = "diameter" if normalization == "diameter" else float(np.sqrt(area))
        return _engine().map_accuracy(D, [pred], [gt], scale=scale, return_all=True)[1][0]
    D = np.asarray(D)
    result_dists = D[np.asarray(pred), np.asarray(gt)]
    return result_dists / (np.max(D) if normalization == "diameter" else np.sqrt(area))


def _maps_of(entry):
    """the named maps of one pair: a dict stays, one map is wrapped"""
    return (dict(entry), True) if isinstance(entry, dict) else ({None: entry}, False)


def evaluate_pairs(meshes, pairs, maps, gt_maps, dijkstra=False, robust=False, sym=False, normalization=None, continuity=True,
                   coverage=True):
    """Geodesic accuracy, continuity and coverage of the maps of a set of mesh pairs.
    meshes: a list of TriMesh; pairs: a list of (i_source, i_target) indices into it; maps[q]: the target -> source vertex map of
    pair q ((n_target,) source vertex of every target vertex, what accuracy takes as p2p), or a dict name -> map (the vertex maps of
    a compute_surface_map result under their names); gt_maps[q]: the ground-truth map of pair q.
    The geodesic matrices (get_geodesic's, chosen by dijkstra / robust / sym) of the DISTINCT meshes that the pairs name are
    computed once, on the device for dijkstra=True or robust=False, and read there: accuracy on the source matrix (normalization:
    None, "diameter" = np.max of the source matrix, "area" = sqrt of the source mesh's area), continuity of the target's edges,
    coverage of the source's vertex areas -- at most three device calls, no N x N matrix crosses to the host.  robust=True (the
    potpourri3d wheel's host matrices) and meshes outside the device's shortest-path route use get_geodesic_many and the host
    functions.  Returns one dict {"accuracy", "continuity", "coverage"} per pair (measures that were not asked for are left out),
    or a dict name -> such a dict where maps[q] is a dict."""
    from ..mesh import geometry
    from ..mesh.trimesh import TriMesh
    if normalization not in (None, "diameter", "area"):
        raise ValueError('unrecognized normalization')
    pairs = [(int(i), int(j)) for i, j in pairs]
    if len(maps) != len(pairs) or len(gt_maps) != len(pairs):
        raise ValueError("evaluate_pairs: one entry of maps and of gt_maps per pair")
    for i, j in pairs:
        if not (0 <= i < len(meshes) and 0 <= j < len(meshes)):
            raise IndexError(f"evaluate_pairs: pair ({i}, {j}) names a mesh outside the list of {len(meshes)}")
    # the distinct meshes in use: one slot per mesh OBJECT
    slot_of, used = {}, []
    for i in sorted({i for pr in pairs for i in pr}):
        if id(meshes[i]) not in slot_of:
            slot_of[id(meshes[i])] = len(used)
            used.append(meshes[i])
    slot = {i: slot_of[id(meshes[i])] for pr in pairs for i in pr}
    named = [_maps_of(m) for m in maps]
    probs = [(q, name, np.asarray(_host(m))) for q, (d, _) in enumerate(named) for name, m in d.items()]
    gts = [np.asarray(_host(g)) for g in gt_maps]
    src = np.asarray([slot[pairs[q][0]] for q, _, _ in probs], np.int64)
    tgt = np.asarray([slot[pairs[q][1]] for q, _, _ in probs], np.int64)
    p2ps = [m for _, _, m in probs]
    nv = [mesh.n_vertices for mesh in used]
    D = None
    if used and dijkstra:
        D = geometry._dijkstra_many_device([geometry.edge_graph(mesh.vertlist, mesh.facelist) for mesh in used])
    elif used and not robust:
        import torch
        if torch.cuda.is_available():
            D = TriMesh._heat_geodesic_many_device(used, sym)
    scale = None
    if D is None:
        D = TriMesh.get_geodesic_many(used, dijkstra=dijkstra, robust=robust, sym=sym) if used else []
        nv_arg = None
        if normalization == "diameter":
            scale = np.asarray([np.max(D[s]) for s in src])
    else:
        nv_arg = nv
        if normalization == "diameter":
            scale = _engine().geodesic_diameter(D, nv)[src]
    if normalization == "area":
        scale = np.asarray([np.sqrt(used[s].area) for s in src])
    acc = accuracy_many(p2ps, [gts[q] for q, _, _ in probs], D, mesh=src, sqrt_area=scale, n_verts=nv_arg)
    cont = cov = None
    if continuity:
        edges = [mesh.edges for mesh in used]                # (one object per mesh: uploaded once)
        cont = continuity_many(p2ps, D, None, [edges[t] for t in tgt], mesh1=src, mesh2=tgt, n_verts1=nv_arg)
    if coverage:
        areas = [np.asarray(mesh.vertex_areas, np.float64) for mesh in used]
        if nv_arg is None:
            cov = coverage_many(p2ps, areas, mesh=src)
        else:
            import torch
            pad = np.zeros((len(used), max(nv)))
            for b, a in enumerate(areas):
                pad[b, :len(a)] = a
            cov = coverage_many(p2ps, torch.as_tensor(pad).to(D.device), mesh=src, n_verts=nv)
    out = [dict() if is_dict else None for _, is_dict in named]
    for k, (q, name, _) in enumerate(probs):
        res = {"accuracy": acc[k]}
        if cont is not None:
            res["continuity"] = cont[k]
        if cov is not None:
            res["coverage"] = cov[k]
        if named[q][1]:
            out[q][name] = res
        else:
            out[q] = res
    return out

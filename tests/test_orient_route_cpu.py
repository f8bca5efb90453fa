"""CPU: the arguments that select the orientation operators' route are checked before anything touches the GPU."""
import numpy as np
import pytest
import scipy.sparse as sp


def _model(fx):
    from densematcher_amd.pyFM.functional import FunctionalMapping
    from densematcher_amd.pyFM.mesh import TriMesh
    meshes = []
    for which in (1, 2):
        m = TriMesh(fx[f"verts{which}"], fx[f"faces{which}"])
        m.A = sp.diags(fx[f"a{which}"].astype(np.float64)).tocsr()
        m.W = sp.identity(m.n_vertices).tocsr()
        m.eigenvalues = fx[f"lam{which}"][:10].copy()
        m.eigenvectors = fx[f"Phi{which}"][:, :10].astype(np.float64)
        meshes.append(m)
    model = FunctionalMapping(meshes[0], meshes[1], partial=False, optimizer="L-BFGS-B")
    model.preprocess(n_ev=(10, 10), n_descr=2, descr1=fx["F1"][:, :2], descr2=fx["F2"][:, :2], subsample_step=1)
    return model


def test_route_arguments(fx_cfg1):
    model = _model(fx_cfg1)
    with pytest.raises(NotImplementedError):
        model.compute_orientation_op(route="device", normalize=True)
    with pytest.raises(ValueError, match="route"):
        model.compute_orientation_op(route="x")
    with pytest.raises(ValueError, match="orient_route"):
        model.fit(w_descr=1e4, w_lap=1e3, w_dcomm=0, w_orient=1, orient_route="x")
    # the host route is the default and what it was
    ops = model.compute_orientation_op()
    same = model.compute_orientation_op(route="host")
    assert all(np.array_equal(a, c) and np.array_equal(b, d) for (a, b), (c, d) in zip(ops, same))


def test_batched_call_checks_orient_route():
    from densematcher_amd.functional_map import compute_surface_map_batch
    with pytest.raises(ValueError, match="orient_route"):
        compute_surface_map_batch([], [], [], [], fit_params=dict(w_orient=1, orient_route="x"))


def test_row_scale_of_a_lumped_mass_is_one(fx_cfg1):
    """A diagonal: the row sums are the diagonal, so compute_orientation_op's two area forms coincide and one device call serves both;
    a mass matrix that is not diagonal is not a row scale and stays on the host route"""
    from densematcher_amd.pyFM.functional import _orient_row_scale
    model = _model(fx_cfg1)
    assert _orient_row_scale(model.mesh1) is None
    a = model.mesh1.A.tolil()
    a[0, 1] = a[1, 0] = 1e-3
    model.mesh1.A = a.tocsr()
    with pytest.raises(NotImplementedError):
        _orient_row_scale(model.mesh1)

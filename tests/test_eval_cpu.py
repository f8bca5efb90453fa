"""CPU: the host route of pyFM.eval against the numbers the reference's functions returned (tests/golden/fx_eval.npz, written by
tools/make_golden_eval.py), and the list forms (accuracy_many, continuity_many, coverage_many, geodesic_label_errors) on NumPy
inputs against the loop of the host functions and the same fixture.  Host arithmetic is the reference's: everything is compared
bit for bit (assert_array_equal treats NaN as equal to NaN)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sparse

from conftest import load_golden
from densematcher_amd.pyFM import eval as ev


@pytest.fixture(scope="module")
def fx():
    e, geod, groups = load_golden("fx_eval.npz"), load_golden("fx_geod.npz"), load_golden("fx_groups.npz")
    e["small_D"], e["small_edges"], e["b_D"] = geod["small_D"], geod["small_edges"], groups["b_D"]
    for v in e.values():
        v.setflags(write=False)
    return e


@pytest.fixture(autouse=True)
def quiet():
    """x / 0 and the mean of nothing are NumPy's own warnings: part of the behaviour, not of what is asserted"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def test_host_functions_reproduce_the_reference(fx):
    D = fx["small_D"]
    for tag in ("", "_long"):
        p2p, gt = fx["a_p2p" + tag], fx["a_gt" + tag]
        acc, dists = ev.accuracy(p2p, gt, D, return_all=True)
        np.testing.assert_array_equal(acc, fx["a_acc" + tag])
        np.testing.assert_array_equal(dists, fx["a_dists" + tag])
        np.testing.assert_array_equal(ev.accuracy(p2p, gt, D), fx["a_acc" + tag])
        acc, dists = ev.accuracy(p2p, gt, D, return_all=True, sqrt_area=float(fx["a_sqrt_area"]))
        np.testing.assert_array_equal(acc, fx["a_acc" + tag + "_scaled"])
        np.testing.assert_array_equal(dists, fx["a_dists" + tag + "_scaled"])
    np.testing.assert_array_equal(ev.continuity(fx["a_p2p"], D, D, fx["small_edges"]), fx["a_cont"])
    np.testing.assert_array_equal(ev.continuity(fx["a_p2p"], D, D, fx["a_edges_pos"]), fx["a_cont_pos"])
    assert np.isposinf(fx["a_cont"]) and np.isfinite(fx["a_cont_pos"])
    A = sparse.diags(fx["a_area"]).tocsr()
    np.testing.assert_array_equal(ev.coverage(fx["a_p2p"], A), fx["a_cov"])
    np.testing.assert_array_equal(ev.coverage(fx["a_p2p_long"], A), fx["a_cov_long"])
    bD = fx["b_D"]
    np.testing.assert_array_equal(ev.continuity(fx["b_p2p"], bD, bD, fx["b_edges_inf"]), np.inf)
    assert np.isposinf(fx["b_cont_inf"]) and np.isnan(fx["b_cont_nan"])
    assert np.isnan(ev.continuity(fx["b_p2p"], bD, bD, fx["b_edges_nan"]))
    acc, dists = ev.accuracy(fx["b_acc_p2p"], fx["b_acc_gt"], bD, return_all=True)
    np.testing.assert_array_equal(acc, fx["b_acc"])
    np.testing.assert_array_equal(dists, fx["b_dists"])
    assert len(np.unique(dists)) <= 4                                             # (the elements tie)


def test_accuracy_many_on_numpy_is_the_host_loop(fx):
    D, bD = fx["small_D"], fx["b_D"]
    p2ps = [fx["a_p2p"], fx["a_p2p_long"], fx["b_acc_p2p"], fx["a_p2p"]]
    gts = [fx["a_gt"], fx["a_gt_long"], fx["b_acc_gt"], fx["a_gt"]]
    means, dists = ev.accuracy_many(p2ps, gts, [D, bD], mesh=[0, 0, 1, 0], return_all=True)
    assert means.shape == (4,) and means.dtype == np.float64
    np.testing.assert_array_equal(means, [fx["a_acc"], fx["a_acc_long"], fx["b_acc"], fx["a_acc"]])
    for got, name in zip(dists, ("a_dists", "a_dists_long", "b_dists", "a_dists")):
        np.testing.assert_array_equal(got, fx[name])
    np.testing.assert_array_equal(ev.accuracy_many(p2ps[:2], gts[:2], D, sqrt_area=float(fx["a_sqrt_area"])),
                                  [fx["a_acc_scaled"], fx["a_acc_long_scaled"]])
    per = ev.accuracy_many(p2ps[:2], gts[:2], D, sqrt_area=[float(fx["a_sqrt_area"]), 1.0], return_all=True)
    np.testing.assert_array_equal(per[0], [fx["a_acc_scaled"], fx["a_acc_long"]])
    np.testing.assert_array_equal(per[1][0], fx["a_dists_scaled"])
    # a padded batch: the matrix of a mesh is its leading n_verts block, negative indices count from its own end
    pad = np.full((2, 160, 160), 1e300)
    pad[0] = D
    pad[1, :96, :96] = bD
    got = ev.accuracy_many([fx["b_acc_p2p"] - 96, fx["a_p2p"]], [fx["b_acc_gt"], fx["a_gt"]], pad, mesh=[1, 0], n_verts=[160, 96])
    np.testing.assert_array_equal(got, [fx["b_acc"], fx["a_acc"]])
    assert ev.accuracy_many([], [], D).shape == (0,)
    assert np.isnan(ev.accuracy_many([np.zeros(0, np.int64)], [np.zeros(0, np.int64)], D)[0])


def test_continuity_many_and_coverage_many_on_numpy(fx):
    D, bD = fx["small_D"], fx["b_D"]
    got = ev.continuity_many([fx["a_p2p"], fx["b_p2p"], fx["b_p2p"], fx["a_p2p"]], [D, bD], None,
                             [fx["a_edges_pos"], fx["b_edges_inf"], fx["b_edges_nan"], fx["small_edges"]], mesh1=[0, 1, 1, 0], mesh2=[0, 1, 1, 0])
    assert got.shape == (4,) and got.dtype == np.float64
    np.testing.assert_array_equal(got, [fx["a_cont_pos"], np.inf, np.nan, np.inf])
    # two tensors: the target side in one of its own
    np.testing.assert_array_equal(ev.continuity_many([fx["a_p2p"], fx["b_p2p"]], [D, bD], [bD, D], [fx["a_edges_pos"], fx["b_edges_inf"]], mesh1=[0, 1], mesh2=[1, 0]),
                                  [fx["a_cont_pos"], np.inf])
    area = fx["a_area"]
    got = ev.coverage_many([fx["a_p2p"], fx["a_p2p_long"], np.arange(160)[::-1], [7, 7, 7]], area)
    np.testing.assert_array_equal(got, [fx["a_cov"], fx["a_cov_long"], 1.0, area[7] / area.sum()])
    pad = np.full((2, 200), 1e300)
    pad[0, :160], pad[1, :3] = area, (1.0, 2.0, 5.0)
    np.testing.assert_array_equal(ev.coverage_many([fx["a_p2p"], [2, -3]], pad, mesh=[0, 1], n_verts=[160, 3]), [fx["a_cov"], 0.75])
    np.testing.assert_array_equal(ev.coverage_many([fx["a_p2p"]], [sparse.diags(area).tocsr()]), [fx["a_cov"]])


def test_geodesic_label_errors_restated(fx):
    """The reference (diffusion_net/geometry.py:754-781) takes its distances from libigl, which cannot be run here: the function is
    pinned to its arithmetic on a GIVEN matrix, restated in NumPy -- D[pred, gt] / D.max(), or / sqrt(total area)."""
    D, pred, gt = fx["small_D"], fx["a_p2p_long"], fx["a_gt_long"]
    np.testing.assert_array_equal(ev.geodesic_label_errors(D, pred, gt), D[pred, gt] / D.max())
    np.testing.assert_array_equal(ev.geodesic_label_errors(D, pred, gt, normalization="diameter"), fx["a_dists_long"] / np.max(D))
    np.testing.assert_array_equal(ev.geodesic_label_errors(D, pred, gt, normalization="area", area=3.0), D[pred, gt] / np.sqrt(3.0))
    with pytest.raises(ValueError, match="unrecognized normalization"):
        ev.geodesic_label_errors(D, pred, gt, normalization="radius")
    with pytest.raises(ValueError, match="area"):
        ev.geodesic_label_errors(D, pred, gt, normalization="area")


def test_index_and_shape_errors(fx):
    D = fx["small_D"]
    with pytest.raises(IndexError):
        ev.accuracy_many([[0, 160]], [[0, 1]], D)
    with pytest.raises(IndexError):
        ev.accuracy_many([[0, 1]], [[-161, 1]], D)
    with pytest.raises(IndexError):
        ev.accuracy_many([[0, 100]], [[0, 1]], np.zeros((2, 160, 160)), mesh=[1], n_verts=[160, 96])
    with pytest.raises(ValueError, match="as many"):
        ev.accuracy_many([[0, 1]], [], D)
    with pytest.raises(ValueError, match="as many"):
        ev.continuity_many([[0, 1]], D, None, [])
    with pytest.raises(ValueError, match="mesh indices"):
        ev.accuracy_many([[0, 1]], [[0, 1]], D, mesh=[1])
    with pytest.raises(IndexError):
        ev.continuity_many([np.arange(5)], D, None, [np.array([[0, 5]])])
    with pytest.raises(IndexError):
        ev.coverage_many([[0, 160]], fx["a_area"])
    with pytest.raises(ValueError, match="unrecognized normalization"):
        ev.evaluate_pairs([], [], [], [], normalization="radius")
    with pytest.raises(ValueError, match="per pair"):
        ev.evaluate_pairs([], [], [[0]], [])
    assert ev.evaluate_pairs([], [], [], []) == []

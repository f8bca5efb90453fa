"""CPU: multi-view feature lifting.  The float64 restatement (tests/lift_restate.py) and get_features_per_vertex(route="host") against the
reference's recorded float32 run (tests/golden/fx_lift.npz), the raster's invariants, and the refusals."""
import numpy as np
import pytest
import torch

import lift_checks as lc
import lift_restate as rs
from densematcher_amd import projection as pj


@pytest.mark.parametrize("c", lc.CASES)
def test_restatement_reproduces_the_fixture(c):
    d, res = lc.case(c), lc.restated(c)
    assert np.array_equal(res["pix2face"], d["pix2face"]) and np.array_equal(res["ambiguous"], d["ambiguous"])
    assert np.array_equal(lc.visible_mask(res, len(d["verts"])), d["visible"])
    assert np.array_equal(res["count"], d["count"]) and np.array_equal(d["visible"].sum(0), d["count"])
    lc.check(res["features"], d["y_ref32"], d["f32_floor"], f"restatement case {c}")
    covered = int((d["pix2face"] >= 0).sum())
    print(f"case {c}: {int(d['ambiguous'].sum())} ambiguous of {covered} covered pixels")
    assert d["ambiguous"].sum() <= 0.01 * covered


@pytest.mark.parametrize("c", lc.CASES)
@pytest.mark.parametrize("given", [False, True])
def test_host_route_reproduces_the_fixture(c, given):
    d = lc.case(c)
    mesh = lc.Mesh(torch.from_numpy(d["verts"].astype(np.float32)), torch.from_numpy(d["faces"]))
    cams = (torch.from_numpy(d["R"].astype(np.float32)), torch.from_numpy(d["T"].astype(np.float32)))
    fts = torch.from_numpy(d["fts"])
    H = fts.shape[2]
    p2f = torch.from_numpy(d["pix2face"])[..., None] if given else None          # (views, H, W, 1): pytorch3d's shape
    got = pj.get_features_per_vertex("cpu", None, None, mesh, None, ft_dim=fts.shape[1], H=H, W=H, cameras=cams, fts=fts, pix2face=p2f, route="host")
    assert got.dtype == torch.float32 and got.device.type == "cpu"
    lc.check(got, d["y_ref32"], d["f32_floor"], f"host route case {c} given={given}")
    feats, counts = pj.lift_features_many([fts], [(d["verts"], d["faces"])], [(d["R"], d["T"])], route="host", return_counts=True)
    assert np.array_equal(counts[0].numpy(), d["count"])
    assert np.array_equal((feats[0].abs().sum(1) > 0).numpy(), d["count"] > 0)
    p2f_host, vis = pj.rasterize_visibility(mesh, cams, H, H, route="host")
    same = (p2f_host.numpy() == d["pix2face"]) | d["ambiguous"]
    assert same.all() and np.array_equal(vis.numpy(), d["visible"])


@pytest.mark.parametrize("c", lc.CASES)
def test_face_order_does_not_matter(c):
    d = lc.case(c)
    perm = np.random.default_rng(5).permutation(len(d["faces"]))
    for v in range(len(d["R"])):
        want = d["pix2face"][v]
        for raster in (lambda F: rs.raster(d["verts"], F, d["R"][v], d["T"][v], *want.shape)[0],
                       lambda F: pj.host_raster(d["verts"], F, d["R"][v], d["T"][v], *want.shape)):
            got = raster(d["faces"][perm])
            back = np.where(got >= 0, perm[np.maximum(got, 0)], -1)
            assert ((back == want) | d["ambiguous"][v]).all(), (c, v)


def test_equal_depths_go_to_the_lowest_face():
    d = lc.case("a")
    F = np.concatenate((d["faces"], d["faces"]))                 # every face twice: the copy never wins
    flipped = np.concatenate((d["faces"][::-1], d["faces"]))     # ... and the lower index wins whichever copy it is
    for v in (0, 3):
        H, W = d["pix2face"][v].shape
        for raster in (lambda f: rs.raster(d["verts"], f, d["R"][v], d["T"][v], H, W)[0], lambda f: pj.host_raster(d["verts"], f, d["R"][v], d["T"][v], H, W)):
            got = raster(F)
            assert got.max() < len(d["faces"]) and np.array_equal(got, d["pix2face"][v])
            got = raster(flipped)
            assert got.max() < len(d["faces"])
            assert np.array_equal(np.where(got >= 0, len(d["faces"]) - 1 - got, -1), d["pix2face"][v])


def test_degenerate_and_hidden_faces_own_nothing():
    d = lc.case("d")
    nf = len(d["faces"])
    behind, degenerate, rim = nf - 3, nf - 2, nf - 1
    assert not (d["pix2face"] == degenerate).any() and not (d["pix2face"][0] == behind).any() and (d["pix2face"][0] == rim).any()
    x, y, Z = rs.project(d["verts"], d["R"][0], d["T"][0])
    assert (Z[d["faces"][behind]] < 0).all()
    ix = (1.0 - x[d["faces"][rim][0]]) / 2.0 * (d["pix2face"].shape[2] - 1)
    assert d["pix2face"].shape[2] - 1 - 1e-3 <= ix < d["pix2face"].shape[2] - 1
    host = np.stack([pj.host_raster(d["verts"], d["faces"], d["R"][v], d["T"][v], *d["pix2face"][v].shape) for v in range(len(d["R"]))])
    assert np.array_equal(host, d["pix2face"])


def test_look_at_faces_the_target():
    R, T = rs.orbit(3.0, 20.0, 35.0)
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(R), 1.0)
    assert np.allclose(np.zeros(3) @ R + T, [0.0, 0.0, 3.0], atol=1e-14)          # the target lies 3 in front of the camera
    x, y, Z = rs.project(np.array([[0.0, 1.0, 0.0]]), R, T)
    assert y[0] > 0 and abs(x[0]) < 1e-12                                         # +y is up


def test_refusals():
    d = lc.case("c")
    mesh, cams, fts = (d["verts"], d["faces"]), (d["R"], d["T"]), torch.from_numpy(d["fts"])
    call = lambda **kw: pj.get_features_per_vertex("cpu", None, None, kw.pop("mesh", mesh), None, **{**dict(H=24, W=24, cameras=cams, fts=fts, route="host"), **kw})
    with pytest.raises(ValueError, match="square"):
        call(H=24, W=32)
    with pytest.raises(ValueError, match="square"):
        call(fts=torch.zeros((3, 2, 24, 32)))
    with pytest.raises(NotImplementedError, match="fts"):
        call(fts=None)
    with pytest.raises(ValueError, match="cameras"):
        call(cameras=None)
    with pytest.raises(NotImplementedError):
        call(dummy_testing=True)
    bad = d["faces"].copy()
    bad[3, 1] = len(d["verts"])
    with pytest.raises(ValueError, match="indices into"):
        call(mesh=(d["verts"], bad))
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="indices into"):
        call(mesh=(d["verts"], bad))
    p2f = d["pix2face"].copy()
    p2f[0, 0, 0] = len(d["faces"])
    with pytest.raises(ValueError, match="face indices"):
        call(pix2face=p2f)
    with pytest.raises(ValueError, match="one feature map per camera"):
        call(fts=fts[:2])
    with pytest.raises(ValueError, match="route"):
        call(route="gpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            call(route="device")
    with pytest.raises(ValueError, match="square"):
        rs.raster(d["verts"], d["faces"], d["R"][0], d["T"][0], 24, 32)
    assert call().shape == (len(d["verts"]), fts.shape[1])

"""Multi-view feature lifting on the GPU (dm_raster_pix2face, dm_lift_features, MatchEngine.raster_visibility / lift_features, the device
routes of projection.get_features_per_vertex and MeshFeaturizer) against the float64 restatement tests/lift_restate.py and the
reference's recorded float32 runs (tests/golden/fx_lift.npz, fx_featurizer.npz).  Every figure is printed before it is asserted.

Raster sizes: every case at its own size and at 24, 33 and 48.  Case c at 33 has cameras of its own in the fixture (lift_checks.cameras):
with the fixture's view 0 the centre row and column of pixels of an odd size lie ON edges of the unperturbed torus (20 of 418 covered
pixels ambiguous), so that view is stepped by one degree in azimuth and elevation, as the fixture tool steps a view that fails its checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import lift_checks as lc
import lift_restate as rs
import placement as pl
from densematcher_amd import _lib
from densematcher_amd import projection as pj

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def maps_for(views, Cw, H, dtype, seed=0):
    return np.random.default_rng(100 + seed + Cw).standard_normal((views, Cw, H, H)).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- 1. raster
SIZES = [(c, H) for c in lc.CASES for H in sorted({24, 33, 48, lc.case(c)["pix2face"].shape[1]})]


@pytest.mark.parametrize("c,H", SIZES)
def test_raster_against_the_restatement(eng, c, H):
    d = lc.case(c)
    res = lc.restated(c, None if H == d["pix2face"].shape[1] else H)
    p2f, vis = eng.raster_visibility([d["verts"]], [d["faces"]], [lc.cameras(c, H)], H, H)
    got, want, amb = p2f[0].cpu().numpy(), res["pix2face"], res["ambiguous"]
    assert got.dtype == np.int32 and got.shape == want.shape
    covered, differ = int((want >= 0).sum()), int((got != want).sum())
    print(f"case {c} at {H} x {H}: {covered} covered pixels, {int(amb.sum())} ambiguous, {differ} differ from the restatement "
          f"({int(((got != want) & ~amb).sum())} outside the ambiguous ones)")
    assert amb.sum() <= 0.01 * covered                       # the exclusion below cannot hide a failure
    assert ((got == want) | amb).all()
    assert np.array_equal(vis[0].cpu().numpy(), lc.visible_mask(res, len(d["verts"])))
    assert got.min() >= -1 and got.max() < len(d["faces"])


def test_raster_with_pixel_centres_on_mesh_edges(eng):
    """Case c at 33 x 33 with the fixture's OWN cameras: the centre row and column of pixels of view 0 lie exactly on edges of the
    unperturbed torus (a centre on an edge belongs to neither face), and the restatement calls 20 of 418 covered pixels ambiguous
    (4.8 %: above the 1 % that test_raster_against_the_restatement requires, which is why that test steps this view).  Here: equality
    outside the ambiguous pixels, exact visible sets, and the same image whatever the order of the faces."""
    d, H = lc.case("c"), 33
    res = rs.lift(np.zeros((len(d["R"]), 1, H, H)), d["verts"], d["faces"], d["R"], d["T"])
    perm = np.random.default_rng(8).permutation(len(d["faces"]))
    p2f, vis = eng.raster_visibility([d["verts"]] * 2, [d["faces"], d["faces"][perm]], [(d["R"], d["T"])] * 2, H, H)
    got, amb = p2f[0].cpu().numpy(), res["ambiguous"]
    covered = int((res["pix2face"] >= 0).sum())
    print(f"case c at 33 x 33, own cameras: {covered} covered pixels, {int(amb.sum())} ambiguous ({amb.sum() / covered:.3f}), "
          f"{int((got != res['pix2face']).sum())} differ from the restatement ({int(((got != res['pix2face']) & ~amb).sum())} outside the ambiguous ones)")
    assert ((got == res["pix2face"]) | amb).all()
    assert np.array_equal(vis[0].cpu().numpy(), lc.visible_mask(res, len(d["verts"])))
    other = p2f[1].cpu().numpy()
    assert np.array_equal(np.where(other >= 0, perm[np.maximum(other, 0)], -1), got)
    assert torch.equal(vis[0], vis[1])


def test_raster_face_order_and_ties(eng):
    d = lc.case("d")
    nf, H = len(d["faces"]), d["pix2face"].shape[1]
    perm = np.random.default_rng(6).permutation(nf)
    twice = np.concatenate((d["faces"][::-1], d["faces"]))       # every face twice: geometry g lies at nf - 1 - g and at nf + g
    p2f, _ = eng.raster_visibility([d["verts"]] * 2, [d["faces"][perm], twice], [(d["R"], d["T"])] * 2, H, H)
    got = p2f[0].cpu().numpy()
    back = np.where(got >= 0, perm[np.maximum(got, 0)], -1)
    assert ((back == d["pix2face"]) | d["ambiguous"]).all()
    got = p2f[1].cpu().numpy()
    assert got.max() < nf                                        # equal depths: the lower index
    assert ((np.where(got >= 0, nf - 1 - got, -1) == d["pix2face"]) | d["ambiguous"]).all()
    assert not (d["pix2face"] == nf - 2).any() and not (d["pix2face"][0] == nf - 3).any()        # degenerate / behind camera 0


# ---------------------------------------------------------------------------------------------------------------- 2. lifting
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("Cw", [1, 5, 70, 130])
def test_lift_against_the_restatement(eng, Cw, dtype, layout):
    d = lc.case("d")
    H = d["pix2face"].shape[1]
    fts = maps_for(len(d["R"]), Cw, H, dtype)
    ref = rs.lift(fts.astype(np.float64), d["verts"], d["faces"], d["R"], d["T"], pix2face=lc.restated("d")["pix2face"])
    ft = dev(fts)
    if layout == "channels_last":
        ft = ft.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert ft.stride(1) == 1 or Cw == 1
    feats, counts = eng.lift_features([ft], [d["verts"]], [d["faces"]], [(d["R"], d["T"])], return_counts=True)
    assert feats[0].dtype == torch.float32 and tuple(feats[0].shape) == (len(d["verts"]), Cw)
    assert np.array_equal(counts[0].cpu().numpy(), ref["count"])
    lc.check(feats[0], ref["features"], d["f32_floor"], f"lift C={Cw} {np.dtype(dtype).name} {layout}")
    assert bool((feats[0][dev(ref["count"] == 0)] == 0).all())


@pytest.mark.parametrize("dtype,pad,off", [(np.float16, "nan", 3), (np.float32, "+inf", 1), (np.float16, "-inf", 5)])
def test_lift_reads_the_maps_where_they_lie(eng, dtype, pad, off, monkeypatch):
    """the maps as an offset, non-contiguous view (rows and columns of hostile padding around every channel plane)"""
    d = lc.case("d")
    H, Cw = d["pix2face"].shape[1], 5
    fts = maps_for(len(d["R"]), Cw, H, dtype, seed=7)
    want = eng.lift_features([dev(fts)], [d["verts"]], [d["faces"]], [(d["R"], d["T"])])[0]
    placed = pl.place(fts, offset_elems=off, ld=H + 3, rows=H + 2, pad=pad, device=DEV)
    view = placed[..., :H, :H]
    assert not view.is_contiguous() and pl.mod16(view) != 0
    tables, to_device = [], eng._dev
    monkeypatch.setattr(eng, "_dev", lambda t, dtype, name: (tables.append(to_device(t, dtype, name)) or tables[-1]) if name == "maps" else to_device(t, dtype, name))
    with pl.PointerRecorder(eng.lib, "dm_lift_features") as rec:
        got = eng.lift_features([view], [d["verts"]], [d["faces"]], [(d["R"], d["T"])])[0]
    # the library received the table that names the VIEW's own address and strides: no copy was made on the way
    assert len(rec.calls) == 1 and len(tables) == 1 and rec.saw(tables[0])
    assert tables[0].cpu().tolist() == [[view.data_ptr()] + list(view.stride())]
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    ref = rs.lift(fts.astype(np.float64), d["verts"], d["faces"], d["R"], d["T"], pix2face=lc.restated("d")["pix2face"])
    lc.check(got, ref["features"], d["f32_floor"], f"placed maps {np.dtype(dtype).name} {pad}")


def test_taps_on_the_last_row_and_column_read_nothing_behind_them(eng):
    """A tap index of exactly W - 1 (H - 1) makes the + 1 neighbour fall outside the image: it is not read and adds nothing.  The
    library is called with a hand-made projection (x or y = -1 exactly, marked in frame) over maps whose padding behind the last
    column and row is NaN; a read behind the image would show as NaN."""
    H, Cw, n = 9, 3, 4
    fts = maps_for(1, Cw, H, np.float32, seed=11)
    view = pl.place(fts, offset_elems=1, ld=H + 2, rows=H + 2, pad="nan", device=DEV)[..., :H, :H]
    xy = np.array([[-1.0, 0.3], [0.45, -1.0], [-1.0, -1.0], [0.2, 0.1]])              # last column; last row; the corner; inside
    proj = dev(np.concatenate((xy, np.ones((n, 2))), axis=1).reshape(1, 1, n, 4))
    vis = torch.ones((1, 1, n), dtype=torch.uint8, device=DEV)
    table = torch.tensor([[view.data_ptr()] + list(view.stride())], dtype=torch.int64, device=DEV)
    out = torch.full((1, n, Cw), float("nan"), device=DEV)
    cnt = torch.zeros((1, n), dtype=torch.int32, device=DEV)
    P, null = (lambda t: C.c_void_p(t.data_ptr())), C.c_void_p(0)
    eng._chk(eng.lib.dm_lift_features(eng.ctx, 1, n, 1, Cw, H, H, _lib.DM_F32, P(table), P(proj), P(vis), null, null, P(out), Cw, P(cnt)))
    ix, iy = (1.0 - xy[:, 0]) / 2.0 * (H - 1), (1.0 - xy[:, 1]) / 2.0 * (H - 1)
    assert ix[0] == H - 1 and iy[1] == H - 1 and ix[2] == H - 1 and iy[2] == H - 1
    ref = rs.sample(fts[0].astype(np.float64), xy[:, 0], xy[:, 1])
    got = out[0].cpu().double().numpy()
    err = np.abs(got - ref).max()
    print(f"edge taps: max |got - ref| = {err:.3e}, max |ref| = {np.abs(ref).max():.3e}")
    assert np.all(np.isfinite(got)) and cnt.cpu().tolist() == [[1] * n]
    assert err <= 8 * 2.0 ** -24 * np.abs(fts).max()           # four fp32 weights and three fp32 additions on values up to max |map|
    assert np.array_equal(got[2], fts[0, :, H - 1, H - 1].astype(np.float64))          # the corner: one tap of weight 1


# ---------------------------------------------------------------------------------------------------------------- 3. batches
def test_ragged_batch_equals_the_single_calls(eng):
    a, c = lc.case("a"), lc.case("c")
    H, Cw = 24, 5
    meshes = [(a["verts"], a["faces"], a["R"], a["T"]), (c["verts"], c["faces"], c["R"], c["T"]), (a["verts"], a["faces"], a["R"][3:], a["T"][3:])]
    assert [len(m[0]) for m in meshes] == [160, 96, 160] and [len(m[2]) for m in meshes] == [4, 3, 1]
    fts = [dev(maps_for(len(m[2]), Cw, H, np.float32, seed=b)) for b, m in enumerate(meshes)]
    args = lambda ms: ([m[0] for m in ms], [m[1] for m in ms], [(m[2], m[3]) for m in ms])
    p2f, vis = eng.raster_visibility(*args(meshes), H, H)
    feats, counts = eng.lift_features(fts, *args(meshes), return_counts=True)
    for b, m in enumerate(meshes):
        p1, v1 = eng.raster_visibility(*args([m]), H, H)
        f1, c1 = eng.lift_features([fts[b]], *args([m]), return_counts=True)
        assert torch.equal(p2f[b], p1[0]) and torch.equal(vis[b], v1[0]), b
        assert torch.equal(counts[b], c1[0]) and torch.equal(feats[b], f1[0]), b
        assert tuple(feats[b].shape) == (len(m[0]), Cw) and bool(torch.isfinite(feats[b]).all())
        assert int(counts[b].max()) <= len(m[2]) and int(counts[b].max()) > 0
    assert torch.equal(p2f[2][0], p2f[0][3]) and not torch.equal(feats[0], feats[2])


# ---------------------------------------------------------------------------------------------------------------- 4. given pix2face
@pytest.mark.parametrize("c", lc.CASES)
def test_given_pix2face_reproduces_the_reference_run(eng, c, monkeypatch):
    d = lc.case(c)
    mesh = lc.Mesh(dev(d["verts"].astype(np.float32)), dev(d["faces"]))
    cams = (dev(d["R"].astype(np.float32)), dev(d["T"].astype(np.float32)))
    fts = dev(d["fts"])
    H = fts.shape[2]
    with pl.PointerRecorder(eng.lib, "dm_lift_features") as rec:
        got = pj.get_features_per_vertex(DEV, None, None, mesh, None, ft_dim=fts.shape[1], H=H, W=H, cameras=cams, fts=fts,
                                         pix2face=dev(d["pix2face"])[..., None], route="device")
    assert len(rec.calls) == 1 and got.is_cuda and got.dtype == torch.float32
    lc.check(got, d["y_ref32"], d["f32_floor"], f"device route, given pix2face, case {c}")
    own = pj.get_features_per_vertex(DEV, None, None, mesh, None, ft_dim=fts.shape[1], H=H, W=H, cameras=cams, fts=fts, route="device")
    lc.check(own, d["y_ref32"], d["f32_floor"], f"device route, own raster, case {c}")
    auto = pj.get_features_per_vertex(DEV, None, None, mesh, None, ft_dim=fts.shape[1], H=H, W=H, cameras=cams, fts=fts, route="auto")
    lc.check(auto, d["y_ref32"], d["f32_floor"], f"auto route, case {c}")
    monkeypatch.setattr(pj, "AUTO_DEVICE", {"nchw": False, "channels_last": False})      # what "auto" runs where the device route is not taken
    with pl.PointerRecorder(eng.lib, "dm_lift_features") as rec:
        torch_route = pj.get_features_per_vertex(DEV, None, None, mesh, None, ft_dim=fts.shape[1], H=H, W=H, cameras=cams, fts=fts, route="auto")
    assert not rec.calls and torch_route.is_cuda
    lc.check(torch_route, d["y_ref32"], d["f32_floor"], f"torch expressions on the GPU, case {c}")
    # a given pix2face that differs from the raster is what counts: all background -> nothing is seen
    none = eng.lift_features([fts], [d["verts"]], [d["faces"]], [(d["R"], d["T"])], pix2face_list=[torch.full_like(dev(d["pix2face"]), -1)])
    assert bool((none[0] == 0).all())


def test_refusals_without_a_launch(eng):
    d = lc.case("c")
    fts, H = dev(d["fts"]), 24
    bad = d["pix2face"].copy()
    bad[1, 2, 3] = len(d["faces"])
    faces = d["faces"].copy()
    faces[0, 0] = len(d["verts"])
    with pl.PointerRecorder(eng.lib, "dm_raster_pix2face") as r1, pl.PointerRecorder(eng.lib, "dm_lift_features") as r2:
        with pytest.raises(ValueError, match="face indices"):
            eng.lift_features([fts], [d["verts"]], [d["faces"]], [(d["R"], d["T"])], pix2face_list=[bad])
        with pytest.raises(ValueError, match="indices into"):
            eng.lift_features([fts], [d["verts"]], [faces], [(d["R"], d["T"])])
        with pytest.raises(ValueError, match="square"):
            eng.raster_visibility([d["verts"]], [d["faces"]], [(d["R"], d["T"])], 24, 32)
        with pytest.raises(ValueError, match="views"):
            eng.raster_visibility([d["verts"]], [d["faces"]], [(np.tile(d["R"][:1], (65, 1, 1)), np.tile(d["T"][:1], (65, 1)))], H, H)
    assert not r1.calls and not r2.calls
    # the library's own checks
    null, P = C.c_void_p(0), (lambda t: C.c_void_p(t.data_ptr()))
    buf = torch.zeros(4096, dtype=torch.float64, device=DEV)
    for kw in (dict(H=8, W=9), dict(B=0), dict(views=0), dict(focal=0.0)):
        a = dict(B=1, N=4, nt=2, views=1, H=8, W=8, focal=1.0)
        a.update(kw)
        rc = eng.lib.dm_raster_pix2face(eng.ctx, a["B"], a["N"], a["nt"], a["views"], a["H"], a["W"], P(buf), P(buf), null, P(buf), P(buf), null, a["focal"],
                                        null, P(buf), P(buf), P(buf))
        assert rc == _lib.DM_EINVAL, kw
    for kw in (dict(views=65), dict(C=0), dict(f_dtype=7), dict(ldo=2)):
        a = dict(views=1, C=3, f_dtype=_lib.DM_F32, ldo=3)
        a.update(kw)
        rc = eng.lib.dm_lift_features(eng.ctx, 1, 4, a["views"], a["C"], 8, 8, a["f_dtype"], P(buf), P(buf), P(buf), null, null, P(buf), a["ldo"], null)
        assert rc == _lib.DM_EINVAL, kw
    got = eng.lift_features([fts], [d["verts"]], [d["faces"]], [(d["R"], d["T"])])[0]           # the engine is still usable
    lc.check(got, d["y_ref32"], d["f32_floor"], "lift after the refusals")


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def test_featurizer_device_route_and_forward_many():
    from densematcher_amd.diffusion_net import geometry as geo, layers
    fx = lc.golden("fx_featurizer.npz")
    model, _ = lc.featurizer(DEV)
    mesh, ops, cams, fts, p2f = lc.featurizer_inputs(DEV)
    with torch.no_grad():
        outn, out, mv = model(None, mesh, ops, cams, return_mvfeatures=True, fts=fts, route="device")
        assert model.extractor_3d.last_route == "device"
        lc.check(mv, fx["mv_features"], fx["floor_mv"], "device mv_features")
        lc.check(out, fx["out"], fx["f32_floor"], "device out")
        lc.check(outn, fx["out_normalized"], fx["floor_normalized"], "device out_normalized")
        given = model(None, mesh, ops, cams, fts=fts, pix2face=p2f, route="device")
        lc.check(given, fx["out_normalized"], fx["floor_normalized"], "device out_normalized, given pix2face")
        # ---- a ragged pair: the fixture's mesh and case c's
        c = lc.case("c")
        verts_c, faces_c = torch.from_numpy(c["verts"].astype(np.float32)), torch.from_numpy(c["faces"])
        ops_c = tuple(None if o is None else o.to(DEV) for o in geo.compute_operators(verts_c, faces_c, int(fx["k_eig"]), route="host"))
        mesh_c = lc.Mesh(verts_c.to(DEV), faces_c.to(DEV))
        cams_c = (dev(c["R"].astype(np.float32)), dev(c["T"].astype(np.float32)))
        fts_c = dev(maps_for(len(c["R"]), fts.shape[1], fts.shape[2], np.float32, seed=3))
        packed = layers.pack_operators([ops, ops_c], device=DEV)
        many = model.forward_many([None, None], [mesh, mesh_c], packed, [cams, cams_c], return_mvfeatures=True, fts_list=[fts, fts_c])
        one_c = model(None, mesh_c, ops_c, cams_c, return_mvfeatures=True, fts=fts_c, route="device")
    for name, got, want in zip(("normalized", "out", "mv"), many[0], (outn, out, mv)):
        assert torch.equal(got, want), name
    for name, got, want in zip(("normalized", "out", "mv"), many[1], one_c):
        assert torch.equal(got, want), name
    assert tuple(many[1][0].shape) == (96, int(fx["width"]))
    norms = many[1][0].norm(dim=-1)
    print(f"forward_many: row norms of mesh c in [{float(norms.min()):.6f}, {float(norms.max()):.6f}]")
    assert bool(((norms - 1).abs() < 1e-5).all())

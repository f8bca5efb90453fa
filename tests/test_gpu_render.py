"""Textured-mesh rendering on the GPU (dm_render_phong, MatchEngine.render_phong, the device routes of densematcher_amd.render,
projection.get_features_per_vertex and MeshFeaturizer(backbone=)) against the float64 restatement tests/render_restate.py, within the
fp32 floor measured by tests/render_checks.py.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import lift_checks as lc
import placement as pl
import render_checks as rc
import render_restate as rr
from densematcher_amd import _lib
from densematcher_amd import projection as pj
from densematcher_amd import render as rd

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def operands(c, kind, H=None):
    """(verts, faces, (R, T), texture) of a case as MatchEngine.render_phong takes them"""
    V, F, R, T = rc.geometry(c, H)
    return V, F, (R, T), rc.texture(c, kind)


def render(eng, items, H, **kw):
    return eng.render_phong([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], H, H, [i[3] for i in items], **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. restatement
@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("H", rc.SIZES)
@pytest.mark.parametrize("c", rc.CASES)
def test_device_route_against_the_restatement(eng, c, H, kind):
    res = rc.restated(c, H, kind)
    amb, covered = rc.ambiguity(c, H)
    assert amb <= rc.AMBIGUOUS_CAP * covered                         # the exclusion below cannot hide a failure
    out = render(eng, [operands(c, kind, H)], H)
    img, zb, p2f = out.images[0], out.zbuf[0], out.pix2face[0]
    assert img.dtype == torch.float32 and zb.dtype == torch.float32 and p2f.dtype == torch.int32
    print(f"case {c} at {H} x {H}, {kind}: f32_floor = {res['f32_floor']:.3e}, {covered} covered pixels, {amb} ambiguous")
    rc.compare(img.cpu().numpy(), zb.cpu().numpy(), p2f.cpu().numpy(), res, f"device route, case {c} at {H}, {kind}")
    assert bool(torch.isfinite(img).all())


def test_module_routes(eng):
    """render.run_rendering on the device: the reference's shapes and dtypes, the same bits as the engine's call"""
    c, H, kind = "d", 32, "uv8"
    V, F, cams, tex = operands(c, kind, H)
    mesh = rd.Meshes(torch.from_numpy(V.copy()), torch.from_numpy(F.copy()), rd.TexturesUV([torch.from_numpy(tex[1].copy())], [torch.from_numpy(tex[3].copy())],
                                                                                            [torch.from_numpy(tex[2].copy())]))
    img, cam, depth, p2f, _ = rd.run_rendering(DEV, mesh, None, H, H, cams, None, route="device")
    out = render(eng, [(V, F, cams, tex)], H)
    assert img.is_cuda and torch.equal(img, out.images[0]) and torch.equal(depth[..., 0], out.zbuf[0])
    assert p2f.dtype == torch.int64 and tuple(p2f.shape) == (len(cams[0]), H, H, 1) and torch.equal(p2f[..., 0], out.pix2face[0].long())
    assert cam.R.is_cuda and tuple(cam.get_camera_center().shape) == (len(cams[0]), 3)
    host = rd.run_rendering(DEV, mesh, None, H, H, cams, None, route="host")
    res = rc.restated(c, H, kind)
    rc.compare(host[0].cpu().numpy(), host[2].cpu().numpy()[..., 0], host[3].cpu().numpy()[..., 0], res, "host route from a GPU process")


# ---------------------------------------------------------------------------------------------------------------- 2. order, batch
def test_face_order_changes_pix2face_alone(eng):
    c, H = "d", 32
    V, F, cams, tex = operands(c, "uv8", H)
    perm = np.random.default_rng(6).permutation(len(F))
    out = render(eng, [(V, F, cams, tex), (V, F[perm], cams, ("uv", tex[1], tex[2], tex[3][perm]))], H)
    amb = torch.from_numpy(rc.restated(c, H, "uv8")["ambiguous"].copy()).to(DEV)
    a, b = out.pix2face[0], out.pix2face[1]
    back = torch.where(b >= 0, torch.from_numpy(perm).to(DEV)[b.clamp(min=0).long()].to(torch.int32), b)
    assert bool(((back == a) | amb).all())
    assert torch.equal(out.images[0][~amb], out.images[1][~amb]) and torch.equal(out.zbuf[0][~amb], out.zbuf[1][~amb])


def ragged():
    a, c, t, b = operands("a", "vertex"), operands("c", "uv8"), operands("t", "uv57"), operands("b", "none")
    t = (t[0], t[1], (t[2][0][1:2], t[2][1][1:2]), t[3])
    b = (b[0], b[1], (b[2][0][:2], b[2][1][:2]), b[3])
    items = [a, c, t, b]
    assert [len(i[0]) for i in items] == [160, 96, 288, 160] and [len(i[2][0]) for i in items] == [4, 3, 1, 2]
    assert tuple(c[3][1].shape) == (8, 8, 3) and tuple(t[3][1].shape) == (5, 7, 3)
    return items


def test_ragged_batch_equals_the_single_calls(eng):
    items, H = ragged(), 24
    many = render(eng, items, H, planes=torch.float32)
    for k, item in enumerate(items):
        one = render(eng, [item], H, planes=torch.float32)
        for name in ("images", "zbuf", "pix2face", "normals", "planes"):
            assert torch.equal(getattr(many, name)[k], getattr(one, name)[0]), (k, name)
        assert tuple(many.images[k].shape) == (len(item[2][0]), H, H, 4) and bool((many.pix2face[k] >= 0).any())
        assert bool(torch.isfinite(many.images[k]).all())


# ---------------------------------------------------------------------------------------------------------------- 3. normals
def test_vertex_normals(eng):
    items = ragged()
    many = render(eng, items, 16)
    for k, item in enumerate(items):
        want = rr.vertex_normals(item[0], item[1])
        err = np.abs(many.normals[k].cpu().numpy() - want).max()
        print(f"mesh {k}: max |normals - float64 NumPy| = {err:.3e}")
        assert many.normals[k].dtype == torch.float64 and err <= 1e-12
        alone = render(eng, [item], 16)
        assert torch.equal(alone.normals[0], many.normals[k])
    # caller-given normals are used as they are
    V, F, cams, tex = items[0]
    flipped = render(eng, [items[0]], 16, normals_list=[-rr.vertex_normals(V, F)])
    assert torch.equal(flipped.normals[0].cpu(), torch.from_numpy(-rr.vertex_normals(V, F)))
    res = rr.render(V, F, cams[0], cams[1], 16, 16, tex, normals=-rr.vertex_normals(V, F), rasters=rc.rasters("a", 16))
    keep = rc.restated("a", 16, "vertex")["keep"]
    lc.check(flipped.images[0].cpu().numpy()[keep], res["rgba"][keep], rc.restated("a", 16, "vertex")["f32_floor"], "given normals")


def test_vertices_without_a_normal_give_finite_pixels(eng):
    """an unreferenced vertex and two coincident faces of opposite orientation (the sums of their vertices cancel exactly): the eps rule
    leaves zero normals, cos = 0, and the pixels are ambient times the texel"""
    V = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.2, 0.0], [5.0, 5.0, 5.0]])
    F = np.array([[0, 1, 2], [0, 2, 1]], np.int64)
    R, T = np.eye(3)[None], np.array([[0.0, 0.0, 2.5]])
    colours = np.random.default_rng(1).uniform(0.2, 1, (4, 3)).astype(np.float32)
    out = eng.render_phong([V], [F], [(R, T)], 16, 16, [("vertex", colours)])
    assert bool((out.normals[0] == 0).all())
    img, own = out.images[0], out.pix2face[0] >= 0
    assert bool(own.any()) and bool(torch.isfinite(img).all()) and bool((out.pix2face[0][own] == 0).all())      # equal depths: the lower face
    # the restatement of the first face alone with zero normals (with both faces it calls every pixel ambiguous: equal depths)
    res = rr.render(V, F[:1], R, T, 16, 16, ("vertex", colours), normals=np.zeros((4, 3)))
    keep = (res["pix2face"] >= 0) & ~res["ambiguous"]
    assert keep.sum() > 20 and np.array_equal(out.pix2face[0].cpu().numpy()[keep], res["pix2face"][keep])
    err = np.abs(img.cpu().numpy()[keep] - res["rgba"][keep]).max()
    print(f"zero normals: max |got - restatement| = {err:.3e}")
    # ambient * texel: three fp32 roundings of b', three products, two sums and the product with ambient, each <= 2^-24 on values <= 1
    assert err <= 16 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- 4. padding
def test_padding_is_never_read(eng, monkeypatch):
    """rows behind n_verts[b], faces behind a mesh's own and views behind n_views[b] hold NaN / an index outside every mesh, and the
    operands lie off the 16-byte grid: the same bits as the plain call, and background in the views behind n_views[b]"""
    items, H = ragged()[:2], 24
    bg = (0.5, 0.25, 0.75)
    want = render(eng, items, H, background_color=bg, planes=torch.float16)
    n_verts, n_views, n_faces = [160, 96], [4, 3], [len(i[1]) for i in items]
    to_device, placed = eng._dev, []

    def hostile(t, dtype, name):
        if name not in ("verts", "R", "T", "tri"):
            return to_device(t, dtype, name)
        a = np.array(t)
        for b in range(2):
            if name == "verts":
                a[b, n_verts[b]:] = np.nan
            elif name == "tri":
                a[b, n_faces[b]:] = pl.INT_FILL
            else:
                a[b, n_views[b]:] = np.nan
        flat = pl.place(a.reshape(a.shape[0], -1), offset_elems=1, pad=None, device=DEV)
        assert pl.mod16(flat) != 0
        placed.append(name)
        return flat.view(a.shape)

    monkeypatch.setattr(eng, "_dev", hostile)
    got = render(eng, items, H, background_color=bg, planes=torch.float16)
    monkeypatch.setattr(eng, "_dev", to_device)
    assert sorted(placed) == ["R", "T", "tri", "verts"]
    for name in ("images", "zbuf", "pix2face", "normals", "planes"):
        for k in range(2):
            assert torch.equal(getattr(got, name)[k], getattr(want, name)[k]), (name, k)
    rgba, zbuf, p2f = got.padded
    assert tuple(rgba.shape) == (2, 4, H, H, 4) and bool(torch.isfinite(rgba).all())
    assert torch.equal(rgba[1, 3], torch.tensor(bg + (0.0,), device=DEV).expand(H, H, 4))
    assert bool((zbuf[1, 3] == -1).all()) and bool((p2f[1, 3] == -1).all())


# ---------------------------------------------------------------------------------------------------------------- 5. planes
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_planes_are_the_permuted_rgb(eng, dtype):
    out = render(eng, ragged(), 33, planes=dtype)
    for img, p in zip(out.images, out.planes):
        assert p.dtype == dtype and tuple(p.shape) == (img.shape[0], 3, 33, 33)
        assert torch.equal(p, img[..., :3].permute(0, 3, 1, 2).to(dtype))        # fp16: torch rounds to nearest even, as the kernel does


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_without_a_launch(eng):
    V, F, cams, tex = operands("c", "uv8")
    bad = tex[3].copy()
    bad[0, 0] = len(tex[2])
    with pl.PointerRecorder(eng.lib, "dm_render_phong") as rec:
        with pytest.raises(ValueError, match="square"):
            eng.render_phong([V], [F], [cams], 16, 24)
        with pytest.raises(ValueError, match="views"):
            eng.render_phong([V], [F], [(np.tile(cams[0][:1], (65, 1, 1)), np.tile(cams[1][:1], (65, 1)))], 16, 16)
        with pytest.raises(ValueError, match="indices into"):
            eng.render_phong([V], [F], [cams], 16, 16, [("uv", tex[1], tex[2], bad)])
        with pytest.raises(ValueError, match="one RGB row per vertex"):
            eng.render_phong([V], [F], [cams], 16, 16, [("vertex", np.zeros((len(V) + 1, 3), np.float32))])
    assert not rec.calls
    null, P = C.c_void_p(0), (lambda t: C.c_void_p(t.data_ptr()))
    buf = torch.zeros(4096, dtype=torch.float64, device=DEV)
    shade = np.zeros(13, np.float32)
    for kw in (dict(H=8, W=9), dict(B=0), dict(views=65), dict(focal=0.0), dict(n_inc=0)):
        a = dict(B=1, N=4, nt=2, views=1, H=8, W=8, focal=1.0, n_inc=6)
        a.update(kw)
        rc_ = eng.lib.dm_render_phong(eng.ctx, a["B"], a["N"], a["nt"], a["views"], a["H"], a["W"], P(buf), P(buf), null, P(buf), P(buf), null, a["focal"],
                                      P(buf), P(buf), a["n_inc"], null, P(buf), P(buf), null, shade.ctypes.data_as(C.c_void_p), P(buf), P(buf), P(buf), null,
                                      _lib.DM_F32)
        assert rc_ == _lib.DM_EINVAL, kw
    out = render(eng, [operands("c", "uv8", 16)], 16)                  # the engine is still usable
    rc.compare(out.images[0].cpu().numpy(), out.zbuf[0].cpu().numpy(), out.pix2face[0].cpu().numpy(), rc.restated("c", 16, "uv8"), "render after the refusals")


# ---------------------------------------------------------------------------------------------------------------- 7. end to end
def test_get_features_per_vertex_renders_on_the_device():
    d = lc.case("a")
    V, F = rc.geometry("t")[:2]
    raw = rd.Meshes(torch.from_numpy(V * 0.6), torch.from_numpy(F.copy()), rd.TexturesVertex([torch.from_numpy(rc.texture("t", "vertex")[1].copy())]))
    H = 16
    extractor = lambda image: (torch.cat((image.permute(2, 0, 1), image.permute(2, 0, 1).flip(1) * 2 - 1))[None],) * 2
    cams = (torch.from_numpy(d["R"].astype(np.float32)), torch.from_numpy(d["T"].astype(np.float32)))
    got = pj.get_features_per_vertex(DEV, extractor, raw, (d["verts"], d["faces"]), (3, 1), H=H, W=H, cameras=cams, route="device")
    renders = rd.batch_render(DEV, raw, (3, 1), H, H, cams, None, route="device")[0]
    maps = torch.cat([extractor(renders[v][..., :3])[0] for v in range(len(renders))])
    want = pj.get_features_per_vertex(DEV, None, None, (d["verts"], d["faces"]), None, H=H, W=H, cameras=cams, fts=maps, route="device")
    assert got.is_cuda and tuple(got.shape) == (len(d["verts"]), 6) and torch.equal(got, want) and float(got.abs().max()) > 0


def test_featurizer_renders_for_a_backbone():
    from densematcher_amd.diffusion_net import geometry as geo, layers
    from densematcher_amd.featup.upsamplers import JBUStack
    from densematcher_amd.featurizers import AggregationNetwork
    from densematcher_amd.model import MeshFeaturizer
    fx = lc.golden("fx_featurizer.npz")
    names = [str(n) for n in fx["names"]]
    Cw = fx["fts"].shape[1]
    torch.manual_seed(5)
    up = JBUStack(Cw).eval()
    net = AggregationNetwork(feature_dims=[5, 7, 6, 4], projection_dim=Cw, num_norm_groups=3).eval()
    model = MeshFeaturizer(None, (3, 1), int(fx["blocks"]), int(fx["width"]), num_features=Cw, upsampler=up, aggre_net=net)
    model.load_state_dict({n: torch.from_numpy(fx[f"p{i}"].copy()) for i, n in enumerate(names)}, strict=False)
    model = model.to(DEV).eval()
    mesh, ops, cams, _, _ = lc.featurizer_inputs(DEV)
    size, calls = 32, []

    def backbone(images):                                              # deterministic (s3, s4, s5, dino)-shaped functions of the images
        calls.append(images)
        assert images.is_cuda and images.dtype == torch.float32 and tuple(images.shape[1:]) == (3, size, size)
        pool = lambda h: torch.nn.functional.adaptive_avg_pool2d(images, h)
        return tuple(torch.cat([pool(h) * (k + 1) - 0.5 for k in range(3)], dim=1)[:, :c] for c, h in ((5, 2), (7, 1), (6, 1), (4, 2)))

    def raw_mesh(m, seed):
        v, f = m.verts_list()[0], m.faces_list()[0]
        return rd.Meshes(v, f, rd.TexturesVertex([torch.rand(v.shape[0], 3, generator=torch.Generator().manual_seed(seed))]))

    raw = raw_mesh(mesh, 1)
    with torch.no_grad():
        got = model(raw, mesh, ops, cams, return_mvfeatures=True, backbone=backbone, image_size=size, route="device")
        images = rd.render_many(DEV, [raw], None, size, size, [cams], route="device", planes=torch.float32)[0][5]
        assert len(calls) == 1 and torch.equal(calls[0], images) and float(images.std()) > 0
        want = model(None, mesh, ops, cams, return_mvfeatures=True, raw=backbone(images), images=images, route="device")
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        # cameras=None: generated from num_views around the origin
        auto = model(raw, mesh, ops, None, backbone=backbone, image_size=size, route="device")
        assert tuple(auto.shape) == tuple(got[0].shape) and bool(torch.isfinite(auto).all()) and calls[-1].shape[0] == 5
        # ---- a ragged pair
        c = lc.case("c")
        verts_c, faces_c = torch.from_numpy(c["verts"].astype(np.float32)), torch.from_numpy(c["faces"])
        ops_c = tuple(None if o is None else o.to(DEV) for o in geo.compute_operators(verts_c, faces_c, int(fx["k_eig"]), route="host"))
        mesh_c = lc.Mesh(verts_c.to(DEV), faces_c.to(DEV))
        cams_c = (torch.from_numpy(c["R"].astype(np.float32)).to(DEV), torch.from_numpy(c["T"].astype(np.float32)).to(DEV))
        raw_c = raw_mesh(mesh_c, 2)
        packed = layers.pack_operators([ops, ops_c], device=DEV)
        many = model.forward_many([raw, raw_c], [mesh, mesh_c], packed, [cams, cams_c], return_mvfeatures=True, backbone=backbone, image_size=size)
        one_c = model(raw_c, mesh_c, ops_c, cams_c, return_mvfeatures=True, backbone=backbone, image_size=size, route="device")
    for name, a, b in zip(("normalized", "out", "mv"), many[0], got):
        assert torch.equal(a, b), name
    for name, a, b in zip(("normalized", "out", "mv"), many[1], one_c):
        assert torch.equal(a, b), name
    # without backbone= every call fails as before
    with pytest.raises(ValueError, match="fts="):
        model(raw, mesh, ops, cams, route="device")

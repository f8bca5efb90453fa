"""CPU: textured-mesh rendering.  The restatement's ambiguity cap, the host route of densematcher_amd.render against the restatement
(tests/render_restate.py) within the measured fp32 floor (tests/render_checks.py), the UV rule against torch's grid_sample, analytic
renders that do not use the restatement, the camera generator, the refusals and the wiring into get_features_per_vertex.  Every
figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import lift_checks as lc
import lift_restate as rs
import render_checks as rc
import render_restate as rr
from densematcher_amd import projection as pj
from densematcher_amd import render as rd
from densematcher_amd.utils import get_uniform_SO3_RT, look_at_view_transform, recenter


def mesh_of(c, kind, H=None):
    V, F = rc.geometry(c, H)[:2]
    t = lambda a: torch.from_numpy(np.array(a))
    tex = rc.texture(c, kind)
    if tex is not None:
        tex = rd.TexturesVertex([t(tex[1])]) if tex[0] == "vertex" else rd.TexturesUV([t(tex[1])], [t(tex[3])], [t(tex[2])])
    return rd.Meshes(t(V), t(F), tex)


# ---------------------------------------------------------------------------------------------------------------- 1. restatement
@pytest.mark.parametrize("H", rc.SIZES)
@pytest.mark.parametrize("c", rc.CASES)
def test_ambiguous_pixels_stay_under_the_cap(c, H):
    amb, covered = rc.ambiguity(c, H)
    print(f"case {c} at {H} x {H}: {amb} ambiguous of {covered} covered pixels")
    assert covered > 0 and amb <= rc.AMBIGUOUS_CAP * covered


@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("H", rc.SIZES)
@pytest.mark.parametrize("c", rc.CASES)
def test_host_route_against_the_restatement(c, H, kind):
    res = rc.restated(c, H, kind)
    _, _, R, T = rc.geometry(c, H)
    print(f"case {c} at {H} x {H}, {kind}: f32_floor = {res['f32_floor']:.3e}")
    img, cam, depth, p2f, _ = rd.run_rendering("cpu", mesh_of(c, kind, H), None, H, H, (R, T), None, route="host")
    assert img.dtype == torch.float32 and tuple(img.shape) == (len(R), H, H, 4)
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (len(R), H, H, 1)
    assert p2f.dtype == torch.int64 and tuple(p2f.shape) == (len(R), H, H, 1)
    rc.compare(img.numpy(), depth.numpy()[..., 0], p2f.numpy()[..., 0], res, f"host route, case {c} at {H}, {kind}")
    assert ((depth.numpy()[..., 0] > 0) == (res["pix2face"] >= 0))[~res["ambiguous"]].all()
    assert torch.equal(cam.get_camera_center(), -torch.einsum("vk,vjk->vj", cam.T, cam.R)) and len(cam) == len(R)


def test_vertex_normals_against_the_plain_loop():
    V, F = rc.geometry("d")[:2]
    err = np.abs(rd.vertex_normals(V, F) - rr.vertex_normals(V, F)).max()
    print(f"vertex normals: max |host - loop| = {err:.3e}")
    assert err <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- 2. UV sampling
@pytest.mark.parametrize("Ht,Wt", [(8, 8), (5, 7), (1, 4), (3, 1)])
def test_uv_sampling_is_grid_sample_on_the_flipped_map(Ht, Wt):
    """The part that is pinned to torch.  Bound: both sides evaluate x = u (Wt - 1) in fp32 along different expressions (torch goes
    through 2 u - 1), a few roundings on a value of size <= 1.1 max(Ht, Wt), so the tap position -- and with it each bilinear weight --
    moves by at most 8 * 2^-24 * 1.1 * max(Ht, Wt); two weights per axis change, the texel is a combination of values <= max |map|."""
    rng = np.random.default_rng(Ht * 10 + Wt)
    tmap = torch.from_numpy(rng.uniform(0, 1, (Ht, Wt, 3)).astype(np.float32))
    uv = rng.uniform(-0.3, 1.3, (400, 2)).astype(np.float32)
    uv[:8] = [(0, 0), (1, 1), (0, 1), (1, 0), (0.5, 0.5), (-0.2, 0.5), (0.5, 1.2), (1.0, 0.0)]
    want = torch.nn.functional.grid_sample(tmap.flip(0).permute(2, 0, 1)[None], (2 * torch.from_numpy(uv) - 1)[None, None], mode="bilinear",
                                           align_corners=True, padding_mode="border")[0, :, 0].t().numpy()
    bound = 4 * 8 * 2.0 ** -24 * 1.1 * max(Ht, Wt) * float(tmap.abs().max()) + 8 * 2.0 ** -24
    for name, got in (("package", rd.sample_uv(tmap, torch.from_numpy(uv)).numpy()),
                      ("restatement", rr.sample_map(tmap.numpy().astype(np.float64), uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)))):
        err = np.abs(got - want).max()
        print(f"{Ht} x {Wt} map, {name}: max |taps - grid_sample| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


# ---------------------------------------------------------------------------------------------------------------- 3. analytic
def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        mid, G = {}, []
        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    return np.array(V), np.array(F, np.int64)


def test_unit_sphere_centre_pixel():
    """A unit sphere of one colour c, camera and light on the z axis at distance 3, 32 x 32: the pixel next to the centre sees the point
    p where its ray meets the sphere, with n = p and l = v = unit(C - p): rgb = (ambient + diffuse n.l) c + specular (2 (n.l)^2 - 1)^64.
    Faceting error: with the longest edge h of the mesh, a face lies within h^2 / 8 of the sphere and an interpolated normal within
    h^2 of the radial direction (second-order in the chord), so n, l and v move by <= 2 h^2 together; the colour's derivative with
    respect to n.l is <= |diffuse| + 64 * 2 * |specular| <= 0.5 + 1.28: the tolerance is 2 * 2 h^2."""
    V, F = icosphere(3)
    h = np.linalg.norm(V[F[:, 0]] - V[F[:, 1]], axis=1).max()
    colour, H = np.array([0.8, 0.5, 0.3], np.float32), 32
    R, T = rs.look_at((0.0, 0.0, 3.0))
    mesh = rd.Meshes(torch.from_numpy(V), torch.from_numpy(F), rd.TexturesVertex([torch.from_numpy(np.tile(colour, (len(V), 1)))]))
    img = rd.run_rendering("cpu", mesh, None, H, H, (R[None], T[None]), None, route="host")[0][0].numpy()
    r = c = H // 2
    ray = np.array([1.0 - (2 * c + 1) / H, 1.0 - (2 * r + 1) / H, 1.0]) @ R.T
    C = -T @ R.T
    ray /= np.linalg.norm(ray)
    bq = C @ ray
    p = C + (-bq - np.sqrt(bq * bq - (C @ C - 1.0))) * ray
    l = (C - p) / np.linalg.norm(C - p)
    cs = p @ l
    want = (np.array(rr.AMBIENT) + np.array(rr.DIFFUSE) * cs) * colour + np.array(rr.SPECULAR) * (2 * cs * cs - 1) ** 64
    err = np.abs(img[r, c, :3] - want).max()
    print(f"sphere: longest edge h = {h:.4f}, centre pixel {img[r, c]}, analytic {want}, error {err:.3e}, tolerance {4 * h * h:.3e}")
    assert img[r, c, 3] == 1.0 and err <= 4 * h * h
    assert np.array_equal(img[0, 0], [1, 1, 1, 0])


def test_camera_facing_quad_reproduces_the_bilinear_texture():
    """A camera-facing quad at Z = 2 that fills the frame (NDC [-1.5, 1.5] x [-1.5, 1.75]: its diagonal passes through no pixel centre,
    which would belong to neither face), uv = its own plane coordinates, ambient (1, 1, 1) alone: the render is the bilinear
    resampling of the map at the pixel centres.  Every step is exact up to fp32 rounding of uv and of the taps:
    a few 2^-24 on values <= 1, times the 8 texels a unit of uv spans."""
    Ht, Wt, H = 6, 9, 16
    tmap = np.random.default_rng(2).uniform(0, 1, (Ht, Wt, 3)).astype(np.float32)
    V = np.array([[-3.0, -3.0, 2.0], [3.0, -3.0, 2.0], [3.0, 3.5, 2.0], [-3.0, 3.5, 2.0]])
    F = np.array([[0, 1, 2], [0, 2, 3]], np.int64)
    uv = np.array([[1.25, -0.25], [-0.25, -0.25], [-0.25, 1.375], [1.25, 1.375]], np.float32)     # NDC x = +1 (left) is u = 0
    mesh = rd.Meshes(torch.from_numpy(V), torch.from_numpy(F), rd.TexturesUV([torch.from_numpy(tmap)], [torch.from_numpy(F)], [torch.from_numpy(uv)]))
    cams = (np.eye(3)[None], np.zeros((1, 3)))
    img = rd.run_rendering("cpu", mesh, None, H, H, cams, None, route="host", ambient_color=(1, 1, 1), diffuse_color=(0, 0, 0),
                           specular_color=(0, 0, 0))[0][0].numpy()
    px, py = 1.0 - (2.0 * np.arange(H) + 1.0) / H, 1.0 - (2.0 * np.arange(H) + 1.0) / H
    u, v = np.broadcast_to(((1.0 - px) / 2.0)[None, :], (H, H)), np.broadcast_to(((1.0 + py) / 2.0)[:, None], (H, H))
    want = torch.nn.functional.grid_sample(torch.from_numpy(tmap).flip(0).permute(2, 0, 1)[None].double(),
                                           torch.from_numpy(np.stack((2 * u - 1, 2 * v - 1), axis=-1))[None], mode="bilinear", align_corners=True,
                                           padding_mode="border")[0].permute(1, 2, 0).numpy()
    err = np.abs(img[..., :3] - want).max()
    print(f"quad: max |render - bilinear map| = {err:.3e}")
    assert (img[..., 3] == 1).all() and err <= 64 * 2.0 ** -24


def test_background_and_untextured():
    V, F, R, T = rc.geometry("b", 16)
    bg = (0.25, 0.5, 0.125)
    img, _, depth, p2f, _ = rd.run_rendering("cpu", rd.Meshes(torch.from_numpy(V.copy()), torch.from_numpy(F.copy())), None, 16, 16, (R, T), None,
                                             route="host", background_color=bg)
    empty = p2f[..., 0] < 0
    assert bool(empty.any()) and bool((~empty).any())
    assert torch.equal(img[empty], torch.tensor(bg + (0.0,)).expand(int(empty.sum()), 4)) and bool((depth[..., 0][empty] == -1).all())
    # no textures: white times lighting = the restatement with a texture of ones
    ones = rr.render(V, F, R, T, 16, 16, ("vertex", np.ones((len(V), 3), np.float32)), rasters=rc.rasters("b", 16), background=bg)
    keep = rc.restated("b", 16, "none")["keep"]
    lc.check(img.numpy()[keep], ones["rgba"][keep], rc.restated("b", 16, "none")["f32_floor"], "untextured = white")


# ---------------------------------------------------------------------------------------------------------------- 4. cameras
def test_uniform_cameras():
    center, dist = torch.tensor([[0.3, -0.2, 0.5]]), 2.5
    R, T, azi, ele = get_uniform_SO3_RT(4, 3, dist, center)
    assert tuple(R.shape) == (4 * 3 + 2, 3, 3) and tuple(T.shape) == (14, 3) and R.dtype == torch.float32 and T.dtype == torch.float32
    assert torch.equal(azi, torch.tensor([0.0, 90, 180, 270] * 3 + [0.0, 0.0])) and torch.equal(ele, torch.tensor([-45.0] * 4 + [0.0] * 4 + [45.0] * 4 + [-90.0, 90.0]))
    eye3 = torch.eye(3).expand(14, 3, 3)
    print(f"cameras: max |R^T R - I| = {float((R.transpose(1, 2) @ R - eye3).abs().max()):.3e}, det in [{float(torch.linalg.det(R).min()):.7f}, "
          f"{float(torch.linalg.det(R).max()):.7f}]")
    assert float((R.transpose(1, 2) @ R - eye3).abs().max()) <= 1e-6 and float((torch.linalg.det(R) - 1).abs().max()) <= 1e-6
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(T).all())
    seen = center @ R + T[:, None]                                      # the centre in view coordinates
    assert float((seen[:, 0] - torch.tensor([0.0, 0.0, dist])).abs().max()) <= 4e-6
    assert bool((R[:12, 1, 1] > 0).all())                               # +y is up: the camera's y axis has a positive world-y component
    a = np.deg2rad(azi[12:].double().numpy())
    for k, v in enumerate((12, 13)):                                    # the documented limit: x = (-cos a, 0, sin a)
        assert np.abs(R[v, :, 0].numpy() - np.array([-np.cos(a[k]), 0.0, np.sin(a[k])])).max() <= 1e-6
    # a pole view is the limit of the views next to it
    near, _ = look_at_view_transform(dist, [-90.0 + 1e-3, 90.0 - 1e-3], [0.0, 0.0], center)
    assert float((near - R[12:]).abs().max()) <= 1e-4
    R2, T2, azi2, ele2 = get_uniform_SO3_RT(4, 3, dist, center, add_angle_azi=10.0, add_angle_ele=torch.tensor([-2.0]))
    assert torch.equal(azi2, azi + 10) and torch.equal(ele2, ele - 2)
    want, _ = look_at_view_transform(dist, ele2, azi2, center)
    assert torch.equal(R2, want) and not torch.equal(R2, R)
    for v in range(12):                                                 # against the axes of tests/lift_restate.py
        Rr, Tr = rs.orbit(dist, float(ele[v]), float(azi[v]), at=center[0].double().numpy())
        assert np.abs(R[v].numpy() - Rr).max() <= 1e-6 and np.abs(T[v].numpy() - Tr).max() <= 1e-6


def test_default_cameras_and_recenter():
    V, F = rc.geometry("t")[:2]
    mesh = rd.Meshes(torch.from_numpy(V.copy()), torch.from_numpy(F.copy()))
    img, cam, _, p2f, center = rd.batch_render("cpu", mesh, (3, 1), 16, 16, None, None, route="host")
    lo, hi = V.min(0), V.max(0)
    assert len(cam) == 5 and tuple(img.shape) == (5, 16, 16, 4)
    assert np.allclose(center.numpy(), ((lo + hi) / 2)[None])
    want = get_uniform_SO3_RT(3, 1, 2 * np.abs(V).max(), center)
    assert torch.equal(cam.R, want[0]) and torch.equal(cam.T, want[1])
    assert all(bool((p2f[v] >= 0).any()) for v in range(5))             # the mesh is in every frame
    a, b = recenter(V, V[::3] + 0.5)
    c = ((V[::3] + 0.5).min(0) + (V[::3] + 0.5).max(0)) / 2
    assert np.array_equal(a, V - c) and np.array_equal(b, V[::3] + 0.5 - c)


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    V, F, R, T = rc.geometry("c", 16)
    t = lambda a: torch.from_numpy(np.array(a))
    call = lambda mesh=None, **kw: rd.run_rendering("cpu", mesh or rd.Meshes(t(V), t(F)), None, kw.pop("H", 16), kw.pop("W", 16), kw.pop("cameras", (R, T)), None,
                                                    **{**dict(route="host"), **kw})
    with pytest.raises(ValueError, match="square"):
        call(H=16, W=24)
    with pytest.raises(ValueError, match="views"):
        call(cameras=(np.tile(R[:1], (65, 1, 1)), np.tile(T[:1], (65, 1))))
    with pytest.raises(ValueError, match="one RGB row per vertex"):
        call(rd.Meshes(t(V), t(F), rd.TexturesVertex([torch.zeros(len(V) - 1, 3)])))
    tex = rc.texture("c", "uv8")
    bad = tex[3].copy()
    bad[2, 1] = len(tex[2])
    with pytest.raises(ValueError, match="indices into"):
        call(rd.Meshes(t(V), t(F), rd.TexturesUV([t(tex[1])], [t(bad)], [t(tex[2])])))
    bad[2, 1] = -1
    with pytest.raises(ValueError, match="indices into"):
        call(rd.Meshes(t(V), t(F), rd.TexturesUV([t(tex[1])], [t(bad)], [t(tex[2])])))
    with pytest.raises(ValueError, match="one row per face"):
        call(rd.Meshes(t(V), t(F), rd.TexturesUV([t(tex[1])], [t(tex[3][:-1])], [t(tex[2])])))
    with pytest.raises(ValueError, match="route"):
        call(route="gpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            call(route="device")
    assert tuple(call()[0].shape) == (len(R), 16, 16, 4)


# ---------------------------------------------------------------------------------------------------------------- 6. lifting
def test_get_features_per_vertex_renders_and_lifts():
    d = lc.case("a")
    simp = (d["verts"], d["faces"])
    V, F = rc.geometry("t")[:2]
    raw = rd.Meshes(torch.from_numpy(V * 0.6), torch.from_numpy(F.copy()), rd.TexturesVertex([torch.from_numpy(rc.texture("t", "vertex")[1].copy())]))
    H, seen = 16, []

    def extractor(image):                                               # a known function of the image: (ft_hr, ft_lr)
        seen.append(image)
        assert tuple(image.shape) == (H, H, 3)
        hr = torch.cat((image.permute(2, 0, 1), image.permute(2, 0, 1).flip(1) * 2 - 1))[None]
        return hr, torch.nn.functional.avg_pool2d(hr, 2)

    cams = (torch.from_numpy(d["R"].astype(np.float32)), torch.from_numpy(d["T"].astype(np.float32)))
    for lr in (False, True):
        seen.clear()
        got = pj.get_features_per_vertex("cpu", extractor, raw, simp, (3, 1), H=H, W=H, cameras=cams, fts=None, use_lr_features=lr, route="host")
        renders = rd.batch_render("cpu", raw, (3, 1), H, H, cams, None, route="host")[0]
        assert len(seen) == len(cams[0]) and all(torch.equal(s, renders[v][..., :3]) for v, s in enumerate(seen))
        maps = torch.cat([extractor(renders[v][..., :3])[1 if lr else 0] for v in range(len(renders))])
        h = maps.shape[2]
        owner = torch.from_numpy(np.stack([pj.host_raster(d["verts"].astype(np.float64), d["faces"], d["R"].astype(np.float32).astype(np.float64)[v],
                                                          d["T"].astype(np.float32).astype(np.float64)[v], h, h) for v in range(len(cams[0]))]))
        want, _ = pj._torch_lift(maps, torch.from_numpy(d["verts"]), torch.from_numpy(d["faces"]), cams[0].double(), cams[1].double(), owner, 1.0, "cpu")
        assert tuple(got.shape) == (len(d["verts"]), 6) and torch.equal(got, want) and float(got.abs().max()) > 0
    # cameras=None: generated from num_views and center, the same for the render and the lifting
    got = pj.get_features_per_vertex("cpu", extractor, raw, simp, (3, 1), H=H, W=H, cameras=None, center=None, route="host")
    assert tuple(got.shape) == (len(d["verts"]), 6) and bool(torch.isfinite(got).all())
    # what tests/test_lift_cpu.py::test_refusals pins still raises
    fts = torch.from_numpy(d["fts"])
    with pytest.raises(NotImplementedError, match="fts"):
        pj.get_features_per_vertex("cpu", None, None, simp, None, H=24, W=24, cameras=cams, fts=None, route="host")
    with pytest.raises(ValueError, match="cameras"):
        pj.get_features_per_vertex("cpu", None, None, simp, None, H=24, W=24, cameras=None, fts=fts, route="host")
    with pytest.raises(NotImplementedError):
        pj.get_features_per_vertex("cpu", None, None, simp, None, H=24, W=24, cameras=cams, fts=fts, dummy_testing=True, route="host")

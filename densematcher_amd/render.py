"""
densematcher.render of the reference: run_rendering / batch_render (render.py:13-68), the hard-Phong views of the raw, textured mesh
that the 2D backbone takes, with their cameras, depth and pix2face.  The reference renders with pytorch3d, which has no ROCm build;
this module needs no pytorch3d.

THE DEFINITION ('Textured-mesh rendering').  It is this package's restatement of pytorch3d's defaults for
RasterizationSettings(blur_radius=0, faces_per_pixel=1), HardPhongShader, default Materials and default BlendParams.  The raster rule,
the camera formula and the shading are THIS PACKAGE's: they are not pinned against pytorch3d.
  cameras, pixel centres, the face-skipping rule, ownership: exactly those of projection.py (row vectors, X_view = X_world R + T, focal
              length 1, NDC +x left / +y up, square images, Z_MIN, AREA_MIN, ties to the lowest face).
  barycentrics  at the owning face the screen-space barycentrics b_i of the raster, perspective-corrected:
              b'_i = (b_i / Z_i) / sum_j (b_j / Z_j); no clipping.  zbuf = 1 / sum b_i / Z_i, the fp32 value the raster compares.
              Background: pix2face = -1, zbuf = -1.
  normals     per vertex the sum over the incident faces of cross(v1 - v0, v2 - v0) (area-weighted, the same vector at all three
              corners), n / max(|n|, 1e-6).
  per pixel   position p and normal n interpolated with b' from the face's vertices, n normalised again (eps 1e-6).
  texels      none: white.  Vertex colours: the b'-interpolation of the per-vertex RGB.  UV: uv interpolated from
              verts_uvs[faces_uvs[f]]; the map (Ht, Wt, 3) fp32 is sampled as grid_sample(flip(map, rows), 2 uv - 1, bilinear,
              align_corners=True, padding_mode="border"): x = u (Wt - 1), y = (1 - v)(Ht - 1), clamped to the map, four taps.
  lighting    one point light per view at light_location (default: the camera centre C = -T R^T).  l = unit(L - p), cos = n.l;
              diffuse = diffuse_color relu(cos); v = unit(C - p), r = -l + 2 cos n, alpha = relu(v.r) [cos > 0], specular =
              specular_color alpha^shininess; unit(a) = a / max(|a|, 1e-6).  Materials all ones, shininess 64.
              rgb = (ambient_color + diffuse) texel + specular.  Defaults (render.py:37-43): diffuse (0.4, 0.4, 0.5), ambient
              (0.6, 0.6, 0.6), specular (0.01, 0.01, 0.01).
  blend       (views, H, W, 4) fp32: a covered pixel gets (rgb, 1), background (background_color, 0), default (1, 1, 1).  Nothing is
              clamped (the reference clips only when it saves PNGs).
  cameras=None  radius = max |bounding box|, centre = the bounding box's mean unless given, utils.get_uniform_SO3_RT(num_views[0],
              num_views[1], distance = 2 radius, centre); its pole views deviate from pytorch3d's as stated there.

Routes:
  host     the raster in float64 NumPy (projection.host_raster), barycentrics in float64, shading in vectorised fp32 torch on the CPU
  device   MatchEngine.render_phong: dm_render_phong, every mesh and view of a call in one device call
  auto     the device route when a GPU is present and tools/render_time.py measured it not slower (AUTO_DEVICE), else host
Loading OBJ / MTL / image files is outside this package.
"""
import numpy as np
import torch

from . import _routes
from ._engine_render import AMBIENT, BACKGROUND, DIFFUSE, SHININESS, SPECULAR, shade_params
from ._operands import image_frame, lift_cameras, lift_mesh, render_normals, render_points, render_texture
from .projection import host_raster, mesh_arrays

# whether route="auto" takes the device in a process with a GPU: where tools/render_time.py measured the device route not slower than the
# host route on an MI355X (README.md): 4.4 ms against 9.9 s for one mesh of 102 400 faces, five 512 x 512 views
AUTO_DEVICE = True

MAX_VIEWS = 64
EPS = 1e-6


# ------------------------------------------------------------------------------------------------------------------ containers
class TexturesVertex:
    """per-vertex RGB, under pytorch3d's accessor: verts_features_list()"""

    def __init__(self, verts_features):
        self._f = [verts_features] if isinstance(verts_features, torch.Tensor) and verts_features.dim() == 2 else list(verts_features)

    def verts_features_list(self):
        return self._f


class TexturesUV:
    """a UV map per mesh, under pytorch3d's accessors: maps_padded(), verts_uvs_list(), faces_uvs_list()"""

    def __init__(self, maps, faces_uvs, verts_uvs):
        one = lambda a, d: [a] if isinstance(a, torch.Tensor) and a.dim() == d else list(a)
        self._maps, self._fuv, self._uv = one(maps, 3), one(faces_uvs, 2), one(verts_uvs, 2)

    def maps_padded(self):
        return torch.stack(self._maps)

    def verts_uvs_list(self):
        return self._uv

    def faces_uvs_list(self):
        return self._fuv


class Meshes:
    """what this package reads of a pytorch3d Meshes: verts_list(), faces_list(), .textures (for callers, tools and tests without pytorch3d)"""

    def __init__(self, verts, faces, textures=None):
        self._v = [verts] if isinstance(verts, torch.Tensor) and verts.dim() == 2 else list(verts)
        self._f = [faces] if isinstance(faces, torch.Tensor) and faces.dim() == 2 else list(faces)
        self.textures = textures

    def __len__(self):
        return len(self._v)

    def verts_list(self):
        return self._v

    def faces_list(self):
        return self._f


class Cameras:
    """the cameras of a rendering: R (views, 3, 3), T (views, 3) and get_camera_center() (the reference returns PerspectiveCameras)"""

    def __init__(self, R, T):
        self.R, self.T = R, T

    def __len__(self):
        return self.R.shape[0]

    def get_camera_center(self):
        """C = -T R^T, (views, 3)"""
        return -torch.einsum("vk,vjk->vj", self.T, self.R)


def texture_of(mesh):
    """the texture of a mesh argument as MatchEngine.render_phong takes it: None, ("vertex", colours) or ("uv", map, verts_uvs, faces_uvs)"""
    tex = getattr(mesh, "textures", None)
    if tex is None:
        return None
    if hasattr(tex, "verts_features_list"):
        return ("vertex", tex.verts_features_list()[0])
    if hasattr(tex, "verts_uvs_list") and hasattr(tex, "faces_uvs_list"):
        return ("uv", tex.maps_padded()[0], tex.verts_uvs_list()[0], tex.faces_uvs_list()[0])
    raise TypeError("a texture offers verts_features_list(), or maps_padded() / verts_uvs_list() / faces_uvs_list()")


# ------------------------------------------------------------------------------------------------------------------ host route
def vertex_normals(V, F):
    """(n, 3) float64: the sum over the incident faces of cross(v1 - v0, v2 - v0), n / max(|n|, 1e-6)"""
    cr = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    s = np.zeros_like(V)
    for k in range(3):
        np.add.at(s, F[:, k], cr)
    return s / np.maximum(np.linalg.norm(s, axis=1, keepdims=True), EPS)


def sample_uv(tmap, uv):
    """the UV rule of the definition on torch: tmap (Ht, Wt, 3), uv (k, 2) -> (k, 3), four taps nw, ne, sw, se"""
    Ht, Wt = tmap.shape[:2]
    x = (uv[:, 0] * (Wt - 1)).clamp(0, Wt - 1)
    y = ((1 - uv[:, 1]) * (Ht - 1)).clamp(0, Ht - 1)
    fx, fy = x.floor(), y.floor()
    xa, ya = fx.long(), fy.long()
    xb, yb = (xa + 1).clamp(max=Wt - 1), (ya + 1).clamp(max=Ht - 1)
    tx, ty = (x - fx)[:, None], (y - fy)[:, None]
    return (1 - tx) * (1 - ty) * tmap[ya, xa] + tx * (1 - ty) * tmap[ya, xb] + (1 - tx) * ty * tmap[yb, xa] + tx * ty * tmap[yb, xb]


def _unit(a):
    return a / a.norm(dim=1, keepdim=True).clamp(min=EPS)


def _host_view(V, F, R, T, H, W, focal, tex, normals, light, shade):
    """one view on the host: (rgba (H, W, 4) fp32, zbuf (H, W) fp32, pix2face (H, W) int32)"""
    owner = host_raster(V, F, R, T, H, W, focal)
    amb, dif, spc, bg = (torch.from_numpy(shade[3 * k:3 * k + 3].copy()) for k in range(4))
    rgba = torch.cat((bg, torch.zeros(1))).repeat(H, W, 1)
    zbuf = torch.full((H, W), -1.0)
    rr, cc = np.nonzero(owner >= 0)
    if len(rr) == 0:
        return rgba, zbuf, torch.from_numpy(owner)
    idx = F[owner[rr, cc]]
    Xv = V @ R + T
    x, y, Z = focal * Xv[:, 0] / Xv[:, 2], focal * Xv[:, 1] / Xv[:, 2], Xv[:, 2]
    (x0, x1, x2), (y0, y1, y2), Zf = x[idx].T, y[idx].T, Z[idx]
    area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
    px, py = 1.0 - (2.0 * cc + 1.0) / W, 1.0 - (2.0 * rr + 1.0) / H
    b = np.stack(((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1), (px - x2) * (y0 - y2) - (py - y2) * (x0 - x2),
                  (px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)), axis=1) / area[:, None]
    q = b / Zf
    zbuf[rr, cc] = torch.from_numpy((1.0 / q.sum(1)).astype(np.float32))
    c = torch.from_numpy((q / q.sum(1, keepdims=True)).astype(np.float32))                  # fp32 from here on
    mix = lambda a: (c[:, :, None] * a).sum(1)
    idx_t = torch.from_numpy(idx)
    p = mix(torch.from_numpy(V.astype(np.float32))[idx_t])
    n = _unit(mix(torch.from_numpy(normals.astype(np.float32))[idx_t]))
    if tex[0] == 0:
        texel = torch.ones_like(p)
    elif tex[0] == 1:
        texel = mix(tex[1].cpu()[idx_t])
    else:
        fuv = torch.from_numpy(tex[3].astype(np.int64))[torch.from_numpy(owner[rr, cc].astype(np.int64))]
        texel = sample_uv(tex[1].cpu(), mix(tex[2].cpu()[fuv]))
    centre = torch.from_numpy((-(R @ T)).astype(np.float32))
    L = centre if light is None else torch.from_numpy(light.astype(np.float32))
    l, e = _unit(L - p), _unit(centre - p)
    cs = (n * l).sum(1, keepdim=True)
    r = -l + 2 * cs * n
    alpha = (e * r).sum(1, keepdim=True).clamp(min=0) * (cs > 0)
    rgb = (amb + dif * cs.clamp(min=0)) * texel + spc * alpha ** float(shade[12])
    rgba[rr, cc] = torch.cat((rgb, torch.ones(len(rr), 1)), dim=1)
    return rgba, zbuf, torch.from_numpy(owner)


# ------------------------------------------------------------------------------------------------------------------ public
def default_cameras(verts, num_views, center, device="cpu", add_angle_azi=0, add_angle_ele=0):
    """((R, T), center) as run_rendering places them without cameras (render.py:21-26): radius = max |bounding box|, centre = the
    bounding box's mean unless given, get_uniform_SO3_RT at distance 2 radius"""
    from .utils import get_uniform_SO3_RT
    v = verts if isinstance(verts, torch.Tensor) else torch.as_tensor(np.asarray(verts))
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    radius = torch.maximum(lo.abs().max(), hi.abs().max())
    if center is None:
        center = ((lo + hi) / 2)[None]
    R, T, _, _ = get_uniform_SO3_RT(num_azimuth=num_views[0], num_elevation=num_views[1], center=center, distance=radius * 2, device=device,
                                    add_angle_azi=add_angle_azi, add_angle_ele=add_angle_ele)
    return (R, T), center


def render_many(device, meshes, num_views, H, W, cameras_list=None, centers=None, add_angle_azi=0, add_angle_ele=0, *, route="auto",
                normals_list=None, light_location=None, ambient_color=AMBIENT, diffuse_color=DIFFUSE, specular_color=SPECULAR, shininess=SHININESS,
                background_color=BACKGROUND, focal_length=1.0, planes=None):
    """run_rendering for a list of meshes: ONE device call on the device route.  cameras_list[b] = (R, T) or None (generated from
    num_views and centers[b]); light_location: None (the camera centres) or a list of (views_b, 3) per mesh.  Returns per mesh
    (batched_renderings (views, H, W, 4), camera, depth (views, H, W, 1), pix2face (views, H, W, 1) int64, center); with planes=
    torch.float32 | torch.float16 a sixth entry, the RGB planes (views, 3, H, W)."""
    who = "render_many"
    Bn = len(meshes)
    H, W = image_frame(H, W, None, who)
    cameras_list = [None] * Bn if cameras_list is None else list(cameras_list)
    centers = [None] * Bn if centers is None else list(centers)
    if Bn == 0 or len(cameras_list) != Bn or len(centers) != Bn or (light_location is not None and len(light_location) != Bn):
        raise ValueError(f"{who}: one (R, T) pair (or None), one centre (or None) and one light list (or None) per mesh")
    pairs = [mesh_arrays(m) for m in meshes]
    cams = []
    for b in range(Bn):
        if cameras_list[b] is None:
            cam, centers[b] = default_cameras(pairs[b][0], num_views, centers[b], "cpu", add_angle_azi, add_angle_ele)
        else:
            cam = cameras_list[b]
        cams.append(cam)
    textures = [texture_of(m) for m in meshes]
    if _routes.pick_host(route, AUTO_DEVICE) == "device":
        out = _routes.engine_or_none().render_phong([p[0] for p in pairs], [p[1] for p in pairs], cams, H, W, textures, normals_list, light_location,
                                     ambient_color, diffuse_color, specular_color, shininess, background_color, focal_length, planes)
        images, zbufs, p2fs, pls = out.images, out.zbuf, out.pix2face, out.planes
    else:
        if planes not in (None, torch.float32, torch.float16):
            raise ValueError(f"{who}: planes must be None, torch.float32 or torch.float16")
        shade = shade_params(ambient_color, diffuse_color, specular_color, background_color, shininess, who)
        images, zbufs, p2fs, pls = [], [], [], None if planes is None else []
        for b in range(Bn):
            tag = f"{who}: mesh {b}"
            V, F = lift_mesh(*pairs[b], tag)
            R, T = lift_cameras(cams[b], tag, MAX_VIEWS)
            tex = render_texture(textures[b], len(V), len(F), tag)
            nrm = render_normals(None if normals_list is None else normals_list[b], len(V), tag)
            nrm = vertex_normals(V, F) if nrm is None else nrm
            light = render_points(None if light_location is None else light_location[b], len(R), tag, "light_location")
            views = [_host_view(V, F, R[v], T[v], H, W, focal_length, tex, nrm, None if light is None else light[v], shade) for v in range(len(R))]
            images.append(torch.stack([v[0] for v in views])), zbufs.append(torch.stack([v[1] for v in views]))
            p2fs.append(torch.stack([v[2] for v in views]))
            if pls is not None:
                pls.append(images[-1][..., :3].permute(0, 3, 1, 2).contiguous().to(planes))
    res = []
    for b in range(Bn):
        R, T = (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.array(t)) for t in cams[b])
        one = (images[b].to(device), Cameras(R.to(device), T.to(device)), zbufs[b].to(device)[..., None], p2fs[b].to(device=device, dtype=torch.int64)[..., None],
               centers[b])
        res.append(one if pls is None else one + (pls[b].to(device),))
    return res


def run_rendering(device, mesh, num_views, H, W, cameras, center, add_angle_azi=0, add_angle_ele=0, *, route="auto", **shading):
    """The reference's run_rendering (render.py:13-54), its names and argument order.  mesh: anything with verts_list()[0] /
    faces_list()[0] and an optional .textures (pytorch3d's accessors, or TexturesVertex / TexturesUV of this module); num_views =
    (num_azimuth, num_elevation), ignored when cameras = (R, T) is given.  Returns (batched_renderings (views, H, W, 4), camera, depth
    (views, H, W, 1), pix2face (views, H, W, 1) int64 of the mesh's own face indices, center)."""
    return render_many(device, [mesh], num_views, H, W, [cameras], [center], add_angle_azi, add_angle_ele, route=route, **shading)[0]


def batch_render(device, mesh, num_views, H, W, cameras, center, *, route="auto", **shading):
    """The reference's batch_render (render.py:56-68).  Its retry loop answers a LinAlgError of pytorch3d's pole views; the pole views
    here are defined by their limit (utils.look_at_view_transform) and nothing is retried."""
    return run_rendering(device, mesh, num_views, H, W, cameras, center, route=route, **shading)

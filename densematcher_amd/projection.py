"""
densematcher.projection of the reference: get_features_per_vertex, the back-projection of per-view 2D feature maps onto the vertices
of the simplified mesh (reference projection.py:27-130), with the feature maps GIVEN (fts=) or made from the rendered views of the raw
mesh (render.py) by a callable extractor=.  The 2D backbone itself is outside this package.

What the reference takes from pytorch3d is restated here ('Multi-view feature lifting'):
  cameras     (R (views,3,3), T (views,3)), row vectors: X_view = X_world R + T; PerspectiveCameras' defaults: focal length 1, principal
              point 0, NDC with +x left, +y up: x = X / Z, y = Y / Z.  Square images only.
  pix2face    the face of the simplified mesh nearest to the camera at each pixel centre x_c = 1 - (2c+1)/W, y_r = 1 - (2r+1)/H, -1 for
              background.  A face is skipped when a vertex has Z <= 1e-6 or a non-finite projection or when |signed area| <= 1e-8; a
              centre is inside where all three barycentric coordinates are > 0; depth 1 / sum b_i / Z_i, compared as fp32; equal
              depths go to the lowest face index.
The raster rule and the camera formula are THIS PACKAGE's: they are not pinned against pytorch3d.  A caller who has pytorch3d's
rasteriser passes its pix2face= (any integer (views,H,W) or (views,H,W,1) array of face indices of the simplified mesh); from there on
-- visible faces, their vertices, the frame test, grid_sample, the mean over views -- the computation is the reference's, pinned by
its own recorded run (tests/golden/fx_lift.npz).

Routes:
  host     the raster in float64 NumPy, then the stage on PyTorch (_torch_lift) on the CPU
  device   MatchEngine.lift_features: dm_raster_pix2face + dm_lift_features (float64 projection and raster, fp32 taps)
  auto     the device route when a GPU is present and tools/lift_time.py measured it not slower (AUTO_DEVICE), else the NumPy raster and
           _torch_lift on the device of the maps
"""
import numpy as np
import torch

from . import _routes
from ._operands import image_frame, lift_cameras, lift_mesh, lift_pix2face

# where tools/lift_time.py measured the device route (its own raster pass included) not slower than the torch route on an MI355X
# (README.md), by the layout of the maps: 1.07 ms against 32.5 ms (NCHW), 0.38 ms against 17.4 ms (channels-last)
AUTO_DEVICE = {"nchw": True, "channels_last": True}

Z_MIN = 1e-6
AREA_MIN = 1e-8


def mesh_arrays(mesh):
    """(verts, faces) of a mesh argument: anything with verts_list()[0] / faces_list()[0] (pytorch3d's Meshes), or a (verts, faces) pair"""
    if hasattr(mesh, "verts_list"):
        return mesh.verts_list()[0], mesh.faces_list()[0]
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        return mesh[0], mesh[1]
    raise TypeError("a mesh is an object with verts_list() / faces_list() or a (verts, faces) pair")


# ---------------------------------------------------------------------------------------------------------------------
def host_raster(V, F, R, T, H, W, focal_length=1.0):
    """pix2face (H, W) int32 of one view in float64 NumPy: the rule at the top of this file, one face at a time over its pixel box"""
    Xv = V @ R + T
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y, Z = focal_length * Xv[:, 0] / Xv[:, 2], focal_length * Xv[:, 1] / Xv[:, 2], Xv[:, 2]
        xf, yf, Zf = x[F], y[F], Z[F]
        area = (xf[:, 2] - xf[:, 0]) * (yf[:, 1] - yf[:, 0]) - (yf[:, 2] - yf[:, 0]) * (xf[:, 1] - xf[:, 0])
        keep = (Zf > Z_MIN).all(1) & np.isfinite(xf).all(1) & np.isfinite(yf).all(1) & (np.abs(area) > AREA_MIN)
    best = np.full((H, W), np.inf, np.float32)
    owner = np.full((H, W), -1, np.int32)
    cols, rows = 1.0 - (2.0 * np.arange(W) + 1.0) / W, 1.0 - (2.0 * np.arange(H) + 1.0) / H
    for f in np.flatnonzero(keep):
        c_lo = int(max(0.0, np.floor(((1.0 - xf[f].max()) * W - 1.0) * 0.5) - 1.0))
        c_hi = int(min(W - 1.0, np.ceil(((1.0 - xf[f].min()) * W - 1.0) * 0.5) + 1.0))
        r_lo = int(max(0.0, np.floor(((1.0 - yf[f].max()) * H - 1.0) * 0.5) - 1.0))
        r_hi = int(min(H - 1.0, np.ceil(((1.0 - yf[f].min()) * H - 1.0) * 0.5) + 1.0))
        if c_lo > c_hi or r_lo > r_hi:
            continue
        px, py = cols[None, c_lo:c_hi + 1], rows[r_lo:r_hi + 1, None]
        (x0, x1, x2), (y0, y1, y2) = xf[f], yf[f]
        b0 = ((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1)) / area[f]
        b1 = ((px - x2) * (y0 - y2) - (py - y2) * (x0 - x2)) / area[f]
        b2 = ((px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)) / area[f]
        inside = (b0 > 0) & (b1 > 0) & (b2 > 0)
        if not inside.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            z = (1.0 / (b0 / Zf[f, 0] + b1 / Zf[f, 1] + b2 / Zf[f, 2])).astype(np.float32)
        bb, oo = best[r_lo:r_hi + 1, c_lo:c_hi + 1], owner[r_lo:r_hi + 1, c_lo:c_hi + 1]
        take = inside & (z < bb)            # ascending face index: an equal depth keeps the lower face
        bb[take], oo[take] = z[take], f
    return owner


def _torch_lift(maps, verts, faces, R, T, pix2face, focal_length, device):
    """The stage on PyTorch, any device, from its definitions (top of this file): maps (views, C, H, W), pix2face (views, H, W) integers.
    All vertices of a view are projected at once (in the vertices' dtype, fp32 at least), the vertices of the owning faces are marked
    through a mask, and the marked vertices inside the frame are sampled with grid_sample at -(x, y).  Returns (mean (n, C) fp32,
    number of views per vertex (n) int32)."""
    real = verts.dtype if verts.dtype in (torch.float32, torch.float64) else torch.float32
    verts = verts.to(device=device, dtype=real)
    corners = faces.to(device=device, dtype=torch.long)
    owner = pix2face.to(device=device, dtype=torch.long).flatten(1)
    n, n_views = verts.shape[0], maps.shape[0]
    total = torch.zeros((n, maps.shape[1]), dtype=torch.float32, device=device)
    seen_by = torch.zeros(n, dtype=torch.int32, device=device)
    for v in range(n_views):
        cam = verts @ R[v].to(device=device, dtype=real) + T[v].to(device=device, dtype=real)
        xy = focal_length * cam[:, :2] / cam[:, 2:]
        on_owning_face = torch.zeros(n, dtype=torch.bool, device=device)
        on_owning_face[corners[owner[v][owner[v] >= 0]].flatten()] = True
        keep = torch.nonzero(on_owning_face & (xy.abs() < 1).all(dim=1)).flatten()
        grid = (-xy[keep]).to(torch.float32).reshape(1, 1, -1, 2)
        taps = torch.nn.functional.grid_sample(maps[v:v + 1].to(device=device, dtype=torch.float32), grid, mode="bilinear", padding_mode="zeros",
                                               align_corners=True)
        total.index_add_(0, keep, taps[0, :, 0, :].t())
        seen_by[keep] += 1
    return torch.where(seen_by[:, None] > 0, total / seen_by.clamp(min=1)[:, None], total), seen_by


def _layout(ft):
    return "channels_last" if ft.dim() == 4 and ft.stride(1) == 1 and ft.shape[1] > 1 else "nchw"


def _as_maps(fts, who):
    ft = fts if isinstance(fts, torch.Tensor) else torch.as_tensor(np.asarray(fts))
    if ft.dim() != 4:
        raise ValueError(f"{who}: fts must be (views, C, H, W): one feature map per camera")
    image_frame(ft.shape[2], ft.shape[3], None, who)
    return ft


def lift_features_many(fts_list, meshes, cameras_list, pix2face_list=None, route="auto", return_counts=False, device=None, focal_length=1.0):
    """get_features_per_vertex for a ragged list of meshes: fts_list[b] (views_b, C, H, W), meshes[b] a mesh object or a (verts, faces)
    pair, cameras_list[b] = (R, T), pix2face_list[b] optional.  On the device route the whole list is two device calls, and the
    operands are checked by MatchEngine.lift_features alone.
    Returns the list of (n_b, C) fp32 tensors (with return_counts: and the list of (n_b,) int32 numbers of views that see a vertex)."""
    who = "lift_features_many"
    Bn = len(meshes)
    if Bn == 0 or len(fts_list) != Bn or len(cameras_list) != Bn or (pix2face_list is not None and len(pix2face_list) != Bn):
        raise ValueError(f"{who}: one stack of maps, one mesh and one (R, T) pair per mesh")
    pairs = [mesh_arrays(m) for m in meshes]
    maps = [_as_maps(ft, f"{who}: mesh {b}") for b, ft in enumerate(fts_list)]
    picked = _routes.pick_host(route, all(AUTO_DEVICE[_layout(ft)] for ft in maps))      # "auto" left: torch where the maps lie
    if picked == "device":
        out = _routes.engine_or_none().lift_features(maps, [p[0] for p in pairs], [p[1] for p in pairs], cameras_list, pix2face_list=pix2face_list,
                                      return_counts=return_counts, focal_length=focal_length)
        feats, cnts = out if return_counts else (out, None)
    else:
        feats, cnts = [], []
        for b in range(Bn):
            tag = f"{who}: mesh {b}"
            V, F = lift_mesh(*pairs[b], tag)
            R, T = lift_cameras(cameras_list[b], tag)
            if maps[b].shape[0] != R.shape[0]:
                raise ValueError(f"{tag}: fts must be ({R.shape[0]}, C, H, W): one feature map per camera")
            H, W = maps[b].shape[2:]
            if pix2face_list is None or pix2face_list[b] is None:
                owner = torch.from_numpy(np.stack([host_raster(V, F, R[v], T[v], H, W, focal_length) for v in range(R.shape[0])]))
            else:
                owner = lift_pix2face(pix2face_list[b], R.shape[0], len(F), tag)
            where = torch.device("cpu") if picked == "host" else maps[b].device
            verts = pairs[b][0] if isinstance(pairs[b][0], torch.Tensor) else torch.as_tensor(np.asarray(pairs[b][0]))
            f, c = _torch_lift(maps[b], verts, torch.from_numpy(F), torch.from_numpy(R), torch.from_numpy(T), owner, focal_length, where)
            feats.append(f), cnts.append(c)
    if device is not None:
        feats, cnts = [f.to(device) for f in feats], None if cnts is None else [c.to(device) for c in cnts]
    return (feats, cnts) if return_counts else feats


def rasterize_visibility(mesh_simp, cameras, H, W, route="auto", focal_length=1.0):
    """The raster alone, for one mesh: (pix2face (views, H, W) int32, visible (views, n) bool -- the vertices of the faces that own a
    pixel, kept where they project strictly inside the frame).  route 'host': float64 NumPy; 'device': dm_raster_pix2face; 'auto': the
    device when a GPU is present."""
    who = "rasterize_visibility"
    H, W = image_frame(H, W, None, who)
    V, F = lift_mesh(*mesh_arrays(mesh_simp), who)
    R, T = lift_cameras(cameras, who)
    if _routes.pick_host(route) == "device":
        p2f, vis = _routes.engine_or_none().raster_visibility([V], [F], [(R, T)], H, W, focal_length)
        return p2f[0], vis[0]
    p2f = np.stack([host_raster(V, F, R[v], T[v], H, W, focal_length) for v in range(R.shape[0])])
    vis = np.zeros((R.shape[0], V.shape[0]), bool)
    for v in range(R.shape[0]):
        Xv = V @ R[v] + T[v]
        with np.errstate(divide="ignore", invalid="ignore"):
            x, y = focal_length * Xv[:, 0] / Xv[:, 2], focal_length * Xv[:, 1] / Xv[:, 2]
        own = np.unique(F[np.unique(p2f[v][p2f[v] >= 0])])
        vis[v, own] = (x[own] > -1) & (x[own] < 1) & (y[own] > -1) & (y[own] < 1)
    return torch.from_numpy(p2f), torch.from_numpy(vis)


def get_features_per_vertex(device, extractor, mesh, mesh_simp, num_views, ft_dim=768, H=512, W=512, cameras=None, center=torch.zeros((1, 3)),
                            dummy_testing=False, render_dir=None, fts=None, use_lr_features=False, *, pix2face=None, route="auto"):
    """The reference's get_features_per_vertex (projection.py:27-130).  mesh_simp: the simplified mesh (verts_list()[0] / faces_list()[0],
    or a (verts, faces) pair).  Returns ft_per_vertex (V, C) fp32 on `device`: the mean of the bilinear samples over the views that see
    a vertex, zeros where no view does.  No normalisation is applied.
    With fts (views, C, H, W) given, cameras = (R (views,3,3), T (views,3)) are those the maps were rendered with; extractor, mesh (the
    raw mesh), num_views, center and use_lr_features are not read, and the width and the size -- of the maps and of the raster alike --
    are those of fts (ft_dim, H and W are not read beyond H == W).
    With fts=None and a callable extractor the function does what the reference does: `mesh` (raw, textured) is rendered at H x W
    (render.batch_render; cameras=None generates them from num_views and center), extractor(batched_renderings[idx][..., :3]) gives
    (ft_hr, ft_lr) per view, (1, C, h, w) each, of which use_lr_features picks one; mesh_simp is rasterised with the same cameras at the
    maps' size and the maps are lifted.  render_dir is not read.  pix2face: see the top of this file."""
    who = "get_features_per_vertex"
    if dummy_testing:
        raise NotImplementedError(f"{who}: dummy_testing is not built")
    if fts is None:
        if not callable(extractor):
            raise NotImplementedError(f"{who}: the 2D backbone is outside this package: pass the per-view feature maps as fts=, or an "
                                      "extractor= that maps a rendered (H, W, 3) view to (ft_hr, ft_lr)")
        from .render import batch_render
        renders, camera, _, _, _ = batch_render(device, mesh, num_views, H, W, cameras, center, route=route)
        cameras = (camera.R, camera.T)
        maps = [extractor(renders[idx][..., :3])[1 if use_lr_features else 0] for idx in range(len(renders))]
        fts = torch.cat([ft if ft.dim() == 4 else ft[None] for ft in maps])
    image_frame(H, W, None, who)
    return lift_features_many([fts], [mesh_simp], [cameras], None if pix2face is None else [pix2face], route=route, device=device)[0]

"""
Float64 NumPy restatement of multi-view feature lifting ('Multi-view feature lifting'): cameras, the raster rule,
visible vertex sets, bilinear sampling and the mean over views.  Written from the definitions, one face at a time over the WHOLE image
(no bounding boxes), so that it shares no shortcut with the kernels it checks.

Cameras are pytorch3d's row-vector convention X_view = X_world R + T, focal length f, NDC with +x left and +y up: x = f X / Z, y = f Y / Z.
Pixel centres: x_c = 1 - (2c + 1) / W, y_r = 1 - (2r + 1) / H.

A pixel is AMBIGUOUS when a face that is not skipped has |min barycentric| <= AMBIGUOUS at its centre, or when its two nearest depths
differ by <= AMBIGUOUS relative: the float64 evaluation order matters at 1e-15 and the fp32 depth key at 6e-8, 1e-5 lies well above both.
"""
import numpy as np

Z_MIN = 1e-6
AREA_MIN = 1e-8
AMBIGUOUS = 1e-5


# ------------------------------------------------------------------------------------------------------------------ cameras
def _unit(v):
    return v / np.linalg.norm(v)


def look_at(eye, at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """(R (3,3), T (3)) of a camera at `eye` that looks at `at`: the columns of R are the camera's x (left), y (up), z (forward) axes in
    world coordinates, T = -eye R, so that X_view = X_world R + T"""
    eye, at, up = (np.asarray(a, np.float64) for a in (eye, at, up))
    z = _unit(at - eye)
    x = _unit(np.cross(up, z))
    y = _unit(np.cross(z, x))
    R = np.stack((x, y, z), axis=1)
    return R, -eye @ R


def orbit(dist, elev_deg, azim_deg, at=(0.0, 0.0, 0.0)):
    """look_at from the point at distance `dist`, elevation and azimuth in degrees (y up, azimuth 0 on +z)"""
    e, a = np.deg2rad(elev_deg), np.deg2rad(azim_deg)
    eye = np.asarray(at, np.float64) + dist * np.array([np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)])
    return look_at(eye, at)


def project(V, R, T, focal=1.0):
    """x, y, Z (n each) of the vertices V (n,3)"""
    Xv = np.asarray(V, np.float64) @ np.asarray(R, np.float64) + np.asarray(T, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return focal * Xv[:, 0] / Xv[:, 2], focal * Xv[:, 1] / Xv[:, 2], Xv[:, 2]


def in_frame(x, y):
    return (x > -1) & (x < 1) & (y > -1) & (y < 1)


# ------------------------------------------------------------------------------------------------------------------ raster
def skipped(F, x, y, Z):
    """(mask of the faces the raster skips, signed areas)"""
    x0, x1, x2 = (x[F[:, k]] for k in range(3))
    y0, y1, y2 = (y[F[:, k]] for k in range(3))
    with np.errstate(invalid="ignore"):
        area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
    bad = (Z[F] <= Z_MIN).any(1) | ~np.isfinite(x[F]).all(1) | ~np.isfinite(y[F]).all(1) | ~(np.abs(area) > AREA_MIN)
    return bad, area


def raster(V, F, R, T, H, W, focal=1.0):
    """pix2face (H,W) int32, ambiguous (H,W) bool, runner_up (H,W) int32: the owner of each pixel, whether it is ambiguous, and the owner
    an ambiguous pixel would have had with every near-edge coverage flipped (or, for near-equal depths, the second-nearest face)"""
    if H != W:
        raise ValueError("square images only")
    F = np.asarray(F, np.int64)
    x, y, Z = project(V, R, T, focal)
    bad, area = skipped(F, x, y, Z)
    px = (1.0 - (2.0 * np.arange(W) + 1.0) / W)[None, :]
    py = (1.0 - (2.0 * np.arange(H) + 1.0) / H)[:, None]
    inf = np.float32(np.inf)
    best = np.full((H, W), inf, np.float32)      # the comparison runs on the fp32-rounded depth: what a packed key holds
    owner = np.full((H, W), -1, np.int32)
    z1 = np.full((H, W), np.inf)                 # the two nearest float64 depths
    z2 = np.full((H, W), np.inf)
    nearest = np.full((H, W), -1, np.int32)
    second = np.full((H, W), -1, np.int32)
    alt_best = np.full((H, W), inf, np.float32)
    alt = np.full((H, W), -1, np.int32)
    edge = np.zeros((H, W), bool)
    for f in np.flatnonzero(~bad):
        i0, i1, i2 = F[f]
        w0 = (px - x[i1]) * (y[i2] - y[i1]) - (py - y[i1]) * (x[i2] - x[i1])
        w1 = (px - x[i2]) * (y[i0] - y[i2]) - (py - y[i2]) * (x[i0] - x[i2])
        w2 = (px - x[i0]) * (y[i1] - y[i0]) - (py - y[i0]) * (x[i1] - x[i0])
        b0, b1, b2 = w0 / area[f], w1 / area[f], w2 / area[f]
        bmin = np.minimum(b0, np.minimum(b1, b2))
        inside = bmin > 0
        near = np.abs(bmin) <= AMBIGUOUS
        edge |= near
        with np.errstate(divide="ignore", invalid="ignore"):
            z = 1.0 / (b0 / Z[i0] + b1 / Z[i1] + b2 / Z[i2])
        z32 = z.astype(np.float32)
        take = inside & (z32 < best)             # faces come in ascending index: a tie keeps the lower one
        best[take], owner[take] = z32[take], f
        inside_alt = inside ^ near
        take = inside_alt & (z32 < alt_best) & (z32 > 0)
        alt_best[take], alt[take] = z32[take], f
        first = inside & (z < z1)
        nxt = inside & ~first & (z < z2)
        z2[first], second[first] = z1[first], nearest[first]
        z1[first], nearest[first] = z[first], f
        z2[nxt], second[nxt] = z[nxt], f
    with np.errstate(invalid="ignore"):
        close = np.isfinite(z2) & (np.abs(z2 - z1) <= AMBIGUOUS * np.abs(z1))
    ambiguous = edge | close
    runner = np.where(edge, alt, np.where(close, second, owner)).astype(np.int32)
    return owner, ambiguous, runner


def visible_vertices(pix2face, F, x, y):
    """projection.py:94-101: the vertices of the faces that own a pixel, kept where the projection lies strictly inside the frame"""
    faces = np.unique(pix2face[pix2face >= 0])
    verts = np.unique(np.asarray(F)[faces]) if faces.size else np.zeros(0, np.int64)
    return verts[in_frame(x[verts], y[verts])]


# ------------------------------------------------------------------------------------------------------------------ sampling
def sample(ft, x, y):
    """grid_sample(ft (C,H,W), grid = -(x, y), bilinear, zero padding, align_corners=True) at m points -> (m, C) float64"""
    ft = np.asarray(ft, np.float64)
    _, H, W = ft.shape
    ix, iy = (-x + 1.0) / 2.0 * (W - 1), (-y + 1.0) / 2.0 * (H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    tx, ty = ix - x0, iy - y0
    out = np.zeros((len(x), ft.shape[0]))
    for dx, dy, w in ((0, 0, (1 - tx) * (1 - ty)), (1, 0, tx * (1 - ty)), (0, 1, (1 - tx) * ty), (1, 1, tx * ty)):
        xx, yy = x0 + dx, y0 + dy
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        out[ok] += w[ok, None] * ft[:, yy[ok], xx[ok]].T
    return out


def lift(fts, V, F, R, T, pix2face=None, focal=1.0):
    """The whole stage for one mesh: fts (views,C,H,W), cameras R (views,3,3), T (views,3).  Returns a dict: features (n,C) float64,
    count (n) int, pix2face (views,H,W), ambiguous (views,H,W), runner_up (views,H,W), visible (list of index arrays per view)."""
    fts = np.asarray(fts)
    views, C, H, W = fts.shape
    n = len(V)
    total, count = np.zeros((n, C)), np.zeros(n, np.int64)
    p2f, amb, run, vis = [], [], [], []
    for v in range(views):
        x, y, _ = project(V, R[v], T[v], focal)
        if pix2face is None:
            o, a, r = raster(V, F, R[v], T[v], H, W, focal)
        else:
            o = np.asarray(pix2face[v]).reshape(H, W)
            a, r = np.zeros((H, W), bool), o
        keep = visible_vertices(o, F, x, y)
        total[keep] += sample(fts[v], x[keep], y[keep])
        count[keep] += 1
        p2f.append(o), amb.append(a), run.append(r), vis.append(keep)
    seen = count > 0
    total[seen] /= count[seen, None]
    return dict(features=total, count=count, pix2face=np.stack(p2f).astype(np.int32), ambiguous=np.stack(amb), runner_up=np.stack(run).astype(np.int32),
                visible=vis)

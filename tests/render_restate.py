"""
Float64 NumPy restatement of textured-mesh rendering ('Textured-mesh rendering'; the definition at the top of
densematcher_amd/render.py): vertex normals, perspective-corrected barycentrics, texels, point-light Phong and the hard blend.  Written
from the definition, one face at a time over the WHOLE image (no boxes), normals from a plain loop over the faces, the texture taps
written out: it shares no code with the package.  The raster (cameras, pixel centres, skipped faces, ownership) and its `ambiguous`
mask are those of tests/lift_restate.py.

`real`: the dtype of interpolation, taps and lighting.  np.float64 is the restatement; np.float32 is the second evaluation that
tests/render_checks.py measures the fp32 floor with (the barycentrics stay float64 either way: the kernel's split).
"""
import numpy as np

import lift_restate as rs

EPS = 1e-6
AMBIENT, DIFFUSE, SPECULAR, BACKGROUND, SHININESS = (0.6, 0.6, 0.6), (0.4, 0.4, 0.5), (0.01, 0.01, 0.01), (1.0, 1.0, 1.0), 64.0


def vertex_normals(V, F):
    """the sum over the incident faces, in ascending face order, of cross(v1 - v0, v2 - v0); n / max(|n|, 1e-6)"""
    V = np.asarray(V, np.float64)
    s = np.zeros_like(V)
    for f in range(len(F)):
        i0, i1, i2 = F[f]
        a, b = V[i1] - V[i0], V[i2] - V[i0]
        cr = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        s[i0] += cr
        s[i1] += cr
        s[i2] += cr
    for i in range(len(V)):
        s[i] = s[i] / max(np.sqrt(s[i, 0] ** 2 + s[i, 1] ** 2 + s[i, 2] ** 2), EPS)
    return s


def unit(a):
    """a / max(|a|, 1e-6) along the last axis"""
    return a / np.maximum(np.sqrt((a * a).sum(-1, keepdims=True)), a.dtype.type(EPS))


def sample_map(tmap, u, v):
    """grid_sample(flip(map, rows), 2 uv - 1, bilinear, align_corners=True, border): x = u (Wt - 1), y = (1 - v)(Ht - 1), clamped to the
    map; the four taps nw, ne, sw, se written out.  tmap (Ht, Wt, 3), u, v (k) in tmap's dtype -> (k, 3)"""
    Ht, Wt = tmap.shape[:2]
    one = tmap.dtype.type(1)
    x = np.minimum(np.maximum(u * tmap.dtype.type(Wt - 1), 0), tmap.dtype.type(Wt - 1))
    y = np.minimum(np.maximum((one - v) * tmap.dtype.type(Ht - 1), 0), tmap.dtype.type(Ht - 1))
    out = np.zeros((len(u), 3), tmap.dtype)
    for k in range(len(u)):
        xa, ya = int(np.floor(x[k])), int(np.floor(y[k]))
        xb, yb = min(xa + 1, Wt - 1), min(ya + 1, Ht - 1)
        tx, ty = x[k] - tmap.dtype.type(xa), y[k] - tmap.dtype.type(ya)
        out[k] = ((one - tx) * (one - ty) * tmap[ya, xa] + tx * (one - ty) * tmap[ya, xb] + (one - tx) * ty * tmap[yb, xa] + tx * ty * tmap[yb, xb])
    return out


def render_view(V, F, R, T, H, W, texture=None, normals=None, light=None, ambient=AMBIENT, diffuse=DIFFUSE, specular=SPECULAR,
                shininess=SHININESS, background=BACKGROUND, focal=1.0, real=np.float64, raster=None):
    """One view.  texture: None, ("vertex", colours (n, 3)) or ("uv", map (Ht, Wt, 3), verts_uvs (n_uv, 2), faces_uvs (m, 3)).
    Returns rgba (H, W, 4) in `real`, zbuf (H, W) float32, pix2face (H, W) int32, ambiguous (H, W) bool."""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    R, T = np.asarray(R, np.float64), np.asarray(T, np.float64)
    owner, ambiguous, _ = rs.raster(V, F, R, T, H, W, focal) if raster is None else raster
    nrm = vertex_normals(V, F) if normals is None else np.asarray(normals, np.float64)
    x, y, Z = rs.project(V, R, T, focal)
    px = (1.0 - (2.0 * np.arange(W) + 1.0) / W)[None, :]
    py = (1.0 - (2.0 * np.arange(H) + 1.0) / H)[:, None]
    centre = -T @ R.T                                        # C = -T R^T
    L = centre if light is None else np.asarray(light, np.float64)
    Vr, Nr, Cr, Lr = V.astype(real), nrm.astype(real), centre.astype(real), L.astype(real)
    amb, dif, spc = (np.asarray(a, np.float32).astype(real) for a in (ambient, diffuse, specular))
    rgba = np.zeros((H, W, 4), real)
    rgba[..., :3] = np.asarray(background, np.float32).astype(real)
    zbuf = np.full((H, W), -1.0, np.float32)
    for f in np.unique(owner[owner >= 0]):
        i = F[f]
        area = (x[i[2]] - x[i[0]]) * (y[i[1]] - y[i[0]]) - (y[i[2]] - y[i[0]]) * (x[i[1]] - x[i[0]])
        b0 = ((px - x[i[1]]) * (y[i[2]] - y[i[1]]) - (py - y[i[1]]) * (x[i[2]] - x[i[1]])) / area
        b1 = ((px - x[i[2]]) * (y[i[0]] - y[i[2]]) - (py - y[i[2]]) * (x[i[0]] - x[i[2]])) / area
        b2 = ((px - x[i[0]]) * (y[i[1]] - y[i[0]]) - (py - y[i[0]]) * (x[i[1]] - x[i[0]])) / area
        own = owner == f
        q = np.stack((b0[own] / Z[i[0]], b1[own] / Z[i[1]], b2[own] / Z[i[2]]), axis=1)
        zbuf[own] = (1.0 / q.sum(1)).astype(np.float32)
        c = (q / q.sum(1, keepdims=True)).astype(real)       # perspective-corrected, float64; `real` from here on
        mix = lambda a: c[:, 0:1] * a[0] + c[:, 1:2] * a[1] + c[:, 2:3] * a[2]
        p, n = mix(Vr[i]), unit(mix(Nr[i]))
        if texture is None:
            texel = np.ones((len(p), 3), real)
        elif texture[0] == "vertex":
            texel = mix(np.asarray(texture[1], np.float32).astype(real)[i])
        else:
            uv = mix(np.asarray(texture[2], np.float32).astype(real)[np.asarray(texture[3])[f]])
            texel = sample_map(np.asarray(texture[1], np.float32).astype(real), uv[:, 0], uv[:, 1])
        l, e = unit(Lr - p), unit(Cr - p)
        cs = (n * l).sum(1, keepdims=True)
        r = -l + 2 * cs * n
        alpha = np.maximum((e * r).sum(1, keepdims=True), 0) * (cs > 0)
        rgb = (amb + dif * np.maximum(cs, 0)) * texel + spc * alpha ** real(shininess)
        rgba[own] = np.concatenate((rgb, np.ones((len(p), 1), real)), axis=1)
    return rgba, zbuf, owner, ambiguous


def render(V, F, R, T, H, W, texture=None, real=np.float64, rasters=None, **kw):
    """every view of one mesh: dict of rgba (views, H, W, 4), zbuf, pix2face, ambiguous; rasters: optional list of rs.raster results"""
    light = kw.pop("light", None)
    views = [render_view(V, F, R[v], T[v], H, W, texture, light=None if light is None else light[v], real=real,
                         raster=None if rasters is None else rasters[v], **kw) for v in range(len(R))]
    return dict(rgba=np.stack([v[0] for v in views]), zbuf=np.stack([v[1] for v in views]), pix2face=np.stack([v[2] for v in views]),
                ambiguous=np.stack([v[3] for v in views]))

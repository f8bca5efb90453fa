"""Shared by the rendering tests (CPU and GPU): the geometry cases, the textures, one restatement per (case, size, texture) -- computed
once, shared, never modified -- and the fp32 floor that sets the tolerance.

Geometry: the four meshes and cameras of tests/golden/fx_lift.npz (lift_checks.case / cameras: about 160 vertices, with the degenerate
face, the face behind the camera and the object leaving the frame) and one finer 'raw' mesh "t", synth.torus_mesh(24, 12, perturb > 0),
whose faces are smaller than a pixel at 16 x 16; each at 16, 32 and 33.
Textures: none, vertex colours, an 8 x 8 UV map and a non-square 5 x 7 one, with UVs that reach 0 and 1 and lie slightly outside [0, 1]
(border clamp) and faces_uvs that differ from faces (a seam).

Tolerance: the restatement is evaluated a second time with interpolation, taps and lighting in fp32 (barycentrics float64: the kernel's
split); f32_floor = max |fp32 - f64| / max |f64| over the unambiguous covered pixels; the bound is lift_checks.bound: (4 f32_floor +
2^-23) max |ref|.  The alpha^64 specular term is why the floor is measured and not guessed."""
import functools

import numpy as np

import lift_checks as lc
import lift_restate as rs
import render_restate as rr
from densematcher_amd import synth

CASES = lc.CASES + ("t",)
SIZES = (16, 32, 33)
KINDS = ("none", "vertex", "uv8", "uv57")
AMBIGUOUS_CAP = 0.01


@functools.lru_cache(maxsize=None)
def geometry(c, H=None):
    """(verts float64, faces int64, R, T) of case c for an H x H image"""
    if c == "t":
        V, F = synth.torus_mesh(24, 12, perturb=0.3, seed=4)
        cams = [rs.orbit(3.4, e, a) for e, a in ((20.0, 10.0), (-35.0, 130.0), (65.0, 250.0))]
        out = (V, F, np.stack([k[0] for k in cams]), np.stack([k[1] for k in cams]))
    else:
        d = lc.case(c)
        out = (d["verts"].astype(np.float64), d["faces"]) + tuple(lc.cameras(c, H))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def texture(c, kind):
    """the texture of case c: None, ("vertex", colours) or ("uv", map, verts_uvs, faces_uvs), fp32 / int64 NumPy arrays"""
    V, F = geometry(c)[:2]
    n = len(V)
    rng = np.random.default_rng(sum(map(ord, c + kind)))
    if kind == "none":
        return None
    if kind == "vertex":
        return ("vertex", rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32))
    Ht, Wt = (8, 8) if kind == "uv8" else (5, 7)
    tmap = rng.uniform(0.0, 1.0, (Ht, Wt, 3)).astype(np.float32)
    uv = rng.uniform(-0.08, 1.08, (n, 2))
    uv[0::7], uv[1::7, 0], uv[2::7, 1] = (0.0, 1.0), 1.0, 0.0                 # values that reach 0 and 1 exactly
    seam = np.arange(0, len(F), 5)                                            # every fifth face has uv rows of its own
    fuv = F.copy()
    fuv[seam] = n + np.arange(3 * len(seam)).reshape(-1, 3)
    uv = np.concatenate((uv, rng.uniform(-0.08, 1.08, (3 * len(seam), 2))))
    assert not np.array_equal(fuv, F) and uv.min() < 0 and uv.max() > 1
    return ("uv", tmap, uv.astype(np.float32), fuv)


@functools.lru_cache(maxsize=None)
def rasters(c, H):
    V, F, R, T = geometry(c, H)
    return [rs.raster(V, F, R[v], T[v], H, H) for v in range(len(R))]


@functools.lru_cache(maxsize=None)
def restated(c, H, kind):
    """the restatement of (case, size, texture): rgba (float64), zbuf, pix2face, ambiguous, and f32_floor"""
    V, F, R, T = geometry(c, H)
    res = rr.render(V, F, R, T, H, H, texture(c, kind), rasters=rasters(c, H))
    low = rr.render(V, F, R, T, H, H, texture(c, kind), real=np.float32, rasters=rasters(c, H))
    keep = (res["pix2face"] >= 0) & ~res["ambiguous"]
    res["f32_floor"] = float(np.abs(low["rgba"].astype(np.float64) - res["rgba"])[keep].max() / np.abs(res["rgba"][keep]).max())
    res["keep"] = keep
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def ambiguity(c, H):
    """(ambiguous pixels, covered pixels) of (case, size)"""
    r = rasters(c, H)
    return int(sum(a[1].sum() for a in r)), int(sum((a[0] >= 0).sum() for a in r))


def compare(got_rgba, got_zbuf, got_p2f, res, tag):
    """a render (NumPy arrays; pix2face (views, H, W)) against the restatement `res`: pix2face, covered pixels and the fp32 zbuf equal
    outside the ambiguous pixels, alpha equal there, RGBA within the bound on the unambiguous covered pixels and exact background"""
    amb, keep = res["ambiguous"], res["keep"]
    got_rgba, got_zbuf, got_p2f = (np.asarray(a) for a in (got_rgba, got_zbuf, got_p2f))
    assert got_rgba.shape == res["rgba"].shape and got_p2f.shape == res["pix2face"].shape, tag
    assert ((got_p2f == res["pix2face"]) | amb).all(), tag
    assert ((got_zbuf == res["zbuf"]) | amb).all(), tag
    assert ((got_rgba[..., 3] == res["rgba"][..., 3]) | amb).all(), tag
    bg = (res["pix2face"] < 0) & ~amb
    assert np.array_equal(got_rgba[bg].astype(np.float64), res["rgba"][bg]), tag
    return lc.check(got_rgba[keep], res["rgba"][keep], res["f32_floor"], tag)

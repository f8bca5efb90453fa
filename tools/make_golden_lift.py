#!/usr/bin/env python
"""
Multi-view feature lifting fixture, produced by RUNNING THE REFERENCE's get_features_per_vertex(fts=...) on the CPU in float32.

    python tools/make_golden_lift.py <reference checkout>        -> tests/golden/fx_lift.npz

The reference's densematcher/projection.py is imported as tools/make_golden_dnet_layers.py imports layers.py: an empty package module
named densematcher whose __path__ is the reference's directory, and stub modules for what projection.py imports and this machine lacks
(the pytorch3d names, torchvision.utils).  Two stubs carry meaning:
  densematcher.render.batch_render   returns the pix2face of tests/lift_restate.py (views, H, W, 1) and a camera object
  the camera object                  camera[i].get_full_projection_transform().transform_points(p) = (X/Z, Y/Z, Z) of p R_i + T_i, in p's dtype

WHAT THE FIXTURE PINS to the reference's own code: which faces are visible given a pix2face, their vertices, the frame test
-1 < x, y < 1, grid_sample(align_corners=True) at -(x, y), the sum over views and the division by the count.
WHAT IT DOES NOT PIN: the raster rule (which face owns a pixel) and the camera formula.  Both are this package's restatement of
pytorch3d's PerspectiveCameras defaults and MeshRasterizer(blur_radius=0, faces_per_pixel=1); pytorch3d has no supported build on ROCm.  A
caller who has pytorch3d passes its pix2face= to get_features_per_vertex.

Cases, all on synth.torus_mesh, centred, the cameras at distance 2 x the largest coordinate looking at the origin (render.py:23-26):
  a  16 x 10 torus, perturb 0.12, seed 11 (160 vertices); 32 x 32; azimuth 0 / 120 / 240 at elevation 0 and azimuth 37 at elevation 55;
     C = 5, fp32 maps
  b  the same mesh; 33 x 33; two views on one side; C = 70, fp16 maps; asserted: at least 10 % of the vertices are seen by no view
  c  12 x 8 torus; 24 x 24; three views, the last translated so that the object leaves the frame; C = 3; asserted: in that view at
     least 10 % of the vertices of visible faces fail the frame test and no kept vertex lies within 1e-4 of the border
  d  a, plus one degenerate face, one face behind camera 0 and one triangle whose corner projects onto the last texel column of view 0
     (ix within 1e-3 below W - 1)
Asserted per case: ambiguous pixels (tests/lift_restate.py) are at most 1 % of the covered ones, and every visible set is unchanged
when each ambiguous pixel is handed to its runner-up; a view that fails the latter has its azimuth stepped by 1 degree until it holds
(the angles used are stored).  Case c also carries cameras for 33 x 33 (c_R33, c_T33, c_steps33): at an odd size the centre row and column of
pixels of its view 0 lie exactly on edges of the unperturbed torus (20 of 418 covered pixels ambiguous).  y = 0 and x = 0 are mirror planes
of the mesh; the first holds every camera of elevation 0 and the second every camera of azimuth 0, so stepping one angle alone never
helps: that view's azimuth AND elevation are stepped together by 1 degree until at most 1 % of its covered pixels are ambiguous and its
visible set is stable (c_steps33: the steps taken per view).
Stored per case <k>: <k>_verts, <k>_faces, <k>_R, <k>_T, <k>_azim, <k>_fts, <k>_pix2face, <k>_ambiguous, <k>_visible (views, n) bool,
<k>_count, <k>_y_ref32 (the reference's output), <k>_f32_floor = max |y_ref32 - y64| / max |y64| with y64 from tests/lift_restate.py.
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "fx_lift.npz")

_STATE = {}


class _Transform:
    def __init__(self, R, T):
        self.R, self.T = R, T

    def transform_points(self, pts):
        v = pts @ self.R.to(pts.dtype) + self.T.to(pts.dtype)
        return torch.cat((v[:, :2] / v[:, 2:3], v[:, 2:3]), dim=1)


class _Cameras:
    def __init__(self, R, T):
        self.R, self.T = R, T

    def __getitem__(self, i):
        return _Cameras(self.R[i:i + 1], self.T[i:i + 1])

    def get_full_projection_transform(self):
        return _Transform(self.R[0], self.T[0])


class MeshStub:
    """what the reference reads of a pytorch3d Meshes"""

    def __init__(self, verts, faces):
        self.v, self.f, self.device = verts, faces, verts.device

    def verts_list(self):
        return [self.v]

    def faces_list(self):
        return [self.f]

    def to(self, device):
        return self


def _batch_render(device, mesh, num_views, H, W, cameras, center):
    R, T = cameras
    p2f = torch.from_numpy(_STATE["pix2face"].astype(np.int64))[..., None]
    return torch.zeros((len(R), H, W, 4)), _Cameras(R, T), None, p2f, center


def import_reference(checkout, more=()):
    root = os.path.join(checkout, "densematcher")
    if not os.path.isdir(root):
        root = checkout
    for name in ("pytorch3d", "pytorch3d.ops", "pytorch3d.structures", "pytorch3d.structures.meshes", "torchvision", "torchvision.utils",
                 "potpourri3d", "robust_laplacian") + tuple(more):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["pytorch3d.ops"].__dict__.setdefault("ball_query", None)
    sys.modules["pytorch3d.structures.meshes"].__dict__.setdefault("Meshes", MeshStub)
    sys.modules["torchvision.utils"].__dict__.setdefault("make_grid", None)
    pkg = types.ModuleType("densematcher")
    pkg.__path__ = [root]
    sys.modules["densematcher"] = pkg
    render = types.ModuleType("densematcher.render")
    render.batch_render = _batch_render
    sys.modules["densematcher.render"] = render
    import densematcher.projection as ref_projection
    return ref_projection


# ------------------------------------------------------------------------------------------------------------------ cases
def centred(V):
    return V - 0.5 * (V.max(0) + V.min(0))


def case_geometry(case):
    """(verts float64, faces int64, [(elevation, azimuth)], shift of the last view in view space or None, H, C, map dtype)"""
    from densematcher_amd import synth
    if case == "c":
        V, F = synth.torus_mesh(12, 8)
        return centred(np.asarray(V, np.float64)), np.asarray(F, np.int64), [(0.0, 0.0), (20.0, 120.0), (-15.0, 240.0)], 2.4, 24, 3, np.float32
    V, F = synth.torus_mesh(16, 10, perturb=0.12, seed=11)
    V, F = centred(np.asarray(V, np.float64)), np.asarray(F, np.int64)
    if case == "b":
        return V, F, [(0.0, 0.0), (10.0, 25.0)], None, 33, 70, np.float16
    return V, F, [(0.0, 0.0), (0.0, 120.0), (0.0, 240.0), (55.0, 37.0)], None, 32, 5, np.float32


def hostile_additions(V, F, R0, T0, dist, W):
    """case d: three vertices + a face behind camera 0, a degenerate face, and a triangle whose first corner projects onto the last texel
    column of view 0"""
    world = lambda pv: (np.asarray(pv, np.float64) - T0) @ R0.T
    n = len(V)
    behind = [world((0.1, 0.1, -0.5)), world((0.3, 0.1, -0.5)), world((0.1, 0.3, -0.6))]
    x_edge = -1.0 + 2.0 * 5e-4 / (W - 1)
    rim = [world((x_edge * dist, 0.1 * dist, dist)), world((-0.8 * dist, 0.0, dist)), world((-0.8 * dist, 0.25 * dist, dist))]
    V = np.concatenate((V, np.stack(behind + rim)))
    F = np.concatenate((F, np.array([[n, n + 1, n + 2], [10, 10, 25], [n + 3, n + 4, n + 5]], np.int64)))
    return V, F, dict(behind=len(F) - 3, degenerate=len(F) - 2, rim=len(F) - 1, rim_vertex=n + 3)


def visible_masks(rs, res, n):
    m = np.zeros((len(res["visible"]), n), bool)
    for v, idx in enumerate(res["visible"]):
        m[v, idx] = True
    return m


def stepped_cameras(rs, case, V, F, angles, shift, dist, H, share=None, step_elevation=False):
    """(R, T, azimuths used) of the views at size H: a view whose visible set changes when its ambiguous pixels go to their runner-up --
    or, with `share`, whose ambiguous pixels exceed that share of its covered ones -- has its azimuth (step_elevation: its azimuth and its
    elevation) stepped by 1 degree until it holds; the number of steps per view is returned"""
    Rs, Ts, used = [], [], []
    for v, (elev, azim) in enumerate(angles):
        for step in range(30):
            R, T = rs.orbit(dist, elev + step, azim + step) if step_elevation else rs.orbit(dist, elev, azim + step)
            if shift is not None and v == len(angles) - 1:
                T = T + np.array([shift, 0.0, 0.0])
            own, amb, run = rs.raster(V, F, R, T, H, H)
            x, y, _ = rs.project(V, R, T)
            same = np.array_equal(rs.visible_vertices(own, F, x, y), rs.visible_vertices(np.where(amb, run, own), F, x, y))
            few = share is None or amb.sum() <= share * (own >= 0).sum()
            if (same and few) or (case == "d" and v == 0):        # (view 0 of case d is tied to the added geometry)
                assert same, "case d view 0: an ambiguous pixel changes the visible set"
                break
            print(f"case {case} view {v} at {H} x {H}: elevation {elev + step if step_elevation else elev}, azimuth {azim + step}: {int(amb.sum())} ambiguous of {int((own >= 0).sum())} covered pixels, "
                  f"visible set {'kept' if same else 'changed'}: stepping")
        else:
            raise AssertionError((case, v))
        Rs.append(R), Ts.append(T), used.append(step if step_elevation else azim + step)
    return np.stack(Rs), np.stack(Ts), np.asarray(used)


def build_case(case, rs):
    V, F, angles, shift, H, C, dt = case_geometry("a" if case == "d" else case)
    dist = 2.0 * np.abs(V).max()
    extra = None
    rng = np.random.default_rng({"a": 1, "b": 2, "c": 3, "d": 4}[case])
    fts = rng.standard_normal((len(angles), C, H, H)).astype(dt)
    if case == "d":
        R0, T0 = rs.orbit(dist, *angles[0])
        V, F, extra = hostile_additions(V, F, R0, T0, dist, H)
    R, T, used = stepped_cameras(rs, case, V, F, angles, shift, dist, H)
    res = rs.lift(fts.astype(np.float64), V, F, R, T)
    covered, amb = int((res["pix2face"] >= 0).sum()), int((res["ambiguous"] & (res["pix2face"] >= 0)).sum())
    print(f"case {case}: {len(V)} vertices, {len(F)} faces, {len(angles)} views of {H} x {H}: {covered} covered pixels, {amb} ambiguous "
          f"({int(res['ambiguous'].sum())} with the background), counts {np.bincount(res['count'])}")
    assert res["ambiguous"].sum() <= 0.01 * covered, (case, int(res["ambiguous"].sum()), covered)
    vis = visible_masks(rs, res, len(V))
    if case == "b":
        unseen = float((res["count"] == 0).mean())
        print(f"case b: {unseen:.3f} of the vertices are seen by no view")
        assert unseen >= 0.10
    if case == "c":
        v = len(angles) - 1
        x, y, _ = rs.project(V, R[v], T[v])
        own = np.unique(F[np.unique(res["pix2face"][v][res["pix2face"][v] >= 0])])
        out = float((~rs.in_frame(x[own], y[own])).mean())
        margin = float(np.min(1.0 - np.maximum(np.abs(x[vis[v]]), np.abs(y[vis[v]]))))
        print(f"case c: view {v}: {out:.3f} of the {len(own)} vertices of visible faces fail the frame test; nearest kept vertex {margin:.3e} from the border")
        assert out >= 0.10 and margin > 1e-4
    if case == "d":
        p0 = res["pix2face"][0]
        assert not (p0 == extra["behind"]).any() and not (res["pix2face"] == extra["degenerate"]).any()
        assert (p0 == extra["rim"]).any() and vis[0, extra["rim_vertex"]]
        x, _, _ = rs.project(V, R[0], T[0])
        ix = (1.0 - x[extra["rim_vertex"]]) / 2.0 * (H - 1)
        print(f"case d: the rim vertex taps at ix = {ix:.6f} of {H - 1}; its face owns {int((p0 == extra['rim']).sum())} pixels")
        assert H - 1 - 1e-3 <= ix < H - 1
    more = {}
    if case == "c":
        # at an odd size the centre row and column of pixels of view 0 lie ON edges of the unperturbed torus: y = 0 and x = 0 are mirror
        # planes of the mesh, the first holds every camera of elevation 0, the second every camera of azimuth 0.  Cameras of their own
        # for 33 x 33, azimuth AND elevation stepped together
        R33, T33, used33 = stepped_cameras(rs, case, V, F, angles, shift, dist, 33, share=0.01, step_elevation=True)
        more = dict(R33=R33, T33=T33, steps33=used33)
    return dict(verts=V, faces=F.astype(np.int32), R=R, T=T, azim=used, fts=fts, **more, pix2face=res["pix2face"], ambiguous=res["ambiguous"],
                visible=vis, count=res["count"].astype(np.int32)), res


def run_reference(ref, c):
    """the reference's get_features_per_vertex on the CPU in float32 with the case's pix2face"""
    _STATE["pix2face"] = c["pix2face"]
    verts, faces = torch.tensor(c["verts"].astype(np.float32)), torch.tensor(c["faces"].astype(np.int64))
    mesh = MeshStub(verts, faces)
    fts = torch.tensor(c["fts"].astype(np.float32))
    cams = (torch.tensor(c["R"].astype(np.float32)), torch.tensor(c["T"].astype(np.float32)))
    H = fts.shape[2]
    with torch.no_grad():
        y = ref.get_features_per_vertex("cpu", None, mesh, mesh, None, ft_dim=fts.shape[1], H=H, W=H, cameras=cams, fts=fts)
    return y.numpy()


def main():
    ref = import_reference(sys.argv[1])
    import lift_restate as rs
    out = {}
    for case in "abcd":
        c, res = build_case(case, rs)
        y = run_reference(ref, c)
        y64 = res["features"]
        assert y.shape == y64.shape and y.dtype == np.float32
        assert np.array_equal((np.abs(y).sum(1) > 0), res["count"] > 0), "the reference fills other vertices than the restatement"
        floor = float(np.abs(y.astype(np.float64) - y64).max() / np.abs(y64).max())
        print(f"case {case}: max |y| = {np.abs(y64).max():.4f}, f32_floor = {floor:.3e}")
        c["y_ref32"], c["f32_floor"] = y, np.array(floor)
        for key, val in c.items():
            out[f"{case}_{key}"] = val
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

"""Shared by the lifting and featurizer tests (CPU and GPU): the fixtures tests/golden/fx_lift.npz (tools/make_golden_lift.py) and
tests/golden/fx_featurizer.npz (tools/make_golden_featurizer.py) -- the reference's own float32 runs --, one float64 restatement per case
(computed once, shared, never modified) and the bound of the layers fixture."""
import functools
import os

import numpy as np
import torch

import lift_restate as rs

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("a", "b", "c", "d")


@functools.lru_cache(maxsize=None)
def golden(name="fx_lift.npz"):
    with np.load(os.path.join(HERE, "golden", name)) as z:
        return {k: z[k] for k in z.files}


def case(c):
    """the arrays of case c as a dict: verts, faces (int64), R, T, fts, pix2face, ambiguous, visible, count, y_ref32, f32_floor"""
    fx = golden()
    d = {k[2:]: v for k, v in fx.items() if k.startswith(c + "_")}
    d["faces"] = d["faces"].astype(np.int64)
    return d


def cameras(c, H=None):
    """(R, T) of case c for a raster of H x H: its own, except case c at 33 x 33, whose view 0 is stepped off the mesh's mirror planes
    (tools/make_golden_lift.py: c_R33, c_T33)"""
    d = case(c)
    return (d["R33"], d["T33"]) if (c, H) == ("c", 33) else (d["R"], d["T"])


@functools.lru_cache(maxsize=None)
def restated(c, H=None):
    """tests/lift_restate.py on case c (at another raster size H: the raster only, on zero maps of one channel, with cameras(c, H))"""
    d = case(c)
    R, T = cameras(c, H)
    fts = d["fts"].astype(np.float64) if H is None else np.zeros((len(R), 1, H, H))
    res = rs.lift(fts, d["verts"], d["faces"], R, T)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def visible_mask(res, n):
    m = np.zeros((len(res["visible"]), n), bool)
    for v, idx in enumerate(res["visible"]):
        m[v, idx] = True
    return m


def bound(floor, ref):
    """(4 f32_floor + 2^-23) max |ref|: the floor is one fp32 evaluation's distance from exact arithmetic, the factor 4 covers another
    evaluation order, 2^-23 the final rounding (tests/dnet_layers_checks.py: check_output)"""
    return (4.0 * float(floor) + 2.0 ** -23) * float(np.abs(ref).max())


def check(got, ref, floor, tag):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err, b = float(np.abs(got - ref).max()), bound(floor, ref)
    print(f"{tag}: max |got - ref| = {err:.3e}, max |ref| = {np.abs(ref).max():.3e}, bound {b:.3e}")
    assert np.all(np.isfinite(got)) and err <= b, (tag, err, b)
    return err


class Mesh:
    """what the package reads of a pytorch3d Meshes"""

    def __init__(self, verts, faces):
        self.v, self.f = verts, faces

    def verts_list(self):
        return [self.v]

    def faces_list(self):
        return [self.f]


# ------------------------------------------------------------------------------------------------------------------ featurizer
def featurizer(device="cpu"):
    from densematcher_amd.model import MeshFeaturizer
    fx = golden("fx_featurizer.npz")
    model = MeshFeaturizer(None, (3, 1), int(fx["blocks"]), int(fx["width"]), num_features=fx["fts"].shape[1])
    names = [str(n) for n in fx["names"]]
    model.load_state_dict({n: torch.from_numpy(fx[f"p{i}"].copy()) for i, n in enumerate(names)}, strict=True)
    return model.to(device).eval(), names


def featurizer_inputs(device="cpu"):
    """(mesh, operators tuple, cameras, fts, pix2face) of the fixture on `device`"""
    fx = golden("fx_featurizer.npz")
    n = fx["verts"].shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    sp = lambda name: torch.sparse_coo_tensor(torch.from_numpy(np.stack((fx[f"{name}_row"], fx[f"{name}_col"])).astype(np.int64)),
                                              torch.from_numpy(fx[f"{name}_val"]), (n, n)).coalesce().to(device)
    mesh = Mesh(t(fx["verts"].astype(np.float32)), t(fx["faces"].astype(np.int64)))
    ops = (None, t(fx["mass"]), None, t(fx["evals"]), t(fx["evecs"]), sp("gradX"), sp("gradY"))
    cams = (t(fx["R"].astype(np.float32)), t(fx["T"].astype(np.float32)))
    return mesh, ops, cams, t(fx["fts"]), t(fx["pix2face"])

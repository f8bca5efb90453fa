#!/usr/bin/env python
"""
MeshFeaturizer fixture, produced by RUNNING THE REFERENCE's MeshFeaturizer.forward on the CPU in float32.

    python tools/make_golden_featurizer.py <reference checkout>        -> tests/golden/fx_featurizer.npz

The reference's densematcher/model.py is imported on top of the stubs of tools/make_golden_lift.py (same pix2face and camera stubs; read
that file's docstring for what they pin and what they do not), plus:
  densematcher.extractor        SDDINOFeatureExtractor = an object with num_patches = 2 (H = W = 32) and featurizer.num_features = 12
  densematcher.functional_map   an empty compute_surface_map (model.py imports the name, forward does not use it)
The reference's forward does not pass ft_dim to get_features_per_vertex (its default is 768, the real backbone's width), so the name
model.py imported is bound to partial(get_features_per_vertex, ft_dim=12).  The per-view maps enter through the `extractor` argument:
the instance's extract_features_2d is replaced by a function that returns the stored maps in order.

The mesh, the cameras and the pix2face are case a of tests/golden/fx_lift.npz; the maps are 4 x 12 x 32 x 32 float32, seeded.  width 32,
2 blocks, k_eig = 16; the operators come from THIS package's host route in float32 (compute_operators(route="host")) and are stored, as
tests/golden/fx_dnet_layers.npz stores them; diffusion times uniform in [0, 0.05).  The module runs seeded, in eval mode.
Stored: names / p<i> (the state_dict in order), verts, faces, R, T, fts, pix2face, mass, evals, evecs, gradX_* / gradY_* (COO), and the
reference's float32 results pos_enc, hks, mv_features, out, out_normalized, each with its floor max |ref32 - x64| / max |x64| against a
float64 restatement (tests/lift_restate.py, tests/dnet_layers_restate.py, the formulas of model.py:155-158): floor_pos, floor_hks, floor_mv,
f32_floor (out), floor_normalized.
"""
import functools
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
OUT = os.path.join(REPO, "tests", "golden", "fx_featurizer.npz")
K_EIG, WIDTH, BLOCKS, C_FT = 16, 32, 2, 12


class _Extractor:
    num_patches = 2
    featurizer = types.SimpleNamespace(num_features=C_FT)

    def __init__(self, *args, **kwargs):
        pass


def main():
    import make_golden_lift as mgl
    ext = types.ModuleType("densematcher.extractor")
    ext.DINOv2FeatureExtractor = ext.DIFTFeatureExtractor = ext.SDDINOFeatureExtractor = _Extractor
    fmap = types.ModuleType("densematcher.functional_map")
    fmap.compute_surface_map = None
    ref_projection = mgl.import_reference(sys.argv[1])
    sys.modules["densematcher.extractor"], sys.modules["densematcher.functional_map"] = ext, fmap
    import densematcher.model as ref_model
    ref_model.get_features_per_vertex = functools.partial(ref_projection.get_features_per_vertex, ft_dim=C_FT)
    import dnet_layers_restate as dl
    import lift_restate as rs
    from densematcher_amd.diffusion_net import geometry as geo

    with np.load(os.path.join(REPO, "tests", "golden", "fx_lift.npz")) as z:
        V, F, R, T, p2f = z["a_verts"], z["a_faces"].astype(np.int64), z["a_R"], z["a_T"], z["a_pix2face"]
    fts = np.random.default_rng(21).standard_normal((len(R), C_FT, 32, 32)).astype(np.float32)
    verts, faces = torch.tensor(V.astype(np.float32)), torch.tensor(F)
    ops = geo.compute_operators(verts, faces, K_EIG, route="host")
    frames, mass, L, evals, evecs, gX, gY = ops
    gX, gY = gX.coalesce(), gY.coalesce()
    assert all(t.dtype == torch.float32 for t in (mass, evals, evecs, gX, gY))

    torch.manual_seed(301)
    model = ref_model.MeshFeaturizer(None, (3, 1), BLOCKS, WIDTH).float().eval()
    assert model.H == 32 and model.diffusion_in_channels == C_FT + 16 + 51
    with torch.no_grad():
        for blk in model.extractor_3d.blocks:
            blk.diffusion.diffusion_time.copy_(0.05 * torch.rand(WIDTH))
    names = list(model.state_dict().keys())
    params = {n: p.detach().clone().numpy() for n, p in model.state_dict().items()}
    it = iter(range(len(fts)))
    model.extract_features_2d = lambda img: (torch.from_numpy(fts[next(it)][None]), None)
    mgl._STATE["pix2face"] = p2f
    mesh = mgl.MeshStub(verts, faces)
    cams = (torch.tensor(R.astype(np.float32)), torch.tensor(T.astype(np.float32)))
    with torch.no_grad():
        outn, out, mv = model(mesh, mesh, (frames, mass, L, evals, evecs, gX, gY), cams, return_mvfeatures=True)

    # ---- float64 restatement of the same
    mv64 = rs.lift(fts.astype(np.float64), V.astype(np.float32).astype(np.float64), F, R.astype(np.float32).astype(np.float64),
                   T.astype(np.float32).astype(np.float64), pix2face=p2f)["features"]
    x = V.astype(np.float32).astype(np.float64) * (np.pi * 6)
    enc = [x]
    for k in range(8):
        enc += [np.sin(x * 2.0 ** k), np.cos(x * 2.0 ** k)]
    pos64 = np.concatenate(enc, axis=1)
    ev, ec, ms = evals.double().numpy(), evecs.double().numpy(), mass.double().numpy()
    scales = np.logspace(-2.0, 0.0, 16)
    hks64 = (ec * ec) @ np.exp(-scales[:, None] * ev[None, :]).T
    x64 = np.concatenate((mv64, pos64, hks64), axis=1)
    cfg = dict(C_in=x64.shape[1], C_out=WIDTH, C_width=WIDTH, N_block=BLOCKS, with_gradient_features=True, with_gradient_rotations=True,
               outputs_at="vertices")
    p3d = {n[len("extractor_3d."):]: v for n, v in params.items() if n.startswith("extractor_3d.")}
    out64, dots = dl.forward(cfg, p3d, x64, ms, ev, ec, gX.to_dense().double().numpy(), gY.to_dense().double().numpy(), F)
    for i, d in enumerate(dots):
        print(f"block {i}: |dots| < 2 at {float((np.abs(d) < 2).mean()):.3f} of the entries, largest {np.abs(d).max():.3f}")
    outn64 = out64 / np.maximum(np.linalg.norm(out64, axis=1, keepdims=True), 1e-5)
    rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
    floor, floor_n, floor_mv = rel(out.numpy(), out64), rel(outn.numpy(), outn64), rel(mv.numpy(), mv64)
    with torch.no_grad():
        pos32 = model.positional_encoding(verts * np.pi * 6).numpy()
        hks32 = ref_model.diffusion_net.geometry.compute_hks_autoscale(evals, evecs, 16).numpy()
    floor_pos, floor_hks = rel(pos32, pos64), rel(hks32, hks64)
    print(f"pos_enc {pos32.shape}: floor {floor_pos:.3e}; hks {hks32.shape}: floor {floor_hks:.3e}")
    print(f"out {tuple(out.shape)}: max |out| = {np.abs(out64).max():.4f}, f32_floor = {floor:.3e}, normalised {floor_n:.3e}, mv_features {floor_mv:.3e}")
    res = dict(k_eig=np.array(K_EIG), width=np.array(WIDTH), blocks=np.array(BLOCKS), names=np.array(names), verts=V, faces=F.astype(np.int32),
               R=R, T=T, fts=fts, pix2face=p2f, mass=mass.numpy(), evals=evals.numpy(), evecs=evecs.numpy(), pos_enc=pos32, hks=hks32, floor_pos=np.array(floor_pos), floor_hks=np.array(floor_hks),
               mv_features=mv.numpy(), out=out.numpy(), out_normalized=outn.numpy(), f32_floor=np.array(floor), floor_normalized=np.array(floor_n),
               floor_mv=np.array(floor_mv))
    for i, n in enumerate(names):
        res[f"p{i}"] = params[n]
    for name, G in (("gradX", gX), ("gradY", gY)):
        res[f"{name}_row"], res[f"{name}_col"] = G.indices()[0].numpy().astype(np.int32), G.indices()[1].numpy().astype(np.int32)
        res[f"{name}_val"] = G.values().numpy()
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

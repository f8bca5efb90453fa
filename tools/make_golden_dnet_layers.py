#!/usr/bin/env python
"""
DiffusionNet forward fixture, produced by RUNNING THE REFERENCE's diffusion_net/layers.py on the CPU.

    python tools/make_golden_dnet_layers.py <reference checkout>        -> tests/golden/fx_dnet_layers.npz

The reference's module is imported as tools/make_golden_dnet.py imports geometry: an empty package module named diffusion_net whose
__path__ is the reference's directory, and empty stub modules for potpourri3d and robust_laplacian.  Its DiffusionNet runs in float32,
eval mode, seeded, unbatched with sparse (N, N) gradient operators (case c: a (B, N, C) batch without gradient features), on operators
from THIS package's host route in float32 (compute_operators(route="host")), which are stored: no test depends on an eigensolver.

Meshes: t, f, r of tools/make_golden_dnet.py, and t2 = the torus of t perturbed with seed 12.  k_eig = 16.
Cases (settings in <case>_cfg, JSON):
  a  mesh t: C_in 19, width 32, C_out 24, 2 blocks, defaults
  b  mesh f: C_in 5, width 48, C_out 3, 1 block, mlp_hidden_dims=[40], with_gradient_rotations=False
  c  meshes t, t2 as a (2, N, C) batch: C_in 7, width 32, C_out 8, 2 blocks, with_gradient_features=False, outputs_at="global_mean"
  d  mesh t: C_in 19, width 32, C_out 6, 1 block, outputs_at="faces", last_activation=log_softmax over the channels
diffusion_time is uniform in [0, 0.05) with channel 0 left at 0 and channel 1 set to -0.01: the clamp branch.
Stored per case: <case>_names (parameter names in order), <case>_p<i> (the parameters BEFORE the forward), <case>_x, <case>_y_ref32,
<case>_f32_floor = max |y_ref32 - y64| / max |y64| with y64 from tests/dnet_layers_restate.py.
Asserted: in every block with gradient features at least half of the values in front of tanh satisfy |dots| < 2 (a saturated tanh
would hide the gradient path); the largest is printed.
"""
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
OUT = os.path.join(REPO, "tests", "golden", "fx_dnet_layers.npz")
K_EIG = 16

CASES = {
    "a": dict(meshes=["t"], seed=101, net=dict(C_in=19, C_out=24, C_width=32, N_block=2)),
    "b": dict(meshes=["f"], seed=102, net=dict(C_in=5, C_out=3, C_width=48, N_block=1, mlp_hidden_dims=[40], with_gradient_rotations=False)),
    "c": dict(meshes=["t", "t2"], seed=103, net=dict(C_in=7, C_out=8, C_width=32, N_block=2, with_gradient_features=False, outputs_at="global_mean")),
    "d": dict(meshes=["t"], seed=104, net=dict(C_in=19, C_out=6, C_width=32, N_block=1, outputs_at="faces", last_activation="log_softmax")),
}


def import_reference(checkout):
    root = os.path.join(checkout, "densematcher", "diffusion_net")
    if not os.path.isdir(root):
        root = os.path.join(checkout, "diffusion_net")
    for name in ("potpourri3d", "robust_laplacian"):
        sys.modules.setdefault(name, types.ModuleType(name))
    pkg = types.ModuleType("diffusion_net")
    pkg.__path__ = [root]
    sys.modules["diffusion_net"] = pkg
    import diffusion_net.layers as ref_layers
    return ref_layers


def log_softmax(x):
    return torch.nn.functional.log_softmax(x, dim=-1)


def main():
    ref = import_reference(sys.argv[1])
    import dnet_layers_restate as rs
    from make_golden_dnet import fan_mesh
    from densematcher_amd import synth
    from densematcher_amd.diffusion_net import geometry as geo
    meshes = {"t": synth.torus_mesh(16, 10, perturb=0.12, seed=11), "f": fan_mesh(), "t2": synth.torus_mesh(16, 10, perturb=0.12, seed=12),
              "r": synth.torus_mesh(12, 8)}
    out, ops = {"k_eig": np.array(K_EIG)}, {}
    for key, (V, F) in meshes.items():
        verts, faces = torch.tensor(np.asarray(V, np.float32)), torch.tensor(np.asarray(F, np.int64))
        _, mass, _, evals, evecs, gX, gY = geo.compute_operators(verts, faces, K_EIG, route="host")
        assert all(t.dtype == torch.float32 for t in (mass, evals, evecs, gX, gY))
        ops[key] = (mass, evals, evecs, gX.coalesce(), gY.coalesce(), faces)
        out[f"faces_{key}"] = np.asarray(F, np.int32)
        out[f"mass_{key}"], out[f"evals_{key}"], out[f"evecs_{key}"] = mass.numpy(), evals.numpy(), evecs.numpy()
        for name, G in (("gradX", gX.coalesce()), ("gradY", gY.coalesce())):
            out[f"{name}_row_{key}"], out[f"{name}_col_{key}"] = G.indices()[0].numpy().astype(np.int32), G.indices()[1].numpy().astype(np.int32)
            out[f"{name}_val_{key}"] = G.values().numpy()
    for case, spec in CASES.items():
        torch.manual_seed(spec["seed"])
        kw = dict(spec["net"])
        if kw.get("last_activation") == "log_softmax":
            kw["last_activation"] = log_softmax
        net = ref.DiffusionNet(**kw).float().eval()
        with torch.no_grad():
            for blk in net.blocks:
                t = blk.diffusion.diffusion_time
                t.copy_(0.05 * torch.rand(t.shape))
                t[0], t[1] = 0.0, -0.01
        names = [n for n, _ in net.named_parameters()]
        params = {n: p.detach().clone().numpy() for n, p in net.named_parameters()}
        ks = spec["meshes"]
        n = ops[ks[0]][0].shape[0]
        x = torch.randn((len(ks), n, kw["C_in"]), dtype=torch.float32)
        with torch.no_grad():
            if len(ks) == 1:
                mass, evals, evecs, gX, gY, faces = ops[ks[0]]
                y = net(x[0], mass, L=None, evals=evals, evecs=evecs, gradX=gX, gradY=gY, faces=faces)
            else:
                st = lambda i: torch.stack([ops[k][i] for k in ks])
                y = net(x, st(0), L=None, evals=st(1), evecs=st(2))
        dn = lambda G: G.to_dense().double().numpy()
        stn = lambda i: np.stack([ops[k][i].numpy() for k in ks])
        xs, ms, ev, ec = x.numpy(), stn(0), stn(1), stn(2)
        Gx, Gy = np.stack([dn(ops[k][3]) for k in ks]), np.stack([dn(ops[k][4]) for k in ks])
        fc = np.stack([ops[k][5].numpy() for k in ks])
        cfg = dict(spec["net"])
        cfg.setdefault("with_gradient_features", True)
        cfg.setdefault("with_gradient_rotations", True)
        cfg.setdefault("outputs_at", "vertices")
        if len(ks) == 1:
            y64, dots = rs.forward(cfg, params, xs[0], ms[0], ev[0], ec[0], Gx[0], Gy[0], fc[0])
        else:
            y64, dots = rs.forward(cfg, params, xs, ms, ev, ec, Gx, Gy, fc)
        for i, d in enumerate(dots):
            share = float((np.abs(d) < 2).mean())
            print(f"case {case}: block {i}: |dots| < 2 at {share:.3f} of the entries, largest {np.abs(d).max():.3f}")
            assert share >= 0.5, (case, i, share)
        floor = float(np.abs(y.numpy().astype(np.float64) - y64).max() / np.abs(y64).max())
        print(f"case {case}: output {tuple(y.shape)}, max |y| = {np.abs(y64).max():.4f}, f32_floor = {floor:.3e}")
        out[f"{case}_cfg"] = np.array(json.dumps(dict(cfg, meshes=ks)))
        out[f"{case}_names"] = np.array(names)
        for i, nme in enumerate(names):
            out[f"{case}_p{i}"] = params[nme]
        out[f"{case}_x"] = xs if len(ks) > 1 else xs[0]
        out[f"{case}_y_ref32"] = y.numpy()
        out[f"{case}_f32_floor"] = np.array(floor)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

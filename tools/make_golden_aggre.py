#!/usr/bin/env python
"""
Aggregation network fixture, produced by RUNNING THE REFERENCE's AggregationNetwork (densematcher/featurizers/modules/projection_network.py
with modules/resnet.py) on the CPU in float32.

    python tools/make_golden_aggre.py <reference checkout>        -> tests/golden/fx_aggre.npz

The two files are imported by path under a stub package, with a stub fvcore.nn.weight_init whose c2_msra_fill is what fvcore's is:
Kaiming-normal weights with fan-out and the ReLU gain, zero bias (fvcore is not installed; every parameter is overwritten below anyway).
The rotation-averaged gathering in front of the network (SDDINO.py) cannot be recorded: it needs the SD model and torchvision.  It is
pinned to tests/aggre_restate.py instead, which tests/test_aggre_cpu.py pins to F.grid_sample / F.interpolate.

Cases (seeded; every parameter moved away from its initial value, norm weights, biases and mixing_weights included; eval mode):
  a  feature_dims [8, 12, 16, 6], projection_dim 16, num_norm_groups 2, B = 2, 3 x 5
  b  feature_dims [40, 72, 72, 24], projection_dim 64, num_norm_groups 8, B = 1, 6 x 6
Stored per case <k>: <k>_names (the state_dict keys), <k>_p<i> (their arrays), <k>_dims, <k>_proj, <k>_groups, <k>_x (the input),
<k>_level0 .. (the output of every level's block, by forward hooks), <k>_y_ref32 (the reference's output) and
<k>_f32_floor = max |y_ref32 - y64| / max |y64| with y64 from tests/aggre_restate.py.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "fx_aggre.npz")

CASES = {"a": dict(dims=[8, 12, 16, 6], proj=16, groups=2, B=2, hw=(3, 5), seed=301),
         "b": dict(dims=[40, 72, 72, 24], proj=64, groups=8, B=1, hw=(6, 6), seed=302)}


def import_reference(checkout):
    root = os.path.join(checkout, "densematcher", "featurizers", "modules")
    if not os.path.isdir(root):
        raise SystemExit(f"{root} not found")

    def c2_msra_fill(module):
        torch.nn.init.kaiming_normal_(module.weight, mode="fan_out", nonlinearity="relu")
        if module.bias is not None:
            torch.nn.init.constant_(module.bias, 0)

    fv, fvnn, wi = types.ModuleType("fvcore"), types.ModuleType("fvcore.nn"), types.ModuleType("fvcore.nn.weight_init")
    fv.__path__, fvnn.__path__ = [], []
    wi.c2_msra_fill = c2_msra_fill
    fv.nn, fvnn.weight_init = fvnn, wi
    pkg = types.ModuleType("ref_modules")
    pkg.__path__ = [root]
    sys.modules.update({"fvcore": fv, "fvcore.nn": fvnn, "fvcore.nn.weight_init": wi, "ref_modules": pkg})
    mods = {}
    for name in ("resnet", "projection_network"):
        spec = importlib.util.spec_from_file_location(f"ref_modules.{name}", os.path.join(root, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[f"ref_modules.{name}"] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["projection_network"]


def run_case(ref, c):
    import aggre_restate as rs
    gen = torch.Generator().manual_seed(c["seed"])
    model = ref.AggregationNetwork(feature_dims=c["dims"], projection_dim=c["proj"], num_norm_groups=c["groups"]).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.add_((0.5 if name == "mixing_weights" else 0.25) * torch.randn(p.shape, generator=gen))
    x = torch.randn((c["B"], sum(c["dims"])) + c["hw"], generator=gen)
    levels = {}
    hooks = [layer.register_forward_hook(lambda m, i, o, l=l: levels.__setitem__(l, o.detach().clone()))
             for l, layer in enumerate(model.bottleneck_layers)]
    with torch.no_grad():
        y = model(x)
    for h in hooks:
        h.remove()
    state = {k: v.numpy().copy() for k, v in model.state_dict().items()}
    y64 = rs.network(x.numpy(), state, c["dims"], c["groups"])
    floor = float(np.abs(y.numpy() - y64["y"]).max() / np.abs(y64["y"]).max())
    out = {"names": np.array(list(state)), "dims": np.array(c["dims"]), "proj": np.int64(c["proj"]), "groups": np.int64(c["groups"]),
           "x": x.numpy(), "y_ref32": y.numpy(), "f32_floor": np.float64(floor)}
    out.update({f"p{i}": v for i, v in enumerate(state.values())})
    out.update({f"level{l}": levels[l].numpy() for l in range(len(c["dims"]))})
    return out, floor


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    fx = {}
    for k, c in CASES.items():
        out, floor = run_case(ref, c)
        print(f"case {k}: y {out['y_ref32'].shape}, max |y| {np.abs(out['y_ref32']).max():.3f}, f32_floor {floor:.2e}")
        assert floor < 5e-6, floor
        fx.update({f"{k}_{n}": v for n, v in out.items()})
    np.savez_compressed(OUT, **fx)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()

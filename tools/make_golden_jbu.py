#!/usr/bin/env python
"""
JBU feature upsampling fixture, produced by RUNNING THE REFERENCE's JBUStack (third_party/featup/featup/upsamplers.py) on the CPU in float32.

    python tools/make_golden_jbu.py <reference checkout>        -> tests/golden/fx_jbu.npz

upsamplers.py is imported under its own name through stub package modules: an empty `featup` package whose __path__ is the reference's
directory, and a stub featup.adaptive_conv_cuda.adaptive_conv whose AdaptiveConv.apply calls the REFERENCE's own CPU operator
(featup/adaptive_conv_cuda/adaptive_conv.cpp: forward), compiled here with torch.utils.cpp_extension.load into a temporary directory
outside the repository (the reference's adaptive_conv.py cannot be imported: it needs the CUDA extension too).  Nothing compiled is kept.

Cases (seeded weights, every parameter moved away from its initial value, range_temp and sigma_spatial included; eval mode):
  a  C = 6, source 3 x 3, image 48 x 48, B = 1
  b  C = 5, source 2 x 3, image 32 x 48, B = 2 with different images
Stored per case <k>: <k>_names (the state_dict keys), <k>_p<i> (their arrays), <k>_src, <k>_img, <k>_stage1 .. <k>_stage4 (the outputs of
up1 .. up4, by forward hooks), <k>_kernel1 (up1's combined kernel (B, 2h, 2w, 7, 7): the second argument of its AdaptiveConv call),
<k>_y_ref32 (the reference's output) and <k>_f32_floor = max |y_ref32 - y64| / max |y64| with y64 from tests/jbu_restate.py.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "fx_jbu.npz")

CASES = {"a": dict(C=6, hw=(3, 3), img=(48, 48), B=1, seed=101), "b": dict(C=5, hw=(2, 3), img=(32, 48), B=2, seed=202)}
_SEEN = {}


def import_reference(checkout):
    root = os.path.join(checkout, "third_party", "featup", "featup")
    if not os.path.isdir(root):
        raise SystemExit(f"{root} not found")
    from torch.utils.cpp_extension import load
    build_dir = tempfile.mkdtemp(prefix="jbu_ref_op_")
    op = load(name="adaptive_conv_cpp_impl", sources=[os.path.join(root, "adaptive_conv_cuda", "adaptive_conv.cpp")], build_directory=build_dir,
              verbose=False)

    class AdaptiveConv:
        @staticmethod
        def apply(padded, kernel):
            _SEEN.setdefault("kernels", []).append(kernel.detach().clone())
            return op.forward(padded, kernel)

    pkg = types.ModuleType("featup")
    pkg.__path__ = [root]
    sub = types.ModuleType("featup.adaptive_conv_cuda")
    sub.__path__ = []
    stub = types.ModuleType("featup.adaptive_conv_cuda.adaptive_conv")
    stub.AdaptiveConv = AdaptiveConv
    sys.modules.update({"featup": pkg, "featup.adaptive_conv_cuda": sub, "featup.adaptive_conv_cuda.adaptive_conv": stub})
    spec = importlib.util.spec_from_file_location("featup.upsamplers", os.path.join(root, "upsamplers.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["featup.upsamplers"] = mod
    spec.loader.exec_module(mod)
    return mod


def run_case(ups, c):
    import jbu_restate as rs
    gen = torch.Generator().manual_seed(c["seed"])
    model = ups.get_upsampler("jbu_stack", c["C"]).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            scale = 0.3 if name.endswith(("range_temp", "sigma_spatial")) else 0.25
            p.add_(scale * torch.randn(p.shape, generator=gen))
    src = torch.randn((c["B"], c["C"]) + c["hw"], generator=gen)
    img = torch.randn((c["B"], 3) + c["img"], generator=gen)
    stages = {}
    hooks = [getattr(model, f"up{s}").register_forward_hook(lambda m, i, o, s=s: stages.__setitem__(s, o.detach().clone())) for s in range(1, 5)]
    _SEEN.clear()
    with torch.no_grad():
        y = model(src, img)
    for h in hooks:
        h.remove()
    state = {k: v.numpy().copy() for k, v in model.state_dict().items()}
    y64 = rs.stack(src.numpy(), img.numpy(), state)
    floor = float(np.abs(y.numpy() - y64["y"]).max() / np.abs(y64["y"]).max())
    out = {"names": np.array(list(state)), "src": src.numpy(), "img": img.numpy(), "kernel1": _SEEN["kernels"][0].numpy(),
           "y_ref32": y.numpy(), "f32_floor": np.float64(floor)}
    out.update({f"p{i}": v for i, v in enumerate(state.values())})
    out.update({f"stage{s}": stages[s].numpy() for s in range(1, 5)})
    return out, floor


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ups = import_reference(sys.argv[1])
    fx = {}
    for k, c in CASES.items():
        out, floor = run_case(ups, c)
        print(f"case {k}: y {out['y_ref32'].shape}, max |y| {np.abs(out['y_ref32']).max():.3f}, f32_floor {floor:.2e}")
        assert floor < 5e-6, floor
        fx.update({f"{k}_{n}": v for n, v in out.items()})
    np.savez_compressed(OUT, **fx)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()

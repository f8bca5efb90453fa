#!/usr/bin/env python
"""
Time of the DINOv2 encoder (featurizers.dinov2.DinoVisionTransformer.tokens) at the workload's size on one GPU: the device route
(MatchEngine.vit_tokens: dm_vit_patch_rows_f16, dm_vit_layernorm_f16, dm_vit_linear_f16, dm_vit_attention_f16) against the torch route of
the same process -- the baseline: the parent commit has no ViT -- in fp16 as the reference runs it (module.half(), fp16 activations,
F.scaled_dot_product_attention) and in fp32.

    python tools/vit_time.py [--images 20] [--out result.json]

Input: ViT-B/14 (768 wide, 12 heads, 12 blocks) with seeded weights (no checkpoint is needed), 20 images -- 5 views x 4 rotations
-- of 336 x 336 (P = 24, 577 tokens), layer 11.  The routes' outputs are compared first.  Two warm-up calls per route, then five timed
windows taken alternately between the routes; a window is `reps` calls between two device synchronisations on the host clock, the figure
is the median window over reps.  "kernels": launches and milliseconds per kernel name over one device call (dm_profile_kernel("*"): HIP
events around every launch, which serialises them -- the sum is an upper bound of the call).  "linear_tflops" / "attention_tflops": the
FLOPs of those launches (2 M N K per product; 4 T^2 64 per image and head) over their summed event times, and as fractions of the fp16
matrix peak of 2.5 PFLOP/s (MI355X spec, dense).  Prints one JSON line.

featurizers.dinov2.AUTO_DEVICE is True only where device_ms <= torch_fp16_ms here.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_F16 = 2.5e15


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--patches", type=int, default=24)
    ap.add_argument("--layer", type=int, default=11)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vit_time: needs a ROCm GPU; a time taken elsewhere says nothing")
    from densematcher_amd.engine import default_engine
    from densematcher_amd.featurizers import dinov2
    dev = torch.device("cuda")
    eng = default_engine()
    torch.manual_seed(0)
    model = dinov2.dinov2_vitb14().eval().requires_grad_(False)
    with torch.no_grad():
        for name, p in model.named_parameters():                         # moved off the initial values; LayerScale around 0.5
            if name.endswith("gamma"):
                p.copy_(0.2 + 0.6 * torch.rand_like(p))
            elif p.dim() == 1 and "norm" in name and name.endswith("weight"):
                p.copy_(0.5 + torch.rand_like(p))
            elif name in ("cls_token", "pos_embed"):
                p.copy_(0.5 * torch.randn_like(p))
            else:
                p.add_(0.02 * torch.randn_like(p))
    model = model.to(dev)
    half = copy.deepcopy(model).half()
    sdpa = copy.deepcopy(half)
    for blk in sdpa.blocks:
        blk.attn.sdpa = True
    n, P, L = a.images, a.patches, a.layer
    T, D = 1 + P * P, model.embed_dim
    x = torch.randn((n, 3, 14 * P, 14 * P), device=dev)
    xh = x.half()
    result = {"tool": "tools/vit_time.py", "model": "dinov2_vitb14 (seeded)", "images": n, "patches": P, "tokens": T, "layer": L,
              "gpu": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        routes = {"device": lambda: model.tokens(x, layer=L, route="device"),
                  "torch_fp16": lambda: sdpa.tokens(xh, layer=L, route="torch"),
                  "torch_fp16_plain": lambda: half.tokens(xh, layer=L, route="torch"),
                  "torch_fp32": lambda: model.tokens(x, layer=L, route="torch")}
        ref = routes["torch_fp32"]()
        scale = float(ref.abs().max())
        for k in ("device", "torch_fp16"):
            result[f"max_rel_diff_{k}_vs_fp32"] = float((routes[k]().float() - ref).abs().max()) / scale
        del ref
        for fn in routes.values():
            fn(), fn()
        times = {k: [] for k in routes}
        for _ in range(5):
            for k, fn in routes.items():
                times[k].append(window(fn, a.reps))
        for k, v in times.items():
            result[f"{k}_ms"] = round(statistics.median(v), 3)
            result[f"{k}_ms_all"] = [round(t, 3) for t in v]
        result["auto_device"] = result["device_ms"] <= result["torch_fp16_ms"]
        eng.profile_kernel("*")
        routes["device"]()
        torch.cuda.synchronize()
        kern = eng.profile_report()
        eng.profile_kernel(None)
    result["kernels"] = {k: [v[0], round(v[1], 3)] for k, v in kern.items()}
    blocks, hidden = L + 1, 4 * D
    lin_flops = 2.0 * n * (P * P * 640 * D + blocks * T * (3 * D * D + D * D + 2 * D * hidden))
    att_flops = 4.0 * n * model.num_heads * blocks * T * T * 64
    for name, flops in (("linear", lin_flops), ("attention", att_flops)):
        ms = kern.get(f"vit_{name}", (0, 0.0))[1]
        if ms > 0:
            result[f"{name}_tflops"] = round(flops / ms * 1e-9, 1)
            result[f"{name}_peak_fraction"] = round(flops / (ms * 1e-3) / PEAK_F16, 4)
    result["total_tflop"] = round((lin_flops + att_flops) * 1e-12, 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""
Time and peak memory of one training step's forward + backward of JBU feature upsampling (featup.upsamplers.JBUStack in training mode)
on one GPU: the differentiable device route (route="device", differentiable=True: per stage the kernels from the torch expressions, then
ONE autograd node -- dm_jbu_apply forward, dm_jbu_apply_bwd_filters_f32 + dm_jbu_apply_bwd_source_f32 backward) against the torch route
of the same process (the reference's expressions under autograd, the adaptive convolution as a loop over the 49 taps) -- the
baseline: the parent commit has no device backward to compare with.

    python tools/jbu_train_time.py [--cases full,small] [--out result.json]

Cases: "full" the settings of tools/jbu_time.py (5 views, C = 768, source 24 x 24 fp16, image 384 x 384), "small" 2 views of 128
channels at the same sizes, which fits where the full case does not.  Seeded weights moved off their initial values; the source and
every parameter require grad; the upstream gradient is a fixed random tensor, so that the step is forward + backward and nothing else.
Both routes are run once first and their source gradients compared (dropout drawn from the same seed).  Per route: two warm-up steps,
then five timed steps, each between two device synchronisations on the host clock; the figure is the median.  Peak memory is
torch.cuda.max_memory_allocated over one step after a reset, minus what was allocated before it (the weights and inputs), to which
the library's own workspace (dm_workspace_bytes) is added for the device route.  The three kernels are timed the same way on the
operands of each stage.  A case that does not fit is reported as "out of memory" and the tool goes on.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CASES = {"full": dict(views=5, channels=768, source=24), "small": dict(views=2, channels=128, source=24)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, steps=5, warmup=2):
    for _ in range(warmup):
        fn()
    return round(statistics.median([timed(fn) for _ in range(steps)]), 3)


def run_case(name, views, channels, source):
    from densematcher_amd.engine import default_engine
    from densematcher_amd.featup.upsamplers import JBUStack
    dev, eng = torch.device("cuda"), default_engine()
    torch.manual_seed(0)
    model = JBUStack(channels)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    model = model.to(dev).train()
    h, size = source, 16 * source
    src = torch.randn((views, channels, h, h), device=dev).half().requires_grad_(True)
    img = torch.randn((views, 3, size, size), device=dev)
    gout = torch.randn((views, channels, size, size), device=dev)
    rec = {"case": name, "views": views, "channels": channels, "source": h, "size": size, "dtype": "float16"}

    def step(route):
        model.zero_grad(set_to_none=True)
        src.grad = None
        model(src, img, route=route, differentiable=True).backward(gout)

    grads = {}
    for route in ("device", "torch"):
        try:
            torch.manual_seed(1)
            step(route)
            grads[route] = src.grad.float().clone()
            rec[f"{route}_ms"] = median_ms(lambda: step(route))
            torch.cuda.synchronize()
            src.grad = None
            model.zero_grad(set_to_none=True)
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(route)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            if route == "device":
                rec["device_workspace_mb"] = round(eng.lib.dm_workspace_bytes(eng.ctx) / 2 ** 20, 1)
                peak += eng.lib.dm_workspace_bytes(eng.ctx)
            rec[f"{route}_peak_mb"] = round(peak / 2 ** 20, 1)
        except torch.cuda.OutOfMemoryError:
            rec[f"{route}_ms"] = rec[f"{route}_peak_mb"] = "out of memory"
        src.grad = None
        model.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
    if len(grads) == 2:
        rec["max_rel_diff_source_grad"] = float((grads["device"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
    grads.clear()
    # ---- the kernels, on the operands of each stage
    stages = []
    with torch.no_grad():
        x = src.detach()
        for s in range(4):
            g = F.adaptive_avg_pool2d(img, (2 * h << s, 2 * h << s))
            filt = getattr(model, f"up{s + 1}").eval().combined_kernel(g).reshape(views, g.shape[2], g.shape[3], 49).contiguous()
            go = gout[:, :, :g.shape[2], :g.shape[3]].contiguous()
            stages.append({"out": int(g.shape[2]),
                           "apply_ms": median_ms(lambda: eng.jbu_apply(x, filt)),
                           "bwd_filters_ms": median_ms(lambda: eng.jbu_apply_bwd_filters(go, x)),
                           "bwd_source_ms": median_ms(lambda: eng.jbu_apply_bwd_source(go, filt))})
            x = eng.jbu_apply(x, filt)
            del go, filt
    rec["stages"] = stages
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="small,full")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jbu_train_time: needs a ROCm GPU; a time taken elsewhere says nothing")
    result = {"tool": "tools/jbu_train_time.py", "gpu": torch.cuda.get_device_name(0), "cases": []}
    for name in a.cases.split(","):
        result["cases"].append(run_case(name, **CASES[name]))
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

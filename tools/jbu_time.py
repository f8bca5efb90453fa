#!/usr/bin/env python
"""
Time of JBU feature upsampling (featup.upsamplers.JBUStack) at the workload's size on one GPU: the device route (MatchEngine.jbu_stack:
dm_jbu_filters_f32 + dm_jbu_apply per stage, dm_dnet_linear_f32 for the final 1x1 convolution) against the torch route of the same
process (the reference's expressions, the adaptive convolution as a loop over the 49 taps) -- the baseline: the parent commit has no
upsampler to compare with.

    python tools/jbu_time.py [--views 5] [--out result.json]

Input: 5 views, C = 768, source 24 x 24 fp16, image 384 x 384, seeded weights moved off their initial values.  The routes' outputs are
compared first (the device route converts the fp16 source to fp32 on load, so it is compared with the torch route on the converted
source; the torch route as timed interpolates the fp16 source in fp16, "max_rel_diff_torch_fp16_source").  Two warm-up calls per figure, then five timed windows taken alternately between the routes; a window is `reps` calls
between two device synchronisations on the host clock, the figure is the median window over reps.  The device route's parts are timed the
same way on the operands of each stage: the kernels of the stage (filters), the apply, and the final convolution (fixup); "pool_ms" is
torch's adaptive_avg_pool2d of all four stages.  Prints one JSON line.

featup.upsamplers.AUTO_DEVICE["stack"] takes the device route where device_ms <= torch_ms; ["stage"] where every stage's
filters + apply is not slower than the stage on torch.
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


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def median_ms(fn, reps, windows=5):
    for _ in range(2):
        fn()
    return round(statistics.median([window(fn, reps) for _ in range(windows)]), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--channels", type=int, default=768)
    ap.add_argument("--source", type=int, default=24)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jbu_time: needs a ROCm GPU; a time taken elsewhere says nothing")
    from densematcher_amd.engine import default_engine
    from densematcher_amd.featup.upsamplers import JBUStack
    dev = torch.device("cuda")
    eng = default_engine()
    torch.manual_seed(0)
    model = JBUStack(a.channels).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    model = model.to(dev)
    h, size = a.source, 16 * a.source
    src = torch.randn((a.views, a.channels, h, h), device=dev).half()
    img = torch.randn((a.views, 3, size, size), device=dev)
    result = {"tool": "tools/jbu_time.py", "views": a.views, "channels": a.channels, "source": h, "size": size, "dtype": "float16",
              "gpu": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        device_route = lambda: model(src, img, route="device")
        torch_route = lambda: model(src, img, route="torch")
        yd, yt = device_route(), torch_route()
        result["max_rel_diff_torch_fp16_source"] = float((yd - yt).abs().max() / yt.abs().max())     # torch interpolates an fp16 source in fp16
        yt = model(src.float(), img, route="torch")
        result["max_rel_diff"] = float((yd - yt).abs().max() / yt.abs().max())
        del yd, yt
        for _ in range(2):
            device_route(), torch_route()
        td, tt = [], []
        for _ in range(5):
            td.append(window(device_route, a.reps))
            tt.append(window(torch_route, a.reps))
        result.update({"device_ms": round(statistics.median(td), 3), "torch_ms": round(statistics.median(tt), 3),
                       "device_ms_all": [round(v, 3) for v in td], "torch_ms_all": [round(v, 3) for v in tt]})
        result["auto_device_stack"] = result["device_ms"] <= result["torch_ms"]
        # ---- the parts, on the operands of each stage
        packed = model.packed(eng.device)
        guides = [F.adaptive_avg_pool2d(img, (2 * h << s, 2 * h << s)) for s in range(4)]
        result["pool_ms"] = median_ms(lambda: [F.adaptive_avg_pool2d(img, (2 * h << s, 2 * h << s)) for s in range(4)], a.reps)
        x, stages, stage_ok = src, [], True
        for s in range(4):
            up = getattr(model, f"up{s + 1}")
            filt = eng.jbu_filters(guides[s], packed.stages[s])
            last = s == 3
            rec = {"out": int(guides[s].shape[2]),
                   "filters_ms": median_ms(lambda: eng.jbu_filters(guides[s], packed.stages[s]), a.reps),
                   "apply_ms": median_ms(lambda: eng.jbu_apply(x, filt, channels_last=last), a.reps),
                   "torch_stage_ms": median_ms(lambda: up(x, guides[s], route="torch"), a.reps)}
            stage_ok = stage_ok and rec["filters_ms"] + rec["apply_ms"] <= rec["torch_stage_ms"]
            stages.append(rec)
            x = eng.jbu_apply(x, filt, channels_last=last)
        result["stages"] = stages
        result["auto_device_stage"] = stage_ok
        rows = x.permute(0, 2, 3, 1).reshape(a.views, size * size, a.channels)
        out = torch.empty_like(rows)
        result["fixup_ms"] = median_ms(lambda: eng.dnet_linear(rows, packed.fix_w, bias=packed.fix_b, resid=rows, out=out), a.reps)
        conv = model.fixup_proj[1]
        result["torch_fixup_ms"] = median_ms(lambda: conv(x) * 0.1 + x, a.reps)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

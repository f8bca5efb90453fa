"""
featup.upsamplers of the reference (third_party/featup/featup/upsamplers.py:184-303), the part DenseMatcher uses: JBULearnedRange, JBUStack,
Bilinear and get_upsampler("jbu_stack" | "bilinear", dim).  Class names, constructor arguments and state_dict keys are the reference's:
the `upsampler.*` entries of a released FeatUp checkpoint load into JBUStack(dim) with strict=True (extractor.load_upsampler).  The other
upsamplers of that file (resize_conv, carafe, sapa, ifa) are not built.

Routes (forward(..., route=)):
  torch    the reference's expressions on PyTorch, any device, with autograd; the adaptive convolution is adaptive_conv's tap loop.  The
           training path.
  device   inference in HIP (MatchEngine.jbu_filters / jbu_apply / jbu_stack: dm_jbu_filters_f32, dm_jbu_apply, and dm_dnet_linear_f32
           for the final 1x1 convolution).  Refused with ValueError in training mode, when a gradient is required and when the guidance is
           not exactly twice the source size (JBULearnedRange alone is more general than JBUStack ever uses; those cases stay on torch);
           RuntimeError without a GPU.
  auto     the device route where its conditions hold and tools/jbu_time.py measured it not slower (AUTO_DEVICE), else torch.

forward(..., route="device", differentiable=True) is the device route that records the autograd graph (opt-in; 'torch' and 'auto' ignore
the flag): the kernels of a stage come from the torch expressions (combined_kernel: autograd, training mode and Dropout2d as on the
torch route), upsampling + padding + convolution run as ONE autograd node (featup.backward: dm_jbu_apply forward, dm_jbu_apply_bwd_*
backward) that keeps the source and the kernels only, and JBUStack's final fixup_proj is the torch module.  In eval mode the node
takes the kernels' VALUES from dm_jbu_filters_f32, so that a module's output has the bits of its inference device route whether or
not a gradient is recorded (the gradient flows through the torch expressions; the two evaluations differ by fp32 rounding), and a
call that records no graph is the inference route itself.  Conditions: source float16 | float32 and at least 2 x 2, guidance exactly
twice the source, float32 parameters and guidance, everything on the GPU; anything else is refused by name.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .. import _routes
from .adaptive_conv import adaptive_conv
from .backward import jbu_apply

# where tools/jbu_time.py measured the device route not slower than the torch route of the same process on an MI355X (README.md,
# DESIGN.md section 4): "stack" = JBUStack, 17.9 ms against 155 ms (5 views, 768 channels, 24 x 24 -> 384 x 384, fp16 source);
# "stage" = one JBULearnedRange, every stage of that run (filters + apply against the stage on torch: 0.34 / 4.2, 0.41 / 9.5,
# 1.03 / 28.2, 5.61 / 104 ms)
AUTO_DEVICE = {"stage": True, "stack": True}

# the packed parameter block of dm_jbu_filters_f32 (include/densematch.h), offsets in floats
PB_RP_W1, PB_RP_B1, PB_RP_W2, PB_RP_B2, PB_FX_W1, PB_FX_B1, PB_FX_W2T, PB_FX_B2, PB_SPATIAL, PB_TEMP, PB_SIZE = (
    0, 96, 128, 1152, 1184, 3732, 3784, 6332, 6384, 6436, 6440)


def _obstacle(module, source, guidance, shape_obstacle):
    """why the device route cannot run this call, or None"""
    if shape_obstacle:
        return shape_obstacle
    if module.training:
        return "the module is in training mode (the device route is inference only: call .eval())"
    return _routes.grad_obstacle([source, guidance] + list(module.parameters()))


def _route_of(module, route, source, guidance, kind, shape_obstacle):
    """what both modules hand to the one picker: "torch" or "device" for this call"""
    return _routes.pick_torch(route, type(module).__name__, lambda: _obstacle(module, source, guidance, shape_obstacle), AUTO_DEVICE[kind],
                              lambda: source.is_cuda and guidance.is_cuda and all(p.is_cuda for p in module.parameters()))


def _diff_obstacle(module, source, guidance, shape_obstacle):
    """why the differentiable device route cannot run this call, or None.  Training mode and tensors that require grad are none;
    where the operands lie is asked only in a process that has a GPU (without one the answer is _routes.NO_GPU, as on the device route)"""
    if shape_obstacle:
        return shape_obstacle
    if source.dtype not in (torch.float16, torch.float32):
        return f"the source must be float16 or float32, not {source.dtype}"
    if guidance.dtype != torch.float32 or any(p.dtype != torch.float32 for p in module.parameters()):
        return "the guidance and the parameters must be float32 (the kernels of the adaptive convolution are)"
    if _routes.engine_or_none() is not None and not (source.is_cuda and guidance.is_cuda and all(p.is_cuda for p in module.parameters())):
        return "the source, the guidance and the parameters must be on the GPU"
    return None


def _differentiable_route(module, source, guidance, shape_obstacle):
    """route='device', differentiable=True: passes, or raises as the one picker does"""
    _routes.pick_torch("device", type(module).__name__ + " differentiable=True,", lambda: _diff_obstacle(module, source, guidance, shape_obstacle),
                       True, lambda: True)


class JBULearnedRange(nn.Module):
    """One guided upsampling stage: a 7 x 7 kernel per output pixel -- softmax of the products of learned keys of the guidance, times a
    Gaussian of the offset, normalised, plus a learned correction -- applied to the bicubically upsampled, reflect-padded source."""

    def __init__(self, guidance_dim, feat_dim, key_dim, scale=2, radius=3):
        super().__init__()
        self.scale, self.radius, self.diameter = scale, radius, 2 * radius + 1
        self.guidance_dim, self.key_dim, self.feat_dim = guidance_dim, key_dim, feat_dim
        taps = self.diameter ** 2
        self.range_temp = nn.Parameter(torch.tensor(0.0))
        # positions 1 and 2 (GELU, Dropout2d) hold no parameters: the checkpoint's keys are range_proj.0 / .3 and fixup_proj.0 / .3
        self.range_proj = nn.Sequential(nn.Conv2d(guidance_dim, key_dim, 1, 1), nn.GELU(), nn.Dropout2d(0.1), nn.Conv2d(key_dim, key_dim, 1, 1))
        self.fixup_proj = nn.Sequential(nn.Conv2d(guidance_dim + taps, taps, 1, 1), nn.GELU(), nn.Dropout2d(0.1), nn.Conv2d(taps, taps, 1, 1))
        self.sigma_spatial = nn.Parameter(torch.tensor(1.0))
        self._packed = None

    # ------------------------------------------------------------------ torch route
    def temperature(self):
        return self.range_temp.exp().clamp_min(1e-4).clamp_max(1e4)

    def get_range_kernel(self, x):
        """(B, taps, H, W): softmax over the taps of temperature * <key of the reflected neighbour, key of the pixel>"""
        B, _, H, W = x.shape
        d, keys = self.diameter, self.range_proj(x)
        halo = F.pad(keys, [self.radius] * 4, mode="reflect")
        logits = torch.stack([(halo[:, :, i:i + H, j:j + W] * keys).sum(1) for i in range(d) for j in range(d)], dim=1)
        return F.softmax(self.temperature() * logits, dim=1)

    def get_spatial_kernel(self, device):
        """(1, taps, 1, 1): exp(-|offset|^2 / (2 sigma^2)) with the offsets of a row or column spread over [-1, 1]"""
        off = torch.linspace(-1, 1, self.diameter, device=device)
        dist2 = off[:, None].square() + off[None, :].square()
        return torch.exp(-dist2 / (2 * self.sigma_spatial ** 2)).reshape(1, self.diameter ** 2, 1, 1)

    def combined_kernel(self, guidance):
        """(B, H, W, d, d): the kernel the adaptive convolution applies"""
        B, _, H, W = guidance.shape
        kernel = self.get_range_kernel(guidance) * self.get_spatial_kernel(guidance.device)
        kernel = kernel / kernel.sum(1, keepdim=True).clamp(1e-7)
        kernel = kernel + 0.1 * self.fixup_proj(torch.cat([kernel, guidance], dim=1))
        return kernel.permute(0, 2, 3, 1).reshape(B, H, W, self.diameter, self.diameter)

    def _forward_torch(self, source, guidance):
        H, W = guidance.shape[2:]
        hr = F.interpolate(source, size=(H, W), mode="bicubic", align_corners=False)
        return adaptive_conv(F.pad(hr, [self.radius] * 4, mode="reflect"), self.combined_kernel(guidance), route="torch")

    # ------------------------------------------------------------------ device route
    def packed(self, device):
        """the parameter block of dm_jbu_filters_f32 on `device`, rebuilt when a parameter changed"""
        if (self.guidance_dim, self.key_dim, self.radius) != (3, 32, 3):
            raise ValueError("the device route is built for guidance_dim 3, key_dim 32, radius 3")
        stamp = (torch.device(device),) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed is None or self._packed[0] != stamp:
            with torch.no_grad():
                f = lambda t: t.detach().to(device="cpu", dtype=torch.float32)
                blk = torch.zeros(PB_SIZE, dtype=torch.float32)
                blk[PB_RP_W1:PB_RP_W1 + 96] = f(self.range_proj[0].weight).reshape(-1)
                blk[PB_RP_B1:PB_RP_B1 + 32] = f(self.range_proj[0].bias)
                blk[PB_RP_W2:PB_RP_W2 + 1024] = f(self.range_proj[3].weight).reshape(-1)
                blk[PB_RP_B2:PB_RP_B2 + 32] = f(self.range_proj[3].bias)
                blk[PB_FX_W1:PB_FX_W1 + 49 * 52] = f(self.fixup_proj[0].weight).reshape(-1)
                blk[PB_FX_B1:PB_FX_B1 + 49] = f(self.fixup_proj[0].bias)
                w2t = torch.zeros(49, 52)
                w2t[:, :49] = f(self.fixup_proj[3].weight).reshape(49, 49).t()
                blk[PB_FX_W2T:PB_FX_W2T + 49 * 52] = w2t.reshape(-1)
                blk[PB_FX_B2:PB_FX_B2 + 49] = f(self.fixup_proj[3].bias)
                blk[PB_SPATIAL:PB_SPATIAL + 49] = f(self.get_spatial_kernel(self.sigma_spatial.device)).reshape(-1)
                blk[PB_TEMP] = f(self.temperature())
            self._packed = (stamp, blk.to(device))
        return self._packed[1]

    def _shape_obstacle(self, source, guidance):
        if (self.guidance_dim, self.key_dim, self.radius) != (3, 32, 3):
            return "the device route is built for guidance_dim 3, key_dim 32, radius 3"
        if tuple(guidance.shape[2:]) != (2 * source.shape[2], 2 * source.shape[3]):
            return f"the guidance {tuple(guidance.shape[2:])} is not exactly twice the source {tuple(source.shape[2:])}"
        if source.shape[2] < 2 or source.shape[3] < 2:
            return "the source must be at least 2 x 2"
        return None

    def _forward_device_differentiable(self, source, guidance):
        eng = _routes.engine_or_none()
        B, _, H, W = guidance.shape
        if self.training:
            return jbu_apply(source, self.combined_kernel(guidance).reshape(B, H, W, self.diameter ** 2))
        values = eng.jbu_filters(guidance, self.packed(eng.device))
        if _routes.grad_obstacle([source, guidance] + list(self.parameters())) is None:
            return eng.jbu_apply(source, values)                      # no graph to record: the inference route
        return jbu_apply(source, self.combined_kernel(guidance).reshape(B, H, W, self.diameter ** 2), values)

    def forward(self, source, guidance, route="auto", differentiable=False):
        """source (B, C, h, w), guidance (B, 3, H, W) -> (B, C, H, W).  differentiable: with route="device", record the autograd graph
        (module docstring); the other routes ignore it"""
        if source.shape[0] != guidance.shape[0]:
            raise ValueError("source and guidance differ in their batch size")
        if differentiable and route == "device":
            _differentiable_route(self, source, guidance, self._shape_obstacle(source, guidance))
            return self._forward_device_differentiable(source, guidance)
        if _route_of(self, route, source, guidance, "stage", self._shape_obstacle(source, guidance)) == "torch":
            return self._forward_torch(source, guidance)
        eng = _routes.engine_or_none()
        return eng.jbu_apply(source, eng.jbu_filters(guidance, self.packed(eng.device)))


class PackedStack:
    """what MatchEngine.jbu_stack reads of a JBUStack: the four parameter blocks and the final 1x1 convolution with its 0.1 folded in"""

    def __init__(self, stages, fix_w, fix_b):
        self.stages, self.fix_w, self.fix_b = stages, fix_w, fix_b
        self.dim = fix_w.shape[0]


class JBUStack(nn.Module):
    """Four guided 2x stages (16x in all), each guided by the image pooled to the stage's size, then x + 0.1 conv1x1(x)."""

    def __init__(self, feat_dim, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.up1 = JBULearnedRange(3, feat_dim, 32, radius=3)
        self.up2 = JBULearnedRange(3, feat_dim, 32, radius=3)
        self.up3 = JBULearnedRange(3, feat_dim, 32, radius=3)
        self.up4 = JBULearnedRange(3, feat_dim, 32, radius=3)
        self.fixup_proj = nn.Sequential(nn.Dropout2d(0.2), nn.Conv2d(feat_dim, feat_dim, kernel_size=1))
        self._packed = None

    def upsample(self, source, guidance, up, route="torch", differentiable=False):
        h, w = source.shape[2:]
        return up(source, F.adaptive_avg_pool2d(guidance, (2 * h, 2 * w)), route=route, differentiable=differentiable)

    def packed(self, device):
        conv = self.fixup_proj[1]
        stamp = (torch.device(device), conv.weight.data_ptr(), conv.weight._version, conv.bias._version)
        if self._packed is None or self._packed[0] != stamp:
            with torch.no_grad():
                w = (0.1 * conv.weight.detach().to(device=device, dtype=torch.float32).reshape(conv.out_channels, conv.in_channels)).contiguous()
                b = (0.1 * conv.bias.detach().to(device=device, dtype=torch.float32)).contiguous()
            self._packed = (stamp, w, b)
        return PackedStack([up.packed(device) for up in (self.up1, self.up2, self.up3, self.up4)], self._packed[1], self._packed[2])

    def forward(self, source, guidance, route="auto", out_dtype=None, memory_format=None, chunk=None, differentiable=False):
        """source (B, C, h, w) fp16 | fp32, guidance (B, 3, Hg, Wg) the image -> (B, C, 16 h, 16 w).
        Device route: fp32, NCHW-shaped with channels-last strides (the layout lifting reads fastest) unless out_dtype= / memory_format=
        (torch.contiguous_format | torch.channels_last) ask otherwise -- both convert with torch; chunk= bounds the views in flight
        (at 384 x 384, C = 768 one view's fp32 output is 453 MB).  Torch route: the reference's result, converted likewise when asked.
        differentiable: with route="device", record the autograd graph (module docstring): every stage on its differentiable device
        route, the final fixup_proj on torch, fp32 NCHW, all views at once (chunk= is the inference route's); the other routes ignore it."""
        if source.shape[0] != guidance.shape[0]:
            raise ValueError("source and guidance differ in their batch size")
        shape_obstacle = None if min(source.shape[2:]) >= 2 else "the source must be at least 2 x 2"
        recorded = differentiable and route == "device"
        if recorded:
            _differentiable_route(self, source, guidance, shape_obstacle)
        if recorded or _route_of(self, route, source, guidance, "stack", shape_obstacle) == "torch":
            x = source
            for up in (self.up1, self.up2, self.up3, self.up4):
                x = self.upsample(x, guidance, up, route="device" if recorded else "torch", differentiable=recorded)
            y = self.fixup_proj(x) * 0.1 + x
        else:
            eng = _routes.engine_or_none()
            y = eng.jbu_stack(self.packed(eng.device), source, guidance, chunk=chunk)
        if out_dtype is not None or memory_format is not None:
            y = y.to(dtype=out_dtype or y.dtype, memory_format=memory_format or torch.preserve_format)
        return y


class Bilinear(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)

    def forward(self, feats, img):
        return F.interpolate(feats, tuple(img.shape[2:]), mode="bilinear")


def get_upsampler(upsampler, dim):
    if upsampler == "bilinear":
        return Bilinear()
    if upsampler == "jbu_stack":
        return JBUStack(dim)
    if upsampler in ("resize_conv", "carafe", "sapa", "ifa"):
        raise NotImplementedError(f"upsampler {upsampler!r} of FeatUp is not built here: 'jbu_stack' and 'bilinear' are")
    raise ValueError(f"Unknown upsampler {upsampler}")

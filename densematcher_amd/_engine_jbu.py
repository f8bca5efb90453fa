"""
MatchEngine, guided feature upsampling (FeatUp's JBUStack at inference): the combined 7 x 7 kernels of a stage (dm_jbu_filters_f32), the
fused bicubic upsampling + reflect padding + adaptive convolution (dm_jbu_apply), its two gradients (dm_jbu_apply_bwd_filters_f32,
dm_jbu_apply_bwd_source_f32: what featup.backward chains into autograd), and the four stages with the final 1x1 convolution
(dm_dnet_linear_f32 on pixels as rows).  Filters and apply stay separate entry points: evaluating the last stage only where lifting
samples it needs exactly that split.
"""
import torch
import torch.nn.functional as F

from . import _lib
from ._operands import ptr as _ptr

PARAM_FLOATS = 6440


def _flag(dtype):
    return _lib.DM_F16 if dtype == torch.float16 else _lib.DM_F32


class _JbuOps:
    def _jbu_operand(self, t, what, dtypes):
        """a 4-d operand the kernels read through element strides: on the device, in one of `dtypes` (else float32), where it lies
        unless a stride is negative"""
        t = t if isinstance(t, torch.Tensor) else torch.as_tensor(t)
        if t.dim() != 4:
            raise ValueError(f"{what}, got {tuple(t.shape)}")
        if t.dtype not in dtypes:
            t = t.to(torch.float32)
        if t.device != self.device:
            t = t.to(self.device)
        if any(s < 0 for s in t.stride()):
            t = t.contiguous()
        self._check_stream()
        return t

    def jbu_filters(self, guidance, params):
        """dm_jbu_filters_f32: guidance (B, 3, H, W), already at the stage's output size; params the packed block of the stage
        (featup.upsamplers.JBULearnedRange.packed).  Returns the kernels (B, H, W, 49) fp32."""
        g = self._dev(guidance, torch.float32, "guidance")
        if g.dim() != 4 or g.shape[1] != 3:
            raise ValueError(f"jbu_filters: guidance must be (B, 3, H, W), got {tuple(g.shape)}")
        p = self._dev(params, torch.float32, "params")
        if p.numel() != PARAM_FLOATS:
            raise ValueError(f"jbu_filters: params must hold {PARAM_FLOATS} floats (include/densematch.h), got {p.numel()}")
        Bn, _, H, W = g.shape
        filt = torch.empty((Bn, H, W, 49), dtype=torch.float32, device=self.device)
        self._chk(self.lib.dm_jbu_filters_f32(self.ctx, Bn, H, W, _ptr(g), _ptr(p), _ptr(filt)))
        return filt

    def jbu_apply(self, source, filters, out=None, out_dtype=torch.float32, channels_last=False):
        """dm_jbu_apply: source (B, C, h, w) fp16 | fp32 in any strides (read where it lies), filters (B, 2h, 2w, 49) fp32.
        out: an optional (B, C, 2h, 2w) fp32 | fp16 device tensor in any strides that give every element its own address (written where
        it lies); without it a new one of out_dtype, NCHW, or NCHW-shaped over channels-last memory."""
        src = self._jbu_operand(source, "jbu_apply: source must be (B, C, h, w)", (torch.float16, torch.float32))
        Bn, Cw, h, w = src.shape
        filt = self._dev(filters, torch.float32, "filters")
        if tuple(filt.shape[:3]) != (Bn, 2 * h, 2 * w) or filt.numel() != Bn * 4 * h * w * 49:
            raise ValueError(f"jbu_apply: filters must be ({Bn}, {2 * h}, {2 * w}, 49) for a source {tuple(src.shape)}, got {tuple(filt.shape)}")
        if out is None:
            if out_dtype not in (torch.float16, torch.float32):
                raise ValueError("jbu_apply: out_dtype must be torch.float32 or torch.float16")
            if channels_last:
                out = torch.empty((Bn, 2 * h, 2 * w, Cw), dtype=out_dtype, device=self.device).permute(0, 3, 1, 2)
            else:
                out = torch.empty((Bn, Cw, 2 * h, 2 * w), dtype=out_dtype, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype not in (torch.float16, torch.float32)
              or tuple(out.shape) != (Bn, Cw, 2 * h, 2 * w)):
            raise ValueError(f"jbu_apply: out must be a float32 or float16 ({Bn}, {Cw}, {2 * h}, {2 * w}) tensor on {self.device}")
        self._chk(self.lib.dm_jbu_apply(self.ctx, Bn, Cw, h, w, _flag(src.dtype), _ptr(src), *src.stride(), _ptr(filt), _flag(out.dtype), _ptr(out),
                                        *out.stride()))
        return out

    def jbu_apply_bwd_filters(self, grad_out, source):
        """dm_jbu_apply_bwd_filters_f32: the gradient of jbu_apply's output with respect to its filters.  grad_out (B, C, 2h, 2w) fp32
        and source (B, C, h, w) fp16 | fp32, both in any strides and read where they lie -- the all-zero strides of the expanded
        scalar that out.sum().backward() hands over included: the kernels only read it.  Returns (B, 2h, 2w, 49) fp32."""
        src = self._jbu_operand(source, "jbu_apply_bwd_filters: source must be (B, C, h, w)", (torch.float16, torch.float32))
        Bn, Cw, h, w = src.shape
        g = self._jbu_operand(grad_out, f"jbu_apply_bwd_filters: grad_out must be ({Bn}, {Cw}, {2 * h}, {2 * w})", (torch.float32,))
        if tuple(g.shape) != (Bn, Cw, 2 * h, 2 * w):
            raise ValueError(f"jbu_apply_bwd_filters: grad_out must be ({Bn}, {Cw}, {2 * h}, {2 * w}) for a source {tuple(src.shape)}, "
                             f"got {tuple(g.shape)}")
        gfilt = torch.empty((Bn, 2 * h, 2 * w, 49), dtype=torch.float32, device=self.device)
        self._chk(self.lib.dm_jbu_apply_bwd_filters_f32(self.ctx, Bn, Cw, h, w, _flag(src.dtype), _ptr(src), *src.stride(), _ptr(g), *g.stride(),
                                                        _ptr(gfilt)))
        return gfilt

    def jbu_apply_bwd_source(self, grad_out, filters, out_dtype=torch.float32):
        """dm_jbu_apply_bwd_source_f32: the gradient of jbu_apply's output with respect to its source.  grad_out (B, C, 2h, 2w) fp32 in
        any strides, read where it lies (see jbu_apply_bwd_filters); filters (B, 2h, 2w, 49) fp32.  Returns (B, C, h, w), NCHW: fp32
        as the kernel writes it, or that rounded to out_dtype=torch.float16 with torch."""
        if out_dtype not in (torch.float16, torch.float32):
            raise ValueError("jbu_apply_bwd_source: out_dtype must be torch.float32 or torch.float16")
        g = self._jbu_operand(grad_out, "jbu_apply_bwd_source: grad_out must be (B, C, 2h, 2w)", (torch.float32,))
        Bn, Cw, H, W = g.shape
        if H % 2 or W % 2 or H < 4 or W < 4:
            raise ValueError(f"jbu_apply_bwd_source: grad_out must be (B, C, 2h, 2w) with h, w >= 2, got {tuple(g.shape)}")
        filt = self._dev(filters, torch.float32, "filters")
        if tuple(filt.shape[:3]) != (Bn, H, W) or filt.numel() != Bn * H * W * 49:
            raise ValueError(f"jbu_apply_bwd_source: filters must be ({Bn}, {H}, {W}, 49) for a grad_out {tuple(g.shape)}, got {tuple(filt.shape)}")
        gsrc = torch.empty((Bn, Cw, H // 2, W // 2), dtype=torch.float32, device=self.device)
        self._chk(self.lib.dm_jbu_apply_bwd_source_f32(self.ctx, Bn, Cw, H // 2, W // 2, _ptr(g), *g.stride(), _ptr(filt), _ptr(gsrc)))
        return gsrc if out_dtype == torch.float32 else gsrc.to(out_dtype)

    def jbu_stack(self, packed, source, guidance, chunk=None):
        """JBUStack.forward at inference: packed (featup.upsamplers.PackedStack: four parameter blocks, the final 1x1 convolution with
        its 0.1 folded in), source (B, C, h, w) fp16 | fp32, guidance (B, 3, Hg, Wg) the image.  Per stage: the guidance pooled to the
        stage's size (torch), the kernels, the apply; stage 4 writes fp32 channels-last rows, on which out = x W'^T + b' + x runs as
        dm_dnet_linear_f32 with the pixels as rows.  chunk: views in flight at a time (None: all); a view's bits do not depend on it.
        Returns (B, C, 16h, 16w) fp32, NCHW-shaped over channels-last memory."""
        src = source if isinstance(source, torch.Tensor) else torch.as_tensor(source)
        if src.dim() != 4 or src.shape[1] != packed.dim:
            raise ValueError(f"jbu_stack: source must be (B, {packed.dim}, h, w), got {tuple(src.shape)}")
        g = self._dev(guidance, torch.float32, "guidance")
        if g.dim() != 4 or g.shape[1] != 3 or g.shape[0] != src.shape[0]:
            raise ValueError(f"jbu_stack: guidance must be ({src.shape[0]}, 3, H, W), got {tuple(g.shape)}")
        Bn, Cw, h, w = src.shape
        step = Bn if chunk is None else int(chunk)
        if step < 1:
            raise ValueError("jbu_stack: chunk must be at least 1")
        H, W = 16 * h, 16 * w
        rows = torch.empty((Bn, H * W, Cw), dtype=torch.float32, device=self.device)
        for b0 in range(0, Bn, step):
            x, gb = src[b0:b0 + step], g[b0:b0 + step]
            for s, params in enumerate(packed.stages):
                small = F.adaptive_avg_pool2d(gb, (2 * x.shape[2], 2 * x.shape[3]))
                x = self.jbu_apply(x, self.jbu_filters(small, params), channels_last=(s == 3))
            x = x.permute(0, 2, 3, 1).reshape(x.shape[0], H * W, Cw)          # the memory as it lies: pixels as rows
            self.dnet_linear(x, packed.fix_w, bias=packed.fix_b, resid=x, out=rows[b0:b0 + step])
        return rows.view(Bn, H, W, Cw).permute(0, 3, 1, 2)

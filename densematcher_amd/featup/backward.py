"""
The JBU apply as one differentiable operation on the device: bicubic 2x upsampling, reflect padding by 3 and the adaptive convolution,
forward in dm_jbu_apply, backward in the two kernels FeatUp ships next to its forward (adaptive_conv_cuda: grad_filters, grad_input),
here dm_jbu_apply_bwd_filters_f32 and dm_jbu_apply_bwd_source_f32, which fold the adjoints of the padding and of the upsampling in.
Autograd keeps the source and the kernels only: the upsampled and the padded source, two tensors of the output's size on the torch
route, are rebuilt in LDS by both passes.  Reached through JBULearnedRange / JBUStack with route="device", differentiable=True.
No double backward.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _routes


class JBUApply(torch.autograd.Function):
    """out = jbu_apply(source, filters): source (B, C, h, w) fp16 | fp32, filters (B, 2h, 2w, 49) fp32 -> (B, C, 2h, 2w) fp32.
    values: None, or the same kernels from another evaluation (dm_jbu_filters_f32) whose bits the output and the source's gradient
    take; the gradient still flows to `filters`."""

    @staticmethod
    def forward(ctx, source, filters, values):
        used = filters if values is None else values
        ctx.save_for_backward(source, used)
        return _routes.engine_or_none().jbu_apply(source, used)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        source, used = ctx.saved_tensors
        eng = _routes.engine_or_none()
        gsrc = eng.jbu_apply_bwd_source(grad_out, used, out_dtype=source.dtype) if ctx.needs_input_grad[0] else None
        gfilt = eng.jbu_apply_bwd_filters(grad_out, source) if ctx.needs_input_grad[1] else None
        return gsrc, gfilt, None


def jbu_apply(source, filters, values=None):
    """JBUApply on GPU tensors; the caller (featup.upsamplers) has checked shapes, dtypes and placement"""
    return JBUApply.apply(source, filters, values)

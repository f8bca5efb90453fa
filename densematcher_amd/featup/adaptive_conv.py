"""
featup.adaptive_conv_cuda of the reference: the per-pixel ("adaptive") convolution
    out[b, c, y, x] = sum_{i, j} filters[b, y, x, i, j] * input[b, c, y + i, x + j]
with input (B, C, H + I - 1, W + J - 1) already padded and filters (B, H, W, I, J).

Routes:
  torch    a loop over the I * J taps that accumulates shifted slices of the input in the reference kernel's order (i outer, j inner).
           No (I J) x C x H x W buffer is formed (unfold would form one), autograd records it, it runs on any device: the training path.
  device   dm_jbu_apply -- which fuses the bicubic upsampling and the padding into the convolution -- is reached through
           JBULearnedRange / JBUStack: route='device' at inference, route='device', differentiable=True with its backward kernels
           (featup.backward: dm_jbu_apply_bwd_filters_f32, dm_jbu_apply_bwd_source_f32).  A bare padded input has no device kernel of
           its own, forward or backward, so here 'device' is refused and 'auto' is the torch route.
"""
import torch

from .. import _routes


def _tap_loop(padded, filters):
    B, C, Hp, Wp = padded.shape
    _, H, W, I, J = filters.shape
    out = None
    for i in range(I):
        for j in range(J):
            term = filters[:, None, :, :, i, j] * padded[:, :, i:i + H, j:j + W]
            out = term if out is None else out + term
    return out


def adaptive_conv(input, filters, route="auto"):
    """input (B, C, H + I - 1, W + J - 1), filters (B, H, W, I, J) of the same dtype and device -> (B, C, H, W)"""
    _routes.check(route, _routes.TORCH)
    if input.dim() != 4 or filters.dim() != 5 or filters.shape[0] != input.shape[0]:
        raise ValueError("adaptive_conv: input (B, C, H + I - 1, W + J - 1) and filters (B, H, W, I, J)")
    if input.shape[2] != filters.shape[1] + filters.shape[3] - 1 or input.shape[3] != filters.shape[2] + filters.shape[4] - 1:
        raise ValueError(f"adaptive_conv: input {tuple(input.shape)} is not filters {tuple(filters.shape)} padded by the kernel size - 1")
    if route == "device":
        raise ValueError("adaptive_conv: the device kernels (dm_jbu_apply and its backward) upsample and pad the source themselves: use "
                         "JBULearnedRange / JBUStack with route='device' (differentiable=True where a gradient is needed), or "
                         "MatchEngine.jbu_apply")
    return _tap_loop(input, filters)


class AdaptiveConv:
    """the reference's autograd.Function by its call: AdaptiveConv.apply(input, filters)"""

    @staticmethod
    def apply(input, filters):
        return adaptive_conv(input, filters, route="torch")

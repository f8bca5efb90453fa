"""
featup.layers of the reference (third_party/featup/featup/layers.py:81-102), the two normalisations the extractor applies to the backbone
features before upsampling: ChannelNorm (LayerNorm over the channels, no affine) and UnitNorm (unit length over the channels).
"""
import torch
from torch import nn


class ChannelNorm(nn.Module):
    def __init__(self, dim, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.norm = nn.LayerNorm(dim, elementwise_affine=False)

    def forward(self, x):
        """x (B, C, H, W): zero mean and unit variance over C at every pixel"""
        return self.norm(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class UnitNorm(nn.Module):
    def __init__(self, dim, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dim = dim

    def forward(self, x):
        """x (B, C, H, W): divided by its length over C, the length floored at 1e-8"""
        if x.shape[1] != self.dim:
            raise ValueError(f"UnitNorm({self.dim}) got {x.shape[1]} channels")
        return x / torch.linalg.norm(x, dim=1, keepdim=True).clamp(min=1e-8)

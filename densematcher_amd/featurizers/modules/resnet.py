"""
densematcher.featurizers.modules.resnet of the reference, the part the aggregation network is built from: get_norm, Conv2d (a
convolution with an optional `.norm` and `.activation` behind it), BottleneckBlock and ResNet.make_stage.  Constructor arguments and
state_dict keys are the reference's: shortcut | conv1 | conv2 | conv3 with .weight, .norm.weight, .norm.bias.  Initialisation restates
what the reference takes from fvcore (c2_msra_fill): Kaiming-normal weights with fan-out and the ReLU gain, zero biases; fvcore is not a
dependency.  The ResNet trunk itself (stem, stages, classifier) and EfficientSpatialContextNet are not built.
"""
import torch.nn.functional as F
from torch import nn


def get_norm(norm, out_channels, num_norm_groups=32):
    """None or "" -> None; "GN" -> nn.GroupNorm(num_norm_groups, out_channels); a callable -> norm(out_channels)"""
    if norm is None or (isinstance(norm, str) and not norm):
        return None
    if isinstance(norm, str):
        if norm != "GN":
            raise KeyError(norm)
        return nn.GroupNorm(num_norm_groups, out_channels)
    return norm(out_channels)


def msra_fill(module):
    nn.init.kaiming_normal_(module.weight, mode="fan_out", nonlinearity="relu")
    if module.bias is not None:
        nn.init.constant_(module.bias, 0)


class Conv2d(nn.Conv2d):
    """nn.Conv2d with the keyword arguments norm= (a module) and activation= (a callable): applied in that order behind the convolution"""

    def __init__(self, *args, norm=None, activation=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.norm = norm
        self.activation = activation

    def forward(self, x):
        x = super().forward(x)
        if self.norm is not None:
            x = self.norm(x)
        if self.activation is not None:
            x = self.activation(x)
        return x


class CNNBlockBase(nn.Module):
    def __init__(self, in_channels, out_channels, stride):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride


class BottleneckBlock(CNNBlockBase):
    """conv1 -> norm -> ReLU -> conv2 -> norm -> ReLU -> conv3 -> norm, plus the input (through a 1x1 convolution + norm, `shortcut`,
    when the channel counts differ), then ReLU.  kernel_size: the three convolutions' kernels, (1, 3, 1) in the aggregation network."""

    def __init__(self, in_channels, out_channels, *, bottleneck_channels, stride=1, num_groups=1, norm="GN", stride_in_1x1=False, dilation=1,
                 num_norm_groups=32, kernel_size=(1, 3, 1)):
        super().__init__(in_channels, out_channels, stride)
        mk = lambda channels: get_norm(norm, channels, num_norm_groups)
        self.shortcut = None
        if in_channels != out_channels:
            self.shortcut = Conv2d(in_channels, out_channels, kernel_size=1, stride=stride, bias=False, norm=mk(out_channels))
        stride_1x1, stride_3x3 = (stride, 1) if stride_in_1x1 else (1, stride)
        k1, k2, k3 = kernel_size
        self.conv1 = Conv2d(in_channels, bottleneck_channels, kernel_size=k1, stride=stride_1x1, padding=(k1 - 1) // 2, bias=False,
                            norm=mk(bottleneck_channels))
        self.conv2 = Conv2d(bottleneck_channels, bottleneck_channels, kernel_size=k2, stride=stride_3x3, padding=dilation * (k2 - 1) // 2,
                            bias=False, groups=num_groups, dilation=dilation, norm=mk(bottleneck_channels))
        self.conv3 = Conv2d(bottleneck_channels, out_channels, kernel_size=k3, bias=False, norm=mk(out_channels))
        for layer in (self.conv1, self.conv2, self.conv3, self.shortcut):
            if layer is not None:
                msra_fill(layer)

    def forward(self, x):
        out = F.relu_(self.conv1(x))
        out = F.relu_(self.conv2(out))
        out = self.conv3(out)
        out += self.shortcut(x) if self.shortcut is not None else x
        return F.relu_(out)


class ResNet:
    """only the stage builder of the reference's ResNet: the aggregation network calls ResNet.make_stage and nothing else of it"""

    @staticmethod
    def make_stage(block_class, num_blocks, *, in_channels, out_channels, **kwargs):
        """num_blocks blocks of block_class, the first from in_channels, all to out_channels.  A keyword that ends in `_per_block` is a
        list with one value per block, passed under the name without the suffix; every other keyword goes to every block."""
        blocks = []
        for i in range(num_blocks):
            own = {}
            for key, value in kwargs.items():
                if key.endswith("_per_block"):
                    name = key[:-len("_per_block")]
                    if len(value) != num_blocks or name in kwargs:
                        raise ValueError(f"make_stage: '{key}' needs {num_blocks} values and excludes '{name}'")
                    own[name] = value[i]
                else:
                    own[key] = value
            blocks.append(block_class(in_channels=in_channels, out_channels=out_channels, **own))
            in_channels = out_channels
        return blocks

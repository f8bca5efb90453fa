"""FeatUp's guided feature upsampling as DenseMatcher uses it: upsamplers (JBUStack and its stages), layers (the two normalisations) and
adaptive_conv (the per-pixel convolution).  `from featup.upsamplers import get_upsampler` of the reference becomes
`from densematcher_amd.featup.upsamplers import get_upsampler`."""
from .adaptive_conv import AdaptiveConv, adaptive_conv  # noqa: F401
from .layers import ChannelNorm, UnitNorm  # noqa: F401
from .upsamplers import AUTO_DEVICE, Bilinear, JBULearnedRange, JBUStack, get_upsampler  # noqa: F401

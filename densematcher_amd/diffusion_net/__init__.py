"""DiffusionNet's operator precomputation (diffusion_net.geometry of the reference) with the reference's names; the network itself
(layers, weights, forward pass) stays with PyTorch and is not part of this package."""
from . import geometry, utils  # noqa: F401

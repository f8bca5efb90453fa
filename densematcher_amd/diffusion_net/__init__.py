"""DiffusionNet with the reference's names: the operator precomputation (diffusion_net.geometry) and the network (diffusion_net.layers:
the reference's modules and state_dict keys, with an inference route through fp32 HIP kernels next to the PyTorch expressions)."""
from . import geometry, layers, utils  # noqa: F401

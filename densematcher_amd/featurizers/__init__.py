"""densematcher.featurizers of the reference, the part behind the frozen backbones: the aggregation network (modules), the gathering and
rotation-averaged fusion of the backbones' raw outputs (SDDINO), the image rotation in front of them (util), and the DINOv2 encoder
itself (dinov2)."""
from .SDDINO import aggregate_features, dino_features, gather_features  # noqa: F401
from .modules.projection_network import AggregationNetwork  # noqa: F401
from .util import rotate  # noqa: F401

"""densematcher.featurizers of the reference, the part behind the frozen backbones: the aggregation network (modules), the gathering and
rotation-averaged fusion of the backbones' raw outputs (SDDINO) and the image rotation in front of them (util)."""
from .SDDINO import aggregate_features, gather_features  # noqa: F401
from .modules.projection_network import AggregationNetwork  # noqa: F401
from .util import rotate  # noqa: F401

"""featup.model_utils of the reference, the part DenseMatcher uses: extractor_dino (ViTExtractor)."""
from .extractor_dino import ViTExtractor  # noqa: F401

"""
densematcher.extractor of the reference, the part behind the 2D backbone (extractor.py:177-254): loading FeatUp's JBUStack from a
released checkpoint, and the path from the backbone's low-resolution features to the per-view feature maps that lifting reads.  The
backbone itself (SD / DINO, the aggregation network) and the image preprocessing are outside this package.
"""
import os
import re

import torch

from .featup.layers import ChannelNorm, UnitNorm
from .featup.upsamplers import get_upsampler

PREFIX = "upsampler."


def parse_upsampler_name(path):
    """what the reference reads off the checkpoint's file name (extractor.py:185-195): {'imsize': int | None, 'channelnorm': bool,
    'unitnorm': bool}; a missing flag is False, a missing size None"""
    name = os.fspath(path)
    size = re.search(r"imsize=(\d+)", name)
    flag = lambda key: (re.search(key + r"=(True|False)", name) or [None, "False"])[1] == "True"
    return {"imsize": int(size.group(1)) if size else None, "channelnorm": flag("channelnorm"), "unitnorm": flag("unitnorm")}


def load_upsampler(path_or_state_dict, num_features):
    """JBUStack(num_features) with the `upsampler.*` entries of a FeatUp checkpoint (extractor.py:206-212), loaded strict=True, in eval
    mode.  path_or_state_dict: the checkpoint file (a dict with 'state_dict', as released), such a dict, or a state_dict itself, with
    or without the prefix.  Returns (upsampler, settings): settings = parse_upsampler_name(path) for a path, else {}."""
    settings = {}
    state = path_or_state_dict
    if isinstance(state, (str, os.PathLike)):
        settings = parse_upsampler_name(state)
        state = torch.load(state, map_location="cpu")
    if "state_dict" in state and not isinstance(state["state_dict"], torch.Tensor):
        state = state["state_dict"]
    if any(k.startswith(PREFIX) for k in state):
        state = {k[len(PREFIX):]: v for k, v in state.items() if k.startswith(PREFIX)}
    upsampler = get_upsampler("jbu_stack", num_features)
    upsampler.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=True)
    return upsampler.eval(), settings


def upsample_features(upsampler, features_lr, image, use_unitnorm=False, use_channelnorm=False, route="auto", **kwargs):
    """SDDINOFeatureExtractor.forward without the backbone (extractor.py:246-251): features_lr (B, C, h, w) from the 2D backbone, image
    (B, 3, H, W) the normalised image they were computed from -> features_hr (B, C, 16h, 16w).  route and kwargs (out_dtype=,
    memory_format=, chunk=) go to JBUStack.forward; another upsampler (Bilinear) is called as the reference calls it."""
    num_features = features_lr.shape[1]
    if use_unitnorm:
        features_lr = UnitNorm(num_features)(features_lr)
    if use_channelnorm:
        features_lr = ChannelNorm(num_features)(features_lr)
    if hasattr(upsampler, "up1"):
        return upsampler(features_lr, image, route=route, **kwargs)
    return upsampler(features_lr, image)

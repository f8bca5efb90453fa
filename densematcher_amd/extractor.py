"""
densematcher.extractor of the reference, the part behind the 2D backbone (extractor.py:177-254): loading FeatUp's JBUStack from a
released checkpoint, and the path from the backbone's low-resolution features to the per-view feature maps that lifting reads.  With
load_aggre_net / features_from_backbone the path starts one stage earlier, at the raw outputs of the two frozen backbones (SD's s3, s4,
s5 and DINO's tokens): the aggregation network (featurizers) runs here too.  Of the two backbones the DINOv2 ViT is in this package
(featurizers.dinov2, with a checkpoint the caller loads; its positional-embedding interpolation restates the reference's local copy of
the rule and is not pinned against the hub model's own method); the SD model and the image-file preprocessing are outside it.

A backbone= callable of MeshFeaturizer, images (views, 3, H, W) in [0, 1] -> (s3, s4, s5, dino), chains the caller's own SD call with
this package's ViT:

    vit = ViTExtractor("dinov2_vitb14", stride=14, model=load_dinov2(path, "dinov2_vitb14").to(device))     # featup.model_utils, featurizers.dinov2
    def backbone(images):
        sd = sd_model(images, raw=True)                                    # the caller's: SDDINO.py:46
        return sd["s3"], sd["s4"], sd["s5"], dino_features(vit, images, num_patches)                    # featurizers.dino_features: SDDINO.py:49-51

dino is a permuted view of the token buffer, which aggregate_features reads where it lies.
"""
import os
import re

import torch

from .featurizers.SDDINO import aggregate_features
from .featurizers.modules.projection_network import AggregationNetwork
from .featup.layers import ChannelNorm, UnitNorm
from .featup.upsamplers import get_upsampler

PREFIX = "upsampler."


def parse_upsampler_name(path):
    """what the reference reads off the checkpoint's file name (extractor.py:185-195): {'imsize': int | None, 'channelnorm': bool,
    'unitnorm': bool, 'rotinv': bool}; a missing flag is False, a missing size None.  rotinv: the aggregation network was trained on
    rotation-averaged features (features_from_backbone(rot_inv=True))."""
    name = os.fspath(path)
    size = re.search(r"imsize=(\d+)", name)
    flag = lambda key: (re.search(key + r"=(True|False)", name) or [None, "False"])[1] == "True"
    return {"imsize": int(size.group(1)) if size else None, "channelnorm": flag("channelnorm"), "unitnorm": flag("unitnorm"),
            "rotinv": flag("rotinv")}


def load_upsampler(path_or_state_dict, num_features):
    """JBUStack(num_features) with the `upsampler.*` entries of a FeatUp checkpoint (extractor.py:206-212), loaded strict=True, in eval
    mode.  path_or_state_dict: the checkpoint file (a dict with 'state_dict', as released), such a dict, or a state_dict itself, with
    or without the prefix.  Returns (upsampler, settings): for a path the settings parse_upsampler_name reads that concern the upsampler
    (imsize, channelnorm, unitnorm), else {}."""
    settings = {}
    state = path_or_state_dict
    if isinstance(state, (str, os.PathLike)):
        settings = {k: v for k, v in parse_upsampler_name(state).items() if k != "rotinv"}
        state = torch.load(state, map_location="cpu")
    if "state_dict" in state and not isinstance(state["state_dict"], torch.Tensor):
        state = state["state_dict"]
    if any(k.startswith(PREFIX) for k in state):
        state = {k[len(PREFIX):]: v for k, v in state.items() if k.startswith(PREFIX)}
    upsampler = get_upsampler("jbu_stack", num_features)
    upsampler.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=True)
    return upsampler.eval(), settings


def upsample_features(upsampler, features_lr, image, use_unitnorm=False, use_channelnorm=False, route="auto", differentiable=False,
                      **kwargs):
    """SDDINOFeatureExtractor.forward without the backbone (extractor.py:246-251): features_lr (B, C, h, w) from the 2D backbone, image
    (B, 3, H, W) the normalised image they were computed from -> features_hr (B, C, 16h, 16w).  route and kwargs (out_dtype=,
    memory_format=, chunk=) go to JBUStack.forward, and so does differentiable (with route="device": record the autograd graph, so that
    the upsampler can be trained or a loss on features_hr reach features_lr); another upsampler (Bilinear) is called as the reference
    calls it."""
    num_features = features_lr.shape[1]
    if use_unitnorm:
        features_lr = UnitNorm(num_features)(features_lr)
    if use_channelnorm:
        features_lr = ChannelNorm(num_features)(features_lr)
    if hasattr(upsampler, "up1"):
        return upsampler(features_lr, image, route=route, differentiable=differentiable, **kwargs)
    return upsampler(features_lr, image)


def load_aggre_net(path_or_state_dict, feature_dims=(640, 1280, 1280, 768), projection_dim=768, **kwargs):
    """AggregationNetwork(feature_dims, projection_dim) with a released best_<size>.PTH (SDDINO.py:29-31), loaded by the reference's rule
    (AggregationNetwork.load_pretrained_weights), in eval mode.  path_or_state_dict: the file or the state dict itself; kwargs: further constructor arguments."""
    state = path_or_state_dict
    if isinstance(state, (str, os.PathLike)):
        state = torch.load(state, map_location="cpu")
    net = AggregationNetwork(feature_dims=list(feature_dims), projection_dim=projection_dim, **kwargs)
    net.load_pretrained_weights(state)
    return net.eval()


def features_from_backbone(aggre_net, upsampler, s3, s4, s5, dino, image, num_rotations=4, rot_inv=False, use_unitnorm=False,
                           use_channelnorm=False, route="auto", **kwargs):
    """SDDINOFeatureExtractor.forward behind the two backbone calls: s3, s4, s5 (SD's decoder features), dino (the ViT's tokens as a
    (R B, C, P, P) view), R B images in rotation-major order with R = num_rotations when rot_inv, else 1 (featurizers.SDDINO.
    aggregate_features), and image (B, 3, H, W), the unrotated normalised images -> features_hr (B, C, 16 P, 16 P).  route goes to both
    stages, kwargs to upsample_features."""
    features_lr = aggregate_features(aggre_net, s3, s4, s5, dino, num_rotations=num_rotations, rot_inv=rot_inv, route=route)
    return upsample_features(upsampler, features_lr, image, use_unitnorm, use_channelnorm, route=route, **kwargs)

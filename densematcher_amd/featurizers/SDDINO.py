"""
densematcher.featurizers.SDDINO of the reference WITHOUT the backbones (SDDINO.py:35-90): what happens to the raw outputs of the frozen
SD-1.5 and DINOv2 models on their way to features_lr.  There is no SDDINOFeaturizer class here -- the backbones are third-party models
whose weights are not part of this package; a caller runs SD and hands over s3, s4, s5 (the UNet's decoder features).  dino (the ViT's
layer-11 tokens as a (B, C, P, P) view) comes from dino_features below: the DINOv2 encoder itself is featurizers.dinov2, with a
checkpoint the caller loads.

Routes of aggregate_features: 'torch' the reference's expressions (interpolate, cat, rotate, the network on torch), 'device' the HIP
path (MatchEngine.agg_gather + MatchEngine.aggregate: the concatenated and rotated intermediates are never stored), 'auto' as
AggregationNetwork.forward decides.
"""
import torch
import torch.nn.functional as F

from .. import _routes
from .modules import projection_network as pn
from .util import rotate


def dino_features(extractor_vit, img_batch01, num_patches, route="auto"):
    """SDDINO.py:49-51 (under the no_grad of SDDINO.py:44: the backbone is frozen): images (bs, 3, H, W) in [0, 1] -> resized to
    14 num_patches and normalised (extractor_vit.mean / std), the tokens of block 11 without the cls token, as (bs, D, P, P): a
    permuted view of the token buffer (the reference's reshape copies it), which aggregate_features reads where it lies.
    extractor_vit: a featup.model_utils.extractor_dino.ViTExtractor.  route: as DinoVisionTransformer.tokens; on the device route the
    resize and the normalisation happen while the patch rows are written."""
    P = int(num_patches)
    with torch.no_grad():
        model = extractor_vit.model
        if hasattr(model, "tokens_from_images"):
            desc = model.tokens_from_images(img_batch01, P, extractor_vit.mean, extractor_vit.std, layer=11, route=route)[:, 1:]
        else:                                                # another model under the hub's interface: the torch expressions only
            _routes.check(route, _routes.TORCH)
            if route == "device":
                raise ValueError("dino_features route='device': the model is not a featurizers.dinov2.DinoVisionTransformer")
            desc = extractor_vit.extract_descriptors(extractor_vit.resize_and_normalize(img_batch01, P * 14), layer=11, facet="token", route="torch")[:, 0]
    return desc.permute(0, 2, 1).unflatten(2, (P, P))


def gather_features(s3, s4, s5, dino, num_patches=None):
    """SDDINO.py:53-57: s4 and s5 interpolated (bilinear, align_corners=False) to the patch grid, then [s3, s4, s5, dino] side by side
    along the channels.  num_patches: the grid's side (None: s3's size)."""
    size = tuple(s3.shape[2:]) if num_patches is None else (int(num_patches), int(num_patches))
    up = lambda t: F.interpolate(t, size=size, mode="bilinear", align_corners=False)
    return torch.cat([s3, up(s4), up(s5), dino], dim=1)


def aggregate_features(aggre_net, s3, s4, s5, dino, num_rotations=1, rot_inv=False, route="auto"):
    """get_features (rot_inv=False) / get_rotinv_features (rot_inv=True) behind the backbone calls.  The sources hold R B images in the
    reference's order, torch.cat(images, 0) with images[r] = rotate(image, r 360 / R): rotation-major; R = num_rotations with rot_inv,
    else 1.  dino (R B, C, P, P) in any strides: the permuted view of a token tensor is read where it lies.  Returns
    (B, projection_dim, P, P); on the device route NCHW-shaped over channels-last memory."""
    R = int(num_rotations) if rot_inv else 1
    if R < 1 or s3.shape[0] % R or any(t.shape[0] != s3.shape[0] for t in (s4, s5, dino)):
        raise ValueError(f"aggregate_features: every source needs the same number of images, a multiple of the {R} rotations")
    size = tuple(s3.shape[2:])
    if tuple(dino.shape[2:]) != size:
        raise ValueError(f"aggregate_features: dino {tuple(dino.shape[2:])} is not on s3's patch grid {size}")
    step = 360.0 / R if rot_inv else 0.0
    if pn.route_of(aggre_net, route, (s3, s4, s5, dino)) == "device":
        eng = _routes.engine_or_none()
        rows = eng.agg_gather([s3, s4, s5, dino], num_rotations=R, step_deg=step, size=size)
        return eng.aggregate(aggre_net.packed(eng.device), rows, *size)
    gathered = gather_features(s3.float(), s4.float(), s5.float(), dino.float())
    if rot_inv:
        parts = gathered.chunk(R, dim=0)
        fused = torch.zeros_like(parts[0])
        for r in range(R):
            fused += rotate(parts[r], -r * step)
        gathered = fused / R
    return aggre_net(gathered, route="torch")

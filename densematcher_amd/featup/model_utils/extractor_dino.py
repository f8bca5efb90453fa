"""
featup.model_utils.extractor_dino of the reference (third_party/featup/featup/model_utils/extractor_dino.py): ViTExtractor, the wrapper
through which SDDINO.py:27, 49-51 reaches the DINOv2 ViT, restated under its names and argument order -- resize_and_normalize,
extract_descriptors(batch, layer=11, facet='key', bin=False, include_cls=False), the attributes p, stride, mean, std, model.

What is built: the descriptors of the facets 'token' (both routes) and 'key' / 'query' / 'value' (torch route, through forward hooks on
model.blocks[layer].attn as extractor_dino.py:192-232).  What is not, each refused by name: creating a model (this package never fetches
one: pass model=featurizers.dinov2.load_dinov2(path, name)), a stride other than the patch size (extractor_dino.py:130-151 patches the
convolution's stride; the kernels are built for stride 14), bin=True (extractor_dino.py:262-308), saliency maps (:336-350) and the
image-file preprocess (:153-179).
"""
import torch
import torch.nn.functional as F
from torch import nn

from ... import _routes

FACETS = ("key", "query", "value", "token")


class ViTExtractor(nn.Module):
    def __init__(self, model_type="dinov2_vitb14", stride=14, model=None):
        super().__init__()
        if model is None:
            raise ValueError("ViTExtractor: model=None would fetch a model from a hub, which this package never does: pass "
                             "model=densematcher_amd.featurizers.dinov2.load_dinov2(path_or_state_dict, name) with a checkpoint of your own")
        self.model_type = model_type
        self.model = model
        self.model.eval()
        p = self.model.patch_embed.patch_size
        self.p = p[0] if isinstance(p, tuple) else p
        if int(stride) != self.p:
            raise ValueError(f"ViTExtractor: stride {stride} is not the patch size {self.p}: overlapping patches are not built")
        self.stride = self.model.patch_embed.proj.stride
        dino = "dino" in self.model_type
        self.mean = (0.485, 0.456, 0.406) if dino else (0.5, 0.5, 0.5)
        self.std = (0.229, 0.224, 0.225) if dino else (0.5, 0.5, 0.5)
        self.load_size = None
        self.num_patches = None

    def resize_and_normalize(self, image_tensor, size):
        """image_tensor (bs, C, H, W) float -> resized (bilinear, align_corners=False) to (size, size), (x - mean) / std"""
        x = F.interpolate(image_tensor, size=(size, size), mode="bilinear", align_corners=False)
        m, s = (torch.as_tensor(v, dtype=x.dtype, device=x.device).view(1, -1, 1, 1) for v in (self.mean, self.std))
        return (x - m) / s

    def preprocess(self, image_path, load_size=None, patch_size=14):
        raise NotImplementedError("ViTExtractor.preprocess reads and resamples an image file with PIL (LANCZOS), which is outside this "
                                  "package: load the image yourself and call resize_and_normalize")

    def extract_saliency_maps(self, batch):
        raise NotImplementedError("ViTExtractor.extract_saliency_maps: the reference builds them for dino_vits8 only and DenseMatcher never "
                                  "calls them; not built")

    def _hooked(self, batch, layer, facet):
        """Forward hooks as extractor_dino.py:192-232, for any model under the hub's interface: 'token' records the output of
        model.blocks[layer] (B, t, D); key / query / value hook the block's attention module and recompute qkv from its input as
        :210-215, (B, h, t, d)"""
        feats = []

        def token_hook(module, inputs, output):
            feats.append(output)

        def qkv_hook(module, inputs, output):
            x = inputs[0]
            B, N, C = x.shape
            idx = {"query": 0, "key": 1, "value": 2}[facet]
            feats.append(module.qkv(x).reshape(B, N, 3, module.num_heads, C // module.num_heads).permute(2, 0, 3, 1, 4)[idx])

        block = self.model.blocks[layer]
        handle = block.register_forward_hook(token_hook) if facet == "token" else block.attn.register_forward_hook(qkv_hook)
        try:
            self.model(batch)
        finally:
            handle.remove()
        return feats[0]

    def extract_descriptors(self, batch, layer=11, facet="key", bin=False, include_cls=False, route="auto"):
        """batch (B, 3, H, W), normalised -> (B, 1, t, d'): facet 'token' the output of block `layer` (d' = D), 'key' | 'query' | 'value'
        in the reference's layout (d' = d h, index d * heads + head); without the cls token unless include_cls.  route: 'token' runs on
        either route of the model; the other facets on the torch route only."""
        if facet not in FACETS:
            raise ValueError(f"{facet} is not a supported facet for descriptors. choose from ['key' | 'query' | 'value' | 'token']")
        if bin:
            raise NotImplementedError("ViTExtractor.extract_descriptors: bin=True (the log-binned descriptor) is not built; DenseMatcher calls "
                                      "it with bin=False")
        _routes.check(route, _routes.TORCH)
        H, W = batch.shape[2:]
        if facet == "token" and hasattr(self.model, "tokens"):                            # featurizers.dinov2: stops at `layer`, either route
            x = self.model.tokens(batch, layer=layer, route=route).unsqueeze(1)          # (B, 1, t, D)
        else:
            if route == "device":
                raise ValueError(f"ViTExtractor.extract_descriptors route='device': facet {facet!r} of a {type(self.model).__name__} is built on "
                                 "the torch route only (the device route serves 'token' of a featurizers.dinov2.DinoVisionTransformer)")
            x = self._hooked(batch, layer, facet)                                         # (B, h, t, d), or (B, t, D)
            x = x.unsqueeze(1) if facet == "token" else x
        self.load_size = (H, W)
        self.num_patches = (1 + (H - self.p) // self.stride[0], 1 + (W - self.p) // self.stride[1])
        if not include_cls:
            x = x[:, :, 1:, :]
        return x.permute(0, 2, 3, 1).flatten(start_dim=-2, end_dim=-1).unsqueeze(dim=1)

"""
The DINOv2 ViT encoder behind the reference's `dino` tokens (SDDINO.py:27 builds ViTExtractor('dinov2_vitb14', stride=14) and
SDDINO.py:49-51 takes the output of block 11): DinoVisionTransformer, a plain nn.Module that restates the encoder under the hub model's
state_dict keys -- a released dinov2_vit{s,b,l}14_pretrain.pth loads with strict=True (load_dinov2).  This package never fetches a model.

Architecture: Conv2d 14 x 14 / stride 14 patch embedding, cls token, positional table, pre-norm residual blocks with LayerScale
(x + ls1(attn(norm1 x)), then x + ls2(mlp(norm2 x))), LayerNorm eps 1e-6, exact (erf) GELU, qkv split q | k | v with the heads adjacent
within each, head dimension 64, scores scaled by 64^-1/2, no register tokens.

Positional embedding of a P x P grid: the bicubic resampling of the stored 37 x 37 table by the rule written at the reference's
third_party/featup/featup/model_utils/extractor_dino.py:101-125 (scale factor (P + 0.1) / 37, align_corners=False,
recompute_scale_factor=False; the stored table itself at P = 37), computed once per P with F.interpolate and cached; both routes read the
same tensor.  NOT pinned against the hub model's own interpolate_pos_encoding, which is not available here: this one detail is restated
from the reference's local copy of the rule.

Routes (tokens(..., route=), the TORCH vocabulary of _routes):
  torch    the expressions above on PyTorch: any dtype, any device, autograd.
  device   inference in HIP (MatchEngine.vit_tokens: dm_vit_patch_rows_f16, dm_vit_layernorm_f16, dm_vit_linear_f16,
           dm_vit_attention_f16): fp16 operands on the matrix cores, fp32 accumulation, fp32 residual stream; an image's bits do not
           depend on the batch.  Refused with ValueError for a tensor that requires grad, a head dimension other than 64, a non-square
           input, a side that is not a multiple of 14, operands not on the GPU; RuntimeError without a GPU.
  auto     the device route where its conditions hold and tools/vit_time.py measured it not slower than the torch route in fp16
           (AUTO_DEVICE), else torch.
"""
import types

import torch
import torch.nn.functional as F
from torch import nn

from .. import _routes

# whether tools/vit_time.py measured the device route not slower than the torch route of the same process in fp16 on an MI355X
# (README.md): 6.75 ms against 4.94 ms (ViT-B/14, 20 images, P = 24, layer 11; fp32 torch 26.8 ms), so 'auto'
# stays on torch; route="device" has half the fp16 route's error and bits that do not depend on the batch
AUTO_DEVICE = False

PATCH, TABLE_SIDE, HEAD_DIM = 14, 37, 64
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.patch_size = (PATCH, PATCH)
        self.proj = nn.Conv2d(3, dim, kernel_size=PATCH, stride=PATCH)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class Attention(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.sdpa = False            # tools/vit_time.py: the torch route through F.scaled_dot_product_attention

    def forward(self, x):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        if self.sdpa:
            out = F.scaled_dot_product_attention(q, k, v, scale=self.scale)
        else:
            out = ((q * self.scale) @ k.transpose(-2, -1)).softmax(dim=-1) @ v
        return self.proj(out.transpose(1, 2).reshape(B, N, C))


class LayerScale(nn.Module):
    def __init__(self, dim, init_values=1.0):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads)
        self.ls1 = LayerScale(dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.ls2 = LayerScale(dim)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class PackedViT:
    """what MatchEngine.vit_tokens reads of a DinoVisionTransformer on the device: the weights rounded once to fp16 (w_patch (D, 640):
    Conv2d's flattening c 196 + dy 14 + dx, zero-padded to the GEMM's granule), biases, LayerScale gammas and LayerNorm parameters in
    fp32, and pos(P): the (1 + P P, D) fp32 positional table of a P x P grid with the constant cls row (cls_token + pos_embed[0]) in
    row 0"""

    def __init__(self, model, device):
        from .._engine_vit import VIT_PATCH_K, vit_pad_k
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        f16 = lambda t: t.detach().to(device=device, dtype=torch.float32).to(torch.float16).contiguous()
        self.model, self.device = model, device
        self.dim, self.heads, self.hidden = model.embed_dim, model.num_heads, model.blocks[0].mlp.fc1.out_features
        w = torch.zeros((self.dim, vit_pad_k(VIT_PATCH_K)), dtype=torch.float16, device=device)
        w[:, :VIT_PATCH_K] = f16(model.patch_embed.proj.weight.reshape(self.dim, VIT_PATCH_K))
        self.w_patch, self.b_patch = w, f32(model.patch_embed.proj.bias)
        self.blocks = [types.SimpleNamespace(
            g1=f32(b.norm1.weight), b1=f32(b.norm1.bias), w_qkv=f16(b.attn.qkv.weight), b_qkv=f32(b.attn.qkv.bias),
            w_proj=f16(b.attn.proj.weight), b_proj=f32(b.attn.proj.bias), ls1=f32(b.ls1.gamma),
            g2=f32(b.norm2.weight), b2=f32(b.norm2.bias), w_fc1=f16(b.mlp.fc1.weight), b_fc1=f32(b.mlp.fc1.bias),
            w_fc2=f16(b.mlp.fc2.weight), b_fc2=f32(b.mlp.fc2.bias), ls2=f32(b.ls2.gamma)) for b in model.blocks]
        self.g_norm, self.b_norm = f32(model.norm.weight), f32(model.norm.bias)
        self._pos = {}

    def pos(self, P):
        if P not in self._pos:
            with torch.no_grad():
                table = self.model.pos_table(P).detach().to(device=self.device, dtype=torch.float32)[0].clone()
                table[0] += self.model.cls_token.detach().to(device=self.device, dtype=torch.float32)[0, 0]
            self._pos[P] = table.contiguous()
        return self._pos[P]


class DinoVisionTransformer(nn.Module):
    def __init__(self, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0):
        super().__init__()
        self.embed_dim, self.num_heads, self.patch_size = embed_dim, num_heads, PATCH
        self.patch_embed = PatchEmbed(embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + TABLE_SIDE * TABLE_SIDE, embed_dim))
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))          # part of the released state dict; inference never reads it
        self.blocks = nn.ModuleList(Block(embed_dim, num_heads, mlp_ratio) for _ in range(depth))
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self._tables, self._packed = {}, None

    # ------------------------------------------------------------------ positional table
    def _stamp(self):
        return tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in self.parameters())

    def pos_table(self, P):
        """(1, 1 + P P, D): pos_embed resampled to a P x P grid by the rule of extractor_dino.py:101-125, in pos_embed's dtype and on
        its device; computed once per P (and per state of pos_embed) and cached.  The stored table itself at P = 37."""
        P = int(P)
        if P == TABLE_SIDE:
            return self.pos_embed
        key = (P, self.pos_embed.data_ptr(), self.pos_embed._version, self.pos_embed.dtype, self.pos_embed.device)
        recorded = torch.is_grad_enabled() and self.pos_embed.requires_grad      # a table with an autograd graph is not kept
        if recorded or key not in self._tables:
            if len(self._tables) > 16:
                self._tables.clear()
            dim = self.pos_embed.shape[-1]
            side = P + 0.1                                   # "a small number to avoid floating point error in the interpolation"
            grid = self.pos_embed[:, 1:].reshape(1, TABLE_SIDE, TABLE_SIDE, dim).permute(0, 3, 1, 2)
            grid = F.interpolate(grid, scale_factor=(side / TABLE_SIDE, side / TABLE_SIDE), mode="bicubic", align_corners=False,
                                 recompute_scale_factor=False)
            if tuple(grid.shape[-2:]) != (P, P):
                raise RuntimeError(f"positional table: expected a {P} x {P} grid, got {tuple(grid.shape[-2:])}")
            table = torch.cat((self.pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, P * P, dim)), dim=1)
            if recorded:
                return table
            self._tables[key] = table
        return self._tables[key]

    def interpolate_pos_encoding(self, x, w, h):
        """the hub model's method name: x (n, 1 + P P, D) tokens of a w x h image -> the positional table in x's dtype"""
        if w != h or x.shape[1] - 1 != (w // PATCH) ** 2:
            raise ValueError(f"interpolate_pos_encoding: square inputs with (side / 14)^2 patches only, got {w} x {h} and {x.shape[1] - 1} patches")
        return self.pos_table(w // PATCH).to(x.dtype)

    # ------------------------------------------------------------------ torch route
    def prepare_tokens(self, x):
        n, _, w, h = x.shape
        x = self.patch_embed(x)
        x = torch.cat((self.cls_token.expand(n, -1, -1), x), dim=1)
        return x + self.interpolate_pos_encoding(x, w, h)

    def _tokens_torch(self, x, layer, norm):
        x = self.prepare_tokens(x)
        for blk in self.blocks[:layer + 1]:
            x = blk(x)
        return self.norm(x) if norm else x

    # ------------------------------------------------------------------ device route
    def device_obstacle(self, x, side=None):
        """why the device route cannot run this call, or None; side: the side the kernel resizes x to (None: x's own)"""
        if self.embed_dim != HEAD_DIM * self.num_heads:
            return f"head dimension {self.embed_dim // self.num_heads} (the attention kernel is built for 64)"
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            return f"a non-square input {tuple(x.shape)} (the kernels take (n, 3, S, S))"
        side = x.shape[2] if side is None else side
        if side % PATCH or side <= 0:
            return f"a side of {side} is not a multiple of {PATCH}"
        why = _routes.grad_obstacle([x] + list(self.parameters()))
        if why is not None:
            return why
        if torch.cuda.is_available() and not (x.is_cuda and all(p.is_cuda for p in self.parameters())):
            return "operands not on the GPU (move the module and the images to the device)"
        return None

    def route_of(self, route, x, side=None):
        """'torch' or 'device' for a call on x: what this module hands to the one picker"""
        on_gpu = lambda: x.is_cuda and all(p.is_cuda for p in self.parameters())
        return _routes.pick_torch(route, "DinoVisionTransformer", lambda: self.device_obstacle(x, side), AUTO_DEVICE, on_gpu)

    def packed(self, device):
        """the device-side weight blocks (PackedViT) on `device`, rebuilt when a parameter changed"""
        stamp = (torch.device(device),) + self._stamp()
        if self._packed is None or self._packed[0] != stamp:
            with torch.no_grad():
                self._packed = (stamp, PackedViT(self, torch.device(device)))
        return self._packed[1]

    def _layer(self, layer):
        layer = len(self.blocks) - 1 if layer is None else int(layer)
        if not 0 <= layer < len(self.blocks):
            raise ValueError(f"layer {layer} outside the {len(self.blocks)} blocks")
        return layer

    # ------------------------------------------------------------------ public
    def tokens(self, x, layer=None, norm=False, route="auto"):
        """x (n, 3, 14 P, 14 P), normalised -> (n, 1 + P P, D): the output of block `layer` (None: the last), what a forward hook on
        model.blocks[layer] records; norm: the final LayerNorm applied.  The device route returns fp32."""
        layer = self._layer(layer)
        if self.route_of(route, x) == "torch":
            return self._tokens_torch(x, layer, norm)
        eng = _routes.engine_or_none()
        return eng.vit_tokens(self.packed(eng.device), x, x.shape[2] // PATCH, layer, norm=norm, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))

    def tokens_from_images(self, images, num_patches, mean=IMAGENET_MEAN, std=IMAGENET_STD, layer=None, norm=False, route="auto"):
        """images (n, 3, S, S) in [0, 1] -> tokens of the images resized (bilinear, align_corners=False) to 14 num_patches and
        normalised with mean / std (extractor_dino.py:181-190 in front of tokens()).  On the device route the resize and the
        normalisation happen while the patch rows are written."""
        layer, P = self._layer(layer), int(num_patches)
        if self.route_of(route, images, side=PATCH * P) == "torch":
            x = F.interpolate(images, size=(PATCH * P, PATCH * P), mode="bilinear", align_corners=False)
            m, s = (torch.as_tensor(v, dtype=x.dtype, device=x.device).view(1, 3, 1, 1) for v in (mean, std))
            return self._tokens_torch((x - m) / s, layer, norm)
        eng = _routes.engine_or_none()
        return eng.vit_tokens(self.packed(eng.device), images, P, layer, norm=norm, mean=mean, std=std)

    def forward(self, x):
        """the normalised cls token (n, D), as the hub model's forward with its identity head"""
        return self._tokens_torch(x, len(self.blocks) - 1, True)[:, 0]


def dinov2_vits14():
    return DinoVisionTransformer(384, 12, 6)


def dinov2_vitb14():
    return DinoVisionTransformer(768, 12, 12)


def dinov2_vitl14():
    return DinoVisionTransformer(1024, 24, 16)


FACTORIES = {"dinov2_vits14": dinov2_vits14, "dinov2_vitb14": dinov2_vitb14, "dinov2_vitl14": dinov2_vitl14}


def load_dinov2(path_or_state_dict, name="dinov2_vitb14"):
    """A DinoVisionTransformer with the weights of a released checkpoint (a path for torch.load, or the state dict itself), loaded with
    strict=True, in eval mode.  The file comes from the caller: nothing is downloaded."""
    if name not in FACTORIES:
        raise ValueError(f"load_dinov2: name must be one of {sorted(FACTORIES)}, not {name!r}")
    state = path_or_state_dict
    if not isinstance(state, dict):
        state = torch.load(state, map_location="cpu")
    model = FACTORIES[name]()
    model.load_state_dict(state, strict=True)
    return model.eval()

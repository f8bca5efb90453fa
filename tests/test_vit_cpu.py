"""CPU: the DINOv2 encoder of densematcher_amd.featurizers.dinov2, its ViTExtractor surface and dino_features -- the state dict's keys,
the torch route against an independent composition from nn.MultiheadAttention / nn.LayerNorm / F.gelu / nn.Conv2d in float64, the
positional table against the formula of extractor_dino.py:101-125 evaluated directly, the float64 restatement tests/vit_restate.py
against the torch route, the ABI entries without a GPU and the routes."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import vit_restate as vr
from densematcher_amd.featup.model_utils.extractor_dino import ViTExtractor
from densematcher_amd.featurizers import dino_features
from densematcher_amd.featurizers import dinov2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dm_vit_patch_rows_f16", "dm_vit_layernorm_f16", "dm_vit_linear_f16", "dm_vit_attention_f16")
FACTORY_SIZES = {"dinov2_vits14": (384, 12, 6), "dinov2_vitb14": (768, 12, 12), "dinov2_vitl14": (1024, 24, 16)}


def small_model(dim=128, depth=2, heads=2, seed=3, dtype=torch.float64):
    m = dinov2.DinoVisionTransformer(dim, depth, heads)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vr.seeded_state(dim, depth, seed).items()}, strict=True)
    return m.to(dtype).eval()


@pytest.fixture(scope="module")
def model():
    return small_model()


@pytest.fixture(scope="module")
def images():
    return torch.from_numpy(np.random.default_rng(11).normal(0, 1, (2, 3, 42, 42)))


# ---------------------------------------------------------------------------------------------------------------- loading
@pytest.mark.parametrize("name", sorted(FACTORY_SIZES))
def test_state_dict_with_the_hub_keys_loads_strict(name):
    dim, depth, heads = FACTORY_SIZES[name]
    keys = vr.state_dict_keys(dim, depth)
    with torch.device("meta"):                                         # shapes and names only: nothing of this size is allocated
        m = dinov2.FACTORIES[name]()
        m.load_state_dict({k: torch.empty(shape) for k, shape in keys.items()}, strict=True)
    assert set(m.state_dict()) == set(keys)
    assert all(tuple(m.state_dict()[k].shape) == shape for k, shape in keys.items())
    assert (m.embed_dim, len(m.blocks), m.num_heads) == (dim, depth, heads) and dim // heads == 64
    if name == "dinov2_vits14":                                        # one real load through load_dinov2 (the smallest of the three)
        state = {k: torch.full(shape, 0.25) for k, shape in keys.items()}
        loaded = dinov2.load_dinov2(state, name)
        assert not loaded.training and loaded.blocks[11].ls2.gamma[0].item() == 0.25
        with pytest.raises(RuntimeError):
            dinov2.load_dinov2({k: v for k, v in state.items() if k != "mask_token"}, name)
    with pytest.raises(ValueError):
        dinov2.load_dinov2({}, "dinov2_vitg14")


def test_hub_attributes(model):
    assert model.patch_embed.patch_size == (14, 14) and model.patch_embed.proj.stride == (14, 14)
    assert callable(model.interpolate_pos_encoding) and len(model.blocks) == 2
    assert all(m.eps == 1e-6 for m in model.modules() if isinstance(m, nn.LayerNorm))


# ---------------------------------------------------------------------------------------------------------------- torch route
def independent_forward(m, x, layer, norm):
    """the encoder composed from torch's own modules in float64: nn.Conv2d, nn.MultiheadAttention (in_proj_weight = qkv.weight: its
    q | k | v split, its head split, its 1 / sqrt(d) scale), nn.LayerNorm, F.gelu"""
    D, H = m.embed_dim, m.num_heads
    conv = nn.Conv2d(3, D, 14, 14).double()
    conv.weight.data, conv.bias.data = m.patch_embed.proj.weight.data, m.patch_embed.proj.bias.data
    tok = conv(x).flatten(2).transpose(1, 2)
    tok = torch.cat([m.cls_token.expand(len(x), -1, -1), tok], 1) + m.pos_table(x.shape[-1] // 14)
    for blk in list(m.blocks)[:layer + 1]:
        mha = nn.MultiheadAttention(D, H, batch_first=True).double()
        mha.in_proj_weight.data, mha.in_proj_bias.data = blk.attn.qkv.weight.data, blk.attn.qkv.bias.data
        mha.out_proj.weight.data, mha.out_proj.bias.data = blk.attn.proj.weight.data, blk.attn.proj.bias.data
        ln1, ln2 = nn.LayerNorm(D, eps=1e-6).double(), nn.LayerNorm(D, eps=1e-6).double()
        ln1.weight.data, ln1.bias.data, ln2.weight.data, ln2.bias.data = blk.norm1.weight.data, blk.norm1.bias.data, blk.norm2.weight.data, blk.norm2.bias.data
        h = ln1(tok)
        tok = tok + blk.ls1.gamma * mha(h, h, h, need_weights=False)[0]
        h = ln2(tok)
        tok = tok + blk.ls2.gamma * F.linear(F.gelu(F.linear(h, blk.mlp.fc1.weight, blk.mlp.fc1.bias)), blk.mlp.fc2.weight, blk.mlp.fc2.bias)
    return F.layer_norm(tok, (D,), m.norm.weight, m.norm.bias, 1e-6) if norm else tok


@pytest.mark.parametrize("layer,norm", [(0, False), (1, False), (1, True)])
def test_torch_route_against_an_independent_composition(model, images, layer, norm):
    with torch.no_grad():
        got = model.tokens(images, layer=layer, norm=norm, route="torch")
        want = independent_forward(model, images, layer, norm)
        auto = model.tokens(images, layer=layer, norm=norm)                # no GPU tensors (or AUTO_DEVICE off): the torch route
    assert got.shape == (2, 10, 128) and got.dtype == torch.float64
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    if not images.is_cuda:
        assert torch.equal(got, auto)


def test_layer_is_the_unnormed_block_output_and_forward_the_normed_cls(model, images):
    rec = []
    h = model.blocks[1].register_forward_hook(lambda mod, i, o: rec.append(o))
    with torch.no_grad():
        cls = model(images)
        last = model.tokens(images, route="torch")
    h.remove()
    assert torch.equal(rec[0], last) and torch.equal(last, model.tokens(images, layer=1, route="torch"))
    assert torch.equal(cls, F.layer_norm(last, (128,), model.norm.weight, model.norm.bias, 1e-6)[:, 0])
    with pytest.raises(ValueError):
        model.tokens(images, layer=2, route="torch")


def test_restatement_against_the_torch_route(model, images):
    params = {k: v.numpy() for k, v in model.state_dict().items()}
    with torch.no_grad():
        for layer, norm in ((0, False), (1, True)):
            want = model.tokens(images, layer=layer, norm=norm, route="torch").numpy()
            got = vr.forward(params, images.numpy(), model.pos_table(3)[0].numpy(), 2, layer=layer, norm=norm)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the seeded weights do what vit_restate.seeded_state says: the softmax is not flat
    tok0 = vr.forward(params, images.numpy(), model.pos_table(3)[0].detach().numpy(), 2, layer=0)
    qkv = vr.linear(vr.layernorm(tok0, params["blocks.1.norm1.weight"], params["blocks.1.norm1.bias"]), params["blocks.1.attn.qkv.weight"],
                    params["blocks.1.attn.qkv.bias"])
    q, k, _ = vr.split_heads(qkv, 2)
    s = (q / 8) @ k.transpose(0, 1, 3, 2)
    p = np.exp(s - s.max(-1, keepdims=True))
    assert (p / p.sum(-1, keepdims=True)).max(-1).mean() > 0.3


# ---------------------------------------------------------------------------------------------------------------- positional table
def test_positional_table_is_the_reference_formula(model):
    N = model.pos_embed.shape[1] - 1
    M = int(math.sqrt(N))
    assert M == 37
    torch.set_grad_enabled(False)                                       # (a table that carries an autograd graph is not kept)
    for P in (3, 8, 24):
        w0 = h0 = P + 0.1
        grid = F.interpolate(model.pos_embed[:, 1:].reshape(1, M, M, 128).permute(0, 3, 1, 2), scale_factor=(w0 / math.sqrt(N), h0 / math.sqrt(N)),
                             mode="bicubic", align_corners=False, recompute_scale_factor=False)
        assert int(w0) == grid.shape[-2] and int(h0) == grid.shape[-1]
        want = torch.cat((model.pos_embed[:, 0].unsqueeze(0), grid.permute(0, 2, 3, 1).reshape(1, -1, 128)), dim=1)
        got = model.pos_table(P)
        assert torch.equal(got, want) and got.shape == (1, 1 + P * P, 128)
        assert model.pos_table(P) is got                                 # computed once per P
        x = torch.zeros(1, 1 + P * P, 128, dtype=torch.float64)
        assert torch.equal(model.interpolate_pos_encoding(x, 14 * P, 14 * P), want)
    torch.set_grad_enabled(True)
    assert model.pos_table(37) is model.pos_embed                         # the stored table itself
    assert model.pos_table(3) is not model.pos_table(3) and model.pos_table(3).requires_grad
    with pytest.raises(ValueError):
        model.interpolate_pos_encoding(torch.zeros(1, 7, 128), 28, 42)


# ---------------------------------------------------------------------------------------------------------------- extractor, dino_features
def test_extractor_surface_and_shapes(model, images):
    ex = ViTExtractor("dinov2_vitb14", stride=14, model=model)
    assert ex.p == 14 and ex.stride == (14, 14) and ex.mean == (0.485, 0.456, 0.406) and ex.std == (0.229, 0.224, 0.225) and ex.model is model
    with torch.no_grad():
        tok = ex.extract_descriptors(images, layer=1, facet="token")
        tok_cls = ex.extract_descriptors(images, 1, "token", False, True)
        key = ex.extract_descriptors(images, layer=1)                      # facet='key' is the default
        want = model.tokens(images, layer=1, route="torch")
        h = model.blocks[1].norm1(model.tokens(images, layer=0, route="torch"))
        k_want = model.blocks[1].attn.qkv(h)[:, :, 128:256]                  # the k third; the reference's layout is index d * heads + head
        k_want = k_want.reshape(2, 10, 2, 64).permute(0, 1, 3, 2).flatten(-2)
    assert tok.shape == (2, 1, 9, 128) and tok_cls.shape == (2, 1, 10, 128) and key.shape == (2, 1, 9, 128)
    assert torch.equal(tok[:, 0], want[:, 1:]) and torch.equal(tok_cls[:, 0], want)
    assert (key[:, 0] - k_want[:, 1:]).abs().max() <= 1e-12
    assert ex.num_patches == (3, 3) and ex.load_size == (42, 42)
    with pytest.raises(ValueError, match="load_dinov2"):
        ViTExtractor("dinov2_vitb14", stride=14)
    with pytest.raises(ValueError, match="stride"):
        ViTExtractor("dinov2_vitb14", stride=7, model=model)
    with pytest.raises(NotImplementedError):
        ex.extract_descriptors(images, bin=True)
    with pytest.raises(NotImplementedError):
        ex.extract_saliency_maps(images)
    with pytest.raises(NotImplementedError):
        ex.preprocess("image.png")
    with pytest.raises(ValueError, match="torch route only"):
        ex.extract_descriptors(images, facet="key", route="device")
    with pytest.raises(ValueError):
        ex.extract_descriptors(images, facet="attn")


def test_dino_features_is_the_three_lines_of_the_reference():
    m = small_model(depth=12, seed=5)
    ex = ViTExtractor("dinov2_vitb14", stride=14, model=m)
    img = torch.from_numpy(np.random.default_rng(2).uniform(0, 1, (2, 3, 48, 48)))
    bs, P = 2, 3
    got = dino_features(ex, img, P, route="torch")
    with torch.no_grad():
        x = F.interpolate(img, size=(P * 14, P * 14), mode="bilinear", align_corners=False)
        x = (x - torch.tensor(ex.mean, dtype=x.dtype).view(1, 3, 1, 1)) / torch.tensor(ex.std, dtype=x.dtype).view(1, 3, 1, 1)
        assert torch.equal(x, ex.resize_and_normalize(img, P * 14))
        feats = m.tokens(x, layer=11, route="torch")[:, 1:].unsqueeze(1)                       # (bs, 1, t - 1, D)
        want = feats.permute(0, 1, 3, 2).reshape(bs, -1, P, P)
    assert got.shape == (2, 128, 3, 3) and torch.equal(got, want)
    assert got.stride(1) == 1 and not got.requires_grad                  # a permuted view of the token buffer, computed under no_grad
    assert torch.equal(got, dino_features(ex, img, P))                    # auto without a GPU tensor


def test_a_model_without_tokens_goes_through_forward_hooks():
    class Foreign(nn.Module):                                           # the hub's interface only: patch_embed, blocks, forward
        def __init__(self, inner):
            super().__init__()
            self.inner, self.patch_embed, self.blocks = inner, inner.patch_embed, inner.blocks

        def forward(self, x):
            return self.inner(x)

    m = small_model(depth=12, seed=5)
    ex, own = ViTExtractor("dinov2_vitb14", model=Foreign(m)), ViTExtractor("dinov2_vitb14", model=m)
    img = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (1, 3, 30, 30)))
    with torch.no_grad():
        batch = ex.resize_and_normalize(img, 28)
        assert torch.equal(ex.extract_descriptors(batch, facet="token"), own.extract_descriptors(batch, facet="token"))
    assert torch.equal(dino_features(ex, img, 2), dino_features(own, img, 2))
    with pytest.raises(ValueError, match="torch route only"):
        ex.extract_descriptors(batch, facet="token", route="device")
    with pytest.raises(ValueError, match="not a featurizers.dinov2"):
        dino_features(ex, img, 2, route="device")


# ---------------------------------------------------------------------------------------------------------------- ABI and routes
@pytest.fixture(scope="module")
def lib():
    from densematcher_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_new_symbols_declared_bound_and_exported(lib):
    from densematcher_amd import _build, _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "densematch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in _lib.SIGNATURES and name in declared and hasattr(lib, name), name
    assert "dm_vit.hip" in _build.SOURCES
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [15, 10, 20, 11]
    from densematcher_amd.engine import MatchEngine
    assert all(hasattr(MatchEngine, n) for n in ("vit_patch_rows", "vit_layernorm", "vit_linear", "vit_attention", "vit_tokens"))


def test_bad_arguments_are_refused_without_a_gpu(lib):
    import ctypes as C
    three = (C.c_double * 3)(0.5, 0.5, 0.5)
    assert lib.dm_vit_patch_rows_f16(None, 1, 14, 1, 1, None, 0, 0, 0, 0, three, three, 640, None, 640) != 0
    assert lib.dm_vit_layernorm_f16(None, 0, 64, None, 64, None, None, 0, None, 64) != 0
    assert lib.dm_vit_linear_f16(None, 1, 1, 8, 60, None, 60, 0, None, 60, None, None, None, 0, 0, 0, 1, None, 8, 0) != 0
    assert lib.dm_vit_attention_f16(None, 1, 2, 1, 32, None, 96, 0, None, 32, 0) != 0


def test_device_route_without_a_gpu_is_the_runtime_error_of_routes(model, images):
    from densematcher_amd import _routes
    if torch.cuda.is_available():                                      # with a GPU the same call names its obstacle instead (test_gpu_vit.py)
        return
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=re.escape(_routes.NO_GPU)):
            model.tokens(images, route="device")
        with pytest.raises(RuntimeError, match=re.escape(_routes.NO_GPU)):
            dino_features(ViTExtractor("dinov2_vitb14", model=small_model(depth=12)), images, 3, route="device")
    with pytest.raises(ValueError, match="route must be"):
        model.tokens(images, route="host")


def test_device_obstacles_are_stated_by_name(model, images):
    with torch.no_grad():
        with pytest.raises(ValueError, match="non-square"):
            model.tokens(images[:, :, :28], route="device")
        with pytest.raises(ValueError, match="not a multiple of 14"):
            model.tokens(torch.zeros(1, 3, 40, 40, dtype=torch.float64), route="device")
        odd = dinov2.DinoVisionTransformer(96, 1, 2).eval()
        with pytest.raises(ValueError, match="head dimension 48"):
            odd.tokens(torch.zeros(1, 3, 14, 14), route="device")
    with pytest.raises(ValueError, match="requires grad"):
        model.tokens(images, route="device")
    assert dinov2.AUTO_DEVICE in (True, False)

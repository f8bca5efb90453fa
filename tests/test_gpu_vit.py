"""The DINOv2 encoder on the GPU (dm_vit_patch_rows_f16, dm_vit_layernorm_f16, dm_vit_linear_f16, dm_vit_attention_f16,
MatchEngine.vit_tokens, the device route of featurizers.dinov2, ViTExtractor and dino_features) against the float64 restatement
tests/vit_restate.py and its derived bounds.

Inputs are fp16-representable wherever a kernel takes fp16, so that a comparison measures the kernel and not the rounding of its inputs.
Shapes.  linear: the kernel's tile is 128 x 128 outputs and its granule 64 contraction indices; M in {1, 127, 128, 129, 577},
N in {8, 129, 2304}, K in {64, 640 (588 padded), 3072}: one product per K at the largest M and N, every case a block of it.
attention: queries in tiles of 128, keys staged in tiles of 64 and multiplied in halves of 32; T in {2, 31, 32, 33, 63, 64, 65, 127, 128,
129, 577}.  LayerNorm: D in {64, 384, 768, 1024}, five rows (more than one workgroup of four), values around 1000.
The encoder: vit_restate.seeded_state -- LayerNorm weights in [0.5, 1.5], LayerScale gammas in [0.2, 1] of both signs, and the q and k
rows of every qkv scaled so that the logits q . k / 8 have a standard deviation of about 4: the softmax is not flat (test_vit_cpu.py
measures a mean largest weight above 0.3).  Acceptance of the whole encoder: the RMS error of the device route against float64 must not
exceed that of the torch route run as the reference runs it (module.half(), fp16 activations) against the same float64 result; no
margin."""
import copy
import functools

import numpy as np
import pytest
import torch

import placement as pl
import vit_restate as vr
from densematcher_amd.featup.model_utils.extractor_dino import ViTExtractor
from densematcher_amd.featurizers import AggregationNetwork, aggregate_features, dino_features, dinov2

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIN_M, LIN_N, LIN_K = (1, 127, 128, 129, 577), (8, 129, 2304), (64, 640, 3072)
ATT_T = (2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 577)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def rng(*key):
    return np.random.default_rng([77] + [int(k) for k in key])


def h16(a):
    """the nearest fp16 values, as float64"""
    return np.asarray(a, np.float16).astype(np.float64)


def dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(DEV).to(dtype)                  # a copy: the shared operands are read-only


def within(got, want, bound, what):
    got = got.detach().double().cpu().numpy()
    err = np.abs(got - want)
    assert np.isfinite(got).all(), what
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"{what}: max |err| {err.max():.3e}, largest err / bound {worst:.3f}")
    assert (err <= bound).all(), f"{what}: err / bound up to {worst:.3f}"


def nan_buffer(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. linear
@functools.lru_cache(maxsize=None)
def lin_operands(K):
    """A (577, K), W (2304, K) fp16-representable, the epilogue operands, A W^T and |A| |W|^T in float64: read-only, shared"""
    g = rng(1, K)
    A, W = h16(g.normal(0, 1, (577, K))), h16(g.normal(0, K ** -0.5, (2304, K)))
    d = dict(A=A, W=W, bias=g.normal(0, 0.5, 2304).astype(np.float32), scale=(g.uniform(0.2, 1.0, 2304) * g.choice([-1, 1], 2304)).astype(np.float32),
             resid=g.normal(0, 2, (577, 2304)).astype(np.float32), z=A @ W.T, mag=np.abs(A) @ np.abs(W).T)
    for v in d.values():
        v.setflags(write=False)
    return d


def lin_case(M, N, K, bias, scale, resid, act, half):
    d = lin_operands(K)
    kw = dict(bias=d["bias"][:N] if bias else None, scale=d["scale"][:N] if scale else None, resid=d["resid"][:M, :N] if resid else None, act=act)
    want = vr.linear(d["A"][:M], d["W"][:N], z=d["z"][:M, :N], **kw)
    bound = vr.linear_bound(d["A"][:M], d["W"][:N], half=half, z=d["z"][:M, :N], mag=d["mag"][:M, :N], **kw)
    t = lambda name, dt: None if kw.get(name) is None else dev(kw[name], dt)
    args = dict(bias=t("bias", torch.float32), scale=t("scale", torch.float32), resid=t("resid", torch.float32), gelu=act,
                out_dtype=torch.float16 if half else torch.float32)
    return dev(d["A"][:M], torch.float16), dev(d["W"][:N], torch.float16), args, want, bound


@pytest.mark.parametrize("K", LIN_K)
@pytest.mark.parametrize("N", LIN_N)
@pytest.mark.parametrize("M", LIN_M)
def test_linear_shapes_within_the_bound(eng, M, N, K):
    for full in (True, False):                                           # every epilogue term into fp32; the bare product into fp16
        A, W, args, want, bound = lin_case(M, N, K, full, full, full, full, not full)
        got = eng.vit_linear(A, W, **args)
        assert got.shape == (M, N) and got.dtype == args["out_dtype"]
        within(got, want, bound, f"linear M={M} N={N} K={K} {'full epilogue, fp32' if full else 'bare, fp16'}")


def test_linear_every_epilogue_combination(eng):
    M, N, K = 129, 129, 640
    for code in range(32):
        bias, scale, resid, act, half = (bool(code >> i & 1) for i in range(5))
        A, W, args, want, bound = lin_case(M, N, K, bias, scale, resid, act, half)
        within(eng.vit_linear(A, W, **args), want, bound, f"linear epilogue bias={bias} scale={scale} resid={resid} gelu={act} fp16={half}")


def test_linear_out_aliasing_resid_and_the_batched_broadcast_form(eng):
    A, W, args, want, bound = lin_case(129, 129, 640, True, True, True, True, False)
    apart = eng.vit_linear(A, W, **args)
    x = args["resid"].clone()
    assert eng.vit_linear(A, W, **{**args, "resid": x, "out": x}) is x    # out is resid itself: read and written by the same lane
    assert torch.equal(pl.bits(x), pl.bits(apart)) and not torch.equal(x, args["resid"])
    # B = 3 blocks of Mb = 43 rows of A, one residual block for all, output blocks further apart than Mb N (rows 1 .. of a token block)
    Bn, Mb, N = 3, 43, 129
    Ab = A.view(Bn, Mb, 640)
    r = args["resid"][:Mb].contiguous()
    buf = nan_buffer((Bn, Mb + 1, N), torch.float32)
    with pl.PointerRecorder(eng.lib, "dm_vit_linear_f16") as rec:
        eng.vit_linear(Ab, W, bias=args["bias"], scale=args["scale"], resid=r, gelu=True, out=buf[:, 1:])
    assert rec.saw(buf[:, 1:], r, Ab) and len(rec.calls) == 1
    assert bool(torch.isnan(buf[:, 0]).all())                             # the row in front of every block is untouched
    d = lin_operands(640)
    for b in range(Bn):
        kw = dict(bias=d["bias"][:N], scale=d["scale"][:N], resid=d["resid"][:Mb, :N], act=True)
        rows = slice(b * Mb, (b + 1) * Mb)
        within(buf[b, 1:], vr.linear(d["A"][rows], d["W"][:N], **kw), vr.linear_bound(d["A"][rows], d["W"][:N], **kw), f"batched linear, block {b}")
        alone = eng.vit_linear(Ab[b], W, bias=args["bias"], scale=args["scale"], resid=r, gelu=True)
        assert torch.equal(pl.bits(alone), pl.bits(buf[b, 1:]))


def test_linear_identity_times_an_asymmetric_matrix_is_exact(eng):
    M, N, K = 70, 67, 128                                                 # out[m, n] = W[n, m]: a transposed store would show
    g = rng(2)
    W = g.integers(-9, 10, (N, K)).astype(np.float64)
    A = np.eye(M, K)
    got = eng.vit_linear(dev(A, torch.float16), dev(W, torch.float16))
    assert torch.equal(got.cpu(), torch.from_numpy(W.T[:M].astype(np.float32)))
    assert not np.array_equal(W[:N, :N], W[:N, :N].T)


def test_linear_refuses_bad_arguments(eng):
    A, W = torch.zeros(4, 60, dtype=torch.float16, device=DEV), torch.zeros(8, 60, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="multiple of 64"):
        eng.vit_linear(A, W)
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    A, W, out = torch.zeros(4, 64, dtype=torch.float16, device=DEV), torch.zeros(8, 64, dtype=torch.float16, device=DEV), torch.zeros(4, 8, device=DEV)
    call = lambda **kw: eng.lib.dm_vit_linear_f16(eng.ctx, *[kw.get(k, v) for k, v in dict(
        B=1, Mb=4, N=8, K=64, A=p(A), lda=64, sA=0, W=p(W), ldw=64, bias=None, scale=None, resid=None, ldr=0, sR=0, act=0, dt=1, out=p(out), ldo=8, sO=0).items()])
    assert call() == 0
    for bad in (dict(Mb=0), dict(K=96), dict(lda=56), dict(ldo=7), dict(A=None), dict(out=None), dict(act=2), dict(dt=5), dict(A=C.c_void_p(A.data_ptr() + 2)),
                dict(B=2, sO=16)):
        assert call(**bad) == -1, bad
    q = torch.zeros(1, 2, 96, dtype=torch.float16, device=DEV)
    o = torch.zeros(1, 2, 32, dtype=torch.float16, device=DEV)
    assert eng.lib.dm_vit_attention_f16(eng.ctx, 1, 2, 1, 32, p(q), 96, 0, p(o), 32, 0) == -1        # head dimension 32
    assert eng.lib.dm_vit_attention_f16(eng.ctx, 1, 0, 1, 64, p(q), 192, 0, p(o), 64, 0) == -1
    assert eng.lib.dm_vit_layernorm_f16(eng.ctx, 4, 8, p(out), 7, p(out), p(out), 0, p(o), 8) == -1     # ldx below D
    eng.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2. LayerNorm
@pytest.mark.parametrize("D", (64, 384, 768, 1024))
def test_layernorm_with_a_large_common_offset(eng, D):
    g = rng(3, D)
    x = (1000.0 + g.normal(0, 1, (5, D))).astype(np.float32)            # mean >> spread: a one-pass variance would lose every digit
    gamma, beta = g.uniform(0.5, 1.5, D).astype(np.float32), g.normal(0, 0.5, D).astype(np.float32)
    want = vr.layernorm(x, gamma, beta)
    xd = dev(x, torch.float32)
    got = eng.vit_layernorm(xd, dev(gamma, torch.float32), dev(beta, torch.float32))
    assert got.dtype == torch.float16 and got.shape == (5, D)
    within(got, want, vr.layernorm_bound(x, gamma, beta), f"layernorm D={D} fp16")
    got32 = eng.vit_layernorm(xd, dev(gamma, torch.float32), dev(beta, torch.float32), out_dtype=torch.float32)
    within(got32, want, vr.layernorm_bound(x, gamma, beta, half=False), f"layernorm D={D} fp32")
    assert torch.equal(pl.bits(got32.half()), pl.bits(got))               # the same value, rounded once more


# ---------------------------------------------------------------------------------------------------------------- 3. attention
@functools.lru_cache(maxsize=None)
def att_operands(heads, T):
    """qkv (2, T, 192 heads) fp16-representable.  Per (image, head): rows i % 3 == 0 are plain N(0, 1) queries; the others aim at one
    key j* -- q = 960 k_j* / |k_j*|^2, so that q . k_j* / 8 = 120 and a softmax without the maximum subtracted overflows --, j* in the
    first half tile of keys for i % 3 == 1 and in the last, partial tile for i % 3 == 2."""
    g = rng(4, heads, T)
    D = 64 * heads
    qkv = g.normal(0, 1, (2, T, 3, heads, 64))
    for i in range(T):
        if i % 3:
            j = (i * 7) % min(32, T) if i % 3 == 1 else T - 1 - (i % min(16, T))
            kj = h16(qkv[:, j, 1])
            qkv[:, i, 0] = 960.0 * kj / (kj ** 2).sum(-1, keepdims=True)
    qkv = h16(qkv.reshape(2, T, 3 * D))
    qkv.setflags(write=False)
    return qkv


@pytest.mark.parametrize("T", ATT_T)
@pytest.mark.parametrize("heads", (1, 12))
def test_attention_within_the_bound(eng, heads, T):
    qkv = att_operands(heads, T)
    q, k, _ = vr.split_heads(qkv, heads)
    peak = np.abs((q / 8) @ k.transpose(0, 1, 3, 2)).max()
    assert peak > 100 or T < 2
    got = eng.vit_attention(dev(qkv, torch.float16), heads)
    assert got.shape == (2, T, 64 * heads) and got.dtype == torch.float16
    within(got, vr.attention(qkv, heads), vr.attention_bound(qkv, heads), f"attention heads={heads} T={T} (largest |logit| {peak:.0f})")


def test_attention_one_hot_values_and_integer_scores_are_exact(eng):
    T, heads = 256, 2
    qkv = np.zeros((1, T, 3, heads, 64))
    for i in range(T):
        qkv[0, i, 0, :, (i * 5) % 64] = 64.0                             # q . k / 8 is 512 for the four keys of the query's class, else 0:
        qkv[0, i, 1, :, i % 64] = 64.0                                   # expf(-512) is exactly 0, the four weights exactly 1
        qkv[0, i, 2, 0, (i // 64) * 3] = 1.0
        qkv[0, i, 2, 1, 63 - (i // 64) % 2] = 1.0
    qkv = qkv.reshape(1, T, 3 * 64 * heads)
    want = vr.attention(qkv, heads)
    assert set(np.unique(want)) == {0.0, 0.25, 0.5}
    got = eng.vit_attention(dev(qkv, torch.float16), heads)
    assert torch.equal(got.cpu().double(), torch.from_numpy(want))


# ---------------------------------------------------------------------------------------------------------------- 4. patch rows
@pytest.mark.parametrize("P", (1, 3))
def test_patch_rows_at_the_native_size_are_a_gather(eng, P):
    S = 14 * P
    x = torch.from_numpy(rng(5, P).uniform(0, 1, (2, 3, S, S)).astype(np.float32))
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)

    def gather(img):                                                      # on the CPU: IEEE subtraction and division in fp32
        y = (img.float() - m) / s
        return y.reshape(2, 3, P, 14, P, 14).permute(0, 2, 4, 1, 3, 5).reshape(2 * P * P, 588).half()

    for name, src in (("nchw fp32", x.to(DEV)), ("channels-last fp32", x.to(DEV).contiguous(memory_format=torch.channels_last)),
                      ("nchw fp16", x.half().to(DEV)), ("channels-last fp16", x.half().to(DEV).contiguous(memory_format=torch.channels_last))):
        got = eng.vit_patch_rows(src, P, MEAN, STD)
        assert got.shape == (2 * P * P, 640) and got.dtype == torch.float16, name
        assert torch.equal(pl.bits(got[:, :588].cpu()), pl.bits(gather(src.cpu()))), name
        assert not bool(got[:, 588:].any()), name


def test_patch_rows_resized_within_the_bound(eng):
    P, S = 3, 48
    x = h16(rng(6).uniform(0, 1, (2, 3, S, S)))
    want, bound = vr.patch_rows(x, P, MEAN, STD), vr.patch_rows_bound(x, P, MEAN, STD)
    for name, src in (("fp32", dev(x, torch.float32)), ("fp16 channels-last", dev(x, torch.float16).contiguous(memory_format=torch.channels_last))):
        within(eng.vit_patch_rows(src, P, MEAN, STD), want, bound, f"patch rows 48 -> 42, {name}")


# ---------------------------------------------------------------------------------------------------------------- 5. placement
def test_operands_are_read_and_written_where_they_lie(eng):
    A, W, args, _, _ = lin_case(129, 129, 640, True, True, True, True, False)
    want = eng.vit_linear(A, W, **args)
    Ab, Wb = nan_buffer((131, 648), torch.float16), nan_buffer((131, 656), torch.float16)
    Ab[1:130, 8:648], Wb[1:130, 16:656] = A, W                            # interior views on the 16-byte grid, leading dimensions above K
    rb, ob = nan_buffer((131, 133), torch.float32), nan_buffer((131, 135), torch.float32)
    rb[1:130, 3:132] = args["resid"]
    Av, Wv, rv, ov = Ab[1:130, 8:648], Wb[1:130, 16:656], rb[1:130, 3:132], ob[1:130, 5:134]
    with pl.PointerRecorder(eng.lib, "dm_vit_linear_f16") as rec:
        eng.vit_linear(Av, Wv, **{**args, "resid": rv, "out": ov})
    assert rec.saw(Av, Wv, rv, ov), "an operand was copied instead of being used where it lies"
    assert torch.equal(pl.bits(ov), pl.bits(want))
    mask = torch.ones_like(ob, dtype=torch.bool)
    mask[1:130, 5:134] = False
    assert bool(torch.isnan(ob[mask]).all())                              # the bytes around the output view are untouched
    off = nan_buffer((129 * 640 + 8,), torch.float16)[3:3 + 129 * 640].view(129, 640)                      # off the 16-byte grid: copied, same bits
    off.copy_(A)
    assert off.data_ptr() % 16 and torch.equal(pl.bits(eng.vit_linear(off, W, **args)), pl.bits(want))
    # attention: qkv and the output inside NaN-filled buffers, rows and images further apart than their widths
    qkv = dev(att_operands(1, 65), torch.float16)
    want = eng.vit_attention(qkv, 1)
    qb, outb = nan_buffer((2, 67, 208), torch.float16), nan_buffer((2, 67, 80), torch.float16)
    qb[:, 1:66, 8:200] = qkv
    qv, outv = qb[:, 1:66, 8:200], outb[:, 1:66, 8:72]
    with pl.PointerRecorder(eng.lib, "dm_vit_attention_f16") as rec:
        eng.vit_attention(qv, 1, out=outv)
    assert rec.saw(qv, outv) and torch.equal(pl.bits(outv), pl.bits(want))
    mask = torch.ones_like(outb, dtype=torch.bool)
    mask[:, 1:66, 8:72] = False
    assert bool(torch.isnan(outb[mask]).all())
    # LayerNorm
    g = rng(7)
    x, gamma, beta = dev(g.normal(3, 2, (5, 384)), torch.float32), dev(g.uniform(0.5, 1.5, 384), torch.float32), dev(g.normal(0, 1, 384), torch.float32)
    want = eng.vit_layernorm(x, gamma, beta)
    xb, yb = nan_buffer((7, 389), torch.float32), nan_buffer((7, 391), torch.float16)
    xb[1:6, 3:387] = x
    with pl.PointerRecorder(eng.lib, "dm_vit_layernorm_f16") as rec:
        eng.vit_layernorm(xb[1:6, 3:387], gamma, beta, out=yb[1:6, 5:389])
    assert rec.saw(xb[1:6, 3:387], yb[1:6, 5:389]) and torch.equal(pl.bits(yb[1:6, 5:389]), pl.bits(want))
    mask = torch.ones_like(yb, dtype=torch.bool)
    mask[1:6, 5:389] = False
    assert bool(torch.isnan(yb[mask]).all())
    # patch rows: the images as a window of a larger NaN-filled batch, the rows with a leading dimension above 640
    img = dev(rng(8).uniform(0, 1, (2, 3, 28, 28)), torch.float32)
    want = eng.vit_patch_rows(img, 2, MEAN, STD)
    ib, pb = nan_buffer((3, 4, 30, 31), torch.float32), nan_buffer((10, 648), torch.float16)
    ib[1:3, 1:4, 1:29, 2:30] = img
    with pl.PointerRecorder(eng.lib, "dm_vit_patch_rows_f16") as rec:
        eng.vit_patch_rows(ib[1:3, 1:4, 1:29, 2:30], 2, MEAN, STD, out=pb[1:9, 8:648])
    assert rec.saw(ib[1:3, 1:4, 1:29, 2:30], pb[1:9, 8:648]) and torch.equal(pl.bits(pb[1:9, 8:648]), pl.bits(want))
    mask = torch.ones_like(pb, dtype=torch.bool)
    mask[1:9, 8:648] = False
    assert bool(torch.isnan(pb[mask]).all())


# ---------------------------------------------------------------------------------------------------------------- 6. the encoder
@functools.lru_cache(maxsize=None)
def encoder(dim, depth, heads, seed):
    state = vr.seeded_state(dim, depth, seed)
    m = dinov2.DinoVisionTransformer(dim, depth, heads)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return state, m.to(DEV).eval().requires_grad_(False)


def rms(a, ref):
    return float(np.sqrt(np.mean((a.detach().double().cpu().numpy() - ref) ** 2)))


def half_route(model, x, **kw):
    """the torch route as the reference runs it: module.half() on the GPU, fp16 activations"""
    with torch.no_grad():
        return copy.deepcopy(model).half().tokens(x.half(), route="torch", **kw)


@pytest.mark.parametrize("dim,heads,P,n", [(128, 2, 3, 3), (128, 2, 8, 3), (768, 12, 24, 2)])
def test_encoder_against_float64_is_no_worse_than_the_half_route(eng, dim, heads, P, n):
    state, model = encoder(dim, 2, heads, 21)
    x = h16(rng(9, dim, P).normal(0, 1, (n, 3, 14 * P, 14 * P)))
    xd = dev(x, torch.float32)
    with torch.no_grad():
        pos = model.pos_table(P)[0].double().cpu().numpy()
        ref = vr.forward(state, x, pos, heads)
        got = model.tokens(xd, route="device")
        got_norm = model.tokens(xd, layer=0, norm=True, route="device")
    assert got.shape == (n, 1 + P * P, dim) and got.dtype == torch.float32
    e_dev, e_half = rms(got, ref), rms(half_route(model, xd), ref)
    print(f"encoder D={dim} P={P} n={n}: rms error device {e_dev:.3e}, half route {e_half:.3e}, ratio {e_dev / e_half:.3f} (rms of the tokens {np.sqrt((ref ** 2).mean()):.3f})")
    assert e_dev <= e_half
    ref0 = vr.forward(state, x, pos, heads, layer=0, norm=True)
    assert rms(got_norm, ref0) <= rms(half_route(model, xd, layer=0, norm=True), ref0)


def test_an_image_has_the_same_bits_alone_and_in_a_batch(eng):
    _, model = encoder(128, 2, 2, 21)
    x = dev(h16(rng(10).normal(0, 1, (3, 3, 112, 112))), torch.float32)
    with torch.no_grad():
        together = model.tokens(x, route="device")
        alone = model.tokens(x[1:2], route="device")
    assert torch.equal(pl.bits(together[1:2]), pl.bits(alone)) and not torch.equal(together[0], together[1])


def test_obstacles_with_a_gpu(eng):
    _, model = encoder(128, 2, 2, 21)
    with torch.no_grad():
        with pytest.raises(ValueError, match="not on the GPU"):
            model.tokens(torch.zeros(1, 3, 14, 14), route="device")
        assert model.tokens(torch.zeros(1, 3, 14, 14, device=DEV)).shape == (1, 2, 128)      # auto runs on either route


# ---------------------------------------------------------------------------------------------------------------- 7. extractor path
def test_extractor_and_dino_features_feed_the_aggregation_network(eng):
    _, model = encoder(128, 12, 2, 22)
    ex = ViTExtractor("dinov2_vitb14", stride=14, model=model)
    P, bs = 4, 2
    img = dev(h16(rng(11).uniform(0, 1, (bs, 3, 64, 64))), torch.float32)
    with torch.no_grad():
        batch = ex.resize_and_normalize(img, 14 * P)
        ref = ex.extract_descriptors(batch, layer=11, facet="token", route="torch").double().cpu().numpy()        # fp32 torch route
        got = ex.extract_descriptors(batch, layer=11, facet="token", route="device")
        half = half_route(model, batch, layer=11)[:, None, 1:]
        assert got.shape == (bs, 1, P * P, 128)
        e_dev, e_half = rms(got, ref), rms(half, ref)
        print(f"extract_descriptors: rms error against the fp32 torch route: device {e_dev:.3e}, half route {e_half:.3e}")
        assert e_dev <= e_half
        want = dino_features(ex, img, P, route="torch")
        dino = dino_features(ex, img, P, route="device")
        assert dino.shape == (bs, 128, P, P) and dino.stride(1) == 1 and not dino.is_contiguous()
        ref = want.double().cpu().numpy()
        half_img = copy.deepcopy(model).half().tokens_from_images(img.half(), P, MEAN, STD, layer=11, route="torch")[:, 1:].permute(0, 2, 1).unflatten(2, (P, P))
        e_dev, e_half = rms(dino, ref), rms(half_img, ref)
        print(f"dino_features: rms error against the fp32 torch route: device {e_dev:.3e}, half route {e_half:.3e}")
        assert e_dev <= e_half
        torch.manual_seed(3)
        net = AggregationNetwork(feature_dims=[6, 8, 8, 128], projection_dim=16, num_norm_groups=2).to(DEV).eval()
        s3, s4, s5 = (torch.randn(bs, c, h, h, device=DEV) for c, h in ((6, P), (8, 2), (8, 1)))
        with pl.PointerRecorder(eng.lib, "dm_agg_gather_f32") as rec:
            out = aggregate_features(net, s3, s4, s5, dino, route="device")
        assert rec.saw(dino), "the token view was copied on its way into the aggregation network"
        assert out.shape == (bs, 16, P, P) and bool(torch.isfinite(out).all())
        assert torch.equal(pl.bits(out), pl.bits(aggregate_features(net, s3, s4, s5, dino.contiguous(), route="device")))

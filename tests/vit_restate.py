"""
The DINOv2 encoder and the formulas of its four kernels (dm_vit_patch_rows_f16, dm_vit_layernorm_f16, dm_vit_linear_f16,
dm_vit_attention_f16) restated in float64 NumPy, each with a running-error bound for the kernel.

Error model.  u32 = 2^-24 is the unit roundoff of the fp32 accumulations, u16 = 2^-11 that of every stated rounding to fp16.  A product of
two fp16 numbers has 22 significant bits and is exact in fp32; a sum of n of them accumulated in fp32, in any fixed order and with at most
one rounding per addition, satisfies |s_hat - s| <= gamma_n sum |a_j b_j|, gamma_n = n u32 / (1 - n u32) (Higham, Accuracy and Stability
of Numerical Algorithms, section 3.1).  SLACK = 1 + 2^-9 carries the 1 / (1 - n u32) factors (n <= 2^14 here) and the products of two
error terms.  Library functions: erff and expf are taken as within E_FUN = 4 u32 (two units in the last place of fp32), relative for expf
and absolute for erff (|erf| <= 1).  The bounds are derived here from the kernels' stated order of operations; none is fitted to their
output.

  patch rows  v = the bilinear sample: coordinates in fp64 (exact to 2^-40 of a pixel), two weights rounded to fp32 (u32 each), seven
              fp32 products and sums on values within [-a, a], a = max |pixel|: |v_hat - v| <= 12 u32 a.  y = (v - mean_c) / std_c: the
              subtraction and the division round once each, mean_c and std_c are fp32 roundings of the given doubles (relative u32
              each; the restatement uses the rounded values, as the kernel does): |y_hat - y| <= (12 u32 a + 2 u32 (|v| + |mean_c|))
              / std_c + u32 |y|, then one rounding to fp16: + u16 |y|.  At S = 14 P the sample is the pixel itself and the result is
              fl16(fl32(fl32(v - mean) / std)) exactly.
  layernorm   statistics in fp64 on exact fp32 inputs: the mean of D terms through a chain of ceil(D / 64) additions and a tree of 6,
              |mean_hat - mean| <= c u64 mean|x|, c = ceil(D / 64) + 7, u64 = 2^-53; the variance likewise on squared deviations,
              relative error <= (c + 4) u64 + 2 |mean_hat - mean|^2 / var, so rstd has relative error <= c + 8 u64 (half of it, plus the
              square root and the division).  n = fl32((x - mean) rstd): |n_hat - n| <= u32 |n| + c u64 mean|x| rstd + (c + 10) u64 |n|.
              y = fmaf(n, gamma, beta), one rounding, then fl16: |y_hat - y| <= |gamma| |n_hat - n| + u32 |y| + u16 |y|.
  linear      z = A W^T over K: e_z = gamma_K |A| |W|^T.  + bias: e1 = e_z + u32 |z + b|.  GELU g(v) = 0.5 v (1 + erf(v / sqrt 2)) is
              1.13-Lipschitz; computed as fl(fl(0.5 v) fl(1 + erff(fl(v c)))): 0.5 v exact, v c one rounding, which moves erf by at
              most 0.5 u32 (max x erf'(x) = 0.48), erff E_FUN, the sum u32 on a value <= 2, the product u32 |g|:
              e2 = 1.13 e1 + |0.5 v| (E_FUN + 3 u32) + u32 |g|.  * scale: e3 = |s| e2 + u32 |s g|.  + resid: e4 = e3 + u32 |r + s g|.
              fp16 output: + u16 |out|.
  attention   s_j = (q / 8) . k_j over 64: e_s = gamma_64 (|q| / 8) . |k_j| (q / 8 is exact unless it falls below the fp16 normal range;
              the tests keep |q| >= 2^-10 or zero).  With M the row maximum, p_j = exp(s_j - M), l = sum p_j >= 1, the kernel's
              weight of key j -- expf of a rounded difference against the running maximum, then one multiplication by
              alpha = expf(difference of maxima) per later tile, nt = ceil(T / 32) tiles -- is p_j (1 + r_j) + a_j with
                  |r_j| <= e_s exp(e_s) + R,  R = (nt + 1) (E_FUN + 3 u32)            (score error; expf; the products)
                  |a_j| <= A = (nt + 1) 0.37 u32                                        (rounding x = M - s moves e^-x by <= u32 x e^-x)
              The sum l adds 17 positive terms per tile and lane and one more at the end: relative (17 nt + 2) u32 on top.  The
              numerator rounds each weight to fp16 (relative u16, or 2^-25 absolute below the normal range) and accumulates T products
              and nt rescalings in fp32: (T + nt + 2) u32 sum p_j |v_jd|.  The quotient rounds once in fp32 and once to fp16.
                  e_num = sum_j |v_jd| (p_j (|r_j| + u16) + A + 2^-25) + (T + nt + 2) u32 sum_j p_j |v_jd|
                  rho_l = (sum_j (p_j |r_j| + A)) / l + (17 nt + 2) u32
                  |out_hat - out| <= SLACK (e_num / l + |out| rho_l) + (u32 + u16) |out|
"""
import math

import numpy as np

U32, U16, U64 = 2.0 ** -24, 2.0 ** -11, 2.0 ** -53
SLACK = 1.0 + 2.0 ** -9
E_FUN = 4 * U32
PATCH, PATCH_K = 14, 588

f64 = lambda a: np.asarray(a, dtype=np.float64)

try:
    from scipy.special import erf as _erf
except ImportError:                                       # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(v):
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def gamma_n(n):
    return n * U32 / (1.0 - n * U32)


# --------------------------------------------------------------------------------------------------------------------- patch rows
def resize_bilinear(img, Z):
    """F.interpolate(bilinear, align_corners=False) of (n, C, S, S) to (Z, Z) in float64"""
    img = f64(img)
    S = img.shape[-1]
    if S == Z:
        return img
    f = np.maximum((np.arange(Z) + 0.5) * (S / Z) - 0.5, 0.0)
    i0 = np.minimum(f.astype(np.int64), S - 1)
    i1 = i0 + (i0 < S - 1)
    w = f - i0
    rows = img[:, :, i0, :] * (1 - w)[None, None, :, None] + img[:, :, i1, :] * w[None, None, :, None]
    return rows[:, :, :, i0] * (1 - w) + rows[:, :, :, i1] * w


def normalise(img, mean, std):
    m, s = (f64(np.asarray(v, np.float32)).reshape(1, 3, 1, 1) for v in (mean, std))
    return (f64(img) - m) / s


def patchify(x, Kp=640):
    """(n, 3, 14 P, 14 P) -> (n P P, Kp): row i P P + py P + px, column 196 c + 14 dy + dx, zero padding behind column 587"""
    n, C, Z, _ = x.shape
    P = Z // PATCH
    rows = x.reshape(n, C, P, PATCH, P, PATCH).transpose(0, 2, 4, 1, 3, 5).reshape(n * P * P, PATCH_K)
    out = np.zeros((n * P * P, Kp), x.dtype)
    out[:, :PATCH_K] = rows
    return out


def patch_rows(img, P, mean, std, Kp=640):
    return patchify(normalise(resize_bilinear(img, PATCH * P), mean, std), Kp)


def patch_rows_bound(img, P, mean, std, Kp=640):
    a = np.abs(f64(img)).max()
    v = resize_bilinear(img, PATCH * P)
    m, s = (f64(np.asarray(t, np.float32)).reshape(1, 3, 1, 1) for t in (mean, std))
    y = (v - m) / s
    e = (12 * U32 * a + 2 * U32 * (np.abs(v) + np.abs(m))) / s + (U32 + U16) * np.abs(y)
    return patchify(SLACK * e, Kp)


# --------------------------------------------------------------------------------------------------------------------- LayerNorm
def layernorm(x, gamma, beta, eps=1e-6):
    x = f64(x)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * f64(gamma) + f64(beta)


def layernorm_bound(x, gamma, beta, eps=1e-6, half=True):
    x, g = f64(x), np.abs(f64(gamma))
    D = x.shape[-1]
    c = -(-D // 64) + 7
    mean = x.mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=-1, keepdims=True) + eps)
    n = np.abs(x - mean) * rstd
    e_n = U32 * n + c * U64 * np.abs(x).mean(axis=-1, keepdims=True) * rstd + (c + 10) * U64 * n
    y = np.abs(layernorm(x, gamma, beta, eps))
    return SLACK * (g * e_n + (U32 + (U16 if half else 0.0)) * y)


# --------------------------------------------------------------------------------------------------------------------- linear
def linear(A, W, bias=None, scale=None, resid=None, act=False, z=None):
    """z: A W^T where the caller has it already (a block of a larger product)"""
    v = f64(A) @ f64(W).T if z is None else f64(z)
    if bias is not None:
        v = v + f64(bias)
    if act:
        v = gelu(v)
    if scale is not None:
        v = v * f64(scale)
    return v if resid is None else f64(resid) + v


def linear_bound(A, W, bias=None, scale=None, resid=None, act=False, half=False, z=None, mag=None):
    """z, mag: A W^T and |A| |W|^T where the caller has them already"""
    A, W = f64(A), f64(W)
    z = A @ W.T if z is None else f64(z)
    e = gamma_n(A.shape[-1]) * (np.abs(A) @ np.abs(W).T if mag is None else f64(mag))
    v = z
    if bias is not None:
        v = z + f64(bias)
        e = e + U32 * (np.abs(v) + e)
    if act:
        g = gelu(v)
        e = 1.13 * e + (0.5 * np.abs(v) + e) * (E_FUN + 3 * U32) + U32 * np.abs(g)
        v = g
    if scale is not None:
        s = np.abs(f64(scale))
        e = s * e + U32 * s * np.abs(v)
        v = v * f64(scale)
    if resid is not None:
        v = f64(resid) + v
        e = e + U32 * (np.abs(v) + e)
    return SLACK * (e + (U16 * np.abs(v) if half else 0.0))


# --------------------------------------------------------------------------------------------------------------------- attention
def split_heads(qkv, heads):
    """(n, T, 3 D) -> q, k, v each (n, heads, T, 64): q | k | v, the heads adjacent within each"""
    n, T, W3 = qkv.shape
    d = W3 // (3 * heads)
    q, k, v = f64(qkv).reshape(n, T, 3, heads, d).transpose(2, 0, 3, 1, 4)
    return q, k, v


def attention(qkv, heads):
    """(n, T, 3 D) -> (n, T, D): softmax(q k^T / sqrt(d)) v per image and head"""
    q, k, v = split_heads(qkv, heads)
    n, H, T, d = q.shape
    s = (q * d ** -0.5) @ k.transpose(0, 1, 3, 2)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    o = (p @ v) / p.sum(axis=-1, keepdims=True)
    return o.transpose(0, 2, 1, 3).reshape(n, T, H * d)


def attention_bound(qkv, heads):
    q, k, v = split_heads(qkv, heads)
    n, H, T, d = q.shape
    nt = -(-T // 32)
    q = q * d ** -0.5
    s = q @ k.transpose(0, 1, 3, 2)
    e_s = gamma_n(d) * (np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2))
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    l = p.sum(axis=-1, keepdims=True)
    R = (nt + 1) * (E_FUN + 3 * U32)
    A = (nt + 1) * 0.37 * U32
    r = e_s * np.exp(e_s) + R
    av = np.abs(v)
    e_num = (p * (r + U16) + A + 2.0 ** -25) @ av + (T + nt + 2) * U32 * (p @ av)
    rho = (p * r + A).sum(axis=-1, keepdims=True) / l + (17 * nt + 2) * U32
    out = np.abs((p @ v) / l)
    e = SLACK * (e_num / l + out * rho) + (U32 + U16) * out
    return e.transpose(0, 2, 1, 3).reshape(n, T, H * d)


# --------------------------------------------------------------------------------------------------------------------- the encoder
def forward(params, x, pos, heads, layer=None, norm=False):
    """The encoder in float64.  params: name -> array, the hub model's state dict; x (n, 3, 14 P, 14 P) normalised images; pos
    (1 + P P, D): the positional table of the P x P grid (the module's pos_table: both routes read the same tensor).  Returns the
    output of block `layer` (None: the last) as (n, 1 + P P, D), with the final LayerNorm on request."""
    g = lambda name: f64(params[name])
    x = f64(x)
    n, D = x.shape[0], g("cls_token").shape[-1]
    rows = patchify(x, PATCH_K) @ g("patch_embed.proj.weight").reshape(D, PATCH_K).T + g("patch_embed.proj.bias")
    tok = np.concatenate([np.broadcast_to(g("cls_token").reshape(1, 1, D), (n, 1, D)), rows.reshape(n, -1, D)], axis=1) + f64(pos)[None]
    depth = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("blocks."))
    layer = depth - 1 if layer is None else layer
    for i in range(layer + 1):
        b = f"blocks.{i}."
        h = layernorm(tok, g(b + "norm1.weight"), g(b + "norm1.bias"))
        a = attention(linear(h, g(b + "attn.qkv.weight"), g(b + "attn.qkv.bias")), heads)
        tok = tok + g(b + "ls1.gamma") * linear(a, g(b + "attn.proj.weight"), g(b + "attn.proj.bias"))
        h = layernorm(tok, g(b + "norm2.weight"), g(b + "norm2.bias"))
        m = linear(h, g(b + "mlp.fc1.weight"), g(b + "mlp.fc1.bias"), act=True)
        tok = tok + g(b + "ls2.gamma") * linear(m, g(b + "mlp.fc2.weight"), g(b + "mlp.fc2.bias"))
    return layernorm(tok, g("norm.weight"), g("norm.bias")) if norm else tok


def state_dict_keys(dim, depth):
    """the hub model's key list with its shapes"""
    keys = {"cls_token": (1, 1, dim), "pos_embed": (1, 1 + 37 * 37, dim), "mask_token": (1, dim),
            "patch_embed.proj.weight": (dim, 3, 14, 14), "patch_embed.proj.bias": (dim,), "norm.weight": (dim,), "norm.bias": (dim,)}
    for i in range(depth):
        b = f"blocks.{i}."
        keys.update({b + "norm1.weight": (dim,), b + "norm1.bias": (dim,), b + "attn.qkv.weight": (3 * dim, dim), b + "attn.qkv.bias": (3 * dim,),
                     b + "attn.proj.weight": (dim, dim), b + "attn.proj.bias": (dim,), b + "ls1.gamma": (dim,),
                     b + "norm2.weight": (dim,), b + "norm2.bias": (dim,), b + "mlp.fc1.weight": (4 * dim, dim), b + "mlp.fc1.bias": (4 * dim,),
                     b + "mlp.fc2.weight": (dim, 4 * dim), b + "mlp.fc2.bias": (dim,), b + "ls2.gamma": (dim,)})
    return keys


def seeded_state(dim, depth, seed, logit_gain=4.0):
    """A state dict with the hub's keys whose softmax is not flat: weights N(0, 1 / fan_in), except that the q and k rows of every qkv
    are scaled by sqrt(logit_gain) each (LayerNorm output has unit variance, so q . k / 8 has a standard deviation of about
    logit_gain sqrt(64) / 8 = logit_gain instead of 1 / 8 ... 1); LayerNorm weights in [0.5, 1.5] and biases N(0, 0.1); LayerScale
    gammas in [0.2, 1.0] with both signs; biases N(0, 0.02); cls token and positional table N(0, 0.5)."""
    rng = np.random.default_rng(seed)
    st = {}
    for k, shape in state_dict_keys(dim, depth).items():
        if k.endswith("gamma"):
            v = rng.uniform(0.2, 1.0, shape) * rng.choice([-1.0, 1.0], shape)
        elif "norm" in k and k.endswith("weight"):
            v = rng.uniform(0.5, 1.5, shape)
        elif "norm" in k:
            v = rng.normal(0, 0.1, shape)
        elif k in ("cls_token", "pos_embed", "mask_token"):
            v = rng.normal(0, 0.5, shape)
        elif k.endswith("bias"):
            v = rng.normal(0, 0.02, shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            v = rng.normal(0, fan_in ** -0.5, shape)
            if k.endswith("qkv.weight"):
                v[:2 * dim] *= math.sqrt(logit_gain)
        st[k] = v.astype(np.float32)
    return st

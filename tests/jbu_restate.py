"""FeatUp's JBUStack restated in float64 NumPy from its definitions (reference third_party/featup/featup/upsamplers.py:184-276): the
yardstick of the JBU tests.  Nothing here shares code with the package; weights come as a dict of arrays under the state_dict's names.

  keys        W2 gelu(W1 g + b1) + b2 per pixel, gelu(x) = x (1 + erf(x / sqrt 2)) / 2
  logits      temperature * <key at the reflected neighbour (y + i - 3, x + j - 3), key at (y, x)>, temperature = clip(exp(range_temp), 1e-4, 1e4)
  kernel      softmax over the 49 taps, times exp(-(d_i^2 + d_j^2) / (2 sigma^2)) with d = linspace(-1, 1, 7), divided by max(sum, 1e-7),
              plus 0.1 * (V2 gelu(V1 [kernel, g] + c1) + c2)
  source      bicubic (A = -0.75, align_corners=False: source coordinate (u + 0.5) n_in / n_out - 0.5, four taps with clamped indices)
              to the guidance's size, reflect-padded by 3
  output      out[b, c, y, x] = sum_{i, j} kernel[b, y, x, i, j] * padded[b, c, y + i, x + j]
  stack       four stages, each guided by the image average-pooled (adaptive: window [floor(i n / m), ceil((i + 1) n / m))) to twice the
              stage's source; then x + 0.1 (W x + b)
"""
import numpy as np
from scipy.special import erf

R, D = 3, 7


def gelu(x):
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def conv1x1(x, w, b):
    """x (B, Ci, H, W), w (Co, Ci[, 1, 1]), b (Co)"""
    w = np.asarray(w, np.float64).reshape(w.shape[0], -1)
    return np.einsum("oc,bchw->bohw", w, x) + np.asarray(b, np.float64)[None, :, None, None]


def adaptive_avg_pool(x, out_hw):
    def windows(n, m):
        return [(int(np.floor(i * n / m)), int(np.ceil((i + 1) * n / m))) for i in range(m)]
    rows, cols = windows(x.shape[2], out_hw[0]), windows(x.shape[3], out_hw[1])
    tmp = np.stack([x[:, :, a:b].mean(axis=2) for a, b in rows], axis=2)
    return np.stack([tmp[:, :, :, a:b].mean(axis=3) for a, b in cols], axis=3)


def _cubic_weights(t, A=-0.75):
    inner = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    outer = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return np.stack([outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)])


def _bicubic_axis(x, n_out, axis):
    n_in = x.shape[axis]
    coord = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
    base = np.floor(coord).astype(np.int64)
    wts = _cubic_weights(coord - base)                                     # (4, n_out)
    shape = [1] * x.ndim
    shape[axis] = n_out
    out = 0.0
    for q in range(4):
        idx = np.clip(base - 1 + q, 0, n_in - 1)
        out = out + np.take(x, idx, axis=axis) * wts[q].reshape(shape)
    return out


def bicubic(x, out_hw):
    return _bicubic_axis(_bicubic_axis(x, out_hw[1], 3), out_hw[0], 2)


def stage_weights(P, prefix):
    """the arrays of one JBULearnedRange out of a dict under state_dict names (prefix 'up1.' ...), float64"""
    return {k[len(prefix):]: np.asarray(v, np.float64) for k, v in P.items() if k.startswith(prefix)}


def filters(g, Wt):
    """the combined kernel (B, H, W, 49) of guidance g (B, 3, H, W)"""
    g = np.asarray(g, np.float64)
    B, _, H, W = g.shape
    keys = conv1x1(gelu(conv1x1(g, Wt["range_proj.0.weight"], Wt["range_proj.0.bias"])), Wt["range_proj.3.weight"], Wt["range_proj.3.bias"])
    halo = np.pad(keys, ((0, 0), (0, 0), (R, R), (R, R)), mode="reflect")
    temp = np.clip(np.exp(float(Wt["range_temp"])), 1e-4, 1e4)
    logits = np.stack([(halo[:, :, i:i + H, j:j + W] * keys).sum(1) for i in range(D) for j in range(D)], axis=1) * temp
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    soft = e / e.sum(axis=1, keepdims=True)
    d = np.linspace(-1.0, 1.0, D)
    spatial = np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * float(Wt["sigma_spatial"]) ** 2)).reshape(1, D * D, 1, 1)
    k = soft * spatial
    k = k / np.maximum(k.sum(axis=1, keepdims=True), 1e-7)
    fix = conv1x1(gelu(conv1x1(np.concatenate([k, g], axis=1), Wt["fixup_proj.0.weight"], Wt["fixup_proj.0.bias"])),
                  Wt["fixup_proj.3.weight"], Wt["fixup_proj.3.bias"])
    return np.ascontiguousarray((k + 0.1 * fix).transpose(0, 2, 3, 1))


def apply(src, filt):
    """src (B, C, h, w), filt (B, H, W, 49) -> (B, C, H, W): bicubic to (H, W), reflect padding, the adaptive convolution"""
    src, filt = np.asarray(src, np.float64), np.asarray(filt, np.float64)
    B, H, W, _ = filt.shape
    pad = np.pad(bicubic(src, (H, W)), ((0, 0), (0, 0), (R, R), (R, R)), mode="reflect")
    out = np.zeros((B, src.shape[1], H, W))
    for i in range(D):
        for j in range(D):
            out += filt[:, None, :, :, i * D + j] * pad[:, :, i:i + H, j:j + W]
    return out


def stage(src, g, Wt):
    f = filters(g, Wt)
    return apply(src, f), f


def stack(src, image, P):
    """JBUStack on src (B, C, h, w) and image (B, 3, Hg, Wg) with the state_dict P: {'stages': the four stage outputs, 'kernel1': stage
    1's combined kernel (B, 2h, 2w, 7, 7), 'y': the result}"""
    x, image = np.asarray(src, np.float64), np.asarray(image, np.float64)
    res = {"stages": []}
    for s in range(1, 5):
        g = adaptive_avg_pool(image, (2 * x.shape[2], 2 * x.shape[3]))
        x, f = stage(x, g, stage_weights(P, f"up{s}."))
        res["stages"].append(x)
        if s == 1:
            res["kernel1"] = f.reshape(f.shape[:3] + (D, D))
    res["y"] = x + 0.1 * conv1x1(x, np.asarray(P["fixup_proj.1.weight"], np.float64), P["fixup_proj.1.bias"])
    return res

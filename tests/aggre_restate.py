"""
The aggregation network behind the 2D backbones in NumPy float64, from the formulas alone (no torch, nothing of the reference imported):
the yardstick of tests/test_aggre_cpu.py and tests/test_gpu_aggre.py.

  interp       F.interpolate(bilinear, align_corners=False): source coordinate max(0, (t + 1/2) h / P - 1/2), taps floor and floor + 1
               clamped to the last row / column
  rotate       torchvision's rotate(img, angle, BILINEAR) as the package restates it (featurizers/util.py): output pixel (y, x) samples
               at ix = cos xb - sin yb + W/2 - 1/2, iy = sin xb + cos yb + H/2 - 1/2, bilinear, taps outside the map are zero
  gather       [s3, interp(s4), interp(s5), dino] along the channels, optionally the mean over R rotated copies turned back
  group_norm   biased variance per (image, group), eps 1e-5
  conv3x3      stride 1, zero padding 1
  block        the bottleneck block: conv1 GN ReLU conv2 GN ReLU conv3 GN + (shortcut GN, or the input where the block has none), ReLU
  network      softmax(mixing_weights)-weighted sum of the levels' blocks
"""
import math

import numpy as np

EPS = 1e-5


def _axis(n_out, n_in):
    """(i0, i1, lam) of F.interpolate's bilinear taps along one axis"""
    if n_out == n_in:
        i = np.arange(n_out)
        return i, i, np.zeros(n_out)
    src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), src - i0


def interp(x, size):
    """x (B, C, h, w) -> (B, C, P_h, P_w)"""
    x = np.asarray(x, np.float64)
    y0, y1, ly = _axis(size[0], x.shape[2])
    x0, x1, lx = _axis(size[1], x.shape[3])
    top = x[:, :, y0][:, :, :, x0] * (1 - lx) + x[:, :, y0][:, :, :, x1] * lx
    bot = x[:, :, y1][:, :, :, x0] * (1 - lx) + x[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def rotate(x, angle):
    """x (B, C, H, W), angle in degrees, positive = counter-clockwise"""
    x = np.asarray(x, np.float64)
    H, W = x.shape[2:]
    t = math.radians(angle)
    cos, sin = math.cos(t), math.sin(t)
    xb = np.arange(W)[None, :] - W / 2 + 0.5
    yb = np.arange(H)[:, None] - H / 2 + 0.5
    ix = cos * xb - sin * yb + W / 2 - 0.5
    iy = sin * xb + cos * yb + H / 2 - 0.5
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    tx, ty = ix - x0, iy - y0
    out = np.zeros_like(x)
    for dy, dx, w in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
        yy, xx = y0 + dy, x0 + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        vals = x[:, :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        out += np.where(inside, w, 0.0) * np.where(inside, vals, 0.0)
    return out


def gather(sources, size=None, num_rotations=1, step_deg=0.0):
    """sources: arrays (R B, C_s, h_s, w_s) in rotation-major order -> (B, sum C_s, P_h, P_w): every source interpolated to `size` (None:
    the first source's), copy r turned back by -r step_deg, the mean over r"""
    size = tuple(sources[0].shape[2:]) if size is None else tuple(size)
    cat = np.concatenate([interp(s, size) for s in sources], axis=1)
    R = int(num_rotations)
    parts = np.split(cat, R, axis=0)
    total = np.zeros_like(parts[0])
    for r in range(R):
        total += parts[r] if (r == 0 or step_deg == 0.0) else rotate(parts[r], -r * step_deg)
    return total / R


def rows(x):
    """(B, C, H, W) -> (B, H W, C): the layout of the device route"""
    x = np.asarray(x)
    return x.transpose(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])


def group_stats(x, G):
    """x (B, C, ...) -> (mean, rstd), each (B, G)"""
    x = np.asarray(x, np.float64)
    g = x.reshape(x.shape[0], G, -1)
    mean = g.mean(axis=2)
    var = ((g - mean[:, :, None]) ** 2).mean(axis=2)
    return mean, 1.0 / np.sqrt(var + EPS)


def group_norm(x, G, gamma, beta):
    x = np.asarray(x, np.float64)
    mean, rstd = group_stats(x, G)
    g = (x.reshape(x.shape[0], G, -1) - mean[:, :, None]) * rstd[:, :, None]
    shape = (1, -1) + (1,) * (x.ndim - 2)
    return g.reshape(x.shape) * np.asarray(gamma, np.float64).reshape(shape) + np.asarray(beta, np.float64).reshape(shape)


def conv1x1(x, w):
    return np.einsum("bchw,oc->bohw", np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(w.shape[0], -1))


def conv3x3(x, w):
    """x (B, C_in, H, W), w (C_out, C_in, 3, 3) -> (B, C_out, H, W)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, _, H, W = x.shape
    pad = np.zeros((B, x.shape[1], H + 2, W + 2))
    pad[:, :, 1:-1, 1:-1] = x
    out = np.zeros((B, w.shape[0], H, W))
    for dy in range(3):
        for dx in range(3):
            out += np.einsum("bchw,oc->bohw", pad[:, :, dy:dy + H, dx:dx + W], w[:, :, dy, dx])
    return out


def block(x, state, prefix, G):
    """the bottleneck block whose parameters are state[prefix + 'conv1.weight'] ..."""
    p = lambda name: np.asarray(state[prefix + name], np.float64)
    gn = lambda y, conv: group_norm(y, G, p(conv + ".norm.weight"), p(conv + ".norm.bias"))
    y = np.maximum(gn(conv1x1(x, p("conv1.weight")), "conv1"), 0.0)
    y = np.maximum(gn(conv3x3(y, p("conv2.weight")), "conv2"), 0.0)
    y = gn(conv1x1(y, p("conv3.weight")), "conv3")
    short = gn(conv1x1(x, p("shortcut.weight")), "shortcut") if prefix + "shortcut.weight" in state else np.asarray(x, np.float64)
    return np.maximum(y + short, 0.0)


def network(batch, state, feature_dims, G):
    """{'y': (B, projection_dim, H, W), 'levels': the blocks' outputs, 'mix': the softmax weights}"""
    batch = np.asarray(batch, np.float64)
    mw = np.asarray(state["mixing_weights"], np.float64)
    mix = np.exp(mw - mw.max())
    mix /= mix.sum()
    levels, start = [], 0
    for l, dim in enumerate(feature_dims):
        levels.append(block(batch[:, start:start + dim], state, f"bottleneck_layers.{l}.0.", G))
        start += dim
    return {"y": sum(m * v for m, v in zip(mix, levels)), "levels": levels, "mix": mix}

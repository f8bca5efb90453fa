"""
The rotation the reference takes from torchvision (torchvision.transforms.functional.rotate(img, angle, BILINEAR), SDDINO.py:76,83,87):
the image rotation in front of the backbone and the rotation of the feature maps back.  torchvision is not a dependency of this package,
so this is a RESTATEMENT of its tensor path (an inverse affine grid about the image centre, then grid_sample with align_corners=False,
bilinear, zero padding), not a call into it, and it is not pinned against torchvision by any test here: it is pinned to torch.rot90 for
multiples of 90 degrees on square maps and to the float64 restatement of the tests.
"""
import math

import torch
import torch.nn.functional as F


def rotate(img, angle):
    """img (..., H, W) floating point, angle in degrees, positive = counter-clockwise, about the image centre, same size, bilinear, zero
    fill.  With t = radians(angle), xb = x - W/2 + 1/2, yb = y - H/2 + 1/2, output pixel (y, x) samples the input at
    ix = cos t xb - sin t yb + W/2 - 1/2, iy = sin t xb + cos t yb + H/2 - 1/2."""
    if img.dim() < 2 or not img.is_floating_point():
        raise ValueError("rotate: a floating-point tensor (..., H, W)")
    H, W = img.shape[-2:]
    t = math.radians(float(angle))
    cos, sin = math.cos(t), math.sin(t)
    dt = img.dtype if img.dtype in (torch.float32, torch.float64) else torch.float32
    xb = torch.arange(W, dtype=dt, device=img.device) - W / 2 + 0.5
    yb = torch.arange(H, dtype=dt, device=img.device) - H / 2 + 0.5
    # grid_sample's normalised coordinates with align_corners=False: pixel i sits at (2 i + 1) / n - 1
    gx = (cos * xb[None, :] - sin * yb[:, None]) * (2.0 / W)
    gy = (sin * xb[None, :] + cos * yb[:, None]) * (2.0 / H)
    flat = img.reshape((-1, 1, H, W)) if img.dim() < 4 else img.reshape((-1,) + tuple(img.shape[-3:]))
    grid = torch.stack((gx, gy), dim=-1)[None].expand(flat.shape[0], H, W, 2)
    out = F.grid_sample(flat.to(dt), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out.to(img.dtype).reshape(img.shape)

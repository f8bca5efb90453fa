"""Shared by the tests of the JBU apply's backward (CPU and GPU): the oracle, its floors and a float64 restatement of the adjoint.

  oracle       the reference's expressions -- F.interpolate bicubic (align_corners=False), F.pad reflect by 3, adaptive_conv's tap loop --
               under autograd in float64 on the inputs of jbu_checks.seeded_stage (its source and its float32 kernels), with the
               upstream gradient numpy.random.default_rng(5).standard_normal(out.shape) rounded to float32 (what a kernel is handed), or
               with the all-ones gradient of out.sum().  That torch route is pinned to the reference's recorded run by
               tests/test_jbu_cpu.py.
  floor        the same expressions in float32 on the CPU against the float64 result, relative to max |float64 gradient|, measured on
               the very inputs of each case.  The bound is lift_checks.bound(floor, ref) = (4 floor + 2^-23) max |ref|.
  restatement  NumPy float64 from the definitions, sharing nothing with torch's backward: per axis P = A src with A of (2 n + 6) x n
               built explicitly (axis_matrix: row p holds the four bicubic weights of upsampled index reflect(p - 3) on its clamped
               texels, so the border folds are sums of matrix entries), gsrc = Ay^T gP Ax with gP the scatter of gout * kernel on the
               padded grid, gfilt by its definition.
References are computed once per case, shared and read-only."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

import jbu_checks as jc
import jbu_restate as rs
import lift_checks as lc

R, D = 3, 7
SOURCE_TILE = 10          # source texels per axis of a workgroup of dm_jbu_apply_bwd_source_f32 (dm_jbu_bwd.hip: BS_T)
# (B, C, h, w): the four of tests/test_gpu_jbu.py, then one texel more than the source kernel's tile in both directions, then a shape
# whose rows have a tile that touches no border (texels 10 .. 19 of 24) and whose columns fill the padded window to its last index (13),
# then the smallest output (64 tiles of 16 x 32) whose channel sum dm_jbu_apply_bwd_filters_f32 does not cut into chunks
SHAPES = [(1, 1, 2, 2), (2, 5, 3, 2), (1, 70, 5, 7), (1, 3, 9, 17), (1, 3, SOURCE_TILE + 1, SOURCE_TILE + 1), (1, 2, 24, 13),
          (1, 2, 64, 128)]
bound, check = lc.bound, lc.check


# ---------------------------------------------------------------------------------------------------------------- restatement
def axis_matrix(n):
    """A (2 n + 6, n) float64: padded = A @ source along one axis"""
    N = 2 * n
    A = np.zeros((N + 2 * R, n))
    for p in range(N + 2 * R):
        u = p - R
        u = -u if u < 0 else (2 * (N - 1) - u if u >= N else u)
        coord = (u + 0.5) * n / N - 0.5
        base = int(np.floor(coord))
        wts = rs._cubic_weights(np.float64(coord - base))
        for q in range(4):
            A[p, min(max(base - 1 + q, 0), n - 1)] += wts[q]
    return A


def restate(src, filt, gout):
    """(gsrc (B, C, h, w), gfilt (B, H, W, 49)) of out = apply(src, filt) under the upstream gradient gout, float64"""
    src, filt, gout = (np.asarray(a, np.float64) for a in (src, filt, gout))
    B, Cw, h, w = src.shape
    H, W = 2 * h, 2 * w
    Ay, Ax = axis_matrix(h), axis_matrix(w)
    P = np.einsum("py,bcyx,qx->bcpq", Ay, src, Ax)
    gP = np.zeros((B, Cw, H + 2 * R, W + 2 * R))
    gfilt = np.zeros((B, H, W, D * D))
    for i in range(D):
        for j in range(D):
            gP[:, :, i:i + H, j:j + W] += gout * filt[:, None, :, :, i * D + j]
            gfilt[..., i * D + j] = (gout * P[:, :, i:i + H, j:j + W]).sum(1)
    return np.einsum("py,bcpq,qx->bcyx", Ay, gP, Ax), gfilt


# ---------------------------------------------------------------------------------------------------------------- oracle
def upstream(shape, kind="normal"):
    """the upstream gradient of an output of this shape, float32: 'normal' seeded, 'ones' that of out.sum()"""
    if kind == "ones":
        return np.ones(shape, np.float32)
    return np.random.default_rng(5).standard_normal(shape).astype(np.float32)


def _autograd(src, filt, gout, dtype):
    from densematcher_amd.featup.adaptive_conv import adaptive_conv
    s = torch.from_numpy(np.array(src)).to(dtype).requires_grad_(True)
    f = torch.from_numpy(np.array(filt)).to(dtype).requires_grad_(True)
    H, W = f.shape[1:3]
    hr = F.pad(F.interpolate(s, size=(H, W), mode="bicubic", align_corners=False), [R] * 4, mode="reflect")
    out = adaptive_conv(hr, f.reshape(f.shape[:3] + (D, D)), route="torch")
    out.backward(torch.from_numpy(np.array(gout)).to(dtype))
    return s.grad.numpy(), f.grad.numpy()


def _floor(got32, ref64):
    return float(np.abs(np.asarray(got32, np.float64) - ref64).max() / np.abs(ref64).max())


@functools.lru_cache(maxsize=None)
def oracle(shape, kind="normal", half=False):
    """dict for seeded_stage(*shape): src (float32; rounded to fp16 and back when half: what a kernel reading fp16 is handed), filt
    (float32), gout (float32), gsrc64, gfilt64, floor_gsrc, floor_gfilt; arrays read-only"""
    st = jc.seeded_stage(*shape)
    src = st["src"].astype(np.float16).astype(np.float32) if half else st["src"]
    gout = upstream(st["apply64"].shape, kind)
    gsrc64, gfilt64 = _autograd(src, st["f32"], gout, torch.float64)
    gsrc32, gfilt32 = _autograd(src, st["f32"], gout, torch.float32)
    d = {"src": src, "filt": st["f32"], "gout": gout, "gsrc64": gsrc64, "gfilt64": gfilt64,
         "floor_gsrc": _floor(gsrc32, gsrc64), "floor_gfilt": _floor(gfilt32, gfilt64)}
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------- through a module
def _module_grads(up, src, g, gout, dtype):
    up = copy.deepcopy(up).to(dtype).eval()
    s = torch.from_numpy(np.array(src)).to(dtype).requires_grad_(True)
    out = up(s, torch.from_numpy(np.array(g)).to(dtype), route="torch")
    out.backward(torch.from_numpy(np.array(gout)).to(dtype))
    grads = {"source": s.grad.numpy()}
    grads.update({n: p.grad.numpy() for n, p in up.named_parameters()})
    return grads


@functools.lru_cache(maxsize=None)
def module_oracle(shape):
    """seeded_stage(*shape)'s module on the torch route in eval mode: {'gout', 'grads64': {'source' | parameter name: array},
    'floors': the float32 run of the same route on the CPU against it, per tensor}"""
    st = jc.seeded_stage(*shape)
    gout = upstream(st["out64"].shape)
    g64 = _module_grads(st["up"], st["src"], st["g"], gout, torch.float64)
    g32 = _module_grads(st["up"], st["src"], st["g"], gout, torch.float32)
    for a in g64.values():
        a.setflags(write=False)
    gout.setflags(write=False)
    return {"gout": gout, "grads64": g64, "floors": {n: _floor(g32[n], g64[n]) for n in g64}}

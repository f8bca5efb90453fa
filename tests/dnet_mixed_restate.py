"""
The mixed-precision backward of DiffusionNet (dm_dnet_linear_bwd_data_f16 / dm_dnet_linear_bwd_weight_f16, dm_dnet_diffuse_bwd_f16,
dm_dnet_gradfeat_bwd_f16) restated in NumPy float64 for ONE mesh with the declared roundings to fp16 applied, an entrywise bound for
each kernel, the whole route (forward and backward) emulated on the CPU, and the masked oracle the whole-network tests compare with.

Error model: that of tests/dnet_half_restate.py.  U32 = 2^-24, U16 = 2^-11.
  * A product of two fp16 numbers is exact in fp32; a sum of n of them accumulated in fp32 in a fixed order errs by at most
    (n + 2) U32 sum |a_j b_j| (up to two more fp32 roundings on the way to the stored value).
  * A declared rounding of an INTERMEDIATE v to fp16 contributes U16 |v_hat| + TINY16, propagated through the magnitudes of what
    follows.  The kernel restatements do NOT round their intermediates unless round_mid=True (the spectrum of the diffusion; gX, gY, U, V
    as matrix operands): their reference value is the exact one and the rounding is a term of the bound.  Roundings of a kernel's INPUTS
    (dZ, an fp32 source, dO, x) are part of the definition and always applied.
  * fp32 elementwise steps (the gather chains, p, U, V, the assembly of dgX / dgY) are bounded as tests/dnet_backward_restate.py bounds
    them, with (n + 4) u per chain of n.
SLACK = 1 + 2^-9 carries the second-order terms.  Nothing here is fitted to a kernel's output.

The masked oracle.  With fp16 forward errors of about 5e-4 of a layer's largest entry no input keeps every ReLU preactivation of a
network on the side a float64 run puts it, and a flipped mask is a gradient error that says nothing about the backward kernels.  So
every run under test is compared with masked_network: the dense float64 network of dnet_backward_restate.dense_network on the
fp16-rounded matrices (rounded_parameters), every ReLU replaced by multiplication with a given 0/1 mask -- the masks of that very run.
"""
import numpy as np
import torch
import torch.nn as nn

import dnet_backward_restate as br
import dnet_half_restate as hr
import dnet_layers_restate as rs
from dnet_half_restate import h16, half_operands

U32, U16, TINY16, SLACK = hr.U32, hr.U16, hr.TINY16, hr.SLACK
f64 = rs.f64


def as_operand(a):
    """an operand as the kernels stage it: a float16 array as it is, anything else rounded to fp16; float64"""
    return h16(a)


# --------------------------------------------------------------------------------------------------------------------- linear
def linear_backward(dY, srcs, W_h, Y=None):
    """one mesh: dY (N, C_out) fp32, srcs a list of (N, w_s) fp32 or fp16, W_h (C_out, sum w_s) fp16, Y the saved fp32 output or None.
    dZ = fp16(dY * [Y > 0]).  Returns ([d_src], dW, db)"""
    dZ = h16(br.masked(dY, Y))
    d = dZ @ f64(W_h)
    offs = np.cumsum([0] + [np.shape(s)[-1] for s in srcs])
    x = np.concatenate([as_operand(s) for s in srcs], axis=-1)
    return [d[:, offs[i]:offs[i + 1]] for i in range(len(srcs))], dZ.T @ x, dZ.sum(axis=0)


def linear_backward_bound(dY, srcs, W_h, Y=None):
    dZ = np.abs(h16(br.masked(dY, Y)))
    N, Co = dZ.shape
    d = (Co + 2) * U32 * SLACK * (dZ @ np.abs(f64(W_h)))
    offs = np.cumsum([0] + [np.shape(s)[-1] for s in srcs])
    x = np.abs(np.concatenate([as_operand(s) for s in srcs], axis=-1))
    return [d[:, offs[i]:offs[i + 1]] for i in range(len(srcs))], (N + 2) * U32 * SLACK * (dZ.T @ x), (N + 2) * U32 * SLACK * dZ.sum(axis=0)


# --------------------------------------------------------------------------------------------------------------------- diffuse
def diffuse_backward(dO, x, mass, evals, evecs, times, round_mid=False):
    """one mesh.  dx: the forward with the two matrix operands exchanged; dtimes with respect to the clamped times"""
    eh, mh, e1, e2 = half_operands(mass, evecs)
    coef = hr.coefficients(evals, times)
    g = eh.T @ h16(dO)
    d = np.ldexp(coef * g, 14 - e1 - e2)
    dx = np.ldexp(mh @ (h16(d) if round_mid else d), -14)
    dt = None
    if x is not None:
        s = mh.T @ h16(x)
        T = np.ldexp(f64(evals)[:, None] * coef * g * s, -(e1 + e2))
        dt = -(T.astype(np.float32).astype(np.float64) if round_mid else T).sum(axis=0)
    return dx, dt


def diffuse_backward_bound(dO, x, mass, evals, evecs, times):
    N, K = np.shape(evecs)
    eh, mh, e1, e2 = half_operands(mass, evecs)
    eh, mh, coef = np.abs(eh), np.abs(mh), hr.coefficients(evals, times)
    G = eh.T @ np.abs(h16(dO))
    scale = 2.0 ** (14 - e1 - e2)
    # dx: hr.diffuse_bound with the operands exchanged
    e_d = scale * coef * ((N + 2) * U32 * G + 2 * U32 * G)
    d = scale * coef * G
    e_d = e_d + U16 * (d + e_d) + TINY16
    dx = SLACK * 2.0 ** -14 * (mh @ e_d + (K + 2) * U32 * (mh @ (d + e_d)))
    # dtimes: two accumulators over N, coef from another exp() (2 u), the rounding of T, the K additions, the sum over the meshes' one
    S = mh.T @ np.abs(h16(x))
    dt = SLACK * (2 * (N + 2) + K + 6) * U32 * (np.abs(f64(evals))[:, None] * coef * G * S).sum(axis=0) * 2.0 ** -(e1 + e2)
    return dx, dt


# --------------------------------------------------------------------------------------------------------------------- gradient features
def gradfeat_backward(dO, x, Gx, Gy, A_re_h, A_im_h=None, round_mid=False):
    """one mesh: x fp32 (not rounded), A_re_h / A_im_h fp16.  round_mid: gX, gY, U, V rounded as matrix operands, as the kernel does.
    Returns (dx, dA_re, dA_im or None)"""
    Gx, Gy, R = f64(Gx), f64(Gy), f64(A_re_h)
    I = np.zeros_like(R) if A_im_h is None else f64(A_im_h)
    op = h16 if round_mid else (lambda a: a)
    gX, gY = Gx @ f64(x), Gy @ f64(x)
    mX, mY = op(gX), op(gY)
    b_re, b_im = mX @ R.T - mY @ I.T, mY @ R.T + mX @ I.T
    out = np.tanh(gX * b_re + gY * b_im)
    p = f64(dO) * (1.0 - out * out)
    Uu, V = p * gX, p * gY
    mU, mV = op(Uu), op(V)
    dgX = p * b_re + mU @ R + mV @ I
    dgY = p * b_im - mU @ I + mV @ R
    return Gx.T @ dgX + Gy.T @ dgY, mU.T @ mX + mV.T @ mY, None if A_im_h is None else mV.T @ mX - mU.T @ mY


def gradfeat_backward_bound(dO, x, Gx, Gy, A_re_h, A_im_h=None):
    Gx, Gy, x, dO = f64(Gx), f64(Gy), f64(x), np.abs(f64(dO))
    N, C = x.shape
    pattern = (Gx != 0) | (Gy != 0)
    L = np.maximum(np.count_nonzero(pattern, axis=1), 1)[:, None]
    Lt = np.maximum(np.count_nonzero(pattern, axis=0), 1)[:, None]
    U = U32
    # ---- the forward's quantities (dnet_half_restate.gradfeat_bound); h.: the error of the value as a rounded matrix operand
    eX, eY = (L + 4) * U * (np.abs(Gx) @ np.abs(x)), (L + 4) * U * (np.abs(Gy) @ np.abs(x))
    aX, aY = np.abs(Gx @ x) + eX, np.abs(Gy @ x) + eY
    hX, hY = eX + U16 * aX + TINY16, eY + U16 * aY + TINY16
    R = np.abs(f64(A_re_h))
    I = np.zeros_like(R) if A_im_h is None else np.abs(f64(A_im_h))
    Bre, Bim = aX @ R.T + aY @ I.T, aY @ R.T + aX @ I.T
    eBre = hX @ R.T + hY @ I.T + (C + 4) * U * Bre
    eBim = hY @ R.T + hX @ I.T + (C + 4) * U * Bim
    e_out = eX * Bre + aX * eBre + eY * Bim + aY * eBim + 4 * U * (aX * Bre + aY * Bim) + 4 * U
    # ---- the backward
    ep, ap = dO * (2 * e_out + 2 * U), dO
    eU, aU = ep * aX + ap * eX + U * ap * aX, ap * aX
    eV, aV = ep * aY + ap * eY + U * ap * aY, ap * aY
    hU, hV = eU + U16 * (aU + eU) + TINY16, eV + U16 * (aV + eV) + TINY16
    a_dgX, a_dgY = ap * Bre + aU @ R + aV @ I, ap * Bim + aU @ I + aV @ R
    e_dgX = ep * Bre + ap * eBre + U * ap * Bre + hU @ R + hV @ I + (C + 4) * U * (aU @ R + aV @ I) + 2 * U * a_dgX
    e_dgY = ep * Bim + ap * eBim + U * ap * Bim + hU @ I + hV @ R + (C + 4) * U * (aU @ I + aV @ R) + 2 * U * a_dgY
    dx = np.abs(Gx).T @ e_dgX + np.abs(Gy).T @ e_dgY + (2 * Lt + 4) * U * (np.abs(Gx).T @ a_dgX + np.abs(Gy).T @ a_dgY)
    dRe = hU.T @ (aX + hX) + aU.T @ hX + hV.T @ (aY + hY) + aV.T @ hY + (N + 5) * U * (aU.T @ aX + aV.T @ aY)
    dIm = hV.T @ (aX + hX) + aV.T @ hX + hU.T @ (aY + hY) + aU.T @ hY + (N + 5) * U * (aV.T @ aX + aU.T @ aY)
    return SLACK * dx, SLACK * dRe, None if A_im_h is None else SLACK * dIm


# --------------------------------------------------------------------------------------------------------------------- the route, emulated
npy = lambda t: t.detach().cpu().numpy()
t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


class _Linear(torch.autograd.Function):
    """dm_dnet_linear_f16 / dm_dnet_linear_bwd_*_f16 of one mesh with exact sums (float64 tensors that hold the values of the route)"""

    @staticmethod
    def forward(ctx, relu, W, bias, resid, *srcs):
        W_h = h16(npy(W).astype(np.float32))
        xs = [npy(s).astype(np.float32) for s in srcs]
        z = hr.linear(xs, W_h, npy(bias), None, relu).astype(np.float32)          # what the kernel hands on is fp32
        ctx.saved, ctx.has_resid = (xs, W_h, z if relu else None), resid is not None
        y = z.astype(np.float64) if resid is None else (z.astype(np.float64) + npy(resid)).astype(np.float32).astype(np.float64)
        return t64(y)

    @staticmethod
    def backward(ctx, dy):
        xs, W_h, z = ctx.saved
        d, dW, db = linear_backward(npy(dy).astype(np.float32), xs, W_h, z)
        return (None, t64(dW), t64(db), dy if ctx.has_resid else None, *[t64(v) for v in d])


class _Diffuse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ops, x, times):
        mass, evals, evecs = ops
        xv, tv = npy(x).astype(np.float32), npy(times).astype(np.float32)
        ctx.saved = (ops, xv, tv)
        return t64(hr.diffuse(xv, mass, evals, evecs, tv, round_mid=True).astype(np.float32))

    @staticmethod
    def backward(ctx, d_out):
        (mass, evals, evecs), xv, tv = ctx.saved
        dx, dt = diffuse_backward(npy(d_out).astype(np.float32), xv, mass, evals, evecs, tv, round_mid=True)
        return None, t64(dx), t64(dt)


class _GradFeat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, x, A_re, A_im):
        xv = npy(x).astype(np.float32)
        R, I = h16(npy(A_re).astype(np.float32)), None if A_im is None else h16(npy(A_im).astype(np.float32))
        ctx.saved = (G, xv, R, I)
        return t64(hr.gradfeat(xv, G[0], G[1], R, I, round_mid=True)[0].astype(np.float32))

    @staticmethod
    def backward(ctx, d_out):
        G, xv, R, I = ctx.saved
        dx, dR, dI = gradfeat_backward(npy(d_out).astype(np.float32), xv, G[0], G[1], R, I, round_mid=True)
        return None, t64(dx), t64(dR), None if dI is None else t64(dI)


def emulated_network(net, params, xs, ops, edges=None, faces=None):
    """The mixed-precision device route of `net` on the CPU: the forward and backward kernels' restatements with every declared rounding
    applied (round_mid=True), every sum exact, values between the kernels rounded to fp32.  params: float64 leaves of the fp32 masters
    (dnet_backward_restate.leaf_parameters(net, torch.float64)); xs[b] (n_b, C_in) float64; ops from dense_operators(packed,
    torch.float64).  No dropout.  Returns (outputs, ReLU masks: per layer a list over the meshes)."""
    outs, masks = [], []
    for b, (x, (mass, evals, evecs, Gx, Gy)) in enumerate(zip(xs, ops)):
        layer = 0
        op3, G = (npy(mass), npy(evals), npy(evecs)), (npy(Gx), npy(Gy))
        h = _Linear.apply(False, params["first_lin.weight"], params["first_lin.bias"], None, x)
        for i, blk in enumerate(net.blocks):
            p = "block_%d." % i
            xd = _Diffuse.apply(op3, h, params[p + "diffusion.diffusion_time"])
            feats = [h, xd]
            if blk.with_gradient_features:
                A = (params[p + "gradient_features.A_re.weight"], params[p + "gradient_features.A_im.weight"]) if blk.with_gradient_rotations \
                    else (params[p + "gradient_features.A.weight"], None)
                feats.append(_GradFeat.apply(G, xd, *A))
            lins = [(name, m) for name, m in blk.mlp.named_children() if isinstance(m, nn.Linear)]
            for j, (name, m) in enumerate(lins):
                last = j + 1 == len(lins)
                z = _Linear.apply(not last, params[p + "mlp." + name + ".weight"], params[p + "mlp." + name + ".bias"], h if last else None, *feats)
                if not last:
                    if len(masks) <= layer:
                        masks.append([])
                    masks[layer].append(z.detach() > 0)
                    layer += 1
                feats = [z]
            h = feats[0]
        y = _Linear.apply(False, params["last_lin.weight"], params["last_lin.bias"], None, h)
        outs.append(net._tail(y.unsqueeze(0), mass.unsqueeze(0), None if edges is None else edges[b].unsqueeze(0),
                              None if faces is None else faces[b].unsqueeze(0)).squeeze(0))
    return outs, masks


# --------------------------------------------------------------------------------------------------------------------- the masked oracle
def rounded_parameters(net, dtype=torch.float64, device=None):
    """dnet_backward_restate.leaf_parameters with every matrix (nn.Linear.weight, A_re, A_im, A) rounded to fp16 first: leaves that hold
    the values the route multiplies.  The gradient with respect to such a leaf is the master's (the rounding is passed straight through)."""
    out = {}
    for name, p in net.named_parameters():
        v = p.detach()
        if name.endswith("diffusion_time"):
            v = torch.clamp(v, min=1e-8)
        if v.dim() == 2:
            v = v.to(torch.float16)
        out[name] = v.to(dtype=dtype, device=v.device if device is None else device).clone().requires_grad_(p.requires_grad)
    return out


def masked_network(net, params, xs, ops, relu_masks, drop_masks=None, edges=None, faces=None, taps=None):
    """dnet_backward_restate.dense_network with every ReLU replaced by multiplication with relu_masks[layer][b] ((n_b, C) 0/1 or bool).
    taps: a list that receives ("act", t) for every tensor whose gradient a backward kernel stages as a matrix operand (the output of
    every linear in front of its mask product, of every diffusion and of every gradient-feature layer) and ("grad", gX, gY, out) for
    the gradient features' U = p gX, V = p gY.  Returns (outputs, the preactivations per layer and mesh)."""
    outs, pre = [], []
    tap = (lambda *a: None) if taps is None else (lambda *a: taps.append(a))
    for b, (x, (mass, evals, evecs, Gx, Gy)) in enumerate(zip(xs, ops)):
        n, layer, drop = x.shape[0], 0, 0
        h = nn.functional.linear(x, params["first_lin.weight"], params["first_lin.bias"])
        tap("act", h)
        for i, blk in enumerate(net.blocks):
            p = "block_%d." % i
            spec = evecs.transpose(-2, -1) @ (mass.unsqueeze(-1) * h)
            xd = evecs @ (torch.exp(-evals.unsqueeze(-1) * params[p + "diffusion.diffusion_time"].unsqueeze(0)) * spec)
            tap("act", xd)
            feats = [h, xd]
            if blk.with_gradient_features:
                vx, vy = torch.matmul(Gx, xd), torch.matmul(Gy, xd)
                lin = nn.functional.linear
                if blk.with_gradient_rotations:
                    A_re, A_im = params[p + "gradient_features.A_re.weight"], params[p + "gradient_features.A_im.weight"]
                    b_re, b_im = lin(vx, A_re) - lin(vy, A_im), lin(vy, A_re) + lin(vx, A_im)
                else:
                    b_re, b_im = lin(vx, params[p + "gradient_features.A.weight"]), lin(vy, params[p + "gradient_features.A.weight"])
                feats.append(torch.tanh(vx * b_re + vy * b_im))
                tap("act", feats[-1])
                tap("grad", vx, vy, feats[-1])
            z = torch.cat(feats, dim=-1)
            for name, m in blk.mlp.named_children():
                if isinstance(m, nn.Linear):
                    z = nn.functional.linear(z, params[p + "mlp." + name + ".weight"], params[p + "mlp." + name + ".bias"])
                    tap("act", z)
                elif isinstance(m, nn.ReLU):
                    if len(pre) <= layer:
                        pre.append([])
                    pre[layer].append(z)
                    z = z * relu_masks[layer][b].to(device=z.device, dtype=z.dtype)
                    layer += 1
                elif isinstance(m, nn.Dropout):
                    if drop_masks is not None:
                        z = z * (drop_masks[drop][b, :n].to(z.dtype) / (1.0 - m.p))
                    drop += 1
                else:
                    raise NotImplementedError(type(m).__name__)
            h = z + h
        y = nn.functional.linear(h, params["last_lin.weight"], params["last_lin.bias"])
        tap("act", y)
        outs.append(net._tail(y.unsqueeze(0), mass.unsqueeze(0), None if edges is None else edges[b].unsqueeze(0),
                              None if faces is None else faces[b].unsqueeze(0)).squeeze(0))
    return outs, pre


def oracle_gradients(net, xs, ops, gs, relu_masks, scale=1.0, drop_masks=None, faces=None):
    """the gradients of scale * sum_b (y_b * g_b).sum() through the masked oracle in float64 on the CPU: (name -> gradient; 'x': the list
    of leaves), the largest magnitude of a gradient that a backward kernel stages as a matrix operand (masked_network's taps: the
    gradient of every kernel output -- a mask only zeroes entries of it -- and |dO| max(|gX|, |gY|) for U and V) and the outputs"""
    cpu = lambda t: t.detach().double().cpu()
    params = rounded_parameters(net, torch.float64, device="cpu")
    leaves = [cpu(x).requires_grad_() for x in xs]
    ops = [tuple(cpu(t) for t in op) for op in ops]
    taps = []
    ys, pre = masked_network(net, params, leaves, ops, [[cpu(m) for m in layer] for layer in relu_masks],
                             None if drop_masks is None else [m.cpu() for m in drop_masks], faces=None if faces is None else [f.cpu() for f in faces],
                             taps=taps)
    for tp in taps:
        if tp[0] == "act":
            tp[1].retain_grad()
    (scale * sum((y * cpu(g)).sum() for y, g in zip(ys, gs))).backward()
    grads = {name: p.grad for name, p in params.items() if p.grad is not None}
    grads["x"] = leaves
    top = max([float(tp[1].grad.abs().max()) for tp in taps if tp[0] == "act"] +
              [float((tp[3].grad.abs() * torch.maximum(tp[1].detach().abs(), tp[2].detach().abs())).max()) for tp in taps if tp[0] == "grad"])
    return grads, top, ys

"""
The DiffusionNet backward pass restated, in two parts.

1. The three backward kernels (dm_dnet_linear_bwd_data_f32 / dm_dnet_linear_bwd_weight_f32, dm_dnet_diffuse_bwd_f32,
   dm_dnet_gradfeat_bwd_f32) in dense float64 NumPy for ONE mesh, each with a running-error bound for the fp32 kernel, built as
   tests/dnet_layers_restate.py builds its bounds: a kernel sum is a chain of n fmaf's, |s_hat - s| <= (n + 4) u sum |a_j b_j| with up
   to four more roundings on the way to the stored value; an operand that is itself computed carries its own bound e and the
   magnitude bound a = |value| + e, and a product of two such operands errs by at most e_1 a_2 + a_1 e_2 (+ u a_1 a_2 for its
   rounding).  SLACK = 1 + 2^-10 carries the second-order terms.

     linear    dZ = dY * [Y > 0] with the mask taken from the Y that is passed in: exact.  d_src = dZ W over C_out:
               (C_out + 4) u |dZ| |W|.  dW = dZ^T src, db = sum dZ over the N vertices: (N + 4) u |dZ|^T |src|, (N + 4) u sum |dZ|.
     diffuse   g = evecs^T dO, s = evecs^T (mass x) over N: e_g = (N + 4) u G, e_s = (N + 4) u S with G = |evecs|^T |dO|,
               S = |evecs|^T (|mass| |x|).  H = coef g (coef: relative u, the product: u): (N + 5) u coef G, as the forward's spectrum;
               dx = mass (evecs H) over K, the last product one of the four spare roundings:
               ((N + 4) + 1 + (K + 4)) u mass |evecs| (coef G).  A term of dtimes, evals coef g s, has the operand errors
               evals coef (e_g |s| + |g| e_s) <= 2 (N + 4) u evals coef G S and four roundings (coef and three products); the K terms
               are added with K more: (2 (N + 4) + 4 + K + 1) u sum_k evals coef G S.
     gradfeat  the forward's quantities with the forward's bounds (e_X, a_X, .., e_out = e_dots + 4 u).  1 - out^2 has slope <= 2 in
               out and one rounding: e_p = |dO| (2 e_out + 2 u), a_p = |dO|.  U = p gX: e_U = e_p a_X + a_p e_X + u a_p a_X,
               a_U = a_p a_X; V alike.  dgX = p B_re + U A_re + V A_im: the first term errs by e_p B + a_p e_B + u a_p B, each chain
               over C by e_U |A| + (C + 4) u a_U |A|, the two additions by 2 u a_dgX; dgY alike.  dx gathers 2 L_t entries per row
               (L_t: the entries of the transposed row): |G_x|^T e_dgX + |G_y|^T e_dgY + (2 L_t + 4) u (|G_x|^T a_dgX + |G_y|^T a_dgY).
               dA_re = U^T gX + V^T gY over N with one addition: e_U^T a_X + a_U^T e_X + .. + (N + 5) u (a_U^T a_X + a_V^T a_Y);
               dA_im alike.

2. The whole network as dense torch expressions in any dtype (float64 autograd on it is the oracle of the GPU tests): first_lin,
   the spectral diffusion, torch.matmul with the dense gradient operators, the expression of SpatialGradientFeatures, the MLP with
   optional given dropout masks, the skip, last_lin and the module's own tail.
"""
import numpy as np
import torch
import torch.nn as nn

import dnet_layers_restate as rs

U, SLACK, f64 = rs.U, rs.SLACK, rs.f64


# --------------------------------------------------------------------------------------------------------------------- 1. kernels
def masked(dY, Y=None):
    return f64(dY) if Y is None else f64(dY) * (np.asarray(Y) > 0)


def linear_backward(dY, srcs, W, Y=None):
    """one mesh: dY (N, C_out), srcs a list of (N, w_s), W (C_out, sum w_s), Y the saved output or None.  Returns ([d_src], dW, db)"""
    dZ = masked(dY, Y)
    d = dZ @ f64(W)
    offs = np.cumsum([0] + [s.shape[-1] for s in srcs])
    return [d[:, offs[i]:offs[i + 1]] for i in range(len(srcs))], dZ.T @ np.concatenate([f64(s) for s in srcs], axis=-1), dZ.sum(axis=0)


def linear_backward_bound(dY, srcs, W, Y=None):
    dZ = np.abs(masked(dY, Y))
    N, Co = dZ.shape
    d = (Co + 4) * U * SLACK * (dZ @ np.abs(f64(W)))
    offs = np.cumsum([0] + [s.shape[-1] for s in srcs])
    x = np.abs(np.concatenate([f64(s) for s in srcs], axis=-1))
    return [d[:, offs[i]:offs[i + 1]] for i in range(len(srcs))], (N + 4) * U * SLACK * (dZ.T @ x), (N + 4) * U * SLACK * dZ.sum(axis=0)


def diffuse_backward(dO, x, mass, evals, evecs, times):
    """one mesh.  Returns (dx, dtimes), dtimes with respect to the clamped times"""
    E, m = f64(evecs), f64(mass)[:, None]
    coef = rs.coefficients(evals, times)
    g, s = E.T @ f64(dO), E.T @ (m * f64(x))
    return m * (E @ (coef * g)), -(f64(evals)[:, None] * coef * g * s).sum(axis=0)


def diffuse_backward_bound(dO, x, mass, evals, evecs, times):
    N, K = np.shape(evecs)
    E, m = np.abs(f64(evecs)), np.abs(f64(mass))[:, None]
    coef = rs.coefficients(evals, times)
    G, S = E.T @ np.abs(f64(dO)), E.T @ (m * np.abs(f64(x)))
    dx = ((N + 4) + 1 + (K + 4)) * U * SLACK * m * (E @ (coef * G))
    dt = (2 * (N + 4) + 4 + K + 1) * U * SLACK * (np.abs(f64(evals))[:, None] * coef * G * S).sum(axis=0)
    return dx, dt


def gradfeat_backward(dO, x, Gx, Gy, A_re, A_im=None):
    """one mesh.  Returns (dx, dA_re, dA_im or None)"""
    Gx, Gy, R = f64(Gx), f64(Gy), f64(A_re)
    I = np.zeros_like(R) if A_im is None else f64(A_im)
    gX, gY = Gx @ f64(x), Gy @ f64(x)
    b_re, b_im = gX @ R.T - gY @ I.T, gY @ R.T + gX @ I.T
    out = np.tanh(gX * b_re + gY * b_im)
    p = f64(dO) * (1.0 - out * out)
    Uu, V = p * gX, p * gY
    dgX = p * b_re + Uu @ R + V @ I
    dgY = p * b_im - Uu @ I + V @ R
    return Gx.T @ dgX + Gy.T @ dgY, Uu.T @ gX + V.T @ gY, None if A_im is None else V.T @ gX - Uu.T @ gY


def gradfeat_backward_bound(dO, x, Gx, Gy, A_re, A_im=None):
    Gx, Gy, x, dO = f64(Gx), f64(Gy), f64(x), np.abs(f64(dO))
    N, C = x.shape
    pattern = (Gx != 0) | (Gy != 0)
    L = np.maximum(np.count_nonzero(pattern, axis=1), 1)[:, None]
    Lt = np.maximum(np.count_nonzero(pattern, axis=0), 1)[:, None]
    # ---- the forward's quantities (dnet_layers_restate.gradfeat_bound)
    eX, eY = (L + 4) * U * (np.abs(Gx) @ np.abs(x)), (L + 4) * U * (np.abs(Gy) @ np.abs(x))
    aX, aY = np.abs(Gx @ x) + eX, np.abs(Gy @ x) + eY
    R = np.abs(f64(A_re))
    I = np.zeros_like(R) if A_im is None else np.abs(f64(A_im))
    Bre, Bim = aX @ R.T + aY @ I.T, aY @ R.T + aX @ I.T
    eBre = eX @ R.T + eY @ I.T + (C + 4) * U * Bre
    eBim = eY @ R.T + eX @ I.T + (C + 4) * U * Bim
    e_out = eX * Bre + aX * eBre + eY * Bim + aY * eBim + 4 * U * (aX * Bre + aY * Bim) + 4 * U
    # ---- the backward
    ep, ap = dO * (2 * e_out + 2 * U), dO
    eU, aU = ep * aX + ap * eX + U * ap * aX, ap * aX
    eV, aV = ep * aY + ap * eY + U * ap * aY, ap * aY
    a_dgX, a_dgY = ap * Bre + aU @ R + aV @ I, ap * Bim + aU @ I + aV @ R
    e_dgX = ep * Bre + ap * eBre + U * ap * Bre + eU @ R + eV @ I + (C + 4) * U * (aU @ R + aV @ I) + 2 * U * a_dgX
    e_dgY = ep * Bim + ap * eBim + U * ap * Bim + eU @ I + eV @ R + (C + 4) * U * (aU @ I + aV @ R) + 2 * U * a_dgY
    dx = np.abs(Gx).T @ e_dgX + np.abs(Gy).T @ e_dgY + (2 * Lt + 4) * U * (np.abs(Gx).T @ a_dgX + np.abs(Gy).T @ a_dgY)
    dRe = eU.T @ aX + aU.T @ eX + eV.T @ aY + aV.T @ eY + (N + 5) * U * (aU.T @ aX + aV.T @ aY)
    dIm = eV.T @ aX + aV.T @ eX + eU.T @ aY + aU.T @ eY + (N + 5) * U * (aV.T @ aX + aU.T @ aY)
    return SLACK * dx, SLACK * dRe, None if A_im is None else SLACK * dIm


# --------------------------------------------------------------------------------------------------------------------- 2. network
def dense_operators(packed, dtype, device=None):
    """per mesh of a PackedOperators (mass (n), evals (K), evecs (n, K), dense gradX (n, n), dense gradY (n, n)) in `dtype`"""
    to = lambda t: t.to(dtype=dtype, device=packed.device if device is None else device)
    return [(to(packed.mass[b, :n]), to(packed.evals[b]), to(packed.evecs[b, :n]), to(packed.dense_grad(b, "gx")), to(packed.dense_grad(b, "gy")))
            for b, n in enumerate(packed.n_verts)]


def leaf_parameters(net, dtype, device=None):
    """name -> a leaf copy of the parameter in `dtype` that requires grad where the parameter does; the diffusion times clamped in
    float32 first, as LearnedTimeDiffusion.clamp_time leaves them"""
    out = {}
    for name, p in net.named_parameters():
        v = p.detach()
        if name.endswith("diffusion_time"):
            v = torch.clamp(v, min=1e-8)
        out[name] = v.to(dtype=dtype, device=v.device if device is None else device).clone().requires_grad_(p.requires_grad)
    return out


def dense_network(net, params, xs, ops, masks=None, edges=None, faces=None):
    """The network `net` (its structure; the values come from params, leaf_parameters) on a list of meshes: xs[b] (n_b, C_in), ops
    from dense_operators.  masks: None (no dropout), or the keep masks of the nn.Dropout modules in the order in which they are
    called, each (B, N, C) (entry [b, :n_b] is mesh b's; scale 1 / (1 - p)).  Returns (the list of outputs, each what net.forward
    returns for the mesh alone; the list of ReLU preactivations, per layer a list over the meshes)."""
    outs, pre = [], []
    for b, (x, (mass, evals, evecs, Gx, Gy)) in enumerate(zip(xs, ops)):
        n, layer, drop = x.shape[0], 0, 0
        h = nn.functional.linear(x, params["first_lin.weight"], params["first_lin.bias"])
        for i, blk in enumerate(net.blocks):
            p = "block_%d." % i
            spec = evecs.transpose(-2, -1) @ (mass.unsqueeze(-1) * h)
            xd = evecs @ (torch.exp(-evals.unsqueeze(-1) * params[p + "diffusion.diffusion_time"].unsqueeze(0)) * spec)
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
            z = torch.cat(feats, dim=-1)
            for name, m in blk.mlp.named_children():
                if isinstance(m, nn.Linear):
                    z = nn.functional.linear(z, params[p + "mlp." + name + ".weight"], params[p + "mlp." + name + ".bias"])
                elif isinstance(m, nn.ReLU):
                    if len(pre) <= layer:
                        pre.append([])
                    pre[layer].append(z)
                    layer += 1
                    z = torch.relu(z)
                elif isinstance(m, nn.Dropout):
                    if masks is not None:
                        z = z * (masks[drop][b, :n].to(z.dtype) / (1.0 - m.p))
                    drop += 1
                else:
                    raise NotImplementedError(type(m).__name__)
            h = z + h
        y = nn.functional.linear(h, params["last_lin.weight"], params["last_lin.bias"])
        outs.append(net._tail(y.unsqueeze(0), mass.unsqueeze(0), None if edges is None else edges[b].unsqueeze(0),
                              None if faces is None else faces[b].unsqueeze(0)).squeeze(0))
    return outs, pre


def relu_margin(pre):
    """the smallest |z| / max |z| over the ReLU preactivations, each layer against its own largest magnitude (all meshes together)"""
    worst = float("inf")
    for per_mesh in pre:
        z = torch.cat([t.detach().reshape(-1) for t in per_mesh]).abs()
        worst = min(worst, float(z.min() / z.max()))
    return worst


def figures(got, ref):
    """per name max |got - ref| / max |ref| of two dicts of tensors (float64 on the CPU)"""
    out = {}
    for name, r in ref.items():
        r, g = r.detach().double().cpu(), got[name].detach().double().cpu()
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), name
        out[name] = float((g - r).abs().max() / r.abs().max()) if float(r.abs().max()) > 0 else float((g - r).abs().max())
    return out

"""
The fp16 route through DiffusionNet (dm_dnet_linear_f16, dm_dnet_diffuse_f16, dm_dnet_gradfeat_f16) restated in NumPy: the declared
roundings to fp16 applied, every product and sum in float64, and an entrywise bound for each kernel.

Error model (the pattern of vit_restate.linear_bound and dnet_layers_restate.diffuse_bound).  U32 = 2^-24, U16 = 2^-11.
  * A product of two fp16 numbers is exact in fp32.  A sum of n of them accumulated in fp32 in a fixed order, one rounding per addition:
    |s_hat - s| <= gamma_n sum |a_j b_j| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); with up to two more fp32
    roundings on the way to the stored value this is taken as (n + 2) U32 sum |a_j b_j|.
  * A declared rounding of an INTERMEDIATE v to fp16 contributes U16 |v_hat| + TINY16 (TINY16 = 2^-25, half the smallest subnormal,
    covers values below the normal range); what follows propagates it through the magnitudes of its other operand.  The kernel
    restatements below do NOT round their intermediates (d of the diffusion; gX, gY as matrix operands): their reference value is the
    exact one and the rounding is a term of the bound.  round_mid=True applies these roundings too: that is the route itself with exact
    sums, which forward() chains into the whole network.
  * An fp16 output adds U16 |out_hat| + TINY16.
SLACK = 1 + 2^-9 carries the 1 / (1 - n U32) factors and the products of two error terms.  Nothing here is fitted to a kernel's output.

Operands are rounded where the route rounds them: float32 sources and x become fp16(.) -- float16 ones are taken as they are -- and the
diffusion's matrix operands are those of PackedOperators.half_operands(), rebuilt here from their definition.
"""
import numpy as np

import dnet_layers_restate as rs

U32, U16, TINY16 = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
SLACK = 1.0 + 2.0 ** -9

f64 = rs.f64


def h16(a):
    """the fp16 rounding (to nearest even, one rounding from float32 or float64) as float64"""
    return np.asarray(a).astype(np.float16).astype(np.float64)


def half_params(params):
    """a state_dict's arrays after .half(), as float64"""
    return {k: h16(np.asarray(v, np.float32)) for k, v in params.items()}


# --------------------------------------------------------------------------------------------------------------------- linear
def linear(srcs, W, bias=None, resid=None, relu=False, out16=False):
    y = rs.linear([h16(s) for s in srcs], W, bias, resid, relu)
    return h16(y) if out16 else y


def linear_bound(srcs, W, bias=None, resid=None, out16=False):
    x = np.abs(np.concatenate([h16(s) for s in srcs], axis=-1))
    P = x @ np.abs(f64(W)).T
    e = (x.shape[-1] + 2) * U32 * P
    mag = P + e
    if bias is not None:
        mag = mag + np.abs(f64(bias))
        e = e + U32 * mag
    if resid is not None:
        mag = mag + np.abs(f64(resid))
        e = e + U32 * mag
    e = SLACK * e
    return e + U16 * (mag + e) + TINY16 if out16 else e


# --------------------------------------------------------------------------------------------------------------------- diffuse
def window_exponent(a):
    """the integer e with 2^e max |a| in [2^14, 2^15); 0 for zeros"""
    top = float(np.abs(a).max()) if np.size(a) else 0.0
    return 15 - int(np.frexp(top)[1]) if top > 0 else 0


def half_operands(mass, evecs):
    """one mesh: (evecs_h, mevecs_h, e1, e2) with evecs_h = fp16(2^e1 evecs), mevecs_h = fp16(2^e2 mass * evecs), as float64"""
    ev, me = f64(evecs), f64(mass)[:, None] * f64(evecs)
    e1, e2 = window_exponent(ev), window_exponent(me)
    return h16(np.ldexp(ev, e1)), h16(np.ldexp(me, e2)), e1, e2


def coefficients(evals, times):
    """exp(-evals_k max(t_c, 1e-8)) in float64, rounded once to fp32; the clamp in fp32"""
    return rs.coefficients(evals, np.asarray(times).astype(np.float32)).astype(np.float32).astype(np.float64)


def diffuse(x, mass, evals, evecs, times, round_mid=False):
    """one mesh: x (N,C), mass (N), evals (K), evecs (N,K), times (C)"""
    eh, mh, e1, e2 = half_operands(mass, evecs)
    d = np.ldexp(coefficients(evals, times) * (mh.T @ h16(x)), 14 - e1 - e2)
    return np.ldexp(eh @ (h16(d) if round_mid else d), -14)


def diffuse_bound(x, mass, evals, evecs, times):
    N, K = np.shape(evecs)
    eh, mh, e1, e2 = half_operands(mass, evecs)
    eh, mh, coef = np.abs(eh), np.abs(mh), coefficients(evals, times)
    S = mh.T @ np.abs(h16(x))
    scale = 2.0 ** (14 - e1 - e2)
    # the accumulated spectrum; coef from another exp() may differ by one unit of fp32; then the one rounding of d
    e_d = scale * coef * ((N + 2) * U32 * S + 2 * U32 * S)
    d = scale * coef * S
    e_d = e_d + U16 * (d + e_d) + TINY16
    return SLACK * 2.0 ** -14 * (eh @ e_d + (K + 2) * U32 * (eh @ (d + e_d)))


# --------------------------------------------------------------------------------------------------------------------- gradient features
def gradfeat(x, Gx, Gy, A_re, A_im=None, round_mid=False):
    """one mesh: x (N,C) float32 (NOT rounded: the gradients come from the fp32 x), Gx / Gy dense (N,N), A_re / A_im (C,C) fp16.
    Returns (features, the values in front of tanh)"""
    gX, gY = f64(Gx) @ f64(x), f64(Gy) @ f64(x)
    mX, mY = (h16(gX), h16(gY)) if round_mid else (gX, gY)
    if A_im is None:
        b_re, b_im = mX @ f64(A_re).T, mY @ f64(A_re).T
    else:
        b_re = mX @ f64(A_re).T - mY @ f64(A_im).T
        b_im = mY @ f64(A_re).T + mX @ f64(A_im).T
    dots = gX * b_re + gY * b_im
    return np.tanh(dots), dots


def gradfeat_bound(x, Gx, Gy, A_re, A_im=None):
    Gx, Gy, x = f64(Gx), f64(Gy), f64(x)
    C = x.shape[1]
    L = np.maximum(np.count_nonzero((Gx != 0) | (Gy != 0), axis=1)[:, None], 1)
    eX, eY = (L + 2) * U32 * (np.abs(Gx) @ np.abs(x)), (L + 2) * U32 * (np.abs(Gy) @ np.abs(x))       # the fp32 gather
    aX, aY = np.abs(Gx @ x) + eX, np.abs(Gy @ x) + eY
    hX, hY = eX + U16 * aX + TINY16, eY + U16 * aY + TINY16                                             # as operands: rounded once
    R = np.abs(f64(A_re)).T
    I = np.zeros_like(R) if A_im is None else np.abs(f64(A_im)).T
    Bre, Bim = aX @ R + aY @ I, aY @ R + aX @ I
    eBre = hX @ R + hY @ I + (C + 4) * U32 * Bre
    eBim = hY @ R + hX @ I + (C + 4) * U32 * Bim
    e_dots = eX * Bre + aX * eBre + eY * Bim + aY * eBim + 4 * U32 * (aX * Bre + aY * Bim)
    return SLACK * e_dots + 4 * U32


# --------------------------------------------------------------------------------------------------------------------- whole network
def forward(cfg, params, x, mass, evals, evecs, Gx=None, Gy=None, faces=None, out16=True):
    """The route on one mesh or a batch, every declared rounding applied and every sum exact: dnet_layers_restate.forward with the three
    kernels above (round_mid=True).  params: the state_dict after .half() (half_params); x (N,C_in) / (B,N,C_in) or a list of up to three
    sources, each float16 or float32.  out16: the network's output rounded to fp16, as the module returns it, in front of the
    outputs_at / last_activation tail (float64 here).  Returns the output."""
    srcs = list(x) if isinstance(x, (list, tuple)) else [x]
    flat = np.ndim(srcs[0]) == 2
    if flat:
        srcs, mass, evals, evecs = [s[None] for s in srcs], mass[None], evals[None], evecs[None]
        Gx, Gy = (None, None) if Gx is None else (Gx[None], Gy[None])
        faces = None if faces is None else faces[None]
    outs = []
    for b in range(len(srcs[0])):
        h = linear([s[b] for s in srcs], params["first_lin.weight"], params["first_lin.bias"])
        for i in range(cfg["N_block"]):
            p = "block_%d." % i
            xd = diffuse(h.astype(np.float32), mass[b], evals[b], evecs[b], params[p + "diffusion.diffusion_time"], round_mid=True)
            parts = [h, xd]
            if cfg["with_gradient_features"]:
                A = ("gradient_features.A_re.weight", "gradient_features.A_im.weight") if cfg["with_gradient_rotations"] else ("gradient_features.A.weight",)
                parts.append(gradfeat(xd, Gx[b], Gy[b], *[params[p + a] for a in A], round_mid=True)[0])
            names = sorted({k[:-len(".weight")] for k in params if k.startswith(p + "mlp.") and k.endswith(".weight")})
            for j, name in enumerate(names):
                last = j + 1 == len(names)
                parts = [linear([q.astype(np.float32) for q in parts], params[name + ".weight"], params[name + ".bias"], resid=h if last else None, relu=not last)]
            h = parts[0]
        y = linear([h.astype(np.float32)], params["last_lin.weight"], params["last_lin.bias"], out16=out16)
        if cfg["outputs_at"] == "faces":
            y = y[np.asarray(faces[b], np.int64)].mean(axis=1)
        elif cfg["outputs_at"] == "global_mean":
            y = (y * f64(mass[b])[:, None]).sum(axis=0) / f64(mass[b]).sum()
        elif cfg["outputs_at"] != "vertices":
            raise NotImplementedError(cfg["outputs_at"])
        if cfg.get("last_activation") == "log_softmax":
            y = rs.log_softmax(y)
        outs.append(y)
    return outs[0] if flat else np.stack(outs)


def rms(a, ref):
    return float(np.sqrt(np.mean((f64(a) - f64(ref)) ** 2)))

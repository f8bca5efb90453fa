"""
The DiffusionNet forward pass and the formulas of its three kernels (dm_dnet_linear_f32, dm_dnet_diffuse_f32, dm_dnet_gradfeat_f32)
restated in dense float64 NumPy, each with a running-error bound for the fp32 kernel.

Error model.  u = 2^-24 is the unit roundoff of fp32.  A kernel sum is a chain of n fmaf's in a fixed order (v_mfma_f32_32x32x2_f32,
or fmaf in the gather of the gradient rows), s_j = fl(s_{j-1} + a_j b_j) with one rounding each.  By the standard running-error
analysis (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: |s_hat - s| <= gamma_n sum |a_j b_j|, gamma_n =
n u / (1 - n u)), and with up to four more roundings on the way to the stored value (an operand formed by one product, the bias, the
residual or a difference of two chains, the last store),

    |computed - exact| <= (n + 4) u * (the same expression evaluated on absolute values)          (1)

up to the factor 1 / (1 - (n + 4) u) <= 1 + 2^-10 for every n here, which SLACK carries.

  linear    y = act(x W^T + bias) + resid, n = the summed source width: bound (1) on |x| |W|^T + |bias| + |resid| (ReLU is exact and
            1-Lipschitz).
  diffuse   s = evecs^T (mass * x) is a chain over the N vertices of the mesh (mass * x is one of the four extra roundings):
            |s_hat - s| <= (N + 4) u S, S = |evecs|^T (|mass| |x|).  coef = fl(exp(.)) has relative error u (float64 evaluation, one
            rounding), and coef * s_hat is one more rounding, which the first chain's spare roundings cover: d = coef * s has
            |d_hat - d| <= (N + 5) u coef S.  out = evecs d_hat is a chain over K with operand bound coef S:
            |out_hat - out| <= |evecs| |d_hat - d| + (K + 4) u |evecs| (coef S) = ((N + 4) + 1 + (K + 4)) u |evecs| (coef S).
  gradfeat  gX = G_x x over the L_i stored entries of row i: e_X = (L_i + 4) u |G_x| |x| (e_Y alike); a_X = |gX| + e_X bounds the
            computed magnitude.  B_re = gX A_re^T - gY A_im^T are two chains over C on computed operands and one difference:
            e_Bre = e_X |A_re|^T + e_Y |A_im|^T + (C + 4) u (a_X |A_re|^T + a_Y |A_im|^T), likewise B_im.  dots = gX B_re + gY B_im:
            e_dots = e_X |B_re| + a_X e_Bre + e_Y |B_im| + a_Y e_Bim + 4 u (a_X |B_re| + a_Y |B_im|) with |B| taken as its bound.
            tanh is 1-Lipschitz and tanhf is within 4 u absolute: e_out = e_dots + 4 u.
"""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
TIME_FLOOR = np.float32(1e-8)

f64 = lambda a: np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
def linear(srcs, W, bias=None, resid=None, relu=False):
    x = np.concatenate([f64(s) for s in srcs], axis=-1)
    y = x @ f64(W).T
    if bias is not None:
        y = y + f64(bias)
    if relu:
        y = np.maximum(y, 0.0)
    return y if resid is None else y + f64(resid)


def linear_bound(srcs, W, bias=None, resid=None):
    x = np.abs(np.concatenate([f64(s) for s in srcs], axis=-1))
    mag = x @ np.abs(f64(W)).T
    if bias is not None:
        mag = mag + np.abs(f64(bias))
    if resid is not None:
        mag = mag + np.abs(f64(resid))
    return (x.shape[-1] + 4) * U * SLACK * mag


def coefficients(evals, times):
    """exp(-evals_k max(t_c, 1e-8)): the clamp in fp32 as the reference clamps, the rest in float64"""
    t = np.maximum(np.asarray(times, np.float32), TIME_FLOOR).astype(np.float64)
    return np.exp(-f64(evals)[:, None] * t[None, :])


def diffuse(x, mass, evals, evecs, times):
    """one mesh: x (N,C), mass (N), evals (K), evecs (N,K), times (C)"""
    spec = f64(evecs).T @ (f64(mass)[:, None] * f64(x))
    return f64(evecs) @ (coefficients(evals, times) * spec)


def diffuse_bound(x, mass, evals, evecs, times):
    N, K = np.shape(evecs)
    S = np.abs(f64(evecs)).T @ (np.abs(f64(mass))[:, None] * np.abs(f64(x)))
    return ((N + 4) + 1 + (K + 4)) * U * SLACK * (np.abs(f64(evecs)) @ (coefficients(evals, times) * S))


def dense_rows(row_len, cols, vals, n):
    """(n, n) float64 matrix of ELL rows; slots q >= row_len[i] are not looked at"""
    G = np.zeros((n, n))
    for i in range(n):
        for q in range(int(row_len[i])):
            G[i, int(cols[i, q])] += float(vals[i, q])
    return G


def gradfeat(x, Gx, Gy, A_re, A_im=None):
    """one mesh: x (N,C), Gx / Gy dense (N,N), A_re / A_im (C,C).  Returns (features, the values in front of tanh)"""
    gX, gY = f64(Gx) @ f64(x), f64(Gy) @ f64(x)
    if A_im is None:
        b_re, b_im = gX @ f64(A_re).T, gY @ f64(A_re).T
    else:
        b_re = gX @ f64(A_re).T - gY @ f64(A_im).T
        b_im = gY @ f64(A_re).T + gX @ f64(A_im).T
    dots = gX * b_re + gY * b_im
    return np.tanh(dots), dots


def gradfeat_bound(x, Gx, Gy, A_re, A_im=None):
    Gx, Gy, x = f64(Gx), f64(Gy), f64(x)
    C = x.shape[1]
    L = np.count_nonzero((Gx != 0) | (Gy != 0), axis=1)[:, None]
    L = np.maximum(L, 1)
    eX, eY = (L + 4) * U * (np.abs(Gx) @ np.abs(x)), (L + 4) * U * (np.abs(Gy) @ np.abs(x))
    aX, aY = np.abs(Gx @ x) + eX, np.abs(Gy @ x) + eY
    R = np.abs(f64(A_re)).T
    I = np.zeros_like(R) if A_im is None else np.abs(f64(A_im)).T
    Bre, Bim = aX @ R + aY @ I, aY @ R + aX @ I
    eBre = eX @ R + eY @ I + (C + 4) * U * Bre
    eBim = eY @ R + eX @ I + (C + 4) * U * Bim
    e_dots = eX * Bre + aX * eBre + eY * Bim + aY * eBim + 4 * U * (aX * Bre + aY * Bim)
    return SLACK * e_dots + 4 * U


# ---------------------------------------------------------------------------------------------------------------------
def log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def forward(cfg, params, x, mass, evals, evecs, Gx=None, Gy=None, faces=None):
    """The whole network in float64.  cfg: the constructor's settings (N_block, with_gradient_features, with_gradient_rotations,
    outputs_at, last_activation: None or "log_softmax"); params: name -> array, the state_dict; x (N,C_in) or (B,N,C_in) with mass,
    evals, evecs (and dense Gx, Gy, faces) shaped alike.  Returns (output, [values in front of tanh, per block and mesh])."""
    flat = np.ndim(x) == 2
    if flat:
        x, mass, evals, evecs = x[None], mass[None], evals[None], evecs[None]
        Gx, Gy = (None, None) if Gx is None else (Gx[None], Gy[None])
        faces = None if faces is None else faces[None]
    outs, dots_all = [], []
    for b in range(len(x)):
        h = linear([x[b]], params["first_lin.weight"], params["first_lin.bias"])
        for i in range(cfg["N_block"]):
            p = "block_%d." % i
            xd = diffuse(h, mass[b], evals[b], evecs[b], params[p + "diffusion.diffusion_time"])
            srcs = [h, xd]
            if cfg["with_gradient_features"]:
                if cfg["with_gradient_rotations"]:
                    g, dots = gradfeat(xd, Gx[b], Gy[b], params[p + "gradient_features.A_re.weight"], params[p + "gradient_features.A_im.weight"])
                else:
                    g, dots = gradfeat(xd, Gx[b], Gy[b], params[p + "gradient_features.A.weight"])
                dots_all.append(dots)
                srcs.append(g)
            names = sorted({k[:-len(".weight")] for k in params if k.startswith(p + "mlp.") and k.endswith(".weight")})
            for j, name in enumerate(names):
                last = j + 1 == len(names)
                srcs = [linear(srcs, params[name + ".weight"], params[name + ".bias"], resid=h if last else None, relu=not last)]
            h = srcs[0]
        y = linear([h], params["last_lin.weight"], params["last_lin.bias"])
        if cfg["outputs_at"] == "faces":
            y = y[np.asarray(faces[b], np.int64)].mean(axis=1)
        elif cfg["outputs_at"] == "global_mean":
            y = (y * f64(mass[b])[:, None]).sum(axis=0) / f64(mass[b]).sum()
        elif cfg["outputs_at"] != "vertices":
            raise NotImplementedError(cfg["outputs_at"])
        if cfg.get("last_activation") == "log_softmax":
            y = log_softmax(y)
        outs.append(y)
    return (outs[0] if flat else np.stack(outs)), dots_all

"""
The differentiable device route of DiffusionNet: three torch.autograd.Functions whose forward is the fp32 forward kernel
(dm_dnet_linear_f32, dm_dnet_diffuse_f32, dm_dnet_gradfeat_f32) and whose backward is its gradient kernel (dm_dnet_linear_bwd_*_f32,
dm_dnet_diffuse_bwd_f32, dm_dnet_gradfeat_bwd_f32), and the network composed of them.  Each function saves only what its backward
reads and computes only the gradients that ctx.needs_input_grad asks for.  Dropout, the outputs_at tail and whatever follows stay
ordinary torch operations.

A second set of three (run(..., half=True)) is the mixed-precision route: float32 master parameters, fp16 matrix operands.  Its forward
rounds each matrix (nn.Linear.weight, A_re, A_im, A) to float16 once per call with a torch cast and runs the fp16 forward kernels
(dm_dnet_linear_f16, dm_dnet_diffuse_f16, dm_dnet_gradfeat_f16; biases and times float32, everything between the kernels float32); the
copies live until that call's backward (dm_dnet_linear_bwd_*_f16, dm_dnet_diffuse_bwd_f16, dm_dnet_gradfeat_bwd_f16) and no longer: the
parameters change every step.  The gradients are float32 and go to the float32 masters, the rounding passed straight through.  The
route scales nothing: a gradient entry below fp16's range is lost where it is staged as a matrix operand and one beyond 65504 becomes
infinite, so it is used with torch.amp.GradScaler exactly as torch.autocast is.
"""
import torch
import torch.nn as nn

K_MAX = 1024        # the diffusion kernels' limit on k_eig (dm_dnet_diffuse_f32, dm_dnet_diffuse_bwd_f32)


def _same(A):
    return A


def _rounded(A):
    """a float32 master matrix rounded to float16 for this call (None stays None)"""
    return None if A is None else A.detach().to(torch.float16)


class LinearFn(torch.autograd.Function):
    """act(concat(srcs) W^T + bias) + resid; saved: the sources (for the weight / bias gradient), W as the kernels read it (for a
    source's gradient), the output (relu)."""
    fwd, bwd, matrix = "dnet_linear", "dnet_linear_backward", staticmethod(_same)      # the engine's methods; W as the kernels read it

    @classmethod
    def forward(cls, ctx, eng, nv, relu, W, bias, resid, *srcs):
        if relu and resid is not None:
            raise ValueError(f"{cls.__name__}: relu with resid is not differentiated (the saved output would not show the mask)")
        W = cls.matrix(W)
        y = getattr(eng, cls.fwd)(list(srcs), W, bias, resid, relu=relu, n_verts=nv)
        need = ctx.needs_input_grad
        ctx.eng, ctx.nv, ctx.relu = eng, nv, relu
        ctx.widths = [int(s.shape[-1]) for s in srcs]
        ctx.keep_srcs, ctx.keep_W = bool(need[3] or (bias is not None and need[4])), any(need[6:])
        ctx.save_for_backward(*((list(srcs) if ctx.keep_srcs else []) + ([W] if ctx.keep_W else []) + ([y] if relu else [])))
        return y

    @classmethod
    def backward(cls, ctx, dy):
        need, saved = ctx.needs_input_grad, list(ctx.saved_tensors)
        y = saved.pop() if ctx.relu else None
        W = saved.pop() if ctx.keep_W else None
        srcs = saved if ctx.keep_srcs else ctx.widths
        d_src, dW, db = getattr(ctx.eng, cls.bwd)(dy, srcs, W, y=y, n_verts=ctx.nv, need_src=list(need[6:]), need_weight=need[3], need_bias=need[4])
        return (None, None, None, dW, db, dy if need[5] else None, *d_src)


class DiffuseFn(torch.autograd.Function):
    """the spectral diffusion of x with the (clamped) times; saved: the times, and x for the gradient of the times"""
    fwd, bwd = "dnet_diffuse", "dnet_diffuse_backward"

    @staticmethod
    def operands(packed):                      # what the engine's two methods take between x and the times
        return packed.mass, packed.evals, packed.evecs

    @classmethod
    def forward(cls, ctx, eng, packed, x, times):
        out = getattr(eng, cls.fwd)(x, *cls.operands(packed), times, n_verts=packed.n_verts_dev)
        ctx.eng, ctx.packed = eng, packed
        ctx.save_for_backward(times, *([x] if ctx.needs_input_grad[3] else []))
        return out

    @classmethod
    def backward(cls, ctx, d_out):
        need, p = ctx.needs_input_grad, ctx.packed
        times, x = (list(ctx.saved_tensors) + [None])[:2]
        dx, dt = getattr(ctx.eng, cls.bwd)(d_out, x, *cls.operands(p), times, n_verts=p.n_verts_dev, need_x=need[2], need_times=need[3])
        return None, None, dx, dt


class GradFeatFn(torch.autograd.Function):
    """SpatialGradientFeatures of the diffused features x; saved: x and the matrices as the kernels read them"""
    fwd, bwd, matrix = "dnet_gradient_features", "dnet_gradient_features_backward", staticmethod(_same)

    @classmethod
    def forward(cls, ctx, eng, packed, x, A_re, A_im):
        A_re, A_im = cls.matrix(A_re), cls.matrix(A_im)
        out = getattr(eng, cls.fwd)(x, packed.row_len, packed.cols, packed.gx, packed.gy, A_re, A_im, n_verts=packed.n_verts_dev)
        ctx.eng, ctx.packed, ctx.rot = eng, packed, A_im is not None
        ctx.save_for_backward(x, A_re, *([A_im] if ctx.rot else []))
        return out

    @classmethod
    def backward(cls, ctx, d_out):
        need, p = ctx.needs_input_grad, ctx.packed
        x, A_re, A_im = (list(ctx.saved_tensors) + [None])[:3]
        dx, dA_re, dA_im = getattr(ctx.eng, cls.bwd)(d_out, x, p.row_len, p.cols, p.gx, p.gy, p.transposed_rows() if need[2] else None, A_re, A_im,
                                                     n_verts=p.n_verts_dev, need_x=need[2], need_A=bool(need[3] or need[4]))
        return None, None, dx, dA_re if need[3] else None, dA_im if need[4] else None


class LinearHalfFn(LinearFn):
    """LinearFn with the float32 master W rounded to float16 for this call; saved: the sources, the float16 copy, the output (relu)"""
    fwd, bwd, matrix = "dnet_linear_f16", "dnet_linear_backward_f16", staticmethod(_rounded)


class DiffuseHalfFn(DiffuseFn):
    """DiffuseFn on the pack's half_operands(); saved: the times, and x for the gradient of the times"""
    fwd, bwd = "dnet_diffuse_f16", "dnet_diffuse_backward_f16"

    @staticmethod
    def operands(packed):
        return (*packed.half_operands(), packed.evals)


class GradFeatHalfFn(GradFeatFn):
    """GradFeatFn with the float32 masters A_re / A_im rounded to float16 for this call; saved: x and the float16 copies"""
    fwd, bwd, matrix = "dnet_gradient_features_f16", "dnet_gradient_features_backward_f16", staticmethod(_rounded)


def run(net, eng, xs, packed, half=False):
    """first_lin .. last_lin of the DiffusionNet `net` on the padded batch xs (a list of up to three (B,N,w) tensors read as
    concatenated; the two concatenations of a block are never formed either), recorded for autograd.  The MLP's nn.Dropout modules are
    the block's own, called between the kernels.  half: the mixed-precision set of functions (module docstring)."""
    nv = packed.n_verts_dev
    Linear, Diffuse, GradFeat = (LinearHalfFn, DiffuseHalfFn, GradFeatHalfFn) if half else (LinearFn, DiffuseFn, GradFeatFn)
    lin = lambda srcs, m, relu=False, resid=None: Linear.apply(eng, nv, relu, m.weight, m.bias, resid, *srcs)
    for blk in net.blocks:
        blk.diffusion.clamp_time()
    x = lin(xs, net.first_lin)
    for blk in net.blocks:
        xd = Diffuse.apply(eng, packed, x, blk.diffusion.diffusion_time)
        srcs = [x, xd]
        if blk.with_gradient_features:
            gf = blk.gradient_features
            A_re, A_im = (gf.A_re.weight, gf.A_im.weight) if blk.with_gradient_rotations else (gf.A.weight, None)
            srcs.append(GradFeat.apply(eng, packed, xd, A_re, A_im))
        mods = list(blk.mlp)
        last = max(j for j, m in enumerate(mods) if isinstance(m, nn.Linear))
        fused = False
        for j, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                fused = j + 1 < len(mods) and isinstance(mods[j + 1], nn.ReLU)
                srcs = [lin(srcs, m, relu=fused, resid=x if j == last else None)]      # (MiniMLP puts no activation behind its last layer)
            elif fused and isinstance(m, nn.ReLU):
                fused = False                                      # applied by the kernel of the layer in front of it
            else:
                srcs = [m(srcs[0])]
        x = srcs[0]
    return lin([x], net.last_lin)

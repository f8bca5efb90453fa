"""The DiffusionNet backward kernels on the GPU (dm_dnet_linear_bwd_data_f32, dm_dnet_linear_bwd_weight_f32, dm_dnet_diffuse_bwd_f32,
dm_dnet_gradfeat_bwd_f32) and the differentiable device route of diffusion_net.layers: every kernel against its float64 restatement
within the restatement's running-error bound (tests/dnet_backward_restate.py), batches against single calls bit for bit, hostile
operand placement, the gradients of the whole network against float64 autograd of the dense restatement, training mode, the tails,
and the refusals.  Every figure is printed before it is asserted.

Whole-network figures measured on an MI355X are recorded in DESIGN.md section 4, 'DiffusionNet backward'."""
import copy
import functools

import numpy as np
import pytest
import torch

import dnet_backward_restate as br
import dnet_layers_checks as lc
import dnet_layers_restate as rs
import placement as pl
from densematcher_amd import _lib
from densematcher_amd.diffusion_net import layers
from densematcher_amd.diffusion_net.backward import K_MAX

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def rnd(seed, *shape, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def within(got, ref, bound, tag):
    got = got.detach().cpu().double().numpy()
    err = np.abs(got - ref)
    share = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{tag}: max |got - ref| = {err.max():.3e}, max |ref| = {np.abs(ref).max():.3e}, largest share of the bound {share:.3e}")
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert np.all(err <= bound), (tag, share)


# ---------------------------------------------------------------------------------------------------------------- 1. linear
OPTS = [(False, False, False), (True, True, False), (True, False, True), (True, True, True), (False, True, True)]
LINEAR = [(N, Co, w, OPTS[i % len(OPTS)]) for i, (N, Co, w) in enumerate(
    (N, Co, w) for N in (1, 81, 257) for Co in (1, 48, 130) for w in ((19,), (32, 32, 32)))]
LINEAR += [(81, 48, (768, 51, 16), o) for o in (OPTS[0], OPTS[3])]


def linear_operands(N, Co, widths, opts):
    """the forward test's operands, the saved output of the activation (float32, without resid: the mask both sides use) and dY"""
    bias, relu, _ = opts
    srcs = [rnd(10 + i, N, w) for i, w in enumerate(widths)]
    W = rnd(20, Co, sum(widths), scale=sum(widths) ** -0.5)
    b = rnd(21, Co) if bias else None
    Y = rs.linear(srcs, W, b, None, True).astype(np.float32) if relu else None
    return srcs, W, Y, rnd(23, N, Co)


@pytest.mark.parametrize("N,Co,widths,opts", LINEAR)
def test_linear_backward_against_the_restatement(eng, N, Co, widths, opts):
    srcs, W, Y, dY = linear_operands(N, Co, widths, opts)
    tag = f"linear backward N={N} C_out={Co} widths={widths} {opts}"
    d_src, dW, db = eng.dnet_linear_backward(dev(dY), [dev(s) for s in srcs], dev(W), y=None if Y is None else dev(Y))
    ref, bound = br.linear_backward(dY, srcs, W, Y), br.linear_backward_bound(dY, srcs, W, Y)
    if Y is not None:
        print(f"{tag}: the mask keeps {float((Y > 0).mean()):.3f} of the entries")
    for i in range(len(widths)):
        within(d_src[i], ref[0][i], bound[0][i], f"{tag} d_src{i}")
    within(dW, ref[1], bound[1], f"{tag} dW")
    within(db, ref[2], bound[2], f"{tag} db")


def test_linear_backward_null_outputs(eng):
    """a source without a data gradient (first_lin's input), no weight or no bias gradient: the others keep their bits"""
    srcs, W, Y, dY = linear_operands(81, 48, (32, 32, 32), OPTS[1])
    d = lambda a: dev(a)
    full = eng.dnet_linear_backward(d(dY), [d(s) for s in srcs], d(W), y=d(Y))
    part, dW, db = eng.dnet_linear_backward(d(dY), [d(s) for s in srcs], d(W), y=d(Y), need_src=[False, True, False], need_bias=False)
    assert part[0] is None and part[2] is None and db is None and torch.equal(part[1], full[0][1]) and torch.equal(dW, full[1])
    part, dW, db = eng.dnet_linear_backward(d(dY), [32, 32, 32], d(W), y=d(Y), need_src=[True, False, False], need_weight=False, need_bias=False)
    assert dW is None and db is None and torch.equal(part[0], full[0][0])
    part, dW, db = eng.dnet_linear_backward(d(dY), [d(s) for s in srcs], None, y=d(Y), need_src=False, need_weight=False)
    assert part == [None, None, None] and dW is None and torch.equal(db, full[2])


# ---------------------------------------------------------------------------------------------------------------- 2. diffuse
def diffuse_operands(N, K, Cw, seed=0):
    g = np.random.default_rng(seed)
    x, evecs = rnd(seed + 1, N, Cw), rnd(seed + 2, N, K, scale=0.3)
    mass = (0.002 + 0.01 * g.random(N)).astype(np.float32)
    evals = np.sort(40.0 * g.random(K)).astype(np.float32)
    times = (0.05 * g.random(Cw)).astype(np.float32)
    times[0] = 0.0                                             # at the floor
    if Cw > 1:
        times[1] = -0.01
    return x, mass, evals, evecs, times


DIFFUSE = [((1, 81, 257)[(i + j) % 3], K, Cw) for i, K in enumerate((1, 33, 128, 130, K_MAX)) for j, Cw in enumerate((1, 32, 48))]


@pytest.mark.parametrize("N,K,Cw", DIFFUSE)
def test_diffuse_backward_against_the_restatement(eng, N, K, Cw):
    x, mass, evals, evecs, times = diffuse_operands(N, K, Cw)
    dO = rnd(7, N, Cw)
    dx, dt = eng.dnet_diffuse_backward(dev(dO)[None], dev(x)[None], dev(mass)[None], dev(evals)[None], dev(evecs)[None], dev(times))
    ref, bound = br.diffuse_backward(dO, x, mass, evals, evecs, times), br.diffuse_backward_bound(dO, x, mass, evals, evecs, times)
    within(dx[0], ref[0], bound[0], f"diffuse backward N={N} K={K} C={Cw} dx")
    within(dt, ref[1], bound[1], f"diffuse backward N={N} K={K} C={Cw} dtimes")
    only_x, none = eng.dnet_diffuse_backward(dev(dO)[None], None, dev(mass)[None], dev(evals)[None], dev(evecs)[None], dev(times), need_times=False)
    assert none is None and torch.equal(only_x, dx)
    none, only_t = eng.dnet_diffuse_backward(dev(dO)[None], dev(x)[None], dev(mass)[None], dev(evals)[None], dev(evecs)[None], dev(times), need_x=False)
    assert none is None and torch.equal(only_t, dt)


# ---------------------------------------------------------------------------------------------------------------- 3. gradient features
@functools.lru_cache(maxsize=None)
def packed(*keys):
    return layers.pack_operators([lc.operators(k) for k in keys]).to(DEV)


@pytest.mark.parametrize("key", ["t", "f", "t2"])
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("Cw", [1, 32, 48, 130])
def test_gradfeat_backward_against_the_restatement(eng, key, rot, Cw):
    p = packed(key)
    n = p.n_verts[0]
    tag = f"gradfeat backward mesh {key} C={Cw} rotations={rot}"
    x, dO = rnd(31, n, Cw, scale=0.1), rnd(37, n, Cw)
    A_re, A_im = rnd(32, Cw, Cw, scale=Cw ** -0.5), (rnd(33, Cw, Cw, scale=Cw ** -0.5) if rot else None)
    dx, dRe, dIm = eng.dnet_gradient_features_backward(dev(dO)[None], dev(x)[None], p.row_len, p.cols, p.gx, p.gy, p.transposed_rows(), dev(A_re),
                                                       None if A_im is None else dev(A_im))
    Gx, Gy = p.dense_grad(0, "gx").cpu().numpy(), p.dense_grad(0, "gy").cpu().numpy()
    dots = rs.gradfeat(x, Gx, Gy, A_re, A_im)[1]
    share = float((np.abs(dots) < 2).mean())
    print(f"{tag}: |dots| < 2 at {share:.3f} of the entries, largest {np.abs(dots).max():.3f}")
    assert share >= 0.5                                        # a saturated tanh would hide the gradient path
    ref, bound = br.gradfeat_backward(dO, x, Gx, Gy, A_re, A_im), br.gradfeat_backward_bound(dO, x, Gx, Gy, A_re, A_im)
    within(dx[0], ref[0], bound[0], f"{tag} dx")
    within(dRe, ref[1], bound[1], f"{tag} dA_re")
    if rot:
        within(dIm, ref[2], bound[2], f"{tag} dA_im")
    else:
        assert dIm is None
    only_x = eng.dnet_gradient_features_backward(dev(dO)[None], dev(x)[None], p.row_len, p.cols, p.gx, p.gy, p.transposed_rows(), dev(A_re),
                                                 None if A_im is None else dev(A_im), need_A=False)
    only_A = eng.dnet_gradient_features_backward(dev(dO)[None], dev(x)[None], p.row_len, p.cols, p.gx, p.gy, None, dev(A_re),
                                                 None if A_im is None else dev(A_im), need_x=False)
    assert only_x[1] is None and only_x[2] is None and torch.equal(only_x[0], dx)
    assert only_A[0] is None and torch.equal(only_A[1], dRe) and (dIm is None or torch.equal(only_A[2], dIm))


# ---------------------------------------------------------------------------------------------------------------- 4. batches
def cut_operators(key, n):
    """mesh `key` of the fixture cut to its first n vertices: the operators' leading blocks (any matrices do for these tests)"""
    _, mass, _, evals, evecs, gX, gY = lc.operators(key)
    sub = lambda g: g.to_dense()[:n, :n].to_sparse().coalesce()
    return (None, mass[:n], None, evals, evecs[:n], sub(gX), sub(gY))


def test_ragged_batch_equals_the_single_calls(eng):
    n_verts = (160, 97, 1)
    ops = [cut_operators("t", n) for n in n_verts]
    p, singles = layers.pack_operators(ops).to(DEV), [layers.pack_operators([o]).to(DEV) for o in ops]
    Bn, N, Cw, Co = 3, 160, 32, 48
    assert p.n_verts == list(n_verts) and p.n_verts_dev is not None
    nan = lambda c: torch.full((Bn, N, c), float("nan"), device=DEV)
    x, x2, dO, dY, Y = nan(Cw), nan(19), nan(Cw), nan(Co), nan(Co)
    for b, n in enumerate(n_verts):
        x[b, :n], x2[b, :n], dO[b, :n] = dev(rnd(40 + b, n, Cw, scale=0.1)), dev(rnd(43 + b, n, 19)), dev(rnd(46 + b, n, Cw))
        dY[b, :n], Y[b, :n] = dev(rnd(49 + b, n, Co)), dev(rnd(52 + b, n, Co))
    W, times = dev(rnd(55, Co, Cw + 19, scale=0.1)), dev(diffuse_operands(4, 4, Cw)[4])
    A_re, A_im = dev(rnd(56, Cw, Cw, scale=0.2)), dev(rnd(57, Cw, Cw, scale=0.2))
    nv = p.n_verts_dev

    def run():
        lin = eng.dnet_linear_backward(dY, [x, x2], W, y=Y, n_verts=nv)
        dif = eng.dnet_diffuse_backward(dO, x, p.mass, p.evals, p.evecs, times, n_verts=nv)
        grd = eng.dnet_gradient_features_backward(dO, x, p.row_len, p.cols, p.gx, p.gy, p.transposed_rows(), A_re, A_im, n_verts=nv)
        return [lin[0][0], lin[0][1], dif[0], grd[0]], [lin[1], lin[2], dif[1], grd[1], grd[2]]
    acts, params = run()
    again_a, again_p = run()
    for a, c in zip(acts + params, again_a + again_p):
        assert bool(torch.isfinite(a).all()) and torch.equal(pl.bits(a), pl.bits(c))          # two runs, the same bits
    sums = [None] * len(params)
    for b, (n, one) in enumerate(zip(n_verts, singles)):
        sl = lambda t: t[b:b + 1, :n].contiguous()
        lin = eng.dnet_linear_backward(sl(dY), [sl(x), sl(x2)], W, y=sl(Y))
        dif = eng.dnet_diffuse_backward(sl(dO), sl(x), one.mass, one.evals, one.evecs, times)
        grd = eng.dnet_gradient_features_backward(sl(dO), sl(x), one.row_len, one.cols, one.gx, one.gy, one.transposed_rows(), A_re, A_im)
        for name, got, alone in zip(("d_src0", "d_src1", "diffuse dx", "gradfeat dx"), acts, [lin[0][0], lin[0][1], dif[0], grd[0]]):
            assert torch.equal(pl.bits(got[b, :n]), pl.bits(alone[0])), (name, b)              # its own mesh only
            assert bool((got[b, n:] == 0).all()), (name, b, "padding rows")
        for i, t in enumerate([lin[1], lin[2], dif[1], grd[1], grd[2]]):
            sums[i] = t if b == 0 else sums[i] + t                                              # the meshes in ascending order
    for name, got, want in zip(("dW", "db", "dtimes", "dA_re", "dA_im"), params, sums):
        print(f"{name}: max |batch - ascending sum of the single calls| = {float((got - want).abs().max()):.3e}")
        assert torch.equal(pl.bits(got), pl.bits(want)), name


# ---------------------------------------------------------------------------------------------------------------- 5. placement
def hostile(a, n_real, pad):
    """rows >= n_real[b] of a (B, n, ...) operand replaced by the fill"""
    a = a.copy()
    for b, n in enumerate(n_real):
        a[b, n:] = pl.INT_FILL if a.dtype.kind == "i" else pl.fill_value(torch.float32, pad)
    return a


@pytest.mark.parametrize("pad,off", [("nan", 1), ("+inf", 2), ("-inf", 3)])
def test_placement_of_every_operand(eng, pad, off):
    p = packed("t", "f")
    n_real, n, R = [160, 76], 160, 163                          # mesh 1 is cut to 76 of its 81 rows: rows 76.. are padding too
    Cw, Co, K = 32, 48, 16
    cpu = lambda t: t.cpu().numpy()
    rl, cols, gx, gy = cpu(p.row_len), cpu(p.cols), cpu(p.gx), cpu(p.gy)
    cols[1][cols[1] >= 76] = 0                                  # (a cut mesh keeps no column outside itself)
    cut = layers.PackedOperators(n_real, mass=p.mass, evals=p.evals, evecs=p.evecs, row_len=dev(rl), cols=dev(cols), gx=p.gx, gy=p.gy)
    rlt, colst, gxt, gyt = (cpu(t) for t in cut.transposed_rows())
    mass, evals, evecs = cpu(p.mass), cpu(p.evals), cpu(p.evecs)
    x, x2, dO, dY, Y = rnd(60, 2, n, Cw, scale=0.1), rnd(61, 2, n, 19), rnd(62, 2, n, Cw), rnd(67, 2, n, Co), rnd(68, 2, n, Co)
    W, times = rnd(63, Co, Cw + 19, scale=0.1), diffuse_operands(4, 4, Cw)[4]
    A_re, A_im = rnd(65, Cw, Cw, scale=0.2), rnd(66, Cw, Cw, scale=0.2)
    nv = dev(np.asarray(n_real, np.int32))

    def pad_rows(a, fill=0):
        out = np.full((a.shape[0], R) + a.shape[2:], fill, a.dtype)
        out[:, :n] = a
        return out
    # ---- control: aligned, dense, benign padding
    ctl = dict(x=pad_rows(x), x2=pad_rows(x2), dO=pad_rows(dO), dY=pad_rows(dY), Y=pad_rows(Y), mass=pad_rows(mass, 1), evecs=pad_rows(evecs),
               rl=pad_rows(rl, 1), cols=pad_rows(cols), gx=pad_rows(gx), gy=pad_rows(gy), rlt=pad_rows(rlt, 1), colst=pad_rows(colst),
               gxt=pad_rows(gxt), gyt=pad_rows(gyt))
    d = {k: dev(v) for k, v in ctl.items()}
    lin = eng.dnet_linear_backward(d["dY"], [d["x"], d["x2"]], dev(W), y=d["Y"], n_verts=nv)
    dif = eng.dnet_diffuse_backward(d["dO"], d["x"], d["mass"], dev(evals), d["evecs"], dev(times), n_verts=nv)
    grd = eng.dnet_gradient_features_backward(d["dO"], d["x"], d["rl"], d["cols"], d["gx"], d["gy"], (d["rlt"], d["colst"], d["gxt"], d["gyt"]),
                                              dev(A_re), dev(A_im), n_verts=nv)
    want_act, want_par = [lin[0][0], lin[0][1], dif[0], grd[0]], [lin[1], lin[2], dif[1], grd[1], grd[2]]
    # ---- hostile: every operand off the 16-byte grid, ld > width, the fill in padding columns, rows >= n_verts, slots >= row_len
    def slots(c, vx, vy, lens):
        c, vx, vy = c.copy(), vx.copy(), vy.copy()
        dead = np.arange(c.shape[2])[None, None, :] >= lens[:, :, None]
        c[dead], vx[dead], vy[dead] = pl.INT_FILL, pl.fill_value(torch.float32, pad), pl.fill_value(torch.float32, pad)
        return c, vx, vy
    hc, hx, hy = slots(cols, gx, gy, rl)
    hct, hxt, hyt = slots(colst, gxt, gyt, rlt)

    def mat(a, width_pad=5):
        """(B, n, W) -> the view (B, R, W) of a placed (B, R, W + 5) buffer"""
        v = pl.place(hostile(a, n_real, pad), offset_elems=off, ld=a.shape[-1] + width_pad, rows=R, pad=None if a.dtype.kind == "i" else pad, device=DEV)
        return v[..., :a.shape[-1]]

    def vec(a):
        """(B, n) -> (B, R) with the fill behind n_verts"""
        return pl.place(hostile(a, n_real, pad), offset_elems=off, ld=R, pad=None if a.dtype.kind == "i" else pad, device=DEV)

    def flat(a, ld=None):
        return pl.place(a, offset_elems=off, ld=ld, pad=pad, device=DEV)[..., :a.shape[-1]]
    hx_, hx2_, hdO, hdY, hY = mat(x), mat(x2), mat(dO), mat(dY), mat(Y)
    hm, he, hrl, hrlt = vec(mass), mat(evecs), vec(rl), vec(rlt)
    hcols, hgx, hgy, hcolst, hgxt, hgyt = mat(hc, 0), mat(hx, 0), mat(hy, 0), mat(hct, 0), mat(hxt, 0), mat(hyt, 0)
    outs = [pl.place(np.zeros((2, R, c), np.float32), offset_elems=off, ld=c + 3, pad=pad, device=DEV) for c in (Cw, 19, Cw, Cw)]
    assert all(pl.mod16(t) != 0 for t in (hx_, hx2_, hdO, hdY, hY, hm, he, hrl, hcols, hgx, hgy, hcolst, hgxt, hgyt, outs[0]))
    hW, hA, hAi = flat(W, W.shape[1] + 7), flat(A_re, Cw + 1), flat(A_im, Cw + 1)
    hnv = pl.place(np.asarray(n_real, np.int32), offset_elems=off, device=DEV)
    with pl.PointerRecorder(eng.lib, "dm_dnet_linear_bwd_data_f32") as rec, pl.PointerRecorder(eng.lib, "dm_dnet_linear_bwd_weight_f32") as rec2:
        lin = eng.dnet_linear_backward(hdY, [hx_, hx2_], hW, y=hY, n_verts=hnv, out=[outs[0][..., :Cw], outs[1][..., :19]])
    assert rec.saw(hdY, hY, hW, hnv, outs[0], outs[1]) and rec2.saw(hdY, hY, hx_, hx2_, hnv)
    with pl.PointerRecorder(eng.lib, "dm_dnet_diffuse_bwd_f32") as rec:
        dif = eng.dnet_diffuse_backward(hdO, hx_, hm, flat(evals), he, flat(times), n_verts=hnv, out=outs[2][..., :Cw])
    assert rec.saw(hdO, hx_, hm, he, hnv, outs[2])
    with pl.PointerRecorder(eng.lib, "dm_dnet_gradfeat_bwd_f32") as rec:
        grd = eng.dnet_gradient_features_backward(hdO, hx_, hrl, hcols, hgx, hgy, (hrlt, hcolst, hgxt, hgyt), hA, hAi, n_verts=hnv, out=outs[3][..., :Cw])
    assert rec.saw(hdO, hx_, hrl, hcols, hgx, hgy, hrlt, hcolst, hgxt, hgyt, hA, hAi, hnv, outs[3])
    fill_bits = pl.bits(torch.full((1,), pl.fill_value(torch.float32, pad), device=DEV))
    for name, w, o, c in zip(("d_src0", "d_src1", "diffuse dx", "gradfeat dx"), want_act, outs, (Cw, 19, Cw, Cw)):
        assert torch.equal(pl.bits(o[..., :c]), pl.bits(w)), (name, pad, off)
        assert bool((pl.bits(o[..., c:]) == fill_bits).all()), (name, "a padding column of the output was written")
        assert bool(torch.isfinite(w).all()) and bool((w[0, n_real[0]:] == 0).all()) and bool((w[1, n_real[1]:] == 0).all())
    for name, w, g in zip(("dW", "db", "dtimes", "dA_re", "dA_im"), want_par, [lin[1], lin[2], dif[1], grd[1], grd[2]]):
        assert bool(torch.isfinite(w).all()) and torch.equal(pl.bits(g), pl.bits(w)), (name, pad, off)


# ---------------------------------------------------------------------------------------------------------------- 6. whole network
MARGIN = 2.0 ** -17         # every ReLU preactivation of the oracle is at least this far (relative to its layer's largest) from the kink:
                            # about ten times the forward bound 4 f32_floor + 2^-23, so no mask of the fp32 run differs from the oracle's


def collect(net, x):
    out = {name: p.grad for name, p in net.named_parameters() if p.grad is not None}
    if x is not None and x.grad is not None:
        out["x"] = x.grad
    return out


def oracle(net, xs, ops_packed, gs, dtype, masks=None, faces=None):
    """gradients of sum_b (y_b * g_b).sum() through the dense restatement in `dtype`: (name -> gradient ('x': a list), ReLU margin)"""
    params = br.leaf_parameters(net, dtype)
    leaves = [x.detach().to(dtype).requires_grad_() for x in xs]
    ys, pre = br.dense_network(net, params, leaves, br.dense_operators(ops_packed, dtype), masks=masks, faces=faces)
    sum((y * g.to(dtype)).sum() for y, g in zip(ys, gs)).backward()
    grads = {name: p.grad for name, p in params.items() if p.grad is not None}
    grads["x"] = leaves
    return grads, br.relu_margin(pre) if pre else 1.0, ys


def compare(tag, got, ref64, ref32):
    """per tensor max |got - ref| / max |ref| against the float64 oracle; the yardstick: the same figure of the dense restatement in
    fp32 on the GPU, its largest over the network's tensors; the bound 4 x yardstick + 2^-23 (check_output's margin for another
    evaluation order).  Returns (figures, bound)"""
    figs, yard = br.figures(got, ref64), br.figures(ref32, ref64)
    bound = 4.0 * max(yard.values()) + 2.0 ** -23
    for name in sorted(figs):
        print(f"{tag} {name}: device {figs[name]:.3e}, dense fp32 {yard[name]:.3e}")
    print(f"{tag}: largest device figure {max(figs.values()):.3e}, yardstick {max(yard.values()):.3e}, bound {bound:.3e}")
    assert set(figs) == set(yard)
    assert all(f <= bound for f in figs.values()), (tag, {k: v for k, v in figs.items() if v > bound}, bound)
    return figs, bound


def flat_grads(grads, n_verts=None):
    """the oracle's per-mesh input gradients as one padded (B, N, C) tensor (or (N, C) for one mesh given flat)"""
    out = dict(grads)
    xs = out.pop("x")
    N = max(x.shape[0] for x in xs)
    out["x"] = torch.stack([torch.nn.functional.pad(x.grad, (0, 0, 0, N - x.shape[0])) for x in xs])
    return out


def drawn_input(case, run):
    """x = std(fixture x) N(0, 1) from default_rng(100 + seed), the first seed below 32 whose oracle preactivations keep MARGIN;
    run(x) -> (.., margin, ..) is the float64 oracle.  Returns (seed, x, what run returned)"""
    fx = lc.golden()[f"{case}_x"]
    for seed in range(32):
        x = (float(fx.std()) * np.random.default_rng(100 + seed).standard_normal(fx.shape)).astype(np.float32)
        res = run(dev(x))
        print(f"case {case} seed {seed}: smallest |z| / max |z| over the ReLU preactivations {res[1]:.3e} (needs {MARGIN:.3e})")
        if res[1] >= MARGIN:
            return seed, dev(x), res
    raise AssertionError(f"case {case}: no seed below 32 keeps the ReLU preactivations {MARGIN:.3e} from zero")


def case_setup(case):
    net = lc.network(case, DEV)
    _, kw = lc.call_arguments(case, DEV)
    p = packed(*lc.config(case)["meshes"])
    shape = lc.golden()[f"{case}_x"].shape
    batched = len(shape) == 3
    Bn = shape[0] if batched else 1
    g = dev(rnd(90, *net(torch.zeros(shape, device=DEV), route="torch", **kw).shape))
    split = (lambda t: [t[b] for b in range(Bn)]) if batched else (lambda t: [t])
    return net, kw, p, g, split, batched


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_whole_network_gradients_against_the_float64_oracle(case):
    with torch.no_grad():
        net, kw, p, g, split, batched = case_setup(case)
    faces = [kw["faces"]] if "faces" in kw else None
    seed, x, (ref64, margin, _) = drawn_input(case, lambda x: oracle(net, split(x), p, split(g), torch.float64, faces=faces))
    assert margin >= MARGIN
    ref32, _, _ = oracle(net, split(x), p, split(g), torch.float32, faces=faces)
    xi = x.clone().requires_grad_()
    net.zero_grad()
    y = net(xi, route="device", differentiable=True, **kw)
    assert net.last_route == "device" and y.dtype == torch.float32 and y.requires_grad
    (y * g).sum().backward()
    unbatch = (lambda d: d) if batched else (lambda d: {k: (v[0] if k == "x" else v) for k, v in d.items()})
    compare(f"case {case} seed {seed}", collect(net, xi), unbatch(flat_grads(ref64)), unbatch(flat_grads(ref32)))
    with torch.no_grad():                                       # the forward value is the inference route's, bit for bit
        assert torch.equal(y.detach(), net(x, route="device", **kw))
    with pytest.raises(RuntimeError, match="requires grad"):   # without the switch the device route still refuses
        net(xi, route="device", **kw)
    assert net(xi, route="auto", differentiable=True, **kw).requires_grad and net.last_route == "torch"


# ---------------------------------------------------------------------------------------------------------------- 7. training mode
def test_training_mode_with_dropout():
    """dropout=True after .train(): each nn.Dropout's keep mask is recorded by a forward hook during the device run (an entry whose
    input is zero does not matter) and handed to the oracle"""
    with torch.no_grad():
        net, kw, p, g, split, _ = case_setup("a")
    net = copy.deepcopy(net).train()
    assert net.dropout and net.training
    drops = [m for m in net.modules() if isinstance(m, torch.nn.Dropout)]
    assert len(drops) == 4
    masks = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: masks.append((out != 0)[None] if out.dim() == 2 else out != 0)) for m in drops]
    state = {}

    def run(x):
        masks.clear()
        torch.manual_seed(1234)
        xi = x.clone().requires_grad_()
        net.zero_grad()
        y = net(xi, route="device", differentiable=True, **kw)
        (y * g).sum().backward()
        state["got"], state["masks"] = collect(net, xi), [m.clone() for m in masks]
        assert len(masks) == 4 and 0.1 < float(masks[0].float().mean()) < 0.7          # (half of the ReLU's outputs are zero to begin with)
        return oracle(net, [x], p, [g], torch.float64, masks=state["masks"])
    try:
        seed, x, (ref64, margin, _) = drawn_input("a", run)
    finally:
        for h in hooks:
            h.remove()
    ref32, _, _ = oracle(net, [x], p, [g], torch.float32, masks=state["masks"])
    one = lambda d: {k: (v[0] if k == "x" else v) for k, v in d.items()}
    compare(f"training mode seed {seed}", state["got"], one(flat_grads(ref64)), one(flat_grads(ref32)))


# ---------------------------------------------------------------------------------------------------------------- 8. tails
def test_faces_tail_and_log_softmax():
    with torch.no_grad():
        net, kw, p, g, split, _ = case_setup("d")
    faces = [kw["faces"]]
    seed, x, (ref64, margin, _) = drawn_input("d", lambda x: oracle(net, [x], p, [g], torch.float64, faces=faces))
    ref32, _, _ = oracle(net, [x], p, [g], torch.float32, faces=faces)
    xi = x.clone().requires_grad_()
    net.zero_grad()
    y = net(xi, route="device", differentiable=True, **kw)
    assert tuple(y.shape) == (faces[0].shape[0], 6)
    (y * g).sum().backward()
    one = lambda d: {k: (v[0] if k == "x" else v) for k, v in d.items()}
    compare(f"case d (faces, log_softmax) seed {seed}", collect(net, xi), one(flat_grads(ref64)), one(flat_grads(ref32)))


def test_forward_many_on_a_ragged_list():
    keys = ("t", "r", "f")
    p = packed(*keys)
    net = lc.network("a", DEV)
    gs = [dev(rnd(91 + b, n, 24)) for b, n in enumerate(p.n_verts)]
    std = float(lc.golden()["a_x"].std())
    for seed in range(32):
        xs = [dev(std * rnd(100 + seed + 1000 * b, n, 19)) for b, n in enumerate(p.n_verts)]
        ref64, margin, _ = oracle(net, xs, p, gs, torch.float64)
        print(f"forward_many seed {seed}: ReLU margin {margin:.3e}")
        if margin >= MARGIN:
            break
    assert margin >= MARGIN
    ref32, _, _ = oracle(net, xs, p, gs, torch.float32)
    leaves = [x.clone().requires_grad_() for x in xs]
    net.zero_grad()
    ys = net.forward_many(leaves, p, differentiable=True)
    assert net.last_route == "device" and [tuple(y.shape) for y in ys] == [(n, 24) for n in p.n_verts]
    sum((y * g).sum() for y, g in zip(ys, gs)).backward()
    got = collect(net, None)
    got["x"] = torch.stack([torch.nn.functional.pad(x.grad, (0, 0, 0, 160 - x.shape[0])) for x in leaves])
    compare(f"forward_many seed {seed}", got, flat_grads(ref64), flat_grads(ref32))
    with torch.no_grad():
        for y, alone in zip(ys, net.forward_many(xs, p)):
            assert torch.equal(y.detach(), alone)
    with pytest.raises(RuntimeError, match="requires grad"):
        net.forward_many(leaves, p)


def test_frozen_parameters_and_one_sgd_step(eng, monkeypatch):
    with torch.no_grad():
        net, kw, p, g, split, _ = case_setup("a")
    net = copy.deepcopy(net)
    frozen = ["first_lin.weight", "block_0.diffusion.diffusion_time", "block_0.gradient_features.A_re.weight", "block_0.gradient_features.A_im.weight",
              "block_1.mlp.miniMLP_mlp_layer_000.weight", "block_1.mlp.miniMLP_mlp_layer_000.bias"]
    named = dict(net.named_parameters())
    for name in frozen:
        named[name].requires_grad_(False)
    seed, x, (ref64, margin, _) = drawn_input("a", lambda x: oracle(net, [x], p, [g], torch.float64))
    ref32, _, _ = oracle(net, [x], p, [g], torch.float32)
    calls = {"linear": [], "diffuse": [], "gradfeat": []}
    for key, name in (("linear", "dnet_linear_backward"), ("diffuse", "dnet_diffuse_backward"), ("gradfeat", "dnet_gradient_features_backward")):
        def spy(*a, _orig=getattr(eng, name), _key=key, **k):
            calls[_key].append(k)
            return _orig(*a, **k)
        monkeypatch.setattr(eng, name, spy)
    net.zero_grad()
    before = {name: q.detach().clone() for name, q in named.items()}
    y = net(x, route="device", differentiable=True, **kw)           # x needs no gradient either
    (y * g).sum().backward()
    assert all(named[name].grad is None for name in frozen)
    # backward order: last_lin first, first_lin last.  first_lin: no source gradient, no weight gradient, the bias gradient
    first = calls["linear"][-1]
    assert first["need_src"] == [False] and not first["need_weight"] and first["need_bias"]
    assert any(k["need_weight"] is False and k["need_bias"] is False and all(k["need_src"]) for k in calls["linear"][:-1])       # block_1's frozen layer
    assert [k["need_times"] for k in calls["diffuse"]] == [True, False] and all(k["need_x"] for k in calls["diffuse"])
    assert [k["need_A"] for k in calls["gradfeat"]] == [True, False]
    ref64 = {k: v for k, v in flat_grads(ref64).items() if k != "x"}
    ref32 = {k: v for k, v in flat_grads(ref32).items() if k != "x"}
    assert not any(name in ref64 for name in frozen)
    figs, bound = compare(f"frozen parameters seed {seed}", collect(net, None), ref64, ref32)
    lr = 0.05
    torch.optim.SGD([q for q in net.parameters() if q.requires_grad], lr=lr).step()
    for name, q in named.items():
        if name in frozen:
            assert torch.equal(q.detach(), before[name]), name
            continue
        want = before[name].double() - lr * ref64[name]
        err = float((q.detach().double() - want).abs().max())
        # fl(w - lr g): lr |g - g_ref| <= lr bound max |g_ref|, and the roundings of the product and of the update
        allow = lr * bound * float(ref64[name].abs().max()) + 2.0 ** -23 * float(want.abs().max())
        print(f"SGD step {name}: max |w - oracle step| = {err:.3e} (allowed {allow:.3e}), moved by {float((q.detach() - before[name]).abs().max()):.3e}")
        assert err <= allow and not torch.equal(q.detach(), before[name]), name


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(eng):
    net = lc.network("a", DEV)
    x, kw = lc.call_arguments("a", DEV)
    xi = x.clone().requires_grad_()
    with pytest.raises(RuntimeError, match="requires grad"):
        net(xi, route="device", differentiable=False, **kw)
    with pytest.raises(RuntimeError, match="on the GPU"):
        net(x.cpu(), route="device", differentiable=True, **{k: v.cpu() for k, v in kw.items()})
    half = copy.deepcopy(net).half()
    for xin in (x, x.half()):
        with pytest.raises(RuntimeError, match="float32 .the fp16 kernels have no backward"):
            half(xin, route="device", differentiable=True, **kw)
    with pytest.raises(RuntimeError, match="float32"):
        net(x.double(), route="device", differentiable=True, **kw)
    n, K = 8, K_MAX + 1
    wide = layers.pack_operators([(None, torch.ones(n), None, torch.zeros(K), torch.zeros((n, K)), None, None)]).to(DEV)
    with pytest.raises(RuntimeError, match="k_eig must be at most 1024"):
        net(torch.zeros((n, 19), device=DEV), route="device", differentiable=True, operators=wide)
    z = lambda *s: torch.zeros(s, device=DEV)
    with pytest.raises(ValueError):
        eng.dnet_diffuse_backward(z(1, n, 4), z(1, n, 4), wide.mass, wide.evals, wide.evecs, z(4))
    P, null = (lambda t: __import__("ctypes").c_void_p(t.data_ptr())), __import__("ctypes").c_void_p(0)
    dY, dX, W, ws = z(1, n, 4), z(1, n, 4), z(4, 4), torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def data(B=1, N=n, Co=4, w=4, ld=4, lddy=4, ldw=4, act=0, Y=null, nsrc=1):
        return eng.lib.dm_dnet_linear_bwd_data_f32(eng.ctx, B, N, Co, nsrc, P(dY), lddy, Y, 4, act, P(W), ldw, null, P(dX), w, ld, null, 0, 0, null, 0, 0)

    def weight(B=1, N=n, Co=4, w=4, ld=4, lddy=4, lddw=4, act=0, Y=null, nsrc=1, wsp=P(ws)):
        return eng.lib.dm_dnet_linear_bwd_weight_f32(eng.ctx, B, N, Co, nsrc, P(dY), lddy, Y, 4, act, P(dX), w, ld, null, 0, 0, null, 0, 0, null, wsp,
                                                     P(W), lddw, null)
    bad = [("data", data, k) for k in (dict(B=0), dict(N=0), dict(Co=0), dict(w=0), dict(ld=3), dict(lddy=3), dict(ldw=3), dict(act=1), dict(act=2),
                                        dict(nsrc=0), dict(nsrc=4))]
    bad += [("weight", weight, k) for k in (dict(B=0), dict(N=-1), dict(Co=0), dict(w=0), dict(ld=3), dict(lddy=3), dict(lddw=3), dict(act=1),
                                            dict(nsrc=4), dict(wsp=null))]
    for name, fn, k in bad:
        rc = fn(**k)
        assert rc == _lib.DM_EINVAL, (name, k, rc)
        with pytest.raises(ValueError):
            eng._chk(rc)
    for counts in ([0], [n + 1]):
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_linear_backward(dY, [dY], W, n_verts=counts)
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_diffuse_backward(dY, dY, z(1, n), z(1, 3), z(1, n, 3), z(4), n_verts=counts)
    assert data() == 0 and weight() == 0
    y = net(xi, route="device", differentiable=True, **kw)          # the engine and the route are usable afterwards
    y.sum().backward()
    assert bool(torch.isfinite(xi.grad).all()) and float(xi.grad.abs().max()) > 0

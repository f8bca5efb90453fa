"""The mixed-precision DiffusionNet backward on the GPU (dm_dnet_linear_bwd_data_f16, dm_dnet_linear_bwd_weight_f16,
dm_dnet_diffuse_bwd_f16, dm_dnet_gradfeat_bwd_f16) and the route compute_dtype=torch.float16 of diffusion_net.layers: every entry
against its restatement within the restatement's bound (tests/dnet_mixed_restate.py), batches against single calls bit for bit, tile
position, hostile operand placement, the forward value against the engine call, the gradients of the whole network against the
masked oracle with the torch route under torch.autocast as the yardstick, training mode, GradScaler and the refusals.  Every figure is
printed before it is asserted.

Whole-network figures measured on an MI355X are recorded in DESIGN.md section 4, 'DiffusionNet backward, fp16'."""
import copy
import ctypes
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import dnet_backward_restate as br
import dnet_layers_checks as lc
import dnet_mixed_checks as mc
import dnet_mixed_restate as mr
import placement as pl
from densematcher_amd import _lib
from densematcher_amd.diffusion_net import layers
from densematcher_amd.diffusion_net.backward import K_MAX

pytestmark = pytest.mark.gpu
DEV = "cuda"
rnd = mc.rnd


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


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
KINDS = {"fp32": (np.float32,) * 3, "fp16": (np.float16,) * 3, "mixed": (np.float32, np.float16, np.float32)}
WIDTHS = ((19,), (33, 7, 5), (64, 64, 64))           # (33, 7, 5): a chunk of 16 of the contraction straddles two sources


def linear_operands(N, Co, widths, kind):
    srcs = [rnd(10 + i, N, w).astype(KINDS[kind][i]) for i, w in enumerate(widths)]
    W = rnd(20, Co, sum(widths), scale=sum(widths) ** -0.5).astype(np.float16)
    return srcs, W, rnd(22, N, Co), rnd(23, N, Co)             # Y: any fp32 array is a saved output (its sign is the mask)


@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("Co", [8, 33, 70])
@pytest.mark.parametrize("N", [1, 33, 97, 160])
def test_linear_backward_against_the_restatement(eng, N, Co, widths):
    for act, kind in itertools.product((0, 1), KINDS):
        srcs, W, Y, dY = linear_operands(N, Co, widths, kind)
        Y = Y if act else None
        tag = f"linear backward N={N} C_out={Co} widths={widths} act={act} sources {kind}"
        d_src, dW, db = eng.dnet_linear_backward_f16(dev(dY), [dev(s) for s in srcs], dev(W), y=None if Y is None else dev(Y))
        ref, bound = mr.linear_backward(dY, srcs, W, Y), mr.linear_backward_bound(dY, srcs, W, Y)
        for i in range(len(widths)):
            assert d_src[i].dtype == torch.float32
            within(d_src[i], ref[0][i], bound[0][i], f"{tag} d_src{i}")
        assert dW.dtype == torch.float32 and db.dtype == torch.float32
        within(dW, ref[1], bound[1], f"{tag} dW")
        within(db, ref[2], bound[2], f"{tag} db")


def test_linear_backward_every_combination_of_null_outputs(eng):
    srcs, W, Y, dY = linear_operands(97, 33, (33, 7, 5), "mixed")
    d = [dev(s) for s in srcs]
    full = eng.dnet_linear_backward_f16(dev(dY), d, dev(W), y=dev(Y))
    for need in itertools.product((False, True), repeat=5):
        ns, nw, nb = list(need[:3]), need[3], need[4]
        part, dW, db = eng.dnet_linear_backward_f16(dev(dY), d if (nw or nb) else [33, 7, 5], dev(W) if any(ns) else None, y=dev(Y), need_src=ns,
                                                    need_weight=nw, need_bias=nb)
        for i in range(3):
            assert (part[i] is None) == (not ns[i]) and (part[i] is None or torch.equal(pl.bits(part[i]), pl.bits(full[0][i]))), (need, i)
        assert (dW is None) == (not nw) and (dW is None or torch.equal(pl.bits(dW), pl.bits(full[1]))), need
        assert (db is None) == (not nb) and (db is None or torch.equal(pl.bits(db), pl.bits(full[2]))), need


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


def pack_basis(mass, evals, evecs):
    """a PackedOperators of one mesh that has only the diffusion's operators"""
    return layers.pack_operators([(None, torch.from_numpy(mass), None, torch.from_numpy(evals), torch.from_numpy(evecs), None, None)]).to(DEV)


@pytest.mark.parametrize("N,K,Cw", [(1, 1, 3), (97, 40, 33), (160, 130, 70)])            # K > 128 crosses the spectrum sweep of the kernel of dx
def test_diffuse_backward_against_the_restatement(eng, N, K, Cw):
    x, mass, evals, evecs, times = diffuse_operands(N, K, Cw)
    dO = rnd(7, N, Cw)
    p = pack_basis(mass, evals, evecs)
    eh, mh, e1, e2 = p.half_operands()
    rh = mr.half_operands(mass, evecs)
    assert np.array_equal(eh[0].cpu().double().numpy(), rh[0]) and np.array_equal(mh[0].cpu().double().numpy(), rh[1]) and (int(e1), int(e2)) == rh[2:]
    call = lambda **kw: eng.dnet_diffuse_backward_f16(dev(dO)[None], dev(x)[None] if kw.get("need_times", True) else None, eh, mh, e1, e2, p.evals,
                                                      dev(times), **kw)
    dx, dt = call()
    ref, bound = mr.diffuse_backward(dO, x, mass, evals, evecs, times), mr.diffuse_backward_bound(dO, x, mass, evals, evecs, times)
    within(dx[0], ref[0], bound[0], f"diffuse backward N={N} K={K} C={Cw} dx")
    within(dt, ref[1], bound[1], f"diffuse backward N={N} K={K} C={Cw} dtimes")
    only_x, none = call(need_times=False)
    assert none is None and torch.equal(pl.bits(only_x), pl.bits(dx))
    none, only_t = call(need_x=False)
    assert none is None and torch.equal(pl.bits(only_t), pl.bits(dt))
    # dx is the forward entry with the two matrix operands and their exponents exchanged, bit for bit
    assert torch.equal(pl.bits(dx), pl.bits(eng.dnet_diffuse_f16(dev(dO)[None], mh, eh, e2, e1, p.evals, dev(times))))


# ---------------------------------------------------------------------------------------------------------------- 3. gradient features
@functools.lru_cache(maxsize=None)
def packed(*keys):
    return layers.pack_operators([lc.operators(k) for k in keys]).to(DEV)


@pytest.mark.parametrize("key", ["t", "f", "t2"])
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("Cw", [8, 33, 70])
def test_gradfeat_backward_against_the_restatement(eng, key, rot, Cw):
    p = packed(key)
    n = p.n_verts[0]
    tag = f"gradfeat backward mesh {key} C={Cw} rotations={rot}"
    x, dO = rnd(31, n, Cw, scale=0.1), rnd(37, n, Cw)
    A_re = rnd(32, Cw, Cw, scale=Cw ** -0.5).astype(np.float16)
    A_im = rnd(33, Cw, Cw, scale=Cw ** -0.5).astype(np.float16) if rot else None
    call = lambda rows_t, **kw: eng.dnet_gradient_features_backward_f16(dev(dO)[None], dev(x)[None], p.row_len, p.cols, p.gx, p.gy, rows_t, dev(A_re),
                                                                        None if A_im is None else dev(A_im), **kw)
    dx, dRe, dIm = call(p.transposed_rows())
    Gx, Gy = p.dense_grad(0, "gx").cpu().numpy(), p.dense_grad(0, "gy").cpu().numpy()
    ref, bound = mr.gradfeat_backward(dO, x, Gx, Gy, A_re, A_im), mr.gradfeat_backward_bound(dO, x, Gx, Gy, A_re, A_im)
    within(dx[0], ref[0], bound[0], f"{tag} dx")
    within(dRe, ref[1], bound[1], f"{tag} dA_re")
    if rot:
        within(dIm, ref[2], bound[2], f"{tag} dA_im")
    else:
        assert dIm is None
    only_x, only_A = call(p.transposed_rows(), need_A=False), call(None, need_x=False)
    assert only_x[1] is None and only_x[2] is None and torch.equal(pl.bits(only_x[0]), pl.bits(dx))
    assert only_A[0] is None and torch.equal(pl.bits(only_A[1]), pl.bits(dRe)) and (dIm is None or torch.equal(pl.bits(only_A[2]), pl.bits(dIm)))


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
    Bn, N, Cw, Co = 3, 160, 33, 70
    assert p.n_verts == list(n_verts) and p.n_verts_dev is not None
    nan = lambda c: torch.full((Bn, N, c), float("nan"), device=DEV)
    x, dO, dY, Y = nan(Cw), nan(Cw), nan(Co), nan(Co)
    x2 = torch.full((Bn, N, 19), float("nan"), device=DEV, dtype=torch.float16)                # an fp16 source
    for b, n in enumerate(n_verts):
        x[b, :n], x2[b, :n], dO[b, :n] = dev(rnd(40 + b, n, Cw, scale=0.1)), dev(rnd(43 + b, n, 19)).half(), dev(rnd(46 + b, n, Cw))
        dY[b, :n], Y[b, :n] = dev(rnd(49 + b, n, Co)), dev(rnd(52 + b, n, Co))
    W, times = dev(rnd(55, Co, Cw + 19, scale=0.1)).half(), dev(diffuse_operands(4, 4, Cw)[4])
    A_re, A_im = dev(rnd(56, Cw, Cw, scale=0.2)).half(), dev(rnd(57, Cw, Cw, scale=0.2)).half()
    nv = p.n_verts_dev

    def run(q, sl, nv):
        lin = eng.dnet_linear_backward_f16(sl(dY), [sl(x), sl(x2)], W, y=sl(Y), n_verts=nv)
        dif = eng.dnet_diffuse_backward_f16(sl(dO), sl(x), *q.half_operands(), q.evals, times, n_verts=nv)
        grd = eng.dnet_gradient_features_backward_f16(sl(dO), sl(x), q.row_len, q.cols, q.gx, q.gy, q.transposed_rows(), A_re, A_im, n_verts=nv)
        return [lin[0][0], lin[0][1], dif[0], grd[0]], [lin[1], lin[2], dif[1], grd[1], grd[2]]
    acts, params = run(p, lambda t: t, nv)
    again_a, again_p = run(p, lambda t: t, nv)
    for a, c in zip(acts + params, again_a + again_p):
        assert bool(torch.isfinite(a).all()) and torch.equal(pl.bits(a), pl.bits(c))          # two runs, the same bits
    sums = [None] * len(params)
    for b, (n, one) in enumerate(zip(n_verts, singles)):
        alone_a, alone_p = run(one, lambda t: t[b:b + 1, :n].contiguous(), None)
        for name, got, alone in zip(("d_src0", "d_src1", "diffuse dx", "gradfeat dx"), acts, alone_a):
            assert torch.equal(pl.bits(got[b, :n]), pl.bits(alone[0])), (name, b)              # its own mesh only
            assert bool((got[b, n:] == 0).all()), (name, b, "padding rows")
        for i, t in enumerate(alone_p):
            sums[i] = t if b == 0 else sums[i] + t                                              # the meshes in ascending order, fp32
    for name, got, want in zip(("dW", "db", "dtimes", "dA_re", "dA_im"), params, sums):
        print(f"{name}: max |batch - ascending sum of the single calls| = {float((got - want).abs().max()):.3e}")
        assert torch.equal(pl.bits(got), pl.bits(want)), name


# ---------------------------------------------------------------------------------------------------------------- 5. tiles
def test_the_bits_do_not_depend_on_the_tile(eng):
    """The forward's test compared the 128 x 128 launch of a batch of 52 padded meshes with the 64 x 64 launch of its parts.  No entry of
    this family switches decomposition: every product runs in 64 x 64 tiles at every size (the rule implemented: none), and dx of the
    diffusion is dm_dnet_diffuse_f16, which has one shape too -- there is no count at which a launch changes.  What can differ is the
    tile an element falls in: rows 70.. of a mesh given as a mesh of their own start in the first row tile instead of the second, and
    one source of 192 columns cuts the column tiles where three of 64 do; a batch of 52 meshes puts the same tiles at other grid
    positions.  The bits must agree."""
    N, Co = 160, 70
    srcs, W, Y, dY = linear_operands(N, Co, (64, 64, 64), "fp32")
    three = eng.dnet_linear_backward_f16(dev(dY), [dev(s) for s in srcs], dev(W), y=dev(Y))
    one = eng.dnet_linear_backward_f16(dev(dY), [dev(np.concatenate(srcs, axis=-1))], dev(W), y=dev(Y))
    assert torch.equal(pl.bits(torch.cat(three[0], dim=-1)), pl.bits(one[0][0])) and torch.equal(pl.bits(three[1]), pl.bits(one[1]))
    tail = eng.dnet_linear_backward_f16(dev(dY[70:]), [192], dev(W), y=dev(Y[70:]), need_weight=False, need_bias=False)
    assert torch.equal(pl.bits(tail[0][0]), pl.bits(one[0][0][70:]))
    Bn = 52
    rep = lambda a: dev(a)[None].repeat(Bn, 1, 1)
    many = eng.dnet_linear_backward_f16(rep(dY), [rep(s) for s in srcs], dev(W), y=rep(Y), need_weight=False, need_bias=False)
    for i in range(3):
        assert torch.equal(pl.bits(many[0][i]), pl.bits(three[0][i][None].repeat(Bn, 1, 1)))
    p = packed("t")
    n, Cw = p.n_verts[0], 70
    x, dO = rnd(31, n, Cw, scale=0.1), rnd(37, n, Cw)
    A_re, A_im = dev(rnd(32, Cw, Cw, scale=Cw ** -0.5)).half(), dev(rnd(33, Cw, Cw, scale=Cw ** -0.5)).half()
    alone = eng.dnet_gradient_features_backward_f16(dev(dO)[None], dev(x)[None], p.row_len, p.cols, p.gx, p.gy, p.transposed_rows(), A_re, A_im, need_A=False)[0]
    big = layers.pack_operators([lc.operators("t")] * Bn).to(DEV)
    both = eng.dnet_gradient_features_backward_f16(rep(dO), rep(x), big.row_len, big.cols, big.gx, big.gy, big.transposed_rows(), A_re, A_im, need_A=False)[0]
    assert torch.equal(pl.bits(both), pl.bits(alone.repeat(Bn, 1, 1)))
    eh, mh, e1, e2 = p.half_operands()
    beh, bmh, be1, be2 = big.half_operands()
    times = dev(diffuse_operands(4, 4, Cw)[4])
    d1 = eng.dnet_diffuse_backward_f16(dev(dO)[None], None, eh, mh, e1, e2, p.evals, times, need_times=False)[0]
    dB = eng.dnet_diffuse_backward_f16(rep(dO), None, beh, bmh, be1, be2, big.evals, times, need_times=False)[0]
    assert torch.equal(pl.bits(dB), pl.bits(d1.repeat(Bn, 1, 1)))


# ---------------------------------------------------------------------------------------------------------------- 6. placement
def hostile(a, n_real, pad):
    """rows >= n_real[b] of a (B, n, ...) operand replaced by the fill"""
    a = a.copy()
    for b, n in enumerate(n_real):
        a[b, n:] = pl.INT_FILL if a.dtype.kind == "i" else pl.fill_value(torch.float16 if a.dtype == np.float16 else torch.float32, pad)
    return a


@pytest.mark.parametrize("pad,off", [("nan", 1), ("+inf", 2), ("-inf", 3)])
def test_placement_of_every_operand(eng, pad, off):
    p = packed("t", "f")
    n_real, n, R = [160, 76], 160, 163                          # mesh 1 is cut to 76 of its 81 rows: rows 76.. are padding too
    Cw, Co = 33, 70
    cpu = lambda t: t.cpu().numpy()
    rl, cols, gx, gy = cpu(p.row_len), cpu(p.cols), cpu(p.gx), cpu(p.gy)
    cols[1][cols[1] >= 76] = 0                                  # (a cut mesh keeps no column outside itself)
    cut = layers.PackedOperators(n_real, mass=p.mass, evals=p.evals, evecs=p.evecs, row_len=dev(rl), cols=dev(cols), gx=p.gx, gy=p.gy)
    rlt, colst, gxt, gyt = (cpu(t) for t in cut.transposed_rows())
    eh, mh, e1, e2 = cut.half_operands()
    eh, mh = cpu(eh), cpu(mh)
    x, dO, dY, Y = rnd(60, 2, n, Cw, scale=0.1), rnd(62, 2, n, Cw), rnd(67, 2, n, Co), rnd(68, 2, n, Co)
    x2 = rnd(61, 2, n, 19).astype(np.float16)
    W, times = rnd(63, Co, Cw + 19, scale=0.1).astype(np.float16), diffuse_operands(4, 4, Cw)[4]
    A_re, A_im = rnd(65, Cw, Cw, scale=0.2).astype(np.float16), rnd(66, Cw, Cw, scale=0.2).astype(np.float16)
    nv = dev(np.asarray(n_real, np.int32))

    def pad_rows(a, fill=0):
        out = np.full((a.shape[0], R) + a.shape[2:], fill, a.dtype)
        out[:, :n] = a
        return out
    # ---- control: aligned, dense, benign padding
    ctl = dict(x=pad_rows(x), x2=pad_rows(x2), dO=pad_rows(dO), dY=pad_rows(dY), Y=pad_rows(Y), eh=pad_rows(eh), mh=pad_rows(mh),
               rl=pad_rows(rl, 1), cols=pad_rows(cols), gx=pad_rows(gx), gy=pad_rows(gy), rlt=pad_rows(rlt, 1), colst=pad_rows(colst),
               gxt=pad_rows(gxt), gyt=pad_rows(gyt))
    d = {k: dev(v) for k, v in ctl.items()}
    lin = eng.dnet_linear_backward_f16(d["dY"], [d["x"], d["x2"]], dev(W), y=d["Y"], n_verts=nv)
    dif = eng.dnet_diffuse_backward_f16(d["dO"], d["x"], d["eh"], d["mh"], e1, e2, p.evals, dev(times), n_verts=nv)
    grd = eng.dnet_gradient_features_backward_f16(d["dO"], d["x"], d["rl"], d["cols"], d["gx"], d["gy"], (d["rlt"], d["colst"], d["gxt"], d["gyt"]),
                                                  dev(A_re), dev(A_im), n_verts=nv)
    want_act, want_par = [lin[0][0], lin[0][1], dif[0], grd[0]], [lin[1], lin[2], dif[1], grd[1], grd[2]]
    # ---- hostile: every operand an offset view with ld > width, fp16 ones off the 16-byte grid, the fill in padding columns, rows >= n_verts, slots >= row_len
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
        return pl.place(hostile(a, n_real, pad), offset_elems=off, ld=R, pad=None if a.dtype.kind == "i" else pad, device=DEV)

    def flat(a, ld=None):
        return pl.place(a, offset_elems=off, ld=ld, pad=pad, device=DEV)[..., :a.shape[-1]]
    hx_, hx2_, hdO, hdY, hY = mat(x), mat(x2), mat(dO), mat(dY), mat(Y)
    heh, hmh, hrl, hrlt = mat(eh), mat(mh), vec(rl), vec(rlt)
    hcols, hgx, hgy, hcolst, hgxt, hgyt = mat(hc, 0), mat(hx, 0), mat(hy, 0), mat(hct, 0), mat(hxt, 0), mat(hyt, 0)
    outs = [pl.place(np.zeros((2, R, c), np.float32), offset_elems=off, ld=c + 3, pad=pad, device=DEV) for c in (Cw, 19, Cw, Cw)]
    hW, hA, hAi = flat(W, W.shape[1] + 7), flat(A_re, Cw + 1), flat(A_im, Cw + 1)
    assert all(pl.mod16(t) != 0 for t in (hx_, hx2_, hdO, hdY, hY, heh, hmh, hrl, hcols, hgx, hgy, hcolst, hgxt, hgyt, outs[0], hW, hA, hAi))
    assert all(t.dtype == torch.float16 for t in (hx2_, heh, hmh, hW, hA, hAi))
    hnv = pl.place(np.asarray(n_real, np.int32), offset_elems=off, device=DEV)
    with pl.PointerRecorder(eng.lib, "dm_dnet_linear_bwd_data_f16") as rec, pl.PointerRecorder(eng.lib, "dm_dnet_linear_bwd_weight_f16") as rec2:
        lin = eng.dnet_linear_backward_f16(hdY, [hx_, hx2_], hW, y=hY, n_verts=hnv, out=[outs[0][..., :Cw], outs[1][..., :19]])
    assert rec.saw(hdY, hY, hW, hnv, outs[0], outs[1]) and rec2.saw(hdY, hY, hx_, hx2_, hnv)
    with pl.PointerRecorder(eng.lib, "dm_dnet_diffuse_bwd_f16") as rec:
        he1, he2 = (pl.place(cpu(e), offset_elems=off, device=DEV) for e in (e1, e2))
        dif = eng.dnet_diffuse_backward_f16(hdO, hx_, heh, hmh, he1, he2, flat(cpu(p.evals)), flat(times), n_verts=hnv,
                                            out=outs[2][..., :Cw])
    assert rec.saw(hdO, hx_, heh, hmh, hnv, outs[2])
    with pl.PointerRecorder(eng.lib, "dm_dnet_gradfeat_bwd_f16") as rec:
        grd = eng.dnet_gradient_features_backward_f16(hdO, hx_, hrl, hcols, hgx, hgy, (hrlt, hcolst, hgxt, hgyt), hA, hAi, n_verts=hnv,
                                                      out=outs[3][..., :Cw])
    assert rec.saw(hdO, hx_, hrl, hcols, hgx, hgy, hrlt, hcolst, hgxt, hgyt, hA, hAi, hnv, outs[3])
    fill_bits = pl.bits(torch.full((1,), pl.fill_value(torch.float32, pad), device=DEV))
    for name, w, o, c in zip(("d_src0", "d_src1", "diffuse dx", "gradfeat dx"), want_act, outs, (Cw, 19, Cw, Cw)):
        assert torch.equal(pl.bits(o[..., :c]), pl.bits(w)), (name, pad, off)
        assert bool((pl.bits(o[..., c:]) == fill_bits).all()), (name, "a padding column of the output was written")
        assert bool(torch.isfinite(w).all()) and bool((w[0, n_real[0]:] == 0).all()) and bool((w[1, n_real[1]:] == 0).all())
    for name, w, g in zip(("dW", "db", "dtimes", "dA_re", "dA_im"), want_par, [lin[1], lin[2], dif[1], grd[1], grd[2]]):
        assert bool(torch.isfinite(w).all()) and torch.equal(pl.bits(g), pl.bits(w)), (name, pad, off)


# ---------------------------------------------------------------------------------------------------------------- 7. the forward value
def rounded_weights(net):
    """the weight dict of MatchEngine.diffusion_net_forward with every matrix rounded to float16, biases and times float32"""
    w = net.device_weights()
    h = lambda t: None if t is None else t.to(torch.float16)
    return {"first": (h(w["first"][0]), w["first"][1]), "last": (h(w["last"][0]), w["last"][1]),
            "blocks": [{"times": b["times"], "A_re": h(b["A_re"]), "A_im": h(b["A_im"]), "mlp": [(h(W), bias) for W, bias in b["mlp"]]} for b in w["blocks"]]}


@pytest.mark.parametrize("case", ["a", "b", "c", "many"])
def test_forward_value_is_the_engine_call(eng, case, monkeypatch):
    c = mc.Case(case, DEV)
    xs = torch.zeros((len(c.xs), c.packed.mass.shape[1], c.xs[0].shape[-1]), device=DEV)
    for b, x in enumerate(c.xs):
        xs[b, :x.shape[0]] = x
    with torch.no_grad():
        want = eng.diffusion_net_forward(rounded_weights(c.net), c.packed, xs, out_dtype=torch.float32)
    seen = []
    monkeypatch.setattr(c.net, "_tail", lambda x, *a, _orig=c.net._tail: (seen.append(x), _orig(x, *a))[1])
    leaf = c.leaf()
    if case == "many":
        ys = c.net.forward_many(leaf, c.packed, differentiable=True, compute_dtype=torch.float16)
        got = torch.zeros_like(want)
        for b, t in enumerate(seen):
            got[b, :t.shape[1]] = t[0]
    else:
        ys = [c.net(leaf, route="device", differentiable=True, compute_dtype=torch.float16, operators=c.packed)]
        got = seen[0]
    assert c.net.last_route == "device" and all(y.dtype == torch.float32 and y.requires_grad for y in ys)
    assert got.dtype == torch.float32 and torch.equal(pl.bits(got.detach()), pl.bits(want))
    assert not torch.equal(got.detach(), eng.diffusion_net_forward(c.net.device_weights(), c.packed, xs))           # (not the fp32 kernels)


# ---------------------------------------------------------------------------------------------------------------- 8. whole network
def device_run(c, eng, monkeypatch, train_masks=None):
    """the route under test: (gradients in Case.collect's layout, its ReLU masks, recorded by wrapping the engine's linear wrapper)"""
    recorded = []

    def spy(*a, _orig=eng.dnet_linear_f16, **k):
        out = _orig(*a, **k)
        if k.get("relu"):
            recorded.append(out.detach() > 0)
        return out
    monkeypatch.setattr(eng, "dnet_linear_f16", spy)
    try:
        c.net.zero_grad()
        leaf = c.leaf()
        if c.case == "many":
            ys = c.net.forward_many(leaf, c.packed, differentiable=True, compute_dtype=torch.float16)
        else:
            y = c.net(leaf, route="device", differentiable=True, compute_dtype=torch.float16, **c.kw)
            ys = [y[b] for b in range(y.shape[0])] if c.batched else [y]
        assert c.net.last_route == "device" and all(y.dtype == torch.float32 and y.requires_grad for y in ys)
        c.loss(ys).backward()
    finally:
        monkeypatch.undo()
    return c.collect(leaf), c.split_masks(recorded)


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "many"])
def test_whole_network_gradients_against_torch_autocast(eng, case, monkeypatch):
    """The acceptance.  Loss 2^s sum (y * g) (s: dnet_mixed_checks.SCALE).  Figure: per tensor max |got - ref| / max |ref| against the masked
    oracle under the run's own masks.  Yardstick: the same figure of the same fp32 module on route='torch' under
    torch.autocast('cuda', dtype=torch.float16), same inputs, g and s.  Required: the device route's largest figure over the tensors does
    not exceed the yardstick's largest; no allowance.  A single tensor whose own ratio exceeds 1 is printed, not failed."""
    c = mc.Case(case, DEV)
    got, got_masks = device_run(c, eng, monkeypatch)
    yard, yard_masks = mc.autocast_run(c, "cuda")
    ref_got, top = c.oracle(got_masks)
    ref_yard, _ = c.oracle(yard_masks)
    flips = sum(int((a.cpu() != b.cpu()).sum()) for la, lb in zip(got_masks, yard_masks) for a, b in zip(la, lb))
    print(f"case {case}: s = {mc.SCALE[case]}, largest staged gradient operand of the oracle 2^{math.log2(top):.2f}; {flips} ReLU mask entries differ "
          f"between the two runs")
    assert top < 2.0 ** 14
    top_d, top_y = mc.report(f"case {case}", br.figures(got, ref_got), br.figures(yard, ref_yard))
    assert top_d <= top_y, (case, top_d, top_y)


# ---------------------------------------------------------------------------------------------------------------- 9. training mode
def test_training_mode_with_dropout(eng, monkeypatch):
    """dropout=True after .train(): each nn.Dropout's keep mask is recorded by a forward hook during the device run and handed to the
    masked oracle with the run's ReLU masks.  The yardstick is the acceptance's -- the torch route under autocast -- made to drop the same
    entries: its nn.Dropout outputs are replaced by input * keep / (1 - p).  Required, as there: the largest device figure does not
    exceed the largest yardstick figure."""
    c = mc.Case("a", DEV)
    c.net = copy.deepcopy(c.net).train()
    drops = [m for m in c.net.modules() if isinstance(m, torch.nn.Dropout)]
    assert c.net.dropout and c.net.training and len(drops) == 4
    keep = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: keep.append((out != 0)[None] if out.dim() == 2 else out != 0)) for m in drops]
    try:
        torch.manual_seed(1234)
        got, masks = device_run(c, eng, monkeypatch)
    finally:
        for h in hooks:
            h.remove()
    assert len(keep) == 4 and 0.1 < float(keep[0].float().mean()) < 0.7          # (half of the ReLU's outputs are zero to begin with)
    turn = iter(range(4))
    hooks = [m.register_forward_hook(lambda mod, inp, out: inp[0] * keep[next(turn)].reshape(inp[0].shape).to(inp[0].dtype) / (1.0 - mod.p)) for m in drops]
    try:
        yard, yard_masks = mc.autocast_run(c, "cuda")
    finally:
        for h in hooks:
            h.remove()
    ref_got, _ = c.oracle(masks, drop_masks=keep)
    ref_yard, _ = c.oracle(yard_masks, drop_masks=keep)
    top_d, top_y = mc.report("training mode", br.figures(got, ref_got), br.figures(yard, ref_yard))
    assert top_d <= top_y, (top_d, top_y)


def test_frozen_parameters_and_one_sgd_step(eng, monkeypatch):
    c = mc.Case("a", DEV)
    c.net = net = copy.deepcopy(c.net)
    frozen = ["first_lin.weight", "block_0.diffusion.diffusion_time", "block_0.gradient_features.A_re.weight", "block_0.gradient_features.A_im.weight",
              "block_1.mlp.miniMLP_mlp_layer_000.weight", "block_1.mlp.miniMLP_mlp_layer_000.bias"]
    named = dict(net.named_parameters())
    for name in frozen:
        named[name].requires_grad_(False)
    calls = {"linear": [], "diffuse": [], "gradfeat": []}
    for key, name in (("linear", "dnet_linear_backward_f16"), ("diffuse", "dnet_diffuse_backward_f16"), ("gradfeat", "dnet_gradient_features_backward_f16")):
        def spy(*a, _orig=getattr(eng, name), _key=key, **k):
            calls[_key].append((a, k))
            return _orig(*a, **k)
        monkeypatch.setattr(eng, name, spy)
    recorded = []

    def fwd_spy(*a, _orig=eng.dnet_linear_f16, **k):
        out = _orig(*a, **k)
        if k.get("relu"):
            recorded.append(out.detach() > 0)
        return out
    monkeypatch.setattr(eng, "dnet_linear_f16", fwd_spy)
    net.zero_grad()
    before = {name: q.detach().clone() for name, q in named.items()}
    y = net(c.x, route="device", differentiable=True, compute_dtype=torch.float16, **c.kw)          # x needs no gradient either
    c.loss([y]).backward()
    assert all(named[name].grad is None for name in frozen)
    # backward order: last_lin first, first_lin last.  first_lin: no source gradient, no weight gradient (its weight copy is not saved: None), the bias gradient
    (a, first) = calls["linear"][-1]
    assert first["need_src"] == [False] and not first["need_weight"] and first["need_bias"] and a[2] is None
    layer = [(a, k) for a, k in calls["linear"][:-1] if k["need_weight"] is False and k["need_bias"] is False and all(k["need_src"])]
    assert len(layer) == 1 and all(isinstance(s, int) for s in layer[0][0][1])                       # block_1's frozen layer: its sources were not saved
    assert [k["need_times"] for _, k in calls["diffuse"]] == [True, False] and all(k["need_x"] for _, k in calls["diffuse"])
    assert [a[1] is None for a, _ in calls["diffuse"]] == [False, True]                                # x is saved for the gradient of the times only
    assert [k["need_A"] for _, k in calls["gradfeat"]] == [True, False]
    got = {name: q.grad.detach().clone() for name, q in named.items() if q.grad is not None}
    monkeypatch.undo()
    ref, _ = c.oracle(c.split_masks(recorded))
    ref = {k: v for k, v in ref.items() if k in got}
    assert set(got) == set(named) - set(frozen) and not any(name in ref for name in frozen)
    yard, yard_masks = mc.autocast_run(c, "cuda")                   # the acceptance's yardstick on the same frozen module
    ref_yard, _ = c.oracle(yard_masks)
    top_d, top_y = mc.report("frozen parameters", br.figures(got, ref), br.figures({k: yard[k] for k in got}, {k: ref_yard[k] for k in got}))
    assert top_d <= top_y, (top_d, top_y)
    for name, q in named.items():                                   # (the yardstick run left its own gradients behind)
        q.grad = got.get(name)
    lr = 0.05 / c.scale
    torch.optim.SGD([q for q in net.parameters() if q.requires_grad], lr=lr).step()
    for name, q in named.items():
        if name in frozen:
            assert torch.equal(q.detach(), before[name]), name
            continue
        want = before[name].double().cpu() - lr * ref[name]
        err = float((q.detach().double().cpu() - want).abs().max())
        # fl(w - lr g): lr |g - g_ref| <= lr (the yardstick's largest figure) max |g_ref|, and the roundings of the product and of the update
        allow = lr * top_y * float(ref[name].abs().max()) + 2.0 ** -23 * float(want.abs().max())
        print(f"SGD step {name}: max |w - oracle step| = {err:.3e} (allowed {allow:.3e}), moved by {float((q.detach() - before[name]).abs().max()):.3e}")
        assert err <= allow and not torch.equal(q.detach(), before[name]), name


# ---------------------------------------------------------------------------------------------------------------- 10. GradScaler
def test_grad_scaler():
    """torch.amp.GradScaler exactly as with autocast: a sane scale steps; a scale that pushes a staged gradient past 65504 gives
    non-finite gradients, the step is skipped and the scale halves"""
    c = mc.Case("a", DEV)
    net = copy.deepcopy(c.net)
    g = c.gs[0]
    for init, steps in ((2.0 ** mc.SCALE["a"], True), (2.0 ** (mc.SCALE["a"] + 8), False)):
        opt = torch.optim.SGD(net.parameters(), lr=1e-3)
        scaler = torch.amp.GradScaler("cuda", init_scale=init)
        opt.zero_grad()
        loss = (net(c.x, route="device", differentiable=True, compute_dtype=torch.float16, **c.kw) * g).sum()
        before = [q.detach().clone() for q in net.parameters()]            # (behind the forward: it clamps the times in place)
        scaler.scale(loss).backward()
        finite = all(bool(torch.isfinite(q.grad).all()) for q in net.parameters())
        scaler.step(opt)
        scaler.update()
        moved = any(not torch.equal(q.detach(), w) for q, w in zip(net.parameters(), before))
        print(f"GradScaler init 2^{math.log2(init):.0f}: gradients finite {finite}, parameters moved {moved}, scale afterwards 2^{math.log2(scaler.get_scale()):.0f}")
        assert finite == steps and moved == steps
        assert scaler.get_scale() == (init if steps else init / 2)


# ---------------------------------------------------------------------------------------------------------------- 11. refusals
def test_refusals(eng):
    net = lc.network("a", DEV)
    x, kw = lc.call_arguments("a", DEV)
    mixed = dict(route="device", differentiable=True, compute_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="on the GPU"):
        net(x.cpu(), **mixed, **{k: v.cpu() for k, v in kw.items()})
    half = copy.deepcopy(net).half()
    for xin in (x, x.half()):
        with pytest.raises(RuntimeError, match="float32 .the fp16 kernels have no backward"):
            half(xin, **mixed, **kw)
    with pytest.raises(RuntimeError, match="float32 or float16, not float64"):
        net(x.double(), **mixed, **kw)
    with pytest.raises(RuntimeError, match="must not require grad"):
        net(x.half().requires_grad_(), **mixed, **kw)
    with pytest.raises(ValueError, match="compute_dtype"):
        net(x, route="device", differentiable=True, compute_dtype=torch.bfloat16, **kw)
    with pytest.raises(RuntimeError, match="requires grad"):       # without differentiable= the keyword is ignored and the route still refuses
        net(x.clone().requires_grad_(), route="device", compute_dtype=torch.float16, **kw)
    imp = copy.deepcopy(net)
    imp.diffusion_method = "implicit_dense"
    with pytest.raises(RuntimeError, match="spectral"):
        imp(x, **mixed, **kw)
    n, K = 8, K_MAX + 1
    wide = layers.pack_operators([(None, torch.ones(n), None, torch.zeros(K), torch.zeros((n, K)), None, None)]).to(DEV)
    with pytest.raises(RuntimeError, match="k_eig must be at most 1024"):
        net(torch.zeros((n, 19), device=DEV), operators=wide, **mixed)
    y = net(x.half(), **mixed, **kw)                                # a float16 input that needs no gradient is taken
    assert y.dtype == torch.float32 and y.requires_grad
    # ---- DM_EINVAL of the four entries
    z = lambda *s: torch.zeros(s, device=DEV)
    zh = lambda *s: torch.zeros(s, device=DEV, dtype=torch.float16)
    P, null = (lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)), ctypes.c_void_p(0)
    dY, dX, W, ws = z(1, n, 4), z(1, n, 4), zh(4, 8), torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    F32, F16 = _lib.DM_F32, _lib.DM_F16

    def data(B=1, N=n, Co=4, w=4, ld=4, lddy=4, ldw=4, act=0, Y=null, nsrc=1, Wp=P(W), dYp=P(dY)):
        return eng.lib.dm_dnet_linear_bwd_data_f16(eng.ctx, B, N, Co, nsrc, dYp, lddy, Y, 4, act, Wp, ldw, null, P(dX), w, ld, null, 0, 0, null, 0, 0)

    def weight(B=1, N=n, Co=4, w=4, ld=4, lddy=4, lddw=4, act=0, Y=null, nsrc=1, wsp=P(ws), src=P(dX), dt=F32):
        return eng.lib.dm_dnet_linear_bwd_weight_f16(eng.ctx, B, N, Co, nsrc, P(dY), lddy, Y, 4, act, src, w, ld, dt, null, 0, 0, F32, null, 0, 0, F32,
                                                     null, wsp, P(dX), lddw, null)
    K4 = 3
    eh, mh, e12, ev, tm = zh(1, n, K4 + 1), zh(1, n, K4 + 1), torch.zeros(1, dtype=torch.int32, device=DEV), z(1, K4), z(4)

    def diffuse(B=1, N=n, K=K4, Cc=4, lddo=4, ldx=4, lde=K4, ldm=K4, xp=P(dX), ehp=P(eh), wsp=P(ws), lddx=4, dt=P(tm), dOp=P(dY)):
        return eng.lib.dm_dnet_diffuse_bwd_f16(eng.ctx, B, N, K, Cc, dOp, lddo, xp, ldx, ehp, lde, P(mh), ldm, P(e12), P(e12), P(ev), P(tm), null, wsp,
                                               P(dX), lddx, dt)
    rl, cl, gv, A = torch.ones((1, n), dtype=torch.int32, device=DEV), torch.zeros((1, n, 1), dtype=torch.int32, device=DEV), z(1, n, 1), zh(4, 8)
    dA = z(4, 4)

    def gradfeat(B=1, N=n, Cc=4, nnz=1, nnz_t=1, rlt=P(rl), lddo=4, ldx=4, lda=4, Ap=P(A), Aip=null, wsp=P(ws), lddx=4, dAim=null, ldda=4):
        return eng.lib.dm_dnet_gradfeat_bwd_f16(eng.ctx, B, N, Cc, nnz, P(rl), P(cl), P(gv), P(gv), nnz_t, rlt, P(cl), P(gv), P(gv), P(dY), lddo, P(dX), ldx,
                                                Ap, Aip, lda, null, wsp, P(dX), lddx, P(dA), dAim, ldda)
    bad = [("data", data, k) for k in (dict(B=0), dict(N=0), dict(Co=0), dict(w=0), dict(ld=3), dict(lddy=3), dict(ldw=3), dict(act=1), dict(act=2),
                                        dict(nsrc=0), dict(nsrc=4), dict(Wp=P(W, 1)), dict(Wp=null), dict(dYp=P(dY, 2)))]
    bad += [("weight", weight, k) for k in (dict(B=0), dict(N=-1), dict(Co=0), dict(w=0), dict(ld=3), dict(lddy=3), dict(lddw=3), dict(act=1),
                                            dict(nsrc=4), dict(wsp=null), dict(dt=7), dict(src=P(dX, 2)), dict(src=P(dX, 1), dt=F16), dict(src=null))]
    bad += [("diffuse", diffuse, k) for k in (dict(B=0), dict(N=0), dict(K=0), dict(K=K_MAX + 1, lde=K_MAX + 1, ldm=K_MAX + 1), dict(Cc=0), dict(lddo=3),
                                              dict(lde=2), dict(ldm=2), dict(xp=null), dict(ldx=3), dict(ehp=P(eh, 1)), dict(ehp=null), dict(wsp=null),
                                              dict(lddx=3), dict(dOp=P(dY, 2)))]
    bad += [("gradfeat", gradfeat, k) for k in (dict(B=0), dict(N=0), dict(Cc=0), dict(nnz=0), dict(nnz_t=0), dict(rlt=null), dict(lddo=3), dict(ldx=3),
                                                dict(lda=3), dict(Ap=P(A, 1)), dict(Ap=null), dict(Aip=P(A, 1)), dict(wsp=null), dict(lddx=3),
                                                dict(dAim=P(dA)), dict(ldda=3))]
    for name, fn, k in bad:
        rc = fn(**k)
        assert rc == _lib.DM_EINVAL, (name, k, rc)
        with pytest.raises(ValueError):
            eng._chk(rc)
    for counts in ([0], [n + 1]):
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_linear_backward_f16(dY, [dY], zh(4, 4), n_verts=counts)
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_diffuse_backward_f16(dY, dY, zh(1, n, 3), zh(1, n, 3), e12, e12, z(1, 3), z(4), n_verts=counts)
    assert data() == 0 and weight() == 0 and diffuse() == 0 and gradfeat() == 0 and gradfeat(Aip=P(A), dAim=P(dA)) == 0
    assert weight(src=P(zh(1, n, 4)), dt=F16) == 0
    xi = x.clone().requires_grad_()
    y = net(xi, **mixed, **kw)                                      # the engine and the route are usable afterwards
    y.sum().backward()
    assert bool(torch.isfinite(xi.grad).all()) and float(xi.grad.abs().max()) > 0

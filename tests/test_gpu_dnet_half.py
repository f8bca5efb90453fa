"""The fp16 route through DiffusionNet on the GPU (dm_dnet_linear_f16, dm_dnet_diffuse_f16, dm_dnet_gradfeat_f16; the device route of a
module after .half()): every kernel against its restatement within the restatement's bound (tests/dnet_half_restate.py), scale
invariance of the diffusion, batches and tile shapes bit for bit, hostile operand placement, the whole network against the float64 network
next to the torch route under autocast, the drop-in behaviour and the refusals.  Every figure is printed before it is asserted."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dnet_checks as dc
import dnet_half_restate as hs
import dnet_layers_checks as lc
import dnet_layers_restate as rs
import lift_checks as lk
import placement as pl
from densematcher_amd import _lib
from densematcher_amd.diffusion_net import layers

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32 = np.float16, np.float32


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


@pytest.fixture(autouse=True)
def inference():
    with torch.no_grad():
        yield


def rnd(seed, *shape, scale=1.0, dtype=F32):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(F32).astype(dtype)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def opt(a):
    return None if a is None else dev(a)


def within(got, ref, bound, tag):
    got = got.detach().cpu().double().numpy()
    err = np.abs(got - ref)
    share = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{tag}: max |got - ref| = {err.max():.3e}, max |ref| = {np.abs(ref).max():.3e}, largest share of the bound {share:.3e}")
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert np.all(err <= bound), (tag, share)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(pl.bits(a), pl.bits(b))


# ---------------------------------------------------------------------------------------------------------------- 1. linear
OPTS = [(b, r, s) for b in (False, True) for r in (False, True) for s in (False, True)]          # bias, ReLU, resid: every combination
WIDTHS = ((19,), (5, 3), (33, 51, 16))
KINDS = {"f32": lambda i: F32, "f16": lambda i: F16, "mixed": lambda i: (F16, F32, F32)[i]}        # mixed: lifted fp16, the rest fp32
LINEAR = [(N, Co, w, ("f32", "f16", "mixed")[(b + c) % 3], OPTS[(9 * a + 3 * b + c) % 8], (F16, F32)[(a + c) % 2])
          for a, N in enumerate((1, 81, 257)) for b, Co in enumerate((1, 48, 130)) for c, w in enumerate(WIDTHS)]


def test_linear_cases_cover_every_option_and_dtype():
    assert {c[4] for c in LINEAR} == set(OPTS)
    assert {(c[2], c[3]) for c in LINEAR} == {(w, k) for w in WIDTHS for k in KINDS}


@pytest.mark.parametrize("N,Co,widths,kind,opts,bias_dtype", LINEAR)
def test_linear_against_the_restatement(eng, N, Co, widths, kind, opts, bias_dtype):
    bias, relu, resid = opts
    srcs = [rnd(10 + i, N, w, dtype=KINDS[kind](i)) for i, w in enumerate(widths)]
    W = rnd(20, Co, sum(widths), scale=sum(widths) ** -0.5, dtype=F16)
    b = rnd(21, Co, dtype=bias_dtype) if bias else None
    r = rnd(22, N, Co) if resid else None
    tag = f"linear_f16 N={N} C_out={Co} widths={widths} {kind} {opts}"
    got = eng.dnet_linear_f16([dev(s) for s in srcs], dev(W), opt(b), opt(r), relu=relu)
    assert got.shape == (N, Co) and got.dtype == torch.float32
    within(got, hs.linear(srcs, W, b, r, relu), hs.linear_bound(srcs, W, b, r), tag)
    low = eng.dnet_linear_f16([dev(s) for s in srcs], dev(W), opt(b), opt(r), relu=relu, out_dtype=torch.float16)
    assert low.dtype == torch.float16 and same_bits(low, got.to(torch.float16))       # the fp32 result rounded once more
    within(low, hs.linear(srcs, W, b, r, relu, out16=True), hs.linear_bound(srcs, W, b, r, out16=True), tag + " fp16 out")


def test_linear_rounds_its_sources_where_they_are_staged(eng):
    """a float32 source gives the bits of its fp16 rounding given as float16, and weights of one exact product per output show them"""
    x = rnd(23, 81, 19)
    W, b = rnd(24, 48, 19, scale=0.2, dtype=F16), rnd(25, 48, dtype=F16)
    a = eng.dnet_linear_f16(dev(x), dev(W), dev(b))
    assert same_bits(a, eng.dnet_linear_f16(dev(x.astype(F16)), dev(W), dev(b)))
    assert same_bits(a, eng.dnet_linear_f16(dev(x), dev(W), dev(b.astype(F32))))              # the bias is widened exactly
    eye = np.eye(19, dtype=F16)
    assert same_bits(eng.dnet_linear_f16(dev(x), dev(eye)), dev(x.astype(F16).astype(F32)))


# ---------------------------------------------------------------------------------------------------------------- 2. diffuse
def diffuse_operands(N, K, Cw, seed=0, mass_scale=1.0):
    g = np.random.default_rng(seed)
    x, evecs = rnd(seed + 1, N, Cw), rnd(seed + 2, N, K, scale=0.3)
    mass = (mass_scale * (0.002 + 0.01 * g.random(N))).astype(F32)
    evals = np.sort(40.0 * g.random(K)).astype(F32)
    times = (0.05 * g.random(Cw)).astype(F32)
    times[0] = 0.0
    if Cw > 1:
        times[1] = -0.01
    return x, mass, evals, evecs, times


def pack_for(mass, evals, evecs):
    """a PackedOperators of the meshes (mass (B,N), evals (B,K), evecs (B,N,K)) without gradient rows, on the GPU"""
    Bn, N = mass.shape
    ones = torch.ones((Bn, N), dtype=torch.int32)
    return layers.PackedOperators([N] * Bn, mass=torch.from_numpy(mass), evals=torch.from_numpy(evals), evecs=torch.from_numpy(evecs), row_len=ones,
                                  cols=torch.zeros((Bn, N, 1), dtype=torch.int32), gx=torch.zeros((Bn, N, 1)), gy=torch.zeros((Bn, N, 1))).to(DEV)


def run_diffuse(eng, x, mass, evals, evecs, times):
    p = pack_for(mass[None], evals[None], evecs[None])
    return eng.dnet_diffuse_f16(dev(x)[None], *p.half_operands(), p.evals, dev(times))[0]


# mass_scale 0.03: vertex masses around 1e-4, the bottom of fp16's normal range, as a 2048-vertex mesh of unit area has them
@pytest.mark.parametrize("N,K,Cw,times_dtype,mass_scale", [(1, 1, 1, F32, 1.0), (81, 16, 48, F16, 1.0), (257, 128, 130, F32, 0.03), (160, 16, 32, F16, 0.03)])
def test_diffuse_against_the_restatement(eng, N, K, Cw, times_dtype, mass_scale):
    x, mass, evals, evecs, times = diffuse_operands(N, K, Cw, mass_scale=mass_scale)
    times = times.astype(times_dtype)
    got = run_diffuse(eng, x, mass, evals, evecs, times)
    assert got.dtype == torch.float32
    ref = hs.diffuse(x, mass, evals, evecs, times)
    within(got, ref, hs.diffuse_bound(x, mass, evals, evecs, times), f"diffuse_f16 N={N} K={K} C={Cw} mass ~ {mass.mean():.1e}")
    # the operands of the device pack are those of the restatement, bit for bit
    eh, mh, e1, e2 = pack_for(mass[None], evals[None], evecs[None]).half_operands()
    weh, wmh, we1, we2 = hs.half_operands(mass, evecs)
    assert (int(e1[0]), int(e2[0])) == (we1, we2)
    assert np.array_equal(eh[0].cpu().numpy().astype(np.float64), weh) and np.array_equal(mh[0].cpu().numpy().astype(np.float64), wmh)
    if N > 1:
        # against the float64 diffusion of the unrounded operands: the error is that of fp16 operands (a few 2^-11 of the magnitudes),
        # not of masses rounded on their own at 1e-4 (the reference's half route: 2^-11 relative at best, flushed below 6e-5)
        # four roundings to fp16 on the way (x, mevecs_h, d, evecs_h), two fp32 accumulations, d below fp16's normal range
        exact, mag = rs.diffuse(x, mass, evals, evecs, times.astype(F32)), rs.diffuse_bound(x, mass, evals, evecs, times.astype(F32)) / (rs.U * rs.SLACK * (N + K + 9))
        allowed = hs.SLACK * (4 * hs.U16 + (N + K + 8) * hs.U32) * mag + np.ldexp(np.abs(weh).sum(axis=1), -14)[:, None] * hs.TINY16
        share = float((np.abs(got.cpu().double().numpy() - exact) / allowed).max())
        print(f"diffuse_f16 N={N} K={K}: error against the float64 diffusion of the unrounded operands, largest share of what fp16 operands allow: {share:.3e}")
        assert share <= 1.0


@pytest.mark.parametrize("mass_exp,evecs_exp", [(-20, 10), (8, -4)])
def test_diffusion_is_invariant_under_the_scaling_of_its_operands(eng, mass_exp, evecs_exp):
    """evecs -> s evecs, mass -> mass / s^2 leaves the diffusion as it is; with s a power of two every output bit stays"""
    x, mass, evals, evecs, times = diffuse_operands(160, 16, 32, seed=5)
    want = run_diffuse(eng, x, mass, evals, evecs, times)
    got = run_diffuse(eng, x, np.ldexp(mass, mass_exp).astype(F32), evals, np.ldexp(evecs, evecs_exp).astype(F32), times)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert same_bits(got, want)


# ---------------------------------------------------------------------------------------------------------------- 3. gradient features
@functools.lru_cache(maxsize=None)
def packed(*keys):
    return layers.pack_operators([lc.operators(k) for k in keys]).to(DEV)


def gradfeat_case(eng, p, b, Cw, rot, tag):
    n = p.n_verts[b]
    x = rnd(31, n, Cw, scale=0.1)
    A_re, A_im = rnd(32, Cw, Cw, scale=Cw ** -0.5, dtype=F16), (rnd(33, Cw, Cw, scale=Cw ** -0.5, dtype=F16) if rot else None)
    sl = lambda t: t[b:b + 1, :n].contiguous()
    got = eng.dnet_gradient_features_f16(dev(x)[None], sl(p.row_len), sl(p.cols), sl(p.gx), sl(p.gy), dev(A_re), opt(A_im))[0]
    assert got.dtype == torch.float32
    Gx, Gy = p.dense_grad(b, "gx").cpu().numpy(), p.dense_grad(b, "gy").cpu().numpy()
    ref, dots = hs.gradfeat(x, Gx, Gy, A_re, A_im)
    share = float((np.abs(dots) < 2).mean())
    print(f"{tag}: |dots| < 2 at {share:.3f} of the entries, largest {np.abs(dots).max():.3f}")
    assert share >= 0.5                                        # a saturated tanh would hide the gradient path
    within(got, ref, hs.gradfeat_bound(x, Gx, Gy, A_re, A_im), tag)
    return got


@pytest.mark.parametrize("key", ["f", "t"])
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("Cw", [32, 48])
def test_gradfeat_against_the_restatement(eng, key, rot, Cw):
    gradfeat_case(eng, packed(key), 0, Cw, rot, f"gradfeat_f16 mesh {key} C={Cw} rotations={rot}")


@pytest.mark.parametrize("width", [64, 65, 90])
def test_gradfeat_row_width_does_not_change_the_bits(eng, width):
    """an ELL width beyond the longest row (41 on mesh f), below and above the 64 slots the kernel keeps in LDS, the extra slots hostile"""
    p = packed("f")
    n, w0, Cw = p.n_verts[0], p.cols.shape[2], 48
    x, A_re, A_im = dev(rnd(34, 1, n, Cw, scale=0.1)), dev(rnd(35, Cw, Cw, scale=0.15, dtype=F16)), dev(rnd(36, Cw, Cw, scale=0.15, dtype=F16))
    want = eng.dnet_gradient_features_f16(x, p.row_len, p.cols, p.gx, p.gy, A_re, A_im)
    cols = torch.full((1, n, width), pl.INT_FILL, dtype=torch.int32, device=DEV)
    gx = torch.full((1, n, width), float("nan"), device=DEV)
    gy = gx.clone()
    keep = (torch.arange(w0, device=DEV)[None, None, :] < p.row_len[:, :, None])
    cols[..., :w0][keep], gx[..., :w0][keep], gy[..., :w0][keep] = p.cols[keep], p.gx[keep], p.gy[keep]
    got = eng.dnet_gradient_features_f16(x, p.row_len, cols, gx, gy, A_re, A_im)
    assert bool(torch.isfinite(got).all()) and same_bits(got, want)


def test_gradfeat_decomposition_does_not_change_the_bits(eng):
    """Up to 768 channels, and once 32-row tiles give every CU one (256 of them), a workgroup keeps the rounded gradients of its rows in
    LDS for every channel; a lone mesh takes 64 x 64 tiles that gather per column tile.  52 padded fixture meshes are 260 row tiles:
    each has the bits of its single call."""
    keys = ("f", "t") * 26
    p = layers.pack_operators([lc.operators(k) for k in keys]).to(DEV)
    Bn, N, Cw = len(keys), p.mass.shape[1], 48
    assert -(-N // 32) * Bn >= 256 > -(-N // 32) * 2
    x = torch.full((Bn, N, Cw), float("nan"), device=DEV)
    for b, n in enumerate(p.n_verts):
        x[b, :n] = dev(rnd(37 + b % 3, n, Cw, scale=0.1))
    for A_im in (dev(rnd(39, Cw, Cw, scale=0.15, dtype=F16)), None):
        A_re = dev(rnd(38, Cw, Cw, scale=0.15, dtype=F16))
        big = eng.dnet_gradient_features_f16(x, p.row_len, p.cols, p.gx, p.gy, A_re, A_im, n_verts=p.n_verts_dev)
        for b in (0, 1, 50, 51):
            one, n = packed(keys[b]), p.n_verts[b]
            alone = eng.dnet_gradient_features_f16(x[b:b + 1, :n].contiguous(), one.row_len, one.cols, one.gx, one.gy, A_re, A_im)
            assert float(alone.abs().max()) > 0 and same_bits(big[b:b + 1, :n], alone), b
            assert bool((big[b, n:] == 0).all())


def test_gradfeat_unreferenced_vertex(eng):
    fx = dc.golden()
    n = fx["verts_u"].shape[0]
    sp = lambda name: torch.sparse_coo_tensor(torch.from_numpy(np.stack((fx[f"{name}_row_u"], fx[f"{name}_col_u"])).astype(np.int64)),
                                              torch.from_numpy(fx[f"{name}_val_u"].astype(np.float32)), (n, n)).coalesce()
    op = (None, torch.ones(n), None, torch.zeros(1), torch.zeros((n, 1)), sp("gradX"), sp("gradY"))
    p = layers.pack_operators([op]).to(DEV)
    assert int(p.row_len[0, n - 1]) == 1 and int(p.cols[0, n - 1, 0]) == n - 1 and float(p.gx[0, n - 1, 0]) == 0.0
    got = gradfeat_case(eng, p, 0, 32, True, "gradfeat_f16 mesh u")
    assert bool((got[n - 1] == 0).all())                       # tanh(0)


# ---------------------------------------------------------------------------------------------------------------- 4. batches and tiles
def test_ragged_batch_equals_the_single_calls(eng):
    keys = ("t", "f")
    p = packed(*keys)
    Bn, N, Cw = 2, p.mass.shape[1], 32
    assert p.n_verts == [160, 81] and p.n_verts_dev is not None
    x = torch.full((Bn, N, Cw), float("nan"), device=DEV)
    for b, n in enumerate(p.n_verts):
        x[b, :n] = dev(rnd(40 + b, n, Cw, scale=0.1))
    xh = x.to(torch.float16)
    W, bias, times = dev(rnd(44, 48, 2 * Cw, scale=0.1, dtype=F16)), dev(rnd(45, 48, dtype=F16)), dev(diffuse_operands(4, 4, Cw)[4].astype(F16))
    A_re, A_im = dev(rnd(46, Cw, Cw, scale=0.2, dtype=F16)), dev(rnd(47, Cw, Cw, scale=0.2, dtype=F16))
    nv = p.n_verts_dev
    lin = eng.dnet_linear_f16([xh, x], W, bias, relu=True, n_verts=nv)
    dif = eng.dnet_diffuse_f16(x, *p.half_operands(), p.evals, times, n_verts=nv)
    grd = eng.dnet_gradient_features_f16(x, p.row_len, p.cols, p.gx, p.gy, A_re, A_im, n_verts=nv)
    for b, (key, n) in enumerate(zip(keys, p.n_verts)):
        one = packed(key)
        xb, xhb = x[b:b + 1, :n].contiguous(), xh[b:b + 1, :n].contiguous()
        assert same_bits(lin[b, :n], eng.dnet_linear_f16([xhb, xb], W, bias, relu=True)[0]), key
        assert same_bits(dif[b, :n], eng.dnet_diffuse_f16(xb, *one.half_operands(), one.evals, times)[0]), key
        assert same_bits(grd[b, :n], eng.dnet_gradient_features_f16(xb, one.row_len, one.cols, one.gx, one.gy, A_re, A_im)[0]), key
        for out in (lin, dif, grd):
            assert bool(torch.isfinite(out[b, :n]).all()) and bool((out[b, n:] == 0).all()), key
            assert float(out[b, :n].abs().max()) > 0
    net = lc.network("a", DEV).half()
    xs = [dev(rnd(50 + b, n, 19)) for b, n in enumerate(p.n_verts)]
    many = net.forward_many(xs, p)
    assert net.last_route == "device" and [tuple(y.shape) for y in many] == [(n, 24) for n in p.n_verts]
    for b, key in enumerate(keys):
        alone = net(xs[b], route="device", operators=packed(key))
        assert many[b].dtype == torch.float16 and same_bits(many[b], alone), key
    assert float((many[0].float() - many[1][:1].float()).abs().max()) > 0


def test_tile_shape_does_not_change_the_bits(eng):
    """257 x 130 outputs per mesh are 3 x 2 tiles of 128 x 128: 43 meshes make 258 of them, enough for the large tile; one mesh alone takes
    64 x 64 tiles.  The same rows give the same bits, in fp32 and fp16 output, with and without the epilogue."""
    Bn, N, Co, widths = 43, 257, 130, (33, 51, 16)
    assert -(-Co // 128) * -(-N // 128) * Bn >= 256 > -(-Co // 128) * -(-N // 128)
    srcs = [dev(rnd(80 + i, Bn, N, w, dtype=(F16, F32, F32)[i])) for i, w in enumerate(widths)]
    W, b, r = dev(rnd(84, Co, sum(widths), scale=0.1, dtype=F16)), dev(rnd(85, Co, dtype=F16)), dev(rnd(86, Bn, N, Co))
    nv = np.full(Bn, N, np.int32)
    nv[7], nv[42] = 130, 1
    for kw in (dict(), dict(bias=b, resid=r, relu=True), dict(bias=b, out_dtype=torch.float16)):
        big = eng.dnet_linear_f16(srcs, W, n_verts=nv, **kw)
        for m in (0, 7, 42):
            n = int(nv[m])
            one = {k: (v[m:m + 1, :n].contiguous() if k == "resid" else v) for k, v in kw.items()}
            small = eng.dnet_linear_f16([s[m:m + 1, :n].contiguous() for s in srcs], W, **one)
            assert same_bits(big[m:m + 1, :n], small), (m, list(kw))
            assert bool((big[m, n:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 5. placement
def hostile(a, n_real, pad):
    """rows >= n_real[b] of a (B, n, ...) operand replaced by the fill"""
    a = a.copy()
    for b, n in enumerate(n_real):
        a[b, n:] = pl.INT_FILL if a.dtype.kind == "i" else pl.fill_value(torch.float32, pad)
    return a


# R: the padded row count.  4099 rows are 2 x 129 row tiles of 32: the gradient features then take their resident decomposition
@pytest.mark.parametrize("pad,off,R", [("nan", 1, 163), ("+inf", 2, 163), ("-inf", 3, 163), ("nan", 3, 4099)])
def test_placement_of_every_operand(eng, pad, off, R):
    p = packed("t", "f")
    n_real, n = [160, 76], 160                                  # mesh 1 is cut to 76 of its 81 rows: rows 76.. are padding too
    Cw, Co, K = 32, 48, 16
    cpu = lambda t: t.cpu().numpy()
    rl, cols, gx, gy = cpu(p.row_len), cpu(p.cols), cpu(p.gx), cpu(p.gy)
    cols[1][cols[1] >= 76] = 0                                  # (a cut mesh keeps no column outside itself)
    evals = cpu(p.evals)
    eh, mh, e1, e2 = p.half_operands()
    eh, mh = cpu(eh), cpu(mh)
    x, x2, res = rnd(60, 2, n, Cw, scale=0.1), rnd(61, 2, n, 19, dtype=F16), rnd(62, 2, n, Co)
    W, bias, times = rnd(63, Co, Cw + 19, scale=0.1, dtype=F16), rnd(64, Co, dtype=F16), diffuse_operands(4, 4, Cw)[4].astype(F16)
    A_re, A_im = rnd(65, Cw, Cw, scale=0.2, dtype=F16), rnd(66, Cw, Cw, scale=0.2, dtype=F16)
    nv = dev(np.asarray(n_real, np.int32))

    def pad_rows(a, fill=0):
        out = np.full((a.shape[0], R) + a.shape[2:], fill, a.dtype)
        out[:, :n] = a
        return out
    # ---- control: aligned, dense, benign padding
    ctl = dict(x=pad_rows(x), x2=pad_rows(x2), res=pad_rows(res), eh=pad_rows(eh), mh=pad_rows(mh), rl=pad_rows(rl, 1),
               cols=pad_rows(cols), gx=pad_rows(gx), gy=pad_rows(gy))
    d = {k: dev(v) for k, v in ctl.items()}
    lin_kw = dict(relu=True, n_verts=nv)
    want = (eng.dnet_linear_f16([d["x"], d["x2"]], dev(W), dev(bias), d["res"], **lin_kw),
            eng.dnet_linear_f16([d["x"], d["x2"]], dev(W), dev(bias), d["res"], out_dtype=torch.float16, **lin_kw),
            eng.dnet_diffuse_f16(d["x"], d["eh"], d["mh"], e1, e2, dev(evals), dev(times), n_verts=nv),
            eng.dnet_gradient_features_f16(d["x"], d["rl"], d["cols"], d["gx"], d["gy"], dev(A_re), dev(A_im), n_verts=nv))
    # ---- hostile: every operand off the 16-byte grid, ld > width, the fill in padding columns, rows >= n_verts, slots >= row_len
    slot = np.arange(cols.shape[2])[None, None, :] >= rl[:, :, None]
    hc, hx, hy = cols.copy(), gx.copy(), gy.copy()
    hc[slot], hx[slot], hy[slot] = pl.INT_FILL, pl.fill_value(torch.float32, pad), pl.fill_value(torch.float32, pad)

    def mat(a, width_pad=5):
        """(B, n, W) -> the view (B, R, W) of a placed (B, R, W + 5) buffer"""
        v = pl.place(hostile(a, n_real, pad), offset_elems=off, ld=a.shape[-1] + width_pad, rows=R, pad=None if a.dtype.kind == "i" else pad, device=DEV)
        return v[..., :a.shape[-1]]

    def vec(a):
        return pl.place(hostile(a, n_real, pad), offset_elems=off, ld=R, pad=None if a.dtype.kind == "i" else pad, device=DEV)

    def flat(a, ld=None):
        return pl.place(a, offset_elems=off, ld=ld, pad=pad, device=DEV)[..., :a.shape[-1]]
    hx_, hx2_, hres_ = mat(x), mat(x2), mat(res)
    heh, hmh, hrl = mat(eh, 3), mat(mh, 7), vec(rl)
    hcols, hgx, hgy = mat(hc, 0), mat(hx, 0), mat(hy, 0)
    outs = [pl.place(np.zeros((2, R, c), t), offset_elems=off, ld=c + 3, pad=pad, device=DEV) for c, t in ((Co, F32), (Co, F16), (Cw, F32), (Cw, F32))]
    assert all(pl.mod16(t) != 0 for t in (hx_, hx2_, hres_, heh, hmh, hrl, hcols, hgx, hgy, *outs))
    hW, hA, hAi = flat(W, W.shape[1] + 7), flat(A_re, Cw + 1), flat(A_im, Cw + 1)
    hb, ht = flat(bias), flat(times)
    hnv = pl.place(np.asarray(n_real, np.int32), offset_elems=off, device=DEV)
    he1, he2 = (pl.place(cpu(e), offset_elems=off, device=DEV) for e in (e1, e2))
    with pl.PointerRecorder(eng.lib, "dm_dnet_linear_f16") as rec:
        eng.dnet_linear_f16([hx_, hx2_], hW, hb, hres_, relu=True, n_verts=hnv, out=outs[0][..., :Co])
        eng.dnet_linear_f16([hx_, hx2_], hW, hb, hres_, relu=True, n_verts=hnv, out=outs[1][..., :Co])
    assert rec.saw(hx_, hx2_, hres_, hW, hb, hnv, outs[0], outs[1])
    with pl.PointerRecorder(eng.lib, "dm_dnet_diffuse_f16") as rec:
        eng.dnet_diffuse_f16(hx_, heh, hmh, he1, he2, flat(evals), ht, n_verts=hnv, out=outs[2][..., :Cw])
    assert rec.saw(hx_, heh, hmh, he1, he2, ht, hnv, outs[2])
    with pl.PointerRecorder(eng.lib, "dm_dnet_gradfeat_f16") as rec:
        eng.dnet_gradient_features_f16(hx_, hrl, hcols, hgx, hgy, hA, hAi, n_verts=hnv, out=outs[3][..., :Cw])
    assert rec.saw(hx_, hrl, hcols, hgx, hgy, hA, hAi, hnv, outs[3])
    for name, w, o, c in zip(("linear", "linear fp16 out", "diffuse", "gradfeat"), want, outs, (Co, Co, Cw, Cw)):
        fill_bits = pl.bits(torch.full((1,), pl.fill_value(o.dtype, pad), dtype=o.dtype, device=DEV))
        assert same_bits(o[..., :c].contiguous(), w), (name, pad, off)
        assert bool((pl.bits(o[..., c:]) == fill_bits).all()), (name, "a padding column of the output was written")
        assert bool(torch.isfinite(w).all()) and bool((w[0, n_real[0]:] == 0).all()) and bool((w[1, n_real[1]:] == 0).all())
        assert float(w[1, :n_real[1]].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 6. whole network
def seeded(width, blocks, seed):
    torch.manual_seed(seed)
    net = layers.DiffusionNet(C_in=24, C_out=16, C_width=width, N_block=blocks).eval()
    for b in net.blocks:
        b.diffusion.diffusion_time.copy_(0.05 * torch.rand(width))
    x = torch.randn((160, 24))
    _, mass, _, evals, evecs, gX, gY = lc.operators("t")
    cfg = dict(N_block=blocks, with_gradient_features=True, with_gradient_rotations=True, outputs_at="vertices", last_activation=None)
    return net, cfg, x, dict(mass=mass, evals=evals, evecs=evecs, gradX=gX, gradY=gY)


def fixture_case(case):
    x, kw = lc.call_arguments(case)
    return lc.network(case), lc.config(case), x, kw


NETWORKS = [("w128", lambda: seeded(128, 4, 1)), ("w256", lambda: seeded(256, 8, 2))] + [(c, functools.partial(fixture_case, c)) for c in lc.CASES]


@pytest.mark.parametrize("name,make", NETWORKS, ids=[c[0] for c in NETWORKS])
def test_whole_network_is_no_worse_than_the_autocast_route(eng, name, make):
    """The acceptance.  Reference: the float64 network (dnet_layers_restate.forward) on the half-rounded parameters.  Against it the RMS
    error of route="device" must not exceed that of the halved module on route="torch" under torch.autocast("cuda"), as the reference's
    driver runs it -- for the engine's fp32 output (through the module's tail) and for the module's fp16 output.  Both routes run under
    the same autocast context.  Measured on an MI355X: DESIGN.md section 4, 'DiffusionNet forward, fp16'."""
    net, cfg, x, kw = make()
    dense = lambda t: None if t is None else t.to_dense().double().numpy()
    params = hs.half_params({k: v.detach().numpy() for k, v in net.state_dict().items()})
    exact, _ = rs.forward(cfg, params, x.double().numpy(), kw["mass"].numpy(), kw["evals"].numpy(), kw["evecs"].numpy(), dense(kw.get("gradX")),
                          dense(kw.get("gradY")), None if kw.get("faces") is None else kw["faces"].numpy())
    half = copy.deepcopy(net).half().to(DEV)
    xd, kwd = x.to(DEV), {k: v.to(DEV) for k, v in kw.items()}
    with torch.autocast("cuda"):
        y_torch = copy.deepcopy(half)(xd, route="torch", **kwd)
        y_dev = half(xd, route="device", **kwd)
        assert half.last_route == "device" and y_dev.dtype == y_torch.dtype and y_dev.shape == y_torch.shape
        flat = xd.dim() == 2
        up = lambda t: None if t is None else (t.unsqueeze(0) if flat else t)
        if flat:
            ops = [(None, kwd["mass"], None, kwd["evals"], kwd["evecs"], kwd.get("gradX"), kwd.get("gradY"))]
        else:                                                   # the fixture's batched cases carry no gradient operators
            ops = [(None, kwd["mass"][b], None, kwd["evals"][b], kwd["evecs"][b], None, None) for b in range(xd.shape[0])]
        raw = eng.diffusion_net_forward(half.device_weights(), layers.pack_operators(ops, device=DEV), up(xd), out_dtype=torch.float32)
        assert raw.dtype == torch.float32
        y32 = half._tail(raw, up(kwd["mass"]), None, up(kwd.get("faces")))
        y32 = y32.squeeze(0) if flat else y32
    e_torch, e_dev, e_32 = (hs.rms(y.double().cpu().numpy(), exact) for y in (y_torch, y_dev, y32))
    print(f"{name}: rms error against the float64 network: torch route under autocast {e_torch:.3e}; device route {e_dev:.3e} (ratio {e_dev / e_torch:.3f}); "
          f"device route, fp32 output {e_32:.3e} (ratio {e_32 / e_torch:.3f})")
    assert all(bool(torch.isfinite(y).all()) for y in (y_torch, y_dev, y32))
    assert e_32 <= e_torch, (name, "fp32 output", e_32, e_torch)
    assert e_dev <= e_torch, (name, "fp16 output", e_dev, e_torch)


# ---------------------------------------------------------------------------------------------------------------- 7. drop-in
def test_tuple_input_equals_the_concatenated_input(eng):
    net = lc.network("a", DEV).half()
    x, kw = lc.call_arguments("a", DEV)
    whole = net(x, route="device", **kw)
    assert whole.dtype == torch.float16 and net.last_route == "device"
    parts = (x[:, :12].contiguous(), x[:, 12:16].contiguous(), x[:, 16:].contiguous())
    assert same_bits(net(parts, route="device", **kw), whole)
    assert same_bits(net((x[:, :12], x[:, 12:]), route="device", **kw), whole)       # column slices are read where they lie
    # a source given as float16 is what the float32 source is rounded to
    xh = x.to(torch.float16)
    assert same_bits(net((xh[:, :12], x[:, 12:]), route="device", **kw), net((xh[:, :12].float(), x[:, 12:]), route="device", **kw))
    assert same_bits(net(xh, route="device", **kw), whole)
    # the weights go to the library where they lie
    with pl.PointerRecorder(eng.lib, "dm_dnet_linear_f16") as rec:
        net(x, route="device", **kw)
    assert rec.saw(net.first_lin.weight, net.first_lin.bias, net.last_lin.weight, net.blocks[0].mlp[0].weight)
    with torch.autocast("cuda"):                                # (the torch route of a halved module needs it for float32 input)
        auto = net(x, route="auto", **kw)
    assert auto.dtype == torch.float16 and net.last_route == ("device" if layers.AUTO_DEVICE["single_half"] else "torch")


def test_halved_featurizer_takes_the_device_route():
    model, _ = lk.featurizer(DEV)
    model = model.half()
    mesh, ops, cams, fts, p2f = lk.featurizer_inputs(DEV)
    unit, raw, lifted = model(None, mesh, ops, cams, return_mvfeatures=True, fts=fts.half(), route="device")
    assert model.extractor_3d.last_route == "device"
    assert unit.dtype == torch.float16 and raw.dtype == torch.float16 and unit.shape == raw.shape
    norms = unit.float().norm(dim=-1)
    print(f"halved featurizer: row norms in [{float(norms.min()):.5f}, {float(norms.max()):.5f}], lifted {lifted.dtype}")
    assert bool(torch.isfinite(unit).all()) and float((norms - 1).abs().max()) <= 2.0 ** -9      # fp16 unit rows: 2^-11 per entry and the norm's own
    p = layers.pack_operators([ops], device=DEV)
    many = model.forward_many([None], [mesh], p, [cams], fts_list=[fts.half()])
    assert same_bits(many[0], unit)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_module_refusals_name_the_condition(eng):
    net = lc.network("a", DEV).half()
    x, kw = lc.call_arguments("a", DEV)
    want = net(x, route="device", **kw)
    mixed = copy.deepcopy(net)
    mixed.last_lin.float()
    with pytest.raises(RuntimeError, match="all float32 or all float16"):
        mixed(x, route="device", **kw)
    with pytest.raises(RuntimeError, match="bfloat16"):
        copy.deepcopy(net).bfloat16()(x, route="device", **kw)
    with pytest.raises(RuntimeError, match="float16 or float32"):
        net(x.to(torch.bfloat16), route="device", **kw)
    with pytest.raises(RuntimeError, match="float32"):
        lc.network("a", DEV)(x.half(), route="device", **kw)
    train = copy.deepcopy(net).train()
    assert train.dropout
    with pytest.raises(RuntimeError, match="eval mode"):
        train(x, route="device", **kw)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="requires grad"):
        net(x, route="device", **kw)
    with pytest.raises(ValueError, match="out_dtype"):
        eng.diffusion_net_forward(lc.network("a", DEV).device_weights(), packed("t"), x[None], out_dtype=torch.float16)
    assert same_bits(net(x, route="device", **kw), want)


def test_entry_refusals_leave_the_engine_usable(eng):
    N, Cw, K, nnz = 8, 4, 3, 2
    x, out = dev(rnd(70, 1, N, Cw)), torch.empty((1, N, Cw), device=DEV)
    W = dev(rnd(71, Cw, Cw, dtype=F16))
    eh, evals, times = dev(rnd(72, 1, N, K, dtype=F16)), torch.ones((1, K), device=DEV), torch.ones(Cw, device=DEV)
    e = torch.zeros(1, dtype=torch.int32, device=DEV)
    rl = torch.ones((1, N), dtype=torch.int32, device=DEV)
    cols, g = torch.zeros((1, N, nnz), dtype=torch.int32, device=DEV), torch.zeros((1, N, nnz), device=DEV)
    P, null = (lambda t: C.c_void_p(t.data_ptr())), C.c_void_p(0)
    H, S = _lib.DM_F16, _lib.DM_F32

    def linear(B=1, N=N, Co=Cw, w=Cw, ld=Cw, ldw=Cw, ldo=Cw, ldr=0, nsrc=1, res=null, dt=S, bdt=S, odt=S, Wp=None, act=0):
        return eng.lib.dm_dnet_linear_f16(eng.ctx, B, N, Co, nsrc, P(x), w, ld, dt, null, 0, 0, S, null, 0, 0, S, P(W) if Wp is None else Wp, ldw, P(x), bdt, res, ldr, act,
                                          null, odt, P(out), ldo)

    def diffuse(B=1, N=N, K=K, Cw=Cw, ldx=Cw, lde=K, ldm=K, ldo=Cw, tdt=S, ep=None):
        return eng.lib.dm_dnet_diffuse_f16(eng.ctx, B, N, K, Cw, P(x), ldx, P(eh), lde, P(eh), ldm, P(e) if ep is None else ep, P(e), P(evals), P(times), tdt, null, P(out), ldo)

    def gradfeat(B=1, N=N, Cw=Cw, nnz=nnz, ldx=Cw, lda=Cw, ldo=Cw, Ap=None):
        return eng.lib.dm_dnet_gradfeat_f16(eng.ctx, B, N, Cw, nnz, P(rl), P(cols), P(g), P(g), P(x), ldx, P(W) if Ap is None else Ap, null, lda, null, P(out), ldo)
    odd = C.c_void_p(W.data_ptr() + 1)
    bad = [("linear", linear, kw) for kw in (dict(B=0), dict(N=0), dict(Co=0), dict(w=0), dict(N=-1), dict(ld=Cw - 1), dict(ldw=Cw - 1), dict(ldo=Cw - 1),
                                             dict(res=P(out), ldr=Cw - 1), dict(nsrc=0), dict(nsrc=4), dict(dt=2), dict(bdt=7), dict(odt=-1), dict(Wp=odd),
                                             dict(act=2))]
    bad += [("diffuse", diffuse, kw) for kw in (dict(B=0), dict(N=0), dict(K=0), dict(K=1025, lde=1025, ldm=1025), dict(Cw=0), dict(ldx=Cw - 1), dict(lde=K - 1),
                                                dict(ldm=K - 1), dict(ldo=Cw - 1), dict(tdt=3), dict(ep=null))]
    bad += [("gradfeat", gradfeat, kw) for kw in (dict(B=0), dict(N=0), dict(Cw=0), dict(nnz=0), dict(ldx=Cw - 1), dict(lda=Cw - 1), dict(ldo=Cw - 1), dict(Ap=odd))]
    for name, fn, kw in bad:
        rc = fn(**kw)
        assert rc == _lib.DM_EINVAL, (name, kw, rc)
        with pytest.raises(ValueError):
            eng._chk(rc)
    for counts in ([0], [N + 1], [-3]):
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_linear_f16(x, W, n_verts=counts)
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_diffuse_f16(x, eh, eh, e, e, evals, times, n_verts=counts)
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_gradient_features_f16(x, rl, cols, g, g, W, n_verts=counts)
    with pytest.raises(ValueError, match="float32 or float16"):
        eng.dnet_linear_f16(x, W, out_dtype=torch.bfloat16)
    assert linear() == 0 and diffuse() == 0 and gradfeat() == 0
    xs, Ws = x[0].cpu().numpy(), W.cpu().numpy()
    within(eng.dnet_linear_f16(x, W)[0], hs.linear([xs], Ws), hs.linear_bound([xs], Ws), "linear_f16 after the refusals")

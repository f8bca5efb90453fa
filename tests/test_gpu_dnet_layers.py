"""The DiffusionNet forward kernels on the GPU (dm_dnet_linear_f32, dm_dnet_diffuse_f32, dm_dnet_gradfeat_f32) and the device route of
diffusion_net.layers: every kernel against its float64 restatement within the restatement's running-error bound
(tests/dnet_layers_restate.py), batches against single calls bit for bit, hostile operand placement, the whole network against the
reference's recorded float32 run, and the refusals.  Every figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dnet_checks as dc
import dnet_layers_checks as lc
import dnet_layers_restate as rs
import placement as pl
from densematcher_amd import _lib
from densematcher_amd.diffusion_net import layers

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


@pytest.fixture(autouse=True)
def inference():
    """the device route records no autograd graph: parameters require grad, so it runs under torch.no_grad()"""
    with torch.no_grad():
        yield


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


@pytest.mark.parametrize("N,Co,widths,opts", LINEAR)
def test_linear_against_the_restatement(eng, N, Co, widths, opts):
    bias, relu, resid = opts
    srcs = [rnd(10 + i, N, w) for i, w in enumerate(widths)]
    W = rnd(20, Co, sum(widths), scale=sum(widths) ** -0.5)
    b = rnd(21, Co) if bias else None
    r = rnd(22, N, Co) if resid else None
    got = eng.dnet_linear([dev(s) for s in srcs], dev(W), None if b is None else dev(b), None if r is None else dev(r), relu=relu)
    assert got.shape == (N, Co)
    within(got, rs.linear(srcs, W, b, r, relu), rs.linear_bound(srcs, W, b, r), f"linear N={N} C_out={Co} widths={widths} {opts}")


# ---------------------------------------------------------------------------------------------------------------- 2. diffuse
def diffuse_operands(N, K, Cw, seed=0):
    g = np.random.default_rng(seed)
    x, evecs = rnd(seed + 1, N, Cw), rnd(seed + 2, N, K, scale=0.3)
    mass = (0.002 + 0.01 * g.random(N)).astype(np.float32)
    evals = np.sort(40.0 * g.random(K)).astype(np.float32)
    times = (0.05 * g.random(Cw)).astype(np.float32)
    times[0] = 0.0
    if Cw > 1:
        times[1] = -0.01
    return x, mass, evals, evecs, times


@pytest.mark.parametrize("N,K,Cw", [(1, 1, 1), (81, 16, 48), (257, 128, 130), (160, 16, 32)])
def test_diffuse_against_the_restatement(eng, N, K, Cw):
    x, mass, evals, evecs, times = diffuse_operands(N, K, Cw)
    got = eng.dnet_diffuse(dev(x)[None], dev(mass)[None], dev(evals)[None], dev(evecs)[None], dev(times))[0]
    within(got, rs.diffuse(x, mass, evals, evecs, times), rs.diffuse_bound(x, mass, evals, evecs, times), f"diffuse N={N} K={K} C={Cw}")


# ---------------------------------------------------------------------------------------------------------------- 3. gradient features
@functools.lru_cache(maxsize=None)
def packed(*keys):
    return layers.pack_operators([lc.operators(k) for k in keys]).to(DEV)


def gradfeat_case(eng, p, b, Cw, rot, tag):
    n = p.n_verts[b]
    x = rnd(31, n, Cw, scale=0.1)
    A_re, A_im = rnd(32, Cw, Cw, scale=Cw ** -0.5), (rnd(33, Cw, Cw, scale=Cw ** -0.5) if rot else None)
    sl = lambda t: t[b:b + 1, :n].contiguous()
    got = eng.dnet_gradient_features(dev(x)[None], sl(p.row_len), sl(p.cols), sl(p.gx), sl(p.gy), dev(A_re), None if A_im is None else dev(A_im))[0]
    Gx, Gy = p.dense_grad(b, "gx").cpu().numpy(), p.dense_grad(b, "gy").cpu().numpy()
    ref, dots = rs.gradfeat(x, Gx, Gy, A_re, A_im)
    share = float((np.abs(dots) < 2).mean())
    print(f"{tag}: |dots| < 2 at {share:.3f} of the entries, largest {np.abs(dots).max():.3f}")
    assert share >= 0.5                                        # a saturated tanh would hide the gradient path
    within(got, ref, rs.gradfeat_bound(x, Gx, Gy, A_re, A_im), tag)
    return got


@pytest.mark.parametrize("key", ["f", "t"])
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("Cw", [32, 48])
def test_gradfeat_against_the_restatement(eng, key, rot, Cw):
    p = packed(key)
    if key == "f":
        assert int(p.row_len.min()) == 4 and int(p.row_len.max()) == 41
    gradfeat_case(eng, p, 0, Cw, rot, f"gradfeat mesh {key} C={Cw} rotations={rot}")


@pytest.mark.parametrize("width", [41, 64, 65, 90])
def test_gradfeat_row_width_does_not_change_the_bits(eng, width):
    """rows up to 64 slots wide are kept in LDS by the kernel, wider ones are read from global memory: the same chain either way.  Mesh f
    (longest row 41) at its own width, at the threshold and beyond it, the extra slots hostile"""
    p = packed("f")
    n, w0, Cw = p.n_verts[0], p.cols.shape[2], 48
    x, A_re, A_im = dev(rnd(34, 1, n, Cw, scale=0.1)), dev(rnd(35, Cw, Cw, scale=0.15)), dev(rnd(36, Cw, Cw, scale=0.15))
    want = eng.dnet_gradient_features(x, p.row_len, p.cols, p.gx, p.gy, A_re, A_im)
    cols = torch.full((1, n, width), pl.INT_FILL, dtype=torch.int32, device=DEV)
    gx = torch.full((1, n, width), float("nan"), device=DEV)
    gy = gx.clone()
    keep = (torch.arange(w0, device=DEV)[None, None, :] < p.row_len[:, :, None])
    cols[..., :w0][keep], gx[..., :w0][keep], gy[..., :w0][keep] = p.cols[keep], p.gx[keep], p.gy[keep]
    got = eng.dnet_gradient_features(x, p.row_len, cols, gx, gy, A_re, A_im)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_gradfeat_unreferenced_vertex(eng):
    fx = dc.golden()
    n = fx["verts_u"].shape[0]
    sp = lambda name: torch.sparse_coo_tensor(torch.from_numpy(np.stack((fx[f"{name}_row_u"], fx[f"{name}_col_u"])).astype(np.int64)),
                                              torch.from_numpy(fx[f"{name}_val_u"].astype(np.float32)), (n, n)).coalesce()
    op = (None, torch.ones(n), None, torch.zeros(1), torch.zeros((n, 1)), sp("gradX"), sp("gradY"))
    p = layers.pack_operators([op]).to(DEV)
    assert int(p.row_len[0, n - 1]) == 1 and int(p.cols[0, n - 1, 0]) == n - 1 and float(p.gx[0, n - 1, 0]) == 0.0
    got = gradfeat_case(eng, p, 0, 32, True, "gradfeat mesh u")
    assert bool((got[n - 1] == 0).all())                       # tanh(0)


# ---------------------------------------------------------------------------------------------------------------- 4. batches
def test_ragged_batch_equals_the_single_calls(eng):
    keys = ("t", "r", "f")
    p = packed(*keys)
    Bn, N, Cw = 3, p.mass.shape[1], 32
    assert p.n_verts == [160, 96, 81] and p.n_verts_dev is not None
    x = torch.full((Bn, N, Cw), float("nan"), device=DEV)
    for b, n in enumerate(p.n_verts):
        x[b, :n] = dev(rnd(40 + b, n, Cw, scale=0.1))
    W, bias, times = dev(rnd(44, 48, 2 * Cw, scale=0.1)), dev(rnd(45, 48)), dev(diffuse_operands(4, 4, Cw)[4])
    A_re, A_im = dev(rnd(46, Cw, Cw, scale=0.2)), dev(rnd(47, Cw, Cw, scale=0.2))
    nv = p.n_verts_dev
    lin = eng.dnet_linear([x, x], W, bias, relu=True, n_verts=nv)
    dif = eng.dnet_diffuse(x, p.mass, p.evals, p.evecs, times, n_verts=nv)
    grd = eng.dnet_gradient_features(x, p.row_len, p.cols, p.gx, p.gy, A_re, A_im, n_verts=nv)
    for b, (key, n) in enumerate(zip(keys, p.n_verts)):
        one = packed(key)
        xb = x[b:b + 1, :n].contiguous()
        assert torch.equal(lin[b, :n], eng.dnet_linear([xb, xb], W, bias, relu=True)[0]), key
        assert torch.equal(dif[b, :n], eng.dnet_diffuse(xb, one.mass, one.evals, one.evecs, times)[0]), key
        assert torch.equal(grd[b, :n], eng.dnet_gradient_features(xb, one.row_len, one.cols, one.gx, one.gy, A_re, A_im)[0]), key
        for out in (lin, dif, grd):
            assert bool(torch.isfinite(out[b, :n]).all()) and bool((out[b, n:] == 0).all()), key
    net = lc.network("a", DEV)
    xs = [dev(rnd(50 + b, n, 19)) for b, n in enumerate(p.n_verts)]
    many = net.forward_many(xs, p)
    assert net.last_route == "device" and [tuple(y.shape) for y in many] == [(n, 24) for n in p.n_verts]
    for b, key in enumerate(keys):
        alone = net(xs[b], route="device", operators=packed(key))
        assert torch.equal(many[b], alone), key
    assert float((many[0] - many[1][:1]).abs().max()) > 0


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
    mass, evals, evecs = cpu(p.mass), cpu(p.evals), cpu(p.evecs)
    x, x2, res = rnd(60, 2, n, Cw, scale=0.1), rnd(61, 2, n, 19), rnd(62, 2, n, Co)
    W, bias, times = rnd(63, Co, Cw + 19, scale=0.1), rnd(64, Co), diffuse_operands(4, 4, Cw)[4]
    A_re, A_im = rnd(65, Cw, Cw, scale=0.2), rnd(66, Cw, Cw, scale=0.2)
    nv = dev(np.asarray(n_real, np.int32))

    def pad_rows(a, fill=0):
        out = np.full((a.shape[0], R) + a.shape[2:], fill, a.dtype)
        out[:, :n] = a
        return out
    # ---- control: aligned, dense, benign padding
    ctl = dict(x=pad_rows(x), x2=pad_rows(x2), res=pad_rows(res), mass=pad_rows(mass, 1), evecs=pad_rows(evecs), rl=pad_rows(rl, 1),
               cols=pad_rows(cols), gx=pad_rows(gx), gy=pad_rows(gy))
    d = {k: dev(v) for k, v in ctl.items()}
    want = (eng.dnet_linear([d["x"], d["x2"]], dev(W), dev(bias), d["res"], relu=True, n_verts=nv),
            eng.dnet_diffuse(d["x"], d["mass"], dev(evals), d["evecs"], dev(times), n_verts=nv),
            eng.dnet_gradient_features(d["x"], d["rl"], d["cols"], d["gx"], d["gy"], dev(A_re), dev(A_im), n_verts=nv))
    # ---- hostile: every operand off the 16-byte grid, ld > width, the fill in padding columns, rows >= n_verts, slots >= row_len
    slot = np.arange(cols.shape[2])[None, None, :] >= rl[:, :, None]
    hc, hx, hy = cols.copy(), gx.copy(), gy.copy()
    hc[slot], hx[slot], hy[slot] = pl.INT_FILL, pl.fill_value(torch.float32, pad), pl.fill_value(torch.float32, pad)

    def mat(a, width_pad=5):
        """(B, n, W) -> the view (B, R, W) of a placed (B, R, W + 5) buffer"""
        v = pl.place(hostile(a, n_real, pad), offset_elems=off, ld=a.shape[-1] + width_pad, rows=R, pad=None if a.dtype.kind == "i" else pad, device=DEV)
        return v[..., :a.shape[-1]]

    def vec(a):
        """(B, n) -> (B, R) with the fill behind n_verts"""
        return pl.place(hostile(a, n_real, pad), offset_elems=off, ld=R, pad=None if a.dtype.kind == "i" else pad, device=DEV)

    def flat(a, ld=None):
        return pl.place(a, offset_elems=off, ld=ld, pad=pad, device=DEV)[..., :a.shape[-1]]
    hx_, hx2_, hres_ = mat(x), mat(x2), mat(res)
    hm, he, hrl = vec(mass), mat(evecs), vec(rl)
    hcols, hgx, hgy = mat(hc, 0), mat(hx, 0), mat(hy, 0)
    outs = [pl.place(np.zeros((2, R, c), np.float32), offset_elems=off, ld=c + 3, pad=pad, device=DEV) for c in (Co, Cw, Cw)]
    assert all(pl.mod16(t) != 0 for t in (hx_, hx2_, hres_, hm, he, hrl, hcols, hgx, hgy, outs[0]))
    hW, hA, hAi = flat(W, W.shape[1] + 7), flat(A_re, Cw + 1), flat(A_im, Cw + 1)
    hnv = pl.place(np.asarray(n_real, np.int32), offset_elems=off, device=DEV)
    with pl.PointerRecorder(eng.lib, "dm_dnet_linear_f32") as rec:
        eng.dnet_linear([hx_, hx2_], hW, flat(bias), hres_, relu=True, n_verts=hnv, out=outs[0][..., :Co])
    assert rec.saw(hx_, hx2_, hres_, hW, hnv, outs[0])
    with pl.PointerRecorder(eng.lib, "dm_dnet_diffuse_f32") as rec:
        eng.dnet_diffuse(hx_, hm, flat(evals), he, flat(times), n_verts=hnv, out=outs[1][..., :Cw])
    assert rec.saw(hx_, hm, he, hnv, outs[1])
    with pl.PointerRecorder(eng.lib, "dm_dnet_gradfeat_f32") as rec:
        eng.dnet_gradient_features(hx_, hrl, hcols, hgx, hgy, hA, hAi, n_verts=hnv, out=outs[2][..., :Cw])
    assert rec.saw(hx_, hrl, hcols, hgx, hgy, hA, hAi, hnv, outs[2])
    fill_bits = pl.bits(torch.full((1,), pl.fill_value(torch.float32, pad), device=DEV))
    for name, w, o, c in zip(("linear", "diffuse", "gradfeat"), want, outs, (Co, Cw, Cw)):
        assert torch.equal(pl.bits(o[..., :c]), pl.bits(w)), (name, pad, off)
        assert bool((pl.bits(o[..., c:]) == fill_bits).all()), (name, "a padding column of the output was written")
        assert bool(torch.isfinite(w).all()) and bool((w[0, n_real[0]:] == 0).all()) and bool((w[1, n_real[1]:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 6. whole network
@pytest.mark.parametrize("case", lc.CASES)
def test_whole_network_against_the_reference_float32_run(case):
    """measured on an MI355X (max |got - ref| / max |ref|): recorded in DESIGN.md section 4, 'DiffusionNet forward'"""
    net = lc.network(case, DEV)
    x, kw = lc.call_arguments(case, DEV)
    y = net(x, route="device", **kw)
    assert net.last_route == "device" and y.dtype == torch.float32 and not y.requires_grad
    lc.check_output(case, y, "device route")
    for b in net.blocks:                                        # the times are left clamped, as the reference leaves them
        assert float(b.diffusion.diffusion_time.min()) == float(np.float32(1e-8))
    lc.check_output(case, net(x, route="torch", **kw), "torch route (GPU)")
    with torch.enable_grad(), pytest.raises(RuntimeError, match="requires grad"):
        net(x, route="device", **kw)


# ---------------------------------------------------------------------------------------------------------------- 7. tuple input
def test_tuple_input_equals_the_concatenated_input():
    net = lc.network("a", DEV)
    x, kw = lc.call_arguments("a", DEV)
    parts = (x[:, :12].contiguous(), x[:, 12:16].contiguous(), x[:, 16:].contiguous())
    whole = net(x, route="device", **kw)
    assert torch.equal(net(parts, route="device", **kw), whole)
    assert torch.equal(net((x[:, :12], x[:, 12:]), route="device", **kw), whole)       # column slices are read where they lie


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_engine_usable(eng):
    N, Cw, K, nnz = 8, 4, 3, 2
    x, W, out = dev(rnd(70, 1, N, Cw)), dev(rnd(71, Cw, Cw)), torch.empty((1, N, Cw), device=DEV)
    mass, evals, evecs, times = torch.ones((1, N), device=DEV), torch.ones((1, K), device=DEV), dev(rnd(72, 1, N, K)), torch.ones(Cw, device=DEV)
    rl = torch.ones((1, N), dtype=torch.int32, device=DEV)
    cols, g = torch.zeros((1, N, nnz), dtype=torch.int32, device=DEV), torch.zeros((1, N, nnz), device=DEV)
    P, null = (lambda t: C.c_void_p(t.data_ptr())), C.c_void_p(0)

    def linear(B=1, N=N, Co=Cw, w=Cw, ld=Cw, ldw=Cw, ldo=Cw, ldr=0, nsrc=1, res=null):
        return eng.lib.dm_dnet_linear_f32(eng.ctx, B, N, Co, nsrc, P(x), w, ld, null, 0, 0, null, 0, 0, P(W), ldw, null, res, ldr, 0, null, P(out), ldo)

    def diffuse(B=1, N=N, K=K, Cw=Cw, ldx=Cw, lde=K, ldo=Cw):
        return eng.lib.dm_dnet_diffuse_f32(eng.ctx, B, N, K, Cw, P(x), ldx, P(mass), P(evals), P(evecs), lde, P(times), null, P(out), ldo)

    def gradfeat(B=1, N=N, Cw=Cw, nnz=nnz, ldx=Cw, lda=Cw, ldo=Cw):
        return eng.lib.dm_dnet_gradfeat_f32(eng.ctx, B, N, Cw, nnz, P(rl), P(cols), P(g), P(g), P(x), ldx, P(W), null, lda, null, P(out), ldo)
    bad = [("linear", linear, kw) for kw in (dict(B=0), dict(N=0), dict(Co=0), dict(w=0), dict(N=-1), dict(ld=Cw - 1), dict(ldw=Cw - 1), dict(ldo=Cw - 1),
                                             dict(res=P(out), ldr=Cw - 1), dict(nsrc=0), dict(nsrc=4))]
    bad += [("diffuse", diffuse, kw) for kw in (dict(B=0), dict(N=0), dict(K=0), dict(Cw=0), dict(ldx=Cw - 1), dict(lde=K - 1), dict(ldo=Cw - 1))]
    bad += [("gradfeat", gradfeat, kw) for kw in (dict(B=0), dict(N=0), dict(Cw=0), dict(nnz=0), dict(ldx=Cw - 1), dict(lda=Cw - 1), dict(ldo=Cw - 1))]
    for name, fn, kw in bad:
        rc = fn(**kw)
        assert rc == _lib.DM_EINVAL, (name, kw, rc)
        with pytest.raises(ValueError):
            eng._chk(rc)
    for counts in ([0], [N + 1], [-3]):
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_linear(x, W, n_verts=counts)
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_diffuse(x, mass, evals, evecs, times, n_verts=counts)
        with pytest.raises(ValueError, match="n_verts"):
            eng.dnet_gradient_features(x, rl, cols, g, g, W, n_verts=counts)
    assert linear() == 0 and diffuse() == 0 and gradfeat() == 0
    xs, Ws = x[0].cpu().numpy(), W.cpu().numpy()
    within(eng.dnet_linear(x, W)[0], rs.linear([xs], Ws), rs.linear_bound([xs], Ws), "linear after the refusals")

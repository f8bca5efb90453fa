"""GPU: shape difference operators on the device (dm_shape_diff_f64, dm_pullback_forms_f64, MatchEngine.shape_difference /
pullback_forms, the device route of pyFM.spectral.shape_difference) against the reference's arrays in tests/golden/fx_sd.npz and
against the host route computed at test time.

Comparison rule -- a bound, not a measurement (tests/sd_restate.py; u = 2^-52, nnz the longest row of W), entrywise on |got - ref|:
    Ga                      (N2 + 2) u |X|^T diag(a2) |X|
    Gw                      (N2 + nnz + 2) u |X|^T |W| |X|
    SD_a from a given FM    (k2 + 2) u |FM|^T |FM|
    SD_c                    |inv1[i]| (the bound of its plain form) + u |ref| for the last multiplication
the standard error bounds of two summation orders of the same products, fused or not.  End to end, the 'spectral' route's map comes
from dm_p2p_to_fm_f64: its perturbation |dFM| <= (N2 + 2) u |Phi2|^T (a2 |X|) adds |FM|^T |dFM| + |dFM|^T |FM|.
Where inv1[0] is not cut (lambda_0 is noise that exceeds np.linalg.pinv's cut-off: the fixture at k1 = 5) the bound on row 0 of the
conformal operator is of order one and the check is VACUOUS there by construction: the reference's row is noise / lambda_0.  Where
it is cut, row 0 must be exactly 0.0, and the cut decision must be the host's.  Every figure is printed before it is asserted.
Equalities between two device calls (independence of the batch, placement, rows against CSR) are bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sparse
import torch

import sd_restate as sdr
from conftest import load_golden
from placement import PointerRecorder, place
from densematcher_amd import synth
from densematcher_amd.pyFM.spectral import shape_difference as sd

pytestmark = pytest.mark.gpu

SLAB, SLABS = sdr.SLAB, sdr.SLABS          # dm_shapediff.hip: PB_SLAB vertices per staged slab, PB_SLABS slabs per workgroup
CHUNK = SLAB * SLABS
DIMS = [(5, None), (12, None), (17, 8), (40, 40)]


def tag(k1, k2):
    return f"{k1}_{'N' if k2 is None else k2}"


class Mesh:
    """what compute_SD reads of a mesh"""
    def __init__(self, fx, q):
        n = fx[f"verts_{q}"].shape[0]
        self.vertlist, self.facelist = fx[f"verts_{q}"], fx[f"faces_{q}"]
        self.eigenvalues, self.eigenvectors = fx[f"lam_{q}"], fx[f"Phi_{q}"]
        self.A = sparse.diags(fx[f"mass_{q}"]).tocsr()
        self.W = sparse.coo_matrix((fx[f"W_val_{q}"], (fx[f"W_row_{q}"], fx[f"W_col_{q}"])), shape=(n, n)).tocsr()
        self.n_vertices = n


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    e = default_engine()
    yield e
    e.reset_options()


@pytest.fixture(scope="module")
def fx():
    return load_golden("fx_sd.npz")


@pytest.fixture(scope="module")
def pairs(fx):
    m = [Mesh(fx, q) for q in range(3)]
    return {"m": (m[0], m[1], fx["p2p"].astype(np.int64)), "i": (m[0], m[2], None)}


def host(t):
    return t.cpu().numpy()


def csr_in_row_order(cols, w, n):
    """the leading n x n block of ELL rows as CSR with the entries of a row IN THEIR STORED ORDER (zeros -- the padding -- left out)"""
    cols, w = cols[:n], w[:n]
    keep = (w != 0.0) & (cols >= 0) & (cols < n)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(1))])
    return sparse.csr_matrix((w[keep], cols[keep].astype(np.int32), indptr), shape=(n, n))


@pytest.fixture(scope="module")
def geo(eng):
    """grid (1200) and torus (2048) of fx_geod.npz: W and masses from the package's own device assembly (one ragged call), bases
    from synth.random_basis (lambda_0 = 0 exactly: a cut row); computed once, read-only"""
    g = load_golden("fx_geod.npz")
    names = ("grid", "torus")
    ell = eng.laplacian_ell([g[n + "_F"] for n in names], verts=[g[n + "_V"] for n in names])
    out = {}
    for b, name in enumerate(names):
        n = g[name + "_V"].shape[0]
        cols, w = ell["cols"][b, :n].contiguous(), ell["w"][b, :n].contiguous()
        lam, Phi, _ = synth.random_basis(n, 128, seed=31 + b)
        out[name] = dict(n=n, cols=cols, w=w, cols_h=host(cols), w_h=host(w), mass=host(ell["mass64"][b, :n]), lam=lam, Phi=Phi)
        for v in out[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def forms_case(eng, geo, src, tgt, n2, k1, p21, lam=True, rows=True, ld1=None):
    """one pair through pullback_forms (the target cut to its first n2 vertices with n_verts2) and its host reference"""
    s, t = geo[src], geo[tgt]
    Phi = s["Phi"] if ld1 is None else s["Phi"][:, :ld1]
    Wh = csr_in_row_order(t["cols_h"], t["w_h"], n2)
    W = [(t["cols"][:n2], t["w"][:n2])] if rows else [Wh]
    full = np.zeros(t["n"], np.int64)
    full[:n2] = p21
    got = eng.pullback_forms(full[None], np.ascontiguousarray(Phi)[None], W, t["mass"][None], k1, lam1=s["lam"][None] if lam else None,
                             n_verts2=None if n2 == t["n"] else [n2])
    X = s["Phi"][p21, :k1]
    ref = sdr.forms_ref(X, t["mass"][:n2], Wh, s["lam"] if lam else None)
    bounds = sdr.forms_bounds(X, t["mass"][:n2], Wh, s["lam"] if lam else None, ref[1])
    return got, ref, bounds


def check_forms(name, got, ref, bounds, lam=None, k1=None):
    sdr.report(name + " Ga", host(got[0][0]), ref[0], bounds[0])
    sdr.report(name + " Gw", host(got[1][0]), ref[1], bounds[1])
    if lam is not None:
        sdr.check_cut_rows(name, host(got[1][0]), lam, k1)


# ---------------------------------------------------------------- the reference's fixture, end to end on the device
@pytest.mark.parametrize("pn", ["m", "i"])
@pytest.mark.parametrize("SD_type", ["spectral", "semican"])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: tag(*d))
def test_fixture_on_the_device(eng, fx, pairs, pn, SD_type, dims):
    m1, m2, p2p = pairs[pn]
    k1, k2 = dims
    a, c = sd.compute_SD(m1, m2, k1=k1, k2=k2, p2p=p2p, SD_type=SD_type, device=True)
    assert a.is_cuda and c.is_cuda and a.shape == (k1, k1) and c.shape == (k1, k1)
    name = f"{pn} {SD_type} {tag(*dims)}"
    ra, rc = fx[f"{pn}_{SD_type}_{tag(*dims)}_a"], fx[f"{pn}_{SD_type}_{tag(*dims)}_c"]
    idx = np.arange(m2.n_vertices) if p2p is None else p2p
    X, mass2 = m1.eigenvectors[idx, :k1], np.asarray(m2.A.diagonal())
    if SD_type == "semican":
        ba, bc = sdr.forms_bounds(X, mass2, m2.W, m1.eigenvalues, rc)
    else:
        FM = fx[f"{pn}_FM_{tag(*dims)}"]
        dFM = sdr.fm_perturbation(X, m2.eigenvectors[:, :FM.shape[0]], mass2)
        ba, bc = sdr.sd_bounds(FM, m1.eigenvalues, m2.eigenvalues, rc, dFM)
    sdr.report(name + " SD_a", host(a), ra, ba)
    sdr.report(name + " SD_c", host(c), rc, bc)
    sdr.check_cut_rows(name, host(c), m1.eigenvalues, k1)
    if k1 == 12:
        assert not torch.any(c[0] != 0.0)
    # a GPU map alone selects the device route
    a2, c2 = sd.compute_SD(m1, m2, k1=k1, k2=k2, p2p=torch.as_tensor(idx).cuda(), SD_type=SD_type)
    assert torch.equal(a2, a) and torch.equal(c2, c)


# ---------------------------------------------------------------- dm_shape_diff_f64
def lam1_variants(rng, k1):
    """first entry exactly 0 (cut) / tiny and kept / a negative entry"""
    base = np.sort(rng.uniform(0.5, 4.0 * k1, k1))
    zero, tiny, neg = base.copy(), base.copy(), base.copy()
    zero[0] = 0.0
    tiny[0] = 1.5e-15 * base.max() if k1 > 1 else 1e-200
    neg[k1 // 2] = -neg[k1 // 2]
    neg[0] = -2e-15 * base.max() if k1 > 1 else -1.0
    return np.stack([zero, tiny, neg])


@pytest.mark.parametrize("k1", [1, 3, 16, 17, 64, 65, 256])
@pytest.mark.parametrize("k2m", ["one", "k1", "3k1"])
def test_shape_diff_seeded_maps(eng, k1, k2m):
    k2 = {"one": 1, "k1": k1, "3k1": min(3 * k1, 768)}[k2m]
    rng = np.random.default_rng(1000 * k1 + k2)
    lam1 = lam1_variants(rng, k1)
    lam2 = np.sort(rng.uniform(0.0, 4.0 * k2, (3, k2)), axis=1)
    FM = rng.standard_normal((3, k2, k1)) / np.sqrt(k2)
    ldf = k1 + 3
    padded = np.full((3, k2, ldf), np.nan)
    padded[:, :, :k1] = FM
    a, c = eng.shape_difference(padded, np.concatenate([lam1, np.full((3, 2), np.nan)], 1), lam2, k1=k1)
    a0, c0 = eng.shape_difference(FM, lam1, lam2)
    assert torch.equal(a, a0) and torch.equal(c, c0), "ldf > k1 changes the bits"
    for b in range(3):
        ra, rc = sdr.sd_ref(FM[b], lam1[b], lam2[b])
        ba, bc = sdr.sd_bounds(FM[b], lam1[b], lam2[b], rc)
        sdr.report(f"k1 {k1} k2 {k2} lam1[{b}] SD_a", host(a[b]), ra, ba)
        sdr.report(f"k1 {k1} k2 {k2} lam1[{b}] SD_c", host(c[b]), rc, bc)
        sdr.check_cut_rows(f"k1 {k1} k2 {k2} lam1[{b}]", host(c[b]), lam1[b], k1)
    assert not torch.any(c[0, 0] != 0.0)                                  # lambda_0 = 0: cut
    if k1 > 1:
        assert torch.any(c[1, 0] != 0.0) and torch.any(c[2, 0] != 0.0)    # tiny, of either sign: kept
    # the module's functions take the same route for tensors and batches
    assert torch.equal(sd.area_SD(torch.as_tensor(FM[1]).cuda()), a0[1])
    assert torch.equal(sd.conformal_SD(FM, lam1, lam2), c0)


@pytest.mark.parametrize("pn", ["m", "i"])
def test_shape_diff_stored_maps(eng, fx, pairs, pn):
    m1, m2, _ = pairs[pn]
    for dims in DIMS:
        FM = fx[f"{pn}_FM_{tag(*dims)}"]
        a, c = sd.area_SD(torch.as_tensor(FM).cuda()), sd.conformal_SD(torch.as_tensor(FM).cuda(), m1.eigenvalues, m2.eigenvalues)
        ra, rc = fx[f"{pn}_FM_{tag(*dims)}_a"], fx[f"{pn}_FM_{tag(*dims)}_c"]
        ba, bc = sdr.sd_bounds(FM, m1.eigenvalues, m2.eigenvalues, rc)
        sdr.report(f"{pn} FM {tag(*dims)} SD_a", host(a), ra, ba)
        sdr.report(f"{pn} FM {tag(*dims)} SD_c", host(c), rc, bc)
        sdr.check_cut_rows(f"{pn} FM {tag(*dims)}", host(c), m1.eigenvalues, FM.shape[1])


def test_shape_diff_limits(eng):
    with pytest.raises(ValueError):
        eng.shape_difference(np.zeros((1, 4, 257)), np.ones((1, 257)), np.ones((1, 4)))
    with pytest.raises(ValueError):
        eng.shape_difference(np.zeros((1, 769, 4)), np.ones((1, 4)), np.ones((1, 769)))
    a, c = eng.shape_difference(np.ones((1, 768, 256)), np.ones((1, 256)), np.ones((1, 768)))       # the limits themselves are served
    assert float(a[0, 3, 5]) == 768.0 and float(c[0, 255, 0]) == 768.0


# ---------------------------------------------------------------- dm_pullback_forms_f64
@pytest.mark.parametrize("n2", [SLAB - 1, SLAB, SLAB + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + SLAB + 3])
def test_forms_around_slab_and_chunk(eng, geo, n2):
    """the torus cut to n2 vertices with n_verts2 (stiffness columns past n2 contribute nothing), N1 = 1200 != N2, ld1 > k1"""
    rng = np.random.default_rng(n2)
    p21 = rng.integers(0, geo["grid"]["n"], n2)
    got, ref, bounds = forms_case(eng, geo, "grid", "torus", n2, 17, p21, ld1=21)
    check_forms(f"n2 {n2}", got, ref, bounds, geo["grid"]["lam"], 17)
    got_csr = forms_case(eng, geo, "grid", "torus", n2, 17, p21, rows=False, ld1=21)[0]
    assert torch.equal(got_csr[0], got[0]) and torch.equal(got_csr[1], got[1]), "host CSR (-1 padding) against device rows (col = row padding)"


@pytest.mark.parametrize("k1", [1, 15, 16, 17, 128])
@pytest.mark.parametrize("tgt", ["grid", "torus"])
def test_forms_every_width(eng, geo, k1, tgt):
    src = "torus" if tgt == "grid" else "grid"
    n2 = geo[tgt]["n"]
    p21 = np.random.default_rng(k1).integers(0, geo[src]["n"], n2)
    out = {}
    for lam in (True, False):
        got, ref, bounds = forms_case(eng, geo, src, tgt, n2, k1, p21, lam=lam)
        check_forms(f"{tgt} k1 {k1} lam1 {'given' if lam else 'null'}", got, ref, bounds, geo[src]["lam"] if lam else None, k1)
        out[lam] = got
    assert torch.equal(out[True][0], out[False][0]), "Ga depends on lam1"
    got_csr = forms_case(eng, geo, src, tgt, n2, k1, p21, lam=False, rows=False)[0]
    assert torch.equal(got_csr[0], out[False][0]) and torch.equal(got_csr[1], out[False][1]), "host CSR against device rows"


@pytest.mark.parametrize("kind", ["identity", "constant", "negative"])
def test_forms_special_maps(eng, geo, kind):
    n = geo["torus"]["n"]
    p21 = {"identity": np.arange(n), "constant": np.full(n, 77), "negative": np.arange(n) - n}[kind]
    got, ref, bounds = forms_case(eng, geo, "torus", "torus", n, 16, p21 % n)
    check_forms(kind, got, ref, bounds, geo["torus"]["lam"], 16)
    if kind == "negative":           # NumPy's rule: -n .. -1 count from the end -- the identity's bits
        t = geo["torus"]
        neg = eng.pullback_forms(p21[None], t["Phi"][None], [(t["cols"], t["w"])], t["mass"][None], 16, lam1=t["lam"][None])
        assert torch.equal(neg[0], got[0]) and torch.equal(neg[1], got[1])
    if kind == "constant":           # W 1 = 0: the stiffness form of a constant pull-back is rounding noise of the row sums
        print("constant map: max |Gw| =", float(got[1].abs().max()))


def ragged_batch(geo):
    """five ragged pairs (source, target, vertices of the target in use, seed)"""
    return [("torus", "grid", 1200, 1), ("grid", "torus", 2048, 2), ("grid", "torus", CHUNK + 1, 3), ("torus", "grid", SLAB + 1, 4),
            ("torus", "torus", 2048, 5)]


def run_batch(eng, geo, spec, k1):
    N1 = max(geo[s]["n"] for s, _, _, _ in spec)
    N2 = max(n2 for _, _, n2, _ in spec)
    B = len(spec)
    Phi, mass, p = np.zeros((B, N1, k1)), np.zeros((B, N2)), np.zeros((B, N2), np.int64)
    lam, W, nv1, nv2 = np.zeros((B, k1)), [], [], []
    for b, (s, t, n2, seed) in enumerate(spec):
        Phi[b, :geo[s]["n"]] = geo[s]["Phi"][:, :k1]
        mass[b, :n2] = geo[t]["mass"][:n2]
        p[b, :n2] = np.random.default_rng(seed).integers(0, geo[s]["n"], n2)
        lam[b] = geo[s]["lam"][:k1]
        W.append((geo[t]["cols"][:n2], geo[t]["w"][:n2]))
        nv1.append(geo[s]["n"])
        nv2.append(n2)
    return eng.pullback_forms(p, Phi, W, mass, k1, lam1=lam, n_verts1=nv1, n_verts2=nv2)


def test_forms_independent_of_the_batch(eng, geo):
    spec = ragged_batch(geo)
    k1 = 17
    for me in (0, 2, 3):                                         # a full mesh, one just past a chunk, one just past a slab
        alone = run_batch(eng, geo, [spec[me]], k1)
        again = run_batch(eng, geo, [spec[me]], k1)
        assert torch.equal(alone[0], again[0]) and torch.equal(alone[1], again[1]), "two calls in a row"
        others = [q for q in range(5) if q != me]
        for pos in (0, 2, 4):
            order = others[:pos] + [me] + others[pos:]
            out = run_batch(eng, geo, [spec[q] for q in order], k1)
            assert torch.equal(out[0][pos], alone[0][0]) and torch.equal(out[1][pos], alone[1][0]), (me, pos)
    # and the batch against the host route, pair by pair
    out = run_batch(eng, geo, spec, k1)
    for b, (s, t, n2, seed) in enumerate(spec):
        p21 = np.random.default_rng(seed).integers(0, geo[s]["n"], n2)
        X, Wh = geo[s]["Phi"][p21, :k1], csr_in_row_order(geo[t]["cols_h"], geo[t]["w_h"], n2)
        ref = sdr.forms_ref(X, geo[t]["mass"][:n2], Wh, geo[s]["lam"])
        bounds = sdr.forms_bounds(X, geo[t]["mass"][:n2], Wh, geo[s]["lam"], ref[1])
        check_forms(f"batch[{b}]", (out[0][b:b + 1], out[1][b:b + 1]), ref, bounds, geo[s]["lam"], k1)


def test_forms_placement(eng, geo):
    """every operand as an offset view of a larger buffer of NaN (INT_FILL for the indices): row strides beyond k1 / nnz, rows beyond
    the vertex counts, one element off the 16-byte grid -- the plain call's bits, and no NaN"""
    s, t, k1 = geo["grid"], geo["torus"], 17
    n1, n2 = s["n"], t["n"]
    p21 = np.random.default_rng(8).integers(0, n1, n2)
    plain = eng.pullback_forms(p21[None], s["Phi"][None, :, :k1], [(t["cols"], t["w"])], t["mass"][None], k1, lam1=s["lam"][None, :k1])
    dev = eng.device
    Phi = place(np.ascontiguousarray(s["Phi"][None, :, :k1]), offset_elems=1, ld=k1 + 5, rows=n1 + 3, pad="nan", device=dev)
    mass = place(t["mass"][None], offset_elems=1, ld=n2 + 3, pad="nan", device=dev)
    pm = place(p21[None].astype(np.int32), offset_elems=3, ld=n2 + 3, device=dev)
    lam = place(s["lam"][None, :k1].copy(), offset_elems=1, ld=k1 + 2, pad="nan", device=dev)
    cols = place(t["cols"][None], offset_elems=1, rows=n2 + 3, pad=2 ** 30, device=dev)
    w = place(t["w"][None], offset_elems=1, rows=n2 + 3, pad="nan", device=dev)
    with PointerRecorder(eng.lib, "dm_pullback_forms_f64") as rec:
        got = eng.pullback_forms(pm, Phi, (cols, w), mass, k1, lam1=lam, n_verts1=[n1], n_verts2=[n2])
    assert rec.saw(Phi, mass, lam, cols, w), "the library did not receive the placed operands"
    for q in range(2):
        assert not torch.isnan(got[q]).any()
        assert torch.equal(got[q], plain[q])
    FM = np.random.default_rng(9).standard_normal((2, 40, k1))
    l2 = np.sort(np.random.default_rng(10).uniform(0, 50, (2, 40)), axis=1)
    sp_plain = eng.shape_difference(FM, np.stack([s["lam"][:k1]] * 2), l2)
    with PointerRecorder(eng.lib, "dm_shape_diff_f64") as rec:
        FMp = place(FM, offset_elems=1, ld=k1 + 5, pad="nan", device=dev)
        l1p = place(np.stack([s["lam"][:k1]] * 2), offset_elems=1, ld=k1 + 2, pad="nan", device=dev)
        l2p = place(l2, offset_elems=1, ld=43, pad="nan", device=dev)
        sp_got = eng.shape_difference(FMp, l1p, l2p, k1=k1)
    assert rec.saw(FMp, l1p, l2p)
    for q in range(2):
        assert not torch.isnan(sp_got[q]).any() and torch.equal(sp_got[q], sp_plain[q])


@pytest.mark.parametrize("bad", ["N1", "-N1-1"])
def test_map_out_of_bounds_raises_before_any_launch(eng, geo, bad):
    s, t = geo["grid"], geo["torus"]
    p21 = np.zeros((1, t["n"]), np.int64)
    p21[0, 5] = s["n"] if bad == "N1" else -s["n"] - 1
    with PointerRecorder(eng.lib, "dm_pullback_forms_f64") as rec:
        with pytest.raises(IndexError, match="out of bounds for axis 0 with size 1200"):
            eng.pullback_forms(p21, s["Phi"][None, :, :8], [(t["cols"], t["w"])], t["mass"][None], 8)
        with pytest.raises(IndexError):
            eng.pullback_forms(torch.as_tensor(p21).cuda(), s["Phi"][None, :, :8], [(t["cols"], t["w"])], t["mass"][None], 8)
    assert not rec.calls


def test_forms_limit(eng, geo):
    t = geo["grid"]
    with pytest.raises(ValueError):
        eng.pullback_forms(np.zeros((1, t["n"]), np.int64), np.zeros((1, 4, 257)), [(t["cols"], t["w"])], t["mass"][None], 257)


# ---------------------------------------------------------------- the module's batched call and the class
@pytest.mark.parametrize("SD_type", ["spectral", "semican"])
def test_compute_SD_many(eng, fx, pairs, SD_type):
    m = [pairs["m"][0], pairs["m"][1], pairs["i"][1]]
    rng = np.random.default_rng(77)
    quad = [(m[0], m[1], pairs["m"][2]), (m[0], m[2], None), (m[2], m[1], pairs["m"][2]), (m[1], m[0], rng.integers(0, 252, 240))]
    A, Cc = sd.compute_SD_many([q[0] for q in quad], [q[1] for q in quad], k1=12, p2ps=[q[2] for q in quad], SD_type=SD_type, device=True)
    assert A.shape == (4, 12, 12) and Cc.shape == (4, 12, 12) and A.is_cuda
    ha, hc = sd.compute_SD_many([q[0] for q in quad], [q[1] for q in quad], k1=12, p2ps=[q[2] for q in quad], SD_type=SD_type, device=False)
    for b, (m1, m2, p2p) in enumerate(quad):
        a1, c1 = sd.compute_SD(m1, m2, k1=12, p2p=p2p, SD_type=SD_type, device=True)
        assert torch.equal(a1, A[b]) and torch.equal(c1, Cc[b]), f"pair {b}: the batched call against the single one"
        idx = np.arange(m2.n_vertices) if p2p is None else p2p
        X, mass2 = m1.eigenvectors[idx, :12], np.asarray(m2.A.diagonal())
        if SD_type == "semican":
            ba, bc = sdr.forms_bounds(X, mass2, m2.W, m1.eigenvalues, hc[b])
        else:
            FM = m2.eigenvectors[:, :36].T @ (m2.A @ X)
            ba, bc = sdr.sd_bounds(FM, m1.eigenvalues, m2.eigenvalues, hc[b], sdr.fm_perturbation(X, m2.eigenvectors[:, :36], mass2))
        sdr.report(f"many[{b}] {SD_type} SD_a", host(A[b]), ha[b], ba)
        sdr.report(f"many[{b}] {SD_type} SD_c", host(Cc[b]), hc[b], bc)
        sdr.check_cut_rows(f"many[{b}] {SD_type}", host(Cc[b]), m1.eigenvalues, 12)
    # mixed k1: grouped by k1, lists out
    la, lc = sd.compute_SD_many([q[0] for q in quad], [q[1] for q in quad], k1=[12, 5, 12, 5], p2ps=[q[2] for q in quad], SD_type=SD_type, device=True)
    assert [tuple(x.shape) for x in la] == [(12, 12), (5, 5), (12, 12), (5, 5)]
    assert torch.equal(la[0], A[0]) and torch.equal(lc[2], Cc[2])
    a5, c5 = sd.compute_SD(quad[3][0], quad[3][1], k1=5, p2p=quad[3][2], SD_type=SD_type, device=True)
    assert torch.equal(la[3], a5) and torch.equal(lc[3], c5)


def test_device_rows_of_a_processed_mesh(eng, fx):
    """a TriMesh that still holds the device stiffness rows of its assembly hands them over as they are"""
    from densematcher_amd.pyFM.mesh import TriMesh
    m1, m2 = TriMesh(fx["verts_0"], fx["faces_0"]), TriMesh(fx["verts_1"], fx["faces_1"])
    TriMesh.process_many([m1, m2], [12, 12])
    assert m2._W is None and m2._W_dev is not None
    p2p = fx["p2p"].astype(np.int64)
    a, c = sd.compute_SD(m1, m2, k1=12, p2p=p2p, SD_type="semican", device=True)
    assert m2._W is None and m2._W_dev is not None, "the device route materialised W on the host"
    ha, hc = sd.compute_SD(m1, m2, k1=12, p2p=p2p, SD_type="semican", device=False)
    X = m1.eigenvectors[p2p, :12]
    ba, bc = sdr.forms_bounds(X, np.asarray(m2.A.diagonal()), m2.W, m1.eigenvalues, hc)
    sdr.report("processed meshes SD_a", host(a), ha, ba)
    sdr.report("processed meshes SD_c", host(c), hc, bc)
    sdr.check_cut_rows("processed meshes", host(c), m1.eigenvalues, 12)


def test_functional_mapping_compute_SD(eng, fx_cfg1):
    from densematcher_amd.pyFM.functional import FunctionalMapping
    from densematcher_amd.pyFM.mesh import TriMesh
    f, k = fx_cfg1, int(fx_cfg1["k"])
    meshes = []
    for which in (1, 2):
        m = TriMesh(f[f"verts{which}"], f[f"faces{which}"])
        m.A = sparse.diags(f[f"a{which}"].astype(np.float64)).tocsr()
        m.W = sparse.identity(m.n_vertices).tocsr()
        m.eigenvalues, m.eigenvectors = f[f"lam{which}"][:k].copy(), f[f"Phi{which}"][:, :k].astype(np.float64)
        meshes.append(m)
    model = FunctionalMapping(meshes[0], meshes[1], partial=False, optimizer="L-BFGS-B")
    model.preprocess(n_ev=(k, k), n_descr=128, descr1=f["F1"], descr2=f["F2"], subsample_step=1)
    with pytest.raises(ValueError, match="must be fit before computing the shape difference"):
        model.compute_SD()
    model.fit(w_descr=1e4, w_lap=1e3, w_dcomm=0)
    model.compute_SD()
    FM, l1, l2 = model.FM, model.mesh1.eigenvalues, model.mesh2.eigenvalues
    ra, rc = sdr.sd_ref(FM, l1, l2)
    assert np.array_equal(model.D_a, ra) and np.array_equal(model.D_c, rc)
    assert model.SD_a is None and model.SD_c is None                       # the reference's mismatch of names, kept
    a, c = sd.area_SD(torch.as_tensor(FM).cuda()), sd.conformal_SD(torch.as_tensor(FM).cuda(), l1, l2)
    ba, bc = sdr.sd_bounds(FM, l1, l2, rc)
    sdr.report("fitted map SD_a", host(a), ra, ba)
    sdr.report("fitted map SD_c", host(c), rc, bc)
    sdr.check_cut_rows("fitted map", host(c), l1, k)

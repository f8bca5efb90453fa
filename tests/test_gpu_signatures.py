"""GPU (-m gpu): heat / wave kernel signatures on the device (dm_spectral_signatures[_f64], MatchEngine.signatures) against the vectors
the reference's own signature code produced (tests/golden/fx_sig.npz) and against the host mirror (pyFM/signatures.py), and the
layers above it: FunctionalMapping.preprocess(signature_route="device"), compute_surface_map_batch(descr_type="HKS" | "WKS").

Bound (derived, not measured).  u = 2^-53; for a finite entry b[n,t] = sum_k w |Phi_p Phi_n| / sum_k w from the mirror's weights.
Device and reference each carry at most about (2K + 6) u b -- two sums of K terms in any order, exp to 2 ulp, the products, the
reciprocal -- so |S_dev - S_ref| <= 4 (K + 8) u b entry by entry, K = the eigen-columns kept.  fp32 output: the same after conversion
plus half an fp32 ulp of the value.  Columns whose weight sum is 0 in the mirror must be NaN in every row; columns with
0 < sum w < 2^-960 (subnormal weights; they only occur at T = 2048, at most 32 of them) only have to be non-finite where the mirror is."""
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from densematcher_amd.pyFM import signatures as sg

GOLD = os.path.join(os.path.dirname(__file__), "golden", "fx_sig.npz")
U = 2.0 ** -53
NOTEBOOK = dict(w_descr=1e4, w_lap=1e3, w_dcomm=0, w_ent=1e-1, w_sumto1=1e1, optinit="zeros", maxiter=5000)   # example.ipynb cell 11


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


def _mirror(kind, lam, ev, num, landmarks=None, plain=True):
    """(S, b, wsum, kept): the mirror's [plain | landmark] blocks, the bound's b, every column's weight sum and term count"""
    ev = np.asarray(ev, dtype=np.float64)
    fn = sg.auto_HKS if kind == "HKS" else sg.auto_WKS
    S, Bd, ws, kept = [], [], [], []
    with np.errstate(all="ignore"):
        for lmv in ([False] if plain else []) + ([True] if landmarks is not None and len(landmarks) else []):
            t, mu, denom, k0 = sg.signature_tables(lam, kind, num, lmv)
            w = np.exp(-(t[:, None] * mu[None, :])) if kind == "HKS" else np.exp(-np.square(t[:, None] - mu[None, k0:]) / denom)
            wsum = w.sum(axis=1)
            E = ev[:, k0:]
            if not lmv:
                S.append(fn(lam, ev, num))
                Bd.append(((E * E) @ w.T) * (1.0 / wsum)[None, :])
                ws.append(wsum); kept.append(np.full(num, E.shape[1]))
            else:
                S.append(fn(lam, ev, num, landmarks=landmarks))
                for p in np.asarray(landmarks).reshape(-1):
                    Bd.append((np.abs(E * E[p][None, :]) @ w.T) * (1.0 / wsum)[None, :])
                    ws.append(wsum); kept.append(np.full(num, E.shape[1]))
    return np.concatenate(S, axis=1), np.concatenate(Bd, axis=1), np.concatenate(ws), np.concatenate(kept)


def _check(dev, ref, b, wsum, kept, what=""):
    """the contract of the module docstring, entry by entry; dev float64 or float32"""
    f32 = dev.dtype == np.float32
    dev = dev.astype(np.float64)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    dead = wsum == 0
    tiny = (wsum > 0) & (wsum < 2.0 ** -960)
    assert tiny.sum() <= 32, what
    assert np.isnan(dev[:, dead]).all(), what
    assert not np.isfinite(dev[:, tiny][~np.isfinite(ref[:, tiny])]).any(), what
    ok = ~dead & ~tiny
    d, r = dev[:, ok], ref[:, ok]
    assert np.isfinite(r).all() and np.isfinite(d).all(), what
    tol = 4.0 * (kept[ok][None, :] + 8.0) * U * b[:, ok]
    if f32:
        tol = tol + 0.5 * np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
    err = np.abs(d - r)
    worst = float((err / np.maximum(U * b[:, ok], 1e-300)).max()) if not f32 else float((err / tol).max())
    print(f"{what}: max error {worst:.1f} {'of the fp32 allowance' if f32 else 'u b'} (allowed {'1' if f32 else 4 * (int(kept.max()) + 8)})")
    assert (err <= tol).all(), (what, worst)
    return tol


def _run(eng, Phi, lam, kind, num, **kw):
    return eng.signatures(np.ascontiguousarray(Phi)[None], np.asarray(lam)[None], kind, num, **kw)[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_fixture_parity(fx, eng, width):
    import torch
    k = int(fx["k"])
    lm = fx["landmarks"]
    Phi1, Phi2 = fx["Phi1"].astype(width), fx["Phi2"].astype(width)
    cases = [("HKS", 16, Phi1, fx["lam1"], k, None, "hks"), ("WKS", 24, Phi1, fx["lam1"], k, None, "wks"),
             ("HKS", 9, Phi2, fx["lam2"], None, None, "hks_allk"),
             ("HKS", 5, Phi1, fx["lam1"], k, lm, "hks_lm"), ("WKS", 7, Phi1, fx["lam1"], k, lm, "wks_lm")]
    for kind, num, Phi, lam, kk, landmarks, gold in cases:
        kk_ = Phi.shape[1] if kk is None else kk
        S, b, wsum, kept = _mirror(kind, lam[:kk_], Phi[:, :kk_], num, landmarks, plain=landmarks is None)
        assert kept[0] == (kk_ if kind == "HKS" else kk_ - 1)
        for odt in (torch.float64, torch.float32):
            got = _run(eng, Phi, lam, kind, num, k=kk, landmarks=None if landmarks is None else landmarks[None], plain=landmarks is None, out_dtype=odt)
            _check(got, fx[gold], b, wsum, kept, f"{gold} vs golden ({np.dtype(width).name} basis)")
            _check(got, S, b, wsum, kept, f"{gold} vs mirror ({np.dtype(width).name} basis)")


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_wks_2048(fx, eng, width):
    """compute_surface_map's WKS size: 263 columns whose weights all underflow (NaN in every row, like the reference's), 30 of subnormal weights"""
    k = int(fx["k"])
    Phi = fx["Phi1"].astype(width)
    S, b, wsum, kept = _mirror("WKS", fx["lam1"][:k], Phi[:, :k], 2048)
    assert (wsum == 0).sum() == 263
    got = _run(eng, Phi, fx["lam1"], "WKS", 2048, k=k)
    tol = _check(got, S, b, wsum, kept, "wks-2048 vs mirror")
    sl = slice(None, None, 64)
    _check(got[:, sl], fx["wks_big_cols"], b[:, sl], wsum[sl], kept[sl], "wks-2048[:, ::64] vs golden")
    # row sums: the golden ones are NaN (every row crosses a NaN column), and so must the device's be; over the columns of normal
    # weights they are held at the summed bound (plus the rounding of the two summations themselves)
    gs = fx["wks_big_sum"]
    with np.errstate(all="ignore"):
        ds = got.sum(axis=1)
    assert np.array_equal(np.isfinite(ds), np.isfinite(gs)) and np.isnan(ds[np.isnan(gs)]).all()
    fin = np.isfinite(gs)
    ok = (wsum >= 2.0 ** -960)
    assert (np.abs(ds[fin] - gs[fin]) <= (tol.sum(axis=1) + 2 * ok.sum() * U * b[:, ok].sum(axis=1))[fin]).all()
    assert (np.abs(got[:, ok].sum(axis=1) - S[:, ok].sum(axis=1)) <= tol.sum(axis=1) + 2 * ok.sum() * U * b[:, ok].sum(axis=1)).all()


# ------------------------------------------------------------------------------------------------ edges, against the mirror
SPEC = np.array([0.0, 3e-4, 5e-3, 0.7, 1.9, 2.4, 3.1, 4.4, 5.0, 6.2, 7.7, 8.1, 9.9, 11.0, 12.5, 13.0])      # plain drops 1 column, landmark 3


def _basis(n, k, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((max(n, k), k)))[0][:n]
    return np.ascontiguousarray(q + 0.01 * rng.standard_normal((n, k)), dtype=dtype)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_edges(eng, n):
    for kept_lm in (1, 5, 13):                                    # K - k0 of the landmark blocks; the plain block keeps two more
        K = kept_lm + 3
        lam = SPEC[:K]
        Phi = _basis(n, K, 10 * n + K)
        lms = np.array([n - 1, 0, n - 1, n // 2])                 # (a repeated landmark)
        for kind in ("HKS", "WKS"):
            for num in (1, 17):
                for plain, landmarks in ((True, None), (False, lms), (True, lms[:1])):
                    S, b, wsum, kept = _mirror(kind, lam, Phi, num, landmarks, plain)
                    if kind == "WKS":
                        assert set(np.unique(kept)) <= {K - 1, K - 3} and (landmarks is None or (kept == K - 3).any())
                    got = _run(eng, Phi, lam, kind, num, landmarks=None if landmarks is None else landmarks[None], plain=plain)
                    _check(got, S, b, wsum, kept, f"n={n} K={K} {kind}-{num} plain={plain} P={0 if landmarks is None else len(landmarks)}")
                    got32 = _run(eng, Phi.astype(np.float32), lam, kind, num, landmarks=None if landmarks is None else landmarks[None], plain=plain)
                    S32, b32, _, _ = _mirror(kind, lam, Phi.astype(np.float32), num, landmarks, plain)
                    _check(got32, S32, b32, wsum, kept, "the same on an fp32 basis")


def test_ragged_and_batch_independence(eng):
    """three meshes of 257, 65 and 200 vertices padded to 257 in one call: rows past n_verts are exactly 0, and every mesh's rows are
    bit-identical to those of a call of its own (other neighbours, other landmark count, no padding)"""
    import torch
    K = 13                                                        # (odd: rows that no 16-byte load can take)
    ns = [257, 65, 200]
    lams = [SPEC[:K], SPEC[:K] * 1.3, np.concatenate([[0.0], np.linspace(0.5, 9.0, K - 1)])]
    Phis = [_basis(n, K, 77 + n) for n in ns]
    lm = np.array([[3, 64, 0], [64, 1, 1], [199, 5, 100]])
    pad = np.full((3, 257, K), 7.5)                               # (padding rows hold finite junk: nothing may leak into the result)
    for q in range(3):
        pad[q, :ns[q]] = Phis[q]
    for kind, num in (("HKS", 17), ("WKS", 17)):
        for odt in (torch.float64, torch.float32):
            both = eng.signatures(pad, np.stack(lams), kind, num, landmarks=lm, plain=True, n_verts=ns, out_dtype=odt).cpu().numpy()
            assert both.shape == (3, 257, 4 * num)
            for q in range(3):
                assert np.array_equal(both[q, ns[q]:], np.zeros((257 - ns[q], 4 * num)))
                alone = eng.signatures(Phis[q][None], lams[q][None], kind, num, landmarks=lm[q:q + 1], plain=True, out_dtype=odt)[0].cpu().numpy()
                assert np.array_equal(both[q, :ns[q]], alone, equal_nan=True), (kind, q)
                # other neighbours, another landmark count: the shared blocks keep their bits
                other = eng.signatures(np.stack([Phis[q], Phis[q][::-1]]), np.stack([lams[q], lams[0]]), kind, num,
                                       landmarks=np.stack([lm[q, :2], lm[q, :2]]), plain=True, out_dtype=odt)[0].cpu().numpy()
                assert np.array_equal(other, alone[:, :3 * num], equal_nan=True), (kind, q)
                if odt == torch.float64:
                    S, b, wsum, kept = _mirror(kind, lams[q], Phis[q], num, lm[q], True)
                    _check(alone, S, b, wsum, kept, f"ragged {kind} mesh {q}")


def test_errors(eng):
    Phi = _basis(40, 3, 5)
    with pytest.raises(ValueError):                               # every eigenvalue <= 1e-2: the landmark blocks keep no column (k0 >= K)
        eng.signatures(Phi[None], np.array([[0.0, 1e-3, 5e-3]]), "WKS", 4, landmarks=np.array([[1]]), plain=False)
    Phi = _basis(40, 6, 5)
    with pytest.raises(ValueError):                               # T = 0
        eng.signatures(Phi[None], SPEC[None, :6], "HKS", 0)
    for bad in (40, -1):                                          # a landmark out of range
        with pytest.raises(ValueError):
            eng.signatures(Phi[None], SPEC[None, :6], "HKS", 4, landmarks=np.array([[2, bad]]))
    with pytest.raises(ValueError):                               # ... or past the mesh's own vertex count in a padded batch
        eng.signatures(Phi[None], SPEC[None, :6], "HKS", 4, landmarks=np.array([[30]]), n_verts=[30])
    # the library's own status codes (the Python layer checks first; here it is bypassed)
    import ctypes as C
    import torch
    from densematcher_amd import _lib
    t = torch.ones((1, 4), dtype=torch.float64, device=eng.device)
    mu = torch.ones((1, 6), dtype=torch.float64, device=eng.device)
    P_ = torch.as_tensor(Phi[None]).to(eng.device)
    out = torch.zeros((1, 40, 8), dtype=torch.float64, device=eng.device)
    ia = lambda *v: (C.c_int32 * len(v))(*v)
    call = lambda T, k0, lmv: eng.lib.dm_spectral_signatures_f64(eng.ctx, 1, 40, None, 6, P_.data_ptr(), 6, 0, T, t.data_ptr(), mu.data_ptr(), None,
                                                                  C.cast(ia(*k0), C.c_void_p), 1, C.cast(ia(lmv), C.c_void_p), 1, 0, out.data_ptr())
    assert call(4, (0, 0), 39) == _lib.DM_OK
    assert call(0, (0, 0), 0) == _lib.DM_EINVAL and call(4, (6, 0), 0) == _lib.DM_EINVAL and call(4, (0, 6), 0) == _lib.DM_EINVAL
    assert call(4, (0, 0), 40) == _lib.DM_EINVAL and call(4, (0, 0), -1) == _lib.DM_EINVAL
    eng.synchronize()


# ------------------------------------------------------------------------------------------------ the layers above
def _fx_mesh(fx, which, k):
    m = types.SimpleNamespace(eigenvalues=fx[f"lam{which}"][:k].copy(), eigenvectors=fx[f"Phi{which}"][:, :k].astype(np.float64),
                              A=sp.diags(fx[f"a{which}"].astype(np.float64)).tocsr())
    m.process = lambda *a, **kw: m
    m.area = float(fx[f"a{which}"].astype(np.float64).sum())
    return m


def test_preprocess_device_route(fx):
    """HKS-16 + two-column landmarks + subsample_step = 2 (functional.py:308-334) against the reference's assembled descriptors"""
    from densematcher_amd.pyFM import FunctionalMapping
    k = int(fx["k"])
    model = FunctionalMapping(_fx_mesh(fx, 1, k), _fx_mesh(fx, 2, k), partial=False, optimizer="L-BFGS-B")
    model.preprocess(n_ev=(k, k), n_descr=16, descr_type="HKS", landmarks=fx["landmarks2"], subsample_step=2, signature_route="device")
    for which, descr, col in ((1, model.descr1, 0), (2, model.descr2, 1)):
        assert isinstance(descr, np.ndarray) and descr.dtype == np.float64
        S, b, wsum, kept = _mirror("HKS", fx[f"lam{which}"][:k], fx[f"Phi{which}"][:, :k], 16, fx["landmarks2"][:, col], True)
        sel = np.arange(0, S.shape[1], 2)
        _check(descr, fx[f"pre_descr{which}"], b[:, sel], wsum[sel], kept[sel], f"preprocess descr{which} vs golden")
        _check(descr, S[:, sel], b[:, sel], wsum[sel], kept[sel], f"preprocess descr{which} vs mirror")


def test_wks_preprocess_and_fit(fx):
    """WKS-128 (every column finite) through preprocess(signature_route="device") + fit: the descriptors within the bound of the mirror's,
    the fitted map against the NumPy fit on the very descriptors the device produced"""
    from densematcher_amd.pyFM import FunctionalMapping
    from oracle import dm_oracle as orc
    k = int(fx["k"])
    model = FunctionalMapping(_fx_mesh(fx, 1, k), _fx_mesh(fx, 2, k), partial=False, optimizer="L-BFGS-B")
    model.preprocess(n_ev=(k, k), n_descr=128, descr_type="WKS", signature_route="device")
    for which, descr in ((1, model.descr1), (2, model.descr2)):
        S, b, wsum, kept = _mirror("WKS", fx[f"lam{which}"][:k], fx[f"Phi{which}"][:, :k], 128)
        assert np.isfinite(S).all() and (wsum >= 2.0 ** -960).all()
        _check(descr, S, b, wsum, kept, f"WKS-128 descr{which}")
    model.fit(w_descr=1e4, w_lap=1e3, w_dcomm=0, optinit="zeros")
    Co = orc.fit(fx["Phi1"][:, :k], fx["Phi2"][:, :k], fx["lam1"][:k], fx["lam2"][:k], fx["a1"], fx["a2"],
                 model.descr1.astype(np.float32), model.descr2.astype(np.float32), 1e4, 1e3)
    assert np.isfinite(model.FM).all() and np.abs(model.FM - Co).max() <= 1e-4


class _Duck:
    """what compute_surface_map needs from a pytorch3d Meshes (reference functional_map.py:17-18)"""
    def __init__(self, v, f):
        import torch
        self.v, self.f = torch.tensor(v), torch.tensor(f)

    def verts_list(self):
        return [self.v]

    def faces_list(self):
        return [self.f]


@pytest.fixture(scope="module")
def synth_meshes():
    """four small tori (two of 300 vertices, two of 288) with their cotangent spectra (15 pairs), computed once on the host"""
    from densematcher_amd import synth
    out = []
    for nu, nv, perturb, seed in ((20, 15, 0.0, 0), (20, 15, 0.15, 1), (18, 16, 0.0, 0), (18, 16, 0.2, 2)):
        v, f = synth.torus_mesh(nu, nv, perturb=perturb, seed=seed)
        lam, phi, a = synth.eigenbasis(v, f, 15)
        W, _ = synth.cotan_laplacian(v, f)
        out.append(dict(v=v, f=f, lam=lam, phi=phi, a=a, W=W))
    return out


def _inject(monkeypatch, meshes):
    """TriMesh.process hands out the stored spectra, so that the single and the batched call see the same eigenbases bit for bit"""
    from densematcher_amd.pyFM.mesh import TriMesh

    def process(self, k=200, **kw):
        for m in meshes:
            if m["v"].shape == self.vertlist.shape and np.array_equal(self.vertlist, m["v"]):
                self.W, self.A = m["W"], sp.diags(m["a"]).tocsr()
                self.eigenvalues, self.eigenvectors = m["lam"][:k].copy(), m["phi"][:, :k].copy()
                return self
        raise RuntimeError("unknown mesh")
    monkeypatch.setattr(TriMesh, "process", process)


def _same_tuple(got, want, q):
    assert np.array_equal(got[7]._FM_base, want[7]._FM_base, equal_nan=True), q     # a pair's fit does not depend on its batch
    assert np.array_equal(got[7].FM, want[7].FM, equal_nan=True), q                 # (the ICP map)
    for slot in (0, 1, 4, 5, 10, 11, 12, 13):
        assert np.array_equal(got[slot], want[slot]), (q, slot)
    for slot in (2, 3, 6):
        assert np.array_equal(got[slot][0], want[slot][0]) and np.array_equal(got[slot][1], want[slot][1]), (q, slot)


def test_batch_hks_equals_single_device_route(synth_meshes, monkeypatch):
    """compute_surface_map_batch(descr_type="HKS", c1s=None, c2s=None) -- an AssertionError before this entry point existed -- returns, pair
    by pair, compute_surface_map(..., signature_route="device"): two pairs of one size, one of another"""
    from densematcher_amd.functional_map import compute_surface_map, compute_surface_map_batch
    _inject(monkeypatch, synth_meshes)
    d = [_Duck(m["v"], m["f"]) for m in synth_meshes]
    pairs = [(d[0], d[1]), (d[1], d[0]), (d[2], d[3])]
    kw = dict(n_ev=15, compute_extra=True, optimizer="L-BFGS-B", descr_type="HKS", fit_params=dict(NOTEBOOK))
    got = compute_surface_map_batch([p[0] for p in pairs], [p[1] for p in pairs], None, None, **kw)
    assert len(got) == 3
    for q, p in enumerate(pairs):
        want = compute_surface_map(p[0], p[1], None, None, signature_route="device", **kw)
        _same_tuple(got[q], want, q)
        # the returned models' descriptors: implicit, the host mirror on demand -- within the bound of what the single call downloaded
        lazy = got[q][7].descr1
        assert lazy.shape == want[7].descr1.shape == (p[0].v.shape[0], 16) and not isinstance(lazy, np.ndarray)
        m = synth_meshes[[0, 1, 2][q]]
        S, b, wsum, kept = _mirror("HKS", m["lam"], m["phi"], 16)
        assert np.array_equal(np.asarray(lazy), S)
        _check(want[7].descr1, S, b, wsum, kept, f"pair {q}: downloaded descr1 vs mirror")


def test_batch_wks_2048_equals_single_device_route(synth_meshes, monkeypatch):
    """WKS-2048 carries the reference's non-finite columns (0 * inf where every weight underflows); nothing special-cases them, so the
    batched call must do exactly what the single device-route call does with them: the same tuple, or the same refusal"""
    from densematcher_amd.functional_map import compute_surface_map, compute_surface_map_batch
    _inject(monkeypatch, synth_meshes)
    d = [_Duck(m["v"], m["f"]) for m in synth_meshes]
    kw = dict(n_ev=15, compute_extra=False, optimizer="L-BFGS-B", descr_type="WKS", fit_params=dict(w_descr=1e4, w_lap=1e3, w_dcomm=0))

    def outcome(fn):
        try:
            return fn()
        except Exception as e:                                    # noqa: BLE001 (the kind of refusal is what is compared)
            return e
    got = outcome(lambda: compute_surface_map_batch([d[0]], [d[1]], None, None, **kw))
    want = outcome(lambda: compute_surface_map(d[0], d[1], None, None, signature_route="device", **kw))
    print("WKS-2048: single call ->", type(want).__name__, "| batched call ->", type(got).__name__)
    if isinstance(want, Exception):
        assert type(got) is type(want), (got, want)
    else:
        assert not isinstance(got, Exception), got
        _same_tuple(got[0], want, 0)

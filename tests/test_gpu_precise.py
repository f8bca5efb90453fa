"""
GPU (-m gpu): dm_precise_map[_f64] (csrc/dm_precise.hip) on every return statement of its projection, at every lane-group width,
on both candidate routes and in the call shapes nothing else makes -- against an independent longdouble solver
(tests/precise_restate.py), the oracle, and the reference's own output on the designed inputs (tests/golden/fx_precise_regions.npz;
tests/test_precise_cpu.py holds the oracle and the solver against each other and against that fixture without a GPU).
"""
import collections
import os

import numpy as np
import pytest

import precise_restate as pr
from oracle import dm_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-9            # the project's precise-map tolerance (tests/test_gpu_parity.py: test_precise_map_and_its_assignment)
WIDTHS = [2, 3, 16, 17, 32, 33, 64, 65, 128, 200]         # G = 16 up to 16 columns, 32 up to 32, else the whole wave
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_precise_regions.npz")


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import MatchEngine
    return MatchEngine()


@pytest.fixture(scope="module")
def fixture():
    fx = dict(np.load(GOLDEN, allow_pickle=False))
    assert pr.fixture_hash(pr.fixture_inputs()) == str(fx["inputs_sha256"]), "regenerated inputs differ from the ones the reference was run on"
    return fx


def _np(t):
    return t.cpu().numpy()


def _run(eng, V, faces, P, C=None, dtype=np.float32, **kw):
    """one pair through eng.precise_map with emb1 = V, emb2 = P C (C = identity unless given) -> numpy outputs without the batch axis"""
    C = np.eye(V.shape[1]) if C is None else C
    out = eng.precise_map(np.ascontiguousarray(V, dtype=dtype)[None], np.ascontiguousarray(P, dtype=dtype)[None],
                          np.ascontiguousarray(C, dtype=np.float64)[None], np.ascontiguousarray(faces, dtype=np.int32)[None], **kw)
    return [_np(x)[0] for x in out]


def _f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def _margin(det):
    """winner to runner-up, in the distances the oracle chooses on (inf: one sound candidate)"""
    out = np.full(len(det), np.inf)
    for i, x in enumerate(det):
        d = np.sort(x["dist"][np.isfinite(x["dist"])])
        if len(d) > 1:
            out[i] = d[1] - d[0]
    return out


def _against_oracle(V, faces, P, fm, bary):
    """the device's result against the oracle's on the same embeddings: the projected point's distance within 1e-9 max(1, d) at every
    point (a face NAME is a tie up to rounding on a shared edge or vertex, the projected point is not), the name and the weights
    wherever the oracle's own margin between winner and runner-up is clear of that.  Returns (share of points with a clear margin,
    the oracle's details)."""
    det = []
    fo, bo = orc.project_pc_to_triangles(V, faces, P, details=det)
    assert fm.min() >= 0 and fm.max() < len(faces)
    d_gpu = np.linalg.norm(pr.projected(V, faces, fm, bary) - P, axis=1)
    d_orc = np.linalg.norm(pr.projected(V, faces, fo, bo) - P, axis=1)
    scale = np.maximum(1.0, d_orc)
    assert np.all(np.abs(d_gpu - d_orc) <= TOL * scale), np.abs(d_gpu - d_orc).max()
    assert np.abs(bary.sum(1) - 1.0).max() <= 1e-12
    clear = _margin(det) > TOL * scale
    assert np.array_equal(fm[clear], fo[clear])
    assert np.abs(bary - bo)[clear].max(initial=0.0) <= TOL * max(1.0, np.abs(bo).max())
    return clear.mean(), det


def random_mesh(N1, nf, N2, k, seed, scale=0.3):
    """N1 vertices anywhere in k dimensions, nf faces on random triples of them (no surface: the kernel does not ask for one; obtuse
    faces, faces through one another and long candidate lists are the point), N2 points near random faces; float32 values"""
    rng = np.random.default_rng(seed)
    V = _f32(rng.standard_normal((N1, k)) * scale)
    faces = np.argsort(rng.random((nf, N1)), axis=1)[:, :3]
    w = rng.dirichlet(np.ones(3), N2)
    P = (w[:, :, None] * V[faces[rng.integers(0, nf, N2)]]).sum(1) + rng.standard_normal((N2, k)) * (0.3 * scale / np.sqrt(k))
    return V, faces, _f32(P)


# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("k", WIDTHS)
def test_every_branch_at_every_width(eng, fixture, k):
    """The four designed triangles, as a one-face mesh (nf = 1, N1 = 3: the scalar code path, multi false) and with the face listed
    twice (several candidates, an exact tie): the 25 return statements are all taken at this width, the face is the reference's (the
    first), the weights and the projected point are the longdouble solver's within 1e-9 -- and the reference's where it was run."""
    count = collections.Counter()
    for shape in pr.SHAPES:
        V, P = pr.designed_case(shape, k)
        count.update(pr.branches(V, P))
        q_ref, b_ref, _ = pr.closest_point(V, P)
        for faces in ([[0, 1, 2]], [[0, 1, 2], [0, 1, 2]]):
            fm, bary = _run(eng, V, np.array(faces), P)
            assert not fm.any(), (shape, len(faces))
            assert np.abs(bary - b_ref).max() <= TOL, (shape, len(faces))
            assert np.abs(pr.projected(V, faces, fm, bary) - q_ref).max() <= TOL, (shape, len(faces))
            name = f"a_{shape}_k{k}_"
            if len(faces) == 2 and name + "face" in fixture:
                assert np.array_equal(fm, fixture[name + "face"]) and np.abs(bary - fixture[name + "bary"]).max() <= TOL
    assert set(count) == set(pr.LABELS) and min(count.values()) >= 10, count


@pytest.mark.parametrize("k", [5, 40])
def test_the_region4_quirk_decides(eng, fixture, k):
    """The open obtuse corner over a far triangle, and its twin, turned into k dimensions (float64 entry point, so that the rotation
    is not rounded to float32 and changes roundings only): the faces are the reference's, run at k = 3 -- among them the points
    where the unclamped region-4 distance names the FARTHER face.
    Names are compared where the oracle's margin exceeds 1e-9; the two triangles share no edge, so that leaves out < 1 %."""
    for which in pr.CORNER_FACES:
        V, faces, P = pr.corner_case(which, k, f32=False)
        ref_face, ref_bary = fixture[f"b_{which}_face"], fixture[f"b_{which}_bary"]
        fm, bary = _run(eng, V, faces, P, dtype=np.float64)
        clear_share, det = _against_oracle(V, faces, P, fm, bary)
        clear = _margin(det) > TOL
        print(f"{which}, k = {k}: margin <= 1e-9 at {1.0 - clear.mean():.4f} of the points")
        assert 1.0 - clear.mean() <= 0.01 and clear_share >= 0.99
        assert np.array_equal(fm[clear], ref_face[clear])
        assert np.abs(bary - ref_bary)[clear].max() <= TOL
        farther = clear & (pr.face_distance(V, faces, P, ref_face) - pr.nearest_distance(V, faces, P)[0] > TOL)
        labels = {pr.branch(*det[i]["abcdef"][0]) for i in np.where(farther)[0]}
        print(f"    the farther face is the reference's at {farther.sum()} points {sorted(labels)}; named there: {(fm[farther] == 1).mean():.3f}")
        assert farther.sum() >= 5 and labels == {"4b", "4e"} and np.all(fm[farther] == 1)


def _torus_case(nu, nv, k, n2):
    from densematcher_amd import synth
    v3, faces = synth.torus_mesh(nu, nv)
    rng = np.random.default_rng(100 * nu + k)
    edge = 2.0 * np.pi * 0.4 / nv
    V = _f32(pr.embed(v3, k, 7, f32=False) + rng.standard_normal((nu * nv, k)) * (0.1 * edge / np.sqrt(k)))
    w = rng.dirichlet(np.ones(3), n2)
    P = (w[:, :, None] * V[faces[rng.integers(0, len(faces), n2)]]).sum(1) + rng.standard_normal((n2, k)) * (0.5 * edge / np.sqrt(k))
    return V, faces, _f32(P)


@pytest.mark.parametrize("nu,nv,k", [(12, 8, 15), (12, 8, 40), (12, 8, 128), (64, 32, 15), (64, 32, 40), (64, 32, 128)])
def test_meshes_with_shared_edges(eng, nu, nv, k):
    """A closed mesh: on a shared edge the face name is a tie up to rounding, so what is compared is the distance |projected point - p|
    -- with the solver's minimum over ALL faces (left out: points with a candidate in 4b / 4e, where the reference's choice is not the
    nearest face by design; their share is stated and <= 10 %), and with the oracle."""
    V, faces, P = _torus_case(nu, nv, k, 300 if nu == 12 else 150)
    fm, bary = _run(eng, V, faces, P)
    clear_share, det = _against_oracle(V, faces, P, fm, bary)
    quirk = np.array([x["multi"] and any(pr.branch(*row) in ("4b", "4e") for row in x["abcdef"]) for x in det])
    d_gpu = np.linalg.norm(pr.projected(V, faces, fm, bary) - P, axis=1)
    d_min, _ = pr.nearest_distance(V, faces, P)
    err = np.abs(d_gpu - d_min)[~quirk].max()
    print(f"torus {nu} x {nv}, k = {k}: candidates per point {np.mean([len(x['cand']) for x in det]):.1f}; 4b / 4e among them at "
          f"{quirk.mean():.3f} of the points; clear margin at {clear_share:.3f}; max |d - d_solver| = {float(err):.2e}")
    assert quirk.mean() <= 0.10
    assert err <= TOL


def _lattice(k, n=5, h=0.5):
    """(n x n) lattice of right triangles with dyadic coordinates in k dimensions (columns past the third hold one dyadic constant
    each, in vertices and points alike), and query points on its vertices, edge midpoints and cell centres, in the plane and 0.25 above"""
    i, j = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    V3 = np.stack([i * h, j * h, np.zeros(n * n)], 1)
    c = [(a * n + b, (a + 1) * n + b, a * n + b + 1, (a + 1) * n + b + 1) for a in range(n - 1) for b in range(n - 1)]
    faces = np.array([t for v00, v10, v01, v11 in c for t in ((v00, v10, v11), (v00, v11, v01))])
    mids = np.concatenate([(V3[faces[:, a]] + V3[faces[:, b]]) / 2 for a, b in ((0, 1), (1, 2), (2, 0))])
    Q3 = np.unique(np.concatenate([V3, mids]), axis=0)
    Q3 = np.concatenate([Q3, Q3 + (0.0, 0.0, 0.25)])

    def widen(X3):
        X = np.tile(0.25 * ((np.arange(k) % 4) - 1.0), (len(X3), 1))
        X[:, :3] = X3
        return X
    return widen(V3), faces, widen(Q3), len(Q3) // 2


@pytest.mark.parametrize("k", [3, 20, 40])
def test_exact_ties_name_the_lowest_face(eng, k):
    """Query points on shared edges and vertices of a dyadic lattice: every intermediate is exact, so the tied faces' distances are
    bitwise equal (asserted on the oracle first) and the lexicographic minimum over lane groups, waves and the atomically filled
    candidate list has to name the lowest face index -- the same in two calls; a point on a vertex (Deltamin = 0) is at distance 0."""
    V, faces, Q, n_plane = _lattice(k)
    det = []
    fo, bo = orc.project_pc_to_triangles(V, faces, Q, details=det)
    tri = V[faces]
    tied_sizes = []
    for i, x in enumerate(det):
        d_true = pr.closest_point(tri[x["cand"]], Q[i])[2]
        tied = np.where(d_true - d_true.min() <= 1e-12)[0]
        assert len(set(x["dist"][tied].tolist())) == 1, (i, x["dist"][tied])          # bitwise equal
        assert x["dist"][tied[0]] == float(d_true.min()) and np.all(np.delete(x["dist"], tied) > x["dist"][tied[0]])
        assert fo[i] == x["cand"][tied].min()
        tied_sizes.append(len(tied))
    tied_sizes = np.array(tied_sizes)
    print(f"lattice, k = {k}: {len(Q)} points, tied faces per point", dict(collections.Counter(tied_sizes.tolist())))
    assert (tied_sizes >= 2).mean() >= 0.7 and tied_sizes.max() == 6
    fm, bary = _run(eng, V, faces, Q)
    fm2, bary2 = _run(eng, V, faces, Q)
    assert np.array_equal(fm, fm2) and np.array_equal(bary, bary2)
    assert np.array_equal(fm, fo)
    assert np.array_equal(bary, bo)
    d = np.linalg.norm(pr.projected(V, faces, fm, bary) - Q, axis=1)
    assert np.array_equal(d, np.r_[np.zeros(n_plane), np.full(n_plane, 0.25)])


def test_candidate_list_boundary(eng):
    """64 x 32 torus: exactly 4096 faces, every one a candidate of the far points -- the list holds them (route word 0); one face more
    and the far points take the route that re-tests every face (route word 1).  Both equal the oracle."""
    from densematcher_amd import synth
    v3, faces = synth.torus_mesh(64, 32)
    assert len(faces) == 4096
    rng = np.random.default_rng(9)
    k = 6
    V = np.zeros((2048, k))                 # the torus in five of six dimensions: the mesh has no extent in the last
    V[:, :5] = pr.embed(v3, 5, 3, f32=False) + rng.standard_normal((2048, 5)) * 0.002
    w = rng.dirichlet(np.ones(3), 40)
    P = (w[:, :, None] * V[faces[rng.integers(0, 4096, 40)]]).sum(1) + rng.standard_normal((40, k)) * 0.01
    P[:6, k - 1] = 1000.0                   # far along that direction: every face's bound exceeds Deltamin
    V, P = _f32(V), _f32(P)
    for extra, route in ((0, 0), (1, 1)):
        F = np.concatenate([faces, faces[1234:1234 + extra, ::-1]])
        fm, bary, info = _run(eng, V, F, P, return_info=True)
        _, det = _against_oracle(V, F, P, fm, bary)
        ncand = np.array([len(x["cand"]) for x in det])
        assert ncand[:6].min() == ncand.max() == 4096 + extra and ncand[6:].max() < 1000
        assert info == route, (extra, info)
        fm2, bary2 = _run(eng, V, F, P)
        assert np.array_equal(fm, fm2) and np.array_equal(bary, bary2)


# --------------------------------------------------------------------------- #
# call shapes
def test_batch_of_three_equals_solo_calls(eng):
    """B = 3 with different vertices, faces and C per pair: every pair bit-identical to its own call, dense matrix included"""
    N1, N2, nf, k2, k1 = 257, 63, 255, 20, 24
    rng = np.random.default_rng(21)
    meshes = [random_mesh(N1, nf, N2, k1, 30 + b) for b in range(3)]
    Cs = [np.eye(k2, k1) + 0.05 * rng.standard_normal((k2, k1)) for _ in range(3)]
    Phi1 = np.stack([m[0] for m in meshes]).astype(np.float32)
    Phi2 = np.stack([m[2][:, :k2] for m in meshes]).astype(np.float32)
    F = np.stack([m[1] for m in meshes]).astype(np.int32)
    fm, bary, M = (_np(x) for x in eng.precise_map(Phi1, Phi2, np.stack(Cs), F, dense=True))
    assert len({fm[b].tobytes() for b in range(3)}) == 3
    for b in range(3):
        fm1, bary1, M1 = _run(eng, Phi1[b], F[b], Phi2[b], C=Cs[b], dense=True)
        assert np.array_equal(fm[b], fm1) and np.array_equal(bary[b], bary1) and np.array_equal(M[b], M1)
        _against_oracle(Phi1[b].astype(np.float64), F[b], Phi2[b].astype(np.float64) @ Cs[b], fm[b], bary[b])


@pytest.mark.parametrize("k2,k1", [(20, 35), (70, 33)])
def test_rectangular_map(eng, k2, k1):
    """C (k2, k1) with k2 != k1: emb2 = Phi2[:, :k2] C has k1 columns"""
    V, faces, _ = random_mesh(300, 200, 1, k1, 40 + k2)
    rng = np.random.default_rng(k1)
    Phi2 = _f32(rng.standard_normal((120, k2)) * 0.3)
    C = rng.standard_normal((k2, k1)) / np.sqrt(k2)
    fm, bary = _run(eng, V, faces, Phi2, C=C)
    _against_oracle(V, faces, Phi2 @ C, fm, bary)
    M, fo, bo = orc.precise_map_dense(C, V, Phi2, faces)
    d_gpu, d_orc = (np.linalg.norm(pr.projected(V, faces, f, b) - Phi2 @ C, axis=1) for f, b in ((fm, bary), (fo, bo)))
    assert np.abs(d_gpu - d_orc).max() <= TOL * max(1.0, d_orc.max())


@pytest.mark.parametrize("k", [6, 30, 70])
def test_row_strides_larger_than_the_map(eng, k):
    """ld1 > k1 and ld2 > k2 (a basis with more columns than the map uses), the columns past the map NaN: never read -- bit-identical
    to the call on the cut basis, float32 and float64"""
    V, faces, P = random_mesh(255, 257, 63, k, 50 + k)
    for dtype in (np.float32, np.float64):
        plain = _run(eng, V, faces, P, dtype=dtype, dense=True)
        Vp, Pp = np.full((255, k + 5), np.nan), np.full((63, k + 3), np.nan)
        Vp[:, :k], Pp[:, :k] = V, P
        padded = _run(eng, Vp, faces, Pp, C=np.eye(k), dtype=dtype, dense=True)
        assert all(np.array_equal(a, b) for a, b in zip(plain, padded))
        assert np.isfinite(padded[1]).all() and np.isfinite(padded[2]).all()
    _against_oracle(V, faces, P, *plain[:2])


@pytest.mark.parametrize("k", [15, 40])
def test_float64_entry_point(eng, k):
    """dm_precise_map_f64: on a basis that float32 cannot hold, against the oracle on those float64 values; on widened float32 values,
    bit-identical to the float32 entry point"""
    rng = np.random.default_rng(60 + k)
    V, faces, P = random_mesh(300, 257, 100, k, 60 + k)
    V64, P64 = V * (1.0 + 1e-9 * rng.standard_normal(V.shape)), P * (1.0 + 1e-9 * rng.standard_normal(P.shape))
    assert not np.array_equal(_f32(V64), V64)
    fm, bary = _run(eng, V64, faces, P64, dtype=np.float64)
    _against_oracle(V64, faces, P64, fm, bary)
    a, b = _run(eng, V, faces, P, dtype=np.float32, dense=True), _run(eng, V, faces, P, dtype=np.float64, dense=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("N1,N2,nf", [(3, 1, 1), (3, 63, 2), (255, 300, 255), (257, 63, 257), (1000, 300, 2), (1000, 1, 257),
                                      (257, 300, 1)])
def test_sizes_off_the_tile_boundaries(eng, N1, N2, nf):
    """N1, N2 and nf around the 256-wide scans and the matrix tiles; nf = 1: one candidate, the scalar code path"""
    for k in (7, 40):
        V, faces, P = random_mesh(N1, nf, N2, k, N1 + N2 + nf + k)
        fm, bary = _run(eng, V, faces, P)
        share, det = _against_oracle(V, faces, P, fm, bary)
        if nf == 1:
            assert not any(x["multi"] for x in det)
            assert np.abs(bary - pr.closest_point(V[faces[0]], P)[1]).max() <= TOL


def test_too_many_vertices_is_refused(eng):
    """the distance row of a point lives in LDS: N1 = 20000 does not fit, and is refused before anything is launched"""
    V, faces, P = random_mesh(20000, 4, 5, 3, 1)
    with pytest.raises(ValueError, match="too many vertices"):
        _run(eng, V, faces, P)
    V, faces, P = random_mesh(50, 4, 5, 3, 1)               # (and the engine goes on working)
    _against_oracle(V, faces, P, *_run(eng, V, faces, P))


# --------------------------------------------------------------------------- #
def _scatter(N1, faces, fm, bary):
    M = np.zeros((len(fm), N1))
    for c in range(3):
        np.add.at(M, (np.arange(len(fm)), faces[fm, c]), bary[:, c])
    return M


def test_dense_output(eng):
    """The dense matrix is the scatter of (face, weights) bit for bit -- every other entry exactly 0 --, rows sum to 1 within 4 ulp,
    nothing leaks between the pairs of a batch, and a second scratch=True call leaves nothing of the first behind."""
    N1, N2, nf, k = 300, 257, 200, 33
    A, B_ = random_mesh(N1, nf, N2, k, 70), random_mesh(N1, nf, N2, k, 71)
    outs = {}
    for name, (V, faces, P) in (("A", A), ("B", B_)):
        fm, bary, M = _run(eng, V, faces, P, dense=True)
        assert np.array_equal(M, _scatter(N1, faces, fm, bary))
        assert (M != 0).sum(1).max() <= 3
        assert np.abs(M.sum(1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
        outs[name] = (fm, bary, M)
    assert not np.array_equal(outs["A"][0], outs["B"][0])
    Phi1, Phi2 = np.stack([A[0], B_[0]]).astype(np.float32), np.stack([A[2], B_[2]]).astype(np.float32)
    F, C = np.stack([A[1], B_[1]]).astype(np.int32), np.stack([np.eye(k)] * 2)
    for scratch in (False, True):
        fm, bary, M = (_np(x) for x in eng.precise_map(Phi1, Phi2, C, F, dense=True, scratch=scratch))
        for b, name in enumerate("AB"):
            assert np.array_equal(fm[b], outs[name][0]) and np.array_equal(bary[b], outs[name][1]) and np.array_equal(M[b], outs[name][2])
    # scratch: the same shape again, the pairs swapped -- the engine hands out the same memory
    M_first = eng.precise_map(Phi1, Phi2, C, F, dense=True, scratch=True)[2]
    M_second = eng.precise_map(Phi1[::-1].copy(), Phi2[::-1].copy(), C, F[::-1].copy(), dense=True, scratch=True)[2]
    assert M_first.data_ptr() == M_second.data_ptr()
    assert np.array_equal(_np(M_second)[0], outs["B"][2]) and np.array_equal(_np(M_second)[1], outs["A"][2])


@pytest.mark.parametrize("k", [3, 40])
def test_zero_area_faces_are_passed_over(eng, k):
    """A vertex row listed twice makes faces of zero area (a = 0): region 0 then forms 0 * inf.  The reference hands that NaN on;
    here NaN candidates are passed over: the result is finite, sums to 1, and is no farther than the nearest sound face."""
    V, faces, P = _torus_case(12, 8, k, 200)
    V = np.concatenate([V, V[:5]])                            # rows 96..100 repeat rows 0..4
    bad = np.array([[0, 96, 50], [97, 1, 1], [2, 98, 98], [99, 3, 77], [4, 100, 30]])
    F = np.concatenate([bad[:2], faces[:40], bad[2:4], faces[40:], bad[4:]])
    fm, bary, M = _run(eng, V, F, P, dense=True)
    assert np.isfinite(bary).all() and np.isfinite(M).all()
    assert np.abs(bary.sum(1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    sound = np.array([len(set(V[f].tobytes() for f in face)) == 3 for face in F])
    assert sound.sum() == len(F) - 5 and np.all(sound[fm])
    d_gpu = np.linalg.norm(pr.projected(V, F, fm, bary) - P, axis=1)
    _, det = _against_oracle(V, F, P, fm, bary)
    assert sum(np.isnan(x["dist"]).any() for x in det) >= 100             # (the NaN candidates are there, and in most lists)
    quirk = np.array([any(pr.branch(*row) in ("4b", "4e") for row in x["abcdef"][np.isfinite(x["dist"])]) for x in det])
    d_min, _ = pr.nearest_distance(V, F[sound], P)
    assert (~quirk).sum() >= 20
    assert np.all(d_gpu[~quirk] <= d_min[~quirk] + TOL)
    # nothing sound at all: face 0 and its first corner, as the oracle
    fm0, bary0 = _run(eng, V, bad, P[:9])
    assert not fm0.any() and np.array_equal(bary0, np.tile([1.0, 0.0, 0.0], (9, 1)))


SLIVER = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 1e-6, 0.0)])


@pytest.mark.parametrize("k", [3, 40])
def test_sliver_face(eng, k):
    """A triangle of height 1e-6 of its base: the weights are ill-conditioned (a c - b^2 cancels twelve digits), so only the
    projected point is compared, with the longdouble solver.  The bound is 8 x the error of the ORACLE's float64 arithmetic on the
    same inputs (the device sums the dot products in another order across lanes and contracts to fma).  That error, measured:
    9.3e-6 at k = 3 and 5.4e-6 at k = 40, one face or two (base 1, coordinates up to 3)"""
    both = pr.embed(np.concatenate([SLIVER, pr.plane_grid(k)]), k, 90 + k)
    V, P = both[:3], both[3:]
    q_ref = pr.closest_point(V, P)[0]
    for faces in (np.array([[0, 1, 2]]), np.array([[0, 1, 2], [0, 1, 2]])):
        fo, bo = orc.project_pc_to_triangles(V, faces, P)
        err_orc = float(np.abs(pr.projected(V, faces, fo, bo) - q_ref).max())
        fm, bary = _run(eng, V, faces, P)
        err_gpu = float(np.abs(pr.projected(V, faces, fm, bary) - q_ref).max())
        print(f"sliver, k = {k}, {len(faces)} face(s): |projected - solver| oracle {err_orc:.3e}  device {err_gpu:.3e}")
        assert not fm.any() and np.isfinite(bary).all()
        assert err_gpu <= 8.0 * err_orc

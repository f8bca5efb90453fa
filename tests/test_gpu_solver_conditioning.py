"""
GPU (-m gpu): the closed-form solver (dm_fmap_solve / dm_fmap_fit) on ILL-CONDITIONED systems, every route.

Row i of C solves (P_ff + diag(dd_i)) x_i = rhs_i (oracle.dm_oracle.fmap_solve).  The library picks its solver by the sizes and the
options alone (dm_fmap.hip: fmap_solve_plan_for), n = k1 - 1:

    n <= 64                                 fmap_solve_reg_kernel<NBT>
    65 <= n <= 128, k2 % 4 == 0             fmap_solve_pcg_kernel<8, 4>, fall-back fmap_solve_reg_kernel<8>   (solve_pcg)
    65 <= n <= 128, k2 % 4 != 0             fmap_solve_reg_kernel<NBT>
    129 <= n <= 176                         fmap_solve_pcgs_kernel,      fall-back fmap_solve_blocked_kernel
    177 <= n <= 199                         fmap_solve_pcgs_kernel,      fall-back fmap_solve_2phase_kernel
    solve_reg = 0, n <= 128                 fmap_solve_blocked_kernel
    solve_packed = 1                        fmap_solve_kernel
    solve_pcg = 0                           the direct kernel of the row

Every route is checked against a float64 Cholesky solve refined with longdouble residuals (oracle fmap_solve_refined, pinned against
mpmath in test_oracle_golden.py) of the same fp32 A, Bm, with a condition-aware bound per system:

    |x_gpu - x_ref|_inf <= max(floor_route, c_route (n + D) u kappa_i) |x_ref|_inf,     u = 2^-53,

and the launch profiler (profile_report(kernels=True)) proves which kernels ran.
"""
import numpy as np
import pytest

from oracle import dm_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
WD, WL = 1e4, 1e3
# floors of the bound (relative to |x_ref|_inf) and the constants of its condition-dependent part, per kind of route.  Measured worst
# cases on the MI355X (the route table this module prints with -s): direct solvers 1.2e-14 at kappa <= 1e2 and 0.04 (n + D) u kappa;
# the iteration, on the systems it accepts, 1.7e-11 at kappa ~ 4 and 0.29 (n + D) u kappa (near-collinear rows: 5e-5 at kappa 5e10,
# the direct solvers 6e-5 there).  The constants allow about ten times that; the iteration's floor stays at 1e-9, the accuracy its
# stopping rule was designed for (it is not measured at every kappa between the families).
FLOOR_DIRECT = 1e-13      # Cholesky: rounding of P (D terms) and of the factorisation (n terms)
FLOOR_ITER = 1e-9         # the iteration stops on its recurrence residual: r^T M^-1 r reduced by 1e-22
C_KAPPA_DIRECT = 0.5
C_KAPPA_ITER = 4.0

PCG_SMALL, PCG_BIG = "(fmap_solve_pcg_kernel<8, 4>)", "fmap_solve_pcgs_kernel"
BLOCKED, TWO_PHASE, PACKED = "fmap_solve_blocked_kernel", "fmap_solve_2phase_kernel", "fmap_solve_kernel"
OPTS = {"default": {}, "pcg0": {"solve_pcg": 0}, "reg0": {"solve_reg": 0}, "packed": {"solve_packed": 1}}


def route(k1, k2, solve_pcg=1, solve_reg=1, solve_packed=0):
    """(iteration kernel or None, direct kernel) the library is expected to launch"""
    n = k1 - 1
    nb = (n + 15) // 16
    if solve_packed:
        return None, PACKED
    if n >= 129:
        return (PCG_BIG if solve_pcg else None), (TWO_PHASE if n >= 177 else BLOCKED)
    if not solve_reg:
        return None, BLOCKED
    nbt = 2 if nb <= 2 else 4 if nb <= 4 else 6 if nb <= 6 else 8
    it = PCG_SMALL if (solve_pcg and n >= 65 and k2 % 4 == 0) else None
    return it, f"fmap_solve_reg_kernel<{nbt}>"


def route_name(k1, k2, opts):
    it, direct = route(k1, k2, **opts)
    return (it.strip("()").split("<")[0] + " + " if it else "") + direct.split("<")[0]


@pytest.fixture(scope="module")
def _engine():
    from densematcher_amd.engine import MatchEngine
    return MatchEngine()


@pytest.fixture
def eng(_engine):
    yield _engine
    _engine.reset_options()
    _engine.profile_kernel("")


TABLE = {}     # route -> [systems, pairs, fell back, worst err / ((n + D) u kappa), worst err, kappa there]


@pytest.fixture(scope="module", autouse=True)
def _route_table():
    yield
    if not TABLE:
        return
    print("\nclosed-form solver on ill-conditioned systems, worst case per route (err = |x - x_ref|_inf / |x_ref|_inf)")
    print(f"{'route':58s} {'systems':>8s} {'pairs':>6s} {'fell back':>9s} {'err/((n+D)u kappa)':>18s} {'worst err':>10s} {'its kappa':>10s}")
    for name in sorted(TABLE):
        s, p, f, r, e, k = TABLE[name]
        print(f"{name:58s} {s:8d} {p:6d} {f:9d} {r:18.2e} {e:10.2e} {k:10.2e}")


def _record(name, systems, fell_back, ratio, err, kappa):
    row = TABLE.setdefault(name, [0, 0, 0, 0.0, 0.0, 0.0])
    row[0] += systems
    row[1] += 1
    row[2] += int(fell_back)
    if ratio > row[3]:
        row[3] = ratio
    if err > row[4]:
        row[4], row[5] = err, kappa


# --------------------------------------------------------------------------- #
# inputs (deterministic; one pair at a time, stacked into batches)
def _lams(rng, k1, k2):
    lam1 = np.sort(rng.uniform(0.0, 4.0 * k1, k1)); lam1[0] = 0.0
    lam2 = np.sort(rng.uniform(0.0, 4.0 * k1, k2)); lam2[0] = 0.0
    return lam1, lam2


def make_pair(family, k1, k2, D, seed, eps=1e-3, npairs=1, rho=0.85, d0=20, noise=0.0, zero_row=None, coincide=None):
    """one pair's (A (k1,D) f32, Bm (k2,D) f32, lam1, lam2).

    well       random A, D >= 2 k1, distinct eigenvalues: kappa <= 1e2
    collinear  lam1 == lam2 with `npairs` repeated values; row c+1 of A = row c + eps noise under each repeated value
    decay      rows of A scaled by rho^c
    rankdef    d0 distinct channels tiled to D (+ noise * N(0, 0.01) on the copies): P = A A^T has rank d0 (about d0 when noisy)
    singular   `well` with row zero_row + 1 of A zero (unknown zero_row); coincide = i0: lam2[i0] = lam1[zero_row + 1], else none
    """
    rng = np.random.default_rng(seed)
    lam1, lam2 = _lams(rng, k1, k2)
    A = rng.standard_normal((k1, D)) * 0.1
    Bm = rng.standard_normal((k2, D)) * 0.1
    if family == "collinear":
        m = min(k1, k2)
        lam1 = np.sort(rng.uniform(0.0, 4.0 * k1, k1)); lam1[0] = 0.0
        cs = np.linspace(1, m - 2, npairs + 2).astype(int)[1:-1] if npairs > 1 else [m // 2]
        for c in cs:
            lam1[c + 1] = lam1[c]
            A[c + 1] = A[c] + eps * rng.standard_normal(D) * 0.1
        lam2[:m] = lam1[:m]
        lam2 = np.sort(lam2)
    elif family == "decay":
        A *= (rho ** np.arange(k1))[:, None]
    elif family == "rankdef":
        base = rng.standard_normal((k1, d0)) * 0.1
        A = np.tile(base, (1, -(-D // d0)))[:, :D]
        A[:, d0:] += noise * rng.standard_normal((k1, D - d0)) * 0.1
    elif family == "singular":
        A[zero_row + 1] = 0.0
        if coincide is not None:
            lam2[coincide] = lam1[zero_row + 1]
    elif family != "well":
        raise ValueError(family)
    return A.astype(np.float32), Bm.astype(np.float32), lam1, lam2


def _stack(pairs):
    return tuple(np.stack([p[j] for p in pairs]) for j in range(4))


def _c00(B):
    return np.array([1.0, -0.9, 0.7, -1.3, 1.1, -0.6][:B])


def solve(eng, A, Bm, lam1, lam2, c00, wd, wl, opts, check=True):
    """C, info and the {launch name: kernel expressions} of one fmap_solve call under the options `opts`"""
    eng.reset_options()
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.profile_kernel("*")
    try:
        C, info = eng.fmap_solve(A, Bm, lam1, lam2, c00, wd, wl, check=check, return_info=True)
        C, info = C.cpu().numpy(), info.cpu().numpy()
        kern = {n: set(v[2]) for n, v in eng.profile_report(kernels=True).items()}
    finally:
        eng.profile_kernel("")
        eng.reset_options()
    return C, info, kern


def assert_route(kern, k1, k2, opts):
    it, direct = route(k1, k2, **opts)
    assert kern.get("fmap_solve_chol") == {direct}, (k1, k2, opts, kern)
    if it is None:
        assert "fmap_solve_pcg" not in kern, (k1, k2, opts, kern)
    else:
        assert kern.get("fmap_solve_pcg") == {it}, (k1, k2, opts, kern)


def check_against_reference(name, C, ref, D, c00, iterated, fell_back):
    """the condition-aware bound on every row of every pair; returns the failures"""
    bad = []
    for b, (Cr, kappa) in enumerate(ref):
        k2, k1 = Cr.shape
        n = k1 - 1
        assert C[b, 0, 0] == c00[b] and np.all(C[b, 1:, 0] == 0.0)          # the pinned column, exactly
        it = iterated and not fell_back[b]
        floor, ck = (FLOOR_ITER, C_KAPPA_ITER) if it else (FLOOR_DIRECT, C_KAPPA_DIRECT)
        xr = Cr[:, 1:]
        err = np.abs(C[b, :, 1:] - xr).max(axis=1) / np.abs(xr).max(axis=1)
        lim = np.maximum(floor, ck * (n + D) * U * kappa)
        ratio = err / ((n + D) * U * kappa)
        w = int(np.argmax(err))
        _record(name, k2, fell_back[b], float(ratio.max()), float(err[w]), float(kappa[w]))
        for i in np.nonzero(~(err <= lim))[0][:3]:
            bad.append(f"{name} pair {b} row {i}: err {err[i]:.2e} > {lim[i]:.2e} (kappa {kappa[i]:.2e})")
    return bad


def run_all_routes(eng, k1, k2, A, Bm, lam1, lam2, wd, wl, family, must_fall_back=()):
    """every option set that gives a distinct route at these sizes, checked against the reference; the pairs listed in
    `must_fall_back` must leave the iteration (where there is one) and come back bit for bit as the solve_pcg = 0 map.
    Returns (the largest kappa, the failures)"""
    B, _, D = A.shape
    c00 = _c00(B)
    ref = [orc.fmap_solve_refined(A[b], Bm[b], lam1[b], lam2[b], c00[b], wd, wl) for b in range(B)]
    it, _ = route(k1, k2)
    sets = ["default", "packed"] + (["pcg0"] if it else []) + (["reg0"] if k1 - 1 <= 128 else [])
    out, bad = {}, []
    for s in sets:
        C, info, kern = solve(eng, A, Bm, lam1, lam2, c00, wd, wl, OPTS[s])
        assert_route(kern, k1, k2, OPTS[s])
        assert np.all(info == 0), (s, info)
        out[s] = C
    fell_back = [False] * B
    if it:
        fell_back = [np.array_equal(out["default"][b], out["pcg0"][b]) for b in range(B)]
        missed = [b for b in must_fall_back if not fell_back[b]]
        if missed:
            bad.append(f"{family} k1={k1} k2={k2}: pairs {missed} accepted by the iteration, not bit-identical to solve_pcg = 0 "
                       f"(max diff {max(np.abs(out['default'][b] - out['pcg0'][b]).max() for b in missed):.2e})")
    for s, C in out.items():
        name = f"{route_name(k1, k2, OPTS[s])} [{family}]"
        iterated = s == "default" and it is not None
        bad += check_against_reference(name, C, ref, D, c00, iterated, fell_back if iterated else [False] * B)
    return max(float(r[1].max()) for r in ref), bad


SHAPES = [(17, 17), (17, 9), (17, 30), (64, 64), (64, 40), (66, 64), (66, 80), (66, 66), (128, 128), (128, 132), (128, 100), (128, 126),
          (129, 128), (129, 129), (130, 130), (130, 96), (177, 177), (177, 60), (178, 178), (178, 200), (200, 200), (200, 24)]


@pytest.mark.parametrize("k1,k2", SHAPES)
def test_conditioning_every_route(eng, k1, k2):
    """families (a) near-collinear degenerate pairs, (b) channel-scale decay, (c) rank-deficient descriptors, (d) well conditioned,
    on every route of these sizes, against the refined reference"""
    bad = []
    D = 2 * k1
    # (d) well conditioned: the tight floors.  With D = 2 k the spectrum of P_ff is spread (kappa ~ 30) and the iteration's six-step
    # gate hands the pairs to the direct solver; with D = 8 k (kappa ~ 3) the iteration keeps them
    for Dw in (D, 8 * k1):
        pairs = [make_pair("well", k1, k2, Dw, 100 * k1 + k2 + Dw + q) for q in range(2)]
        kappa, b0 = run_all_routes(eng, k1, k2, *_stack(pairs), WD, WL, f"well D={Dw // k1}k")
        assert kappa <= 1e2, kappa
        bad += b0
    # (a) one near-collinear pair per system matrix, eps 1e-2 .. 1e-5 (one eps per pair of the batch), then four such pairs at 1e-3 and
    # 1e-5; on both bases (D = 8 k: the rest of the spectrum is clustered, the iteration sees two isolated small eigenvalues)
    for Dw in (D, 8 * k1):
        pairs = [make_pair("collinear", k1, k2, Dw, 200 * k1 + k2 + Dw + q, eps=e) for q, e in enumerate([1e-2, 1e-3, 1e-4, 1e-5])]
        bad += run_all_routes(eng, k1, k2, *_stack(pairs), WD, WL, f"collinear x1 D={Dw // k1}k")[1]
        pairs = [make_pair("collinear", k1, k2, Dw, 300 * k1 + k2 + Dw + q, eps=e, npairs=4) for q, e in enumerate([1e-3, 1e-5])]
        bad += run_all_routes(eng, k1, k2, *_stack(pairs), WD, WL, f"collinear x4 D={Dw // k1}k")[1]
    # (b) channel-scale decay rho^c under three Laplacian weights
    for wl in (1e3, 10.0, 0.1):
        pairs = [make_pair("decay", k1, k2, D, 400 * k1 + k2 + q, rho=r) for q, r in enumerate([0.7, 0.85])]
        bad += run_all_routes(eng, k1, k2, *_stack(pairs), WD, wl, f"decay w_lap={wl:g}")[1]
    # (c) 20 or 60 distinct channels tiled to 120 (exactly, and with 1e-4 noise on the copies): where P_ff is singular the iteration's
    # gate sends the pair to the direct solver, bit for bit the solve_pcg = 0 map
    Dr, n = 120, k1 - 1
    cases = [(20, 0.0), (60, 0.0), (20, 1e-4), (60, 1e-4)]
    pairs = [make_pair("rankdef", k1, k2, Dr, 500 * k1 + k2 + q, d0=d0, noise=nz) for q, (d0, nz) in enumerate(cases)]
    must = [q for q, (d0, nz) in enumerate(cases) if (d0 if nz == 0.0 else Dr) < n]
    bad += run_all_routes(eng, k1, k2, *_stack(pairs), WD, WL, "rankdef", must_fall_back=must)[1]
    assert not bad, "\n".join(bad[:20])


# the k1 of the routes for the tests below (one per row of the route table)
ROUTE_SHAPES = [(17, 17), (64, 40), (66, 64), (66, 66), (128, 128), (129, 129), (130, 96), (177, 60), (178, 178), (200, 24)]


@pytest.mark.parametrize("k1,k2", ROUTE_SHAPES)
def test_conditioning_rank_deficient_falls_back_bit_identical(eng, k1, k2):
    """(c) D in {20, 60} descriptor channels, fewer than the n unknowns (D random channels; D / 2 channels twice, with 1e-4 noise on
    the copies): the iteration, where there is one, hands every pair to the fall-back -- the solve_pcg = 0 map bit for bit"""
    for D in (20, 60):
        pairs = [make_pair("rankdef", k1, k2, D, 600 * k1 + k2 + D, d0=D), make_pair("rankdef", k1, k2, D, 610 * k1 + k2 + D, d0=D // 2, noise=1e-4)]
        must = [0, 1] if D < k1 - 1 else []
        _, bad = run_all_routes(eng, k1, k2, *_stack(pairs), WD, WL, f"rankdef D={D}", must_fall_back=must)
        assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("k1,k2", ROUTE_SHAPES)
@pytest.mark.parametrize("opt", ["default", "pcg0", "reg0", "packed"])
def test_conditioning_exactly_singular(eng, k1, k2, opt):
    """(e) a zero row of A at unknown c (first, last, on a 16-block boundary) with w_lap = 0, or with one eigenvalue of mesh 2 equal
    to lam1[c + 1]: every route raises DenseMatchError; with check=False only that pair's status word is set, it names one of its
    singular systems, and the other pairs are bit for bit their solo solves"""
    from densematcher_amd._lib import DenseMatchError
    n, D = k1 - 1, 2 * k1
    opts = OPTS[opt]
    for c in sorted({0, n - 1, min(16, n - 1)}):
        for mode in ("w_lap=0", "coincide"):
            i0 = min(k2 - 1, 5) if mode == "coincide" else None
            wl = 0.0 if mode == "w_lap=0" else WL
            pairs = [make_pair("well", k1, k2, D, 700 * k1 + k2 + c),
                     make_pair("singular", k1, k2, D, 710 * k1 + k2 + c, zero_row=c, coincide=i0),
                     make_pair("well", k1, k2, D, 720 * k1 + k2 + c)]
            A, Bm, l1, l2 = _stack(pairs)
            c00 = _c00(3)
            with pytest.raises(DenseMatchError):
                solve(eng, A, Bm, l1, l2, c00, WD, wl, opts)
            C, info, kern = solve(eng, A, Bm, l1, l2, c00, WD, wl, opts, check=False)
            assert_route(kern, k1, k2, opts)
            singular = set(range(k2)) if mode == "w_lap=0" else {i0}
            assert info[0] == 0 and info[2] == 0 and (info[1] - 1) in singular, (c, mode, info)
            for b in (0, 2):
                Cs, infos, _ = solve(eng, A[b:b + 1], Bm[b:b + 1], l1[b:b + 1], l2[b:b + 1], c00[b:b + 1], WD, wl, opts)
                assert infos[0] == 0 and np.array_equal(C[b], Cs[0]), (c, mode, b)


@pytest.mark.parametrize("k1,k2", ROUTE_SHAPES)
@pytest.mark.parametrize("opt", ["default", "pcg0", "reg0", "packed"])
def test_conditioning_mixed_batch_equals_solo(eng, k1, k2, opt):
    """(f) well-conditioned, near-collinear, rank-deficient (fall-back) and singular pairs in one batch: every pair's map is its solo
    map bit for bit -- a pair's bits do not depend on its batch, whatever route each pair takes"""
    D = 2 * k1
    pairs = [make_pair("well", k1, k2, D, 800 * k1 + k2),
             make_pair("collinear", k1, k2, D, 810 * k1 + k2, eps=1e-4),
             make_pair("rankdef", k1, k2, D, 820 * k1 + k2, d0=20),
             make_pair("singular", k1, k2, D, 830 * k1 + k2, zero_row=min(16, k1 - 2), coincide=min(k2 - 1, 3))]
    A, Bm, l1, l2 = _stack(pairs)
    c00 = _c00(4)
    C, info, _ = solve(eng, A, Bm, l1, l2, c00, WD, WL, OPTS[opt], check=False)
    assert info[3] != 0
    for b in range(4):
        Cs, infos, _ = solve(eng, A[b:b + 1], Bm[b:b + 1], l1[b:b + 1], l2[b:b + 1], c00[b:b + 1], WD, WL, OPTS[opt], check=False)
        assert infos[0] == info[b] and np.array_equal(C[b], Cs[0]), (b, np.abs(C[b] - Cs[0]).max())


@pytest.mark.parametrize("k1,k2", ROUTE_SHAPES)
@pytest.mark.parametrize("opt", ["default", "pcg0", "reg0", "packed"])
def test_conditioning_scale_invariance(eng, k1, k2, opt):
    """every operation of the solve is homogeneous: w_descr and w_lap both times 2^s (s even: square roots stay exact), or lam1 and
    lam2 both times 2^t (the eigenvalues enter as (lam / max lam)^2), give the same bits -- a mismatch is an absolute threshold or a
    scale-dependent approximation"""
    D = 2 * k1
    pairs = [make_pair("collinear", k1, k2, D, 900 * k1 + k2, eps=1e-4), make_pair("decay", k1, k2, D, 910 * k1 + k2, rho=0.7),
             make_pair("well", k1, k2, D, 920 * k1 + k2)]
    A, Bm, l1, l2 = _stack(pairs)
    c00 = _c00(3)
    C0, info0, _ = solve(eng, A, Bm, l1, l2, c00, WD, WL, OPTS[opt])
    assert np.all(info0 == 0)
    for s in (-40, -10, 10, 40):
        C, _, _ = solve(eng, A, Bm, l1, l2, c00, WD * 2.0 ** s, WL * 2.0 ** s, OPTS[opt])
        assert np.array_equal(C, C0), (f"w * 2^{s}", np.abs(C - C0).max())
    for t in (-20, 7, 30):
        C, _, _ = solve(eng, A, Bm, l1 * 2.0 ** t, l2 * 2.0 ** t, c00, WD, WL, OPTS[opt])
        assert np.array_equal(C, C0), (f"lam * 2^{t}", np.abs(C - C0).max())


@pytest.mark.parametrize("real_dtype", [np.float32, np.float64])
def test_conditioning_fit_isometric_torus(eng, real_dtype):
    """(5) end to end: fmap_fit on two copies of one torus (Phi1 = Phi2, lam1 = lam2 with repeated eigenvalues) with smooth descriptors
    of D = 64 < k = 128 channels: the fit equals the solve of its own projections bit for bit, and that solve meets the condition-aware
    bound against the refined reference of those projections; C within the project's 1e-4 of the float64 oracle"""
    from densematcher_amd import synth
    k, D = 128, 64
    v, f = synth.torus_mesh(24, 16)
    lam, phi, a = synth.eigenbasis(v, f, k)
    F1, F2 = synth.smooth_feature_pair(phi, phi, D, 11, 12)
    P = phi.astype(real_dtype)[None]
    am = a.astype(real_dtype)[None]
    L = lam[None].astype(np.float64)
    eng.profile_kernel("*")
    try:
        Cf = eng.fmap_fit(P, P, am, am, F1[None], F2[None], L, L, WD, WL).cpu().numpy()
        kern = {n: set(v[2]) for n, v in eng.profile_report(kernels=True).items()}
    finally:
        eng.profile_kernel("")
    assert_route(kern, k, k, {})
    A = eng.project(P, am, F1[None], k).cpu().numpy()
    Bm = eng.project(P, am, F2[None], k).cpu().numpy()
    c00 = eng.c00(P, P, am, am).cpu().numpy()
    Cs = eng.fmap_solve(A, Bm, L, L, c00, WD, WL).cpu().numpy()
    assert np.array_equal(Cf, Cs)
    Cr, kappa = orc.fmap_solve_refined(A[0], Bm[0], lam, lam, c00[0], WD, WL)
    Cd, _, _ = solve(eng, A, Bm, L, L, c00, WD, WL, OPTS["pcg0"])
    fell_back = [np.array_equal(Cd[0], Cf[0])]
    bad = check_against_reference(f"fmap_fit isometric torus {np.dtype(real_dtype).name}", Cf, [(Cr, kappa)], D, c00, True, fell_back)
    bad += check_against_reference(f"fmap_fit isometric torus {np.dtype(real_dtype).name}, solve_pcg=0", Cd, [(Cr, kappa)], D, c00, False, [True])
    assert not bad, "\n".join(bad)
    Co = orc.fit(phi, phi, lam, lam, a, a, F1, F2, WD, WL)
    err = np.abs(Cf[0] - Co).max()
    print(f"isometric torus {np.dtype(real_dtype).name}: kappa max {kappa.max():.2e}, |C - C_oracle| = {err:.2e}, fell back: {fell_back[0]}")
    assert err <= 1e-4


@pytest.mark.parametrize("k2", [1, 5])
def test_single_column_map_is_the_pinned_column(eng, k2):
    """k1 = 1 leaves no system to solve: C is the pinned column (c00 in row 0, exact zeros below), info = 0, the same bits on a
    second call -- through fmap_solve and through fmap_fit.  Whichever direct kernel writes it: no iteration runs"""
    B, D, N = 2, 16, 64
    rng = np.random.default_rng(40 + k2)
    A = (rng.standard_normal((B, 1, D)) * 0.1).astype(np.float32)
    Bm = (rng.standard_normal((B, k2, D)) * 0.1).astype(np.float32)
    lam1 = np.zeros((B, 1))
    lam2 = np.sort(rng.uniform(0.0, 4.0, (B, k2)), axis=1); lam2[:, 0] = 0.0
    c00 = _c00(B)
    want = np.zeros((B, k2, 1)); want[:, 0, 0] = c00
    C, info, kern = solve(eng, A, Bm, lam1, lam2, c00, WD, WL, {})
    assert len(kern.get("fmap_solve_chol", ())) == 1 and "fmap_solve_pcg" not in kern, kern
    assert np.array_equal(C, want) and not np.signbit(C[:, 1:]).any() and np.all(info == 0), (C, info)
    C2, info2, _ = solve(eng, A, Bm, lam1, lam2, c00, WD, WL, {})
    assert C2.tobytes() == C.tobytes() and np.all(info2 == 0)

    Phi1 = (rng.standard_normal((B, N, 8)) * 0.1).astype(np.float32)          # (row stride 8; the fit reads lam's k1 = 1, k2 columns)
    Phi2 = (rng.standard_normal((B, N, 8)) * 0.1).astype(np.float32)
    a1 = rng.uniform(0.5, 1.5, (B, N)).astype(np.float32) / N
    a2 = rng.uniform(0.5, 1.5, (B, N)).astype(np.float32) / N
    F1 = rng.standard_normal((B, N, D)).astype(np.float16)
    F2 = rng.standard_normal((B, N, D)).astype(np.float16)
    want[:, 0, 0] = eng.c00(Phi1, Phi2, a1, a2).cpu().numpy()
    assert np.all(want[:, 0, 0] != 0.0)
    Cf = eng.fmap_fit(Phi1, Phi2, a1, a2, F1, F2, lam1, lam2, WD, WL).cpu().numpy()
    assert np.array_equal(Cf, want) and not np.signbit(Cf[:, 1:]).any(), Cf
    Cf2 = eng.fmap_fit(Phi1, Phi2, a1, a2, F1, F2, lam1, lam2, WD, WL).cpu().numpy()
    assert Cf2.tobytes() == Cf.tobytes()


# dm_workspace_bytes after ONE fmap_solve (B = 4, D = 2 k1) on a fresh engine at commit 6252592, which reserved the streamed image and the
# flag words on every route plus 4096 bytes of slack; the plan reserves what it takes, never more
ARENA_BYTES_BEFORE_THE_PLAN = {(17, 17): 1048576, (128, 128): 2097152, (150, 20): 2097152, (194, 24): 18874368}


@pytest.mark.parametrize("k1,k2", sorted(ARENA_BYTES_BEFORE_THE_PLAN))
def test_arena_no_larger_than_before_the_plan(k1, k2):
    from densematcher_amd.engine import MatchEngine
    B, D = 4, 2 * k1
    A, Bm, lam1, lam2 = _stack([make_pair("well", k1, k2, D, 1000 * k1 + k2 + q) for q in range(B)])
    fresh = MatchEngine()
    try:
        fresh.fmap_solve(A, Bm, lam1, lam2, _c00(B), WD, WL)
        got = fresh.workspace_bytes()
    finally:
        fresh.close()
    print(f"arena after one fmap_solve, k1 = {k1}, k2 = {k2}: {got} bytes (before the plan: {ARENA_BYTES_BEFORE_THE_PLAN[(k1, k2)]})")
    assert 0 < got <= ARENA_BYTES_BEFORE_THE_PLAN[(k1, k2)]


ARENA_SMALL_ROUTE_BEFORE_THE_PLAN = 2097152      # measured at commit 6252592 with the call below


def test_arena_small_route_reserves_what_it_takes():
    """a batch sized so that any over-reservation shows: k1 = k2 = 17, B = 156 takes P, Q (156 * 34 * 17 * 8 -> 721408 bytes in
    multiples of 256) and the block image (156 * 2048 = 319488), 1040896 in all; dm_ws_reserve adds 4096 and rounds to 1 MiB, which
    leaves 3584 bytes: the slack and the flag words reserved on this route at commit 6252592 (4096 + 768) made it 2 MiB there"""
    from densematcher_amd.engine import MatchEngine
    k, B, D = 17, 156, 34
    rng = np.random.default_rng(17156)
    A = (rng.standard_normal((B, k, D)) * 0.1).astype(np.float32)
    Bm = (rng.standard_normal((B, k, D)) * 0.1).astype(np.float32)
    lam = np.sort(rng.uniform(0.0, 4.0 * k, (B, k)), axis=1); lam[:, 0] = 0.0
    fresh = MatchEngine()
    try:
        fresh.fmap_solve(A, Bm, lam, lam + 0.5, np.ones(B), WD, WL)
        got = fresh.workspace_bytes()
    finally:
        fresh.close()
    assert got == 1 << 20 < ARENA_SMALL_ROUTE_BEFORE_THE_PLAN, got


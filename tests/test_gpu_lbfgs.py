"""
GPU (-m gpu): the device L-BFGS on its own (dm_lbfgs_init / dm_lbfgs_advance / dm_lbfgs_result, csrc/dm_lbfgs_dev.h), one call at a time.
The kernel is a pure function (state, energy, gradient) -> (state, next trial point): tests/lbfgs_restate.py drives it with energies and
gradients computed on the host and compares EVERY call of EVERY pair with a high-precision reference of that one call started from the
kernel's own state, so nothing drifts and a wrong lane partner, ring-buffer slot or stale rho / gamma shows in the call it happens in.
Both direction routines (registers: n <= 256 and m <= 32; LDS: the rest), both compiled copies (stand-alone, fused fit), every status
word, every line-search branch, the restart, the curvature skip, non-finite energies and the argument guards.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.optimize

import lbfgs_restate as lr

pytestmark = pytest.mark.gpu

STATS = lr.new_stats()              # every checked step of the module: the knife-edge share is asserted at the end


def engine():
    from densematcher_amd.engine import default_engine
    return default_engine()


def check_run(funs, x0, m=10, cap=120, **opts):
    own = lr.new_stats()
    r = lr.drive(engine(), funs, np.atleast_2d(np.asarray(x0, np.float64)), m, dict(lr.TIGHT, **opts), cap=cap, stats=own)
    for k in ("steps", "knife"):
        STATS[k] += own[k]
    STATS["why"].extend(own["why"])
    return r


# ------------------------------------------------------------------------------------------------------------------ (a) single steps
@pytest.mark.parametrize("n,m", list(lr.STEP_SHAPES))
def test_every_call_against_the_reference(n, m):
    """B = 3 (a quadratic of condition 1e3, chained Rosenbrock, the weighted barrier with trials outside x > 0), every call of every pair:
    integer state exact; x and g the trial point and the uploaded gradient bitwise; the new history row xt - x, g_t - g bitwise, no other
    row touched, rho and gamma within n 2^-53 sum |s_i y_i|; d against the dense longdouble -H g of the kernel's own history (tolerance
    8 x the deviation of a sequential float64 two-loop recursion, floor 64 2^-53 |d|_inf); the next trial point within 1 ulp of x + t d
    and t inside the reference's spread over the slope's rounding bound; stopped pairs bitwise unchanged (they are fed NaN).
    Largest direction deviation in units of the float64 two-loop's own (the bound is 8), as printed on an MI355X:
        (1, 1) 0.16  (2, 3) 2.14  (63, 10) 1.27  (64, 10) 1.51  (65, 10) 3.00  (225, 10) 1.29  (256, 32) 0.86  (256, 33) 1.06
        (257, 10) 0.98  (300, 5) 1.10  (513, 64) 0.38
    and 1 of the module's 3936 checked steps was knife-edge (a sufficient-decrease test within 4 ulp, at (2, 3))."""
    funs, x0, opts = lr.step_problem(n, m)
    own = lr.new_stats()
    r = lr.drive(engine(), funs, x0, m, opts, cap=120, stats=own)
    for k in ("steps", "knife"):
        STATS[k] += own[k]
    STATS["why"].extend(own["why"])
    print(f"(n, m) = ({n}, {m}): direction ratio {own['ratio']:.2f} | status {r.status.tolist()} iterations {r.nit.tolist()} evaluations "
          f"{r.nfev.tolist()} | knife-edge {own['knife']} of {own['steps']} {sorted(set(own['why']))}")
    assert (r.status != 0).all()
    if m < 10 and n > 1:
        assert r.nit.max() > 2 * m, "the ring buffer does not wrap"


# ------------------------------------------------------------------------------------------------------------------ (b) designed cases
def test_designed_status_cases_on_the_device():
    zero = lambda x, nit=0: (1.5, np.zeros(x.size))
    r = check_run([zero], np.ones(5))
    assert (r.status[0], r.nit[0], r.nfev[0]) == (1, 0, 1)
    edge = lambda x, nit=0: (0.0, np.array([0.25, -0.5, 0.125]))
    r = check_run([edge], np.ones(3), pgtol=0.5)
    assert (r.status[0], r.nit[0], r.nfev[0]) == (1, 0, 1)
    r = check_run([edge], np.ones(3), pgtol=float(np.nextafter(0.5, 0.0)), maxiter=0)
    assert r.status[0] == 3
    nang = lambda x, nit=0: (1.0, np.array([0.0, np.nan, 0.0]))
    r = check_run([nang], np.ones(3))
    assert (r.status[0], r.nfev[0]) == (5, 1)
    for i in (0, 1, 3):
        r = check_run([lr.rosenbrock], lr.rosen_x0(10), maxiter=i)
        assert (r.status[0], r.nit[0]) == (3, i)
    assert r.stats["knife"] == 0


@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_maxfun_on_the_device(k):
    r = check_run([lr.rosenbrock], lr.rosen_x0(10), maxfun=k, cap=k + 1)
    assert r.status[0] != 0 and r.evaluations <= k + 1 and r.stats["knife"] == 0
    assert r.f[0] == lr.rosenbrock(r.x[0])[0] <= lr.rosenbrock(lr.rosen_x0(10))[0]


def test_flipped_quadratic_on_the_device():
    q = lr.quadratic(7, seed=2, origin=0.5)
    x0 = np.full(7, 0.5)
    r = check_run([lr.flipped(q)], x0, maxls=20)
    assert (r.status[0], r.nit[0], r.nfev[0]) == (5, 0, 21) and r.stats["knife"] == 0
    assert r.x[0].tobytes() == x0.tobytes()
    assert "line-search-fail" in r.labels and "restart" not in r.labels


def test_trap_on_the_device():
    seen = []

    def rec(x, nit=0):
        seen.append((nit, x.copy()))
        return lr.rosenbrock(x, nit)
    r = check_run([lr.trap(rec, 3)], lr.rosen_x0(10))
    assert (r.status[0], r.nit[0], r.nhist[0]) == (5, 3, 0) and r.stats["knife"] == 0
    assert sum("restart" in c for c in r.trace[0]) == 1 and "line-search-fail" in r.trace[0][-1]
    accepted = [x for nit, x in seen if nit == 2][-1]
    assert r.x[0].tobytes() == accepted.tobytes() and r.f[0] == lr.rosenbrock(r.x[0])[0]
    assert r.nfev[0] == len(seen) == len([1 for nit, _ in seen if nit < 3]) + 2 * 20


def test_curvature_skip_on_the_device():
    r = check_run([lr.bump], [[2.0]], maxls=1, maxiter=1)
    assert (r.status[0], r.nit[0], r.nhist[0]) == (3, 1, 0) and r.stats["knife"] == 0
    assert r.trace[0][-1] == ["extrapolate", "maxls-accept", "curvature-skip"]


def test_barrier_on_the_device():
    r = check_run([lr.barrier(lr.BARRIER_C)], np.full(6, 3.0), **lr.BARRIER)
    assert not np.isfinite(r.energies[0]).all()
    assert r.status[0] in (1, 2) and np.abs(r.x[0] - 1.0).max() <= 1e-6 and r.stats["knife"] == 0


def test_fallback_starts_on_the_device():
    (_, s, ls), (_, s2, ls2) = lr.FALLBACK_STARTS
    r = check_run([lr.rosenbrock], [s], maxls=ls, maxfun=400, cap=401)
    assert {"maxls-back", "curvature-skip"} <= r.labels and r.stats["knife"] == 0
    r = check_run([lr.rosenbrock], [s2], maxls=ls2, maxfun=400, cap=401)
    assert {"maxls-back", "zoom-lo", "maxls-accept"} <= r.labels and r.stats["knife"] == 0


# ------------------------------------------------------------------------------------------------------------------ (c) branches
def test_every_branch_label_on_the_device():
    stats = lr.new_stats()
    labels = lr.coverage_runs(engine(), stats)
    STATS["steps"] += stats["steps"]
    print("labels:", sorted(labels), "| knife-edge", stats["knife"], "of", stats["steps"])
    assert set(lr.LABELS) <= labels, set(lr.LABELS) - labels
    assert stats["knife"] == 0, stats["why"]


# ------------------------------------------------------------------------------------------------------------------ (d) end results
@pytest.mark.parametrize("n", [2, 10, 100])
def test_rosenbrock_end_result(n):
    r = check_run([lr.rosenbrock], lr.rosen_x0(n), cap=2000)
    ref = scipy.optimize.minimize(scipy.optimize.rosen, lr.rosen_x0(n), jac=scipy.optimize.rosen_der, method="L-BFGS-B",
                                  options=dict(maxcor=10, ftol=1e-15, gtol=1e-8, maxiter=15000, maxfun=15000, maxls=20))
    print(f"n = {n}: status {r.status[0]}, {r.nit[0]} iterations / {r.nfev[0]} evaluations; SciPy {ref.nit} / {ref.nfev}")
    assert r.status[0] in (1, 2)
    assert np.abs(r.x[0] - 1.0).max() <= 1e-6 and np.abs(r.x[0] - ref.x).max() <= 1e-6
    assert ref.nit / 1.5 <= r.nit[0] <= ref.nit * 1.5


@pytest.mark.parametrize("n", [64, 256, 257, 513])
def test_quadratic_end_result(n):
    """(the per-call check runs at n = 64; the larger ones would spend their time in the host's dense n x n reference: their calls are
    checked at the shapes of test_every_call_against_the_reference)"""
    q = lr.quadratic(n, seed=n, centred=True)
    r = lr.drive(engine(), [q], np.zeros((1, n)), 10, lr.QUAD, check=n <= 64, cap=2000, stats=STATS)
    ref = scipy.optimize.minimize(lambda x: q(x)[0], np.zeros(n), jac=lambda x: q(x)[1], method="L-BFGS-B",
                                  options=dict(maxcor=10, ftol=0.0, gtol=1e-8, maxiter=15000, maxfun=15000, maxls=20))
    print(f"n = {n}: status {r.status[0]}, {r.nit[0]} iterations / {r.nfev[0]} evaluations; SciPy {ref.nit} / {ref.nfev}")
    assert r.status[0] == 1
    assert np.abs(r.x[0] - q.xstar).max() <= np.sqrt(n) * lr.QUAD["pgtol"] / q.lam_min
    assert np.abs(r.x[0] - ref.x).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------------------ (e) batch independence
def test_pairs_do_not_depend_on_their_batch():
    """300 pairs (more workgroups than compute units) that stop at different times, no fit around them: pairs 0, 1, 150, 298, 299 alone
    give the same bits"""
    B, n, m = 300, 100, 10
    rng = np.random.default_rng(5)
    funs, x0 = [], np.empty((B, n))
    for b in range(B):
        if b % 2:
            funs.append(lr.rosenbrock)
            x0[b] = lr.rosen_x0(n) + 0.1 * rng.standard_normal(n)
        else:
            funs.append(lr.quadratic(n, seed=1000 + b, cond=10.0 ** (1 + b % 3)))
            x0[b] = rng.uniform(-1, 1, n)
    opts = dict(lr.TIGHT, ftol=1e-10, pgtol=1e-5)
    eng = engine()
    r = lr.drive(eng, funs, x0, m, opts, check=False, cap=3000)
    print("B = 300:", r.evaluations, "evaluations; iterations", r.nit.min(), "..", r.nit.max(), "status", np.bincount(r.status, minlength=6).tolist())
    assert np.isin(r.status, (1, 2)).all() and len(set(r.nfev.tolist())) > 10
    for b in (0, 1, 150, 298, 299):
        r1 = lr.drive(eng, [funs[b]], x0[b:b + 1], m, opts, check=False, cap=3000)
        assert r1.x[0].tobytes() == r.x[b].tobytes() and r1.f[0] == r.f[b], b
        assert (r1.nit[0], r1.nfev[0], r1.status[0]) == (r.nit[b], r.nfev[b], r.status[b]), b


# ------------------------------------------------------------------------------------------------------------------ (f) guards
def test_argument_guards():
    import torch
    from densematcher_amd.engine import _ptr
    eng = engine()
    lib, ctx = eng.lib, eng.ctx
    B, n, m = 2, 5, 3
    buf = lambda k: torch.zeros(k, dtype=torch.float64, device=eng.device)
    state, xt, x0, f, g = buf(int(lib.dm_lbfgs_state_bytes(B, n, m)) // 8 + 1), buf(B * n), buf(B * n), buf(B), buf(B * n)
    info = torch.zeros(B * 4, dtype=torch.int32, device=eng.device)
    null = C.c_void_p(0)
    init = lambda B=B, n=n, m=m, x0=_ptr(x0), st=_ptr(state), xt=_ptr(xt): lib.dm_lbfgs_init(ctx, B, n, m, x0, st, xt)
    adv = lambda B=B, n=n, m=m, st=_ptr(state), f=_ptr(f), g=_ptr(g), xt=_ptr(xt): lib.dm_lbfgs_advance(ctx, B, n, m, st, f, g, xt, 1e-9, 1e-5, 10, 10, 20)
    res = lambda B=B, n=n, m=m, st=_ptr(state), x=_ptr(xt), f=_ptr(f), i=_ptr(info): lib.dm_lbfgs_result(ctx, B, n, m, st, x, f, i)
    assert init() == 0 and adv() == 0 and res() == 0
    before = lr.snapshot(state[:lr.state_bytes(B, n, m) // 8 + 1], B, n, m)
    bad = [dict(m=0), dict(m=65), dict(n=0), dict(B=0)]
    cases = [(init, kw) for kw in bad + [dict(x0=null), dict(st=null), dict(xt=null)]]
    cases += [(adv, kw) for kw in bad + [dict(st=null), dict(f=null), dict(g=null), dict(xt=null)]]
    cases += [(res, kw) for kw in bad + [dict(st=null), dict(x=null), dict(f=null), dict(i=null)]]
    for fn, kw in cases:
        assert init() == 0                                      # (a successful call in between: the message below is this refusal's)
        assert fn(**kw) == lr.EINVAL, kw
        assert lib.dm_last_error(ctx), kw
    for fn in (lib.dm_lbfgs_init, lib.dm_lbfgs_advance, lib.dm_lbfgs_result):
        assert fn(None, *([0] * (len(fn.argtypes) - 1))) == lr.EINVAL
    assert adv() == 0
    after = lr.snapshot(state[:lr.state_bytes(B, n, m) // 8 + 1], B, n, m)
    assert (after.ic[:, lr.LI_NFEV] == 1).all() and (before.ic[:, lr.LI_NFEV] == 1).all()


# ------------------------------------------------------------------------------------------------------------------ (g) both compiled copies
@pytest.mark.parametrize("fused,maxcor", [(True, 12), (True, 13), (False, 32), (False, 33)])
def test_both_compiled_copies_through_the_fit(fx_cfg1, fused, maxcor):
    """the notebook's fit at k = 15 with the history length on either side of the register-resident update's limit (12 inside the fused
    evaluation kernel, 32 in the stand-alone one), against the oracle's tight float64 minimiser of the same problem
    (tests/golden/oracle_cfg1_fit_k15.npz, tools/make_oracle_vectors.py k15: oracle_cfg1_fits' C_nb is the 30 x 30 fit)"""
    import os
    from densematcher_amd.pyFM.functional import LBFGS_OPTIONS
    from oracle import dm_oracle as orc
    fx, k = fx_cfg1, 15
    w = dict(w_descr=1e4, w_lap=1e3, w_ent=1e-1, w_sumto1=1e1)
    x0 = orc.get_x0(k, k, float(fx["Phi1"][0, 0]), float(fx["Phi2"][0, 0]), float(fx["a1"].astype(np.float64).sum()),
                    float(fx["a2"].astype(np.float64).sum()))
    one = {"Phi1": fx["Phi1"][None, :, :k], "Phi2": fx["Phi2"][None, :, :k], "lam1": fx["lam1"][None, :k], "lam2": fx["lam2"][None, :k],
           "a1": fx["a1"][None], "a2": fx["a2"][None], "F1": fx["F1"][None], "F2": fx["F2"][None]}
    Cm, r = engine().fit_general(one, w, x0[None], lbfgs_options=dict(LBFGS_OPTIONS, maxcor=maxcor), fused=fused)
    assert (getattr(r, "path", "") == "fused") == fused
    C_nb = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_cfg1_fit_k15.npz"))["C_nb"]
    err = np.abs(Cm[0] - C_nb).max()
    print(f"fused = {fused}, maxcor = {maxcor}: status {r.status} iterations {r.nit} evaluations {r.nfev} |C - C_oracle| = {err:.2e}")
    assert np.isin(r.status, (1, 2)).all()
    assert err <= 1e-4
    assert np.array_equal(Cm[0][:, 0], x0[:, 0])


# ------------------------------------------------------------------------------------------------------------------ the knife-edge share
def test_knife_edge_share():
    """(last in the module) steps whose discrete outcome lay within the rounding bound of a comparison and was therefore not asserted"""
    print("knife-edge", STATS["knife"], "of", STATS["steps"], "checked steps", sorted(set(STATS["why"])))
    assert STATS["knife"] <= 0.01 * STATS["steps"]

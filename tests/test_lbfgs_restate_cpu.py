"""
CPU: the one-call reference of the device L-BFGS (tests/lbfgs_restate.py) on its own, before it judges the kernel
(tests/test_gpu_lbfgs.py): the dense -H g against the ordinary two-loop recursion, minimisers and iteration counts against SciPy's
L-BFGS-B, the designed status cases whose outcome follows from the contract, and the twelve line-search branches.
"""
import numpy as np
import pytest
import scipy.optimize

import lbfgs_restate as lr

TIGHT, QUAD, BARRIER, ROSEN_X0 = lr.TIGHT, lr.QUAD, lr.BARRIER, lr.rosen_x0
FALLBACK_STARTS, coverage_runs = lr.FALLBACK_STARTS, lr.coverage_runs


def run(funs, x0, m=10, cap=20000, **opts):
    return lr.drive(None, funs, np.atleast_2d(np.asarray(x0, np.float64)), m, dict(TIGHT, **opts), cap=cap)


@pytest.mark.parametrize("m", [1, 3, 10])
@pytest.mark.parametrize("n", [1, 17, 300])
def test_dense_direction_equals_two_loop(n, m):
    """random histories with s^T y > 0 in a wrapped ring buffer (the newest pair in every slot once): 1e-10 relative"""
    rng = np.random.default_rng(100 * n + m)
    S = rng.standard_normal((m, n))
    Y = S * rng.uniform(0.5, 2.0, (m, n)) + 0.05 * rng.standard_normal((m, n)) * (n > 1)
    assert ((S * Y).sum(1) > 0).all()
    g = rng.standard_normal(n)
    for head in range(m):
        for nh in sorted({0, 1, m}):
            rows = lr.live_rows(head, nh, m)
            assert len(rows) == nh and (nh == 0 or rows[-1] == (head - 1) % m)
            dense = lr.dense_direction(S, Y, rows, g)
            tl = lr.two_loop_f64((S, Y, rows), g)
            assert np.abs(tl - dense).max() <= 1e-10 * np.abs(dense).max(), (head, nh)
            assert (g.astype(lr.LD) * dense).sum() < 0


@pytest.mark.parametrize("n", [2, 10, 100])
def test_rosenbrock_against_scipy(n):
    r = run([lr.rosenbrock], ROSEN_X0(n))
    ref = scipy.optimize.minimize(scipy.optimize.rosen, ROSEN_X0(n), jac=scipy.optimize.rosen_der, method="L-BFGS-B",
                                  options=dict(maxcor=10, ftol=1e-15, gtol=1e-8, maxiter=15000, maxfun=15000, maxls=20))
    print(f"n = {n}: status {r.status[0]}, {r.nit[0]} iterations / {r.nfev[0]} evaluations; SciPy {ref.nit} / {ref.nfev}; knife-edge "
          f"{r.stats['knife']} of {r.stats['steps']}")
    assert r.status[0] in (1, 2)
    assert np.abs(r.x[0] - 1.0).max() <= 1e-6 and np.abs(ref.x - 1.0).max() <= 1e-6
    assert ref.nit / 1.5 <= r.nit[0] <= ref.nit * 1.5


@pytest.mark.parametrize("n", [1, 7, 64, 130])
def test_quadratic_reaches_the_minimiser(n):
    """|g|_inf <= pgtol gives |x - x*|_2 <= sqrt(n) pgtol / lambda_min"""
    q = lr.quadratic(n, seed=n, centred=True)
    r = run([q], np.zeros(n), **QUAD)
    assert r.status[0] == 1
    assert np.abs(r.x[0] - q.xstar).max() <= np.sqrt(n) * QUAD["pgtol"] / q.lam_min


def test_designed_status_cases():
    # zero gradient at x0
    zero = lambda x, nit=0: (1.5, np.zeros(x.size))
    r = run([zero], np.ones(5))
    assert (r.status[0], r.nit[0], r.nfev[0]) == (1, 0, 1)
    # max |g| == pgtol exactly
    edge = lambda x, nit=0: (0.0, np.array([0.25, -0.5, 0.125]))
    r = run([edge], np.ones(3), pgtol=0.5)
    assert (r.status[0], r.nit[0], r.nfev[0]) == (1, 0, 1)
    r = run([edge], np.ones(3), pgtol=np.nextafter(0.5, 0.0), maxiter=0)
    assert r.status[0] == 3
    # a NaN gradient at x0 is never "converged"
    nang = lambda x, nit=0: (1.0, np.array([0.0, np.nan, 0.0]))
    r = run([nang], np.ones(3))
    assert (r.status[0], r.nfev[0]) == (5, 1)
    for i in (0, 1, 3):
        r = run([lr.rosenbrock], ROSEN_X0(10), maxiter=i)
        assert (r.status[0], r.nit[0]) == (3, i)


@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_maxfun(k):
    r = run([lr.rosenbrock], ROSEN_X0(10), maxfun=k, cap=k + 1)
    assert r.status[0] != 0 and r.evaluations <= k + 1
    assert r.f[0] == lr.rosenbrock(r.x[0])[0] <= lr.rosenbrock(ROSEN_X0(10))[0]


def test_flipped_quadratic_fails_the_line_search():
    q = lr.quadratic(7, seed=2, origin=0.5)
    x0 = np.full(7, 0.5)
    r = run([lr.flipped(q)], x0, maxls=20)
    assert r.stats["knife"] == 0
    assert (r.status[0], r.nit[0], r.nfev[0]) == (5, 0, 21)
    assert r.x[0].tobytes() == x0.tobytes()
    assert "line-search-fail" in r.labels and "restart" not in r.labels


def test_trap_restarts_once_then_fails():
    seen = []

    def rec(x, nit=0):
        seen.append((nit, x.copy()))
        return lr.rosenbrock(x, nit)
    r = run([lr.trap(rec, 3)], ROSEN_X0(10))
    assert (r.status[0], r.nit[0], r.nhist[0]) == (5, 3, 0)
    assert sum("restart" in c for c in r.trace[0]) == 1 and "line-search-fail" in r.trace[0][-1]
    accepted = [x for nit, x in seen if nit == 2][-1]          # the last point evaluated before the third acceptance is the third iterate
    assert r.x[0].tobytes() == accepted.tobytes()
    assert r.f[0] == lr.rosenbrock(r.x[0])[0]
    assert r.nfev[0] == len(seen) == len([1 for nit, _ in seen if nit < 3]) + 2 * 20


def test_curvature_skip():
    r = run([lr.bump], [[2.0]], maxls=1, maxiter=1)
    assert (r.status[0], r.nit[0], r.nhist[0]) == (3, 1, 0)
    assert r.trace[0][-1] == ["extrapolate", "maxls-accept", "curvature-skip"]
    assert r.x[0, 0] < 2.0 and r.f[0] < lr.bump(np.array([2.0]))[0]


def test_barrier_survives_non_finite_energies():
    fn = lr.barrier(lr.BARRIER_C)
    r = run([fn], np.full(6, 3.0), **BARRIER)
    assert not np.isfinite(r.energies[0]).all(), "no trial left x > 0: the case does not test what it is for"
    assert r.status[0] in (1, 2) and np.abs(r.x[0] - 1.0).max() <= 1e-6


def test_fallback_starts_take_the_documented_branches():
    (n, s, ls), (_, s2, ls2) = FALLBACK_STARTS
    r = run([lr.rosenbrock], [s], maxls=ls, maxfun=400)
    assert {"maxls-back", "curvature-skip"} <= r.labels
    r = run([lr.rosenbrock], [s2], maxls=ls2, maxfun=400)
    assert {"maxls-back", "zoom-lo", "maxls-accept"} <= r.labels


def test_every_branch_label_occurs():
    stats = lr.new_stats()
    labels = coverage_runs(None, stats)
    print("labels:", sorted(labels), "| knife-edge", stats["knife"], "of", stats["steps"])
    assert set(lr.LABELS) <= labels, set(lr.LABELS) - labels
    assert stats["knife"] == 0


STEP_STATS = lr.new_stats()


@pytest.mark.parametrize("n,m", list(lr.STEP_SHAPES))
def test_single_step_inputs_end_within_the_cap(n, m):
    """the inputs of the device's single-step check, run by the reference alone: every run ends within the 120 evaluations"""
    funs, x0, opts = lr.step_problem(n, m)
    r = lr.drive(None, funs, x0, m, opts, cap=120, stats=STEP_STATS)
    print(f"(n, m) = ({n}, {m}): status {r.status.tolist()} iterations {r.nit.tolist()} evaluations {r.nfev.tolist()}")
    assert (r.status != 0).all()
    if m < 10 and n > 1:
        assert r.nit.max() > 2 * m, "the ring buffer does not wrap"


def test_single_step_inputs_stay_clear_of_knife_edges():
    """... and at most 1 % of the steps above have a decision within the rounding bound of its operands"""
    print("knife-edge", STEP_STATS["knife"], "of", STEP_STATS["steps"])
    assert STEP_STATS["knife"] <= 0.01 * STEP_STATS["steps"]

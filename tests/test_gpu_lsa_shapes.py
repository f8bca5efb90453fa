"""GPU (-m gpu): dm_linear_sum_assignment and dm_lsa_indicator (csrc/dm_assign.hip) against scipy.optimize.linear_sum_assignment at
every kernel shape lsa_run dispatches to -- the whole col_of_row array, ties included, never only the objective.

  a. each side of every dispatch boundary in SciPy's order: lsa_reg_kernel with 1 | 2 | 4 | 8 columns per thread at 512 threads
     (boundaries 512, 1024, 2048, 4096 columns), 8 at 1024 threads (the fold steps compiled in for more than 8 waves; list position
     and column index up to 8191 in the tie key), lsa_kernel past 8192 columns, and with lsa_reg = 0 its column state in the LDS
     (up to 4608 columns) or in global memory; tall matrices (transposition, inversion, unassigned rows).  Inputs:
     lsa_cases.contention -- tests/test_lsa_cases_cpu.py shows that a wrong tie rule or a stale list position changes the result
     on the integer matrix of every counted shape.
  b. square matrices: the column-reduction start, the uniqueness check and the rerun (lsa_reg = 2) at 2 | 4 | 8 columns per
     thread and at 1024 threads, on a matrix whose optimum is unique (the start is kept), one with planted exact ties (the start
     runs and must be rejected) and two the start steps aside from.
  c. the factor form (KP = 16 | 32) with 2 and 4 columns per thread: the assignment of the dense matrix dm_mapped_indicator forms
     from the same factors, by SciPy and by dm_linear_sum_assignment.

The expected value is SciPy's, computed in the test.  Not covered: the register path's own LDS limit (12 R + 8 Cn + 64 > 150 KiB,
first crossed at 7334 x 8192 -- too large for a test); the kernel it falls back to is the one the 8193-column cases run."""
import time

import numpy as np
import pytest
import torch

import lsa_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _engine():
    from densematcher_amd.engine import MatchEngine
    return MatchEngine()


@pytest.fixture
def eng(_engine):
    yield _engine
    _engine.reset_options()


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


def _assign(eng, mats, mx):
    return eng.linear_sum_assignment(np.stack(mats), maximize=mx).cpu().numpy()


def _check_batch(eng, mats, mx, modes, names, what):
    """one batch, every implementation, against SciPy on each matrix"""
    want = [lc.scipy_col_of_row(m, mx) for m in mats]
    for mode in modes:
        eng.set_option("lsa_reg", mode)
        got = _assign(eng, mats, mx)
        assert got.shape == (len(mats), mats[0].shape[0]) and got.dtype == np.int32
        for q, name in enumerate(names):
            np.testing.assert_array_equal(got[q], want[q], err_msg=f"{what} {name} maximize={mx} lsa_reg={mode}")


# ---- a. each side of every dispatch boundary, SciPy's order ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.WIDE + lc.TALL, ids=_id)
def test_each_side_of_a_dispatch_boundary(eng, shape):
    """the four kinds of one shape as one batch, both senses, lsa_reg = 2 (the register kernel in SciPy's order: not square, no
    warm start), 1 and 0"""
    mats = lc.contention_batch(*shape)
    for mx in (False, True):
        _check_batch(eng, [lc.oriented(m, kind, mx) for kind, m in zip(lc.KINDS, mats)], mx, (2, 1, 0), lc.KINDS, shape)


@pytest.mark.parametrize("shape", lc.WIDE_LDS, ids=_id)
def test_list_kernel_each_side_of_its_lds_limit(eng, shape):
    """lsa_reg = 0: lsa_kernel keeps v, the tentative costs, the path, the owners and the list in the LDS up to 4608 columns"""
    mats = lc.contention_batch(*shape)
    for mx in (False, True):
        _check_batch(eng, [lc.oriented(m, kind, mx) for kind, m in zip(lc.KINDS, mats)], mx, (0,), lc.KINDS, shape)


# ---- b. warm start, uniqueness check and rerun at every register shape -----------------------------------------------------------
def _planted_for(n, mx):
    """the planted matrix in the sense its ties are real for: minimise c, maximise -c"""
    c = lc.planted(5, n)[0]
    return -c if mx else c


@pytest.mark.parametrize("n", (520, 1025, 2049))
def test_warm_start_check_and_rerun(eng, n):
    """square: lsa_reg = 2 takes the column-reduction start where the matrix allows it and keeps the result only when no second
    optimum exists.  planted: the start runs, the check must reject it, the rerun restores SciPy's choice; generic: the start is
    kept; round(3 c) and two constant columns (n <= 1025): the start steps aside.  lsa_reg = 0 stops at 1025 (lsa_kernel is the
    slow path on a square matrix)."""
    modes = (2, 1, 0) if n <= 1025 else (2, 1)
    for mx in (False, True):
        mats, names = [_planted_for(n, mx), lc.square_generic(n)], ["planted", "generic"]
        if n <= 1025:
            mats += [lc.square_integer(n), lc.square_two_constant_columns(n)]
            names += ["round(3 c)", "two constant columns"]
        _check_batch(eng, mats, mx, modes, names, n)


def test_warm_start_check_and_rerun_4097(eng):
    """1024 threads with R == Cn: the smallest square that reaches them.  One planted and one generic matrix as one batch;
    lsa_reg = 2 minimising, lsa_reg = 1 maximising."""
    n = 4097
    spent = 0.0
    for mode, mx in ((2, False), (1, True)):
        mats = [_planted_for(n, mx), lc.square_generic(n)]
        want = [lc.scipy_col_of_row(m, mx) for m in mats]
        eng.set_option("lsa_reg", mode)
        dev = eng._dev(np.stack(mats), torch.float64, "cost")
        eng.synchronize()
        t0 = time.perf_counter()
        got = eng.linear_sum_assignment(dev, maximize=mx).cpu().numpy()
        dt = time.perf_counter() - t0
        spent += dt
        print(f"4097 x 4097, batch of 2, lsa_reg={mode} maximize={mx}: {dt:.3f} s on the GPU")
        for q, name in enumerate(("planted", "generic")):
            np.testing.assert_array_equal(got[q], want[q], err_msg=f"{name} maximize={mx} lsa_reg={mode}")
    print(f"4097 x 4097: {spent:.3f} s on the GPU in all")


# ---- c. the factor form past one column per thread -------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("k", (15, 30))
@pytest.mark.parametrize("short", (0, 37))
@pytest.mark.parametrize("N1", (600, 1100, 2048))
def test_factor_form_past_one_column_per_thread(eng, N1, short, k, dt):
    """dm_lsa_indicator[_f64]: psi[CPT][KP] with CPT = 2 (600, 1100) | 4 (2048), KP = 16 | 32; N2 = N1 (warm start, the factor
    form's uniqueness check, rerun) and N2 = N1 - 37 (SciPy's order at once).  The second indicator has two duplicated vertices
    in mesh 1 -- two pairs of identical columns, an optimum that is not unique; a dense random matrix rides in the same launch."""
    N2 = N1 - short
    P1, P2, a1, C, pairs = lc.indicator_factors(1000 * N1 + 10 * k + short, N1, N2, k, dt)
    assert eng.lsa_indicator_ok(N1, N2, k, k)
    dense_dev = eng.mapped_indicator(P1, P2, a1, C)
    dense = dense_dev.cpu().numpy()
    for s, d in pairs:
        assert np.array_equal(dense[1][:, s], dense[1][:, d])
    extra = np.random.default_rng(N1 + k).standard_normal((1, N2, N1))
    got = eng.lsa_indicator(P1, P2, a1, C, dense=extra).cpu().numpy()
    assert got.shape == (3, N2) and got.dtype == np.int32
    for b in range(2):
        np.testing.assert_array_equal(got[b], lc.scipy_col_of_row(dense[b], True), err_msg=f"indicator {b}")
    np.testing.assert_array_equal(got[2], lc.scipy_col_of_row(extra[0], True), err_msg="the dense matrix riding along")
    np.testing.assert_array_equal(got[:2], eng.linear_sum_assignment(dense_dev, maximize=True).cpu().numpy())


def test_factor_form_stops_at_2048_columns(eng):
    P1, P2, a1, C, _ = lc.indicator_factors(9, 2049, 2049, 15, np.float64)
    assert not eng.lsa_indicator_ok(2049, 2049, 15, 15) and eng.lsa_indicator_ok(2048, 2048, 15, 15)
    with pytest.raises(ValueError):
        eng.lsa_indicator(P1, P2, a1, C)

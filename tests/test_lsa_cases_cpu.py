"""CPU: the inputs of tests/test_gpu_lsa_shapes.py can see the faults they are there for (tests/lsa_cases.py).

A search kernel that tracks a list position wrongly, folds one wave slot too few or breaks a tie the wrong way still returns a
valid and usually optimal assignment; it differs from scipy.optimize.linear_sum_assignment only where the list bookkeeping decides
the result.  Here, without a GPU: the restatement `lsa_steps` is SciPy's search (same assignment, both senses, every case); the
events that exercise the bookkeeping occur often in every counted case; and each wrong variant of `lsa_steps` returns another
assignment on every integer case -- so a kernel with that fault cannot pass the comparison with SciPy.

The event bounds are conditions on the inputs, fixed before any seed was chosen: per case at least 50 selections of a column that had
been moved inside the list and a longest search of at least 30 steps (generic and integer kinds); on the integer kind at least 200
steps with a tie at the minimum, 150 of them between columns of different waves and 50 won by a column that is not the first in scan
order.  Measured over the counted cases with the seeds of lsa_cases.SEEDS: 75-282 / 56-161 moved-then-selected (generic / integer),
longest search 46-79, 261-658 tie steps, 235-629 across waves, 54-109 not won by the first.

What the wrong variants cannot show: on the generic kind no two unassigned columns ever tie (continuous data: 0 steps of
`tie_not_first` in every case), the ties that do occur are between assigned columns at the same tentative cost, and whichever of
those is taken first the other follows at the same value -- so neither variant changes a generic case's assignment (none of the 17
does).  A wrong list position is visible in the integer cases only; both variants are asserted there."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import lsa_cases as lc


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


@pytest.fixture(scope="module")
def solved():
    """lsa_steps on the generic and the integer matrix of a shape (minimising), computed once per shape"""
    cache = {}

    def get(shape):
        if shape not in cache:
            mats = lc.contention_batch(*shape)
            cache[shape] = {kind: lc.lsa_steps(mats[lc.KINDS.index(kind)]) for kind in ("generic", "integer")}
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", lc.SHAPES, ids=_id)
def test_restatement_is_scipy(shape):
    """every kind, both senses: the whole col_of_row array, -1 rows of the tall cases included"""
    for kind, m in zip(lc.KINDS, lc.contention_batch(*shape)):
        for mx in (False, True):
            mm = lc.oriented(m, kind, mx)
            got, _ = lc.lsa_steps(mm, maximize=mx)
            np.testing.assert_array_equal(got, lc.scipy_col_of_row(mm, mx), err_msg=f"{shape} {kind} maximize={mx}")
    if shape[0] > shape[1]:
        assert (lc.scipy_col_of_row(lc.contention_batch(*shape)[0]) == -1).sum() == shape[0] - shape[1]


def test_the_table_has_each_side_of_every_dispatch_boundary():
    """columns per thread 1 | 2 | 4 | 8 at 512 threads, 8 at 1024, past the register path; lsa_kernel's LDS limit; tall cases;
    every shape has a seed and every counted shape has at least 96 rows"""
    cols = {max(s) for s in lc.SHAPES}
    assert {512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 4608, 4609} <= cols
    assert (160, 8192) in lc.WIDE and {(1025, 96), (4097, 96), (8193, 64)} <= set(lc.TALL)
    assert set(lc.SEEDS) == set(lc.SHAPES) and len(set(lc.SHAPES)) == len(lc.SHAPES)
    assert set(lc.SHAPES) - set(lc.COUNTED) == {(8193, 64)} and (8193, 96) in lc.COUNTED
    assert lc.threads_for(4096) == 512 and lc.threads_for(4097) == 1024


@pytest.mark.parametrize("shape", lc.COUNTED, ids=_id)
def test_events_that_exercise_the_list_occur_often(solved, shape):
    for kind in ("generic", "integer"):
        cnt = solved(shape)[kind][1]
        print(shape, kind, cnt)
        assert cnt["moved_selected"] >= 50 and cnt["longest"] >= 30, (shape, kind, cnt)
    cnt = solved(shape)["integer"][1]
    assert cnt["tie_steps"] >= 200 and cnt["tie_cross_wave"] >= 150 and cnt["tie_not_first"] >= 50, (shape, cnt)
    assert cnt["tie_cross_wave"] <= cnt["tie_steps"] <= cnt["steps"] and cnt["longest"] <= min(shape)


@pytest.mark.parametrize("shape", lc.COUNTED, ids=_id)
def test_each_wrong_variant_is_seen_on_the_integer_case(solved, shape):
    m = lc.contention_batch(*shape)[lc.KINDS.index("integer")]
    right = solved(shape)["integer"][0]
    np.testing.assert_array_equal(right, lc.scipy_col_of_row(m))
    first, _ = lc.lsa_steps(m, tie_rule="first")
    stale, _ = lc.lsa_steps(m, track_moves=False)
    for name, wrong in (("tie_rule=first", first), ("track_moves=False", stale)):
        assert not np.array_equal(wrong, right), (shape, name)
        # (still a complete assignment of the same value: no objective could tell)
        rows = np.flatnonzero(wrong >= 0)
        assert len(set(wrong[rows].tolist())) == len(rows) == min(shape)
        assert m[rows, wrong[rows]].sum() == m[np.flatnonzero(right >= 0), right[right >= 0]].sum(), (shape, name)


def test_wave_of_a_column_follows_the_workgroup_size():
    """two tied columns 512 apart: one wave at 512 threads, two at 1024"""
    c = np.ones((1, 1024))
    c[0, [3, 515]] = 0.0
    assert lc.lsa_steps(c, nt=512)[1]["tie_cross_wave"] == 0 and lc.lsa_steps(c, nt=1024)[1]["tie_cross_wave"] == 1
    got, cnt = lc.lsa_steps(c, nt=512)
    assert got[0] == 3 and cnt["tie_steps"] == 1 and cnt["tie_not_first"] == 1      # the LAST unassigned one: column 3 comes after 515
    assert lc.lsa_steps(c, tie_rule="first")[0][0] == 515


# ---- square matrices with planted ties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lc.SQUARE_N)
def test_planted_ties_are_real_and_the_warm_start_still_runs(n):
    """the rotated assignments have exactly the optimum's value (entries are multiples of 2^-20: the sums are exact), and the
    matrix passes the condition under which the kernel keeps its column-reduction start, in the sense the ties were planted for
    (minimise c, or maximise -c): the warm start runs, the uniqueness check must reject it, the rerun must restore SciPy's choice"""
    c, two, three, col = lc.planted(5, n)
    assert np.array_equal(c * 2.0 ** 20, np.round(c * 2.0 ** 20))
    assert len(set(two.tolist()) | set(three.tolist())) == 5
    r, best = linear_sum_assignment(c)
    opt = c[r, best].sum()
    idx = np.arange(n)
    for alt in (col, lc.rotated(col, two), lc.rotated(col, three), lc.rotated(lc.rotated(col, two), three)):
        assert np.array_equal(np.sort(alt), idx)
        assert c[idx, alt].sum() == opt
    assert not np.array_equal(lc.rotated(col, two), col) and not np.array_equal(lc.rotated(col, three), col)
    assert lc.warm_start_accepts(c) and lc.warm_start_accepts(-c, maximize=True)


@pytest.mark.parametrize("n", (520, 1025))
def test_which_square_matrices_the_warm_start_steps_aside_from(n):
    assert lc.warm_start_accepts(lc.square_generic(n)) and lc.warm_start_accepts(lc.square_generic(n), maximize=True)
    assert not lc.warm_start_accepts(lc.square_integer(n))                       # most column minima are attained more than once
    assert not lc.warm_start_accepts(lc.square_two_constant_columns(n))          # two constant columns


def test_indicator_factors_have_the_duplicated_vertices():
    P1, P2, a1, C, pairs = lc.indicator_factors(3, 600, 563, 15, np.float32)
    assert P1.shape == (2, 600, 15) and P2.shape == (2, 563, 15) and a1.shape == (2, 600) and C.shape == (2, 15, 15)
    assert P1.dtype == np.float32 and C.dtype == np.float64 and len(pairs) == 2
    M = np.einsum("nk,kl,ml->nm", P2[1].astype(np.float64), C[1], P1[1].astype(np.float64)) * a1[1].astype(np.float64)[None, :]
    for s, d in pairs:
        assert s != d and np.array_equal(M[:, s], M[:, d]) and not np.array_equal(P1[0, s], P1[0, d])
    assert np.abs(P2[0].astype(np.float64).T @ P2[0].astype(np.float64) - np.eye(15)).max() < 1e-5

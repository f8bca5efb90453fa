"""Inputs for the linear-assignment tests (csrc/dm_assign.hip) and a counting restatement of SciPy's search.  NumPy and SciPy only:
tests/test_lsa_cases_cpu.py shows that these inputs can see a wrong tie rule or a wrong list position, tests/test_gpu_lsa_shapes.py
runs them through the kernels.

The register kernel (lsa_reg_kernel<CPT, WARM, NT, KP>) never stores SciPy's `remaining` list: a thread keeps the list position of
each column it owns and patches it when the column at the last position is moved into a vacated place; the tie order is one integer
per candidate, folded inside a wave and then across the NT / 64 wave slots.  A fault in any of that still yields an optimal
assignment unless the input makes the list bookkeeping decide the result: many rows competing for few columns (long searches,
columns at the low indices -- the END of SciPy's reversed list -- moved and then selected) and exact ties between columns of
different waves.  `contention` builds such inputs, `lsa_steps` counts how often each event occurs in them."""
import functools

import numpy as np
from scipy.optimize import linear_sum_assignment

KINDS = ("generic", "integer", "sparse", "inf")


def threads_for(ncols):
    """workgroup size lsa_run gives a search over `ncols` columns (the larger side): 512 up to 4096 columns, else 1024"""
    return 512 if ncols <= 4096 else 1024


def lsa_steps(cost, maximize=False, nt=None, tie_rule="scipy", track_moves=True):
    """scipy.optimize.linear_sum_assignment (rectangular_lsap: Crouse's shortest augmenting paths) restated with a Python loop over
    the steps and a NumPy scan inside a step.  A step relaxes  r = ((min_val + c_ij) - u_i) - v_j  over the `remaining` columns in
    list order (the list starts reversed; the chosen entry is removed by moving the last one into its place) and selects the
    smallest tentative cost: the first column in scan order at the minimum, unless unassigned columns are among the tied, then the
    last unassigned one.  More rows than columns: the transposed problem is solved, as SciPy does.

    Returns (col_of_row, counters): col_of_row (nr,) with -1 for an unassigned row; counters (of the problem as solved, i.e. after the
    transposition; a "wave" of column j is (j mod nt) // 64, the wave of the thread that owns it in the register kernel):
      steps            all search steps            longest       the longest search
      tie_steps        steps where at least two columns tie at the minimum
      tie_cross_wave   ... of those, the tied columns lie in more than one wave
      tie_not_first    ... of those, the winner is not the first tied column in scan order
      moved_selected   selected columns that had been moved inside the list earlier in the same search

    Wrong variants, for showing that an input can see the fault:
      tie_rule="first"    always the first tied column in scan order
      track_moves=False   a moved column keeps its old place in the scan order (the scan runs over the open columns in the
                          order of their initial positions)"""
    c = np.array(cost, dtype=np.float64)
    if maximize:
        c = -c
    transposed = c.shape[0] > c.shape[1]
    if transposed:
        c = np.ascontiguousarray(c.T)
    nr, nc = c.shape
    nt = threads_for(nc) if nt is None else nt
    wave = (np.arange(nc) % nt) // 64
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    path = np.full(nc, -1, np.int64)
    cnt = dict(steps=0, longest=0, tie_steps=0, tie_cross_wave=0, tie_not_first=0, moved_selected=0)
    for cur in range(nr):
        spc = np.full(nc, np.inf)
        remaining = np.arange(nc - 1, -1, -1)
        moved = np.zeros(nc, bool)
        visited_rows, scanned = [], []
        nrem, min_val, sink, i, steps = nc, 0.0, -1, cur, 0
        while sink == -1:
            visited_rows.append(i)
            js = remaining[:nrem] if track_moves else np.sort(remaining[:nrem])[::-1]
            r = ((min_val + c[i, js]) - u[i]) - v[js]
            better = r < spc[js]
            jb = js[better]
            spc[jb] = r[better]
            path[jb] = i
            s = spc[js]
            lowest = s.min()
            if not np.isfinite(lowest):
                raise ValueError("cost matrix is infeasible")
            tied = np.flatnonzero(s == lowest)               # positions in scan order
            free = tied[row4col[js[tied]] == -1]
            index = int(free[-1]) if (tie_rule == "scipy" and free.size) else int(tied[0])
            j = int(js[index])
            steps += 1
            if tied.size >= 2:
                cnt["tie_steps"] += 1
                cnt["tie_cross_wave"] += int(np.unique(wave[js[tied]]).size > 1)
                cnt["tie_not_first"] += int(index != tied[0])
            cnt["moved_selected"] += int(moved[j])
            min_val = lowest
            if row4col[j] == -1:
                sink = j
            else:
                i = int(row4col[j])
            scanned.append(j)
            nrem -= 1
            at = index if track_moves else int(np.flatnonzero(remaining[:nrem + 1] == j)[0])
            if at != nrem:
                moved[remaining[nrem]] = True
            remaining[at] = remaining[nrem]
        cnt["steps"] += steps
        cnt["longest"] = max(cnt["longest"], steps)
        u[cur] += min_val
        for i2 in visited_rows[1:]:
            u[i2] += min_val - spc[col4row[i2]]
        sc = np.asarray(scanned)
        v[sc] -= min_val - spc[sc]
        j = sink
        while True:
            i2 = path[j]
            row4col[j] = i2
            col4row[i2], j = j, col4row[i2]
            if i2 == cur:
                break
    if transposed:
        return row4col.astype(np.int32), cnt
    return col4row.astype(np.int32), cnt


def scipy_col_of_row(cost, maximize=False):
    """SciPy's assignment in the layout the engine returns: (nr,) int32, -1 for a row left unassigned"""
    r, c = linear_sum_assignment(cost, maximize=maximize)
    out = np.full(cost.shape[0], -1, np.int32)
    out[r] = c
    return out


def contention(rng, nr, nc, kind):
    """nr x nc (wide: nr < nc; tall: the transpose of the wide nc x nr case), many rows after few columns:
    cost = pref[None, :] + N(0, 1) with pref = -4 on the first h = min(nr, nc) // 6 columns, the last h and h random ones.  The low
    column indices sit at the end of SciPy's reversed list: they are the ones moved into vacated places, and being wanted they are
    selected afterwards.  kind: "generic"; "integer" round(2 cost) -- ties at every step; "sparse" 98 % exact zeros; "inf" 2 % +inf
    with one finite entry per row kept in a column of its own, so an assignment exists."""
    if nr > nc:
        return np.ascontiguousarray(contention(rng, nc, nr, kind).T)
    h = nr // 6
    pref = np.zeros(nc)
    pref[:h] = -4.0
    pref[nc - h:] = -4.0
    pref[rng.permutation(np.arange(h, nc - h))[:h]] = -4.0
    cost = pref[None, :] + rng.standard_normal((nr, nc))
    if kind == "integer":
        cost = np.round(2.0 * cost)
    elif kind == "sparse":
        cost = cost * (rng.random((nr, nc)) < 0.02)
    elif kind == "inf":
        hole = rng.random((nr, nc)) < 0.02
        hole[np.arange(nr), rng.permutation(nc)[:nr]] = False
        cost[hole] = np.inf
    elif kind != "generic":
        raise ValueError(kind)
    return cost


def oriented(cost, kind, maximize):
    """the matrix handed to a solver for one sense.  SciPy rejects +inf when maximising ("invalid numeric entries"), so the "inf"
    kind is negated for that sense: -inf marks its forbidden entries there.  Every other kind goes in as it is."""
    return -cost if (kind == "inf" and maximize) else cost


# ---- the case tables (shared by the CPU and the GPU tests) ---------------------------------------------------------------------
# columns of the search at each side of every dispatch boundary of lsa_run: columns per thread 1 | 2 | 4 | 8 at 512 threads,
# 8 at 1024 threads, past the register path (8192); 160 rows at 8192 where the key fields are fullest
WIDE = [(96, 512), (96, 513), (96, 1024), (96, 1025), (96, 2048), (96, 2049), (96, 4096), (96, 4097), (96, 8192), (160, 8192), (96, 8193)]
WIDE_LDS = [(96, 4608), (96, 4609)]          # lsa_reg = 0 only: lsa_kernel's column state in the LDS | in global memory
TALL = [(1025, 96), (4097, 96), (8193, 64), (8193, 96)]  # lsa_transpose, lsa_invert, unassigned rows
SHAPES = WIDE + WIDE_LDS + TALL
# 64 x 8193 is too small for the event counts tests/test_lsa_cases_cpu.py asks of a case (its searches total some 230 steps): it stays
# as a shape for the kernels, and 96 x 8193 stands beside it as the case that is shown to see the faults
COUNTED = [s for s in SHAPES if min(s) >= 96]

# One seed per shape.  Where 1000 nr + nc did not meet every condition of tests/test_lsa_cases_cpu.py (event counts, and both wrong
# variants of lsa_steps returning another assignment on the integer matrix) 100000 was added until one did.
SEEDS = {(96, 512): 96512, (96, 513): 96513, (96, 1024): 197024, (96, 1025): 497025, (96, 2048): 298048, (96, 2049): 498049,
         (96, 4096): 600096, (96, 4097): 300097, (96, 8192): 1504192, (160, 8192): 468192, (96, 8193): 1204193, (96, 4608): 800608,
         (96, 4609): 700609, (1025, 96): 1025096, (4097, 96): 4297096, (8193, 64): 8193064, (8193, 96): 8593096}


@functools.lru_cache(maxsize=None)
def contention_batch(nr, nc):
    """the four kinds of one shape, in KINDS' order, read-only"""
    rng = np.random.default_rng(SEEDS[(nr, nc)])
    out = []
    for kind in KINDS:
        m = contention(rng, nr, nc, kind)
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


# ---- square matrices with planted ties -------------------------------------------------------------------------------------------
def _exact_duals(c, col):
    """optimal duals (u, v) of the assignment row i -> col[i] of the square matrix c: u is the fixed point of
    u_i = max_k (u_k + c_i,col[i] - c_k,col[i]), reached by sweeps that propagate only from the rows that changed last, and
    v_col[i] = c_i,col[i] - u_i.  Exact when the entries are multiples of a power of two."""
    n = c.shape[0]
    M = c[:, col]
    d = M[np.arange(n), np.arange(n)].copy()
    u = np.zeros(n)
    changed = np.arange(n)
    for _ in range(n + 1):
        if changed.size == 0:
            v = np.empty(n)
            v[col] = d - u
            assert ((c - u[:, None]) - v[None, :]).min() == 0.0
            return u, v
        cand = ((u[changed, None] + d[None, :]) - M[changed, :]).max(axis=0)
        new = cand > u
        u[new] = cand[new]
        changed = np.flatnonzero(new)
    raise RuntimeError("the assignment is not optimal")


@functools.lru_cache(maxsize=None)
def planted(seed, n):
    """n x n, entries N(0, 1) quantised to multiples of 2^-20 (every sum below is exact), solved once with SciPy (minimising); then
    one 2-cycle and one 3-cycle of assigned pairs are made exactly interchangeable: the off-assignment entries of the cycle
    (row i_a, column of i_a+1) are overwritten with u_i + v_j of optimal duals, so they have no slack, the assignment stays optimal
    and the rotated assignment has the same total.  Returns (matrix, rows of the 2-cycle, rows of the 3-cycle, the assignment SciPy
    gave before the overwrite); read-only."""
    rng = np.random.default_rng(seed)
    c = np.round(rng.standard_normal((n, n)) * 2.0 ** 20) / 2.0 ** 20
    col = linear_sum_assignment(c)[1]
    u, v = _exact_duals(c, col)
    rows = rng.permutation(n)[:5]
    two, three = rows[:2], rows[2:]
    for cyc in (two, three):
        for a in range(len(cyc)):
            i, j = cyc[a], col[cyc[(a + 1) % len(cyc)]]
            c[i, j] = u[i] + v[j]
    for x in (c, two, three, col):
        x.setflags(write=False)
    return c, two, three, col


def rotated(col, cyc):
    """the assignment with the rows of `cyc` taking each other's columns in a circle"""
    out = col.copy()
    for a in range(len(cyc)):
        out[cyc[a]] = col[cyc[(a + 1) % len(cyc)]]
    return out


def warm_start_accepts(c, maximize=False):
    """the condition under which lsa_reg_kernel<.., WARM = 1, ..> keeps its column-reduction start: at most nc / 8 columns whose
    minimum is attained more than once, fewer than two constant columns"""
    c = -c if maximize else c
    nr, nc = c.shape
    cnt = (c == c.min(axis=0)[None, :]).sum(axis=0)
    return int((cnt >= 2).sum()) * 8 <= nc and not (int((cnt == nr).sum()) >= 2 and nr >= 2)


SQUARE_N = (520, 1025, 2049, 4097)


@functools.lru_cache(maxsize=None)
def square_generic(n):
    m = np.random.default_rng(77 + n).standard_normal((n, n))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def square_integer(n):
    m = np.round(3.0 * np.random.default_rng(78 + n).standard_normal((n, n)))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def square_two_constant_columns(n):
    m = np.random.default_rng(79 + n).standard_normal((n, n))
    m[:, [0, n - 1]] = 0.25
    m.setflags(write=False)
    return m


# ---- mapped indicators by their factors ------------------------------------------------------------------------------------------
def indicator_factors(seed, N1, N2, k, dtype):
    """two indicators Phi2 C Phi1^T diag(a1) by their factors: orthonormalised Gaussian columns, a1 uniform in [0.5, 1.5] / N1,
    C = I + 0.05 noise.  The second one has two duplicated vertices in mesh 1 (a row of Phi1 and its a1 entry copied onto another
    vertex, twice): two pairs of identical columns, so its optimum is not unique.  Returns Phi1 (2, N1, k), Phi2 (2, N2, k),
    a1 (2, N1) in `dtype`, C (2, k, k) float64 and the duplicated pairs."""
    rng = np.random.default_rng(seed)
    P1 = np.stack([np.linalg.qr(rng.standard_normal((N1, k)))[0] for _ in range(2)])
    P2 = np.stack([np.linalg.qr(rng.standard_normal((N2, k)))[0] for _ in range(2)])
    a1 = rng.uniform(0.5, 1.5, (2, N1)) / N1
    C = np.eye(k)[None] + 0.05 * rng.standard_normal((2, k, k))
    v = rng.permutation(N1)[:4]
    pairs = [(int(v[0]), int(v[1])), (int(v[2]), int(v[3]))]
    for src, dst in pairs:
        P1[1, dst] = P1[1, src]
        a1[1, dst] = a1[1, src]
    return P1.astype(dtype), P2.astype(dtype), a1.astype(dtype), C, pairs

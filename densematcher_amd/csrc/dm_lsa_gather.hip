// Many ragged linear assignments gathered from one matrix (dm_lsa_gather): the semantic group distances of the reference.
//
// Reference call reproduced: densematcher/utils.py:115-143 (get_distance_between_groups / get_groups_dmtx): for every pair of
// vertex groups  scipy.optimize.linear_sum_assignment(D[np.ix_(g_i, g_j)])  and the mean of the matched entries.  A mesh with G
// groups gives G (G - 1) / 2 problems of tens to a few hundred rows, each of another shape, their entries scattered through D.
//
// One WAVEFRONT per problem, LG_WPB problems per workgroup, no workgroup barrier anywhere: the waves of a workgroup never wait
// for each other.  The search is lsa_reg_body's (dm_assign.hip) cut down to one wave: SciPy's shortest augmenting paths with
// rows in order, the column state (dual v, tentative cost, predecessor, owner, position in SciPy's `remaining` list, address
// offset of the column in D) in registers, CPL columns per lane, the short side's duals and lists in the wave's LDS slice, the
// arg-min of a step by the DPP reductions of dm_lsa_dev.h.  Same scan order, tie rules and operation order of the reduced cost
// as SciPy: the assignment is SciPy's, ties included.  A problem's state never leaves its wave, so its bits do not depend on
// what else shares the call.
//
// Orientation: SciPy solves the transposed problem when nr > nc; so does this kernel (short side R = min, long side Cn = max).
// A search step reads S[i][:] over the long side.  Untransposed that is a gather along ONE row of D (neighbouring lanes read
// nearby columns).  Transposed it would walk down a column of D, a cache line per lane and step: such a problem's block is
// gathered ONCE into context scratch as an R x Cn matrix (lg_block_kernel, coalesced reads, transposed through LDS) and the
// search reads that copy -- while the copies of a call fit the budget (below); a problem past it searches D directly, same bits.
//
// A long side above 64 LG_MAX_CPL = 1024 does not fit one wave: its block is gathered the same way and handed to lsa_run
// (dm_assign.hip, one workgroup of 512 or 1024 threads per matrix), one problem after the other through one buffer.
//
// Work order: the host sorts the table by work (R^2 Cn) descending; workgroups start in index order, so the long searches start
// first and the short ones fill in behind them.  One launch serves every problem up to 1024 columns: the kernel is instantiated
// for the widest class the call contains (MAXC) and a wave picks the body of its own problem's class.
#include <algorithm>
#include <cmath>

#include "dm_device.h"
#include "dm_internal.h"
#include "dm_lsa_dev.h"

constexpr int LG_WPB = 4;            // problems (wavefronts) per workgroup
constexpr int LG_MAX_CPL = 16;       // columns per lane of the widest one-wave body: 1024 columns
constexpr int LG_SLICE = 24;         // LDS bytes per column of a wave's slice: u (8) | row4col, path, col4row, sidx (4 each)

struct lg_prob {
    int b, roff, nr, coff, nc, ooff, p, cls;     // p: the problem's index in the caller's table; cls: log2 of its columns per lane, -1 = wide
    long long stage;                             // element offset of its gathered R x Cn block in the scratch, -1: none
};

__device__ __forceinline__ void lg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int lg_uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ double lg_lane_f64(double x, int k) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), k), __builtin_amdgcn_readlane(__double2loint(x), k));
}
// value(0) + value(1) + ... + value(n - 1) folded left to right (the order of a sequential sum), the same in every lane: the
// values of 64 consecutive k are fetched in parallel, then added in order.  value(k) returns 0.0 for an entry that is left out.
template <typename F>
__device__ __forceinline__ double lg_ordered_sum(int n, int lane, F&& value) {
    double s = 0.0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const double x = k < n ? value(k) : 0.0;
        const int m = n - k0 < 64 ? n - k0 : 64;
        for (int kk = 0; kk < m; ++kk) s += lg_lane_f64(x, kk);
    }
    return s;
}

// one problem on one wave; `sl`: the wave's LDS slice (LG_SLICE * 64 * CPL bytes)
template <int CPL>
__device__ __forceinline__ void lg_search(unsigned char* sl, const lg_prob& pr, const double* __restrict__ D, int N, long long ld,
                                          const int32_t* __restrict__ idx, int negate, const double* __restrict__ stage,
                                          int32_t* __restrict__ col_of_row, double* __restrict__ mean, int32_t* __restrict__ info) {
    constexpr int CM = 64 * CPL;
    const int lane = threadIdx.x & 63;
    double* u = reinterpret_cast<double*>(sl);
    int* row4col = reinterpret_cast<int*>(u + CM);
    int* path = row4col + CM;
    int* col4row = path + CM;
    int* sidx = col4row + CM;
    const bool tr = pr.nr > pr.nc;                        // (uniform) the transposed problem is solved
    const int R = tr ? pr.nc : pr.nr, Cn = tr ? pr.nr : pr.nc;
    const int soff = tr ? pr.coff : pr.roff, loff = tr ? pr.roff : pr.coff;      // the lists of the short / the long side
    const bool staged = pr.stage >= 0;
    // entry (i, j) of the R x Cn problem: base[sidx[i] * istr + joff_j]
    const double* base = staged ? stage + pr.stage : D + (long long)pr.b * N * ld;
    const long long istr = staged ? (long long)Cn : (tr ? 1ll : ld);
    const long long jstr = staged ? 1ll : (tr ? ld : 1ll);
    for (int i = lane; i < R; i += 64) { sidx[i] = staged ? i : idx[soff + i]; u[i] = 0.0; col4row[i] = -1; }
    for (int j = lane; j < Cn; j += 64) { row4col[j] = -1; path[j] = -1; }
    long long joff[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int j = lane + 64 * q, jc = j < Cn ? j : Cn - 1;          // (a padding column reads the last real one's entry and is never open)
        joff[q] = (long long)(staged ? jc : idx[loff + jc]) * jstr;
    }
    lg_wave_sync();
    auto load_row = [&](int i, double (&cv_)[CPL]) {
        const double* rp = base + (long long)sidx[i] * istr;
#pragma unroll
        for (int q = 0; q < CPL; ++q) cv_[q] = rp[joff[q]];
    };
    auto entry = [&](int i, int j) -> double {            // any lane, any entry
        return base[(long long)sidx[i] * istr + (long long)(staged ? j : idx[loff + j]) * jstr];
    };
    auto give_up = [&](int code) {                        // col_of_row of such a problem is not meaningful: all -1
        if (lane == 0) { info[pr.p] = code; mean[pr.p] = __builtin_nan(""); }
        if (col_of_row) for (int r = lane; r < pr.nr; r += 64) col_of_row[pr.ooff + r] = -1;
    };
    // SciPy rejects NaN and the infinity of the wrong sign before it searches
    {
        bool bad = false;
        for (int i = 0; i < R; ++i) {
            double cv[CPL];
            load_row(i, cv);
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const double x = cv[q];
                bad = bad || (x != x) || (negate ? x == DM_INF_F64 : x == -DM_INF_F64);
            }
        }
        if (__builtin_amdgcn_ballot_w64(bad)) { give_up(2); return; }
    }
    const double sgn = negate ? -1.0 : 1.0;
    double v[CPL], spc[CPL];
    int pos[CPL], sc[CPL], r4c[CPL], pth[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) v[q] = 0.0;
    bool infeasible = false;
    for (int cur = 0; cur < R; ++cur) {
        int kb[CPL], ks[CPL];                             // the tie key of column j at list position p is kb + p * ks (lsa_key)
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int j = lane + 64 * q;
            spc[q] = DM_INF_F64; sc[q] = 0; pos[q] = Cn - 1 - j; pth[q] = -1;        // remaining[it] = Cn - it - 1
            r4c[q] = j < Cn ? row4col[j] : -1;
            const bool fr = r4c[q] == -1;
            kb[q] = ((fr ? 8192 : 8191) << 14) | j;
            ks[q] = fr ? (1 << 14) : -(1 << 14);
        }
        int i = cur, nrem = Cn, sink = -1;
        double min_val = 0.0;
        double ui = u[i];
        double cv[CPL];
        load_row(i, cv);
        while (true) {
            double cand[CPL];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int j = lane + 64 * q;
                const bool open = (j < Cn) & (sc[q] == 0);
                const double r = ((min_val + sgn * cv[q]) - ui) - v[q];               // SciPy's operation order
                const bool better = open & (r < spc[q]);
                spc[q] = better ? r : spc[q];
                pth[q] = better ? i : pth[q];
                cand[q] = open ? spc[q] : DM_INF_F64;
            }
            double tv = cand[0];
#pragma unroll
            for (int q = 1; q < CPL; ++q) tv = __builtin_fmin(tv, cand[q]);
            const double wmin = lsa_wave_min(tv);
            const bool feas = wmin < DM_INF_F64;
            int tk = -1, trow = -1;
#pragma unroll
            for (int q = CPL - 1; q >= 0; --q) {
                const int key = kb[q] + pos[q] * ks[q];
                const bool take = (cand[q] == wmin) & feas & (key > tk);
                tk = take ? key : tk; trow = take ? r4c[q] : trow;
            }
            const unsigned long long have = __builtin_amdgcn_ballot_w64(tk >= 0);
            if (!have) { infeasible = true; break; }       // every remaining entry infinite: SciPy's "cost matrix is infeasible"
            int src = (int)__builtin_ctzll(have);
            if ((have & (have - 1)) != 0) {
                const int best = lsa_wave_max(tk);
                src = (int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(tk == best));
            }
            const int wkey = __builtin_amdgcn_readlane(tk, src), wrow = __builtin_amdgcn_readlane(trow, src);
            const int wK = wkey >> 14, wj = wkey & 16383;
            const int wsk = wK >= 8192 ? 1 : 0;
            const int wit = wsk ? wK - 8192 : 8191 - wK;
            min_val = wmin;
            if (!wsk) {                                    // the next row's loads go out before the list is updated
                i = wrow;
                load_row(i, cv);
                ui = u[i];
            }
            // remove the chosen column from the list: the column at the last position takes its place
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int j = lane + 64 * q;
                const bool hit = j == wj;
                const bool moved = (sc[q] == 0) & !hit & (pos[q] == nrem - 1);
                pos[q] = moved ? wit : pos[q];
                sc[q] = hit ? 1 : sc[q];
            }
            --nrem;
            if (wsk) { sink = wj; break; }
        }
        if (infeasible) break;
        // dual updates: every scanned column once; the row it was assigned to (if any) is a visited row
        if (lane == 0) u[cur] += min_val;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            if (sc[q]) {
                path[lane + 64 * q] = pth[q];             // (the flip walks scanned columns only)
                const double dlt = min_val - spc[q];
                if (r4c[q] != -1) u[r4c[q]] += dlt;       // (distinct rows: one column each)
                v[q] -= dlt;
            }
        }
        lg_wave_sync();
        if (lane == 0) {                                  // flip the augmenting path
            int j = sink;
            while (true) {
                const int i2 = path[j];
                row4col[j] = i2;
                const int jn = col4row[i2];
                col4row[i2] = j;
                j = jn;
                if (i2 == cur) break;
            }
        }
        lg_wave_sync();
    }
    if (infeasible) { give_up(1); return; }
    // rows of S in order: untransposed row r is short item r with column col4row[r]; transposed row r is long item r, its
    // column the short item row4col[r] (-1: unassigned)
    double s;
    if (!tr) {
        if (col_of_row) for (int r = lane; r < R; r += 64) col_of_row[pr.ooff + r] = col4row[r];
        s = lg_ordered_sum(R, lane, [&](int k) { return entry(k, col4row[k]); });
    } else {
        if (col_of_row) for (int r = lane; r < Cn; r += 64) col_of_row[pr.ooff + r] = row4col[r];
        s = lg_ordered_sum(Cn, lane, [&](int k) { const int i2 = row4col[k]; return i2 >= 0 ? entry(i2, k) : 0.0; });
    }
    if (lane == 0) mean[pr.p] = s / (double)R;
}

template <int MAXC>      // log2 of the columns per lane of the widest problem of the launch
__global__ __launch_bounds__(64 * LG_WPB) void lg_search_kernel(const double* __restrict__ D, int N, long long ld, const int32_t* __restrict__ idx,
                                                                const lg_prob* __restrict__ tab, int count, int negate,
                                                                const double* __restrict__ stage, int32_t* __restrict__ col_of_row,
                                                                double* __restrict__ mean, int32_t* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lg_smem[];
    const int wave = lg_uni(threadIdx.x >> 6);
    const int w = blockIdx.x * LG_WPB + wave;
    if (w >= count) return;                               // (the whole wave; nothing below waits for another wave)
    const lg_prob* tp = tab + w;
    lg_prob pr;
    pr.b = lg_uni(tp->b); pr.roff = lg_uni(tp->roff); pr.nr = lg_uni(tp->nr); pr.coff = lg_uni(tp->coff); pr.nc = lg_uni(tp->nc);
    pr.ooff = lg_uni(tp->ooff); pr.p = lg_uni(tp->p); pr.cls = lg_uni(tp->cls);
    {
        const long long st = tp->stage;
        pr.stage = ((long long)lg_uni((int)(st >> 32)) << 32) | (unsigned int)lg_uni((int)(st & 0xffffffffll));
    }
    unsigned char* sl = lg_smem + (size_t)wave * (LG_SLICE * 64 << MAXC);
    if (pr.cls <= 0) lg_search<1>(sl, pr, D, N, ld, idx, negate, stage, col_of_row, mean, info);
    else if (MAXC >= 1 && pr.cls == 1) lg_search<(MAXC >= 1 ? 2 : 1)>(sl, pr, D, N, ld, idx, negate, stage, col_of_row, mean, info);
    else if (MAXC >= 2 && pr.cls == 2) lg_search<(MAXC >= 2 ? 4 : 1)>(sl, pr, D, N, ld, idx, negate, stage, col_of_row, mean, info);
    else if (MAXC >= 3 && pr.cls == 3) lg_search<(MAXC >= 3 ? 8 : 1)>(sl, pr, D, N, ld, idx, negate, stage, col_of_row, mean, info);
    else if (MAXC >= 4) lg_search<(MAXC >= 4 ? 16 : 1)>(sl, pr, D, N, ld, idx, negate, stage, col_of_row, mean, info);
}

// The R x Cn blocks (short side x long side) of the table entries [first, first + count) that have a scratch offset:
// blk[i][j] = S[i][j] (nr <= nc) or S[j][i] (nr > nc).  grid (count, tiles in flight); tiles of 32 x 32.  The untransposed block is
// read and written along j; the transposed one is read along i (a row of D) and written along j, through the LDS tile.
__global__ __launch_bounds__(256) void lg_block_kernel(const double* __restrict__ D, int N, long long ld, const int32_t* __restrict__ idx,
                                                       const lg_prob* __restrict__ tab, int first, double* __restrict__ stage) {
    __shared__ double tile[32][33];
    const lg_prob pr = tab[first + blockIdx.x];
    if (pr.stage < 0) return;                             // (uniform)
    const bool tr = pr.nr > pr.nc;
    const int R = tr ? pr.nc : pr.nr, Cn = tr ? pr.nr : pr.nc;
    const int soff = tr ? pr.coff : pr.roff, loff = tr ? pr.roff : pr.coff;
    const double* Db = D + (long long)pr.b * N * ld;
    double* blk = stage + pr.stage;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int ti = dm_cdiv(R, 32), tj = dm_cdiv(Cn, 32);
    for (int t = blockIdx.y; t < ti * tj; t += gridDim.y) {
        const int i0 = (t / tj) * 32, j0 = (t % tj) * 32;
        if (!tr) {
            for (int q = ty; q < 32; q += 8) {
                const int i = i0 + q, j = j0 + tx;
                if (i < R && j < Cn) blk[(long long)i * Cn + j] = Db[(long long)idx[soff + i] * ld + idx[loff + j]];
            }
        } else {
            for (int q = ty; q < 32; q += 8) {
                const int j = j0 + q, i = i0 + tx;
                if (i < R && j < Cn) tile[q][tx] = Db[(long long)idx[loff + j] * ld + idx[soff + i]];
            }
            __syncthreads();
            for (int q = ty; q < 32; q += 8) {
                const int i = i0 + q, j = j0 + tx;
                if (i < R && j < Cn) blk[(long long)i * Cn + j] = tile[tx][q];
            }
            __syncthreads();
        }
    }
}

// inv[c4r[i]] = i (inv preset to -1): the short item of every long item of a wide transposed problem
__global__ __launch_bounds__(256) void lg_invert_kernel(const int32_t* __restrict__ c4r, int R, int Cn, int32_t* __restrict__ inv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int j = c4r[i];
    if (j >= 0 && j < Cn) inv[j] = i;
}
// outputs of a wide problem (one wave): c4r (R) = lsa_run's assignment of the gathered R x Cn block, inv (Cn) its inverse (transposed only)
__global__ __launch_bounds__(64) void lg_finish_kernel(const lg_prob* __restrict__ tab, int w, const double* __restrict__ stage,
                                                       const int32_t* __restrict__ c4r, const int32_t* __restrict__ inv,
                                                       int32_t* __restrict__ col_of_row, double* __restrict__ mean, const int32_t* __restrict__ info) {
    const lg_prob pr = tab[w];
    const int lane = threadIdx.x;
    const bool tr = pr.nr > pr.nc;
    const int R = lg_uni(tr ? pr.nc : pr.nr), Cn = lg_uni(tr ? pr.nr : pr.nc);      // (uniform: the loop bounds of the ordered sum)
    const double* blk = stage + pr.stage;
    if (info[pr.p] != 0) {
        if (lane == 0) mean[pr.p] = __builtin_nan("");
        if (col_of_row) for (int r = lane; r < pr.nr; r += 64) col_of_row[pr.ooff + r] = -1;
        return;
    }
    double s;
    if (!tr) {
        if (col_of_row) for (int r = lane; r < R; r += 64) col_of_row[pr.ooff + r] = c4r[r];
        s = lg_ordered_sum(R, lane, [&](int k) { return blk[(long long)k * Cn + c4r[k]]; });
    } else {
        if (col_of_row) for (int r = lane; r < Cn; r += 64) col_of_row[pr.ooff + r] = inv[r];
        s = lg_ordered_sum(Cn, lane, [&](int k) { const int i2 = inv[k]; return i2 >= 0 ? blk[(long long)i2 * Cn + k] : 0.0; });
    }
    if (lane == 0) mean[pr.p] = s / (double)R;
}

template <int MAXC>
static int lg_launch_search(dm_ctx* ctx, int count, const double* D, int N, long long ld, const int32_t* idx, const lg_prob* tab, int negate,
                            const double* stage, int32_t* col_of_row, double* mean, int32_t* info) {
    const size_t lds = (size_t)LG_WPB * (LG_SLICE * 64 << MAXC);
    const int rc = dm_grant_lds(ctx, (const void*)lg_search_kernel<MAXC>, lds);
    if (rc) return rc;
    DM_LAUNCH(ctx, "lsa_gather_search", lg_search_kernel<MAXC>, dim3(dm_cdiv(count, LG_WPB)), dim3(64 * LG_WPB), lds, D, N, ld, idx, tab, count,
              negate, stage, col_of_row, mean, info);
    return DM_OK;
}

extern "C" int dm_lsa_gather(dm_ctx* ctx, int B, int N, int ld, const double* D, int n_idx, const int32_t* idx, int P,
                             const int32_t* problems, int maximize, int32_t* col_of_row, double* mean, int32_t* info) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && ld >= N && n_idx >= 0 && P >= 0, "sizes must be positive, ld >= N");
    if (P == 0) return DM_OK;
    DM_REQUIRE(ctx, D && idx && problems && mean && info, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    // the table, widest class first and by work within everything that one launch serves
    std::vector<lg_prob> tab((size_t)P);
    std::vector<double> work((size_t)P);
    for (int p = 0; p < P; ++p) {
        const int32_t* e = problems + (size_t)p * 6;
        lg_prob& t = tab[p];
        t.b = e[0]; t.roff = e[1]; t.nr = e[2]; t.coff = e[3]; t.nc = e[4]; t.ooff = e[5]; t.p = p; t.stage = -1;
        DM_REQUIRE(ctx, t.b >= 0 && t.b < B, "problem table: mesh outside the batch");
        DM_REQUIRE(ctx, t.nr > 0 && t.nc > 0, "problem table: empty index list");
        DM_REQUIRE(ctx, t.roff >= 0 && t.coff >= 0 && (long long)t.roff + t.nr <= n_idx && (long long)t.coff + t.nc <= n_idx,
                   "problem table: index list outside the index array");
        DM_REQUIRE(ctx, t.ooff >= 0 || !col_of_row, "problem table: negative output offset");
        const int Cn = std::max(t.nr, t.nc), R = std::min(t.nr, t.nc);
        const int per = dm_cdiv(Cn, 64);
        t.cls = per > LG_MAX_CPL ? -1 : (per <= 1 ? 0 : (per <= 2 ? 1 : (per <= 4 ? 2 : (per <= 8 ? 3 : 4))));
        work[p] = (double)R * R * Cn;
    }
    std::stable_sort(tab.begin(), tab.end(), [&](const lg_prob& a, const lg_prob& b) {
        if ((a.cls < 0) != (b.cls < 0)) return b.cls < 0;              // the wide problems last
        return work[a.p] > work[b.p];
    });
    int n_wave = 0, maxc = 0;
    for (const lg_prob& t : tab) if (t.cls >= 0) { ++n_wave; maxc = std::max(maxc, t.cls); }
    // Scratch: the table, the staged copies of tall one-wave problems (largest first while they fit), and for the wide problems ONE
    // block buffer plus lsa_run's own state.  Kept below the bytes of D: a staged copy that would not fit is not made.
    const size_t d_bytes = (size_t)B * N * (size_t)ld * 8, tab_bytes = dm_align_up((size_t)P * sizeof(lg_prob));
    size_t over_blk = 0, over_ws = 0;
    int over_R = 0, over_C = 0;
    for (const lg_prob& t : tab)
        if (t.cls < 0) {
            const int Cn = std::max(t.nr, t.nc), R = std::min(t.nr, t.nc);
            over_blk = std::max(over_blk, (size_t)R * Cn * 8);
            over_ws = std::max(over_ws, lsa_ws_bytes(1, R, Cn));
            over_R = std::max(over_R, R); over_C = std::max(over_C, Cn);
        }
    const size_t over_bytes = dm_align_up(over_blk) + over_ws + dm_align_up((size_t)over_R * 4) + dm_align_up((size_t)over_C * 4);
    const size_t fixed = tab_bytes + over_bytes + 4096;
    const size_t budget = d_bytes - d_bytes / 8 > fixed ? d_bytes - d_bytes / 8 - fixed : 0;
    size_t staged = 0;
    int n_staged = 0;
    for (int w = 0; w < n_wave; ++w) {
        lg_prob& t = tab[w];
        if (t.nr <= t.nc) continue;
        const size_t need = dm_align_up((size_t)t.nr * t.nc * 8);
        if (staged + need > budget) continue;
        t.stage = (long long)(staged / 8);
        staged += need;
        n_staged = w + 1;
    }
    for (lg_prob& t : tab) if (t.cls < 0) t.stage = (long long)(staged / 8);
    int rc = dm_ws_reserve(ctx, fixed + staged);
    if (rc) return rc;
    lg_prob* d_tab = (lg_prob*)dm_ws_take(ctx, (size_t)P * sizeof(lg_prob));
    double* d_stage = (double*)dm_ws_take(ctx, staged + dm_align_up(over_blk));
    if (!d_tab || !d_stage) return dm_fail(ctx, DM_ENOMEM, "lsa_gather: workspace not reserved");
    DM_CHECK_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), (size_t)P * sizeof(lg_prob), hipMemcpyHostToDevice, ctx->stream));
    DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the table is a local: copied before it goes away)
    DM_CHECK_HIP(ctx, hipMemsetAsync(info, 0, (size_t)P * 4, ctx->stream));
    const int negate = maximize ? 1 : 0;
    if (n_staged > 0)
        DM_LAUNCH(ctx, "lsa_gather_stage", lg_block_kernel, dim3(n_staged, 8), dim3(256), 0, D, N, (long long)ld, idx, (const lg_prob*)d_tab, 0, d_stage);
    if (n_wave > 0) {
#define LG_GO(M_) rc = lg_launch_search<M_>(ctx, n_wave, D, N, (long long)ld, idx, d_tab, negate, d_stage, col_of_row, mean, info)
        if (maxc == 0) LG_GO(0); else if (maxc == 1) LG_GO(1); else if (maxc == 2) LG_GO(2); else if (maxc == 3) LG_GO(3); else LG_GO(4);
#undef LG_GO
        if (rc) return rc;
    }
    if (n_wave < P) {
        int32_t* c4r = (int32_t*)dm_ws_take(ctx, (size_t)over_R * 4);
        int32_t* inv = (int32_t*)dm_ws_take(ctx, (size_t)over_C * 4);
        if (!c4r || !inv) return dm_fail(ctx, DM_ENOMEM, "lsa_gather: workspace not reserved");
        const size_t mark = ctx->ws_off;
        for (int w = n_wave; w < P; ++w) {
            const lg_prob& t = tab[w];
            const bool tr = t.nr > t.nc;
            const int Cn = std::max(t.nr, t.nc), R = std::min(t.nr, t.nc);
            const double* blk = d_stage + t.stage;
            DM_LAUNCH(ctx, "lsa_gather_stage", lg_block_kernel, dim3(1, 256), dim3(256), 0, D, N, (long long)ld, idx, (const lg_prob*)d_tab, w, d_stage);
            ctx->ws_off = mark;                               // (the searches run one after the other on the stream: one state for all)
            rc = lsa_run(ctx, 1, R, Cn, blk, 0, 0, nullptr, nullptr, nullptr, maximize, c4r, info + t.p);
            if (rc) return rc;
            if (tr) {
                DM_CHECK_HIP(ctx, hipMemsetAsync(inv, 0xFF, (size_t)Cn * 4, ctx->stream));
                DM_LAUNCH(ctx, "lsa_gather_invert", lg_invert_kernel, dim3(dm_cdiv(R, 256)), dim3(256), 0, (const int32_t*)c4r, R, Cn, inv);
            }
            DM_LAUNCH(ctx, "lsa_gather_finish", lg_finish_kernel, dim3(1), dim3(64), 0, (const lg_prob*)d_tab, w, (const double*)d_stage,
                      (const int32_t*)c4r, (const int32_t*)inv, col_of_row, mean, (const int32_t*)info);
        }
    }
    return DM_OK;
}

// Functional map networks on the device (dm_fmn_*): SURVEY.md section 2 #8.
//
// Reference computation replaced: pyFM/FMN/FMN.py -- the quadratic form of the consistent latent basis (CLB_quad_form, :690-738: a
// scipy.sparse.bmat of n x n blocks built edge by edge), the orthogonality test of set_isometries (:234-270), the three-cycle costs of
// the ICSM weights (:559-594: three triple products per cycle in a Python loop) and the canonical basis (compute_CCLB, :336-369).  The
// eigenproblem of the quadratic form is dm_eigh_smallest (dm_eigen.hip); the linear program of the ICSM weights stays on the host.
//
// All products run on the f64 matrix cores through the tiles of dm_gemm_f64.h (one K split: a sum's order is the tile's k order and
// nothing else); what follows a product -- "- I, square", the recurrence of the eigensolver -- is the tile's epilogue, and every
// reduction over a matrix is one workgroup adding in a fixed order.  No floating-point atomics; an edge's or a cycle's result does not
// depend on the other problems of the call.
#include "dm_gemm_f64.h"
#include "dm_internal.h"

constexpr int FMN_MAX_M = 256;

// ---- operand and output functors ---------------------------------------------------------------------------------------------
struct FmnMapTN {                   // K-major operand: row n of the cropped map of edge b
    const double* maps; int ldm; int M;
    __device__ __forceinline__ void load4(int b, int n, int col0, double (&v)[4]) const {
        const double* row = maps + ((long long)b * ldm + n) * ldm;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (col0 + e < M) ? row[col0 + e] : 0.0;
    }
};
struct FmnOutGram {                 // G[b] (M x M)
    double* p; int M;
    __device__ __forceinline__ void store(int b, int, int m, int c, double v) const { p[((long long)b * M + m) * M + c] = v; }
};
struct FmnOutGramDefSq {            // (G[b] - I)^2 entry by entry
    double* p; int M;
    __device__ __forceinline__ void store(int b, int, int m, int c, double v) const {
        const double d = v - (m == c ? 1.0 : 0.0);
        p[((long long)b * M + m) * M + c] = d * d;
    }
};
// K-contiguous rows (NT form) of the cropped map in slot `slot` of rotation b % 3 of cycle b / 3: rotation r reads the cycle's edges
// (e_ij, e_jk, e_ki) from position r on.  trans: element (row, k) is map[k][row].
struct FmnCycRows {
    const double* maps; const int32_t* cyc; int E, ldm, M, slot, trans;
    __device__ __forceinline__ void load8(int b, int row, int k0, double (&v)[8]) const {
        const int c = b / 3, r = b - 3 * c;
        int s = r + slot;
        if (s >= 3) s -= 3;
        const int e = min(max(cyc[c * 3 + s], 0), E - 1);
        const double* base = maps + (long long)e * ldm * ldm;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = k0 + q;
            double x = 0.0;
            if (row < M && k < M) x = trans ? base[(long long)k * ldm + row] : base[(long long)row * ldm + k];
            v[q] = x;
        }
    }
};
struct FmnOutNT {
    double* p; long long stride_b; int ld;
    __device__ __forceinline__ void store(int b, int i, int j, double v) const { p[b * stride_b + (long long)i * ld + j] = v; }
};
struct FmnOutDefSq {                // (P - I)^2 entry by entry: the epilogue of a cycle's second product
    double* p; long long stride_b; int ld;
    __device__ __forceinline__ void store(int b, int i, int j, double v) const {
        const double d = v - (i == j ? 1.0 : 0.0);
        p[b * stride_b + (long long)i * ld + j] = d * d;
    }
};
// K-major operand of the canonical basis: row q = i M + k of the stacked Y_i = CLB[i][:, :m], scaled by evals[i][k] when given
struct FmnClbTN {
    const double* clb; int M, m; const double* evals; int ldl;
    __device__ __forceinline__ void load4(int, int q, int col0, double (&v)[4]) const {
        const double* row = clb + (long long)q * M;
        double s = 1.0;
        if (evals) { const int i = q / M; s = evals[(long long)i * ldl + (q - i * M)]; }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (col0 + e < m) ? s * row[col0 + e] : 0.0;
    }
};

// ---- reductions ------------------------------------------------------------------------------------------------------------------
// sum of len doubles by one workgroup of 256 threads: thread t adds the entries t, t + 256, ... in ascending order, the 256 partial sums
// meet in a binary tree (every thread gets the result)
__device__ __forceinline__ double fmn_block_sum(const double* __restrict__ x, int len, double* sh) {
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < len; i += 256) s += x[i];
    __syncthreads();
    sh[t] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if (t < off) sh[t] += sh[t + off]; __syncthreads(); }
    return sh[0];
}
// out[b] = sqrt(sum sq[b])
__global__ __launch_bounds__(256) void fmn_norm_kernel(const double* __restrict__ sq, int len, double* __restrict__ out) {
    __shared__ double sh[256];
    const int b = blockIdx.x;
    const double s = fmn_block_sum(sq + (long long)b * len, len, sh);
    if (threadIdx.x == 0) out[b] = sqrt(s);
}
// cost[c] = max over the three rotations of sqrt(sum sq[3 c + r])
__global__ __launch_bounds__(256) void fmn_cycle_max_kernel(const double* __restrict__ sq, int len, double* __restrict__ cost) {
    __shared__ double sh[256];
    const int c = blockIdx.x;
    double mx = 0.0;
    for (int r = 0; r < 3; ++r) mx = fmax(mx, sqrt(fmn_block_sum(sq + ((long long)c * 3 + r) * len, len, sh)));
    if (threadIdx.x == 0) cost[c] = mx;
}

// ---- quadratic form ----------------------------------------------------------------------------------------------------------------
// One workgroup owns 256 consecutive entries of one M x M block (bi, bj) of W and walks the edge list in index order, so opposite edges
// and the several contributions to a diagonal block meet in a fixed order.  Per edge, in the reference's order of statements:
//   (i,i) += w G,  (j,j) += w I,  (i,j) -= w FM^T,  (j,i) -= w FM       (G = FM^T FM from the tile kernel)
// Product and sum are rounded separately (floating-point contraction is switched off in the loop: no fused multiply-add), so an
// off-diagonal block is the host's 0 - w FM^T [- w' FM'] bit for bit.
__global__ __launch_bounds__(256) void fmn_quad_assemble_kernel(const double* __restrict__ maps, int ldm, int M, int n, int E,
                                                                const int32_t* __restrict__ edges, const double* __restrict__ w,
                                                                const double* __restrict__ G, double* __restrict__ W) {
    const int per_block = (M * M + 255) / 256;
    const long long wg = blockIdx.x;
    const int blk = (int)(wg / per_block), part = (int)(wg - (long long)blk * per_block);
    const int bi = blk / n, bj = blk - bi * n;
    const int idx = part * 256 + threadIdx.x;
    if (idx >= M * M) return;
    const int r = idx / M, c = idx - r * M;
    double acc = 0.0;
    {
#pragma clang fp contract(off)
        for (int e = 0; e < E; ++e) {
            const int i = edges[2 * e], j = edges[2 * e + 1];
            if (i < 0 || i >= n || j < 0 || j >= n) continue;
            if (i != bi && j != bi) continue;
            const double we = w[e];
            const double* FM = maps + (long long)e * ldm * ldm;
            if (bi == bj) {
                if (i == bi) { const double p = we * G[((long long)e * M + r) * M + c]; acc = acc + p; }
                if (j == bi) { const double p = we * (r == c ? 1.0 : 0.0); acc = acc + p; }
            }
            if (i == bi && j == bj) { const double p = we * FM[(long long)c * ldm + r]; acc = acc - p; }
            if (j == bi && i == bj) { const double p = we * FM[(long long)r * ldm + c]; acc = acc - p; }
        }
    }
    W[((long long)bi * M + r) * ((long long)n * M) + (long long)bj * M + c] = acc;
}

// ---- canonical basis -----------------------------------------------------------------------------------------------------------------
// H[r][c] = (E[r][c] + E[c][r]) / 2 / n; a second copy for the Rayleigh quotients (the Jacobi kernel overwrites its matrix)
__global__ __launch_bounds__(256) void fmn_cclb_sym_kernel(const double* __restrict__ Eraw, int m, double n, double* __restrict__ H,
                                                           double* __restrict__ H0) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * m) return;
    const int r = idx / m, c = idx - r * m;
    const double v = 0.5 * (Eraw[idx] + Eraw[(long long)c * m + r]) / n;
    H[idx] = v;
    H0[idx] = v;
}
// theta[j] = (q_j^T H q_j) / (q_j^T q_j) with the matrix as it was before the rotations.  The diagonal the Jacobi sweeps leave carries the
// rounding of every rotation (sweeps x m of them per entry): against NumPy on the same E, m = 19, it is off by 1.0 - 1.5 x m 2^-52 |E|.
// The accumulated vectors are orthonormal to ~4e-15 only, so the quotient needs its denominator: without it the error stays at
// 0.9 - 1.25 of that bound, with it 0.1 (the eigenvector's own error enters squared).
// One workgroup per column; thread t adds rows t, t + 256, ... in order, then a binary tree over the 256 partial sums.
__global__ __launch_bounds__(256) void fmn_rayleigh_kernel(const double* __restrict__ H0, const double* __restrict__ Q, int m,
                                                           double* __restrict__ theta) {
    __shared__ double sh[256], sq[256];
    const int j = blockIdx.x, t = threadIdx.x;
    double s = 0.0, d = 0.0;
    for (int r = t; r < m; r += 256) {
        double hq = 0.0;
        for (int c = 0; c < m; ++c) hq += H0[(long long)r * m + c] * Q[(long long)c * m + j];
        const double q = Q[(long long)r * m + j];
        s += q * hq;
        d += q * q;
    }
    sh[t] = s; sq[t] = d;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if (t < off) { sh[t] += sh[t + off]; sq[t] += sq[t + off]; } __syncthreads(); }
    if (t == 0) theta[j] = sq[0] > 0.0 ? sh[0] / sq[0] : sh[0];
}
// the entry of largest magnitude of every column of Q (m x m) positive (the lowest row on ties): one thread per column
__global__ __launch_bounds__(256) void fmn_sign_kernel(double* __restrict__ Q, int m) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    double best = -1.0; int bi = 0;
    for (int r = 0; r < m; ++r) { const double v = fabs(Q[(long long)r * m + c]); if (v > best) { best = v; bi = r; } }
    if (Q[(long long)bi * m + c] < 0.0)
        for (int r = 0; r < m; ++r) Q[(long long)r * m + c] = -Q[(long long)r * m + c];
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
static int fmn_gram(dm_ctx* ctx, int E, int M, const double* maps, int ldm, double* out, bool defect_sq) {
    FmnMapTN x{maps, ldm, M};
    const dim3 grid(dm_cdiv(M, TN_T) * dm_cdiv(M, TN_T), 1, E);
    if (defect_sq) {
        FmnOutGramDefSq o{out, M};
        DM_LAUNCH(ctx, "fmn_gram_tn_f64", (gemm_tn_f64<FmnMapTN, FmnMapTN, FmnOutGramDefSq>), grid, dim3(256), 0, x, x, o, M, M, M, M);
    } else {
        FmnOutGram o{out, M};
        DM_LAUNCH(ctx, "fmn_gram_tn_f64", (gemm_tn_f64<FmnMapTN, FmnMapTN, FmnOutGram>), grid, dim3(256), 0, x, x, o, M, M, M, M);
    }
    return DM_OK;
}

extern "C" int dm_fmn_orth_defect(dm_ctx* ctx, int E, int M, const double* maps, int ldm, double* out) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, E > 0 && E <= 65535 && M > 0 && M <= FMN_MAX_M && ldm >= M, "1 <= E <= 65535, 1 <= M <= min(ldm, 256)");
    DM_REQUIRE(ctx, maps && out, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)E * M * M * 8;
    int rc = dm_ws_reserve(ctx, dm_align_up(bytes) + 4096);
    if (rc) return rc;
    double* sq = (double*)dm_ws_take(ctx, bytes);
    if (!sq) return dm_fail(ctx, DM_ENOMEM, "fmn_orth_defect: workspace not reserved");
    rc = fmn_gram(ctx, E, M, maps, ldm, sq, true);
    if (rc) return rc;
    DM_LAUNCH(ctx, "fmn_norm", fmn_norm_kernel, dim3(E), dim3(256), 0, (const double*)sq, M * M, out);
    return DM_OK;
}

extern "C" int dm_fmn_cycle_costs(dm_ctx* ctx, int E, int M, const double* maps, int ldm, int n_cyc, const int32_t* cyc_edges, double* cost) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, E > 0 && M > 0 && M <= FMN_MAX_M && ldm >= M && n_cyc > 0, "E, n_cyc >= 1, 1 <= M <= min(ldm, 256)");
    DM_REQUIRE(ctx, maps && cyc_edges && cost, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    // the cycles in chunks whose two intermediates (first products, squared defects) stay within 64 MiB; at most 65535 / 3 per launch
    const size_t per_cycle = (size_t)3 * M * M * 8;
    int chunk = (int)((size_t)(32u << 20) / per_cycle);
    chunk = chunk < 1 ? 1 : (chunk > 21845 ? 21845 : chunk);
    if (chunk > n_cyc) chunk = n_cyc;
    int rc = dm_ws_reserve(ctx, 2 * dm_align_up(per_cycle * chunk) + 4096);
    if (rc) return rc;
    double* P1 = (double*)dm_ws_take(ctx, per_cycle * chunk);
    double* sq = (double*)dm_ws_take(ctx, per_cycle * chunk);
    if (!P1 || !sq) return dm_fail(ctx, DM_ENOMEM, "fmn_cycle_costs: workspace not reserved");
    const int tiles = dm_cdiv(M, NT_T) * dm_cdiv(M, NT_T);
    for (int c0 = 0; c0 < n_cyc; c0 += chunk) {
        const int nc = n_cyc - c0 < chunk ? n_cyc - c0 : chunk;
        const int32_t* cyc = cyc_edges + (size_t)c0 * 3;
        FmnCycRows a{maps, cyc, E, ldm, M, 0, 0}, b{maps, cyc, E, ldm, M, 1, 1}, c{maps, cyc, E, ldm, M, 2, 1};
        FmnOutNT o1{P1, (long long)M * M, M};
        DM_LAUNCH(ctx, "fmn_cycle_ab_nt_f64", (gemm_nt_f64<FmnCycRows, FmnCycRows, FmnOutNT>), dim3(tiles, 1, 3 * nc), dim3(256), 0, a, b, o1, M, M, M);
        KRowsF64 p{P1, (long long)M * M, M, M, M, 0};
        FmnOutDefSq o2{sq, (long long)M * M, M};
        DM_LAUNCH(ctx, "fmn_cycle_abc_nt_f64", (gemm_nt_f64<KRowsF64, FmnCycRows, FmnOutDefSq>), dim3(tiles, 1, 3 * nc), dim3(256), 0, p, c, o2, M, M, M);
        DM_LAUNCH(ctx, "fmn_cycle_max", fmn_cycle_max_kernel, dim3(nc), dim3(256), 0, (const double*)sq, M * M, cost + c0);
    }
    return DM_OK;
}

extern "C" int dm_fmn_quad_form(dm_ctx* ctx, int n, int E, int M, const double* maps, int ldm, const int32_t* edges, const double* w, double* W) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, n > 0 && E > 0 && E <= 65535 && M > 0 && M <= FMN_MAX_M && ldm >= M, "n >= 1, 1 <= E <= 65535, 1 <= M <= min(ldm, 256)");
    DM_REQUIRE(ctx, (long long)n * M <= 4096, "n M must be <= 4096");
    DM_REQUIRE(ctx, maps && edges && w && W, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)E * M * M * 8;
    int rc = dm_ws_reserve(ctx, dm_align_up(bytes) + 4096);
    if (rc) return rc;
    double* G = (double*)dm_ws_take(ctx, bytes);
    if (!G) return dm_fail(ctx, DM_ENOMEM, "fmn_quad_form: workspace not reserved");
    rc = fmn_gram(ctx, E, M, maps, ldm, G, false);
    if (rc) return rc;
    const long long wgs = (long long)n * n * dm_cdiv(M * M, 256);
    DM_LAUNCH(ctx, "fmn_quad_assemble", fmn_quad_assemble_kernel, dim3((unsigned)wgs), dim3(256), 0, maps, ldm, M, n, E, edges, w, (const double*)G, W);
    return DM_OK;
}

extern "C" int dm_fmn_cclb(dm_ctx* ctx, int n, int M, int m, const double* CLB, const double* evals, int ldl, double* cclb, double* cclb_evals) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, n > 0 && n <= 65535 && m > 0 && m <= M && M <= FMN_MAX_M && ldl >= M, "1 <= n <= 65535, 1 <= m <= M <= min(ldl, 256)");
    DM_REQUIRE(ctx, CLB && evals && cclb && cclb_evals, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bm = (size_t)m * m * 8;
    int rc = dm_ws_reserve(ctx, 5 * dm_align_up(bm) + dm_align_up((size_t)m * 8) + 4096);
    if (rc) return rc;
    double* Eraw = (double*)dm_ws_take(ctx, bm);
    double* H = (double*)dm_ws_take(ctx, bm);
    double* H0 = (double*)dm_ws_take(ctx, bm);
    double* th = (double*)dm_ws_take(ctx, (size_t)m * 8);
    double* V = (double*)dm_ws_take(ctx, bm);
    double* Q = (double*)dm_ws_take(ctx, bm);
    if (!Eraw || !H || !H0 || !th || !V || !Q) return dm_fail(ctx, DM_ENOMEM, "fmn_cclb: workspace not reserved");
    // E = sum_i Y_i^T diag(lambda_i) Y_i: ONE product over the n M stacked rows, added in the order (i, k)
    const int K = n * M;
    FmnClbTN x{CLB, M, m, nullptr, 0}, y{CLB, M, m, evals, ldl};
    FmnOutGram oe{Eraw, m};
    DM_LAUNCH(ctx, "fmn_cclb_tn_f64", (gemm_tn_f64<FmnClbTN, FmnClbTN, FmnOutGram>), dim3(dm_cdiv(m, TN_T) * dm_cdiv(m, TN_T), 1, 1), dim3(256), 0,
              x, y, oe, m, m, K, K);
    DM_LAUNCH(ctx, "fmn_cclb_sym", fmn_cclb_sym_kernel, dim3(dm_cdiv(m * m, 256)), dim3(256), 0, (const double*)Eraw, m, (double)n, H, H0);
    rc = dm_eig_jacobi_sorted(ctx, 1, m, H, V, th, Q);
    if (rc) return rc;
    DM_LAUNCH(ctx, "fmn_rayleigh", fmn_rayleigh_kernel, dim3(m), dim3(256), 0, (const double*)H0, (const double*)Q, m, cclb_evals);
    DM_LAUNCH(ctx, "fmn_sign", fmn_sign_kernel, dim3(dm_cdiv(m, 256)), dim3(256), 0, Q, m);
    // cclb[i] = Y_i Q
    KRowsF64 ya{CLB, (long long)M * M, M, M, m, 0};
    KRowsF64 qb{Q, 0, m, m, m, 1};
    FmnOutNT oc{cclb, (long long)M * m, m};
    DM_LAUNCH(ctx, "fmn_cclb_nt_f64", (gemm_nt_f64<KRowsF64, KRowsF64, FmnOutNT>), dim3(dm_cdiv(M, NT_T) * dm_cdiv(m, NT_T), 1, n), dim3(256), 0,
              ya, qb, oc, M, m, m);
    return DM_OK;
}

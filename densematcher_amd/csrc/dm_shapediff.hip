// Shape difference operators on the device (dm_shape_diff_f64, dm_pullback_forms_f64): what pyFM/spectral/shape_difference.py computes per
// pair with NumPy / SciPy products on the host.
//
// Reference arithmetic reproduced (shape_difference.py:20, :44, :94-96):
//   spectral   SD_a = FM^T FM,   SD_c = pinv(diag(lam1)) FM^T (lam2 * FM)                       FM (k2, k1)
//   semican    X = Phi1[p21, :k1]   G_a = X^T diag(mass2) X,   G_w = X^T (W2 X)   [pinv(diag(lam1)) G_w]
// pinv(diag(lam1)) is the diagonal inv1[i] = 1 / lam1[i] where |lam1[i]| > 1e-15 max_j |lam1[j]|, else exactly 0 (np.linalg.pinv's
// cut-off at its default rcond; sd_inv_kernel).
//
// dm_shape_diff_f64: k2 <= 768 rows to contract -- one workgroup per (pair, 64 x 64 tile) of gemm_tn_f64, lam2 as the row scale of the
// second operand, inv1 in the output functor.  One sum per entry, rows l = 0 .. k2 - 1 in order.
//
// dm_pullback_forms_f64: pullback_forms_kernel, the f64 matrix cores (v_mfma_f64_16x16x4_f64).  A workgroup owns a 64 x 64 tile of BOTH
// forms and PB_SLABS slabs of PB_SLAB target vertices.  Per slab it stages three 16 x 64 operands in LDS: the gathered rows X (the
// tile's row block of columns), mass2 * X and W2 X (its column block) -- a row of W2 X is the nnz gathered rows Phi1[p21[col]] of the
// vertex's stiffness row, weighted and added in ELL order in registers, never written to HBM -- and multiplies X^T into both.  The next
// slab's rows are fetched into registers while the current one is multiplied (two LDS buffers, one barrier per slab).
//
// Order of sums: an entry's slab partial adds its vertices in index order (the MFMA's k order), a workgroup its slabs in order; the
// partials of a pair's ceil(n_verts2 / (PB_SLAB PB_SLABS)) workgroups go to the context's workspace and pullback_reduce_kernel adds
// them in that order.  The split depends on nothing but the pair's own vertex count: no atomics, the output is written once, the same
// pair gives the same bits alone, anywhere in a batch and under any padding.
#include "dm_gemm_f64.h"
#include "dm_internal.h"

constexpr int SD_MAX_K1 = 256;
constexpr int SD_MAX_K2 = 768;
constexpr int PB_SLAB = TN_BK;               // target vertices per staged slab (one k-block of four matrix instructions per 16 x 16 block)
constexpr int PB_SLABS = 32;                 // slabs per workgroup: 512 vertices per partial
constexpr int PB_CHUNK = PB_SLAB * PB_SLABS;

// inv1[b][i] = 1 / lam1[b][i] if |lam1[b][i]| > 1e-15 max_j<k1 |lam1[b][j]| else 0     (one workgroup of 256 threads per pair, k1 <= 256)
__global__ __launch_bounds__(256) void sd_inv_kernel(const double* __restrict__ lam1, int ld_l1, int k1, double* __restrict__ inv1) {
    __shared__ double red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const double l = t < k1 ? lam1[(long long)b * ld_l1 + t] : 0.0;
    double m = fabs(l);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    const double mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    if (t < k1) inv1[(long long)b * k1 + t] = (fabs(l) > 1e-15 * mx) ? 1.0 / l : 0.0;
}

struct OutSD {                     // the k1 x k1 operator itself; inv (B, k1) nullable: row i scaled by inv[i], a cut row is exactly +0
    double* p; const double* inv; int k1;
    __device__ __forceinline__ void store(int b, int, int m, int c, double v) const {
        if (inv) {
            const double s = inv[(long long)b * k1 + m];
            v = s == 0.0 ? 0.0 : s * v;
        }
        p[((long long)b * k1 + m) * k1 + c] = v;
    }
};

extern "C" int dm_shape_diff_f64(dm_ctx* ctx, int B, int k1, int k2, const double* FM, int ldf, const double* lam1, int ld_l1,
                                 const double* lam2, int ld_l2, double* SDa, double* SDc) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && k1 > 0 && k2 > 0, "sizes must be positive");
    DM_REQUIRE(ctx, k1 <= SD_MAX_K1 && k2 <= SD_MAX_K2, "maps of up to 768 x 256 (k2 x k1)");
    DM_REQUIRE(ctx, B <= 65535, "too many maps for one launch: split the batch");
    DM_REQUIRE(ctx, FM && (SDa || SDc), "null pointer");
    DM_REQUIRE(ctx, ldf >= k1, "row stride of FM smaller than k1");
    DM_REQUIRE(ctx, !SDc || (lam1 && lam2 && ld_l1 >= k1 && ld_l2 >= k2), "the conformal operator needs k1 / k2 eigenvalues per map");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    typedef RowsScaled<double, double> Rows;
    const long long sF = (long long)k2 * ldf;
    const dim3 grid(dm_cdiv(k1, TN_T) * dm_cdiv(k1, TN_T), 1, B);
    Rows opx{FM, sF, ldf, k1, nullptr, 0};
    if (SDa) {
        OutSD out{SDa, nullptr, k1};
        DM_LAUNCH(ctx, "shape_diff_tn_f64", (gemm_tn_f64<Rows, Rows, OutSD>), grid, dim3(256), 0, opx, opx, out, k1, k1, k2, k2);
    }
    if (SDc) {
        int rc = dm_ws_reserve(ctx, dm_align_up((size_t)B * k1 * 8));
        if (rc) return rc;
        double* inv1 = (double*)dm_ws_take(ctx, (size_t)B * k1 * 8);
        if (!inv1) return dm_fail(ctx, DM_ENOMEM, "shape_diff: workspace not reserved");
        DM_LAUNCH(ctx, "shape_diff_inv", sd_inv_kernel, dim3(B), dim3(256), 0, lam1, ld_l1, k1, inv1);
        Rows opy{FM, sF, ldf, k1, lam2, (long long)ld_l2};
        OutSD out{SDc, inv1, k1};
        DM_LAUNCH(ctx, "shape_diff_tn_f64", (gemm_tn_f64<Rows, Rows, OutSD>), grid, dim3(256), 0, opx, opy, out, k1, k1, k2, k2);
    }
    return DM_OK;
}

// ---- the pulled-back quadratic forms ------------------------------------------------------------------------------------------
struct pb_args {
    const int32_t* p21;                       // (B, N2)
    const double* Phi1; long long s1; int ld1;
    const int32_t* cols; const double* w; int nnz;      // (B, N2, nnz) stiffness rows, ELL
    const double* mass2;                      // (B, N2)
    const int32_t* nv1; const int32_t* nv2;   // (B) device, nullable: the pairs' own vertex counts
    int N1, N2, k1, B;
    double* part;                             // (nchunk, B, 2, k1, k1)
};

// the staged registers of one thread for one slab: four columns of one vertex' row of X (row block m0), of X again for the column
// block c0 (the same registers when the tile lies on the diagonal) and of W2 X
struct pb_regs { double xm[4], xc[4], yw[4]; double mass; };

template <bool DIAG>
__device__ __forceinline__ void pb_fetch(const pb_args& a, int b, int n, int nv1, int nv2, int m0, int c0, int lc, bool al, pb_regs& r) {
    if (n >= nv2) {                           // a row past the pair's vertices: zeros
#pragma unroll
        for (int e = 0; e < 4; ++e) r.xm[e] = r.xc[e] = r.yw[e] = 0.0;
        r.mass = 0.0;
        return;
    }
    const int32_t* pm = a.p21 + (long long)b * a.N2;
    const double* P = a.Phi1 + b * a.s1;
    // (the Python layer checks the map; the clamp keeps a bad entry from ever becoming an address outside Phi1)
    const int p = min(max(pm[n], 0), nv1 - 1);
    const double* row = P + (long long)p * a.ld1;
    dm_load_row4<double>(row, m0 + lc, a.k1, al, r.xm);
    if constexpr (!DIAG) dm_load_row4<double>(row, c0 + lc, a.k1, al, r.xc);
    r.mass = a.mass2[(long long)b * a.N2 + n];
    const int32_t* cr = a.cols + ((long long)b * a.N2 + n) * a.nnz;
    const double* wr = a.w + ((long long)b * a.N2 + n) * a.nnz;
#pragma unroll
    for (int e = 0; e < 4; ++e) r.yw[e] = 0.0;
    for (int q = 0; q < a.nnz; ++q) {         // ELL order; a column outside the pair's vertices (padding -1, another mesh's row) adds nothing
        const int col = cr[q];
        const bool ok = col >= 0 && col < nv2;
        const double wv = ok ? wr[q] : 0.0;
        const int pc = min(max(pm[ok ? col : n], 0), nv1 - 1);
        double x[4];
        dm_load_row4<double>(P + (long long)pc * a.ld1, c0 + lc, a.k1, al, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) r.yw[e] = ok ? fma(wv, x[e], r.yw[e]) : r.yw[e];
    }
}

// grid = (tiles_m * tiles_c, nchunk, B), 256 threads = 4 waves (2 x 2), each wave a 32 x 32 sub-tile of both forms
template <bool DIAG_ONLY>
__global__ __launch_bounds__(256) void pullback_forms_kernel(pb_args a) {
    __shared__ double Xs[2][PB_SLAB * TN_LD];
    __shared__ double Ya[2][PB_SLAB * TN_LD];
    __shared__ double Yw[2][PB_SLAB * TN_LD];
    const int tiles = dm_cdiv(a.k1, TN_T);
    const int tm = blockIdx.x / tiles, tc = blockIdx.x % tiles;
    const int chunk = blockIdx.y, b = blockIdx.z;
    const int nv1 = a.nv1 ? a.nv1[b] : a.N1, nv2 = a.nv2 ? a.nv2[b] : a.N2;
    const int n0 = chunk * PB_CHUNK;
    if (n0 >= nv2) return;                                   // (uniform) the reduction does not read this partial
    const int m0 = tm * TN_T, c0 = tc * TN_T;
    const bool diag = DIAG_ONLY || tm == tc;                 // (uniform)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = t >> 4, lc = (t & 15) * 4;
    const bool al = dm_rows_aligned<double>(a.Phi1, a.s1, a.ld1);
    const int ns = dm_cdiv(min(nv2 - n0, PB_CHUNK), PB_SLAB);

    f64x4 acca[2][2], accw[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acca[i][j] = accw[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    // 16 x 16 blocks that lie completely outside the k1 x k1 result are skipped (wave-uniform)
    const bool vm[2] = {m0 + wm * 32 < a.k1, m0 + wm * 32 + 16 < a.k1};
    const bool vn[2] = {c0 + wn * 32 < a.k1, c0 + wn * 32 + 16 < a.k1};

    pb_regs r;
#define PB_FETCH(s_)                                                                                            \
    {                                                                                                           \
        if (diag) pb_fetch<true>(a, b, n0 + (s_) * PB_SLAB + lrow, nv1, nv2, m0, c0, lc, al, r);                \
        else pb_fetch<false>(a, b, n0 + (s_) * PB_SLAB + lrow, nv1, nv2, m0, c0, lc, al, r);                    \
    }
#define PB_STASH(buf_)                                                                                          \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                             \
        Xs[buf_][lrow * TN_LD + lc + e] = r.xm[e];                                                              \
        Ya[buf_][lrow * TN_LD + lc + e] = r.mass * (diag ? r.xm[e] : r.xc[e]);                                  \
        Yw[buf_][lrow * TN_LD + lc + e] = r.yw[e];                                                              \
    }
    PB_FETCH(0)
    PB_STASH(0)
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
        const int buf = s & 1;
        if (s + 1 < ns) PB_FETCH(s + 1)                      // (uniform) the next slab's rows travel while this one is multiplied
#pragma unroll
        for (int ks = 0; ks < PB_SLAB / 4; ++ks) {
            const int kk = ks * 4 + (lane >> 4);
            double x[2], ya[2], yw[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) x[mt] = Xs[buf][kk * TN_LD + wm * 32 + mt * 16 + (lane & 15)];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                ya[nt] = Ya[buf][kk * TN_LD + wn * 32 + nt * 16 + (lane & 15)];
                yw[nt] = Yw[buf][kk * TN_LD + wn * 32 + nt * 16 + (lane & 15)];
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    if (vm[mt] && vn[nt]) {
                        acca[mt][nt] = mfma_f64_16x16x4(x[mt], ya[nt], acca[mt][nt]);
                        accw[mt][nt] = mfma_f64_16x16x4(x[mt], yw[nt], accw[mt][nt]);
                    }
        }
        if (s + 1 < ns) PB_STASH(buf ^ 1)                    // (its last readers passed the barrier of the previous slab)
        __syncthreads();
    }
#undef PB_FETCH
#undef PB_STASH
    const long long kk1 = (long long)a.k1 * a.k1;
    double* pa = a.part + ((long long)chunk * a.B + b) * 2 * kk1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = m0 + wm * 32 + mt * 16 + (lane >> 4) + 4 * q;
                const int c = c0 + wn * 32 + nt * 16 + (lane & 15);
                if (m < a.k1 && c < a.k1) {
                    pa[(long long)m * a.k1 + c] = acca[mt][nt][q];
                    pa[kk1 + (long long)m * a.k1 + c] = accw[mt][nt][q];
                }
            }
}

// Ga / Gw [b][m][c] = sum over the pair's chunks, in chunk order; Gw's row m times inv1[b][m] when given (a cut row: exactly +0)
__global__ __launch_bounds__(256) void pullback_reduce_kernel(const double* __restrict__ part, const int32_t* __restrict__ nv2, int N2, int B, int k1,
                                                              const double* __restrict__ inv1, double* __restrict__ Ga, double* __restrict__ Gw) {
    const long long kk1 = (long long)k1 * k1;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= kk1) return;
    const int nc = dm_cdiv(nv2 ? nv2[b] : N2, PB_CHUNK);
    double sa = 0.0, sw = 0.0;
    for (int q = 0; q < nc; ++q) {
        const double* p = part + ((long long)q * B + b) * 2 * kk1;
        sa += p[i];
        sw += p[kk1 + i];
    }
    if (Ga) Ga[b * kk1 + i] = sa;
    if (Gw) {
        if (inv1) {
            const double s = inv1[(long long)b * k1 + (int)(i / k1)];
            sw = s == 0.0 ? 0.0 : s * sw;
        }
        Gw[b * kk1 + i] = sw;
    }
}

extern "C" int dm_pullback_forms_f64(dm_ctx* ctx, int B, int N1, int N2, int k1, const int32_t* p21, const double* Phi1, int ld1,
                                     const int32_t* ell_cols, const double* w_vals, int nnz, const double* mass2, const int32_t* n_verts1,
                                     const int32_t* n_verts2, const double* lam1, int ld_l1, double* Ga, double* Gw) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N1 > 0 && N2 > 0 && k1 > 0 && nnz > 0, "sizes must be positive");
    DM_REQUIRE(ctx, k1 <= SD_MAX_K1, "up to 256 source eigenvectors");
    DM_REQUIRE(ctx, B <= 65535, "too many pairs for one launch: split the batch");
    DM_REQUIRE(ctx, p21 && Phi1 && ell_cols && w_vals && mass2 && (Ga || Gw), "null pointer");
    DM_REQUIRE(ctx, ld1 >= k1, "eigenvector row stride smaller than k1");
    DM_REQUIRE(ctx, !lam1 || ld_l1 >= k1, "fewer than k1 eigenvalues per pair");
    for (int b = 0; b < B; ++b) {
        if (n_verts1 && (n_verts1[b] < 1 || n_verts1[b] > N1)) return dm_fail(ctx, DM_EINVAL, "dm_pullback_forms_f64: n_verts1[%d] = %d outside [1, %d]", b, n_verts1[b], N1);
        if (n_verts2 && (n_verts2[b] < 1 || n_verts2[b] > N2)) return dm_fail(ctx, DM_EINVAL, "dm_pullback_forms_f64: n_verts2[%d] = %d outside [1, %d]", b, n_verts2[b], N2);
    }
    const int nchunk = dm_cdiv(N2, PB_CHUNK);
    DM_REQUIRE(ctx, nchunk <= 65535, "too many target vertices for one launch");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bP = (size_t)nchunk * B * 2 * k1 * k1 * 8, bI = (size_t)B * 4, bV = (size_t)B * k1 * 8;
    int rc = dm_ws_reserve(ctx, dm_align_up(bP) + 2 * dm_align_up(bI) + dm_align_up(bV) + 1024);
    if (rc) return rc;
    pb_args a;
    a.part = (double*)dm_ws_take(ctx, bP);
    int32_t* d_nv1 = n_verts1 ? (int32_t*)dm_ws_take(ctx, bI) : nullptr;
    int32_t* d_nv2 = n_verts2 ? (int32_t*)dm_ws_take(ctx, bI) : nullptr;
    double* inv1 = (lam1 && Gw) ? (double*)dm_ws_take(ctx, bV) : nullptr;
    if (!a.part || (n_verts1 && !d_nv1) || (n_verts2 && !d_nv2) || (lam1 && Gw && !inv1))
        return dm_fail(ctx, DM_ENOMEM, "pullback_forms: workspace not reserved");
    if (n_verts1) DM_CHECK_HIP(ctx, hipMemcpyAsync(d_nv1, n_verts1, bI, hipMemcpyHostToDevice, ctx->stream));
    if (n_verts2) DM_CHECK_HIP(ctx, hipMemcpyAsync(d_nv2, n_verts2, bI, hipMemcpyHostToDevice, ctx->stream));
    if (n_verts1 || n_verts2) DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (the caller's host arrays may go away with this call)
    a.p21 = p21; a.Phi1 = Phi1; a.s1 = (long long)N1 * ld1; a.ld1 = ld1;
    a.cols = ell_cols; a.w = w_vals; a.nnz = nnz; a.mass2 = mass2;
    a.nv1 = d_nv1; a.nv2 = d_nv2; a.N1 = N1; a.N2 = N2; a.k1 = k1; a.B = B;
    if (inv1) DM_LAUNCH(ctx, "shape_diff_inv", sd_inv_kernel, dim3(B), dim3(256), 0, lam1, ld_l1, k1, inv1);
    const int tiles = dm_cdiv(k1, TN_T);
    const dim3 grid(tiles * tiles, nchunk, B);
    if (tiles == 1) DM_LAUNCH(ctx, "pullback_forms_f64", pullback_forms_kernel<true>, grid, dim3(256), 0, a);
    else DM_LAUNCH(ctx, "pullback_forms_f64", pullback_forms_kernel<false>, grid, dim3(256), 0, a);
    DM_LAUNCH(ctx, "pullback_reduce", pullback_reduce_kernel, dim3((unsigned)(((long long)k1 * k1 + 255) / 256), B), dim3(256), 0,
              (const double*)a.part, (const int32_t*)d_nv2, N2, B, k1, (const double*)inv1, Ga, Gw);
    return DM_OK;
}

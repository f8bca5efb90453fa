// Orientation operators of the descriptors in the reduced basis on the device (dm_fmap_orient_ops): what
// FunctionalMapping.compute_orientation_op builds per descriptor with one sparse assembly and two sparse-dense products on the host.
//
// Reference arithmetic reproduced (oracle/dm_oracle.py: orientation_ops; pyFM/mesh/geometry.py:919-985, pyFM/functional.py:686-728,
// base_functions.py:430-478):  with I = [f0, f1, f2], J = [f1, f2, f0] over the 3 m (face, corner) rows e,
//   op_p[a][b] = sum_e Sij[e][p] left[I_e][a] (Phi[J_e][b] - Phi[I_e][b]) + sum_e Sji[e][p] left[J_e][a] (Phi[I_e][b] - Phi[J_e][b])
//              = sum_e (Sij[e][p] left[I_e][a] - Sji[e][p] left[J_e][a]) (Phi[J_e][b] - Phi[I_e][b])
//   Sij = [S_2, S_3, S_1] / 3,  Sji = [S_1, S_2, S_3] / 3,  S_x[f][p] = J_x . (n x grad f_p) = sum_c F[f_c][p] (J_x . (n x g_c))
//   J_c = n x (edge opposite to corner c) / 2,  g_c = J_c / area,  left = Phi * row_scale[:, None]
// S is linear in the descriptor, so a face contributes through nine geometric coefficients W[x][c] = J_x . (n x g_c) / 3 (float64 from the
// float64 vertices, orient_face_coef_kernel), and the operators of ALL descriptors of a mesh are one product
//   (D k) x 3m  times  3m x k      rows (p, a) flattened: a small k (15) still fills the 64-row tile
// on the f64 matrix cores (gemm_tn_f64), both operands generated from gathers: rows of Phi, three entries of F, the face's coefficients.
//
// One z-slot per mesh.  Split-K over the 3m rows in chunks whose length depends on (D, k) only -- never on the other meshes of the call, nor
// on the padded face count: rows of faces beyond n_faces[b] are zeros, and a chunk of zeros adds +0.0 -- into workspace partials that
// orient_reduce_kernel adds in split order.  No atomics, the output is written once: the same input gives the same bits, in any batch.
#include "dm_gemm_f64.h"
#include "dm_internal.h"

// the vertices of the face a K row (face, corner) belongs to and the row's own pair I = f[corner], J = f[corner + 1], fetched one stage
// before the rows they select; v0 < 0: a padded face (the row is zero).  (I, J are read by index from memory: selecting them from
// v0 .. v2 by the corner made the compiler keep the struct in scratch)
struct OrFace { int v0, v1, v2, vI, vJ; };

__device__ __forceinline__ OrFace orient_face(const int32_t* __restrict__ faces, const int32_t* __restrict__ nf, int M, int N, int b, int n) {
    const int f = n / 3;
    if (nf && f >= nf[b]) return OrFace{-1, 0, 0, 0, 0};
    const int c = n - 3 * f;
    const int32_t* q = faces + ((long long)b * M + f) * 3;
    // (the callers check the indices on the host; the clamp keeps a bad one from ever becoming an address outside the mesh)
    return OrFace{min(max(q[0], 0), N - 1), min(max(q[1], 0), N - 1), min(max(q[2], 0), N - 1), min(max(q[c], 0), N - 1),
                  min(max(q[c == 2 ? 0 : c + 1], 0), N - 1)};
}

// W[b][f][x][c] = J_x . (n x g_c) / 3; zeros for padded faces
__global__ __launch_bounds__(256) void orient_face_coef_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                               const int32_t* __restrict__ nf, int N, int M, double* __restrict__ W) {
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f >= M) return;
    double* w = W + ((long long)b * M + f) * 9;
    const OrFace fc = orient_face(faces, nf, M, N, b, 3 * f);
    if (fc.v0 < 0) {
#pragma unroll
        for (int q = 0; q < 9; ++q) w[q] = 0.0;
        return;
    }
    const int vi[3] = {fc.v0, fc.v1, fc.v2};
    double v[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double* p = verts + ((long long)b * N + vi[c]) * 3;
        v[c][0] = p[0]; v[c][1] = p[1]; v[c][2] = p[2];
    }
    auto cross = [](const double (&a)[3], const double (&c)[3], double (&o)[3]) {
        o[0] = a[1] * c[2] - a[2] * c[1];
        o[1] = a[2] * c[0] - a[0] * c[2];
        o[2] = a[0] * c[1] - a[1] * c[0];
    };
    double e1[3], e2[3], nn[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { e1[d] = v[1][d] - v[0][d]; e2[d] = v[2][d] - v[0][d]; }
    cross(e1, e2, nn);
    const double len = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
    const double area = 0.5 * len;
    double nrm[3] = {nn[0] / len, nn[1] / len, nn[2] / len};
    double J[3][3], ng[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double opp[3], ne[3], g[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) opp[d] = v[(c + 2) % 3][d] - v[(c + 1) % 3][d];      // v3 - v2, v1 - v3, v2 - v1
        cross(nrm, opp, ne);
#pragma unroll
        for (int d = 0; d < 3; ++d) { J[c][d] = ne[d] / 2.0; g[d] = ne[d] / (2.0 * area); }
        cross(nrm, g, ng[c]);
    }
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int c = 0; c < 3; ++c) w[x * 3 + c] = (J[x][0] * ng[c][0] + J[x][1] * ng[c][1] + J[x][2] * ng[c][2]) / 3.0;
}

// X[e][(p, a)] = Sij[e][p] left[I_e][a] - Sji[e][p] left[J_e][a]     (K row e = 3 f + corner; output rows m = p k + a)
template <typename TR, typename TF>
struct OrientLeft {
    typedef OrFace pre_t;
    struct raw_t { TR lI[4], lJ[4]; double sI, sJ; TF f[4][3]; double cij[3], cji[3]; };
    const TR* Phi; long long stride_b; int ld; int k; int N;
    const double* scale;                       // (B, N), nullable: rows of left are scale * Phi
    const TF* F; int D;                        // (B, N, D)
    const int32_t* faces; const int32_t* nf; int M;
    const double* W;                           // (B, M, 9)
    __device__ __forceinline__ OrFace pre(int b, int n) const { return orient_face(faces, nf, M, N, b, n); }
    __device__ __forceinline__ void load4raw(int b, int n, int col0, const OrFace& fc, raw_t& r) const {
        // (a padded face: vertex 0 everywhere and no descriptor in range -- every entry below is then a zero, without a second path)
        const int Dlim = fc.v0 < 0 ? 0 : D;
        const int f = n / 3, c = n - 3 * f;
        const int vI = fc.vI, vJ = fc.vJ;
        const double* w = W + ((long long)b * M + f) * 9;
        const int xij = c == 2 ? 0 : c + 1;
#pragma unroll
        for (int q = 0; q < 3; ++q) { r.cij[q] = w[xij * 3 + q]; r.cji[q] = w[c * 3 + q]; }
        r.sI = scale ? scale[(long long)b * N + vI] : 1.0;
        r.sJ = scale ? scale[(long long)b * N + vJ] : 1.0;
        const TR* rowI = Phi + b * stride_b + (long long)vI * ld;
        const TR* rowJ = Phi + b * stride_b + (long long)vJ * ld;
        const TF* F0 = F + ((long long)b * N + max(fc.v0, 0)) * D;
        const TF* F1 = F + ((long long)b * N + fc.v1) * D;
        const TF* F2 = F + ((long long)b * N + fc.v2) * D;
        int p = col0 / k, a = col0 - p * k;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p < Dlim) {
                r.lI[e] = rowI[a]; r.lJ[e] = rowJ[a];
                r.f[e][0] = F0[p]; r.f[e][1] = F1[p]; r.f[e][2] = F2[p];
            } else {
                r.lI[e] = r.lJ[e] = (TR)0;
                r.f[e][0] = r.f[e][1] = r.f[e][2] = (TF)0;
            }
            if (++a == k) { a = 0; ++p; }
        }
    }
    static __device__ __forceinline__ void zero(raw_t& r) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r.lI[e] = r.lJ[e] = (TR)0;
            r.f[e][0] = r.f[e][1] = r.f[e][2] = (TF)0;
        }
        r.sI = r.sJ = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) r.cij[q] = r.cji[q] = 0.0;
    }
    static __device__ __forceinline__ void cvt(const raw_t& r, double (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double f0 = (double)r.f[e][0], f1 = (double)r.f[e][1], f2 = (double)r.f[e][2];
            const double sij = f0 * r.cij[0] + f1 * r.cij[1] + f2 * r.cij[2];
            const double sji = f0 * r.cji[0] + f1 * r.cji[1] + f2 * r.cji[2];
            v[e] = sij * (r.sI * (double)r.lI[e]) - sji * (r.sJ * (double)r.lJ[e]);
        }
    }
};

// Y[e][b] = Phi[J_e][b] - Phi[I_e][b]
template <typename TR>
struct OrientRight {
    typedef OrFace pre_t;
    struct raw_t { TR qI[4], qJ[4]; };
    const TR* Phi; long long stride_b; int ld; int k; int N;
    const int32_t* faces; const int32_t* nf; int M;
    __device__ __forceinline__ OrFace pre(int b, int n) const { return orient_face(faces, nf, M, N, b, n); }
    __device__ __forceinline__ void load4raw(int b, int n, int col0, const OrFace& fc, raw_t& r) const {
        const int vI = fc.vI, vJ = fc.vJ, kk = fc.v0 < 0 ? 0 : k;       // (a padded face: no column in range, zeros)
        const bool al = dm_rows_aligned<TR>(Phi, stride_b, ld);
        dm_load_row4<TR>(Phi + b * stride_b + (long long)vI * ld, col0, kk, al, r.qI);
        dm_load_row4<TR>(Phi + b * stride_b + (long long)vJ * ld, col0, kk, al, r.qJ);
    }
    static __device__ __forceinline__ void zero(raw_t& r) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r.qI[e] = r.qJ[e] = (TR)0;
    }
    static __device__ __forceinline__ void cvt(const raw_t& r, double (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (double)r.qJ[e] - (double)r.qI[e];
    }
};

struct OrientOut {                 // split-K partials (nsplit, B, D k, k), or the operators themselves when nsplit == 1
    double* p; long long Z; int M; int N;
    __device__ __forceinline__ void store(int z, int split, int m, int c, double v) const {
        p[(((long long)split * Z + z) * M + m) * N + c] = v;
    }
};

// out[i] = sum_q partial[q][i]   (fixed order)
__global__ __launch_bounds__(256) void orient_reduce_kernel(const double* __restrict__ partial, int nsplit, long long n, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int q = 0; q < nsplit; ++q) s += partial[(long long)q * n + i];
    out[i] = s;
}

template <typename TR, typename TF>
static int orient_launch(dm_ctx* ctx, int B, int N, int M, int D, int k, const int32_t* faces, const int32_t* d_nf, const TR* Phi, int ld,
                         const double* row_scale, const void* F, const double* W, int nsplit, int kchunk, double* dst) {
    OrientLeft<TR, TF> opx{Phi, (long long)N * ld, ld, k, N, row_scale, (const TF*)F, D, faces, d_nf, M, W};
    OrientRight<TR> opy{Phi, (long long)N * ld, ld, k, N, faces, d_nf, M};
    OrientOut out{dst, (long long)B, D * k, k};
    DM_LAUNCH(ctx, "orient_ops_tn_f64", (gemm_tn_f64<OrientLeft<TR, TF>, OrientRight<TR>, OrientOut>),
              dim3(dm_cdiv(D * k, TN_T) * dm_cdiv(k, TN_T), nsplit, B), dim3(256), 0, opx, opy, out, D * k, k, 3 * M, kchunk);
    return DM_OK;
}

template <typename TR>
static int orient_ops_impl(dm_ctx* ctx, int B, int N, int M, int D, int k, const double* verts, const int32_t* faces, const int32_t* n_faces,
                           const TR* Phi, int ld, const double* row_scale, const void* F, int f_dtype, double* ops) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && M > 0 && D > 0 && k > 0, "sizes must be positive");
    DM_REQUIRE(ctx, verts && faces && Phi && F && ops, "null pointer");
    DM_REQUIRE(ctx, ld >= k, "eigenvector row stride smaller than k");
    DM_REQUIRE(ctx, f_dtype == DM_F16 || f_dtype == DM_F32, "f_dtype must be DM_F16 or DM_F32");
    DM_REQUIRE(ctx, B <= 65535, "too many meshes for one launch: split the batch");
    DM_REQUIRE(ctx, (long long)D * k <= 0x7fffffffLL - TN_T && M <= (0x7fffffff - TN_BK) / 3, "operator rows D k or K rows 3 M beyond 2^31 - 1");
    for (int b = 0; n_faces && b < B; ++b)
        if (n_faces[b] < 0 || n_faces[b] > M) return dm_fail(ctx, DM_EINVAL, "dm_fmap_orient_ops: n_faces[%d] = %d outside [0, %d]", b, n_faces[b], M);
    // split-K: the chunk length follows from (D, k) alone, so a mesh's partial sums are the same in every call it is part of
    const long long tiles = (long long)dm_cdiv(D * k, TN_T) * dm_cdiv(k, TN_T);
    DM_REQUIRE(ctx, tiles <= 0x7fffffffLL, "too many output tiles for one launch");
    const long long mult = tiles / 32 < 1 ? 1 : (tiles / 32 > 16 ? 16 : tiles / 32);
    const int kchunk = (int)(512 * mult);
    const int nsplit = dm_cdiv(3 * M, kchunk);
    DM_REQUIRE(ctx, nsplit <= 65535, "too many K splits for one launch");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const long long n_out = (long long)B * D * k * k;
    const size_t bW = (size_t)B * M * 9 * 8, bP = nsplit > 1 ? (size_t)nsplit * n_out * 8 : 0, bI = n_faces ? (size_t)B * 4 : 0;
    int rc = dm_ws_reserve(ctx, dm_align_up(bW) + dm_align_up(bP) + dm_align_up(bI) + 1024);
    if (rc) return rc;
    double* W = (double*)dm_ws_take(ctx, bW);
    double* part = nsplit > 1 ? (double*)dm_ws_take(ctx, bP) : ops;
    int32_t* d_nf = n_faces ? (int32_t*)dm_ws_take(ctx, bI) : nullptr;
    if (!W || !part || (n_faces && !d_nf)) return dm_fail(ctx, DM_ENOMEM, "orient_ops: workspace not reserved");
    if (n_faces) {
        DM_CHECK_HIP(ctx, hipMemcpyAsync(d_nf, n_faces, bI, hipMemcpyHostToDevice, ctx->stream));
        DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (the caller's host array may go away with this call)
    }
    DM_LAUNCH(ctx, "orient_face_coef", orient_face_coef_kernel, dim3(dm_cdiv(M, 256), B), dim3(256), 0, verts, faces, (const int32_t*)d_nf, N, M, W);
    if (f_dtype == DM_F16) rc = orient_launch<TR, _Float16>(ctx, B, N, M, D, k, faces, d_nf, Phi, ld, row_scale, F, W, nsplit, kchunk, part);
    else rc = orient_launch<TR, float>(ctx, B, N, M, D, k, faces, d_nf, Phi, ld, row_scale, F, W, nsplit, kchunk, part);
    if (rc) return rc;
    if (nsplit > 1)
        DM_LAUNCH(ctx, "orient_reduce", orient_reduce_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (const double*)part, nsplit, n_out, ops);
    return DM_OK;
}

extern "C" int dm_fmap_orient_ops(dm_ctx* ctx, int B, int N, int M, int D, int k, const double* verts, const int32_t* faces,
                                  const int32_t* n_faces, const float* Phi, int ld, const double* row_scale, const void* F, int f_dtype,
                                  double* ops) {
    return orient_ops_impl<float>(ctx, B, N, M, D, k, verts, faces, n_faces, Phi, ld, row_scale, F, f_dtype, ops);
}
extern "C" int dm_fmap_orient_ops_f64(dm_ctx* ctx, int B, int N, int M, int D, int k, const double* verts, const int32_t* faces,
                                      const int32_t* n_faces, const double* Phi, int ld, const double* row_scale, const void* F, int f_dtype,
                                      double* ops) {
    return orient_ops_impl<double>(ctx, B, N, M, D, k, verts, faces, n_faces, Phi, ld, row_scale, F, f_dtype, ops);
}

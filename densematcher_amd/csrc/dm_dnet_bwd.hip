// DiffusionNet backward pass, fp32 on the matrix cores: dm_dnet_linear_bwd_data_f32, dm_dnet_linear_bwd_weight_f32,
// dm_dnet_diffuse_bwd_f32, dm_dnet_gradfeat_bwd_f32 -- the gradients of dm_dnet_linear_f32, dm_dnet_diffuse_f32, dm_dnet_gradfeat_f32
// (dm_dnet_layers.hip) with respect to their activations and parameters; the operators of a mesh are constants.
//
// Every product is v_mfma_f32_32x32x2_f32, an exact fp32 fmaf chain in ascending order of the contraction index that starts at +0, so
// the bits of an output element depend on its own row and column of the operands only: never on the tile it falls in, on the CU count,
// on the other meshes of the call or on the padding (operands beyond a mesh's rows, columns or ELL slots are staged as zeros, and
// fma(0, 0, s) = s for every s a chain from +0 can hold).  No atomics.  All loads are scalar: element alignment is enough.
//
// One tile kernel runs all seven products: 64 x 64 outputs per workgroup, four waves with one 32 x 32 block each, the contraction
// staged 32 deep through LDS with the next stage in registers while the current one is multiplied.  It takes up to two left and two
// right operands that share their stages (p1 = A0 B0, p2 = A1 B1, p3 = A1 B0, p4 = A0 B1: the complex products of the gradient
// features, or two spectra from one pass over the eigenvectors); an operand is described by a functor that returns one element or zero,
// and by whether the tile index or the contraction index is the one that is adjacent in memory, which picks the thread -> element map
// of its staging loads.  A functor either tests its indices and loads behind the test, or -- the weight gradient, whose contraction
// is the longest and whose grid the smallest -- loads unconditionally from indices clamped into the operand and selects zero
// afterwards, so that all loads of a stage are in flight together; measured per kernel, the faster form is kept (DESIGN.md section 4,
// 'DiffusionNet backward').  Neither forms an address outside a mesh's rows.  A gradient with respect to a parameter contracts over
// the vertices: one chain per mesh into the caller's workspace, then one pass that adds the meshes in ascending order.
//
// This file holds what is the fp32 family's own: the tile kernel, the operands of the diffusion and dm_dnet_diffuse_bwd_f32.  The
// operand functors of the linear layer and of the gradient features, the elementwise kernels, the argument checks and the bodies of the
// other three entries are those of dm_dnet_bwd_common.h for T = float, shared with dm_dnet_half_bwd.hip.
#include "dm_dnet_bwd_common.h"

typedef float db_f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int DB_T = 64;          // outputs per workgroup side
constexpr int DB_KC = 32;         // contraction depth per stage
constexpr int DB_LD = DB_T + 1;   // LDS row stride of a stage [kk][row]
constexpr int DB_KMAX = 1024;     // dm_dnet_diffuse_f32's limit: a forward pass beyond it does not exist
static_assert(DB_T == DNB_T, "the shared functors skip whole tiles of this side");

__device__ __forceinline__ int db_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// Op: N, nv; rows(), cols(): the extent of the output; depth(nvb): the contraction length; a(w, b, nvb, row, k), b(w, b, nvb, k, col):
// one operand element, zero outside the operand; skip(col0): nothing to store for this column tile; store(b, nvb, row, col, p1..p4)
// for row < rows(), col < cols().  A_TILE / B_TILE: the operand's tile index is the one adjacent in memory.
template <int NA, int NB, bool A_TILE, bool B_TILE, class Op>
__global__ __launch_bounds__(256) void db_tile_kernel(Op op) {
    __shared__ float As[NA][DB_KC * DB_LD], Bs[NB][DB_KC * DB_LD];
    const int b = blockIdx.z, row0 = blockIdx.y * DB_T, col0 = blockIdx.x * DB_T;
    if (op.skip(col0)) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int nvb = op.nv ? op.nv[b] : op.N;
    const int depth = op.depth(nvb);
    // element i of a thread's stage: (tile index, contraction index) inside the stage
    const int at = A_TILE ? (t & 63) : (t >> 5), ak = A_TILE ? (t >> 6) : (t & 31), ati = A_TILE ? 0 : 8, aki = A_TILE ? 4 : 0;
    const int bt = B_TILE ? (t & 63) : (t >> 5), bk = B_TILE ? (t >> 6) : (t & 31), bti = B_TILE ? 0 : 8, bki = B_TILE ? 4 : 0;
    float ra[NA][8], rb[NB][8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int w = 0; w < NA; ++w) ra[w][i] = op.a(w, b, nvb, row0 + at + ati * i, k0 + ak + aki * i);
#pragma unroll
            for (int w = 0; w < NB; ++w) rb[w][i] = op.b(w, b, nvb, k0 + bk + bki * i, col0 + bt + bti * i);
        }
    };
    db_f32x16 p1 = {0}, p2 = {0}, p3 = {0}, p4 = {0};
    fetch(0);
    for (int k0 = 0; k0 < depth; k0 += DB_KC) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int w = 0; w < NA; ++w) As[w][(ak + aki * i) * DB_LD + at + ati * i] = ra[w][i];
#pragma unroll
            for (int w = 0; w < NB; ++w) Bs[w][(bk + bki * i) * DB_LD + bt + bti * i] = rb[w][i];
        }
        __syncthreads();
        if (k0 + DB_KC < depth) fetch(k0 + DB_KC);
#pragma unroll
        for (int s = 0; s < DB_KC / 2; ++s) {
            const int oa = (2 * s + h) * DB_LD + 32 * wr + r, ob = (2 * s + h) * DB_LD + 32 * wc + r;
            const float a0 = As[0][oa], b0 = Bs[0][ob];
            p1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, p1, 0, 0, 0);
            if (NA == 2) p3 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[NA - 1][oa], b0, p3, 0, 0, 0);
            if (NB == 2) p4 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, Bs[NB - 1][ob], p4, 0, 0, 0);
            if (NA == 2 && NB == 2) p2 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[NA - 1][oa], Bs[NB - 1][ob], p2, 0, 0, 0);
        }
        __syncthreads();
    }
    const int col = col0 + 32 * wc + r;
    if (col >= op.cols()) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = row0 + 32 * wr + db_row(reg, h);
        if (row < op.rows()) op.store(b, nvb, row, col, p1[reg], p2[reg], p3[reg], p4[reg]);
    }
}

template <int NA, int NB, bool A_TILE, bool B_TILE, class Op>
int db_launch(dm_ctx* ctx, const char* name, int B, const Op& op) {
    DM_LAUNCH(ctx, name, (db_tile_kernel<NA, NB, A_TILE, B_TILE, Op>), dim3(dm_cdiv(op.cols(), DB_T), dm_cdiv(op.rows(), DB_T), B), dim3(256), 0, op);
    return DM_OK;
}

struct db_family {
    static constexpr const char *sum = "dnet_bwd_sum", *lin_data = "dnet_linear_bwd_data", *lin_weight = "dnet_linear_bwd_weight",
                                *gf_gather = "dnet_gradfeat_bwd_gather", *gf_fwd = "dnet_gradfeat_bwd_fwd", *gf_grad = "dnet_gradfeat_bwd_grad",
                                *gf_gather_t = "dnet_gradfeat_bwd_gather_t", *gf_param = "dnet_gradfeat_bwd_param";
    // (one schedule for every contraction: the weight gradient's loads are clamped instead, dnb_lin_common::dz_clamped)
    template <int NA, int NB, bool A_TILE, bool B_TILE, bool OVER_VERTS, class Op>
    static int tile(dm_ctx* ctx, const char* name, int B, const Op& op) { return db_launch<NA, NB, A_TILE, B_TILE>(ctx, name, B, op); }
};

// ---------------------------------------------------------------------------------------------------------------- diffuse
struct dif_spec_op {                                           // g = evecs^T dO, s = evecs^T (mass * x) -> H = coef * g, T = evals coef g s
    int N, K, C;
    const int32_t* nv;
    const float* dO; int lddo; const float* x; int ldx; const float* mass; const float* evals; const float* evecs; int lde; const float* times;
    float* H; float* T;                                        // [B][K][C]; T null: no dtimes
    __device__ __host__ __forceinline__ int rows() const { return K; }
    __device__ __host__ __forceinline__ int cols() const { return C; }
    __device__ __forceinline__ int depth(int nvb) const { return nvb; }
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ float a(int, int b, int nvb, int k, int i) const {
        return (i < nvb && k < K) ? evecs[((long long)b * N + i) * lde + k] : 0.f;
    }
    __device__ __forceinline__ float b(int w, int b, int nvb, int i, int c) const {
        if (i >= nvb || c >= C) return 0.f;
        const long long br = (long long)b * N + i;
        return w == 0 ? dO[br * lddo + c] : __fmul_rn(mass[br], x[br * ldx + c]);
    }
    __device__ __forceinline__ void store(int b, int, int k, int c, float g, float, float, float s) const {
        const float ev = evals[(long long)b * K + k];
        // the forward's coefficient: the clamp in fp32, the exponent and exp() in float64, one rounding
        const float coef = (float)exp(-(double)ev * (double)fmaxf(times[c], 1e-8f));
        const long long o = ((long long)b * K + k) * C + c;
        H[o] = __fmul_rn(coef, g);
        if (T) T[o] = __fmul_rn(__fmul_rn(__fmul_rn(ev, coef), g), s);
    }
};

struct dif_back_op {                                           // dx = mass ⊙ (evecs H)
    int N, K, C;
    const int32_t* nv;
    const float* mass; const float* evecs; int lde; const float* H;
    float* dx; int lddx;
    __device__ __host__ __forceinline__ int rows() const { return N; }
    __device__ __host__ __forceinline__ int cols() const { return C; }
    __device__ __forceinline__ int depth(int) const { return K; }
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ float a(int, int b, int nvb, int i, int k) const {
        return (i < nvb && k < K) ? evecs[((long long)b * N + i) * lde + k] : 0.f;
    }
    __device__ __forceinline__ float b(int, int b, int, int k, int c) const { return (k < K && c < C) ? H[((long long)b * K + k) * C + c] : 0.f; }
    __device__ __forceinline__ void store(int b, int nvb, int i, int c, float p1, float, float, float) const {
        const long long br = (long long)b * N + i;
        dx[br * lddx + c] = i < nvb ? __fmul_rn(mass[br], p1) : 0.f;
    }
};
}  // namespace

extern "C" int dm_dnet_linear_bwd_data_f32(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/,
                                           int ldy, int act, const float* W, int ldw, const int32_t* n_verts /*nullable*/, float* d0 /*nullable*/,
                                           int w0, int ld0, float* d1 /*nullable*/, int w1, int ld1, float* d2 /*nullable*/, int w2, int ld2) {
    if (!ctx) return DM_EINVAL;
    float* d[3] = {d0, d1, d2};
    int w[3] = {w0, w1, w2}, ld[3] = {ld0, ld1, ld2};
    return dnb_linear_bwd_data<float, db_family>(ctx, __func__, B, N, C_out, n_src, dY, lddy, Y, ldy, act, W, ldw, n_verts, d, w, ld);
}

extern "C" size_t dm_dnet_linear_bwd_bytes(int B, int C_out, int k_tot) {
    if (B <= 0 || C_out <= 0 || k_tot <= 0) return 0;
    return (size_t)B * C_out * ((size_t)k_tot + 1) * sizeof(float);
}

extern "C" int dm_dnet_linear_bwd_weight_f32(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/,
                                             int ldy, int act, const float* src0, int w0, int ld0, const float* src1, int w1, int ld1,
                                             const float* src2, int w2, int ld2, const int32_t* n_verts /*nullable*/, void* ws,
                                             float* dW /*nullable*/, int lddw, float* db /*nullable*/) {
    if (!ctx) return DM_EINVAL;
    const void* src[3] = {src0, src1, src2};
    int w[3] = {w0, w1, w2}, ld[3] = {ld0, ld1, ld2};
    return dnb_linear_bwd_weight<float, db_family>(ctx, __func__, B, N, C_out, n_src, dY, lddy, Y, ldy, act, src, w, ld, nullptr, n_verts, ws, dW, lddw,
                                                   db);
}

extern "C" size_t dm_dnet_diffuse_bwd_bytes(int B, int K, int C) {
    if (B <= 0 || K <= 0 || C <= 0) return 0;
    return 2 * (size_t)B * K * C * sizeof(float);
}

extern "C" int dm_dnet_diffuse_bwd_f32(dm_ctx* ctx, int B, int N, int K, int C, const float* dO, int lddo, const float* x /*nullable*/, int ldx,
                                       const float* mass, const float* evals, const float* evecs, int lde, const float* times,
                                       const int32_t* n_verts /*nullable*/, void* ws, float* dx /*nullable*/, int lddx, float* dtimes /*nullable*/) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && K > 0 && C > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, K <= DB_KMAX, "K <= 1024, the limit of dm_dnet_diffuse_f32");
    DM_REQUIRE(ctx, dO && mass && evals && evecs && times && ws, "null pointer");
    DM_REQUIRE(ctx, lddo >= C && lde >= K, "lddo >= C, lde >= K");
    DM_REQUIRE(ctx, !dtimes || (x && ldx >= C), "dtimes needs the saved x, ldx >= C");
    DM_REQUIRE(ctx, !dx || lddx >= C, "lddx >= C");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "dm_dnet_diffuse_bwd_f32", B, N, n_verts)) return rc;
    if (!dx && !dtimes) return DM_OK;
    float* H = (float*)ws;
    float* T = dtimes ? H + (size_t)B * K * C : nullptr;
    dif_spec_op sp{N, K, C, n_verts, dO, lddo, x, ldx, mass, evals, evecs, lde, times, H, T};
    if (int rc = dtimes ? db_launch<1, 2, true, true>(ctx, "dnet_diffuse_bwd_spec", B, sp) : db_launch<1, 1, true, true>(ctx, "dnet_diffuse_bwd_spec", B, sp))
        return rc;
    if (dx) {
        dif_back_op bk{N, K, C, n_verts, mass, evecs, lde, H, dx, lddx};
        if (int rc = db_launch<1, 1, false, true>(ctx, "dnet_diffuse_bwd_back", B, bk)) return rc;
    }
    if (dtimes) {
        DM_LAUNCH(ctx, "dnet_diffuse_bwd_times", dnb_times_mesh_kernel, dim3(dm_cdiv(C, 64), B), dim3(64), 0, T, K, C);
        DM_LAUNCH(ctx, "dnet_diffuse_bwd_times", dnb_times_kernel, dim3(dm_cdiv(C, 64)), dim3(64), 0, (const float*)T, B, K, C, dtimes);
    }
    return DM_OK;
}

extern "C" size_t dm_dnet_gradfeat_bwd_bytes(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0) return 0;
    return (6 * (size_t)B * N * C + 2 * (size_t)B * C * C) * sizeof(float);
}

extern "C" int dm_dnet_gradfeat_bwd_f32(dm_ctx* ctx, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx,
                                        const float* gy, int nnz_t, const int32_t* row_len_t, const int32_t* cols_t, const float* gx_t,
                                        const float* gy_t, const float* dO, int lddo, const float* x, int ldx, const float* A_re,
                                        const float* A_im /*nullable*/, int lda, const int32_t* n_verts /*nullable*/, void* ws, float* dx /*nullable*/,
                                        int lddx, float* dA_re /*nullable*/, float* dA_im /*nullable*/, int ldda) {
    if (!ctx) return DM_EINVAL;
    return dnb_gradfeat_bwd<float, db_family>(ctx, __func__, B, N, C, nnz, row_len, cols, gx, gy, nnz_t, row_len_t, cols_t, gx_t, gy_t, dO, lddo, x, ldx,
                                              A_re, A_im, lda, n_verts, ws, dx, lddx, dA_re, dA_im, ldda);
}

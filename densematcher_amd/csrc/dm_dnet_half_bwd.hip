// DiffusionNet backward pass for mixed-precision training, fp16 operands on the matrix cores: dm_dnet_linear_bwd_data_f16,
// dm_dnet_linear_bwd_weight_f16, dm_dnet_diffuse_bwd_f16, dm_dnet_gradfeat_bwd_f16 -- the gradients of dm_dnet_linear_f16,
// dm_dnet_diffuse_f16, dm_dnet_gradfeat_f16 (dm_dnet_half.hip) with respect to their activations and to the fp32 master parameters
// whose fp16 roundings the forward multiplied; the operators of a mesh are constants.  The gradient of the diffusion with respect to x
// is a call of dm_dnet_diffuse_f16 itself.
//
// This file holds what is the fp16 family's own: the tile kernel, the operand of the diffusion's time gradient and
// dm_dnet_diffuse_bwd_f16.  The operand functors of the linear layer and of the gradient features, the elementwise kernels, the argument
// checks and the bodies of the other three entries are those of dm_dnet_bwd_common.h for T = _Float16, shared with dm_dnet_bwd.hip: the
// two families differ there in the element type of a staged operand and in nothing else, and the tests hold both to their bits.
//
// Every product is v_mfma_f32_32x32x16_f16: exact fp16 x fp16 products accumulated in fp32, the contraction index in ascending chunks of
// 16 from a zero accumulator, never split, no atomics.  Lane (r = lane & 31, h = lane >> 5) of a step holds A[row r][k = 8 h + j] and
// B[k = 8 h + j][col r], j = 0 .. 7; accumulator register `reg` is row (reg & 3) + 8 (reg >> 2) + 4 h, column r.  Tiles start at
// multiples of 64 rows and columns and every tile walks the same chunks, so the bits of an output element depend on its own row and
// column of the operands only: not on the tile it falls in, the other meshes of the call or the padding (operands behind a mesh's rows,
// a matrix's columns or an ELL row's slots are staged as zeros).
//
// Roundings to fp16 (round to nearest even; a magnitude beyond 65504 becomes infinite), each as the operand is staged, nowhere else:
//   linear    dZ = dY * [Y > 0]; an fp32 source of the weight gradient (the value the forward multiplied).
//   diffuse   dO; x (for dtimes); the spectrum of dx once, at the scale 2^(14 - e1 - e2) (dm_dnet_diffuse_f16).
//   gradfeat  gX, gY, U, V as operands of the products with A_h and of dA_re, dA_im.
// Gradients of activations leave in fp32.  A gradient of a parameter contracts over the vertices: one fp32 chain per mesh into the
// caller's workspace, then one pass that adds the meshes in ascending order.  It is the gradient of the fp32 master parameter: the
// rounding of the matrix is passed straight through.
//
// One tile kernel runs every product: 64 x 64 outputs per workgroup, four waves with one 32 x 32 block each, the contraction staged 32
// deep through LDS.  It takes up to two left and two right operands that share their stages (p1 = A0 B0, p2 = A1 B1 and, with CROSS,
// p3 = A1 B0, p4 = A0 B1); an operand is a functor that returns one fp16 element or zero, and the flag that says whether its tile index
// or the contraction index is adjacent in memory picks the thread -> element map of its staging loads.  All loads are scalar: element
// alignment is enough.  AHEAD = 2 keeps the loads of two stages in flight (the weight gradient, whose contraction over the vertices is
// the longest and whose grid the smallest).
#include <math.h>

#include <type_traits>

#include <hip/hip_fp16.h>

#include "dm_dnet_bwd_common.h"

typedef float hb_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 hb_f16x8 __attribute__((ext_vector_type(8)));

namespace {
constexpr int HB_T = 64;             // outputs per workgroup side
constexpr int HB_KC = 32;            // contraction depth per stage: two chunks of 16
constexpr int HB_LD = HB_KC + 8;     // LDS row [tile index][k] in halves: 80 bytes, the 16-byte fragment reads stay aligned
constexpr int HB_KMAX = 1024;        // dm_dnet_diffuse_f16's limit: a forward pass beyond it does not exist
static_assert(HB_T == DNB_T, "the shared functors skip whole tiles of this side");

__device__ __forceinline__ int hb_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
__device__ __forceinline__ _Float16 hb_zero() { return (_Float16)0.0f; }

// Op: N, nv; rows(), cols(): the extent of the output; depth(nvb): the contraction length; a(w, b, nvb, row, k), b(w, b, nvb, k, col):
// one operand element in fp16, zero outside the operand; skip(col0): nothing to store for this column tile; store(b, nvb, row, col,
// p1..p4) for row < rows(), col < cols().  A_TILE / B_TILE: the operand's tile index is the one adjacent in memory.
template <int NA, int NB, bool A_TILE, bool B_TILE, bool CROSS, int AHEAD, class Op>
__global__ __launch_bounds__(256) void hb_tile_kernel(Op op) {
    __shared__ __attribute__((aligned(16))) _Float16 As[NA][HB_T * HB_LD], Bs[NB][HB_T * HB_LD];
    const int b = blockIdx.z, row0 = blockIdx.y * HB_T, col0 = blockIdx.x * HB_T;
    if (op.skip(col0)) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int nvb = op.nv ? op.nv[b] : op.N;
    const int depth = op.depth(nvb);
    // element i of a thread's stage: (tile index, contraction index) inside the stage.  Tile index adjacent in memory: a wave loads 64
    // adjacent tile indices at one contraction index, and a thread's eight elements are eight adjacent contraction indices of one row
    // of the stage -- one 16-byte store.  Contraction index adjacent: 32 adjacent contraction indices of the rows (t >> 5) + 8 i.
    const int at = A_TILE ? (t & 63) : (t >> 5), ak = A_TILE ? 8 * (t >> 6) : (t & 31), ati = A_TILE ? 0 : 8, aki = A_TILE ? 1 : 0;
    const int bt = B_TILE ? (t & 63) : (t >> 5), bk = B_TILE ? 8 * (t >> 6) : (t & 31), bti = B_TILE ? 0 : 8, bki = B_TILE ? 1 : 0;
    _Float16 ra[AHEAD][NA][8], rb[AHEAD][NB][8];
    hb_f32x16 p1 = {0}, p2 = {0}, p3 = {0}, p4 = {0};
    // one stage: the registers of slot S go to LDS, the slot is refilled AHEAD stages on, the stage is multiplied
    auto stage = [&](auto slot, int k0) {
        constexpr int S = decltype(slot)::value;
#pragma unroll
        for (int w = 0; w < NA; ++w) {
            if (A_TILE) {
                hb_f16x8 v;
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = ra[S][w][i];
                *reinterpret_cast<hb_f16x8*>(&As[w][at * HB_LD + ak]) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) As[w][(at + ati * i) * HB_LD + ak] = ra[S][w][i];
            }
        }
#pragma unroll
        for (int w = 0; w < NB; ++w) {
            if (B_TILE) {
                hb_f16x8 v;
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = rb[S][w][i];
                *reinterpret_cast<hb_f16x8*>(&Bs[w][bt * HB_LD + bk]) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) Bs[w][(bt + bti * i) * HB_LD + bk] = rb[S][w][i];
            }
        }
        __syncthreads();
        const int kn = k0 + AHEAD * HB_KC;
        if (kn < depth) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int w = 0; w < NA; ++w) ra[S][w][i] = op.a(w, b, nvb, row0 + at + ati * i, kn + ak + aki * i);
#pragma unroll
                for (int w = 0; w < NB; ++w) rb[S][w][i] = op.b(w, b, nvb, kn + bk + bki * i, col0 + bt + bti * i);
            }
        }
#pragma unroll
        for (int s = 0; s < HB_KC / 16; ++s) {
            const int oa = (32 * wr + r) * HB_LD + 16 * s + 8 * h, ob = (32 * wc + r) * HB_LD + 16 * s + 8 * h;
            const hb_f16x8 a0 = *reinterpret_cast<const hb_f16x8*>(&As[0][oa]), b0 = *reinterpret_cast<const hb_f16x8*>(&Bs[0][ob]);
            p1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, p1, 0, 0, 0);
            if (NA == 2 && CROSS) p3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const hb_f16x8*>(&As[NA - 1][oa]), b0, p3, 0, 0, 0);
            if (NB == 2 && CROSS) p4 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, *reinterpret_cast<const hb_f16x8*>(&Bs[NB - 1][ob]), p4, 0, 0, 0);
            if (NA == 2 && NB == 2)
                p2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const hb_f16x8*>(&As[NA - 1][oa]),
                                                            *reinterpret_cast<const hb_f16x8*>(&Bs[NB - 1][ob]), p2, 0, 0, 0);
        }
        __syncthreads();
    };
#pragma unroll
    for (int S = 0; S < AHEAD; ++S) {
        const int kn = S * HB_KC;
        if (kn < depth || S == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int w = 0; w < NA; ++w) ra[S][w][i] = op.a(w, b, nvb, row0 + at + ati * i, kn + ak + aki * i);
#pragma unroll
                for (int w = 0; w < NB; ++w) rb[S][w][i] = op.b(w, b, nvb, kn + bk + bki * i, col0 + bt + bti * i);
            }
        }
    }
    for (int k0 = 0; k0 < depth; k0 += AHEAD * HB_KC) {
        stage(std::integral_constant<int, 0>{}, k0);
        if (AHEAD == 2 && k0 + HB_KC < depth) stage(std::integral_constant<int, AHEAD - 1>{}, k0 + HB_KC);      // (uniform in the workgroup)
    }
    const int col = col0 + 32 * wc + r;
    if (col >= op.cols()) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = row0 + 32 * wr + hb_row(reg, h);
        if (row < op.rows()) op.store(b, nvb, row, col, p1[reg], p2[reg], p3[reg], p4[reg]);
    }
}

template <int NA, int NB, bool A_TILE, bool B_TILE, bool CROSS, int AHEAD, class Op>
int hb_launch(dm_ctx* ctx, const char* name, int B, const Op& op) {
    DM_LAUNCH(ctx, name, (hb_tile_kernel<NA, NB, A_TILE, B_TILE, CROSS, AHEAD, Op>), dim3(dm_cdiv(op.cols(), HB_T), dm_cdiv(op.rows(), HB_T), B),
              dim3(256), 0, op);
    return DM_OK;
}

struct hb_family {
    static constexpr const char *sum = "dnet_bwd_f16_sum", *lin_data = "dnet_linear_bwd_data_f16", *lin_weight = "dnet_linear_bwd_weight_f16",
                                *gf_gather = "dnet_gradfeat_bwd_f16_gather", *gf_fwd = "dnet_gradfeat_bwd_f16_fwd",
                                *gf_grad = "dnet_gradfeat_bwd_f16_grad", *gf_gather_t = "dnet_gradfeat_bwd_f16_gather_t",
                                *gf_param = "dnet_gradfeat_bwd_f16_param";
    // all four products where there are two operands a side (with one, CROSS changes nothing); two stages of loads in flight over the vertices
    template <int NA, int NB, bool A_TILE, bool B_TILE, bool OVER_VERTS, class Op>
    static int tile(dm_ctx* ctx, const char* name, int B, const Op& op) {
        return hb_launch<NA, NB, A_TILE, B_TILE, true, OVER_VERTS ? 2 : 1>(ctx, name, B, op);
    }
};

// ---------------------------------------------------------------------------------------------------------------- diffuse
struct hdb_spec_op {                                           // g = evecs_h^T fp16(dO), s = mevecs_h^T fp16(x) -> T = evals coef g s 2^-(e1 + e2)
    int N, K, C;
    const int32_t* nv;
    const float* dO; int lddo; const float* x; int ldx;
    const _Float16* eh; int lde; const _Float16* mh; int ldm; const int32_t* e1; const int32_t* e2;
    const float* evals; const float* times;
    float* T;                                                  // [B][K][C]
    __device__ __host__ __forceinline__ int rows() const { return K; }
    __device__ __host__ __forceinline__ int cols() const { return C; }
    __device__ __forceinline__ int depth(int nvb) const { return nvb; }
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ _Float16 a(int w, int b, int nvb, int k, int i) const {
        if (i >= nvb || k >= K) return hb_zero();
        const long long br = (long long)b * N + i;
        return w == 0 ? eh[br * lde + k] : mh[br * ldm + k];
    }
    __device__ __forceinline__ _Float16 b(int w, int b, int nvb, int i, int c) const {
        if (i >= nvb || c >= C) return hb_zero();
        const long long br = (long long)b * N + i;
        return (_Float16)(w == 0 ? dO[br * lddo + c] : x[br * ldx + c]);
    }
    __device__ __forceinline__ void store(int b, int, int k, int c, float g, float s, float, float) const {
        const float ev = evals[(long long)b * K + k];
        // the forward's coefficient: the clamp in fp32, the exponent and exp() in float64, one rounding
        const float coef = (float)exp(-(double)ev * (double)fmaxf(times[c], 1e-8f));
        T[((long long)b * K + k) * C + c] = (float)((double)ev * (double)coef * (double)g * (double)s * ldexp(1.0, -(e1[b] + e2[b])));
    }
};
}  // namespace

extern "C" int dm_dnet_linear_bwd_data_f16(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/,
                                           int ldy, int act, const void* W, int ldw, const int32_t* n_verts /*nullable*/, float* d0 /*nullable*/,
                                           int w0, int ld0, float* d1 /*nullable*/, int w1, int ld1, float* d2 /*nullable*/, int w2, int ld2) {
    if (!ctx) return DM_EINVAL;
    float* d[3] = {d0, d1, d2};
    int w[3] = {w0, w1, w2}, ld[3] = {ld0, ld1, ld2};
    return dnb_linear_bwd_data<_Float16, hb_family>(ctx, __func__, B, N, C_out, n_src, dY, lddy, Y, ldy, act, reinterpret_cast<const _Float16*>(W), ldw,
                                                    n_verts, d, w, ld);
}

extern "C" size_t dm_dnet_linear_bwd_f16_bytes(int B, int C_out, int k_tot) {
    if (B <= 0 || C_out <= 0 || k_tot <= 0) return 0;
    return (size_t)B * C_out * ((size_t)k_tot + 1) * sizeof(float);
}

extern "C" int dm_dnet_linear_bwd_weight_f16(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/,
                                             int ldy, int act, const void* src0, int w0, int ld0, int dtype0, const void* src1, int w1, int ld1,
                                             int dtype1, const void* src2, int w2, int ld2, int dtype2, const int32_t* n_verts /*nullable*/, void* ws,
                                             float* dW /*nullable*/, int lddw, float* db /*nullable*/) {
    if (!ctx) return DM_EINVAL;
    const void* src[3] = {src0, src1, src2};
    int w[3] = {w0, w1, w2}, ld[3] = {ld0, ld1, ld2}, dt[3] = {dtype0, dtype1, dtype2};
    return dnb_linear_bwd_weight<_Float16, hb_family>(ctx, __func__, B, N, C_out, n_src, dY, lddy, Y, ldy, act, src, w, ld, dt, n_verts, ws, dW, lddw,
                                                      db);
}

extern "C" size_t dm_dnet_diffuse_bwd_f16_bytes(int B, int K, int C) {
    if (B <= 0 || K <= 0 || C <= 0) return 0;
    return (size_t)B * K * C * sizeof(float);
}

extern "C" int dm_dnet_diffuse_bwd_f16(dm_ctx* ctx, int B, int N, int K, int C, const float* dO, int lddo, const float* x /*nullable*/, int ldx,
                                       const void* evecs_h, int lde, const void* mevecs_h, int ldm, const int32_t* e1, const int32_t* e2,
                                       const float* evals, const float* times, const int32_t* n_verts /*nullable*/, void* ws, float* dx /*nullable*/,
                                       int lddx, float* dtimes /*nullable*/) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && K > 0 && C > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, K <= HB_KMAX, "K <= 1024, the limit of dm_dnet_diffuse_f16");
    DM_REQUIRE(ctx, dO && evecs_h && mevecs_h && e1 && e2 && evals && times && ws, "null pointer");
    DM_REQUIRE(ctx,
               dm_dnet_al(evecs_h, 2) && dm_dnet_al(mevecs_h, 2) && dm_dnet_al(dO, 4) && dm_dnet_al(x, 4) && dm_dnet_al(times, 4) && dm_dnet_al(ws, 4) &&
                   dm_dnet_al(dx, 4),
               "operands must be aligned to their elements");
    DM_REQUIRE(ctx, lddo >= C && lde >= K && ldm >= K, "lddo >= C, lde >= K, ldm >= K");
    DM_REQUIRE(ctx, !dtimes || (x && ldx >= C), "dtimes needs the saved x, ldx >= C");
    DM_REQUIRE(ctx, !dx || lddx >= C, "lddx >= C");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "dm_dnet_diffuse_bwd_f16", B, N, n_verts)) return rc;
    if (!dx && !dtimes) return DM_OK;
    if (dx) {
        // dx = M Phi (coef * Phi^T dO): the forward with the two matrix operands and their exponents exchanged
        if (int rc = dm_dnet_diffuse_f16(ctx, B, N, K, C, dO, lddo, mevecs_h, ldm, evecs_h, lde, e2, e1, evals, times, DM_F32, n_verts, dx, lddx)) return rc;
    }
    if (dtimes) {
        float* T = (float*)ws;
        hdb_spec_op sp{N, K, C, n_verts, dO, lddo, x, ldx, reinterpret_cast<const _Float16*>(evecs_h), lde, reinterpret_cast<const _Float16*>(mevecs_h),
                       ldm, e1, e2, evals, times, T};
        if (int rc = hb_launch<2, 2, true, true, false, 1>(ctx, "dnet_diffuse_bwd_f16_spec", B, sp)) return rc;
        DM_LAUNCH(ctx, "dnet_diffuse_bwd_f16_times", dnb_times_mesh_kernel, dim3(dm_cdiv(C, 64), B), dim3(64), 0, T, K, C);
        DM_LAUNCH(ctx, "dnet_diffuse_bwd_f16_times", dnb_times_kernel, dim3(dm_cdiv(C, 64)), dim3(64), 0, (const float*)T, B, K, C, dtimes);
    }
    return DM_OK;
}

extern "C" size_t dm_dnet_gradfeat_bwd_f16_bytes(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0) return 0;
    return (6 * (size_t)B * N * C + 2 * (size_t)B * C * C) * sizeof(float);
}

extern "C" int dm_dnet_gradfeat_bwd_f16(dm_ctx* ctx, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx,
                                        const float* gy, int nnz_t, const int32_t* row_len_t, const int32_t* cols_t, const float* gx_t,
                                        const float* gy_t, const float* dO, int lddo, const float* x, int ldx, const void* A_re,
                                        const void* A_im /*nullable*/, int lda, const int32_t* n_verts /*nullable*/, void* ws, float* dx /*nullable*/,
                                        int lddx, float* dA_re /*nullable*/, float* dA_im /*nullable*/, int ldda) {
    if (!ctx) return DM_EINVAL;
    return dnb_gradfeat_bwd<_Float16, hb_family>(ctx, __func__, B, N, C, nnz, row_len, cols, gx, gy, nnz_t, row_len_t, cols_t, gx_t, gy_t, dO, lddo, x,
                                                 ldx, reinterpret_cast<const _Float16*>(A_re), reinterpret_cast<const _Float16*>(A_im), lda, n_verts,
                                                 ws, dx, lddx, dA_re, dA_im, ldda);
}

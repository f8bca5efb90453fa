// DiffusionNet backward pass for mixed-precision training, fp16 operands on the matrix cores: dm_dnet_linear_bwd_data_f16,
// dm_dnet_linear_bwd_weight_f16, dm_dnet_diffuse_bwd_f16, dm_dnet_gradfeat_bwd_f16 -- the gradients of dm_dnet_linear_f16,
// dm_dnet_diffuse_f16, dm_dnet_gradfeat_f16 (dm_dnet_half.hip) with respect to their activations and to the fp32 master parameters
// whose fp16 roundings the forward multiplied; the operators of a mesh are constants.  This file shares no code with dm_dnet_bwd.hip
// (the fp32 family keeps its bits); the gradient of the diffusion with respect to x is a call of dm_dnet_diffuse_f16 itself.
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

#include "dm_internal.h"

typedef float hb_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 hb_f16x8 __attribute__((ext_vector_type(8)));

namespace {
constexpr int HB_T = 64;             // outputs per workgroup side
constexpr int HB_KC = 32;            // contraction depth per stage: two chunks of 16
constexpr int HB_LD = HB_KC + 8;     // LDS row [tile index][k] in halves: 80 bytes, the 16-byte fragment reads stay aligned
constexpr int HB_KMAX = 1024;        // dm_dnet_diffuse_f16's limit: a forward pass beyond it does not exist

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

// out[r, c] = ((part_0 + part_1) + ..)[r, c] over the B meshes in ascending order
__global__ void hb_sum_meshes_kernel(const float* part, int B, int R, int Cc, int ldp, long long mesh_stride, float* out, int ldo) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)R * Cc) return;
    const int rr = (int)(e / Cc), c = (int)(e - (long long)rr * Cc);
    const float* p = part + (long long)rr * ldp + c;
    float s = p[0];
    for (int b = 1; b < B; ++b) s += p[b * mesh_stride];
    out[(long long)rr * ldo + c] = s;
}

int hb_sum_meshes(dm_ctx* ctx, const float* part, int B, int R, int Cc, int ldp, long long mesh_stride, float* out, int ldo) {
    DM_LAUNCH(ctx, "dnet_bwd_f16_sum", hb_sum_meshes_kernel, dim3((unsigned)(((long long)R * Cc + 255) / 256)), dim3(256), 0, part, B, R, Cc, ldp,
              mesh_stride, out, ldo);
    return DM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- linear
struct hlb_common {
    int N, Cout, Ktot;
    const int32_t* nv;
    const float* dY; int lddy; const float* Y; int ldy;       // Y null: no activation
    // fp16(dZ[b,i,o]), dZ = dY * [Y > 0]: applied and rounded while a tile is staged, never stored
    __device__ __forceinline__ _Float16 dz(int b, int nvb, int i, int o) const {
        if (i >= nvb || o >= Cout) return hb_zero();
        const long long br = (long long)b * N + i;
        const float v = dY[br * lddy + o];
        return (Y && !(Y[br * ldy + o] > 0.f)) ? hb_zero() : (_Float16)v;
    }
    // the same from indices clamped into the operand, selected afterwards: all loads of a stage are in flight together
    __device__ __forceinline__ _Float16 dz_clamped(int b, int nvb, int i, int o) const {
        const long long br = (long long)b * N + min(i, nvb - 1);
        const int oc = min(o, Cout - 1);
        const float v = dY[br * lddy + oc];
        const float y = Y ? Y[br * ldy + oc] : 1.f;
        return (i < nvb && o < Cout && y > 0.f) ? (_Float16)v : hb_zero();
    }
};

struct hlb_data_op : hlb_common {
    const _Float16* W; int ldw;
    float* out[3]; int w[3]; int ld[3];
    __device__ __host__ __forceinline__ int rows() const { return N; }
    __device__ __host__ __forceinline__ int cols() const { return Ktot; }
    __device__ __forceinline__ int depth(int) const { return Cout; }
    __device__ __forceinline__ int source(int& k) const {
        int s = 0;
        if (k >= w[0]) { k -= w[0]; s = 1; if (k >= w[1]) { k -= w[1]; s = 2; } }
        return s;
    }
    __device__ __forceinline__ bool skip(int col0) const {       // every column of the tile belongs to a source without an output
        int lo = col0, hi = min(col0 + HB_T, Ktot) - 1;
        const int s0 = source(lo), s1 = source(hi);
        for (int s = s0; s <= s1; ++s)
            if (out[s]) return false;
        return true;
    }
    __device__ __forceinline__ _Float16 a(int, int b, int nvb, int i, int o) const { return dz(b, nvb, i, o); }
    __device__ __forceinline__ _Float16 b(int, int, int, int o, int k) const { return (o < Cout && k < Ktot) ? W[(long long)o * ldw + k] : hb_zero(); }
    __device__ __forceinline__ void store(int b, int nvb, int i, int k, float p1, float, float, float) const {
        const int s = source(k);
        float* o = s == 0 ? out[0] : (s == 1 ? out[1] : out[2]);
        const long long l = s == 0 ? ld[0] : (s == 1 ? ld[1] : ld[2]);
        if (o) o[((long long)b * N + i) * l + k] = i < nvb ? p1 : 0.f;
    }
};

struct hlb_weight_op : hlb_common {
    const void* src[3]; int w[3]; int ld[3]; int f16[3];
    float* part;                                               // [B][Cout][Ktot + 1]: column Ktot is the bias
    __device__ __host__ __forceinline__ int rows() const { return Cout; }
    __device__ __host__ __forceinline__ int cols() const { return Ktot + 1; }
    __device__ __forceinline__ int depth(int nvb) const { return nvb; }
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ _Float16 a(int, int b, int nvb, int o, int i) const { return dz_clamped(b, nvb, i, o); }
    __device__ __forceinline__ _Float16 b(int, int b, int nvb, int i, int k) const {
        const int kc = min(k, Ktot - 1);
        const int s = kc < w[0] ? 0 : (kc < w[0] + w[1] ? 1 : 2);
        const void* sp = s == 0 ? src[0] : (s == 1 ? src[1] : src[2]);
        const long long l = s == 0 ? ld[0] : (s == 1 ? ld[1] : ld[2]);
        const int half = s == 0 ? f16[0] : (s == 1 ? f16[1] : f16[2]);
        const long long e = ((long long)b * N + min(i, nvb - 1)) * l + (kc - (s == 0 ? 0 : (s == 1 ? w[0] : w[0] + w[1])));
        const _Float16 v = half ? reinterpret_cast<const _Float16*>(sp)[e] : (_Float16)reinterpret_cast<const float*>(sp)[e];
        return i < nvb ? (k < Ktot ? v : (k == Ktot ? (_Float16)1.0f : hb_zero())) : hb_zero();     // column Ktot: db[o] = sum_i dZ[i, o] * 1
    }
    __device__ __forceinline__ void store(int b, int, int o, int k, float p1, float, float, float) const {
        part[((long long)b * Cout + o) * (Ktot + 1) + k] = p1;
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

// m_b[c] = the running sum of T[b, k, c] over ascending k from +0, left in T[b, 0, c] (read and written by this thread only)
__global__ void hdb_times_mesh_kernel(float* T, int K, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (c >= C) return;
    float* p = T + (long long)b * K * C + c;
    float m = 0.f;
    for (int k = 0; k < K; ++k) m += p[(long long)k * C];
    p[0] = m;
}

// dtimes[c] = -((m_0 + m_1) + ..)
__global__ void hdb_times_kernel(const float* T, int B, int K, int C, float* dtimes) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float tot = T[c];
    for (int b = 1; b < B; ++b) tot += T[(long long)b * K * C + c];
    dtimes[c] = -tot;
}

// ---------------------------------------------------------------------------------------------------------------- gradient features
struct hgb_ws {                                                // [B][N][C] each, rows behind a mesh's count neither written nor read
    float* gX; float* gY; float* U; float* V; float* dgX; float* dgY;
};

// gX = G_x x, gY = G_y x in fp32: the forward's chain, entries in stored order, one fmaf each
__global__ void hgb_gather_kernel(int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx, const float* gy, const float* x,
                                  int ldx, const int32_t* nv, float* gX, float* gY) {
    const int b = blockIdx.y;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nvb = nv ? nv[b] : N;
    if (e >= (long long)nvb * C) return;
    const int row = (int)(e / C), ch = (int)(e - (long long)row * C);
    const long long br = (long long)b * N + row;
    const int len = min(max(row_len[br], 0), nnz);
    const int32_t* cl = cols + br * nnz;
    const float* vx = gx + br * nnz;
    const float* vy = gy + br * nnz;
    const float* xb = x + (long long)b * N * ldx + ch;
    float sx = 0.f, sy = 0.f;
    for (int q = 0; q < len; ++q) {
        const int c = cl[q];
        if ((unsigned)c >= (unsigned)nvb) continue;
        const float xv = xb[(long long)c * ldx];
        sx = fmaf(vx[q], xv, sx);
        sy = fmaf(vy[q], xv, sy);
    }
    gX[br * C + ch] = sx;
    gY[br * C + ch] = sy;
}

// dx = G_x^T dgX + G_y^T dgY in fp32 as a gather over the rows of the transposed operators: entry q of row j adds gx_t dgX[col], then
// gy_t dgY[col], one fmaf each, q ascending
__global__ void hgb_gather_t_kernel(int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx, const float* gy,
                                    const float* dgX, const float* dgY, const int32_t* nv, float* dx, int lddx) {
    const int b = blockIdx.y;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)N * C) return;
    const int nvb = nv ? nv[b] : N;
    const int row = (int)(e / C), ch = (int)(e - (long long)row * C);
    const long long br = (long long)b * N + row;
    float s = 0.f;
    if (row < nvb) {
        const int len = min(max(row_len[br], 0), nnz);
        const int32_t* cl = cols + br * nnz;
        const float* vx = gx + br * nnz;
        const float* vy = gy + br * nnz;
        for (int q = 0; q < len; ++q) {
            const int c = cl[q];
            if ((unsigned)c >= (unsigned)nvb) continue;
            const long long o = ((long long)b * N + c) * C + ch;
            s = fmaf(vx[q], dgX[o], s);
            s = fmaf(vy[q], dgY[o], s);
        }
    }
    dx[br * lddx + ch] = s;
}

struct hgb_common {
    int N, C;
    const int32_t* nv;
    hgb_ws ws;
    const _Float16* Are; const _Float16* Aim; int lda;        // Aim null: no rotation
    __device__ __host__ __forceinline__ int cols() const { return C; }
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ _Float16 act(const float* p, int b, int nvb, int i, int c) const {        // an fp32 plane of the workspace, rounded
        return (i < nvb && c < C) ? (_Float16)p[((long long)b * N + i) * C + c] : hb_zero();
    }
    __device__ __forceinline__ _Float16 mat(int w, int row, int col) const {                              // A_re (w = 0) or A_im [row][col]
        return (row < C && col < C) ? (w ? Aim : Are)[(long long)row * lda + col] : hb_zero();
    }
};

struct hgb_fwd_op : hgb_common {                               // B_re, B_im, out; p = dO (1 - out^2); U, V; the first terms of dgX, dgY
    const float* dO; int lddo;
    __device__ __host__ __forceinline__ int rows() const { return N; }
    __device__ __forceinline__ int depth(int) const { return C; }
    __device__ __forceinline__ _Float16 a(int w, int b, int nvb, int i, int k) const { return act(w ? ws.gY : ws.gX, b, nvb, i, k); }
    __device__ __forceinline__ _Float16 b(int w, int, int, int k, int c) const { return mat(w, c, k); }
    __device__ __forceinline__ void store(int b, int nvb, int i, int c, float p1, float p2, float p3, float p4) const {
        if (i >= nvb) return;
        const long long br = (long long)b * N + i, o = br * C + c;
        const float sx = ws.gX[o], sy = ws.gY[o];
        // (dm_dnet_gradfeat_f16's epilogue)
        const float bre = Aim ? __fsub_rn(p1, p2) : p1, bim = Aim ? __fadd_rn(p3, p4) : p3;
        const float out = tanhf(fmaf(sx, bre, __fmul_rn(sy, bim)));
        const float p = __fmul_rn(dO[br * lddo + c], fmaf(-out, out, 1.f));
        ws.U[o] = __fmul_rn(p, sx);
        ws.V[o] = __fmul_rn(p, sy);
        ws.dgX[o] = __fmul_rn(p, bre);
        ws.dgY[o] = __fmul_rn(p, bim);
    }
};

struct hgb_grad_op : hgb_common {                              // dgX += U A_re + V A_im, dgY += V A_re - U A_im
    __device__ __host__ __forceinline__ int rows() const { return N; }
    __device__ __forceinline__ int depth(int) const { return C; }
    __device__ __forceinline__ _Float16 a(int w, int b, int nvb, int i, int c) const { return act(w ? ws.V : ws.U, b, nvb, i, c); }
    __device__ __forceinline__ _Float16 b(int w, int, int, int c, int k) const { return mat(w, c, k); }
    __device__ __forceinline__ void store(int b, int nvb, int i, int k, float p1, float p2, float p3, float p4) const {
        if (i >= nvb) return;
        const long long o = ((long long)b * N + i) * C + k;
        const float x0 = __fadd_rn(ws.dgX[o], p1), y0 = Aim ? __fsub_rn(ws.dgY[o], p4) : ws.dgY[o];
        ws.dgX[o] = Aim ? __fadd_rn(x0, p2) : x0;
        ws.dgY[o] = __fadd_rn(y0, p3);
    }
};

struct hgb_param_op : hgb_common {                             // per mesh: dA_re = U^T gX + V^T gY, dA_im = V^T gX - U^T gY
    float* Pre; float* Pim;                                    // [B][C][C]
    __device__ __host__ __forceinline__ int rows() const { return C; }
    __device__ __forceinline__ int depth(int nvb) const { return nvb; }
    __device__ __forceinline__ _Float16 a(int w, int b, int nvb, int c, int i) const { return act(w ? ws.V : ws.U, b, nvb, i, c); }
    __device__ __forceinline__ _Float16 b(int w, int b, int nvb, int i, int k) const { return act(w ? ws.gY : ws.gX, b, nvb, i, k); }
    __device__ __forceinline__ void store(int b, int, int c, int k, float p1, float p2, float p3, float p4) const {
        const long long o = ((long long)b * C + c) * C + k;
        Pre[o] = __fadd_rn(p1, p2);
        if (Aim) Pim[o] = __fsub_rn(p3, p4);
    }
};

// n_verts lives on the device and bounds every load: read it back once and refuse counts outside [1, N]
int hb_check_counts(dm_ctx* ctx, const char* who, int B, int N, const int32_t* n_verts) {
    if (!n_verts) return DM_OK;
    std::vector<int32_t> h((size_t)B);
    DM_CHECK_HIP(ctx, hipMemcpyAsync(h.data(), n_verts, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < B; ++b)
        if (h[b] < 1 || h[b] > N) return dm_fail(ctx, DM_EINVAL, "%s: n_verts[%d] = %d outside [1, %d]", who, b, (int)h[b], N);
    return DM_OK;
}

bool hb_dtype(int d) { return d == DM_F16 || d == DM_F32; }
bool hb_al(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

// the checks that the two linear entries share; fills w / ld of the absent sources with zeros
int hb_lin_check(dm_ctx* ctx, int B, int N, int C_out, int n_src, const void* const* ptr, bool need_all, int* w, int* ld, const float* dY, int lddy,
                 const float* Y, int ldy, int act, long long* ktot) {
    DM_REQUIRE(ctx, B > 0 && N > 0 && C_out > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, n_src >= 1 && n_src <= 3, "one to three sources");
    DM_REQUIRE(ctx, act == 0 || act == 1, "act: 0 none, 1 ReLU");
    *ktot = 0;
    for (int s = 0; s < 3; ++s) {
        if (s >= n_src) { w[s] = 0; ld[s] = 0; continue; }
        DM_REQUIRE(ctx, !need_all || ptr[s] != nullptr, "null source");
        DM_REQUIRE(ctx, w[s] > 0 && ld[s] >= w[s], "a source needs width > 0 and ld >= width");
        *ktot += w[s];
    }
    DM_REQUIRE(ctx, *ktot <= (1 << 24), "summed source width");
    DM_REQUIRE(ctx, dY && lddy >= C_out, "dY, lddy >= C_out");
    DM_REQUIRE(ctx, !act || (Y && ldy >= C_out), "act = 1 needs the saved output Y, ldy >= C_out");
    DM_REQUIRE(ctx, hb_al(dY, 4) && hb_al(Y, 4), "dY and Y must be aligned to their elements");
    return DM_OK;
}
}  // namespace

extern "C" int dm_dnet_linear_bwd_data_f16(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/,
                                           int ldy, int act, const void* W, int ldw, const int32_t* n_verts /*nullable*/, float* d0 /*nullable*/,
                                           int w0, int ld0, float* d1 /*nullable*/, int w1, int ld1, float* d2 /*nullable*/, int w2, int ld2) {
    if (!ctx) return DM_EINVAL;
    const void* ptr[3] = {d0, d1, d2};
    int w[3] = {w0, w1, w2}, ld[3] = {ld0, ld1, ld2};
    long long ktot = 0;
    if (int rc = hb_lin_check(ctx, B, N, C_out, n_src, ptr, false, w, ld, dY, lddy, Y, ldy, act, &ktot)) return rc;
    DM_REQUIRE(ctx, W && ldw >= (int)ktot, "W, ldw >= summed widths");
    DM_REQUIRE(ctx, hb_al(W, 2) && hb_al(d0, 4) && hb_al(d1, 4) && hb_al(d2, 4), "W and the outputs must be aligned to their elements");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = hb_check_counts(ctx, "dm_dnet_linear_bwd_data_f16", B, N, n_verts)) return rc;
    float* out[3] = {d0, n_src > 1 ? d1 : nullptr, n_src > 2 ? d2 : nullptr};
    if (!out[0] && !out[1] && !out[2]) return DM_OK;
    hlb_data_op op{{N, C_out, (int)ktot, n_verts, dY, lddy, act ? Y : nullptr, ldy}, reinterpret_cast<const _Float16*>(W), ldw,
                   {out[0], out[1], out[2]}, {w[0], w[1], w[2]}, {ld[0], ld[1], ld[2]}};
    return hb_launch<1, 1, false, true, false, 1>(ctx, "dnet_linear_bwd_data_f16", B, op);
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
    const void* ptr[3] = {src0, src1, src2};
    int w[3] = {w0, w1, w2}, ld[3] = {ld0, ld1, ld2}, dt[3] = {dtype0, dtype1, dtype2};
    long long ktot = 0;
    if (int rc = hb_lin_check(ctx, B, N, C_out, n_src, ptr, true, w, ld, dY, lddy, Y, ldy, act, &ktot)) return rc;
    for (int s = 0; s < n_src; ++s) {
        DM_REQUIRE(ctx, hb_dtype(dt[s]), "source dtype: DM_F16 or DM_F32");
        DM_REQUIRE(ctx, hb_al(ptr[s], dt[s] == DM_F16 ? 2 : 4), "a source must be aligned to its element");
    }
    DM_REQUIRE(ctx, ws != nullptr, "null workspace");
    DM_REQUIRE(ctx, hb_al(ws, 4) && hb_al(dW, 4) && hb_al(db, 4), "the workspace and the outputs must be aligned to their elements");
    DM_REQUIRE(ctx, !dW || lddw >= (int)ktot, "lddw >= summed widths");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = hb_check_counts(ctx, "dm_dnet_linear_bwd_weight_f16", B, N, n_verts)) return rc;
    if (!dW && !db) return DM_OK;
    const int K = (int)ktot;
    hlb_weight_op op{{N, C_out, K, n_verts, dY, lddy, act ? Y : nullptr, ldy}, {src0, n_src > 1 ? src1 : nullptr, n_src > 2 ? src2 : nullptr},
                     {w[0], w[1], w[2]}, {ld[0], ld[1], ld[2]}, {n_src > 0 && dt[0] == DM_F16, n_src > 1 && dt[1] == DM_F16, n_src > 2 && dt[2] == DM_F16},
                     (float*)ws};
    if (int rc = hb_launch<1, 1, true, true, false, 2>(ctx, "dnet_linear_bwd_weight_f16", B, op)) return rc;
    const long long stride = (long long)C_out * (K + 1);
    if (dW)
        if (int rc = hb_sum_meshes(ctx, (const float*)ws, B, C_out, K, K + 1, stride, dW, lddw)) return rc;
    if (db)
        if (int rc = hb_sum_meshes(ctx, (const float*)ws + K, B, C_out, 1, K + 1, stride, db, 1)) return rc;
    return DM_OK;
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
    DM_REQUIRE(ctx, hb_al(evecs_h, 2) && hb_al(mevecs_h, 2) && hb_al(dO, 4) && hb_al(x, 4) && hb_al(times, 4) && hb_al(ws, 4) && hb_al(dx, 4),
               "operands must be aligned to their elements");
    DM_REQUIRE(ctx, lddo >= C && lde >= K && ldm >= K, "lddo >= C, lde >= K, ldm >= K");
    DM_REQUIRE(ctx, !dtimes || (x && ldx >= C), "dtimes needs the saved x, ldx >= C");
    DM_REQUIRE(ctx, !dx || lddx >= C, "lddx >= C");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = hb_check_counts(ctx, "dm_dnet_diffuse_bwd_f16", B, N, n_verts)) return rc;
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
        DM_LAUNCH(ctx, "dnet_diffuse_bwd_f16_times", hdb_times_mesh_kernel, dim3(dm_cdiv(C, 64), B), dim3(64), 0, T, K, C);
        DM_LAUNCH(ctx, "dnet_diffuse_bwd_f16_times", hdb_times_kernel, dim3(dm_cdiv(C, 64)), dim3(64), 0, (const float*)T, B, K, C, dtimes);
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
    DM_REQUIRE(ctx, B > 0 && N > 0 && C > 0 && nnz > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, row_len && cols && gx && gy && dO && x && A_re && ws, "null pointer");
    DM_REQUIRE(ctx, hb_al(A_re, 2) && hb_al(A_im, 2) && hb_al(dO, 4) && hb_al(x, 4) && hb_al(ws, 4) && hb_al(dx, 4) && hb_al(dA_re, 4) && hb_al(dA_im, 4),
               "operands must be aligned to their elements");
    DM_REQUIRE(ctx, ldx >= C && lddo >= C && lda >= C, "ldx >= C, lddo >= C, lda >= C");
    DM_REQUIRE(ctx, !dx || (nnz_t > 0 && row_len_t && cols_t && gx_t && gy_t && lddx >= C), "dx needs the transposed rows, lddx >= C");
    DM_REQUIRE(ctx, (!dA_re && !dA_im) || ldda >= C, "ldda >= C");
    DM_REQUIRE(ctx, !dA_im || A_im, "dA_im without A_im");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = hb_check_counts(ctx, "dm_dnet_gradfeat_bwd_f16", B, N, n_verts)) return rc;
    if (!dx && !dA_re && !dA_im) return DM_OK;
    const size_t plane = (size_t)B * N * C;
    float* w = (float*)ws;
    hgb_ws g{w, w + plane, w + 2 * plane, w + 3 * plane, w + 4 * plane, w + 5 * plane};
    float* Pre = w + 6 * plane;
    float* Pim = Pre + (size_t)B * C * C;
    const unsigned nblk = (unsigned)(((long long)N * C + 255) / 256);
    DM_LAUNCH(ctx, "dnet_gradfeat_bwd_f16_gather", hgb_gather_kernel, dim3(nblk, B), dim3(256), 0, N, C, nnz, row_len, cols, gx, gy, x, ldx, n_verts, g.gX, g.gY);
    hgb_common cm{N, C, n_verts, g, reinterpret_cast<const _Float16*>(A_re), reinterpret_cast<const _Float16*>(A_im), lda};
    hgb_fwd_op f{cm, dO, lddo};
    if (int rc = A_im ? hb_launch<2, 2, false, false, true, 1>(ctx, "dnet_gradfeat_bwd_f16_fwd", B, f)
                      : hb_launch<2, 1, false, false, true, 1>(ctx, "dnet_gradfeat_bwd_f16_fwd", B, f))
        return rc;
    if (dx) {
        hgb_grad_op gr{cm};
        if (int rc = A_im ? hb_launch<2, 2, false, true, true, 1>(ctx, "dnet_gradfeat_bwd_f16_grad", B, gr)
                          : hb_launch<2, 1, false, true, true, 1>(ctx, "dnet_gradfeat_bwd_f16_grad", B, gr))
            return rc;
        DM_LAUNCH(ctx, "dnet_gradfeat_bwd_f16_gather_t", hgb_gather_t_kernel, dim3(nblk, B), dim3(256), 0, N, C, nnz_t, row_len_t, cols_t, gx_t, gy_t,
                  (const float*)g.dgX, (const float*)g.dgY, n_verts, dx, lddx);
    }
    if (dA_re || dA_im) {
        hgb_param_op pr{cm, Pre, Pim};
        if (int rc = hb_launch<2, 2, true, true, true, 2>(ctx, "dnet_gradfeat_bwd_f16_param", B, pr)) return rc;
        const long long stride = (long long)C * C;
        if (dA_re)
            if (int rc = hb_sum_meshes(ctx, Pre, B, C, C, C, stride, dA_re, ldda)) return rc;
        if (dA_im)
            if (int rc = hb_sum_meshes(ctx, Pim, B, C, C, C, stride, dA_im, ldda)) return rc;
    }
    return DM_OK;
}

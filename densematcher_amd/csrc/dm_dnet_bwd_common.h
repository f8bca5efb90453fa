// What the two DiffusionNet backward families share: dm_dnet_bwd.hip (fp32 operands) and dm_dnet_half_bwd.hip (fp16 operands) include
// this file and add their own tile kernel, their diffusion operands and their dm_dnet_diffuse_bwd_* entry.
//
// T is the element type in which a family stages the operands of a product: float or _Float16.  An fp32 value that becomes an operand
// goes through one static_cast<T>: the identity for float, round to nearest even for _Float16 (a magnitude beyond 65504 becomes
// infinite).  Everything that is not an operand of a product -- the ELL gathers, the epilogues, the sums over the meshes -- is fp32 in
// both families, every operation rounded on its own (fmaf, __fadd_rn, __fsub_rn, __fmul_rn: nothing is contracted).
//
// A family is a type with
//   tile<NA, NB, A_TILE, B_TILE, OVER_VERTS>(ctx, name, B, op)   the launch of its tile kernel for the operand functor `op` (the protocol is
//                                                                written at the kernel); OVER_VERTS: the contraction runs over the vertices
//   sum, lin_data, lin_weight, gf_gather, gf_fwd, gf_grad, gf_gather_t, gf_param      the names its launches are profiled under
// Kernels and functors live in an unnamed namespace: each of the two translation units compiles its own copy.
#pragma once

#include <math.h>

#include <type_traits>

#include "dm_dnet_common.h"

// DM_REQUIRE under the name of the entry point that the caller sees
#define DNB_REQUIRE(ctx, who, cond, msg)                                                                                        \
    do {                                                                                                                        \
        if (!(cond)) return dm_fail(ctx, DM_EINVAL, "%s: requirement failed: %s (%s)", who, #cond, msg);                        \
    } while (0)

namespace {
constexpr int DNB_T = 64;         // outputs per workgroup side of both tile kernels

// out[r, c] = ((part_0 + part_1) + ..)[r, c] over the B meshes in ascending order
__global__ void dnb_sum_meshes_kernel(const float* part, int B, int R, int Cc, int ldp, long long mesh_stride, float* out, int ldo) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)R * Cc) return;
    const int rr = (int)(e / Cc), c = (int)(e - (long long)rr * Cc);
    const float* p = part + (long long)rr * ldp + c;
    float s = p[0];
    for (int b = 1; b < B; ++b) s += p[b * mesh_stride];
    out[(long long)rr * ldo + c] = s;
}

int dnb_sum_meshes(dm_ctx* ctx, const char* name, const float* part, int B, int R, int Cc, int ldp, long long mesh_stride, float* out, int ldo) {
    DM_LAUNCH(ctx, name, dnb_sum_meshes_kernel, dim3((unsigned)(((long long)R * Cc + 255) / 256)), dim3(256), 0, part, B, R, Cc, ldp, mesh_stride,
              out, ldo);
    return DM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- linear
template <class T>
struct dnb_lin_common {
    int N, Cout, Ktot;
    const int32_t* nv;
    const float* dY; int lddy; const float* Y; int ldy;       // Y null: no activation
    // T(dZ[b,i,o]), dZ = dY * [Y > 0]: applied (and rounded) while a tile is staged, never stored
    __device__ __forceinline__ T dz(int b, int nvb, int i, int o) const {
        if (i >= nvb || o >= Cout) return T(0);
        const long long br = (long long)b * N + i;
        const float v = dY[br * lddy + o];
        return (Y && !(Y[br * ldy + o] > 0.f)) ? T(0) : static_cast<T>(v);
    }
    // the same from indices clamped into the operand, selected afterwards: all loads of a stage are in flight together
    __device__ __forceinline__ T dz_clamped(int b, int nvb, int i, int o) const {
        const long long br = (long long)b * N + min(i, nvb - 1);
        const int oc = min(o, Cout - 1);
        const float v = dY[br * lddy + oc];
        const float y = Y ? Y[br * ldy + oc] : 1.f;
        return (i < nvb && o < Cout && y > 0.f) ? static_cast<T>(v) : T(0);
    }
};

template <class T>
struct dnb_lin_data_op : dnb_lin_common<T> {
    using dnb_lin_common<T>::N; using dnb_lin_common<T>::Cout; using dnb_lin_common<T>::Ktot;
    const T* W; int ldw;
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
        int lo = col0, hi = min(col0 + DNB_T, Ktot) - 1;
        const int s0 = source(lo), s1 = source(hi);
        for (int s = s0; s <= s1; ++s)
            if (out[s]) return false;
        return true;
    }
    __device__ __forceinline__ T a(int, int b, int nvb, int i, int o) const { return this->dz(b, nvb, i, o); }
    __device__ __forceinline__ T b(int, int, int, int o, int k) const { return (o < Cout && k < Ktot) ? W[(long long)o * ldw + k] : T(0); }
    __device__ __forceinline__ void store(int b, int nvb, int i, int k, float p1, float, float, float) const {
        const int s = source(k);
        float* o = s == 0 ? out[0] : (s == 1 ? out[1] : out[2]);
        const long long l = s == 0 ? ld[0] : (s == 1 ? ld[1] : ld[2]);
        if (o) o[((long long)b * N + i) * l + k] = i < nvb ? p1 : 0.f;
    }
};

// The sources of the weight gradient.  The fp32 family's are float.  The fp16 family's are float16 or float32, one flag each (an fp32
// element is rounded as it is staged, the value the forward multiplied): only that specialisation has the member and the branch.
template <class T>
struct dnb_lin_sources {
    using elem = float;
    const float* src[3]; int w[3]; int ld[3];
    __device__ __forceinline__ float load(const float* sp, int, long long e) const { return sp[e]; }
};
template <>
struct dnb_lin_sources<_Float16> {
    using elem = void;
    const void* src[3]; int w[3]; int ld[3]; int f16[3];
    __device__ __forceinline__ _Float16 load(const void* sp, int s, long long e) const {
        const int half = s == 0 ? f16[0] : (s == 1 ? f16[1] : f16[2]);
        return half ? reinterpret_cast<const _Float16*>(sp)[e] : (_Float16)reinterpret_cast<const float*>(sp)[e];
    }
};

template <class T>
struct dnb_lin_weight_op : dnb_lin_common<T>, dnb_lin_sources<T> {
    using dnb_lin_common<T>::N; using dnb_lin_common<T>::Cout; using dnb_lin_common<T>::Ktot;
    using dnb_lin_sources<T>::src; using dnb_lin_sources<T>::w; using dnb_lin_sources<T>::ld;
    float* part;                                               // [B][Cout][Ktot + 1]: column Ktot is the bias
    __device__ __host__ __forceinline__ int rows() const { return Cout; }
    __device__ __host__ __forceinline__ int cols() const { return Ktot + 1; }
    __device__ __forceinline__ int depth(int nvb) const { return nvb; }
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ T a(int, int b, int nvb, int o, int i) const { return this->dz_clamped(b, nvb, i, o); }
    __device__ __forceinline__ T b(int, int b, int nvb, int i, int k) const {
        const int kc = min(k, Ktot - 1);
        const int s = kc < w[0] ? 0 : (kc < w[0] + w[1] ? 1 : 2);
        const auto* sp = s == 0 ? src[0] : (s == 1 ? src[1] : src[2]);
        const long long l = s == 0 ? ld[0] : (s == 1 ? ld[1] : ld[2]);
        const T v = this->load(sp, s, ((long long)b * N + min(i, nvb - 1)) * l + (kc - (s == 0 ? 0 : (s == 1 ? w[0] : w[0] + w[1]))));
        return i < nvb ? (k < Ktot ? v : (k == Ktot ? T(1) : T(0))) : T(0);      // column Ktot: db[o] = sum_i dZ[i, o] * 1
    }
    __device__ __forceinline__ void store(int b, int, int o, int k, float p1, float, float, float) const {
        part[((long long)b * Cout + o) * (Ktot + 1) + k] = p1;
    }
};

// the checks that the two linear entries share; fills w / ld of the absent sources with zeros
int dnb_lin_check(dm_ctx* ctx, const char* who, int B, int N, int C_out, int n_src, const void* const* ptr, bool need_all, int* w, int* ld,
                  const float* dY, int lddy, const float* Y, int ldy, int act, long long* ktot) {
    DNB_REQUIRE(ctx, who, B > 0 && N > 0 && C_out > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DNB_REQUIRE(ctx, who, n_src >= 1 && n_src <= 3, "one to three sources");
    DNB_REQUIRE(ctx, who, act == 0 || act == 1, "act: 0 none, 1 ReLU");
    *ktot = 0;
    for (int s = 0; s < 3; ++s) {
        if (s >= n_src) { w[s] = 0; ld[s] = 0; continue; }
        DNB_REQUIRE(ctx, who, !need_all || ptr[s] != nullptr, "null source");
        DNB_REQUIRE(ctx, who, w[s] > 0 && ld[s] >= w[s], "a source needs width > 0 and ld >= width");
        *ktot += w[s];
    }
    DNB_REQUIRE(ctx, who, *ktot <= (1 << 24), "summed source width");
    DNB_REQUIRE(ctx, who, dY && lddy >= C_out, "dY, lddy >= C_out");
    DNB_REQUIRE(ctx, who, !act || (Y && ldy >= C_out), "act = 1 needs the saved output Y, ldy >= C_out");
    DNB_REQUIRE(ctx, who, dm_dnet_al(dY, 4) && dm_dnet_al(Y, 4), "dY and Y must be aligned to their elements");
    return DM_OK;
}

// dm_dnet_linear_bwd_data_*: d[s] nullable, the gradient of source s
template <class T, class Family>
int dnb_linear_bwd_data(dm_ctx* ctx, const char* who, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y, int ldy, int act,
                        const T* W, int ldw, const int32_t* n_verts, float* const* d, int* w, int* ld) {
    const void* ptr[3] = {d[0], d[1], d[2]};
    long long ktot = 0;
    if (int rc = dnb_lin_check(ctx, who, B, N, C_out, n_src, ptr, false, w, ld, dY, lddy, Y, ldy, act, &ktot)) return rc;
    DNB_REQUIRE(ctx, who, W && ldw >= (int)ktot, "W, ldw >= summed widths");
    DNB_REQUIRE(ctx, who, dm_dnet_al(W, sizeof(T)) && dm_dnet_al(d[0], 4) && dm_dnet_al(d[1], 4) && dm_dnet_al(d[2], 4),
                "W and the outputs must be aligned to their elements");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, who, B, N, n_verts)) return rc;
    float* out[3] = {d[0], n_src > 1 ? d[1] : nullptr, n_src > 2 ? d[2] : nullptr};
    if (!out[0] && !out[1] && !out[2]) return DM_OK;
    dnb_lin_data_op<T> op{{N, C_out, (int)ktot, n_verts, dY, lddy, act ? Y : nullptr, ldy}, W, ldw, {out[0], out[1], out[2]}, {w[0], w[1], w[2]},
                          {ld[0], ld[1], ld[2]}};
    return Family::template tile<1, 1, false, true, false>(ctx, Family::lin_data, B, op);
}

// dm_dnet_linear_bwd_weight_*: dt, the dtype of each source, is read by the fp16 family only (the fp32 family passes null)
template <class T, class Family>
int dnb_linear_bwd_weight(dm_ctx* ctx, const char* who, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y, int ldy, int act,
                          const void* const* src, int* w, int* ld, const int* dt, const int32_t* n_verts, void* ws, float* dW, int lddw, float* db) {
    constexpr bool half = std::is_same<T, _Float16>::value;
    long long ktot = 0;
    if (int rc = dnb_lin_check(ctx, who, B, N, C_out, n_src, src, true, w, ld, dY, lddy, Y, ldy, act, &ktot)) return rc;
    for (int s = 0; s < n_src; ++s) {
        if constexpr (half) DNB_REQUIRE(ctx, who, dm_dnet_dtype(dt[s]), "source dtype: DM_F16 or DM_F32");
        DNB_REQUIRE(ctx, who, dm_dnet_al(src[s], half && dt[s] == DM_F16 ? 2 : 4), "a source must be aligned to its element");
    }
    DNB_REQUIRE(ctx, who, ws != nullptr, "null workspace");
    DNB_REQUIRE(ctx, who, dm_dnet_al(ws, 4) && dm_dnet_al(dW, 4) && dm_dnet_al(db, 4), "the workspace and the outputs must be aligned to their elements");
    DNB_REQUIRE(ctx, who, !dW || lddw >= (int)ktot, "lddw >= summed widths");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, who, B, N, n_verts)) return rc;
    if (!dW && !db) return DM_OK;
    const int K = (int)ktot;
    dnb_lin_weight_op<T> op{};
    static_cast<dnb_lin_common<T>&>(op) = {N, C_out, K, n_verts, dY, lddy, act ? Y : nullptr, ldy};
    for (int s = 0; s < 3; ++s) {
        op.src[s] = s < n_src ? static_cast<const typename dnb_lin_sources<T>::elem*>(src[s]) : nullptr;
        op.w[s] = w[s];
        op.ld[s] = ld[s];
        if constexpr (half) op.f16[s] = s < n_src && dt[s] == DM_F16;
    }
    op.part = (float*)ws;
    if (int rc = Family::template tile<1, 1, true, true, true>(ctx, Family::lin_weight, B, op)) return rc;
    const long long stride = (long long)C_out * (K + 1);
    if (dW)
        if (int rc = dnb_sum_meshes(ctx, Family::sum, (const float*)ws, B, C_out, K, K + 1, stride, dW, lddw)) return rc;
    if (db)
        if (int rc = dnb_sum_meshes(ctx, Family::sum, (const float*)ws + K, B, C_out, 1, K + 1, stride, db, 1)) return rc;
    return DM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- diffuse (the times)
// m_b[c] = the running sum of T[b, k, c] over ascending k from +0, left in T[b, 0, c] (read and written by this thread only)
__global__ void dnb_times_mesh_kernel(float* T, int K, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (c >= C) return;
    float* p = T + (long long)b * K * C + c;
    float m = 0.f;
    for (int k = 0; k < K; ++k) m += p[(long long)k * C];
    p[0] = m;
}

// dtimes[c] = -((m_0 + m_1) + ..)
__global__ void dnb_times_kernel(const float* T, int B, int K, int C, float* dtimes) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float tot = T[c];
    for (int b = 1; b < B; ++b) tot += T[(long long)b * K * C + c];
    dtimes[c] = -tot;
}

// ---------------------------------------------------------------------------------------------------------------- gradient features
struct dnb_gf_ws {                                             // [B][N][C] each, rows behind a mesh's count neither written nor read
    float* gX; float* gY; float* U; float* V; float* dgX; float* dgY;
};

// gX = G_x x, gY = G_y x in fp32: the forward's chain (gf_gather of dm_dnet_layers.hip), entries in stored order, one fmaf each
__global__ void dnb_gather_kernel(int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx, const float* gy, const float* x,
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
__global__ void dnb_gather_t_kernel(int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx, const float* gy,
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

template <class T>
struct dnb_gf_common {
    int N, C;
    const int32_t* nv;
    dnb_gf_ws ws;
    const T* Are; const T* Aim; int lda;                       // Aim null: no rotation
    __device__ __host__ __forceinline__ int cols() const { return C; }
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ T act(const float* p, int b, int nvb, int i, int c) const {               // an fp32 plane of the workspace
        return (i < nvb && c < C) ? static_cast<T>(p[((long long)b * N + i) * C + c]) : T(0);
    }
    __device__ __forceinline__ T mat(int w, int row, int col) const {                                     // A_re (w = 0) or A_im [row][col]
        return (row < C && col < C) ? (w ? Aim : Are)[(long long)row * lda + col] : T(0);
    }
};

template <class T>
struct dnb_gf_fwd_op : dnb_gf_common<T> {                      // B_re, B_im, out; p = dO (1 - out^2); U, V; the first terms of dgX, dgY
    using dnb_gf_common<T>::N; using dnb_gf_common<T>::C; using dnb_gf_common<T>::ws; using dnb_gf_common<T>::Aim;
    const float* dO; int lddo;
    __device__ __host__ __forceinline__ int rows() const { return N; }
    __device__ __forceinline__ int depth(int) const { return C; }
    __device__ __forceinline__ T a(int w, int b, int nvb, int i, int k) const { return this->act(w ? ws.gY : ws.gX, b, nvb, i, k); }
    __device__ __forceinline__ T b(int w, int, int, int k, int c) const { return this->mat(w, c, k); }
    __device__ __forceinline__ void store(int b, int nvb, int i, int c, float p1, float p2, float p3, float p4) const {
        if (i >= nvb) return;
        const long long br = (long long)b * N + i, o = br * C + c;
        const float sx = ws.gX[o], sy = ws.gY[o];
        // (the forward's epilogue)
        const float bre = Aim ? __fsub_rn(p1, p2) : p1, bim = Aim ? __fadd_rn(p3, p4) : p3;
        const float out = tanhf(fmaf(sx, bre, __fmul_rn(sy, bim)));
        const float p = __fmul_rn(dO[br * lddo + c], fmaf(-out, out, 1.f));
        ws.U[o] = __fmul_rn(p, sx);
        ws.V[o] = __fmul_rn(p, sy);
        ws.dgX[o] = __fmul_rn(p, bre);
        ws.dgY[o] = __fmul_rn(p, bim);
    }
};

template <class T>
struct dnb_gf_grad_op : dnb_gf_common<T> {                     // dgX += U A_re + V A_im, dgY += V A_re - U A_im
    using dnb_gf_common<T>::N; using dnb_gf_common<T>::C; using dnb_gf_common<T>::ws; using dnb_gf_common<T>::Aim;
    __device__ __host__ __forceinline__ int rows() const { return N; }
    __device__ __forceinline__ int depth(int) const { return C; }
    __device__ __forceinline__ T a(int w, int b, int nvb, int i, int c) const { return this->act(w ? ws.V : ws.U, b, nvb, i, c); }
    __device__ __forceinline__ T b(int w, int, int, int c, int k) const { return this->mat(w, c, k); }
    __device__ __forceinline__ void store(int b, int nvb, int i, int k, float p1, float p2, float p3, float p4) const {
        if (i >= nvb) return;
        const long long o = ((long long)b * N + i) * C + k;
        const float x0 = __fadd_rn(ws.dgX[o], p1), y0 = Aim ? __fsub_rn(ws.dgY[o], p4) : ws.dgY[o];
        ws.dgX[o] = Aim ? __fadd_rn(x0, p2) : x0;
        ws.dgY[o] = __fadd_rn(y0, p3);
    }
};

template <class T>
struct dnb_gf_param_op : dnb_gf_common<T> {                    // per mesh: dA_re = U^T gX + V^T gY, dA_im = V^T gX - U^T gY
    using dnb_gf_common<T>::C; using dnb_gf_common<T>::ws; using dnb_gf_common<T>::Aim;
    float* Pre; float* Pim;                                    // [B][C][C]
    __device__ __host__ __forceinline__ int rows() const { return C; }
    __device__ __forceinline__ int depth(int nvb) const { return nvb; }
    __device__ __forceinline__ T a(int w, int b, int nvb, int c, int i) const { return this->act(w ? ws.V : ws.U, b, nvb, i, c); }
    __device__ __forceinline__ T b(int w, int b, int nvb, int i, int k) const { return this->act(w ? ws.gY : ws.gX, b, nvb, i, k); }
    __device__ __forceinline__ void store(int b, int, int c, int k, float p1, float p2, float p3, float p4) const {
        const long long o = ((long long)b * C + c) * C + k;
        Pre[o] = __fadd_rn(p1, p2);
        if (Aim) Pim[o] = __fsub_rn(p3, p4);
    }
};

// dm_dnet_gradfeat_bwd_*
template <class T, class Family>
int dnb_gradfeat_bwd(dm_ctx* ctx, const char* who, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx,
                     const float* gy, int nnz_t, const int32_t* row_len_t, const int32_t* cols_t, const float* gx_t, const float* gy_t, const float* dO,
                     int lddo, const float* x, int ldx, const T* A_re, const T* A_im, int lda, const int32_t* n_verts, void* ws, float* dx, int lddx,
                     float* dA_re, float* dA_im, int ldda) {
    DNB_REQUIRE(ctx, who, B > 0 && N > 0 && C > 0 && nnz > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DNB_REQUIRE(ctx, who, row_len && cols && gx && gy && dO && x && A_re && ws, "null pointer");
    DNB_REQUIRE(ctx, who,
                dm_dnet_al(A_re, sizeof(T)) && dm_dnet_al(A_im, sizeof(T)) && dm_dnet_al(dO, 4) && dm_dnet_al(x, 4) && dm_dnet_al(ws, 4) &&
                    dm_dnet_al(dx, 4) && dm_dnet_al(dA_re, 4) && dm_dnet_al(dA_im, 4),
                "operands must be aligned to their elements");
    DNB_REQUIRE(ctx, who, ldx >= C && lddo >= C && lda >= C, "ldx >= C, lddo >= C, lda >= C");
    DNB_REQUIRE(ctx, who, !dx || (nnz_t > 0 && row_len_t && cols_t && gx_t && gy_t && lddx >= C), "dx needs the transposed rows, lddx >= C");
    DNB_REQUIRE(ctx, who, (!dA_re && !dA_im) || ldda >= C, "ldda >= C");
    DNB_REQUIRE(ctx, who, !dA_im || A_im, "dA_im without A_im");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, who, B, N, n_verts)) return rc;
    if (!dx && !dA_re && !dA_im) return DM_OK;
    const size_t plane = (size_t)B * N * C;
    float* w = (float*)ws;
    dnb_gf_ws g{w, w + plane, w + 2 * plane, w + 3 * plane, w + 4 * plane, w + 5 * plane};
    float* Pre = w + 6 * plane;
    float* Pim = Pre + (size_t)B * C * C;
    const unsigned nblk = (unsigned)(((long long)N * C + 255) / 256);
    DM_LAUNCH(ctx, Family::gf_gather, dnb_gather_kernel, dim3(nblk, B), dim3(256), 0, N, C, nnz, row_len, cols, gx, gy, x, ldx, n_verts, g.gX, g.gY);
    dnb_gf_common<T> cm{N, C, n_verts, g, A_re, A_im, lda};
    dnb_gf_fwd_op<T> f{cm, dO, lddo};
    if (int rc = A_im ? Family::template tile<2, 2, false, false, false>(ctx, Family::gf_fwd, B, f)
                      : Family::template tile<2, 1, false, false, false>(ctx, Family::gf_fwd, B, f))
        return rc;
    if (dx) {
        dnb_gf_grad_op<T> gr{cm};
        if (int rc = A_im ? Family::template tile<2, 2, false, true, false>(ctx, Family::gf_grad, B, gr)
                          : Family::template tile<2, 1, false, true, false>(ctx, Family::gf_grad, B, gr))
            return rc;
        DM_LAUNCH(ctx, Family::gf_gather_t, dnb_gather_t_kernel, dim3(nblk, B), dim3(256), 0, N, C, nnz_t, row_len_t, cols_t, gx_t, gy_t,
                  (const float*)g.dgX, (const float*)g.dgY, n_verts, dx, lddx);
    }
    if (dA_re || dA_im) {
        dnb_gf_param_op<T> pr{cm, Pre, Pim};
        if (int rc = Family::template tile<2, 2, true, true, true>(ctx, Family::gf_param, B, pr)) return rc;
        const long long stride = (long long)C * C;
        if (dA_re)
            if (int rc = dnb_sum_meshes(ctx, Family::sum, Pre, B, C, C, C, stride, dA_re, ldda)) return rc;
        if (dA_im)
            if (int rc = dnb_sum_meshes(ctx, Family::sum, Pim, B, C, C, C, stride, dA_im, ldda)) return rc;
    }
    return DM_OK;
}
}  // namespace

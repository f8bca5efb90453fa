// Farthest-point sampling of B meshes on the device (pyFM/mesh/geometry.py:813-851 behind TriMesh.extract_fps).
//
//   out[0] = start, dists = d(start);  size - 1 times:  new = argmax(dists), dists = min(dists, d(new))
//
// The arg-max is np.argmax: the LOWEST index among equal maxima, so the key of every reduction is (value, lowest index) -- a
// total order, hence the result does not depend on how the reduction is arranged.  One workgroup of 1024 threads per mesh runs
// the whole loop: vertex i = thread + 1024 j lives in register j of its thread (N <= 16384), the arg-max goes through the wave
// by DPP (quad_perm, row_half_mirror, row_mirror, then two lane exchanges across the rows) and across the 16 waves through one
// LDS slot per wave, double-buffered by the parity of the step: one barrier per sample, no host synchronisation, no atomics.
// A padded vertex (>= n_verts[b]) carries the distance -1 for ever: below every real distance, so it is never chosen; once all
// real distances are 0 the arg-max is vertex 0, like the reference's (size > n_verts repeats indices).
//
//   dm_fps_euclid   d(i) = np.linalg.norm(V - V[i], axis=1): sqrt((dx dx + dy dy) + dz dz), every operation rounded on its own
//                   (no fused multiply-add: contraction is off in fps_dist3) and a correctly rounded square root.
//   fps_rows        d(i) = row i of a (B, N, N) distance array (the all-pairs heat-method rows, route (a) of dm_fps_heat)
//   fps_step        one step on distances kept in global memory (route (b) of dm_fps_heat: a single-source solve per sample
//                   writes d(new), this kernel folds it in and writes the next source where the next solve reads it)
#include <math.h>

#include "dm_device.h"
#include "dm_fps_dev.h"
#include "dm_internal.h"

namespace {

constexpr int FPS_T = 1024;            // threads per mesh
constexpr int FPS_MAXN = 16384;

__device__ __forceinline__ double fps_dist3(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double s = (xx + yy) + zz;
    return __dsqrt_rn(s);
}

// VPT vertices per thread; their coordinates stay in registers up to VPT = 4, beyond that they are re-read every step (L2)
template <int VPT>
__global__ __launch_bounds__(FPS_T) void fps_euclid_kernel(int N, const double* __restrict__ verts, const int32_t* __restrict__ n_verts, int size,
                                                          const int32_t* __restrict__ start, int32_t* __restrict__ out) {
    __shared__ double sv[32];
    __shared__ int si[32];
    constexpr bool KEEP = VPT <= 4;
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = n_verts ? min(max(n_verts[b], 1), N) : N;
    const double* V = verts + (size_t)b * N * 3;
    double px[KEEP ? VPT : 1], py[KEEP ? VPT : 1], pz[KEEP ? VPT : 1], d[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const int i = t + FPS_T * j;
        d[j] = i < n ? DM_INF_F64 : -1.0;
        if (KEEP) {
            const int ic = min(i, n - 1);
            px[j] = V[3 * ic]; py[j] = V[3 * ic + 1]; pz[j] = V[3 * ic + 2];
        }
    }
    int cur = min(max(start[b], 0), n - 1);
    int32_t* o = out + (size_t)b * size;
    for (int s = 0; s < size; ++s) {
        if (t == 0) o[s] = cur;
        if (s + 1 == size) break;
        const double cx = V[3 * cur], cy = V[3 * cur + 1], cz = V[3 * cur + 2];
        double bv = -2.0;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int i = t + FPS_T * j;
            double x, y, z;
            if (KEEP) { x = px[j]; y = py[j]; z = pz[j]; }
            else { const int ic = min(i, n - 1); x = V[3 * ic]; y = V[3 * ic + 1]; z = V[3 * ic + 2]; }
            const double e = fps_dist3(x, y, z, cx, cy, cz);
            d[j] = (i < n && e < d[j]) ? e : d[j];                 // np.minimum; a padded vertex keeps -1
            if (d[j] > bv) { bv = d[j]; bi = i; }                  // ascending i: the first maximum stays
        }
        cur = fps_block_argmax(bv, bi, sv, si, s & 1);
        cur = min(max(cur, 0), n - 1);                             // (coordinates that are not numbers leave no maximum: stay inside the mesh)
    }
}

// the same loop on the rows of a distance array: d(i) = D[b][i][:] (row stride ldd); info |= 2 where a distance read is not finite
template <int VPT>
__global__ __launch_bounds__(FPS_T) void fps_rows_kernel(int N, const double* __restrict__ D, long long strideD, int ldd,
                                                        const int32_t* __restrict__ nv4, int size, const int32_t* __restrict__ start,
                                                        int32_t* __restrict__ out, int32_t* __restrict__ info) {
    __shared__ double sv[32];
    __shared__ int si[32];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = min(max(nv4[4 * b], 1), N);
    const double* Db = D + (size_t)b * strideD;
    double d[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) d[j] = (t + FPS_T * j) < n ? DM_INF_F64 : -1.0;
    const int s0 = start[b];
    if (t == 0 && (s0 < 0 || s0 >= n)) atomicOr(info + b, 1);
    int cur = min(max(s0, 0), n - 1);
    bool bad = false;
    int32_t* o = out + (size_t)b * size;
    for (int s = 0; s < size; ++s) {
        if (t == 0) o[s] = cur;
        if (s + 1 == size) break;
        const double* row = Db + (size_t)cur * ldd;
        double bv = -2.0;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int i = t + FPS_T * j;
            if (i < n) {
                const double e = row[i];
                bad = bad || !(fabs(e) <= 1.79769313486231570815e308);
                d[j] = e < d[j] ? e : d[j];
            }
            if (d[j] > bv) { bv = d[j]; bi = i; }
        }
        cur = fps_block_argmax(bv, bi, sv, si, s & 1);
        cur = min(max(cur, 0), n - 1);                             // (a row of NaNs leaves no maximum: stay inside the mesh)
    }
    if (bad) atomicOr(info + b, 2);
}

// route (b), before the first solve: dists = +inf (-1 for padding), out[:, 0] = cur = start
__global__ __launch_bounds__(256) void fps_step_init_kernel(int N, const int32_t* __restrict__ nv4, int size, const int32_t* __restrict__ start,
                                                           double* __restrict__ dists, int32_t* __restrict__ cur, int32_t* __restrict__ out,
                                                           int32_t* __restrict__ info) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(max(nv4[4 * b], 1), N);
    if (i < N) dists[(size_t)b * N + i] = i < n ? DM_INF_F64 : -1.0;
    if (i == 0) {
        const int s0 = start[b];
        if (s0 < 0 || s0 >= n) atomicOr(info + b, 1);
        const int c = min(max(s0, 0), n - 1);
        cur[b] = c;
        out[(size_t)b * size] = c;
    }
}
// route (b), after the solve of step s: dists = min(dists, drow), out[:, s + 1] = cur = argmax(dists)
__global__ __launch_bounds__(FPS_T) void fps_step_kernel(int N, const double* __restrict__ drow, const int32_t* __restrict__ nv4, int size, int s,
                                                        double* __restrict__ dists, int32_t* __restrict__ cur, int32_t* __restrict__ out,
                                                        int32_t* __restrict__ info) {
    __shared__ double sv[32];
    __shared__ int si[32];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = min(max(nv4[4 * b], 1), N);
    const double* row = drow + (size_t)b * N;
    double* d = dists + (size_t)b * N;
    double bv = -2.0;
    int bi = 0x7fffffff;
    bool bad = false;
    for (int i = t; i < N; i += FPS_T) {
        double x = d[i];
        if (i < n) {
            const double e = row[i];
            bad = bad || !(fabs(e) <= 1.79769313486231570815e308);
            x = e < x ? e : x;
            d[i] = x;
        }
        if (x > bv) { bv = x; bi = i; }
    }
    int c = fps_block_argmax(bv, bi, sv, si, 0);
    c = min(max(c, 0), n - 1);
    if (t == 0) { cur[b] = c; out[(size_t)b * size + s + 1] = c; }
    if (bad) atomicOr(info + b, 2);
}

}  // namespace

#define FPS_BY_VPT(N_, CALL)                                   \
    do {                                                       \
        const int vpt_ = dm_cdiv(N_, FPS_T);                   \
        if (vpt_ <= 1) { CALL(1); }                            \
        else if (vpt_ <= 2) { CALL(2); }                       \
        else if (vpt_ <= 4) { CALL(4); }                       \
        else if (vpt_ <= 8) { CALL(8); }                       \
        else { CALL(16); }                                     \
    } while (0)

int dm_fps_rows(dm_ctx* ctx, int B, int N, const double* D, long long strideD, int ldd, const int32_t* nv4, int size, const int32_t* start,
                int32_t* out, int32_t* info) {
#define FPS_CALL(V_) DM_LAUNCH(ctx, "fps_rows", fps_rows_kernel<V_>, dim3(B), dim3(FPS_T), 0, N, D, strideD, ldd, nv4, size, start, out, info)
    FPS_BY_VPT(N, FPS_CALL);
#undef FPS_CALL
    return DM_OK;
}
int dm_fps_step_init(dm_ctx* ctx, int B, int N, const int32_t* nv4, int size, const int32_t* start, double* dists, int32_t* cur, int32_t* out,
                     int32_t* info) {
    DM_LAUNCH(ctx, "fps_step_init", fps_step_init_kernel, dim3(dm_cdiv(N, 256), B), dim3(256), 0, N, nv4, size, start, dists, cur, out, info);
    return DM_OK;
}
int dm_fps_step(dm_ctx* ctx, int B, int N, const double* drow, const int32_t* nv4, int size, int s, double* dists, int32_t* cur, int32_t* out,
                int32_t* info) {
    DM_LAUNCH(ctx, "fps_step", fps_step_kernel, dim3(B), dim3(FPS_T), 0, N, drow, nv4, size, s, dists, cur, out, info);
    return DM_OK;
}

extern "C" int dm_fps_euclid(dm_ctx* ctx, int B, int N, const double* verts, const int32_t* n_verts, int size, const int32_t* start,
                             int32_t* out) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && size > 0, "sizes must be positive");
    DM_REQUIRE(ctx, N <= FPS_MAXN, "N <= 16384 (the running minimum of a mesh lives in the registers of one workgroup)");
    DM_REQUIRE(ctx, verts && start && out, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
#define FPS_CALL(V_) DM_LAUNCH(ctx, "fps_euclid", fps_euclid_kernel<V_>, dim3(B), dim3(FPS_T), 0, N, verts, n_verts, size, start, out)
    FPS_BY_VPT(N, FPS_CALL);
#undef FPS_CALL
    return DM_OK;
}

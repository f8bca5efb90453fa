// Per-vertex corner lists of a padded batch of triangle meshes, shared by the translation units that assemble per-vertex rows
// (dm_laplacian.hip: cotangent stiffness rows; dm_dnet.hip: the DiffusionNet operators): count the corners of every vertex, scan,
// scatter.  The lists leave unordered; the row kernels sort each vertex's few corners, so that a vertex's contributions are summed
// in a fixed order.  Also lap_pad_kernel: the decoupled rows of padding vertices in the scaled ELL operand of dm_eigenbasis.
#pragma once
#include "dm_internal.h"

constexpr int LAP_MAXROW = 64;        // entries a vertex's row may hold (its neighbours + the diagonal); more: DM_EINVAL

struct lap_args {
    int B, N, nt;                     // meshes, vertices per mesh, triangles per mesh
    const int32_t* tri;               // (B, nt, 3)
    const double* len;                // (B, nt, 3) intrinsic side lengths, or null: from verts
    const double* verts;              // (B, N, 3)
    double scale;                     // 1, or 1/2 for a double cover
    const int32_t* nv;                // (B) vertices of each mesh (<= N), or null: N.  Meshes of fewer vertices / triangles ride along padded:
                                      // triangles (-1, -1, -1) are skipped, vertices >= nv[b] become decoupled rows (below)
};
__device__ __forceinline__ int lap_nv(const lap_args& a, int b) { return a.nv ? a.nv[b] : a.N; }

// count[b][v] = corners of vertex v
static __global__ __launch_bounds__(256) void lap_count_kernel(lap_args a, int32_t* __restrict__ count, int32_t* __restrict__ bad) {
    const int b = blockIdx.y;
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * a.nt) return;
    const int v = a.tri[(long long)b * 3 * a.nt + h];
    if (v < 0) return;                                       // padding triangle
    if (v >= lap_nv(a, b)) { atomicOr(bad, 1); return; }
    atomicAdd(count + (long long)b * a.N + v, 1);
}
// exclusive prefix sums of a mesh's counts (one workgroup per mesh); cursor = offsets
static __global__ __launch_bounds__(1024) void lap_scan_kernel(int N, const int32_t* __restrict__ count, int32_t* __restrict__ offset, int32_t* __restrict__ cursor) {
    __shared__ int part[1024];
    const int b = blockIdx.x, t = threadIdx.x;
    const int per = (N + 1023) / 1024, i0 = t * per, i1 = min(N, i0 + per);
    int s = 0;
    for (int i = i0; i < i1; ++i) s += count[(long long)b * N + i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = i0; i < i1; ++i) {
        offset[(long long)b * (N + 1) + i] = run; cursor[(long long)b * N + i] = run;
        run += count[(long long)b * N + i];
    }
    if (t == 1023) offset[(long long)b * (N + 1) + N] = part[1023];
}
// corner lists (unordered: the row kernel sorts each vertex's few corners)
static __global__ __launch_bounds__(256) void lap_scatter_kernel(lap_args a, int32_t* __restrict__ cursor, int32_t* __restrict__ list) {
    const int b = blockIdx.y;
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= 3 * a.nt) return;
    const int v = a.tri[(long long)b * 3 * a.nt + h];
    if (v < 0 || v >= lap_nv(a, b)) return;
    const int pos = atomicAdd(cursor + (long long)b * a.N + v, 1);
    list[(long long)b * 3 * a.nt + pos] = h;
}

// Padding vertices (v >= nv[b]) get the single entry L_vv = the Gershgorin bound max_i sum_q |L_iq| of their mesh's own operator: an
// eigenvalue at the upper end of the interval the eigensolver's filter damps, never inside the wanted part of the spectrum.
static __global__ __launch_bounds__(256) void lap_pad_kernel(int N, int nnz, const int32_t* __restrict__ nv, double* __restrict__ ell_vals) {
    __shared__ double sh[256];
    const int b = blockIdx.x, t = threadIdx.x, nb = nv[b];
    if (nb >= N) return;
    double mx = 0.0;
    for (int i = t; i < nb; i += 256) {
        const double* vr = ell_vals + ((long long)b * N + i) * nnz;
        double s = 0.0;
        for (int q = 0; q < nnz; ++q) s += fabs(vr[q]);
        mx = fmax(mx, s);
    }
    sh[t] = mx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if (t < off) sh[t] = fmax(sh[t], sh[t + off]); __syncthreads(); }
    const double g = sh[0];
    for (int i = nb + t; i < N; i += 256) ell_vals[((long long)b * N + i) * nnz] = g;
}

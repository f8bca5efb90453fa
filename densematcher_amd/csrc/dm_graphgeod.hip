// Shortest paths along the edges of B meshes on the device: what scipy.sparse.csgraph.dijkstra returns, bit for bit
// (pyFM/mesh/geometry.py:524-556 geodesic_distmat_dijkstra behind TriMesh.get_geodesic(dijkstra=True), and the distance of the default
// TriMesh.extract_fps of this package).
//
// Why a relaxation gives Dijkstra's bits ("Edge-graph shortest paths").  Dijkstra returns
//   d[v] = min over the paths s -> v of the LEFT-FOLDED float64 sum of the edge weights:
// float addition is monotone (a <= b => fl(a + w) <= fl(b + w)) and, for w >= 0, inflationary (fl(a + w) >= a), so a settled value is
// final.  Every value a relaxation holds is the fold of some path, hence never below that minimum; when no edge can lower anything
// (d[v] <= fl(d[u] + w(u, v)) on every edge), induction along any path puts every value at or below that path's fold.  So ANY order of
// relaxations -- stale reads, any grouping of vertices, threads or sources -- started from d[s] = 0, +inf elsewhere and run until a whole
// sweep changes nothing ends at the same bits.  The same holds for a warm start from the running minimum m of farthest-point sampling:
// every m[u] is the fold of a path from an earlier sample, what spreads from it is the fold of a longer path from that sample, hence
// >= m[v]; setting m[new] = 0 and relaxing gives exactly min(m, d_new).
//
// The scheme (pull style, no read-modify-write anywhere): the distances of one source (or the running minimum of one mesh) live in LDS, 8 N
// bytes; a thread owns the vertices v = t + T j, reads its neighbours' values and writes only its own, IN PLACE (a neighbour's value may
// be this sweep's or the last one's: both are folds of paths); one __syncthreads_or per sweep, and the loop ends after the first sweep
// that wrote nothing -- during that sweep every thread read the final state.  The 8-byte LDS accesses are relaxed atomic loads / stores
// (ds_read_b64 / ds_write_b64: never torn).  The adjacency is ELL in vertex-minor layout (B, nnz, N): lane v reads consecutive words; it
// is re-read from global memory (L2) every sweep.  Weights that are negative or NaN and columns outside the mesh are skipped (the loop
// then still ends: values only fall, inside a finite set) and reported in info.
#include <math.h>

#include "dm_device.h"
#include "dm_fps_dev.h"
#include "dm_internal.h"

namespace {

constexpr int GG_MAXN = 16384;
constexpr int GG_FPS_T = 1024;         // threads of the sampler: one workgroup per mesh

__device__ __forceinline__ double gg_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void gg_st(double* p, double x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// relax m (LDS, n entries) until a sweep changes nothing.  All threads of the workgroup call it, after a barrier that made m visible;
// it returns behind a barrier.  At most n sweeps can change something (after sweep k every vertex is at or below the fold of its best
// path of k edges); the bound only guards the loop.
template <int T>
__device__ __forceinline__ void gg_relax(double* m, int n, int N, int nnz, const int32_t* __restrict__ cols, const double* __restrict__ w) {
    const int t = threadIdx.x;
    for (int sweep = 0; sweep <= n; ++sweep) {
        int changed = 0;
        for (int v = t; v < n; v += T) {
            const double old = gg_ld(m + v);
            double best = old;
            const int32_t* cv = cols + v;
            const double* wv = w + v;
#pragma unroll 4
            for (int e = 0; e < nnz; ++e) {
                const int c = cv[(size_t)e * N];
                const double wt = wv[(size_t)e * N];
                if ((unsigned)c < (unsigned)n && wt >= 0.0) {
                    const double cand = gg_ld(m + c) + wt;
                    best = cand < best ? cand : best;
                }
            }
            if (best < old) { gg_st(m + v, best); changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }
}

// info bits of the adjacency of one mesh: 2 = a weight of an edge that is negative or NaN, 4 = a column outside [-1, n)
template <int T>
__device__ __forceinline__ int gg_check(int n, int N, int nnz, const int32_t* __restrict__ cols, const double* __restrict__ w) {
    int flags = 0;
    for (int e = 0; e < nnz; ++e)
        for (int v = threadIdx.x; v < n; v += T) {
            const int c = cols[(size_t)e * N + v];
            if (c < -1 || c >= n) flags |= 4;
            else if (c >= 0 && !(w[(size_t)e * N + v] >= 0.0)) flags |= 2;
        }
    return flags;
}

// one workgroup per (source, mesh): D[b][s][:] = the distances from sources[b][s]
template <int T>
__global__ __launch_bounds__(T) void graph_geodesic_kernel(int N, int nnz, const int32_t* __restrict__ cols, const double* __restrict__ w,
                                                          const int32_t* __restrict__ n_verts, int ns, const int32_t* __restrict__ sources,
                                                          double* __restrict__ D, int32_t* __restrict__ info) {
    extern __shared__ double gg_m[];
    const int b = blockIdx.y, s = blockIdx.x, t = threadIdx.x;
    const int n = n_verts ? min(max(n_verts[b], 1), N) : N;
    cols += (size_t)b * nnz * N;
    w += (size_t)b * nnz * N;
    double* row = D + ((size_t)b * ns + s) * N;
    const int src = sources[(size_t)b * ns + s];
    if (s == 0) {                                                        // the adjacency is checked once per mesh
        const int flags = gg_check<T>(n, N, nnz, cols, w);
        if (flags) atomicOr(info + b, flags);
    }
    if (src < 0 || src >= n) {                                           // no source: a row of zeros
        if (t == 0 && src != -1) atomicOr(info + b, 1);
        for (int v = t; v < N; v += T) row[v] = 0.0;
        return;
    }
    for (int v = t; v < n; v += T) gg_m[v] = v == src ? 0.0 : DM_INF_F64;
    __syncthreads();
    gg_relax<T>(gg_m, n, N, nnz, cols, w);
    for (int v = t; v < N; v += T) row[v] = v < n ? gg_m[v] : 0.0;
}

// one workgroup per mesh runs the whole sampling loop: the running minimum m stays in LDS, every sample is an arg-max, m[new] = 0 and a
// warm-started relaxation (which only moves the values of the new sample's Voronoi region)
__global__ __launch_bounds__(GG_FPS_T) void fps_graph_kernel(int N, int nnz, const int32_t* __restrict__ cols, const double* __restrict__ w,
                                                            const int32_t* __restrict__ n_verts, int size, const int32_t* __restrict__ start,
                                                            int32_t* __restrict__ out, int32_t* __restrict__ info) {
    extern __shared__ double gg_m[];
    __shared__ double sv[32];
    __shared__ int si[32];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = n_verts ? min(max(n_verts[b], 1), N) : N;
    cols += (size_t)b * nnz * N;
    w += (size_t)b * nnz * N;
    int flags = gg_check<GG_FPS_T>(n, N, nnz, cols, w);
    const int s0 = start[b];
    if (t == 0 && (s0 < 0 || s0 >= n)) flags |= 1;
    if (flags) atomicOr(info + b, flags);
    int cur = min(max(s0, 0), n - 1);
    for (int v = t; v < n; v += GG_FPS_T) gg_m[v] = DM_INF_F64;
    int32_t* o = out + (size_t)b * size;
    __syncthreads();
    for (int s = 0; s < size; ++s) {
        if (t == 0) o[s] = cur;
        if (s + 1 == size) break;
        if (t == 0) gg_m[cur] = 0.0;                                     // (every read of m by the last arg-max lies before its barrier)
        __syncthreads();
        gg_relax<GG_FPS_T>(gg_m, n, N, nnz, cols, w);
        double bv = -2.0;
        int bi = 0x7fffffff;
        for (int v = t; v < n; v += GG_FPS_T) {                          // ascending v: the first maximum stays; +inf is a maximum
            const double x = gg_m[v];
            if (x > bv) { bv = x; bi = v; }
        }
        cur = fps_block_argmax(bv, bi, sv, si, s & 1);
        cur = min(max(cur, 0), n - 1);
    }
}

int gg_require(dm_ctx* ctx, int B, int N, int nnz, const void* cols, const void* w, const void* info) {
    DM_REQUIRE(ctx, B > 0 && N > 0 && nnz > 0, "sizes must be positive");
    DM_REQUIRE(ctx, N <= GG_MAXN, "N <= 16384 (the distances of a source live in the LDS of one workgroup)");
    DM_REQUIRE(ctx, B <= 65535, "at most 65535 meshes per call");
    DM_REQUIRE(ctx, cols && w && info, "null pointer");
    return DM_OK;
}

}  // namespace

extern "C" int dm_graph_geodesic(dm_ctx* ctx, int B, int N, int nnz, const int32_t* cols, const double* w, const int32_t* n_verts, int ns,
                                 const int32_t* sources, double* D, int32_t* info) {
    if (!ctx) return DM_EINVAL;
    int rc = gg_require(ctx, B, N, nnz, cols, w, info);
    if (rc) return rc;
    DM_REQUIRE(ctx, ns > 0 && sources && D, "sources (B, ns) and D (B, ns, N)");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t lds = (size_t)N * sizeof(double);
    // up to 4096 vertices: four waves per source, several sources per CU; above: sixteen waves on the one or two sources whose distances fit
    if (N <= 4096) {
        DM_LAUNCH(ctx, "graph_geodesic", graph_geodesic_kernel<256>, dim3(ns, B), dim3(256), lds, N, nnz, cols, w, n_verts, ns, sources, D, info);
    } else {
        rc = dm_grant_lds(ctx, (const void*)graph_geodesic_kernel<1024>, lds);
        if (rc) return rc;
        DM_LAUNCH(ctx, "graph_geodesic", graph_geodesic_kernel<1024>, dim3(ns, B), dim3(1024), lds, N, nnz, cols, w, n_verts, ns, sources, D, info);
    }
    return DM_OK;
}

extern "C" int dm_fps_graph(dm_ctx* ctx, int B, int N, int nnz, const int32_t* cols, const double* w, const int32_t* n_verts, int size,
                            const int32_t* start, int32_t* out, int32_t* info) {
    if (!ctx) return DM_EINVAL;
    int rc = gg_require(ctx, B, N, nnz, cols, w, info);
    if (rc) return rc;
    DM_REQUIRE(ctx, size > 0 && start && out, "start (B) and out (B, size)");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t lds = (size_t)N * sizeof(double);                       // + 384 bytes of static slots: 128.4 KiB of the CU's 160 at N = 16384
    rc = dm_grant_lds(ctx, (const void*)fps_graph_kernel, lds);
    if (rc) return rc;
    DM_LAUNCH(ctx, "fps_graph", fps_graph_kernel, dim3(B), dim3(GG_FPS_T), lds, N, nnz, cols, w, n_verts, size, start, out, info);
    return DM_OK;
}

// Map quality measures on the geodesic matrices of a padded batch (dm_map_metrics, dm_geodesic_diameter).
//
// Reference calls reproduced: densematcher/pyFM/eval/evaluate.py:29-36 (accuracy), :63-66 (continuity), :89-91 (coverage) and the
// diameter of densematcher/diffusion_net/geometry.py:773 (np.max of the distance matrix).  The reference fancy-indexes a host
// matrix; here the matrices stay where the geodesic calls left them and only the index lists and P numbers cross the bus.
//
// One WORKGROUP of 256 threads per problem, one launch for every problem of a call.  The reads of D are scattered 8-byte gathers,
// a cache line per element: that is the kernel's bound, nothing is staged.  A sum is taken in a fixed order that depends on the
// problem alone -- thread t adds the terms t, t + 256, t + 512, ... in ascending order, then a binary tree over the 256 partial sums
// in LDS -- so a problem's bits do not depend on what shares the call, on B, on the padding or on ld.  No floating-point atomics.
// Coverage marks the map's values in an LDS bitmap (integer OR; N <= 16384 is 2 KiB) and walks the vertices in ascending order,
// which is np.unique's order; the marked sum and the total take the same walk, so a map that reaches every vertex gives exactly 1.
//
// Work order: the host sorts the table by length, longest first (a stable sort); workgroups start in index order.
// An index outside its mesh is never used as an address: the problem's info is set to 1 and its value to NaN.
#include <algorithm>

#include "dm_device.h"
#include "dm_internal.h"

constexpr int MM_T = 256;               // threads per workgroup
constexpr int MM_MAX_N = 16384;         // the dense-storage limit: the bitmap holds one bit per vertex
constexpr int MM_ACCURACY = 0, MM_CONTINUITY = 1, MM_COVERAGE = 2;
constexpr int MM_FLAG_SCALE = 1, MM_FLAG_ALL = 2;

struct mm_prob {
    int kind, b, b2, a, bo, len, aux, flags;      // the table's row (aux: offset in `all` | length of the map's list | unused)
    int p, nv, nv2, pad;                          // index in the caller's table; vertex counts of mesh b / mesh b2
    double scale;
};

// red[0] = the tree sum of the 256 values (every thread passes one); all threads return it
__device__ __forceinline__ double mm_block_sum(double x, double* red) {
    const int t = threadIdx.x;
    __syncthreads();                                       // (red may still be read from the previous sum)
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int off = MM_T / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(MM_T) void mm_metrics_kernel(const double* __restrict__ D, int N, long long ld, const double* __restrict__ D2, int N2,
                                                          long long ld2, const double* __restrict__ area, const int32_t* __restrict__ idx,
                                                          const mm_prob* __restrict__ tab, double* __restrict__ value, double* __restrict__ all,
                                                          int32_t* __restrict__ info) {
    __shared__ double red[MM_T];
    __shared__ unsigned int bits[MM_MAX_N / 32];
    const mm_prob pr = tab[blockIdx.x];                    // (uniform)
    const int t = threadIdx.x;
    const unsigned int nv = (unsigned int)pr.nv, nv2 = (unsigned int)pr.nv2;
    int bad = 0;
    double s = 0.0, result;
    if (pr.kind == MM_ACCURACY) {
        const double* Db = D + (long long)pr.b * N * ld;
        const bool scaled = (pr.flags & MM_FLAG_SCALE) != 0, keep = (pr.flags & MM_FLAG_ALL) != 0;
        for (int i = t; i < pr.len; i += MM_T) {
            const unsigned int r = (unsigned int)idx[pr.a + i], c = (unsigned int)idx[pr.bo + i];
            if (r >= nv || c >= nv) { bad = 1; continue; }
            double d = Db[(long long)r * ld + c];
            if (scaled) d /= pr.scale;                     // element by element, as the reference divides
            if (keep) all[pr.aux + i] = d;
            s += d;
        }
        result = mm_block_sum(s, red) / (double)pr.len;
    } else if (pr.kind == MM_CONTINUITY) {
        const double* Db = D + (long long)pr.b * N * ld;
        const double* D2b = D2 + (long long)pr.b2 * N2 * ld2;
        const unsigned int nmap = (unsigned int)pr.aux;
        for (int e = t; e < pr.len; e += MM_T) {
            const unsigned int e0 = (unsigned int)idx[pr.bo + e], e1 = (unsigned int)idx[pr.bo + pr.len + e];
            if (e0 >= nv2 || e1 >= nv2 || e0 >= nmap || e1 >= nmap) { bad = 1; continue; }
            const unsigned int r = (unsigned int)idx[pr.a + e0], c = (unsigned int)idx[pr.a + e1];
            if (r >= nv || c >= nv) { bad = 1; continue; }
            s += Db[(long long)r * ld + c] / D2b[(long long)e0 * ld2 + e1];      // IEEE division, no guards: inf and NaN are carried
        }
        result = mm_block_sum(s, red) / (double)pr.len;
    } else {
        const double* ab = area + (long long)pr.b * N;
        for (int w = t; w < MM_MAX_N / 32; w += MM_T) bits[w] = 0u;
        __syncthreads();
        for (int i = t; i < pr.len; i += MM_T) {
            const unsigned int v = (unsigned int)idx[pr.a + i];
            if (v >= nv) { bad = 1; continue; }
            atomicOr(&bits[v >> 5], 1u << (v & 31));
        }
        __syncthreads();
        double tot = 0.0;
        for (unsigned int v = t; v < nv; v += MM_T) {
            const double x = ab[v];
            tot += x;
            if ((bits[v >> 5] >> (v & 31)) & 1u) s += x;
        }
        const double hit = mm_block_sum(s, red);
        result = hit / mm_block_sum(tot, red);
    }
    bad = __syncthreads_or(bad);
    if (t == 0) {
        value[pr.p] = bad ? __builtin_nan("") : result;
        info[pr.p] = bad ? 1 : 0;
    }
}

// np.max's rule on a running maximum: the first NaN wins and stays
__device__ __forceinline__ void mm_max_step(double& m, int& isnan_, double x) {
    isnan_ |= (x != x) ? 1 : 0;
    m = x > m ? x : m;
}
// the workgroup's maximum and NaN flag in thread 0
__device__ __forceinline__ void mm_block_max(double& m, int& isnan_, double* red) {
    const int t = threadIdx.x;
    isnan_ = __syncthreads_or(isnan_);
    red[t] = m;
    __syncthreads();
#pragma unroll
    for (int off = MM_T / 2; off > 0; off >>= 1) {
        if (t < off) red[t] = red[t + off] > red[t] ? red[t + off] : red[t];
        __syncthreads();
    }
    m = red[0];
}

// stage 1: workgroup (c, b) takes the rows c, c + gridDim.x, ... of D[b, :n, :n]; part (B, gridDim.x) maxima, flag the same shape
__global__ __launch_bounds__(MM_T) void mm_diam_part_kernel(const double* __restrict__ D, int N, long long ld, const int32_t* __restrict__ n_verts,
                                                            double* __restrict__ part, int32_t* __restrict__ flag) {
    __shared__ double red[MM_T];
    const int b = blockIdx.y, t = threadIdx.x;
    const int n = n_verts[b];
    const double* Db = D + (long long)b * N * ld;
    double m = -DM_INF_F64;
    int isnan_ = 0;
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const double* row = Db + (long long)r * ld;
        for (int c = t; c < n; c += MM_T) mm_max_step(m, isnan_, row[c]);
    }
    mm_block_max(m, isnan_, red);
    if (t == 0) {
        part[(long long)b * gridDim.x + blockIdx.x] = m;
        flag[(long long)b * gridDim.x + blockIdx.x] = isnan_;
    }
}
// stage 2: one workgroup per mesh over its `chunks` partial maxima
__global__ __launch_bounds__(MM_T) void mm_diam_final_kernel(const double* __restrict__ part, const int32_t* __restrict__ flag, int chunks,
                                                             double* __restrict__ out) {
    __shared__ double red[MM_T];
    const int b = blockIdx.x, t = threadIdx.x;
    double m = -DM_INF_F64;
    int isnan_ = 0;
    for (int c = t; c < chunks; c += MM_T) {
        const double x = part[(long long)b * chunks + c];
        m = x > m ? x : m;
        isnan_ |= flag[(long long)b * chunks + c];
    }
    mm_block_max(m, isnan_, red);
    if (t == 0) out[b] = isnan_ ? __builtin_nan("") : m;
}

static int mm_check_nverts(dm_ctx* ctx, int B, int N, const int32_t* n_verts, const char* what) {
    if (n_verts)
        for (int b = 0; b < B; ++b)
            if (n_verts[b] < 1 || n_verts[b] > N) return dm_fail(ctx, DM_EINVAL, "%s: vertex counts must lie in [1, N]", what);
    return DM_OK;
}

extern "C" int dm_map_metrics(dm_ctx* ctx, int B, int N, int ld, const double* D, int B2, int N2, int ld2, const double* D2,
                              const int32_t* n_verts, const int32_t* n_verts2, const double* area, int n_idx, const int32_t* idx, int P,
                              const int32_t* table, const double* scale, int n_all, double* value, double* all, int32_t* info) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && ld >= N && n_idx >= 0 && P >= 0 && n_all >= 0, "sizes must be positive, ld >= N");
    DM_REQUIRE(ctx, N <= MM_MAX_N, "N <= 16384 (the dense-storage limit)");
    if (!D2) { D2 = D; B2 = B; N2 = N; ld2 = ld; if (!n_verts2) n_verts2 = n_verts; }
    DM_REQUIRE(ctx, B2 > 0 && N2 > 0 && ld2 >= N2 && N2 <= MM_MAX_N, "sizes of D2 must be positive, ld2 >= N2, N2 <= 16384");
    if (P == 0) return DM_OK;
    DM_REQUIRE(ctx, idx && table && value && info, "null pointer");
    int rc = mm_check_nverts(ctx, B, N, n_verts, "dm_map_metrics");
    if (rc) return rc;
    rc = mm_check_nverts(ctx, B2, N2, n_verts2, "dm_map_metrics (second side)");
    if (rc) return rc;
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<mm_prob> tab((size_t)P);
    for (int p = 0; p < P; ++p) {
        const int32_t* e = table + (size_t)p * 8;
        mm_prob& t = tab[p];
        t.kind = e[0]; t.b = e[1]; t.b2 = e[2]; t.a = e[3]; t.bo = e[4]; t.len = e[5]; t.aux = e[6]; t.flags = e[7];
        t.p = p; t.pad = 0;
        t.scale = (scale && (t.flags & MM_FLAG_SCALE)) ? scale[p] : 1.0;
        DM_REQUIRE(ctx, t.kind >= MM_ACCURACY && t.kind <= MM_COVERAGE, "problem table: kind must be 0 (accuracy), 1 (continuity) or 2 (coverage)");
        DM_REQUIRE(ctx, t.b >= 0 && t.b < B, "problem table: mesh outside the batch");
        DM_REQUIRE(ctx, t.a >= 0 && t.len >= 0, "problem table: negative offset or length");
        t.nv = n_verts ? n_verts[t.b] : N;
        t.nv2 = 0;
        if (t.kind == MM_ACCURACY) {
            DM_REQUIRE(ctx, D, "an accuracy problem needs D");
            DM_REQUIRE(ctx, t.len > 0, "problem table: empty index list");
            DM_REQUIRE(ctx, t.bo >= 0 && (long long)t.a + t.len <= n_idx && (long long)t.bo + t.len <= n_idx,
                       "problem table: index list outside the index array");
            DM_REQUIRE(ctx, !(t.flags & MM_FLAG_SCALE) || scale, "problem table: a scaled problem needs the scale array");
            if (t.flags & MM_FLAG_ALL)
                DM_REQUIRE(ctx, all && t.aux >= 0 && (long long)t.aux + t.len <= n_all, "problem table: per-element output outside `all`");
        } else if (t.kind == MM_CONTINUITY) {
            DM_REQUIRE(ctx, D && D2, "a continuity problem needs D");
            DM_REQUIRE(ctx, t.len > 0, "problem table: empty edge list");
            DM_REQUIRE(ctx, t.b2 >= 0 && t.b2 < B2, "problem table: second mesh outside its batch");
            DM_REQUIRE(ctx, t.aux >= 0 && (long long)t.a + t.aux <= n_idx, "problem table: map outside the index array");
            DM_REQUIRE(ctx, t.bo >= 0 && (long long)t.bo + 2ll * t.len <= n_idx, "problem table: edge list outside the index array");
            t.nv2 = n_verts2 ? n_verts2[t.b2] : N2;
        } else {
            DM_REQUIRE(ctx, area, "a coverage problem needs the vertex areas");
            DM_REQUIRE(ctx, (long long)t.a + t.len <= n_idx, "problem table: index list outside the index array");
        }
    }
    std::stable_sort(tab.begin(), tab.end(), [](const mm_prob& x, const mm_prob& y) { return x.len > y.len; });
    rc = dm_ws_reserve(ctx, dm_align_up((size_t)P * sizeof(mm_prob)) + 4096);
    if (rc) return rc;
    mm_prob* d_tab = (mm_prob*)dm_ws_take(ctx, (size_t)P * sizeof(mm_prob));
    if (!d_tab) return dm_fail(ctx, DM_ENOMEM, "map_metrics: workspace not reserved");
    DM_CHECK_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), (size_t)P * sizeof(mm_prob), hipMemcpyHostToDevice, ctx->stream));
    DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the table is a local: copied before it goes away)
    DM_LAUNCH(ctx, "map_metrics", mm_metrics_kernel, dim3(P), dim3(MM_T), 0, D, N, (long long)ld, D2, N2, (long long)ld2, area, idx,
              (const mm_prob*)d_tab, value, all, info);
    return DM_OK;
}

extern "C" int dm_geodesic_diameter(dm_ctx* ctx, int B, int N, int ld, const double* D, const int32_t* n_verts, double* out) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && ld >= N, "sizes must be positive, ld >= N");
    DM_REQUIRE(ctx, D && out, "null pointer");
    int rc = mm_check_nverts(ctx, B, N, n_verts, "dm_geodesic_diameter");
    if (rc) return rc;
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int chunks = std::min(N, 128);
    std::vector<int32_t> nv((size_t)B);
    for (int b = 0; b < B; ++b) nv[b] = n_verts ? n_verts[b] : N;
    const size_t cells = (size_t)B * chunks;
    rc = dm_ws_reserve(ctx, dm_align_up((size_t)B * 4) + dm_align_up(cells * 8) + dm_align_up(cells * 4) + 4096);
    if (rc) return rc;
    int32_t* d_nv = (int32_t*)dm_ws_take(ctx, (size_t)B * 4);
    double* part = (double*)dm_ws_take(ctx, cells * 8);
    int32_t* flag = (int32_t*)dm_ws_take(ctx, cells * 4);
    if (!d_nv || !part || !flag) return dm_fail(ctx, DM_ENOMEM, "geodesic_diameter: workspace not reserved");
    DM_CHECK_HIP(ctx, hipMemcpyAsync(d_nv, nv.data(), (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
    DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the counts are a local: copied before they go away)
    DM_LAUNCH(ctx, "geodesic_diameter", mm_diam_part_kernel, dim3(chunks, B), dim3(MM_T), 0, D, N, (long long)ld, (const int32_t*)d_nv, part, flag);
    DM_LAUNCH(ctx, "geodesic_diameter", mm_diam_final_kernel, dim3(B), dim3(MM_T), 0, (const double*)part, (const int32_t*)flag, chunks, out);
    return DM_OK;
}

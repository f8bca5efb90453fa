// Heat-method geodesic distances (Crane et al. 2013) of B meshes, dense float64 on the f64 matrix cores.
//
// Replaces pyFM's heat_geodmat / heat_geodesic_from (pyFM/mesh/geometry.py:587-740) behind TriMesh.get_geodesic(robust=False) /
// geod_from(i, robust=False) (pyFM/mesh/trimesh.py:612-738), where SciPy's SuperLU factors A + tW and W and solves with N
// right-hand sides.  Here both systems are factored dense (blocked right-looking Cholesky, W grounded at vertex 0: its row and
// column replaced by the identity, so the singular W becomes SPD), then solved for a set of sources.  Grounding is exact only for a
// right-hand side in W's range, sum_i r_i = 0: that holds when A is one third of the adjacent face areas (sum_i va_i div_i =
// sum_f area_f (sum_c grad phi_c) . h_f = 0), and then the answer differs from SuperLU's only by the constant that the column
// min-shift removes.  Other masses (the intrinsic Laplacian's) make the system inconsistent: the caller refuses them
// (engine.heat_geodesic_check), since the reference's answer there depends on SuperLU's pivoting.
//   u   = (A + tW)^-1 e_j                                   forward + back substitution (blocked, MFMA)
//   g_f = sum_c u[f_c] grad phi_c,  h_f = -g_f / |g_f|      per face, recomputed by each of its three vertices (never stored)
//   r_i = A_i / va_i * sum_{(f,c) at i} area_f grad phi_c . h_f     (va = one third of the adjacent face areas)
//   phi = W_g^-1 r, phi -= min(phi), phi[j] = 0             forward + back substitution, then one reduction per row
//
// Layout.  Np = N rounded up to 64; block size 64 everywhere (the diagonal-block factorisation, the panel, the tiles of the trailing
// update and of the substitutions).  The factor buffer (dm_heat_geodesic_bytes) holds, for the 2B matrices z = b (A + tW of mesh b)
// and z = B + b (W_g of mesh b): the Np x Np matrix with L in its lower block triangle and L^T in its strictly upper one (the back
// substitution reads L^T row-wise), the inverses of the 64 x 64 diagonal blocks of L and their transposes; then the per-mesh geometry.
// A padded vertex (>= n_verts[b]) gets an identity row and column: it decouples exactly, so a mesh's numbers do not depend on Np.
//
// Bits.  Every sum runs in an order fixed by the block index and the position inside the block (MFMA k order), never by the number
// of sources or meshes of the call; an output column of a product depends only on its own right-hand side.  Skipped work (the zero
// blocks of the all-pairs forward substitution) is work whose result is an exact +0.  So a source's distances are bit-identical
// whichever other sources or meshes share the call.
#include <math.h>

#include "dm_gemm_f64.h"
#include "dm_internal.h"

namespace {

constexpr int GB = 64;                 // block size
constexpr int GEOD_MAXN = 16384;

// ---- layout of the factor buffer -----------------------------------------------------------------------------------------
struct geod_layout {
    int B, N, nt, Np;
    size_t mat, dinv, dinvt, geom, tri, va, mass, off, list, cnt, hdr, total;
    __host__ __device__ geod_layout(int B_, int N_, int nt_) : B(B_), N(N_), nt(nt_) {
        Np = (N + GB - 1) / GB * GB;
        size_t p = 0;
        auto take = [&](size_t bytes) { size_t q = p; p += dm_align_up(bytes); return q; };
        mat = take((size_t)2 * B * Np * Np * 8);
        dinv = take((size_t)2 * B * Np * GB * 8);
        dinvt = take((size_t)2 * B * Np * GB * 8);
        geom = take((size_t)B * nt * 10 * 8);      // per face: grad phi_0, grad phi_1, grad phi_2 (3 x 3), area
        tri = take((size_t)B * nt * 3 * 4);
        va = take((size_t)B * Np * 8);
        mass = take((size_t)B * Np * 8);
        off = take((size_t)B * (Np + 1) * 4);
        list = take((size_t)B * nt * 3 * 4);       // vertex -> (face, corner) as 3 f + c, ascending per vertex
        cnt = take((size_t)2 * B * Np * 4);        // counts and cursors of the list build
        hdr = take((size_t)B * 4 * 4);             // per mesh: n_verts
        total = p;
    }
};

// K-contiguous rows of a (Z, rows, ld) float64 array, columns [col0, col0 + 64); rows >= nrows read as zero
struct GeoRows {
    const double* p; long long stride_b; int ld; int col0; int nrows;
    __device__ __forceinline__ void load8(int b, int row, int k0, double (&v)[8]) const {
        if (row < nrows) {
            const f64x2* q = reinterpret_cast<const f64x2*>(p + b * stride_b + (long long)row * ld + col0 + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const f64x2 x = q[e]; v[2 * e] = x[0]; v[2 * e + 1] = x[1]; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.0;
        }
    }
};

// ---- geometry: per-face gradients and areas, the vertex -> (face, corner) lists ----------------------------------------------
// grads as _get_grad_dir (geometry.py:284-316) with the unit normals of compute_normals (geometry.py:110-133) and the areas of
// compute_faces_areas (geometry.py:48-70).  info bit 4: a face of zero area; bit 8: a face index outside [0, n_verts).
__global__ __launch_bounds__(256) void geod_faces_kernel(int B, int N, int nt, const int32_t* __restrict__ tri, const double* __restrict__ verts,
                                                        const int32_t* __restrict__ nv, double* __restrict__ geom, int32_t* __restrict__ tri_out,
                                                        int32_t* __restrict__ cnt, int Np, int32_t* __restrict__ info) {
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f >= nt) return;
    const int n = nv ? nv[b] : N;
    const int32_t* t3 = tri + ((long long)b * nt + f) * 3;
    int v[3] = {t3[0], t3[1], t3[2]};
    double* g = geom + ((long long)b * nt + f) * 10;
    int32_t* to = tri_out + ((long long)b * nt + f) * 3;
    if (v[0] < 0 && v[1] < 0 && v[2] < 0) {                      // padding face
        for (int e = 0; e < 10; ++e) g[e] = 0.0;
        to[0] = to[1] = to[2] = -1;
        return;
    }
    if (v[0] < 0 || v[0] >= n || v[1] < 0 || v[1] >= n || v[2] < 0 || v[2] >= n) {
        atomicOr(info + b, 8);
        for (int e = 0; e < 10; ++e) g[e] = 0.0;
        to[0] = to[1] = to[2] = -1;
        return;
    }
    double p[3][3];
    for (int c = 0; c < 3; ++c)
        for (int d = 0; d < 3; ++d) p[c][d] = verts[((long long)b * N + v[c]) * 3 + d];
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nrm = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    const double area = 0.5 * nrm;
    if (!(area > 0.0)) atomicOr(info + b, 4);
    const double un[3] = {cr[0] / nrm, cr[1] / nrm, cr[2] / nrm};
    for (int c = 0; c < 3; ++c) {                                // grad phi_c = cross(n, p_{c+2} - p_{c+1}) / (2 area)
        const int a = (c + 1) % 3, z = (c + 2) % 3;
        const double e[3] = {p[z][0] - p[a][0], p[z][1] - p[a][1], p[z][2] - p[a][2]};
        const double x[3] = {un[1] * e[2] - un[2] * e[1], un[2] * e[0] - un[0] * e[2], un[0] * e[1] - un[1] * e[0]};
        for (int d = 0; d < 3; ++d) g[3 * c + d] = x[d] / (2.0 * area);
    }
    g[9] = area;
    for (int c = 0; c < 3; ++c) {
        to[c] = v[c];
        atomicAdd(cnt + (long long)b * Np + v[c], 1);
    }
}

// exclusive scan of the per-vertex counts (one workgroup per mesh; 256 chunks of Np / 256 entries)
__global__ __launch_bounds__(256) void geod_scan_kernel(int Np, const int32_t* __restrict__ cnt, int32_t* __restrict__ off, int32_t* __restrict__ cursor) {
    __shared__ int part[257];
    const int b = blockIdx.x, t = threadIdx.x;
    const int chunk = (Np + 255) / 256, lo = min(Np, t * chunk), hi = min(Np, lo + chunk);
    const int32_t* c = cnt + (long long)b * Np;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += c[i];
    part[t + 1] = s;
    __syncthreads();
    if (t == 0) {
        part[0] = 0;
        for (int i = 1; i <= 256; ++i) part[i] += part[i - 1];
    }
    __syncthreads();
    int32_t* o = off + (long long)b * (Np + 1);
    int32_t* cu = cursor + (long long)b * Np;
    s = part[t];
    for (int i = lo; i < hi; ++i) { o[i] = s; cu[i] = s; s += c[i]; }
    if (t == 255) o[Np] = part[256];
}

__global__ __launch_bounds__(256) void geod_scatter_kernel(int nt, int Np, const int32_t* __restrict__ tri, int32_t* __restrict__ cursor,
                                                          int32_t* __restrict__ list) {
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f >= nt) return;
    const int32_t* t3 = tri + ((long long)b * nt + f) * 3;
    for (int c = 0; c < 3; ++c) {
        const int v = t3[c];
        if (v < 0) continue;
        const int pos = atomicAdd(cursor + (long long)b * Np + v, 1);
        list[(long long)b * nt * 3 + pos] = 3 * f + c;
    }
}

// sort each vertex's (face, corner) list (the atomics of the scatter leave it in arrival order), then the vertex area
// (compute_vertex_areas, geometry.py:73-107: one third of the adjacent face areas) and the lumped mass.  info bit 16: a vertex below
// n_verts that no face references.
__global__ __launch_bounds__(256) void geod_vertex_kernel(int N, int nt, int Np, const int32_t* __restrict__ nv, const int32_t* __restrict__ off,
                                                         int32_t* __restrict__ list, const double* __restrict__ geom, const double* __restrict__ mass64,
                                                         double* __restrict__ va, double* __restrict__ mass, int32_t* __restrict__ hdr,
                                                         int32_t* __restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= Np) return;
    const int n = nv ? nv[b] : N;
    if (i == 0) hdr[4 * b] = n;
    const int32_t* o = off + (long long)b * (Np + 1);
    int32_t* l = list + (long long)b * nt * 3;
    const int lo = o[i], hi = o[i + 1];
    for (int q = lo + 1; q < hi; ++q) {                           // insertion sort (a vertex has a handful of faces)
        const int x = l[q];
        int r = q - 1;
        while (r >= lo && l[r] > x) { l[r + 1] = l[r]; --r; }
        l[r + 1] = x;
    }
    double a = 0.0;
    for (int q = lo; q < hi; ++q) a += geom[((long long)b * nt + l[q] / 3) * 10 + 9] / 3.0;
    va[(long long)b * Np + i] = a;
    mass[(long long)b * Np + i] = i < n ? mass64[(long long)b * N + i] : 0.0;
    if (i < n && hi == lo) atomicOr(info + b, 16);
}

// ---- dense assembly: z = b: A + tW (scipy's A + t*W: A_ii + t W_ii on the diagonal), z = B + b: W grounded at vertex 0 ------------
// The matrices were zeroed by the caller.  One thread per row, the row's ELL entries in their stored order.
__global__ __launch_bounds__(256) void geod_assemble_kernel(int B, int N, int Np, int nnz, const int32_t* __restrict__ cols,
                                                           const double* __restrict__ wv, const double* __restrict__ mass64,
                                                           const double* __restrict__ tvec, const int32_t* __restrict__ nv,
                                                           double* __restrict__ mat, int32_t* __restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= Np) return;
    const int n = nv ? nv[b] : N;
    double* K = mat + (size_t)b * Np * Np + (size_t)i * Np;
    double* W = mat + (size_t)(B + b) * Np * Np + (size_t)i * Np;
    if (i >= n) { K[i] = 1.0; W[i] = 1.0; return; }
    const double t = tvec[b];
    K[i] = mass64[(long long)b * N + i];
    const int32_t* c = cols + ((long long)b * N + i) * nnz;
    const double* w = wv + ((long long)b * N + i) * nnz;
    bool bad = false;
    for (int e = 0; e < nnz; ++e) {
        const int j = c[e];
        if (j < 0 || j >= n) { bad = bad || w[e] != 0.0; continue; }
        K[j] += t * w[e];
        if (i != 0 && j != 0) W[j] += w[e];
    }
    if (i == 0) W[0] = 1.0;
    if (bad) atomicOr(info + b, 8);
}

// ---- blocked right-looking Cholesky, step k -----------------------------------------------------------------------------------
// (a) diagonal block: factored in LDS (one column per barrier), then inverted (one thread per column of L^-1).  The factor itself
//     is not stored: the panel and the substitutions use the inverse.  info bit 1 / 2: a non-positive pivot of A + tW / of W_g.
__global__ __launch_bounds__(256) void geod_potrf_diag_kernel(int B, int Np, int k, const double* __restrict__ mat, double* __restrict__ dinv,
                                                             double* __restrict__ dinvt, int32_t* __restrict__ info) {
    __shared__ double a[GB][GB + 1];
    __shared__ double x[GB][GB + 1];
    const int z = blockIdx.x, t = threadIdx.x;
    const double* M = mat + (size_t)z * Np * Np + (size_t)k * GB * Np + (size_t)k * GB;
    for (int e = t; e < GB * GB; e += 256) a[e >> 6][e & 63] = M[(size_t)(e >> 6) * Np + (e & 63)];
    __syncthreads();
    bool ok = true;
    double dp = 1.0, rp = 1.0;                                   // pivot and 1 / sqrt(pivot) of the previous column
    for (int j = 0; j < GB; ++j) {
        // column j - 1 is final: scale it (nothing else reads or writes it during this step)
        if (j > 0 && t == j - 1) a[t][t] = sqrt(dp);
        if (j > 0 && t > j - 1 && t < GB) a[t][j - 1] *= rp;
        const double d = a[j][j];
        ok = ok && (d > 0.0);
        const double r = 1.0 / sqrt(d);
        for (int e = t; e < GB * GB; e += 256) {
            const int i = e >> 6, c = e & 63;
            if (i > j && c > j && c <= i) a[i][c] -= (a[i][j] * r) * (a[c][j] * r);
        }
        dp = d;
        rp = r;
        __syncthreads();
    }
    if (t == GB - 1) a[t][t] = sqrt(dp);
    __syncthreads();
    if (t == 0 && !ok) atomicOr(info + (z % B), z < B ? 1 : 2);
    if (t < GB) {                                                 // X = L^-1, column t: forward substitution
        const int c = t;
        for (int i = 0; i < c; ++i) x[i][c] = 0.0;
        for (int i = c; i < GB; ++i) {
            double s = (i == c) ? 1.0 : 0.0;
            for (int m = c; m < i; ++m) s -= a[i][m] * x[m][c];
            x[i][c] = s / a[i][i];
        }
    }
    __syncthreads();
    double* Di = dinv + (size_t)z * Np * GB + (size_t)k * GB * GB;
    double* Dt = dinvt + (size_t)z * Np * GB + (size_t)k * GB * GB;
    for (int e = t; e < GB * GB; e += 256) {
        const int r = e >> 6, c = e & 63;
        Di[e] = x[r][c];
        Dt[e] = x[c][r];
    }
}

// (b) panel: L_IK = A_IK L_KK^-T for the block rows I > k, stored in the lower block column k and, transposed, in the upper block row k
__global__ __launch_bounds__(256) void geod_panel_kernel(int Np, int k, double* __restrict__ mat, const double* __restrict__ dinv) {
    __shared__ double As[NT_T * NT_LD];
    __shared__ double Bs[NT_T * NT_LD];
    const int z = blockIdx.z, I = k + 1 + blockIdx.x;
    double* M = mat + (size_t)z * Np * Np;
    const GeoRows opa{mat, (long long)Np * Np, Np, k * GB, Np};
    const GeoRows opb{dinv + (size_t)k * GB * GB, (long long)Np * GB, GB, 0, GB};
    f64x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = f64x4{0.0, 0.0, 0.0, 0.0};
    gemm_nt_body<false, 1>(opa, opb, z, I * GB, 0, GB, As, Bs, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = I * GB + wm * 32 + mt * 16 + (lane >> 4) + 4 * r;
                const int j = k * GB + wn * 32 + nt * 16 + (lane & 15);
                M[(size_t)i * Np + j] = acc[mt][nt][r];
                M[(size_t)j * Np + i] = acc[mt][nt][r];
            }
}

// (c) trailing update of the lower block triangle: A_IJ -= L_Ik L_Jk^T for k < J <= I
__global__ __launch_bounds__(256) void geod_update_kernel(int Np, int k, double* __restrict__ mat) {
    __shared__ double As[NT_T * NT_LD];
    __shared__ double Bs[NT_T * NT_LD];
    const int z = blockIdx.z, id = blockIdx.x;
    int ti = (int)((sqrt(8.0 * id + 1.0) - 1.0) * 0.5);            // id = ti (ti + 1) / 2 + tj, tj <= ti
    while (ti * (ti + 1) / 2 > id) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
    const int tj = id - ti * (ti + 1) / 2;
    const int I = k + 1 + ti, J = k + 1 + tj;
    double* M = mat + (size_t)z * Np * Np;
    const GeoRows op{mat, (long long)Np * Np, Np, k * GB, Np};
    f64x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = f64x4{0.0, 0.0, 0.0, 0.0};
    gemm_nt_body<false, 1>(op, op, z, I * GB, J * GB, GB, As, Bs, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = I * GB + wm * 32 + mt * 16 + (lane >> 4) + 4 * r;
                const int j = J * GB + wn * 32 + nt * 16 + (lane & 15);
                M[(size_t)i * Np + j] -= acc[mt][nt][r];
            }
}

// ---- solve --------------------------------------------------------------------------------------------------------------------
// right-hand sides: X[b][s] = e_{src[b][s]} (a row of zeros for src = -1)
__global__ __launch_bounds__(256) void geod_rhs_kernel(int Np, int ns, const int32_t* __restrict__ src, const int32_t* __restrict__ hdr,
                                                      double* __restrict__ X, int32_t* __restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    if (i >= Np) return;
    const int j = src[(long long)b * ns + s];
    if (i == 0 && (j < -1 || j >= hdr[4 * b])) atomicOr(info + b, 1);
    X[((long long)b * ns + s) * Np + i] = (i == j) ? 1.0 : 0.0;
}

// is every source of the 64-wide source tile s0 .. s0+63 in a vertex block after I? (then its block I of (A + tW)^-1's forward
// substitution is exactly zero and the tile has nothing to do.)  All threads call it.
__device__ __forceinline__ bool geod_tile_zero(const int32_t* src, int ns, int b, int s0, int I) {
    const int t = threadIdx.x;
    int j = -1;
    if (t < GB && s0 + t < ns) j = src[(long long)b * ns + s0 + t];
    const bool live = (t < GB) && (s0 + t < ns) && (j >= 0) && (j / GB <= I);
    return __syncthreads_or(live) == 0;
}

// X_I <- D_I X_I  for every right-hand side (D_I = L_II^-1 in the forward substitution, L_II^-T in the back substitution).
// grid (source tiles, 1, B); z0 selects the matrix (0: A + tW, B: W_g).  In place: a workgroup reads its sources' block before writing it.
__global__ __launch_bounds__(256) void geod_trsm_diag_kernel(int B, int Np, int ns, int I, int z0, const double* __restrict__ dmat,
                                                            double* __restrict__ X, const int32_t* __restrict__ src) {
    __shared__ double As[NT_T * NT_LD];
    __shared__ double Bs[NT_T * NT_LD];
    const int b = blockIdx.z, s0 = blockIdx.x * GB;
    if (src && geod_tile_zero(src, ns, b, s0, I)) return;
    const GeoRows opa{dmat + (size_t)(z0 + b) * Np * GB + (size_t)I * GB * GB, 0, GB, 0, GB};
    const GeoRows opb{X + (size_t)b * ns * Np, 0, Np, I * GB, ns};
    f64x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = f64x4{0.0, 0.0, 0.0, 0.0};
    gemm_nt_body<false, 1>(opa, opb, 0, 0, s0, GB, As, Bs, acc);
    double* Xb = X + (size_t)b * ns * Np;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = wm * 32 + mt * 16 + (lane >> 4) + 4 * r;
                const int s = s0 + wn * 32 + nt * 16 + (lane & 15);
                if (s < ns) Xb[(size_t)s * Np + I * GB + i] = acc[mt][nt][r];
            }
}

// X_R -= M_RI X_I for the block rows R after I (forward: M = L, lower part) or before I (back: M = L^T, upper part).
// grid (row tiles x source tiles, 1, B).
__global__ __launch_bounds__(256) void geod_trsm_update_kernel(int B, int Np, int ns, int I, int z0, int back, const double* __restrict__ mat,
                                                              double* __restrict__ X, const int32_t* __restrict__ src) {
    __shared__ double As[NT_T * NT_LD];
    __shared__ double Bs[NT_T * NT_LD];
    const int b = blockIdx.z;
    const int stiles = (ns + GB - 1) / GB;
    const int rt = blockIdx.x / stiles, s0 = (blockIdx.x % stiles) * GB;
    const int R = back ? rt : I + 1 + rt;
    if (src && geod_tile_zero(src, ns, b, s0, I)) return;
    const GeoRows opa{mat + (size_t)(z0 + b) * Np * Np, 0, Np, I * GB, Np};
    const GeoRows opb{X + (size_t)b * ns * Np, 0, Np, I * GB, ns};
    f64x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = f64x4{0.0, 0.0, 0.0, 0.0};
    gemm_nt_body<false, 1>(opa, opb, 0, R * GB, s0, GB, As, Bs, acc);
    double* Xb = X + (size_t)b * ns * Np;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = R * GB + wm * 32 + mt * 16 + (lane >> 4) + 4 * r;
                const int s = s0 + wn * 32 + nt * 16 + (lane & 15);
                if (s < ns) Xb[(size_t)s * Np + i] -= acc[mt][nt][r];
            }
}

// contract steps 3 - 4 fused (grad_f with use_sym=False and div_f, geometry.py:373-520, 651-660): one thread per (vertex, source);
// each incident face's gradient is recomputed from u (three loads), normalised, and dotted with area * grad phi_c, in the vertex's
// sorted list order.  r_i = A_i (sum / va_i); vertex 0 (grounded) and padding rows get 0.
__global__ __launch_bounds__(256) void geod_graddiv_kernel(int nt, int Np, int ns, const double* __restrict__ U, double* __restrict__ R,
                                                          const int32_t* __restrict__ tri, const double* __restrict__ geom,
                                                          const int32_t* __restrict__ off, const int32_t* __restrict__ list,
                                                          const double* __restrict__ va, const double* __restrict__ mass,
                                                          const int32_t* __restrict__ hdr) {
    const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    if (i >= Np) return;
    const int n = hdr[4 * b];
    double* r = R + ((size_t)b * ns + s) * Np;
    if (i == 0 || i >= n) { r[i] = 0.0; return; }
    const double* u = U + ((size_t)b * ns + s) * Np;
    const int32_t* o = off + (size_t)b * (Np + 1);
    const int32_t* l = list + (size_t)b * nt * 3;
    const int32_t* tb = tri + (size_t)b * nt * 3;
    const double* gb = geom + (size_t)b * nt * 10;
    double acc = 0.0;
    for (int q = o[i], qe = o[i + 1]; q < qe; ++q) {
        const int fc = l[q], f = fc / 3, c = fc - 3 * f;
        const double* g = gb + (size_t)f * 10;
        const double u0 = u[tb[3 * f]], d1 = u[tb[3 * f + 1]] - u0, d2 = u[tb[3 * f + 2]] - u0;
        const double gx = d1 * g[3] + d2 * g[6], gy = d1 * g[4] + d2 * g[7], gz = d1 * g[5] + d2 * g[8];
        const double nr = sqrt(gx * gx + gy * gy + gz * gz);
        const double hx = -gx / nr, hy = -gy / nr, hz = -gz / nr;
        const double a = g[9];
        acc += (a * g[3 * c]) * hx + (a * g[3 * c + 1]) * hy + (a * g[3 * c + 2]) * hz;
    }
    r[i] = mass[(size_t)b * Np + i] * (acc / va[(size_t)b * Np + i]);
}

// phi -= min(phi) over the mesh's vertices, phi[j] = 0; rows of D are (B, ns, N), zero past n_verts and for src = -1
__global__ __launch_bounds__(256) void geod_finish_kernel(int N, int Np, int ns, const double* __restrict__ P, const int32_t* __restrict__ src,
                                                         const int32_t* __restrict__ hdr, double* __restrict__ D) {
    __shared__ double red[256];
    const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int n = hdr[4 * b], j = src[(size_t)b * ns + s];
    const double* p = P + ((size_t)b * ns + s) * Np;
    double* d = D + ((size_t)b * ns + s) * N;
    double mn = DM_INF_F64;
    for (int i = t; i < n; i += 256) mn = fmin(mn, p[i]);
    red[t] = mn;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] = fmin(red[t], red[t + w]);
        __syncthreads();
    }
    mn = red[0];
    const bool live = j >= 0 && j < n;
    for (int i = t; i < N; i += 256) d[i] = (live && i < n && i != j) ? p[i] - mn : 0.0;
}

}  // namespace

extern "C" size_t dm_heat_geodesic_bytes(int B, int N, int nt) {
    if (B <= 0 || N <= 0 || nt <= 0 || N > GEOD_MAXN) return 0;
    return geod_layout(B, N, nt).total;
}

extern "C" int dm_heat_geodesic_factor(dm_ctx* ctx, int B, int N, int nt, const int32_t* tri, const double* verts, const int32_t* ell_cols,
                                       const double* w_vals, int nnz, const double* mass64, const double* t, const int32_t* n_verts,
                                       void* factors, int32_t* info) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && nt > 0 && nnz > 0 && B <= 32767, "sizes must be positive, B <= 32767");
    DM_REQUIRE(ctx, N <= GEOD_MAXN, "N <= 16384 (three N x N float64 matrices per mesh)");
    DM_REQUIRE(ctx, tri && verts && ell_cols && w_vals && mass64 && t && factors && info, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const geod_layout g(B, N, nt);
    char* f = (char*)factors;
    double* mat = (double*)(f + g.mat);
    double* dinv = (double*)(f + g.dinv);
    double* dinvt = (double*)(f + g.dinvt);
    double* geom = (double*)(f + g.geom);
    int32_t* trio = (int32_t*)(f + g.tri);
    double* va = (double*)(f + g.va);
    double* mass = (double*)(f + g.mass);
    int32_t* off = (int32_t*)(f + g.off);
    int32_t* list = (int32_t*)(f + g.list);
    int32_t* cnt = (int32_t*)(f + g.cnt);
    int32_t* cursor = cnt + (size_t)B * g.Np;
    int32_t* hdr = (int32_t*)(f + g.hdr);
    const int Np = g.Np, NB = Np / GB;
    DM_CHECK_HIP(ctx, hipMemsetAsync(info, 0, (size_t)B * 4, ctx->stream));
    DM_CHECK_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)2 * B * Np * 4, ctx->stream));
    DM_CHECK_HIP(ctx, hipMemsetAsync(mat, 0, (size_t)2 * B * Np * Np * 8, ctx->stream));
    const dim3 gf(dm_cdiv(nt, 256), B), gv(dm_cdiv(Np, 256), B);
    DM_LAUNCH(ctx, "geod_faces", geod_faces_kernel, gf, dim3(256), 0, B, N, nt, tri, verts, n_verts, geom, trio, cnt, Np, info);
    DM_LAUNCH(ctx, "geod_scan", geod_scan_kernel, dim3(B), dim3(256), 0, Np, (const int32_t*)cnt, off, cursor);
    DM_LAUNCH(ctx, "geod_scatter", geod_scatter_kernel, gf, dim3(256), 0, nt, Np, (const int32_t*)trio, cursor, list);
    DM_LAUNCH(ctx, "geod_vertex", geod_vertex_kernel, gv, dim3(256), 0, N, nt, Np, n_verts, (const int32_t*)off, list, (const double*)geom, mass64,
              va, mass, hdr, info);
    DM_LAUNCH(ctx, "geod_assemble", geod_assemble_kernel, gv, dim3(256), 0, B, N, Np, nnz, ell_cols, w_vals, mass64, t, n_verts, mat, info);
    for (int k = 0; k < NB; ++k) {
        DM_LAUNCH(ctx, "geod_potrf_diag", geod_potrf_diag_kernel, dim3(2 * B), dim3(256), 0, B, Np, k, (const double*)mat, dinv, dinvt, info);
        const int T = NB - 1 - k;
        if (T == 0) break;
        DM_LAUNCH(ctx, "geod_panel", geod_panel_kernel, dim3(T, 1, 2 * B), dim3(256), 0, Np, k, mat, (const double*)dinv);
        DM_LAUNCH(ctx, "geod_update", geod_update_kernel, dim3(T * (T + 1) / 2, 1, 2 * B), dim3(256), 0, Np, k, mat);
    }
    return DM_OK;
}

namespace {
// forward + back substitution of matrix z0 (0: A + tW, B: W_g) for every right-hand side of X; `src` (nullable): skip the zero blocks
// of unit right-hand sides in the forward pass
int geod_subst(dm_ctx* ctx, const geod_layout& g, int ns, int z0, const double* mat, const double* dinv, const double* dinvt, double* X,
               const int32_t* src) {
    const int B = g.B, Np = g.Np, NB = Np / GB, st = dm_cdiv(ns, GB);
    for (int I = 0; I < NB; ++I) {
        DM_LAUNCH(ctx, "geod_trsm_diag", geod_trsm_diag_kernel, dim3(st, 1, B), dim3(256), 0, B, Np, ns, I, z0, dinv, X, src);
        if (I + 1 < NB)
            DM_LAUNCH(ctx, "geod_trsm_update", geod_trsm_update_kernel, dim3((NB - 1 - I) * st, 1, B), dim3(256), 0, B, Np, ns, I, z0, 0, mat, X, src);
    }
    for (int I = NB - 1; I >= 0; --I) {
        DM_LAUNCH(ctx, "geod_trsm_diag", geod_trsm_diag_kernel, dim3(st, 1, B), dim3(256), 0, B, Np, ns, I, z0, dinvt, X, (const int32_t*)nullptr);
        if (I > 0)
            DM_LAUNCH(ctx, "geod_trsm_update", geod_trsm_update_kernel, dim3(I * st, 1, B), dim3(256), 0, B, Np, ns, I, z0, 1, mat, X,
                      (const int32_t*)nullptr);
    }
    return DM_OK;
}
}  // namespace

namespace {
// the solve on buffers the caller took: X, R = B ns Np doubles each; info is accumulated into (not cleared)
int geod_solve_core(dm_ctx* ctx, const geod_layout& g, const void* factors, int ns, const int32_t* sources, double* D, double* X, double* R,
                    int32_t* info) {
    const int B = g.B, N = g.N, nt = g.nt, Np = g.Np;
    const char* f = (const char*)factors;
    const double* mat = (const double*)(f + g.mat);
    const double* dinv = (const double*)(f + g.dinv);
    const double* dinvt = (const double*)(f + g.dinvt);
    const int32_t* hdr = (const int32_t*)(f + g.hdr);
    DM_LAUNCH(ctx, "geod_rhs", geod_rhs_kernel, dim3(dm_cdiv(Np, 256), ns, B), dim3(256), 0, Np, ns, sources, hdr, X, info);
    int rc = geod_subst(ctx, g, ns, 0, mat, dinv, dinvt, X, sources);
    if (rc != DM_OK) return rc;
    DM_LAUNCH(ctx, "geod_graddiv", geod_graddiv_kernel, dim3(dm_cdiv(Np, 256), ns, B), dim3(256), 0, nt, Np, ns, (const double*)X, R,
              (const int32_t*)(f + g.tri), (const double*)(f + g.geom), (const int32_t*)(f + g.off), (const int32_t*)(f + g.list),
              (const double*)(f + g.va), (const double*)(f + g.mass), hdr);
    rc = geod_subst(ctx, g, ns, B, mat, dinv, dinvt, R, nullptr);
    if (rc != DM_OK) return rc;
    DM_LAUNCH(ctx, "geod_finish", geod_finish_kernel, dim3(ns, B), dim3(256), 0, N, Np, ns, (const double*)R, sources, hdr, D);
    return DM_OK;
}

// sources of the all-pairs solve: src[b][i] = i for i < n_verts[b], else -1
__global__ __launch_bounds__(256) void geod_iota_kernel(int N, const int32_t* __restrict__ hdr, int32_t* __restrict__ src) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i < N) src[(size_t)b * N + i] = i < hdr[4 * b] ? i : -1;
}
}  // namespace

extern "C" int dm_heat_geodesic_solve(dm_ctx* ctx, int B, int N, int nt, const void* factors, int ns, const int32_t* sources, double* D,
                                      int32_t* info) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && nt > 0 && ns > 0 && B <= 32767 && ns <= 65535, "sizes must be positive, B <= 32767, ns <= 65535");
    DM_REQUIRE(ctx, N <= GEOD_MAXN, "N <= 16384");
    DM_REQUIRE(ctx, factors && sources && D && info, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const geod_layout g(B, N, nt);
    const size_t xb = (size_t)B * ns * g.Np * 8;
    int rc = dm_ws_reserve(ctx, 2 * dm_align_up(xb));
    if (rc != DM_OK) return rc;
    double* X = (double*)dm_ws_take(ctx, xb);
    double* R = (double*)dm_ws_take(ctx, xb);
    DM_CHECK_HIP(ctx, hipMemsetAsync(info, 0, (size_t)B * 4, ctx->stream));
    return geod_solve_core(ctx, g, factors, ns, sources, D, X, R, info);
}

// ---- farthest-point sampling on heat-method distances (TriMesh.extract_fps(geodesic=True, robust=False)) ----------------------------
// d(i) = row i of dm_heat_geodesic_solve = the distances FROM vertex i.  Route (a): the all-pairs rows once (B N^2 doubles + the solve's
// 2 B N Np), then ONE sampling launch (dm_fps.hip: fps_rows).  Route (b), where that does not fit (or "fps_heat_route" = 2): per sample
// one single-source solve whose source the previous step left in device memory, and one small kernel that folds the row in and
// writes the next source.  A row's bits do not depend on the other sources of its solve, so both routes return the same indices.
int dm_fps_rows(dm_ctx* ctx, int B, int N, const double* D, long long strideD, int ldd, const int32_t* nv4, int size, const int32_t* start,
                int32_t* out, int32_t* info);
int dm_fps_step_init(dm_ctx* ctx, int B, int N, const int32_t* nv4, int size, const int32_t* start, double* dists, int32_t* cur, int32_t* out,
                     int32_t* info);
int dm_fps_step(dm_ctx* ctx, int B, int N, const double* drow, const int32_t* nv4, int size, int s, double* dists, int32_t* cur, int32_t* out,
                int32_t* info);

extern "C" int dm_fps_heat(dm_ctx* ctx, int B, int N, int nt, const void* factors, int size, const int32_t* start, int32_t* out, int32_t* info) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && nt > 0 && size > 0 && B <= 32767, "sizes must be positive, B <= 32767");
    DM_REQUIRE(ctx, N <= GEOD_MAXN, "N <= 16384");
    DM_REQUIRE(ctx, factors && start && out && info, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const geod_layout g(B, N, nt);
    const int32_t* hdr = (const int32_t*)((const char*)factors + g.hdr);
    const size_t all = dm_align_up((size_t)B * N * N * 8) + 2 * dm_align_up((size_t)B * N * g.Np * 8) + dm_align_up((size_t)B * N * 4);
    size_t free_b = 0, total_b = 0;
    DM_CHECK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    // the all-pairs route while its work space fits what the context already holds plus half of the free device memory, and N <= 65535
    const bool fits = N <= 65535 && all <= ctx->ws_bytes + free_b / 2;
    const bool route_a = ctx->opt_fps_heat_route == 1 || (ctx->opt_fps_heat_route != 2 && fits);
    DM_CHECK_HIP(ctx, hipMemsetAsync(info, 0, (size_t)B * 4, ctx->stream));
    if (route_a) {
        int rc = dm_ws_reserve(ctx, all);
        if (rc != DM_OK) return rc;
        double* D = (double*)dm_ws_take(ctx, (size_t)B * N * N * 8);
        double* X = (double*)dm_ws_take(ctx, (size_t)B * N * g.Np * 8);
        double* R = (double*)dm_ws_take(ctx, (size_t)B * N * g.Np * 8);
        int32_t* src = (int32_t*)dm_ws_take(ctx, (size_t)B * N * 4);
        if (!D || !X || !R || !src) return dm_fail(ctx, DM_ENOMEM, "fps_heat: workspace not reserved");
        DM_LAUNCH(ctx, "geod_iota", geod_iota_kernel, dim3(dm_cdiv(N, 256), B), dim3(256), 0, N, hdr, src);
        rc = geod_solve_core(ctx, g, factors, N, src, D, X, R, info);
        if (rc != DM_OK) return rc;
        return dm_fps_rows(ctx, B, N, D, (long long)N * N, N, hdr, size, start, out, info);
    }
    int rc = dm_ws_reserve(ctx, dm_align_up((size_t)B * N * 8) * 2 + 2 * dm_align_up((size_t)B * g.Np * 8) + dm_align_up((size_t)B * 4));
    if (rc != DM_OK) return rc;
    double* dists = (double*)dm_ws_take(ctx, (size_t)B * N * 8);
    double* drow = (double*)dm_ws_take(ctx, (size_t)B * N * 8);
    double* X = (double*)dm_ws_take(ctx, (size_t)B * g.Np * 8);
    double* R = (double*)dm_ws_take(ctx, (size_t)B * g.Np * 8);
    int32_t* cur = (int32_t*)dm_ws_take(ctx, (size_t)B * 4);
    if (!dists || !drow || !X || !R || !cur) return dm_fail(ctx, DM_ENOMEM, "fps_heat: workspace not reserved");
    rc = dm_fps_step_init(ctx, B, N, hdr, size, start, dists, cur, out, info);
    if (rc != DM_OK) return rc;
    for (int s = 0; s + 1 < size; ++s) {
        rc = geod_solve_core(ctx, g, factors, 1, cur, drow, X, R, info);
        if (rc != DM_OK) return rc;
        rc = dm_fps_step(ctx, B, N, drow, hdr, size, s, dists, cur, out, info);
        if (rc != DM_OK) return rc;
    }
    return DM_OK;
}

// DiffusionNet operator precomputation for a padded batch of triangle meshes: dm_dnet_rows (assembly) and dm_dnet_ell (fill).
//
// Reference computation replaced: diffusion_net.geometry.compute_operators without its eigensolve (diffusion_net/geometry.py:
//   38-48, 80-111   unit face normals raw / (|raw| + 1e-6), vertex normals = their sum over the incident corners, normalised;
//   151-177         tangent frames (bx, by, n): e_x (|n . e_x| < 0.9) or e_y projected to the tangent plane, / (norm + 1e-6), by = n x bx;
//   321-323         the weak cotangent Laplacian 1/2 cot = 1/2 dot / (|cross| + denom_eps) per corner and a third of the incident
//                   areas per vertex (the potpourri3d wheel there; here the formulas its calls name) + mass_eps mean(mass);
//   197-272         build_grad: per vertex the least-squares gradient over the off-diagonal columns of its row of L,
//                   M = sum t t^T + grad_eps I, g_j = M^-1 t_j, g_self = -sum g_j -- a Python loop over edges and vertices there;
//   339-342         the operand of the eigensolve, L + shift I with the masses).
// One thread per vertex does all of it from the vertex's corner list (dm_corners.h, as dm_laplacian.hip): the frame and the gradient
// row of a vertex need its own normal only.  Everything is summed in a fixed order (corners ascending, then columns ascending), so
// a mesh gives the same bits whatever else shares the call.  The ELL width is only known after the assembly: two calls, like
// dm_laplacian_rows / dm_laplacian_ell.
#include <algorithm>
#include <vector>

#include "dm_corners.h"
#include "dm_dnet_common.h"

struct dnet_rows_out {
    int32_t* rowlen; int32_t* rowcol;                 // (B, N), (B, N, LAP_MAXROW)
    double* rowl; double* rowgx; double* rowgy;       // (B, N, LAP_MAXROW) on rowcol's columns; the diagonal slot of gx / gy holds g_self
    double* mass;                                     // (B, N) a third of the incident areas (padding vertices: 1)
    int32_t* maxlen; int32_t* bad;                    // (B), (1)
    double* frames;                                   // (B, N, 3, 3) rows bx, by, n
    int32_t* info;                                    // (B) bit 1: a vertex whose summed face normals have no direction
    const double* normals;                            // (B, N, 3) given normals, or null: from the faces
    double denom_eps, grad_eps;
};

__global__ __launch_bounds__(128) void dnet_rows_kernel(lap_args a, const int32_t* __restrict__ offset, int32_t* __restrict__ list, dnet_rows_out o) {
    const int b = blockIdx.y;
    const int v = blockIdx.x * 128 + threadIdx.x;
    if (v >= a.N) return;
    const long long bv = (long long)b * a.N + v;
    int32_t* rc = o.rowcol + bv * LAP_MAXROW;
    double* rl = o.rowl + bv * LAP_MAXROW;
    double* gx = o.rowgx + bv * LAP_MAXROW;
    double* gy = o.rowgy + bv * LAP_MAXROW;
    double* fr = o.frames + bv * 9;
    const int nvb = lap_nv(a, b);
    if (v >= nvb) {                                          // a padding vertex: a decoupled row, unit mass, zero frame and gradient row
        rc[0] = v; rl[0] = 0.0; gx[0] = 0.0; gy[0] = 0.0;
        o.rowlen[bv] = 1; o.mass[bv] = 1.0;
        for (int e = 0; e < 9; ++e) fr[e] = 0.0;
        atomicMax(o.maxlen + b, 1);
        return;
    }
    const int o0 = offset[(long long)b * (a.N + 1) + v], o1 = offset[(long long)b * (a.N + 1) + v + 1];
    int32_t* lst = list + (long long)b * 3 * a.nt;
    for (int i = o0 + 1; i < o1; ++i) {                      // insertion sort of the (few) corners
        const int x = lst[i];
        int j = i - 1;
        while (j >= o0 && lst[j] > x) { lst[j + 1] = lst[j]; --j; }
        lst[j + 1] = x;
    }
    const double* V = a.verts + (long long)b * a.N * 3;
    const double pi[3] = {V[3 * (long long)v], V[3 * (long long)v + 1], V[3 * (long long)v + 2]};
    int nr = 1;
    rc[0] = v; rl[0] = 0.0;
    double m = 0.0, diag = 0.0, ns[3] = {0.0, 0.0, 0.0};
    bool overflow = false, badidx = false;
    for (int i = o0; i < o1; ++i) {
        const int h = lst[i], t = h / 3, s = h - 3 * t;
        const int32_t* T = a.tri + ((long long)b * a.nt + t) * 3;
        const int vb = T[(s + 1) % 3], vc = T[(s + 2) % 3];
        if ((unsigned)vb >= (unsigned)nvb || (unsigned)vc >= (unsigned)nvb || (unsigned)T[0] >= (unsigned)nvb ||
            (unsigned)T[1] >= (unsigned)nvb || (unsigned)T[2] >= (unsigned)nvb) { badidx = true; continue; }
        // the face's normal and area from its own corner order (the same numbers at its three vertices)
        const double* p0 = V + 3 * (long long)T[0];
        const double* p1 = V + 3 * (long long)T[1];
        const double* p2 = V + 3 * (long long)T[2];
        const double A[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const double Bv[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        const double raw[3] = {A[1] * Bv[2] - A[2] * Bv[1], A[2] * Bv[0] - A[0] * Bv[2], A[0] * Bv[1] - A[1] * Bv[0]};
        const double rn = sqrt(raw[0] * raw[0] + raw[1] * raw[1] + raw[2] * raw[2]);
        const double rd = rn + 1e-6;
        ns[0] += raw[0] / rd; ns[1] += raw[1] / rd; ns[2] += raw[2] / rd;
        m += 0.5 * rn / 3.0;
        // the two weights of this corner's row: w_ab = 1/2 cot(angle at c), w_ac = 1/2 cot(angle at b)
        const double* pb = V + 3 * (long long)vb;
        const double* pc = V + 3 * (long long)vc;
        double w[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double* pk = e ? pb : pc;                  // the corner whose angle faces the edge (v, other)
            const double* pj = e ? pc : pb;
            const double u[3] = {pi[0] - pk[0], pi[1] - pk[1], pi[2] - pk[2]};
            const double x[3] = {pj[0] - pk[0], pj[1] - pk[1], pj[2] - pk[2]};
            const double dt = u[0] * x[0] + u[1] * x[1] + u[2] * x[2];
            const double c0 = u[1] * x[2] - u[2] * x[1], c1 = u[2] * x[0] - u[0] * x[2], c2 = u[0] * x[1] - u[1] * x[0];
            w[e] = 0.5 * (dt / (sqrt(c0 * c0 + c1 * c1 + c2 * c2) + o.denom_eps));
        }
        diag += w[0]; diag += w[1];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int col = e ? vc : vb;
            if (col == v) { diag -= w[e]; continue; }        // (a degenerate face that repeats a vertex contributes nothing to the row)
            int q = 1;
            while (q < nr && rc[q] != col) ++q;
            if (q == nr) {
                if (nr == LAP_MAXROW) { overflow = true; continue; }
                rc[nr] = col; rl[nr] = 0.0; ++nr;
            }
            rl[q] -= w[e];
        }
    }
    rl[0] = diag;
    for (int i = 1; i < nr; ++i) {                           // entries by column (the diagonal keeps its place among them)
        const int c = rc[i]; const double x = rl[i];
        int j = i - 1;
        while (j >= 0 && rc[j] > c) { rc[j + 1] = rc[j]; rl[j + 1] = rl[j]; --j; }
        rc[j + 1] = c; rl[j + 1] = x;
    }
    // ---- normal and tangent frame
    double n[3];
    if (o.normals) {
        n[0] = o.normals[bv * 3]; n[1] = o.normals[bv * 3 + 1]; n[2] = o.normals[bv * 3 + 2];
    } else {
        const double nn = sqrt(ns[0] * ns[0] + ns[1] * ns[1] + ns[2] * ns[2]);
        if (nn > 0.0) { n[0] = ns[0] / nn; n[1] = ns[1] / nn; n[2] = ns[2] / nn; }
        else { n[0] = n[1] = n[2] = 0.0; atomicOr(o.info + b, 1); }     // (unreferenced, exactly cancelling faces, or not a number: the host repairs it)
    }
    const bool use_x = fabs(n[0]) < 0.9;
    const double cd[3] = {use_x ? 1.0 : 0.0, use_x ? 0.0 : 1.0, 0.0};
    const double dots = use_x ? n[0] : n[1];
    double bx[3] = {cd[0] - n[0] * dots, cd[1] - n[1] * dots, cd[2] - n[2] * dots};
    const double bd = sqrt(bx[0] * bx[0] + bx[1] * bx[1] + bx[2] * bx[2]) + 1e-6;
    bx[0] /= bd; bx[1] /= bd; bx[2] /= bd;
    double by[3] = {n[1] * bx[2] - n[2] * bx[1], n[2] * bx[0] - n[0] * bx[2], n[0] * bx[1] - n[1] * bx[0]};
    if (!o.normals && !(n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0)) { bx[0] = bx[1] = bx[2] = 0.0; by[0] = by[1] = by[2] = 0.0; }
    fr[0] = bx[0]; fr[1] = bx[1]; fr[2] = bx[2];
    fr[3] = by[0]; fr[4] = by[1]; fr[5] = by[2];
    fr[6] = n[0]; fr[7] = n[1]; fr[8] = n[2];
    // ---- gradient row over the off-diagonal columns, ascending
    double maa = 0.0, mab = 0.0, mbb = 0.0;
    for (int q = 0; q < nr; ++q) {
        const int c = rc[q];
        if (c == v) continue;
        const double* pj = V + 3 * (long long)c;
        const double d[3] = {pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]};
        const double tx = d[0] * bx[0] + d[1] * bx[1] + d[2] * bx[2];
        const double ty = d[0] * by[0] + d[1] * by[1] + d[2] * by[2];
        gx[q] = tx; gy[q] = ty;
        maa += tx * tx; mab += tx * ty; mbb += ty * ty;
    }
    maa += o.grad_eps; mbb += o.grad_eps;
    const double det = maa * mbb - mab * mab;
    double sx = 0.0, sy = 0.0;
    int qd = 0;
    for (int q = 0; q < nr; ++q) {
        if (rc[q] == v) { qd = q; continue; }
        const double tx = gx[q], ty = gy[q];
        const double ex = (mbb * tx - mab * ty) / det, ey = (maa * ty - mab * tx) / det;
        gx[q] = ex; gy[q] = ey;
        sx += ex; sy += ey;
    }
    gx[qd] = -sx; gy[qd] = -sy;
    o.rowlen[bv] = nr;
    o.mass[bv] = m;
    atomicMax(o.maxlen + b, nr);
    if (overflow) atomicOr(o.bad, 2);
    if (badidx) atomicOr(o.bad, 1);
}

// mass64 = a third of the incident areas + mass_eps * their mean over the mesh's own vertices (one workgroup per mesh, a fixed
// order of additions that depends on the mesh's vertex count alone); padding vertices keep unit mass
__global__ __launch_bounds__(256) void dnet_mass_kernel(int N, const int32_t* __restrict__ nv, double mass_eps, const double* __restrict__ raw,
                                                        double* __restrict__ mass64, float* __restrict__ mass32) {
    __shared__ double sh[256];
    const int b = blockIdx.x, t = threadIdx.x, nb = nv ? nv[b] : N;
    double s = 0.0;
    for (int i = t; i < nb; i += 256) s += raw[(long long)b * N + i];
    sh[t] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if (t < off) sh[t] += sh[t + off]; __syncthreads(); }
    const double add = mass_eps * (sh[0] / (double)nb);
    for (int i = t; i < N; i += 256) {
        const double mv = i < nb ? raw[(long long)b * N + i] + add : 1.0;
        mass64[(long long)b * N + i] = mv;
        mass32[(long long)b * N + i] = (float)mv;
    }
}

// the rows at the ELL width: columns, L, gradX, gradY, and M'^-1/2 (L + shift I) M'^-1/2 with the masses rounded to fp32 first
// (the operand of dm_eigenbasis, as lap_fill_kernel scales it); padded with (col = row, val = 0)
__global__ __launch_bounds__(256) void dnet_fill_kernel(int N, int nnz, double shift, const int32_t* __restrict__ rowlen, const int32_t* __restrict__ rowcol,
                                                        const double* __restrict__ rowl, const double* __restrict__ rowgx, const double* __restrict__ rowgy,
                                                        const float* __restrict__ mass32, int32_t* __restrict__ ell_cols, double* __restrict__ l_vals,
                                                        double* __restrict__ ell_vals, double* __restrict__ gx_vals, double* __restrict__ gy_vals) {
    const int b = blockIdx.y;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)N * nnz) return;
    const int v = (int)(e / nnz), q = (int)(e - (long long)v * nnz);
    const long long bv = (long long)b * N + v;
    const int nr = rowlen[bv];
    const long long o = bv * nnz + q;
    if (q < nr) {
        const int c = rowcol[bv * LAP_MAXROW + q];
        const double w = rowl[bv * LAP_MAXROW + q];
        const double mv = (double)mass32[bv], mc = (double)mass32[(long long)b * N + c];
        ell_cols[o] = c;
        l_vals[o] = w;
        ell_vals[o] = (c == v ? w + shift : w) / (sqrt(mv) * sqrt(mc));
        gx_vals[o] = rowgx[bv * LAP_MAXROW + q];
        gy_vals[o] = rowgy[bv * LAP_MAXROW + q];
    } else {
        ell_cols[o] = v; l_vals[o] = 0.0; ell_vals[o] = 0.0; gx_vals[o] = 0.0; gy_vals[o] = 0.0;
    }
}

namespace {
struct dnet_rows_layout {
    int32_t *count, *cursor, *rowlen, *offset, *list, *rowcol, *maxlen;
    double *rowl, *rowgx, *rowgy, *mass;
    dnet_rows_layout(void* rows, int B, int N, int nt) {
        char* p = (char*)rows;
        auto take = [&](size_t bytes) { char* q = p; p += dm_align_up(bytes); return q; };
        count = (int32_t*)take((size_t)B * N * 4);
        cursor = (int32_t*)take((size_t)B * N * 4);
        rowlen = (int32_t*)take((size_t)B * N * 4);
        offset = (int32_t*)take((size_t)B * (N + 1) * 4);
        list = (int32_t*)take((size_t)B * 3 * nt * 4);
        rowcol = (int32_t*)take((size_t)B * N * LAP_MAXROW * 4);
        rowl = (double*)take((size_t)B * N * LAP_MAXROW * 8);
        rowgx = (double*)take((size_t)B * N * LAP_MAXROW * 8);
        rowgy = (double*)take((size_t)B * N * LAP_MAXROW * 8);
        mass = (double*)take((size_t)B * N * 8);
        maxlen = (int32_t*)take((size_t)(B + 1) * 4);
    }
};
}  // namespace

extern "C" size_t dm_dnet_rows_bytes(int B, int N, int nt) {
    if (B <= 0 || N <= 0 || nt <= 0) return 0;
    return dm_align_up((size_t)B * N * 4) * 3 + dm_align_up((size_t)B * (N + 1) * 4) + dm_align_up((size_t)B * 3 * nt * 4) +
           dm_align_up((size_t)B * N * LAP_MAXROW * 4) + dm_align_up((size_t)B * N * LAP_MAXROW * 8) * 3 + dm_align_up((size_t)B * N * 8) +
           dm_align_up((size_t)(B + 1) * 4) + 4096;
}

// Stage 1: rows of L, gradX, gradY and the raw masses in `rows` (dm_dnet_rows_bytes of device memory the caller owns), the frames
// and info (device); max_row (host) = the longest row over the batch.  Synchronises the stream for that number, and once before for the
// check of n_verts (each in [1, N]).
extern "C" int dm_dnet_rows(dm_ctx* ctx, int B, int N, int nt, const int32_t* tri, const double* verts, const double* normals /*nullable*/,
                            const int32_t* n_verts /*nullable*/, double denom_eps, double grad_eps, void* rows, double* frames, int32_t* info,
                            int* max_row) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && nt > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, tri && verts && rows && frames && info && max_row, "null pointer");
    DM_REQUIRE(ctx, denom_eps >= 0.0 && grad_eps > 0.0, "denom_eps >= 0, grad_eps > 0");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "diffusion operators", B, N, n_verts)) return rc;
    dnet_rows_layout r(rows, B, N, nt);
    int32_t* bad = r.maxlen + B;
    lap_args a{B, N, nt, tri, nullptr, verts, 1.0, n_verts};
    DM_CHECK_HIP(ctx, hipMemsetAsync(r.count, 0, (size_t)B * N * 4, ctx->stream));
    DM_CHECK_HIP(ctx, hipMemsetAsync(r.maxlen, 0, (size_t)(B + 1) * 4, ctx->stream));
    DM_CHECK_HIP(ctx, hipMemsetAsync(info, 0, (size_t)B * 4, ctx->stream));
    const dim3 gh(dm_cdiv(3 * nt, 256), B);
    DM_LAUNCH(ctx, "lap_count", lap_count_kernel, gh, dim3(256), 0, a, r.count, bad);
    DM_LAUNCH(ctx, "lap_scan", lap_scan_kernel, dim3(B), dim3(1024), 0, N, (const int32_t*)r.count, r.offset, r.cursor);
    DM_LAUNCH(ctx, "lap_scatter", lap_scatter_kernel, gh, dim3(256), 0, a, r.cursor, r.list);
    dnet_rows_out o{r.rowlen, r.rowcol, r.rowl, r.rowgx, r.rowgy, r.mass, r.maxlen, bad, frames, info, normals, denom_eps, grad_eps};
    DM_LAUNCH(ctx, "dnet_rows", dnet_rows_kernel, dim3(dm_cdiv(N, 128), B), dim3(128), 0, a, (const int32_t*)r.offset, r.list, o);
    std::vector<int32_t> h((size_t)B + 1);
    DM_CHECK_HIP(ctx, hipMemcpyAsync(h.data(), r.maxlen, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h[B] & 1) return dm_fail(ctx, DM_EINVAL, "diffusion operators: face indices must lie in [0, n_verts)");
    if (h[B] & 2) return dm_fail(ctx, DM_EINVAL, "diffusion operators: a vertex has more than %d neighbours", LAP_MAXROW - 1);
    int mx = 1;
    for (int b = 0; b < B; ++b) mx = std::max(mx, (int)h[b]);
    *max_row = mx;
    return DM_OK;
}

// Stage 2: the rows at the ELL width nnz >= max_row of stage 1 -- row_len (B, N); ell_cols, l_vals, ell_vals, gx_vals, gy_vals
// (B, N, nnz); mass64, mass32 (B, N).  nnz and n_verts are checked against what stage 1 left in `rows` (one read-back each).
extern "C" int dm_dnet_ell(dm_ctx* ctx, int B, int N, int nt, const void* rows, int nnz, const int32_t* n_verts /*nullable*/, double mass_eps,
                           double shift, int32_t* row_len, int32_t* ell_cols, double* l_vals, double* ell_vals, double* gx_vals, double* gy_vals,
                           double* mass64, float* mass32) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && nt > 0 && nnz > 0 && nnz <= LAP_MAXROW && B <= 65535, "sizes");
    DM_REQUIRE(ctx, rows && row_len && ell_cols && l_vals && ell_vals && gx_vals && gy_vals && mass64 && mass32, "null pointer");
    DM_REQUIRE(ctx, mass_eps >= 0.0 && shift >= 0.0, "mass_eps >= 0, shift >= 0");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const dnet_rows_layout r(const_cast<void*>(rows), B, N, nt);
    // what stage 1 left in `rows` decides whether nnz is wide enough (a narrower width would drop entries): read the row maxima back
    if (int rc = dm_dnet_check_counts(ctx, "diffusion operators", B, N, n_verts)) return rc;
    std::vector<int32_t> h((size_t)B + 1);
    DM_CHECK_HIP(ctx, hipMemcpyAsync(h.data(), r.maxlen, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h[B] != 0) return dm_fail(ctx, DM_EINVAL, "diffusion operators: dm_dnet_rows failed on these rows");
    for (int b = 0; b < B; ++b)
        if (h[b] < 1 || h[b] > nnz) return dm_fail(ctx, DM_EINVAL, "diffusion operators: nnz = %d is narrower than the longest row (%d) of dm_dnet_rows, or rows was not written by it", nnz, (int)h[b]);
    DM_LAUNCH(ctx, "dnet_mass", dnet_mass_kernel, dim3(B), dim3(256), 0, N, n_verts, mass_eps, (const double*)r.mass, mass64, mass32);
    const long long per = (long long)N * nnz;
    DM_LAUNCH(ctx, "dnet_fill", dnet_fill_kernel, dim3((unsigned)((per + 255) / 256), B), dim3(256), 0, N, nnz, shift, (const int32_t*)r.rowlen,
              (const int32_t*)r.rowcol, (const double*)r.rowl, (const double*)r.rowgx, (const double*)r.rowgy, (const float*)mass32, ell_cols, l_vals,
              ell_vals, gx_vals, gy_vals);
    if (n_verts) DM_LAUNCH(ctx, "lap_pad", lap_pad_kernel, dim3(B), dim3(256), 0, N, nnz, n_verts, ell_vals);
    DM_CHECK_HIP(ctx, hipMemcpyAsync(row_len, r.rowlen, (size_t)B * N * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return DM_OK;
}

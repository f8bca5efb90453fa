// Textured-mesh rendering: dm_render_phong, the hard-Phong views of a ragged batch of raw meshes (the images the 2D backbone takes).
//
// Reference computation replaced: densematcher/render.py
//   31-35     RasterizationSettings(blur_radius 0, one face per pixel), MeshRasterizer: the raster rule is this library's
//             (densematch.h, dm_raster.h), shared with dm_raster_pix2face
//   36-44     PointLights at the camera centre, HardPhongShader with default Materials and BlendParams
//   47-53     the RGBA images, zbuf and the pix2face of the mesh's own face indices
//
// Three passes besides the shared projection and key-image pass.  Vertex normals: one thread per vertex over its incident corners
// in ascending face order (a host-built CSR), float64, no atomics: a mesh's bits do not depend on what shares the call.  Shade: one
// thread per pixel; the owner's barycentrics are recomputed in float64 with the raster's expressions and perspective-corrected in
// float64; interpolation, the four texture taps and the lighting run in fp32 in a fixed order.  All memory operations are vector
// loads, stores and atomics.
#include <math.h>

#include <hip/hip_fp16.h>

#include "dm_internal.h"
#include "dm_raster.h"

namespace {
constexpr int RN_VIEWS_MAX = 64;
constexpr float RN_EPS = 1e-6f;      // n / max(|n|, eps), for every normalisation

// ---------------------------------------------------------------------------------------------------------------- vertex normals
// normals[b][i] = s / max(|s|, 1e-6), s = the sum over the faces incident to i (one entry per corner, ascending face index) of
// cross(v1 - v0, v2 - v0).  inc_ptr (B, N + 1), inc_face (B, n_inc): the CSR of the corners.
__global__ void __launch_bounds__(256) render_normals_kernel(int N, int nt, int n_inc, const double* __restrict__ verts, const int32_t* __restrict__ tri,
                                                             const int32_t* __restrict__ n_verts, const int32_t* __restrict__ inc_ptr,
                                                             const int32_t* __restrict__ inc_face, const int32_t* __restrict__ given,
                                                             double* __restrict__ normals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= N || (given && given[b])) return;
    double* o = normals + ((size_t)b * N + i) * 3;
    const int nv = lf_count(n_verts, b, N);
    if (i >= nv) {
        o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
        return;
    }
    const int32_t* ptr = inc_ptr + (size_t)b * (N + 1);
    const int lo = min(max(ptr[i], 0), n_inc), hi = min(max(ptr[i + 1], lo), n_inc);
    const double* V = verts + (size_t)b * N * 3;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = lo; k < hi; ++k) {
        const int f = inc_face[(size_t)b * n_inc + k];
        if (f < 0 || f >= nt) continue;
        const int32_t* t = tri + ((size_t)b * nt + f) * 3;
        const int i0 = t[0], i1 = t[1], i2 = t[2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) continue;
        const double ax = V[3 * i1] - V[3 * i0], ay = V[3 * i1 + 1] - V[3 * i0 + 1], az = V[3 * i1 + 2] - V[3 * i0 + 2];
        const double bx = V[3 * i2] - V[3 * i0], by = V[3 * i2 + 1] - V[3 * i0 + 1], bz = V[3 * i2 + 2] - V[3 * i0 + 2];
        sx += ay * bz - az * by;
        sy += az * bx - ax * bz;
        sz += ax * by - ay * bx;
    }
    const double len = fmax(sqrt(sx * sx + sy * sy + sz * sz), 1e-6);
    o[0] = sx / len; o[1] = sy / len; o[2] = sz / len;
}

// ---------------------------------------------------------------------------------------------------------------- shading
struct shade_args {
    int N, nt, Vw, H, W, p_dtype;
    const int32_t* tri; const int32_t* n_verts; const int32_t* n_views;
    const double* verts; const double* normals; const double* R; const double* T; const double* light;
    const double* proj; const unsigned long long* keys;
    const long long* tex;       // (B, 8): kind, address of the colours / the map, Ht, Wt, address of verts_uvs, of faces_uvs, n_uv, n_fuv
    float ambient[3], diffuse[3], specular[3], background[3], shininess;
    float* rgba; float* zbuf; int32_t* pix2face; void* planes;
};

__device__ __forceinline__ float rn_mix(float c0, float a0, float c1, float a1, float c2, float a2) { return fmaf(c2, a2, fmaf(c1, a1, c0 * a0)); }

__device__ __forceinline__ void rn_unit(float& x, float& y, float& z) {
    const float len = fmaxf(sqrtf(fmaf(z, z, fmaf(y, y, x * x))), RN_EPS);
    x /= len; y /= len; z /= len;
}

__device__ __forceinline__ void rn_store_planes(const shade_args& a, size_t bv, int p, float r, float g, float bl) {
    if (!a.planes) return;
    const size_t hw = (size_t)a.H * a.W, at = bv * 3 * hw + p;
    if (a.p_dtype == DM_F16) {
        __half* o = (__half*)a.planes;
        o[at] = __float2half_rn(r); o[at + hw] = __float2half_rn(g); o[at + 2 * hw] = __float2half_rn(bl);
    } else {
        float* o = (float*)a.planes;
        o[at] = r; o[at + hw] = g; o[at + 2 * hw] = bl;
    }
}

// one thread per pixel
__global__ void __launch_bounds__(256) render_shade_kernel(shade_args a) {
    const int v = blockIdx.y, b = blockIdx.z;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.H * a.W) return;
    const size_t bv = (size_t)b * a.Vw + v, at = bv * a.H * a.W + p;
    const int nv = lf_count(a.n_verts, b, a.N);
    int f = -1, i0 = 0, i1 = 0, i2 = 0;
    unsigned long long key = RS_EMPTY;
    if (v < lf_count(a.n_views, b, a.Vw)) {
        key = a.keys[at];
        if (key != RS_EMPTY) f = (int)(unsigned int)(key & 0xffffffffull);
    }
    if (f >= a.nt) f = -1;
    if (f >= 0) {
        const int32_t* t = a.tri + ((size_t)b * a.nt + f) * 3;
        i0 = t[0]; i1 = t[1]; i2 = t[2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) f = -1;
    }
    if (f < 0) {
        *reinterpret_cast<float4*>(a.rgba + at * 4) = make_float4(a.background[0], a.background[1], a.background[2], 0.0f);
        a.zbuf[at] = -1.0f;
        a.pix2face[at] = -1;
        rn_store_planes(a, bv, p, a.background[0], a.background[1], a.background[2]);
        return;
    }
    // ---- the owner's barycentrics, the raster's expressions (dm_raster.h), then the perspective correction, float64
    const double* pr = a.proj + bv * a.N * 4;
    const double x0 = pr[4 * i0], y0 = pr[4 * i0 + 1], Z0 = pr[4 * i0 + 2];
    const double x1 = pr[4 * i1], y1 = pr[4 * i1 + 1], Z1 = pr[4 * i1 + 2];
    const double x2 = pr[4 * i2], y2 = pr[4 * i2 + 1], Z2 = pr[4 * i2 + 2];
    const double area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0);
    const int r = p / a.W, c = p % a.W;
    const double px = 1.0 - (double)(2 * c + 1) / a.W, py = 1.0 - (double)(2 * r + 1) / a.H;
    const double w0 = (px - x1) * (y2 - y1) - (py - y1) * (x2 - x1);
    const double w1 = (px - x2) * (y0 - y2) - (py - y2) * (x0 - x2);
    const double w2 = (px - x0) * (y1 - y0) - (py - y0) * (x1 - x0);
    const double q0 = (w0 / area) / Z0, q1 = (w1 / area) / Z1, q2 = (w2 / area) / Z2;
    const double qs = q0 + q1 + q2;
    const float c0 = (float)(q0 / qs), c1 = (float)(q1 / qs), c2 = (float)(q2 / qs);
    // ---- position and normal, fp32
    const double* V = a.verts + (size_t)b * a.N * 3;
    const double* Nn = a.normals + (size_t)b * a.N * 3;
    const float P0 = rn_mix(c0, (float)V[3 * i0], c1, (float)V[3 * i1], c2, (float)V[3 * i2]);
    const float P1 = rn_mix(c0, (float)V[3 * i0 + 1], c1, (float)V[3 * i1 + 1], c2, (float)V[3 * i2 + 1]);
    const float P2 = rn_mix(c0, (float)V[3 * i0 + 2], c1, (float)V[3 * i1 + 2], c2, (float)V[3 * i2 + 2]);
    float n0 = rn_mix(c0, (float)Nn[3 * i0], c1, (float)Nn[3 * i1], c2, (float)Nn[3 * i2]);
    float n1 = rn_mix(c0, (float)Nn[3 * i0 + 1], c1, (float)Nn[3 * i1 + 1], c2, (float)Nn[3 * i2 + 1]);
    float n2 = rn_mix(c0, (float)Nn[3 * i0 + 2], c1, (float)Nn[3 * i1 + 2], c2, (float)Nn[3 * i2 + 2]);
    rn_unit(n0, n1, n2);
    // ---- texel
    float t0 = 1.0f, t1 = 1.0f, t2 = 1.0f;
    const long long* td = a.tex + (size_t)b * 8;
    const long long kind = td[0];
    if (kind == 1 && td[1] && td[2] >= nv) {                                      // per-vertex colours (n, 3) fp32
        const float* col = reinterpret_cast<const float*>(td[1]);
        t0 = rn_mix(c0, col[3 * i0], c1, col[3 * i1], c2, col[3 * i2]);
        t1 = rn_mix(c0, col[3 * i0 + 1], c1, col[3 * i1 + 1], c2, col[3 * i2 + 1]);
        t2 = rn_mix(c0, col[3 * i0 + 2], c1, col[3 * i1 + 2], c2, col[3 * i2 + 2]);
    } else if (kind == 2 && td[1] && td[4] && td[5] && td[2] > 0 && td[3] > 0 && f < td[7]) {
        const float* map = reinterpret_cast<const float*>(td[1]);
        const float* uvs = reinterpret_cast<const float*>(td[4]);
        const int32_t* fu = reinterpret_cast<const int32_t*>(td[5]) + (size_t)f * 3;
        const int Ht = (int)td[2], Wt = (int)td[3];
        const long long n_uv = td[6];
        const int j0 = fu[0], j1 = fu[1], j2 = fu[2];
        if (j0 >= 0 && j1 >= 0 && j2 >= 0 && j0 < n_uv && j1 < n_uv && j2 < n_uv) {
            const float u = rn_mix(c0, uvs[2 * j0], c1, uvs[2 * j1], c2, uvs[2 * j2]);
            const float w = rn_mix(c0, uvs[2 * j0 + 1], c1, uvs[2 * j1 + 1], c2, uvs[2 * j2 + 1]);
            // grid_sample(flip(map, rows), 2 uv - 1, align_corners=True, border): x = u (Wt - 1), y = (1 - v)(Ht - 1), clamped to the map
            const float x = fminf(fmaxf(u * (float)(Wt - 1), 0.0f), (float)(Wt - 1));
            const float y = fminf(fmaxf((1.0f - w) * (float)(Ht - 1), 0.0f), (float)(Ht - 1));
            const float fx = floorf(x), fy = floorf(y);
            const int xa = (int)fx, ya = (int)fy, xb = min(xa + 1, Wt - 1), yb = min(ya + 1, Ht - 1);
            const float tx = x - fx, ty = y - fy;
            const float wnw = (1.0f - tx) * (1.0f - ty), wne = tx * (1.0f - ty), wsw = (1.0f - tx) * ty, wse = tx * ty;
            const float* nw = map + ((size_t)ya * Wt + xa) * 3;
            const float* ne = map + ((size_t)ya * Wt + xb) * 3;
            const float* sw = map + ((size_t)yb * Wt + xa) * 3;
            const float* se = map + ((size_t)yb * Wt + xb) * 3;
            t0 = fmaf(wse, se[0], fmaf(wsw, sw[0], fmaf(wne, ne[0], wnw * nw[0])));       // taps in the order nw, ne, sw, se
            t1 = fmaf(wse, se[1], fmaf(wsw, sw[1], fmaf(wne, ne[1], wnw * nw[1])));
            t2 = fmaf(wse, se[2], fmaf(wsw, sw[2], fmaf(wne, ne[2], wnw * nw[2])));
        }
    }
    // ---- one point light, Phong
    const double* Rm = a.R + bv * 9;
    const double* Tm = a.T + bv * 3;
    const float C0 = (float)(-(Tm[0] * Rm[0] + Tm[1] * Rm[1] + Tm[2] * Rm[2]));        // the camera centre C = -T R^T
    const float C1 = (float)(-(Tm[0] * Rm[3] + Tm[1] * Rm[4] + Tm[2] * Rm[5]));
    const float C2 = (float)(-(Tm[0] * Rm[6] + Tm[1] * Rm[7] + Tm[2] * Rm[8]));
    float l0 = C0, l1 = C1, l2 = C2;
    if (a.light) { l0 = (float)a.light[bv * 3]; l1 = (float)a.light[bv * 3 + 1]; l2 = (float)a.light[bv * 3 + 2]; }
    l0 -= P0; l1 -= P1; l2 -= P2;
    rn_unit(l0, l1, l2);
    float e0 = C0 - P0, e1 = C1 - P1, e2 = C2 - P2;
    rn_unit(e0, e1, e2);
    const float cs = fmaf(n2, l2, fmaf(n1, l1, n0 * l0));
    const float lit = fmaxf(cs, 0.0f);
    const float r0 = fmaf(2.0f * cs, n0, -l0), r1 = fmaf(2.0f * cs, n1, -l1), r2 = fmaf(2.0f * cs, n2, -l2);
    const float al = cs > 0.0f ? fmaxf(fmaf(e2, r2, fmaf(e1, r1, e0 * r0)), 0.0f) : 0.0f;
    const float sp = powf(al, a.shininess);
    const float o0 = fmaf(fmaf(a.diffuse[0], lit, a.ambient[0]), t0, a.specular[0] * sp);
    const float o1 = fmaf(fmaf(a.diffuse[1], lit, a.ambient[1]), t1, a.specular[1] * sp);
    const float o2 = fmaf(fmaf(a.diffuse[2], lit, a.ambient[2]), t2, a.specular[2] * sp);
    *reinterpret_cast<float4*>(a.rgba + at * 4) = make_float4(o0, o1, o2, 1.0f);
    a.zbuf[at] = __uint_as_float((unsigned int)(key >> 32));
    a.pix2face[at] = f;
    rn_store_planes(a, bv, p, o0, o1, o2);
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry point
extern "C" int dm_render_phong(dm_ctx* ctx, int B, int N, int nt, int views, int H, int W, const double* verts, const int32_t* tri,
                               const int32_t* n_verts /*nullable*/, const double* R, const double* T, const int32_t* n_views /*nullable*/,
                               double focal, const int32_t* inc_ptr, const int32_t* inc_face, int n_inc,
                               const int32_t* normals_given /*nullable*/, double* normals, const long long* tex,
                               const double* light /*nullable*/, const float* shade /*host, 13*/, float* rgba, float* zbuf,
                               int32_t* pix2face, void* planes /*nullable*/, int p_dtype) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && nt > 0 && views > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, views <= RN_VIEWS_MAX, "at most 64 views per mesh");
    DM_REQUIRE(ctx, H > 0 && H == W && H <= 16384, "square images up to 16384 x 16384");
    DM_REQUIRE(ctx, verts && tri && R && T && normals && tex && shade && rgba && zbuf && pix2face, "null pointer");
    DM_REQUIRE(ctx, inc_ptr && inc_face && n_inc > 0, "the corner lists of the vertices");
    DM_REQUIRE(ctx, focal > 0.0 && focal < 1e300, "the focal length must be positive and finite");
    DM_REQUIRE(ctx, !planes || p_dtype == DM_F16 || p_dtype == DM_F32, "p_dtype: DM_F16 or DM_F32");
    for (int k = 0; k < 13; ++k) DM_REQUIRE(ctx, isfinite(shade[k]), "colours and shininess must be finite");
    const long long n_items = (long long)B * views * nt;
    DM_REQUIRE(ctx, n_items / 4 + 1 < (1ll << 31) && (long long)B * views * N < (1ll << 40), "too many (mesh, view, face) items for one launch");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_pix = (size_t)B * views * H * W, key_bytes = n_pix * sizeof(unsigned long long);
    const size_t proj_bytes = (size_t)B * views * N * 4 * sizeof(double);
    if (int rc = dm_ws_reserve(ctx, dm_align_up(key_bytes) + dm_align_up(proj_bytes))) return rc;
    unsigned long long* keys = (unsigned long long*)dm_ws_take(ctx, key_bytes);
    double* proj = (double*)dm_ws_take(ctx, proj_bytes);
    if (!keys || !proj) return dm_fail(ctx, DM_ENOMEM, "dm_render_phong: the key image and the projections do not fit the workspace");
    DM_CHECK_HIP(ctx, hipMemsetAsync(keys, 0xff, key_bytes, ctx->stream));
    DM_LAUNCH(ctx, "render_normals", render_normals_kernel, dim3(dm_cdiv(N, 256), B), dim3(256), 0, N, nt, n_inc, verts, tri, n_verts, inc_ptr, inc_face,
              normals_given, normals);
    DM_LAUNCH(ctx, "lift_project", lift_project_kernel, dim3(dm_cdiv(N, 256), views, B), dim3(256), 0, N, views, verts, n_verts, R, T, n_views, focal, proj);
    face_args fa{N, nt, views, H, W, tri, n_verts, n_views, nullptr, proj, keys};
    DM_LAUNCH(ctx, "lift_faces", lift_faces_kernel, dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, fa, n_items);
    shade_args sa{N, nt, views, H, W, p_dtype, tri, n_verts, n_views, verts, normals, R, T, light, proj, keys, tex,
                  {shade[0], shade[1], shade[2]}, {shade[3], shade[4], shade[5]}, {shade[6], shade[7], shade[8]}, {shade[9], shade[10], shade[11]}, shade[12],
                  rgba, zbuf, pix2face, planes};
    DM_LAUNCH(ctx, "render_shade", render_shade_kernel, dim3(dm_cdiv(H * W, 256), views, B), dim3(256), 0, sa);
    return DM_OK;
}

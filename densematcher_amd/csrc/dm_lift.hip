// Multi-view feature lifting: dm_raster_pix2face (visibility of the simplified mesh in every view) and dm_lift_features (bilinear
// taps of the per-view feature maps at the projected vertices, averaged over the views that see a vertex).
//
// Reference computation replaced: densematcher/projection.py
//   60-62     pix2face of the simplified mesh (pytorch3d's rasteriser behind render.py:31-53: blur_radius 0, one face per pixel, no
//             culling); the raster rule itself is this library's (densematch.h), not pytorch3d's code
//   94-102    visible faces -> their vertices -> the frame test -1 < x, y < 1 on the projected vertices
//   103-105   grid_sample(ft, -(x, y), align_corners=True), bilinear, zero padding; the sum over the views
//   118-121   the count of views per vertex and the mean
//
// Raster: the nearest face per pixel is a MINIMUM over 64-bit keys (fp32 bits of the depth << 32 | face), taken with one integer
// atomic per covered (face, pixel): the result does not depend on the order of faces, wavefronts or workgroups, and equal depths go
// to the lowest face index.  Lifting: one workgroup per (mesh, 8 vertices); the taps of every (vertex, view) are worked out once
// into LDS, the threads then run over (vertex, channel).  A vertex's sum runs over the views in ascending order in its own thread:
// no float atomics, no sums across workgroups, so its bits depend on its own mesh alone.  All memory operations are vector loads,
// stores and atomics.
#include <math.h>

#include <hip/hip_fp16.h>

#include "dm_internal.h"
#include "dm_raster.h"

namespace {
constexpr int LF_VB = 8;            // vertices per workgroup (lifting)
constexpr int LF_VIEWS_MAX = 64;    // views per mesh: LF_VB * 64 tap records of 32 bytes = 16 KB of LDS

// one thread per pixel: pix2face from the key image (or as given), and the marks of the owning face's vertices
__global__ void __launch_bounds__(256) lift_resolve_kernel(face_args a, int32_t* __restrict__ pix2face, unsigned char* __restrict__ vis) {
    const int v = blockIdx.y, b = blockIdx.z;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.H * a.W) return;
    const size_t at = ((size_t)b * a.Vw + v) * a.H * a.W + p;
    const bool given = a.given && a.given[b];
    int f = -1;
    if (v < lf_count(a.n_views, b, a.Vw)) {
        if (given) {
            f = pix2face[at];
        } else {
            const unsigned long long key = a.keys[at];
            f = key == RS_EMPTY ? -1 : (int)(unsigned int)(key & 0xffffffffull);
        }
    }
    if (!given) pix2face[at] = f;
    if (f < 0 || f >= a.nt) return;
    const int nv = lf_count(a.n_verts, b, a.N);
    const int32_t* t = a.tri + ((size_t)b * a.nt + f) * 3;
    const int i0 = t[0], i1 = t[1], i2 = t[2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return;
    unsigned char* m = vis + ((size_t)b * a.Vw + v) * a.N;
    m[i0] = 1; m[i1] = 1; m[i2] = 1;                                // the same value from every writer
}

// ---------------------------------------------------------------------------------------------------------------- lifting
struct lift_args {
    int N, Vw, C, H, W;
    const long long* maps;      // (B, 5): address, then the strides (view, channel, row, col) in elements
    const double* proj; const unsigned char* vis; const int32_t* n_verts; const int32_t* n_views;
    float* out; int ldo; int32_t* count;
};

struct lf_tap { long long base; float w[4]; int ok; int pad; };    // base: element offset of the nw tap; ok: bit q = tap q is read

__device__ __forceinline__ float lf_load(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float lf_load(const float* p) { return *p; }

template <typename TM>
__global__ void __launch_bounds__(256) lift_features_kernel(lift_args a) {
    __shared__ lf_tap taps[LF_VB * LF_VIEWS_MAX];
    const int b = blockIdx.y, i_first = blockIdx.x * LF_VB;
    const int nv = lf_count(a.n_verts, b, a.N), nw = lf_count(a.n_views, b, a.Vw);
    const long long* md = a.maps + (size_t)b * 5;
    const TM* map = reinterpret_cast<const TM*>(md[0]);
    const long long sv = md[1], sc = md[2], sr = md[3], sw = md[4];
    for (int q = threadIdx.x; q < LF_VB * a.Vw; q += blockDim.x) {
        const int j = q / a.Vw, v = q % a.Vw, i = i_first + j;
        lf_tap t;
        t.base = 0; t.w[0] = t.w[1] = t.w[2] = t.w[3] = 0.0f; t.ok = 0; t.pad = 0;
        if (i < nv && v < nw && a.vis[((size_t)b * a.Vw + v) * a.N + i]) {
            const double* pr = a.proj + (((size_t)b * a.Vw + v) * a.N + i) * 4;
            if (pr[3] != 0.0) {
                // grid = -(x, y); align_corners: ix = (g + 1) / 2 (W - 1)
                const double ix = (-pr[0] + 1.0) * 0.5 * (a.W - 1), iy = (-pr[1] + 1.0) * 0.5 * (a.H - 1);
                const double fx = floor(ix), fy = floor(iy);
                const int x0 = (int)fx, y0 = (int)fy;               // in frame: 0 <= ix <= W - 1
                const float tx = (float)(ix - fx), ty = (float)(iy - fy);
                t.w[0] = (1.0f - tx) * (1.0f - ty); t.w[1] = tx * (1.0f - ty); t.w[2] = (1.0f - tx) * ty; t.w[3] = tx * ty;
                const bool xa = x0 >= 0 && x0 < a.W, xb = x0 + 1 >= 0 && x0 + 1 < a.W;
                const bool ya = y0 >= 0 && y0 < a.H, yb = y0 + 1 >= 0 && y0 + 1 < a.H;
                t.ok = 16 | (xa && ya ? 1 : 0) | (xb && ya ? 2 : 0) | (xa && yb ? 4 : 0) | (xb && yb ? 8 : 0);      // 16: the view counts
                t.base = v * sv + (long long)y0 * sr + (long long)x0 * sw;
            }
        }
        taps[q] = t;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < LF_VB * a.C; q += blockDim.x) {
        const int j = q / a.C, c = q % a.C, i = i_first + j;
        if (i >= a.N) break;
        float sum = 0.0f;
        int cnt = 0;
        for (int v = 0; v < a.Vw; ++v) {
            const lf_tap& t = taps[j * a.Vw + v];
            if (!t.ok) continue;
            ++cnt;
            const TM* p = map + t.base + c * sc;
            float val = 0.0f;                                       // taps in the order nw, ne, sw, se; one outside the image adds nothing
            if (t.ok & 1) val = t.w[0] * lf_load(p);
            if (t.ok & 2) val = fmaf(t.w[1], lf_load(p + sw), val);
            if (t.ok & 4) val = fmaf(t.w[2], lf_load(p + sr), val);
            if (t.ok & 8) val = fmaf(t.w[3], lf_load(p + sr + sw), val);
            sum += val;
        }
        a.out[((size_t)b * a.N + i) * a.ldo + c] = cnt ? sum / (float)cnt : 0.0f;
        if (c == 0 && a.count) a.count[(size_t)b * a.N + i] = cnt;
    }
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int dm_raster_pix2face(dm_ctx* ctx, int B, int N, int nt, int Vw, int H, int W, const double* verts, const int32_t* tri,
                                  const int32_t* n_verts /*nullable*/, const double* R, const double* T, const int32_t* n_views /*nullable*/,
                                  double focal, const int32_t* given /*nullable*/, double* proj, int32_t* pix2face, unsigned char* vis) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && nt > 0 && Vw > 0 && B <= 65535 && Vw <= 65535, "sizes must be positive, B, views <= 65535");
    DM_REQUIRE(ctx, H > 0 && H == W && H <= 16384, "square images up to 16384 x 16384");
    DM_REQUIRE(ctx, verts && tri && R && T && proj && pix2face && vis, "null pointer");
    DM_REQUIRE(ctx, focal > 0.0 && focal < 1e300, "the focal length must be positive and finite");
    const long long n_items = (long long)B * Vw * nt;
    DM_REQUIRE(ctx, n_items / 4 + 1 < (1ll << 31) && (long long)B * Vw * N < (1ll << 40), "too many (mesh, view, face) items for one launch");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_pix = (size_t)B * Vw * H * W;
    if (int rc = dm_ws_reserve(ctx, dm_align_up(n_pix * sizeof(unsigned long long)))) return rc;
    unsigned long long* keys = (unsigned long long*)dm_ws_take(ctx, n_pix * sizeof(unsigned long long));
    if (!keys) return dm_fail(ctx, DM_ENOMEM, "dm_raster_pix2face: the key image does not fit the workspace");
    DM_CHECK_HIP(ctx, hipMemsetAsync(keys, 0xff, n_pix * sizeof(unsigned long long), ctx->stream));
    DM_CHECK_HIP(ctx, hipMemsetAsync(vis, 0, (size_t)B * Vw * N, ctx->stream));
    DM_LAUNCH(ctx, "lift_project", lift_project_kernel, dim3(dm_cdiv(N, 256), Vw, B), dim3(256), 0, N, Vw, verts, n_verts, R, T, n_views, focal, proj);
    face_args a{N, nt, Vw, H, W, tri, n_verts, n_views, given, proj, keys};
    DM_LAUNCH(ctx, "lift_faces", lift_faces_kernel, dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, a, n_items);
    DM_LAUNCH(ctx, "lift_resolve", lift_resolve_kernel, dim3(dm_cdiv(H * W, 256), Vw, B), dim3(256), 0, a, pix2face, vis);
    return DM_OK;
}

extern "C" int dm_lift_features(dm_ctx* ctx, int B, int N, int Vw, int C, int H, int W, int f_dtype, const long long* maps,
                                const double* proj, const unsigned char* vis, const int32_t* n_verts /*nullable*/,
                                const int32_t* n_views /*nullable*/, float* out, int ldo, int32_t* count /*nullable*/) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && Vw > 0 && C > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, Vw <= LF_VIEWS_MAX, "at most 64 views per mesh");
    DM_REQUIRE(ctx, H > 0 && H == W && H <= 16384, "square maps up to 16384 x 16384");
    DM_REQUIRE(ctx, f_dtype == DM_F16 || f_dtype == DM_F32, "f_dtype: DM_F16 or DM_F32");
    DM_REQUIRE(ctx, maps && proj && vis && out, "null pointer");
    DM_REQUIRE(ctx, ldo >= C && (long long)LF_VB * C < (1ll << 31), "ldo >= C");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    lift_args a{N, Vw, C, H, W, maps, proj, vis, n_verts, n_views, out, ldo, count};
    const dim3 grid(dm_cdiv(N, LF_VB), B);
    if (f_dtype == DM_F16)
        DM_LAUNCH(ctx, "lift_features", lift_features_kernel<__half>, grid, dim3(256), 0, a);
    else
        DM_LAUNCH(ctx, "lift_features", lift_features_kernel<float>, grid, dim3(256), 0, a);
    return DM_OK;
}

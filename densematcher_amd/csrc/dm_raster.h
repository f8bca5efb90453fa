// The raster core shared by multi-view lifting (dm_lift.hip) and textured-mesh rendering (dm_render.hip): the projection of a padded
// batch of meshes into all their views and the key-image pass.  The rule is densematch.h's ('multi-view feature lifting').
//
// Raster: the nearest face per pixel is a MINIMUM over 64-bit keys (fp32 bits of the depth << 32 | face), taken with one integer
// atomic per covered (face, pixel): the result does not depend on the order of faces, wavefronts or workgroups, and equal depths go
// to the lowest face index.  All memory operations are vector loads, stores and atomics.
#pragma once
#include <math.h>

#include "dm_internal.h"

namespace {
constexpr double RS_Z_MIN = 1e-6;   // a face with a vertex at Z <= this is skipped
constexpr double RS_AREA_MIN = 1e-8;
constexpr unsigned long long RS_EMPTY = ~0ull;

// a mesh's count of vertices / views, kept inside the padded size whatever the array holds
__device__ __forceinline__ int lf_count(const int32_t* a, int b, int dflt) { return a ? min(max(a[b], 0), dflt) : dflt; }

// ---------------------------------------------------------------------------------------------------------------- projection
// proj[b][view][i] = (x, y, Z, in-frame ? 1 : 0) of vertex i: X_view = X_world R + T (row vectors), x = f X / Z, y = f Y / Z
__global__ void __launch_bounds__(256) lift_project_kernel(int N, int Vw, const double* __restrict__ verts, const int32_t* __restrict__ n_verts,
                                                           const double* __restrict__ R, const double* __restrict__ T,
                                                           const int32_t* __restrict__ n_views, double focal, double* __restrict__ proj) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, v = blockIdx.y, b = blockIdx.z;
    if (i >= N) return;
    double* o = proj + (((size_t)b * Vw + v) * N + i) * 4;
    if (i >= lf_count(n_verts, b, N) || v >= lf_count(n_views, b, Vw)) {
        o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0;
        return;
    }
    const double* p = verts + ((size_t)b * N + i) * 3;
    const double* r = R + ((size_t)b * Vw + v) * 9;
    const double* t = T + ((size_t)b * Vw + v) * 3;
    const double X = p[0] * r[0] + p[1] * r[3] + p[2] * r[6] + t[0];
    const double Y = p[0] * r[1] + p[1] * r[4] + p[2] * r[7] + t[1];
    const double Z = p[0] * r[2] + p[1] * r[5] + p[2] * r[8] + t[2];
    const double x = focal * X / Z, y = focal * Y / Z;
    o[0] = x; o[1] = y; o[2] = Z;
    o[3] = (x > -1.0 && x < 1.0 && y > -1.0 && y < 1.0) ? 1.0 : 0.0;      // (NaN fails every comparison)
}

// ---------------------------------------------------------------------------------------------------------------- faces
struct face_args {
    int N, nt, Vw, H, W;
    const int32_t* tri; const int32_t* n_verts; const int32_t* n_views; const int32_t* given;
    const double* proj; unsigned long long* keys;
};

// one wavefront per (mesh, view, face): the lanes stride over the face's pixel box, clamped to the image
__global__ void __launch_bounds__(256) lift_faces_kernel(face_args a, long long n_items) {
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const int f = (int)(item % a.nt);
    const int v = (int)((item / a.nt) % a.Vw), b = (int)(item / ((long long)a.nt * a.Vw));
    if (v >= lf_count(a.n_views, b, a.Vw) || (a.given && a.given[b])) return;
    const int nv = lf_count(a.n_verts, b, a.N);
    const int32_t* t = a.tri + ((size_t)b * a.nt + f) * 3;
    const int i0 = t[0], i1 = t[1], i2 = t[2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return;
    const double* pr = a.proj + ((size_t)b * a.Vw + v) * a.N * 4;
    const double x0 = pr[4 * i0], y0 = pr[4 * i0 + 1], Z0 = pr[4 * i0 + 2];
    const double x1 = pr[4 * i1], y1 = pr[4 * i1 + 1], Z1 = pr[4 * i1 + 2];
    const double x2 = pr[4 * i2], y2 = pr[4 * i2 + 1], Z2 = pr[4 * i2 + 2];
    if (!(Z0 > RS_Z_MIN && Z1 > RS_Z_MIN && Z2 > RS_Z_MIN)) return;
    if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2))) return;
    const double area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0);
    if (!(fabs(area) > RS_AREA_MIN) || !isfinite(area)) return;
    // pixel centres: x_c = 1 - (2c + 1) / W, so column c = ((1 - x) W - 1) / 2; one pixel of slack on each side, clamped as doubles
    const double xmin = fmin(x0, fmin(x1, x2)), xmax = fmax(x0, fmax(x1, x2));
    const double ymin = fmin(y0, fmin(y1, y2)), ymax = fmax(y0, fmax(y1, y2));
    const double cl = fmax(0.0, floor(((1.0 - xmax) * a.W - 1.0) * 0.5) - 1.0), ch = fmin((double)(a.W - 1), ceil(((1.0 - xmin) * a.W - 1.0) * 0.5) + 1.0);
    const double rl = fmax(0.0, floor(((1.0 - ymax) * a.H - 1.0) * 0.5) - 1.0), rh = fmin((double)(a.H - 1), ceil(((1.0 - ymin) * a.H - 1.0) * 0.5) + 1.0);
    if (!(cl <= ch && rl <= rh)) return;
    const int c_lo = (int)cl, r_lo = (int)rl, bw = (int)ch - c_lo + 1, bh = (int)rh - r_lo + 1;
    const int npix = bw * bh;                                       // <= H W <= 2^28
    unsigned long long* keys = a.keys + ((size_t)b * a.Vw + v) * a.H * a.W;
    const double iZ0 = 1.0 / Z0, iZ1 = 1.0 / Z1, iZ2 = 1.0 / Z2;
    for (int p = lane; p < npix; p += 64) {
        const int r = r_lo + p / bw, c = c_lo + p % bw;
        const double px = 1.0 - (double)(2 * c + 1) / a.W, py = 1.0 - (double)(2 * r + 1) / a.H;
        const double w0 = (px - x1) * (y2 - y1) - (py - y1) * (x2 - x1);
        const double w1 = (px - x2) * (y0 - y2) - (py - y2) * (x0 - x2);
        const double w2 = (px - x0) * (y1 - y0) - (py - y0) * (x1 - x0);
        const double b0 = w0 / area, b1 = w1 / area, b2 = w2 / area;
        if (!(b0 > 0.0 && b1 > 0.0 && b2 > 0.0)) continue;
        const float z = (float)(1.0 / (b0 * iZ0 + b1 * iZ1 + b2 * iZ2));
        if (!(z > 0.0f)) continue;                                  // (positive floats order as their bit patterns)
        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned int)f;
        atomicMin(&keys[(size_t)r * a.W + c], key);
    }
}
}  // namespace

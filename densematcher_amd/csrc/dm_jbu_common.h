// What the forward (dm_jbu.hip) and the backward (dm_jbu_bwd.hip) of the JBU apply share: the sizes of the 7 x 7 kernel, the bicubic
// weights and clamped taps of the exact 2x upsampling, the reflection, and loads / stores of fp16 | fp32 elements.
#pragma once

#include <hip/hip_fp16.h>

#include "dm_internal.h"

namespace {
constexpr int JB_T = 49;            // taps of the 7 x 7 kernel
constexpr int JB_R = 3;             // radius

// bicubic weights (A = -0.75) of the two phases of an exact 2x upsampling with align_corners=False: the source coordinate of output
// u is u / 2 - 0.25; u odd: t = 0.25 on taps k-1 .. k+2 (k = u >> 1); u even: t = 0.75 on taps k-2 .. k+1.  All exact in binary.
constexpr float BC_A = -0.10546875f, BC_B = 0.87890625f, BC_C = 0.26171875f, BC_D = -0.03515625f;

__device__ __forceinline__ int jb_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }    // |i| excess < n
__device__ __forceinline__ float jb_load(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float jb_load(const float* p) { return *p; }
__device__ __forceinline__ void jb_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void jb_store(__half* p, float v) { *p = __float2half_rn(v); }

// the four source taps and weights of upsampled index u (0 <= u < 2 n), clamped to [0, n)
__device__ __forceinline__ void jb_taps(int u, int n, int* tap, float* wt) {
    const int k = u >> 1, first = (u & 1) ? k - 1 : k - 2;
#pragma unroll
    for (int q = 0; q < 4; ++q) tap[q] = min(max(first + q, 0), n - 1);
    if (u & 1) { wt[0] = BC_A; wt[1] = BC_B; wt[2] = BC_C; wt[3] = BC_D; }
    else { wt[0] = BC_D; wt[1] = BC_C; wt[2] = BC_B; wt[3] = BC_A; }
}
}  // namespace

// The (value, lowest index) arg-max key of the farthest-point samplers (dm_fps.hip, dm_graphgeod.hip): a total order, so the result does
// not depend on how the reduction is arranged.  Through the wave by DPP (quad_perm, row_half_mirror, row_mirror, then two lane
// exchanges across the rows), across the (up to 16) waves through one LDS slot per wave, double-buffered by the parity of the step.
#pragma once

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ void fps_better(double& v, int& i, double ov, int oi) {
    const bool take = (ov > v) || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
}
template <int CTRL>
__device__ __forceinline__ void fps_dpp_step(double& v, int& i) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    const int oi = __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false);
    fps_better(v, i, __hiloint2double(ohi, olo), oi);
}
// every lane of a row of 16 ends with the row's best key
__device__ __forceinline__ void fps_row_best(double& v, int& i) {
    fps_dpp_step<0xB1>(v, i);          // quad_perm [1, 0, 3, 2]
    fps_dpp_step<0x4E>(v, i);          // quad_perm [2, 3, 0, 1]
    fps_dpp_step<0x141>(v, i);         // row_half_mirror
    fps_dpp_step<0x140>(v, i);         // row_mirror
}
// the best key of the workgroup, in every thread.  sv / si: 2 x 16 slots; par = parity of the step.  All threads call it.
__device__ __forceinline__ int fps_block_argmax(double v, int i, double* sv, int* si, int par) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    fps_row_best(v, i);
    fps_better(v, i, __shfl_xor(v, 16), __shfl_xor(i, 16));
    fps_better(v, i, __shfl_xor(v, 32), __shfl_xor(i, 32));
    if (lane == 0) { sv[par * 16 + wave] = v; si[par * 16 + wave] = i; }
    __syncthreads();
    const int q = lane & 15;
    v = q < nw ? sv[par * 16 + q] : -2.0;
    i = q < nw ? si[par * 16 + q] : 0x7fffffff;
    fps_row_best(v, i);
    return i;
}

}  // namespace

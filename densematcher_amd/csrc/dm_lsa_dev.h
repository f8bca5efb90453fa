// Device helpers shared by the assignment kernels (dm_assign.hip, dm_lsa_gather.hip): the scan and tie rules of SciPy's
// shortest-augmenting-path search and the wave reductions of a search step.
#pragma once
#include "dm_device.h"

struct lsa_cand { double val; int sink; int it; };      // sink: 1 when the column is unassigned
// the sequential scan's choice among two candidates (it = position in the scan)
__device__ __forceinline__ lsa_cand lsa_better(const lsa_cand& a, const lsa_cand& b) {
    if (a.it < 0) return b;
    if (b.it < 0) return a;
    if (a.val != b.val) return (a.val < b.val) ? a : b;
    if (a.sink != b.sink) return a.sink ? a : b;
    if (a.sink) return (a.it > b.it) ? a : b;           // every later unassigned column of equal cost replaces the choice
    return (a.it < b.it) ? a : b;                       // else the first in scan order is kept
}

// the same rule on separate scalars (a struct passed by value ended up in scratch memory: a memory round trip per merge):
// (v, sk, it, j) <- the better of itself and (ov, osk, oit, oj)
__device__ __forceinline__ void lsa_merge(double& v, int& sk, int& it, int& j, double ov, int osk, int oit, int oj) {
    bool take;
    if (it < 0) take = true;
    else if (oit < 0) take = false;
    else if (v != ov) take = ov < v;
    else if (sk != osk) take = osk != 0;
    else if (sk) take = oit > it;
    else take = oit < it;
    v = take ? ov : v; sk = take ? osk : sk; it = take ? oit : it; j = take ? oj : j;
}

// the same rule with (sink, it, column) folded into ONE integer that orders the candidates of equal cost: an unassigned
// column beats an assigned one, among unassigned ones the LAST in scan order wins, among assigned ones the FIRST:
//   key = ((sink ? 8192 + it : 8191 - it) << 14) | column      (it, column < 8192: nc <= 8192 on this path);  -1 = no candidate
//   better = smaller cost, then larger key  (positions are distinct, so the column bits never decide)
// -- two comparisons per merge instead of five, and three shuffled words per butterfly level instead of five
__device__ __forceinline__ int lsa_key(int sink, int it, int j) { return ((sink ? 8192 + it : 8191 - it) << 14) | j; }
// Reductions inside a wave on the vector ALU (DPP), in TWO phases: the smallest cost first, then the largest key among the
// lanes that hold it -- one v_min_f64 / v_max_i32 per level and no divergent branch (a merged (cost, key) compare costs five
// times that).  Levels: lanes i ^ 1, i ^ 2 (quad permutes), 7 - i within 8 (row_half_mirror), 15 - i within 16 (row_mirror)
// leave every lane of a row of 16 with the row's result; row_bcast:15 into rows 1, 3 and row_bcast:31 into rows 2, 3 carry
// it to lane 63, which a readlane hands to the scalar unit.
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ int lsa_dpp(int x) {
    if constexpr (ROWS == 0xf) return __builtin_amdgcn_mov_dpp(x, CTRL, 0xf, 0xf, false);      // (every lane has a source)
    else return __builtin_amdgcn_update_dpp(x, x, CTRL, ROWS, 0xf, false);                      // rows outside the mask keep x
}
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ double lsa_min_dpp(double v) {                                     // (costs are never NaN)
    return __builtin_fmin(v, __hiloint2double(lsa_dpp<CTRL, ROWS>(__double2hiint(v)), lsa_dpp<CTRL, ROWS>(__double2loint(v))));
}
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ int lsa_max_dpp(int k) { const int o = lsa_dpp<CTRL, ROWS>(k); return o > k ? o : k; }
__device__ __forceinline__ double lsa_wave_min(double v) {          // uniform result
    v = lsa_min_dpp<0xB1>(v); v = lsa_min_dpp<0x4E>(v); v = lsa_min_dpp<0x141>(v); v = lsa_min_dpp<0x140>(v);
    v = lsa_min_dpp<0x142, 0xa>(v); v = lsa_min_dpp<0x143, 0xc>(v);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ int lsa_wave_max(int k) {                // uniform result
    k = lsa_max_dpp<0xB1>(k); k = lsa_max_dpp<0x4E>(k); k = lsa_max_dpp<0x141>(k); k = lsa_max_dpp<0x140>(k);
    k = lsa_max_dpp<0x142, 0xa>(k); k = lsa_max_dpp<0x143, 0xc>(k);
    return __builtin_amdgcn_readlane(k, 63);
}

// DiffusionNet forward pass (inference) for a halved module, fp16 operands on the matrix cores: dm_dnet_linear_f16, dm_dnet_diffuse_f16,
// dm_dnet_gradfeat_f16.  The fp32 kernels of dm_dnet_layers.hip are not touched; this file shares no code with them or with dm_vit.hip
// (the main loop of the linear is vit_linear_kernel's, instantiated here on its own so that the encoder's bits cannot move).
//
// Reference computation replaced: diffusion_net/layers.py as dm_dnet_layers.hip lists it, run as the reference's driver runs it
// (model.half() under torch.autocast("cuda")).
//
// Every product is v_mfma_f32_32x32x16_f16: exact fp16 x fp16 products accumulated in fp32, the contraction index in ascending chunks of
// 16 from a zero accumulator, never split, no atomics.  Lane (r = lane & 31, h = lane >> 5) of a step holds A[row r][k = 8 h + j] and
// B[k = 8 h + j][col r], j = 0 .. 7; accumulator register `reg` is row (reg & 3) + 8 (reg >> 2) + 4 h, column r.  Tiles start at
// multiples of 32 rows and columns and every tile walks the same chunks, so an output element's bits depend on its own row and column of
// the operands only: not on the tile shape, the other meshes of the call or the padding (operands beyond a mesh's rows, a matrix's
// columns or an ELL row's slots are staged as zeros).
//
// Roundings to fp16 (round to nearest even; a magnitude beyond 65504 becomes infinite, as in the reference's half route):
//   linear    each fp32 source element as it is staged; the output when out_dtype is DM_F16 (the fp32 value rounded once more).
//   diffuse   x as it is staged; d = coef * spectrum, once, from the exact float64 product.
//   gradfeat  gX and gY as operands of the products with A_re / A_im (the elementwise product takes the fp32 values).
// Loads are 16-byte vectors where the address allows it and scalar otherwise: no operand needs an alignment beyond its element's.
#include <math.h>

#include <hip/hip_fp16.h>

#include "dm_dnet_common.h"

typedef float dh_f32x16 __attribute__((ext_vector_type(16)));
typedef float dh_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 dh_f16x8 __attribute__((ext_vector_type(8)));

namespace {
constexpr int DH_KC = 64, DH_LD = DH_KC + 8;     // linear: contraction stage, LDS row in halves
constexpr int DH_BIG_TILES = 256;                // linear, gradfeat: the larger decomposition once its workgroups fill every CU
constexpr int DH_CT = 32;                        // diffuse: channels per workgroup
constexpr int DH_KG = 128;                       // diffuse: spectrum rows per sweep over the vertices (32 per wave)
constexpr int DH_VC = 64, DH_VLD = DH_VC + 8;    // diffuse: vertices per stage of the first product, LDS row in halves
constexpr int DH_VT = 128;                       // diffuse: vertices per tile of the product back (32 per wave)
constexpr int DH_KMAX = 1024;                    // diffuse: largest K whose 32 x K spectrum fits in LDS next to the stages
constexpr int DH_T = 64;                         // gradfeat: outputs per workgroup side
constexpr int DH_GK = 32, DH_GLD = DH_GK + 8;    // gradfeat: contraction stage, LDS row in halves
constexpr int DH_ELL_MAX = 64;                   // gradfeat: widest ELL rows kept in LDS
constexpr int DH_RR = 32, DH_RC = 128;           // gradfeat with resident gradients: rows per workgroup, columns per pass
constexpr int DH_RK = 64, DH_RLD = DH_RK + 8;    // gradfeat with resident gradients: contraction stage of the matrices, LDS row in halves
constexpr size_t DH_LDS_MAX = 160 * 1024;        // LDS of a CU

__device__ __forceinline__ int dh_nv(const int32_t* nv, int b, int N) { return nv ? nv[b] : N; }
__device__ __forceinline__ int dh_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
__device__ __forceinline__ bool dh_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ dh_f16x8 dh_zero8() { const dh_f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0}; return z; }

// n <= 8 adjacent halves from p (2-byte aligned), zeros behind them
__device__ __forceinline__ dh_f16x8 dh_load_h(const _Float16* p, int n) {
    if (n >= 8 && dh_al16(p)) return *reinterpret_cast<const dh_f16x8*>(p);
    dh_f16x8 v = dh_zero8();
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < n) v[j] = p[j];
    return v;
}

// n <= 8 adjacent floats from p, each rounded to fp16, zeros behind them
__device__ __forceinline__ dh_f16x8 dh_load_f(const float* p, int n) {
    dh_f16x8 v = dh_zero8();
    if (n >= 8 && dh_al16(p)) {
        const dh_f32x4 lo = *reinterpret_cast<const dh_f32x4*>(p), hi = *reinterpret_cast<const dh_f32x4*>(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = (_Float16)lo[j]; v[4 + j] = (_Float16)hi[j]; }
        return v;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < n) v[j] = (_Float16)p[j];
    return v;
}

// one rounding of a double to fp16: to fp32 with round-to-odd (the sticky bit tells the second rounding on which side of a tie the
// value lies), then to nearest even
__device__ __forceinline__ _Float16 dh_round_f16(double p) {
    float f = (float)p;
    const double d = (double)f;
    if (d != p) {
        unsigned u = __float_as_uint(f);
        if (!(u & 1u)) u = fabs(d) < fabs(p) ? u + 1u : u - 1u;
        f = __uint_as_float(u);
    }
    return (_Float16)f;
}

// ---------------------------------------------------------------------------------------------------------------- linear
struct hl_args {
    int N, Cout, Ktot;
    const void* src[3]; int w[3]; int ld[3]; int f16[3];
    const _Float16* W; int ldw;
    const void* bias; int bias_f16; const float* resid; int ldr; int act;
    const int32_t* nv; void* out; int out_f16; int ldo;
};

// columns k .. k + 7 of row `brow` of the concatenation, rounded to fp16; columns >= Ktot are zeros
__device__ __forceinline__ dh_f16x8 hl_load_src(const hl_args& a, long long brow, int k) {
    if (k >= a.Ktot) return dh_zero8();
    int s = 0, kl = k;
    if (kl >= a.w[0]) { kl -= a.w[0]; s = 1; if (kl >= a.w[1]) { kl -= a.w[1]; s = 2; } }
    const int ws = s == 0 ? a.w[0] : (s == 1 ? a.w[1] : a.w[2]);
    if (kl + 8 <= ws || k + (ws - kl) >= a.Ktot) {          // the eight columns lie in one source, or it is the last one
        const void* sp = s == 0 ? a.src[0] : (s == 1 ? a.src[1] : a.src[2]);
        const long long ld = s == 0 ? a.ld[0] : (s == 1 ? a.ld[1] : a.ld[2]);
        const int half = s == 0 ? a.f16[0] : (s == 1 ? a.f16[1] : a.f16[2]);
        const int n = min(8, ws - kl);
        return half ? dh_load_h(reinterpret_cast<const _Float16*>(sp) + brow * ld + kl, n)
                    : dh_load_f(reinterpret_cast<const float*>(sp) + brow * ld + kl, n);
    }
    dh_f16x8 v = dh_zero8();                                 // the eight columns straddle two or three sources
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int q = k + j, sj = 0;
        if (q >= a.Ktot) continue;
        if (q >= a.w[0]) { q -= a.w[0]; sj = 1; if (q >= a.w[1]) { q -= a.w[1]; sj = 2; } }
        const void* sp = sj == 0 ? a.src[0] : (sj == 1 ? a.src[1] : a.src[2]);
        const long long ld = sj == 0 ? a.ld[0] : (sj == 1 ? a.ld[1] : a.ld[2]);
        const int half = sj == 0 ? a.f16[0] : (sj == 1 ? a.f16[1] : a.f16[2]);
        v[j] = half ? reinterpret_cast<const _Float16*>(sp)[brow * ld + q] : (_Float16)reinterpret_cast<const float*>(sp)[brow * ld + q];
    }
    return v;
}

// MI x MI accumulator blocks per wave, 2 x 2 waves: 64 MI x 64 MI outputs per workgroup
template <int MI>
__global__ void __launch_bounds__(256) dnet_linear_f16_kernel(hl_args a) {
    constexpr int BT = 64 * MI, NI = 2 * MI;
    __shared__ __attribute__((aligned(16))) _Float16 As[BT * DH_LD], Bs[BT * DH_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;
    const int b = blockIdx.z, row0 = blockIdx.y * BT, col0 = blockIdx.x * BT;
    const int nvb = dh_nv(a.nv, b, a.N);
    const long long bN = (long long)b * a.N;
    // a thread stages the halves kq .. kq + 7 of the rows sr + 32 i of both tiles
    const int sr = t >> 3, kq = (t & 7) * 8;
    dh_f16x8 ra[NI], rb[NI];
    auto fetch = [&](int k0) {
        const int k = k0 + kq;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int gr = row0 + sr + 32 * i, gc = col0 + sr + 32 * i;
            ra[i] = gr < nvb ? hl_load_src(a, bN + gr, k) : dh_zero8();
            rb[i] = (gc < a.Cout && k < a.Ktot) ? dh_load_h(a.W + (long long)gc * a.ldw + k, min(8, a.Ktot - k)) : dh_zero8();
        }
    };
    dh_f32x16 acc[MI][MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    fetch(0);
    for (int k0 = 0; k0 < a.Ktot; k0 += DH_KC) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            *reinterpret_cast<dh_f16x8*>(&As[(sr + 32 * i) * DH_LD + kq]) = ra[i];
            *reinterpret_cast<dh_f16x8*>(&Bs[(sr + 32 * i) * DH_LD + kq]) = rb[i];
        }
        __syncthreads();
        if (k0 + DH_KC < a.Ktot) fetch(k0 + DH_KC);
#pragma unroll
        for (int s = 0; s < DH_KC / 16; ++s) {
            dh_f16x8 fa[MI], fb[MI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                fa[i] = *reinterpret_cast<const dh_f16x8*>(&As[(32 * MI * wr + 32 * i + r) * DH_LD + 16 * s + 8 * h]);
                fb[i] = *reinterpret_cast<const dh_f16x8*>(&Bs[(32 * MI * wc + 32 * i + r) * DH_LD + 16 * s + 8 * h]);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // epilogue: + bias, act, + resid, each rounded on its own; rows behind the mesh's count are zeros
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const int col = col0 + 32 * MI * wc + 32 * j + r;
        if (col >= a.Cout) continue;
        float bv = 0.0f;
        if (a.bias) bv = a.bias_f16 ? (float)reinterpret_cast<const _Float16*>(a.bias)[col] : reinterpret_cast<const float*>(a.bias)[col];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = row0 + 32 * MI * wr + 32 * i + dh_row(reg, h);
                if (row >= a.N) continue;
                const long long brow = bN + row;
                float v = 0.0f;
                if (row < nvb) {
                    v = __fadd_rn(acc[i][j][reg], bv);
                    if (a.act) v = fmaxf(v, 0.0f);
                    if (a.resid) v = __fadd_rn(v, a.resid[brow * a.ldr + col]);
                }
                if (a.out_f16) reinterpret_cast<_Float16*>(a.out)[brow * a.ldo + col] = (_Float16)v;
                else reinterpret_cast<float*>(a.out)[brow * a.ldo + col] = v;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- diffuse
struct hd_args {
    int N, K, C, Kpad;
    const float* x; int ldx;
    const _Float16* eh; int lde; const _Float16* mh; int ldm; const int32_t* e1; const int32_t* e2;
    const float* evals; const void* times; int times_f16;
    const int32_t* nv; float* out; int ldo;
};

// With E = 2^e1 evecs and M = 2^e2 mass * evecs in fp16: acc1 = M^T fp16(x) = 2^e2 spectrum.  The spectrum goes on at the scale of the
// product back, d = fp16(coef * acc1 * 2^(14 - e1 - e2)) (about max |evecs| times the spectrum: scaling evecs by s and mass by s^-2
// moves no bit of it), so that out = 2^-14 (E d).  Both scalings are by powers of two.
__global__ void __launch_bounds__(256) dnet_diffuse_f16_kernel(hd_args a) {
    extern __shared__ __attribute__((aligned(16))) _Float16 dh_lds[];
    const int ldd = a.Kpad + 8;
    _Float16* Ds = dh_lds;                                  // [32 channels][Kpad + 8]: d transposed, the B operand of the product back
    _Float16* Ms = Ds + DH_CT * ldd;                        // [128 k][64 + 8 vertices]
    _Float16* Xs = Ms + DH_KG * DH_VLD;                     // [32 channels][64 + 8 vertices]
    const int b = blockIdx.y, c0 = blockIdx.x * DH_CT;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int nvb = dh_nv(a.nv, b, a.N);
    const long long bN = (long long)b * a.N;
    const double scale = ldexp(1.0, 14 - a.e1[b] - a.e2[b]);
    // ---- the spectrum, 128 rows of it per sweep over the vertices in ascending order
    const int xv = t >> 2, xc = (t & 3) * 8;
    for (int kg = 0; kg < a.Kpad; kg += DH_KG) {
        dh_f16x8 rm[4], rx;
        auto fetch = [&](int v0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = t + 256 * i, v = v0 + (e >> 4), k = kg + (e & 15) * 8;
                rm[i] = (v < nvb && k < a.K) ? dh_load_h(a.mh + (bN + v) * a.ldm + k, min(8, a.K - k)) : dh_zero8();
            }
            const int v = v0 + xv, c = c0 + xc;
            rx = (v < nvb && c < a.C) ? dh_load_f(a.x + (bN + v) * a.ldx + c, min(8, a.C - c)) : dh_zero8();
        };
        dh_f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        const bool live = kg + 32 * wave < a.Kpad;
        fetch(0);
        for (int v0 = 0; v0 < nvb; v0 += DH_VC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = t + 256 * i, v = e >> 4, kq = (e & 15) * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) Ms[(kq + j) * DH_VLD + v] = rm[i][j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) Xs[(xc + j) * DH_VLD + xv] = rx[j];
            __syncthreads();
            if (v0 + DH_VC < nvb) fetch(v0 + DH_VC);
            if (live) {
#pragma unroll
                for (int s = 0; s < DH_VC / 16; ++s) {
                    const dh_f16x8 fa = *reinterpret_cast<const dh_f16x8*>(&Ms[(32 * wave + r) * DH_VLD + 16 * s + 8 * h]);
                    const dh_f16x8 fb = *reinterpret_cast<const dh_f16x8*>(&Xs[r * DH_VLD + 16 * s + 8 * h]);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc, 0, 0, 0);
                }
            }
            __syncthreads();
        }
        if (live) {
            const int c = c0 + r;
            // the reference clamps the times in fp32 (torch.clamp(diffusion_time, min=1e-8)); the exponent and exp() are float64
            float tm = 0.0f;
            if (c < a.C) tm = a.times_f16 ? (float)reinterpret_cast<const _Float16*>(a.times)[c] : reinterpret_cast<const float*>(a.times)[c];
            const double tc = (double)fmaxf(tm, 1e-8f);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int k = kg + 32 * wave + dh_row(reg, h);
                _Float16 d = (_Float16)0.0f;
                if (k < a.K && c < a.C) {
                    const float coef = (float)exp(-(double)a.evals[(long long)b * a.K + k] * tc);
                    d = dh_round_f16((double)coef * (double)acc[reg] * scale);
                }
                Ds[r * ldd + k] = d;
            }
        }
    }
    __syncthreads();
    // ---- the product back: a wave owns 32 vertices of a tile of 128 and reads its rows of E from memory (no other wave needs them)
    const int c = c0 + r;
    for (int vt = 0; vt < a.N; vt += DH_VT) {
        const int va = vt + 32 * wave + r;                  // the row of E this lane holds
        const _Float16* erow = a.eh + (bN + va) * a.lde;
        dh_f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        if (vt + 32 * wave < nvb) {                          // (uniform in the wave)
            for (int ks = 0; ks < a.Kpad; ks += 16) {
                const int k = ks + 8 * h;
                const dh_f16x8 fa = (va < nvb && k < a.K) ? dh_load_h(erow + k, min(8, a.K - k)) : dh_zero8();
                const dh_f16x8 fb = *reinterpret_cast<const dh_f16x8*>(&Ds[r * ldd + k]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc, 0, 0, 0);
            }
        }
        if (c < a.C) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int v = vt + 32 * wave + dh_row(reg, h);
                if (v < a.N) a.out[(bN + v) * a.ldo + c] = v < nvb ? __fmul_rn(acc[reg], 0x1p-14f) : 0.0f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- gradient features
struct hg_args {
    int N, C, nnz;
    const int32_t* row_len; const int32_t* cols; const float* gx; const float* gy;
    const float* x; int ldx; const _Float16* Are; const _Float16* Aim; int lda;
    const int32_t* nv; float* out; int ldo;
    int ell_lds;
};

// (G_x x)[row][ch], (G_y x)[row][ch] in fp32: the row's entries in stored order, one fmaf each (the chain of dm_dnet_gradfeat_f32)
__device__ __forceinline__ void hg_gather(const hg_args& a, int b, int row, int ch, int nvb, float& sx, float& sy) {
    const long long br = (long long)b * a.N + row;
    const int len = min(max(a.row_len[br], 0), a.nnz);
    const int32_t* cl = a.cols + br * a.nnz;
    const float* vx = a.gx + br * a.nnz;
    const float* vy = a.gy + br * a.nnz;
    const float* xb = a.x + (long long)b * a.N * a.ldx + ch;
    sx = 0.f; sy = 0.f;
    for (int q = 0; q < len; ++q) {
        const int c = cl[q];
        if ((unsigned)c >= (unsigned)nvb) continue;
        const float xv = xb[(long long)c * a.ldx];
        sx = fmaf(vx[q], xv, sx);
        sy = fmaf(vy[q], xv, sy);
    }
}

__device__ __forceinline__ void hg_gather_lds(const hg_args& a, const int32_t* ec, const float* ex, const float* ey, int len, const float* xb,
                                              float& sx, float& sy) {
    sx = 0.f; sy = 0.f;
    for (int q = 0; q < len; ++q) {
        const int c = ec[q];
        if (c < 0) continue;
        const float xv = xb[(long long)c * a.ldx];
        sx = fmaf(ex[q], xv, sx);
        sy = fmaf(ey[q], xv, sy);
    }
}

__global__ void __launch_bounds__(256) dnet_gradfeat_f16_kernel(hg_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hg_lds[];
    _Float16* Xs = reinterpret_cast<_Float16*>(hg_lds);    // [64 rows][32 + 8 channels] of fp16(gX); Ys alike; Rs, Is: [64 matrix rows][32 + 8]
    _Float16* Ys = Xs + DH_T * DH_GLD;
    _Float16* Rs = Ys + DH_T * DH_GLD;
    _Float16* Is = Rs + DH_T * DH_GLD;
    int32_t* El = reinterpret_cast<int32_t*>(Is + DH_T * DH_GLD);      // [64] entries of each row of the tile (0 behind the mesh's rows)
    int32_t* Ec = El + DH_T;                                           // [64][nnz] columns, then the two value planes (ell_lds only)
    float* Ex = reinterpret_cast<float*>(Ec + DH_T * a.nnz);
    float* Ey = Ex + DH_T * a.nnz;
    const int b = blockIdx.z, row0 = blockIdx.y * DH_T, col0 = blockIdx.x * DH_T;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int nvb = dh_nv(a.nv, b, a.N);
    const bool rot = a.Aim != nullptr;
    const int kk = t & 31, r8 = t >> 5;
    _Float16 rgx[8], rgy[8], rre[8], rim[8];
    unsigned rmask = 0, cmask = 0;                         // which of the rows / matrix rows r8 + 8 i this thread stages exist
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (row0 + r8 + 8 * i < nvb) rmask |= 1u << i;
        if (col0 + r8 + 8 * i < a.C) cmask |= 1u << i;
    }
    const long long arow0 = (long long)(col0 + r8) * a.lda, astep = 8LL * a.lda;
    const float* xmesh = a.x + (long long)b * a.N * a.ldx;
    if (a.ell_lds) {
        if (t < DH_T) El[t] = row0 + t < nvb ? min(max(a.row_len[(long long)b * a.N + row0 + t], 0), a.nnz) : 0;
        __syncthreads();
        for (int e = t; e < DH_T * a.nnz; e += 256) {
            const int rl = e / a.nnz, q = e - rl * a.nnz;
            int c = -1; float vx = 0.f, vy = 0.f;
            if (q < El[rl]) {
                const long long o = ((long long)b * a.N + row0 + rl) * a.nnz + q;
                c = a.cols[o];
                if ((unsigned)c >= (unsigned)nvb) c = -1;
                vx = a.gx[o]; vy = a.gy[o];
            }
            Ec[e] = c; Ex[e] = vx; Ey[e] = vy;
        }
        __syncthreads();
    }
    auto gather = [&](int rl, int ch, float& sx, float& sy) {          // row rl of the tile (inside the mesh), channel ch
        if (a.ell_lds) hg_gather_lds(a, Ec + rl * a.nnz, Ex + rl * a.nnz, Ey + rl * a.nnz, El[rl], xmesh + ch, sx, sy);
        else hg_gather(a, b, row0 + rl, ch, nvb, sx, sy);
    };
    auto fetch = [&](int k0) {
        const int k = k0 + kk;
        const bool kin = k < a.C;
        const long long ao = arow0 + k;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float sx = 0.f, sy = 0.f;
            if (kin && ((rmask >> i) & 1u)) gather(r8 + 8 * i, k, sx, sy);
            rgx[i] = (_Float16)sx; rgy[i] = (_Float16)sy;
            const bool in = kin && ((cmask >> i) & 1u);
            rre[i] = in ? a.Are[ao + i * astep] : (_Float16)0.0f;
            rim[i] = (in && rot) ? a.Aim[ao + i * astep] : (_Float16)0.0f;
        }
    };
    dh_f32x16 p1, p2, p3, p4;
#pragma unroll
    for (int e = 0; e < 16; ++e) p1[e] = p2[e] = p3[e] = p4[e] = 0.0f;
    fetch(0);
    for (int k0 = 0; k0 < a.C; k0 += DH_GK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = (r8 + 8 * i) * DH_GLD + kk;
            Xs[o] = rgx[i]; Ys[o] = rgy[i]; Rs[o] = rre[i]; Is[o] = rim[i];
        }
        __syncthreads();
        if (k0 + DH_GK < a.C) fetch(k0 + DH_GK);
#pragma unroll
        for (int s = 0; s < DH_GK / 16; ++s) {
            const int oa = (32 * wr + r) * DH_GLD + 16 * s + 8 * h, ob = (32 * wc + r) * DH_GLD + 16 * s + 8 * h;
            const dh_f16x8 ax = *reinterpret_cast<const dh_f16x8*>(&Xs[oa]), ay = *reinterpret_cast<const dh_f16x8*>(&Ys[oa]);
            const dh_f16x8 bre = *reinterpret_cast<const dh_f16x8*>(&Rs[ob]);
            p1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ax, bre, p1, 0, 0, 0);
            p3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ay, bre, p3, 0, 0, 0);
            if (rot) {
                const dh_f16x8 bim = *reinterpret_cast<const dh_f16x8*>(&Is[ob]);
                p2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ay, bim, p2, 0, 0, 0);
                p4 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ax, bim, p4, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    const int col = col0 + 32 * wc + r;
    if (col >= a.C) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = row0 + 32 * wr + dh_row(reg, h);
        if (row >= a.N) continue;
        float v = 0.f;
        if (row < nvb) {
            float sx, sy;
            gather(row - row0, col, sx, sy);
            const float bre = rot ? __fsub_rn(p1[reg], p2[reg]) : p1[reg];
            const float bim = rot ? __fadd_rn(p3[reg], p4[reg]) : p3[reg];
            v = tanhf(fmaf(sx, bre, __fmul_rn(sy, bim)));
        }
        a.out[((long long)b * a.N + row) * a.ldo + col] = v;
    }
}

// The same computation with the gradients of a row tile resident: a workgroup owns 32 rows and every column.  It gathers fp16(gX),
// fp16(gY) of its rows once for all C channels into LDS (the tile kernel above gathers them again for each of its C / 64 column tiles),
// then walks the columns 128 at a time (32 per wave) with the matrices staged 64 deep.  The gather chain, the chunks of 16 of the
// contraction index and the epilogue are those of the tile kernel: the bits are the same.  Cp: C rounded up to the stage depth.
__global__ void __launch_bounds__(256) dnet_gradfeat_f16_rows_kernel(hg_args a, int Cp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hg_lds[];
    const int ldg = Cp + 8;
    _Float16* Gx = reinterpret_cast<_Float16*>(hg_lds);    // [32 rows][Cp + 8] of fp16(gX); Gy alike
    _Float16* Gy = Gx + DH_RR * ldg;
    _Float16* Rs = Gy + DH_RR * ldg;                        // [128 matrix rows][64 + 8]; Is alike
    _Float16* Is = Rs + DH_RC * DH_RLD;
    int32_t* El = reinterpret_cast<int32_t*>(Is + DH_RC * DH_RLD);     // [32] entries of each row of the tile (0 behind the mesh's rows)
    int32_t* Ec = El + DH_RR;                                          // [32][nnz] columns, then the two value planes (ell_lds only)
    float* Ex = reinterpret_cast<float*>(Ec + DH_RR * a.nnz);
    float* Ey = Ex + DH_RR * a.nnz;
    const int b = blockIdx.y, row0 = blockIdx.x * DH_RR;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int nvb = dh_nv(a.nv, b, a.N);
    const bool rot = a.Aim != nullptr;
    const float* xmesh = a.x + (long long)b * a.N * a.ldx;
    if (a.ell_lds) {
        if (t < DH_RR) El[t] = row0 + t < nvb ? min(max(a.row_len[(long long)b * a.N + row0 + t], 0), a.nnz) : 0;
        __syncthreads();
        for (int e = t; e < DH_RR * a.nnz; e += 256) {
            const int rl = e / a.nnz, q = e - rl * a.nnz;
            int c = -1; float vx = 0.f, vy = 0.f;
            if (q < El[rl]) {
                const long long o = ((long long)b * a.N + row0 + rl) * a.nnz + q;
                c = a.cols[o];
                if ((unsigned)c >= (unsigned)nvb) c = -1;
                vx = a.gx[o]; vy = a.gy[o];
            }
            Ec[e] = c; Ex[e] = vx; Ey[e] = vy;
        }
        __syncthreads();
    }
    auto gather = [&](int rl, int ch, float& sx, float& sy) {          // row rl of the tile (inside the mesh), channel ch
        if (a.ell_lds) hg_gather_lds(a, Ec + rl * a.nnz, Ex + rl * a.nnz, Ey + rl * a.nnz, El[rl], xmesh + ch, sx, sy);
        else hg_gather(a, b, row0 + rl, ch, nvb, sx, sy);
    };
    // ---- the gradients of the tile, rounded once: a thread takes channel kk of the rows r8 + 8 i, 32 channels per step
    {
        const int kk = t & 31, r8 = t >> 5;
        for (int k0 = 0; k0 < Cp; k0 += 32) {
            const int ch = k0 + kk;
#pragma unroll
            for (int i = 0; i < DH_RR / 8; ++i) {
                const int rl = r8 + 8 * i;
                float sx = 0.f, sy = 0.f;
                if (ch < a.C && row0 + rl < nvb) gather(rl, ch, sx, sy);
                Gx[rl * ldg + ch] = (_Float16)sx;
                Gy[rl * ldg + ch] = (_Float16)sy;
            }
        }
    }
    __syncthreads();
    // ---- the four products, 128 columns per pass; a thread stages the halves kq .. kq + 7 of the matrix rows sr + 32 i
    const int sr = t >> 3, kq = (t & 7) * 8;
    for (int col0 = 0; col0 < a.C; col0 += DH_RC) {
        dh_f16x8 rre[4], rim[4];
        auto fetch = [&](int k0) {
            const int k = k0 + kq;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int gc = col0 + sr + 32 * i;
                const bool in = gc < a.C && k < a.C;
                rre[i] = in ? dh_load_h(a.Are + (long long)gc * a.lda + k, min(8, a.C - k)) : dh_zero8();
                rim[i] = (in && rot) ? dh_load_h(a.Aim + (long long)gc * a.lda + k, min(8, a.C - k)) : dh_zero8();
            }
        };
        dh_f32x16 p1, p2, p3, p4;
#pragma unroll
        for (int e = 0; e < 16; ++e) p1[e] = p2[e] = p3[e] = p4[e] = 0.0f;
        fetch(0);
        for (int k0 = 0; k0 < Cp; k0 += DH_RK) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<dh_f16x8*>(&Rs[(sr + 32 * i) * DH_RLD + kq]) = rre[i];
                *reinterpret_cast<dh_f16x8*>(&Is[(sr + 32 * i) * DH_RLD + kq]) = rim[i];
            }
            __syncthreads();
            if (k0 + DH_RK < Cp) fetch(k0 + DH_RK);
#pragma unroll
            for (int s = 0; s < DH_RK / 16; ++s) {
                const int oa = r * ldg + k0 + 16 * s + 8 * h, ob = (32 * wave + r) * DH_RLD + 16 * s + 8 * h;
                const dh_f16x8 ax = *reinterpret_cast<const dh_f16x8*>(&Gx[oa]), ay = *reinterpret_cast<const dh_f16x8*>(&Gy[oa]);
                const dh_f16x8 bre = *reinterpret_cast<const dh_f16x8*>(&Rs[ob]);
                p1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ax, bre, p1, 0, 0, 0);
                p3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ay, bre, p3, 0, 0, 0);
                if (rot) {
                    const dh_f16x8 bim = *reinterpret_cast<const dh_f16x8*>(&Is[ob]);
                    p2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ay, bim, p2, 0, 0, 0);
                    p4 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ax, bim, p4, 0, 0, 0);
                }
            }
            __syncthreads();
        }
        const int col = col0 + 32 * wave + r;
        if (col < a.C) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rl = dh_row(reg, h), row = row0 + rl;
                if (row >= a.N) continue;
                float v = 0.f;
                if (row < nvb) {
                    float sx, sy;
                    gather(rl, col, sx, sy);
                    const float bre = rot ? __fsub_rn(p1[reg], p2[reg]) : p1[reg];
                    const float bim = rot ? __fadd_rn(p3[reg], p4[reg]) : p3[reg];
                    v = tanhf(fmaf(sx, bre, __fmul_rn(sy, bim)));
                }
                a.out[((long long)b * a.N + row) * a.ldo + col] = v;
            }
        }
    }
}
}  // namespace

extern "C" int dm_dnet_linear_f16(dm_ctx* ctx, int B, int N, int C_out, int n_src, const void* src0, int w0, int ld0, int dtype0, const void* src1,
                                  int w1, int ld1, int dtype1, const void* src2, int w2, int ld2, int dtype2, const void* W, int ldw,
                                  const void* bias /*nullable*/, int bias_dtype, const float* resid /*nullable*/, int ldr, int act,
                                  const int32_t* n_verts /*nullable*/, int out_dtype, void* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && C_out > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, dm_cdiv(N, 64) <= 65535, "N <= 65535 * 64");
    DM_REQUIRE(ctx, n_src >= 1 && n_src <= 3, "one to three sources");
    DM_REQUIRE(ctx, act == 0 || act == 1, "act: 0 none, 1 ReLU");
    DM_REQUIRE(ctx, dm_dnet_dtype(out_dtype) && (!bias || dm_dnet_dtype(bias_dtype)), "bias and output dtype: DM_F16 or DM_F32");
    const void* src[3] = {src0, src1, src2};
    int w[3] = {w0, w1, w2}, ld[3] = {ld0, ld1, ld2}, dt[3] = {dtype0, dtype1, dtype2};
    long long ktot = 0;
    for (int s = 0; s < 3; ++s) {
        if (s >= n_src) { src[s] = nullptr; w[s] = 0; ld[s] = 0; dt[s] = DM_F32; continue; }
        DM_REQUIRE(ctx, src[s] != nullptr, "null source");
        DM_REQUIRE(ctx, dm_dnet_dtype(dt[s]), "source dtype: DM_F16 or DM_F32");
        DM_REQUIRE(ctx, w[s] > 0 && ld[s] >= w[s], "a source needs width > 0 and ld >= width");
        DM_REQUIRE(ctx, dm_dnet_al(src[s], dt[s] == DM_F16 ? 2 : 4), "a source must be aligned to its element");
        ktot += w[s];
    }
    DM_REQUIRE(ctx, ktot <= (1 << 24), "summed source width");
    DM_REQUIRE(ctx, W && out, "null pointer");
    DM_REQUIRE(ctx, dm_dnet_al(W, 2) && dm_dnet_al(out, out_dtype == DM_F16 ? 2 : 4), "W and out must be aligned to their elements");
    DM_REQUIRE(ctx, ldw >= (int)ktot && ldo >= C_out, "ldw >= summed widths, ldo >= C_out");
    DM_REQUIRE(ctx, !resid || ldr >= C_out, "ldr >= C_out");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "dm_dnet_linear_f16", B, N, n_verts)) return rc;
    hl_args a{N, C_out, (int)ktot, {src[0], src[1], src[2]}, {w[0], w[1], w[2]}, {ld[0], ld[1], ld[2]},
              {dt[0] == DM_F16, dt[1] == DM_F16, dt[2] == DM_F16}, reinterpret_cast<const _Float16*>(W), ldw, bias, bias_dtype == DM_F16,
              resid, ldr, act, n_verts, out, out_dtype == DM_F16, ldo};
    // 128 x 128 tiles once they give every CU one, 64 x 64 below: the bits are the same
    const long long big = (long long)dm_cdiv(C_out, 128) * dm_cdiv(N, 128) * B;
    if (big >= DH_BIG_TILES) DM_LAUNCH(ctx, "dnet_linear_f16", dnet_linear_f16_kernel<2>, dim3(dm_cdiv(C_out, 128), dm_cdiv(N, 128), B), dim3(256), 0, a);
    else DM_LAUNCH(ctx, "dnet_linear_f16", dnet_linear_f16_kernel<1>, dim3(dm_cdiv(C_out, 64), dm_cdiv(N, 64), B), dim3(256), 0, a);
    return DM_OK;
}

extern "C" int dm_dnet_diffuse_f16(dm_ctx* ctx, int B, int N, int K, int C, const float* x, int ldx, const void* evecs_h, int lde,
                                   const void* mevecs_h, int ldm, const int32_t* e1, const int32_t* e2, const float* evals, const void* times,
                                   int times_dtype, const int32_t* n_verts /*nullable*/, float* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && K > 0 && C > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, K <= DH_KMAX, "K <= 1024: the 32 x K spectrum of a workgroup has to fit in LDS");
    DM_REQUIRE(ctx, x && evecs_h && mevecs_h && e1 && e2 && evals && times && out, "null pointer");
    DM_REQUIRE(ctx, dm_dnet_dtype(times_dtype), "times dtype: DM_F16 or DM_F32");
    DM_REQUIRE(ctx, dm_dnet_al(evecs_h, 2) && dm_dnet_al(mevecs_h, 2) && dm_dnet_al(times, times_dtype == DM_F16 ? 2 : 4), "operands must be aligned to their elements");
    DM_REQUIRE(ctx, ldx >= C && ldo >= C && lde >= K && ldm >= K, "ldx >= C, ldo >= C, lde >= K, ldm >= K");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "dm_dnet_diffuse_f16", B, N, n_verts)) return rc;
    const int Kpad = dm_cdiv(K, 32) * 32;
    const size_t lds = ((size_t)DH_CT * (Kpad + 8) + (size_t)DH_KG * DH_VLD + (size_t)DH_CT * DH_VLD) * sizeof(_Float16);
    if (int rc = dm_grant_lds(ctx, (const void*)dnet_diffuse_f16_kernel, lds)) return rc;
    hd_args a{N, K, C, Kpad, x, ldx, reinterpret_cast<const _Float16*>(evecs_h), lde, reinterpret_cast<const _Float16*>(mevecs_h), ldm, e1, e2,
              evals, times, times_dtype == DM_F16, n_verts, out, ldo};
    DM_LAUNCH(ctx, "dnet_diffuse_f16", dnet_diffuse_f16_kernel, dim3(dm_cdiv(C, DH_CT), B), dim3(256), lds, a);
    return DM_OK;
}

extern "C" int dm_dnet_gradfeat_f16(dm_ctx* ctx, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx,
                                    const float* gy, const float* x, int ldx, const void* A_re, const void* A_im /*nullable*/, int lda,
                                    const int32_t* n_verts /*nullable*/, float* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && C > 0 && nnz > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, dm_cdiv(N, DH_T) <= 65535, "N <= 65535 * 64");
    DM_REQUIRE(ctx, row_len && cols && gx && gy && x && A_re && out, "null pointer");
    DM_REQUIRE(ctx, dm_dnet_al(A_re, 2) && dm_dnet_al(A_im, 2), "A_re and A_im must be aligned to their elements");
    DM_REQUIRE(ctx, ldx >= C && ldo >= C && lda >= C, "ldx >= C, ldo >= C, lda >= C");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "dm_dnet_gradfeat_f16", B, N, n_verts)) return rc;
    const int ell_lds = nnz <= DH_ELL_MAX;
    hg_args a{N, C, nnz, row_len, cols, gx, gy, x, ldx, reinterpret_cast<const _Float16*>(A_re), reinterpret_cast<const _Float16*>(A_im), lda,
              n_verts, out, ldo, ell_lds};
    // Where the fp16 gradients of 32 rows fit in LDS for all C channels (C <= 768) and such row tiles give every CU one (a batch), a
    // workgroup owns those rows and gathers once; else 64 x 64 tiles that gather per column tile (a lone mesh of 2048 vertices is 64 row
    // tiles but 256 of these).  Next to them in LDS: the matrix stages, the row lengths and -- up to DH_ELL_MAX entries per row -- the
    // tile's ELL rows (12 bytes per entry).  The bits are the same.
    const int Cp = dm_cdiv(C, DH_RK) * DH_RK;
    const size_t lds_rows = ((size_t)2 * DH_RR * (Cp + 8) + (size_t)2 * DH_RC * DH_RLD) * sizeof(_Float16) + (size_t)DH_RR * 4 +
                            (ell_lds ? (size_t)DH_RR * nnz * 12 : 0);
    if (lds_rows <= DH_LDS_MAX && (long long)dm_cdiv(N, DH_RR) * B >= DH_BIG_TILES) {
        if (int rc = dm_grant_lds(ctx, (const void*)dnet_gradfeat_f16_rows_kernel, lds_rows)) return rc;
        DM_LAUNCH(ctx, "dnet_gradfeat_f16", dnet_gradfeat_f16_rows_kernel, dim3(dm_cdiv(N, DH_RR), B), dim3(256), lds_rows, a, Cp);
        return DM_OK;
    }
    const size_t lds = (size_t)4 * DH_T * DH_GLD * sizeof(_Float16) + (size_t)DH_T * 4 + (ell_lds ? (size_t)DH_T * nnz * 12 : 0);
    if (int rc = dm_grant_lds(ctx, (const void*)dnet_gradfeat_f16_kernel, lds)) return rc;
    DM_LAUNCH(ctx, "dnet_gradfeat_f16", dnet_gradfeat_f16_kernel, dim3(dm_cdiv(C, DH_T), dm_cdiv(N, DH_T), B), dim3(256), lds, a);
    return DM_OK;
}

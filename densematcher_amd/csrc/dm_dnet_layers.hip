// DiffusionNet forward pass (inference), fp32 on the matrix cores: dm_dnet_linear_f32, dm_dnet_diffuse_f32, dm_dnet_gradfeat_f32.
//
// Reference computation replaced: diffusion_net/layers.py
//   17-90     LearnedTimeDiffusion (spectral): evecs (exp(-evals t) * (evecs^T (mass * x)))
//   93-130    SpatialGradientFeatures: tanh(gX * B_re + gY * B_im), B = (A_re + i A_im) applied to the complex gradient
//   133-165   MiniMLP, 200-241 DiffusionNetBlock (torch.mm(gradX, .) / torch.mm(gradY, .) per mesh, two concatenations, the skip), 366-373
// Every product is v_mfma_f32_32x32x2_f32: an exact fp32 fmaf chain in ascending order of the contraction index, so the bits of an
// output element depend on its own row and column of the operands only -- never on the tile it falls in, on the other meshes of the
// call or on the padding (operands beyond a mesh's rows, columns or ELL slots are replaced by zeros when a tile is staged, and
// fma(0, 0, s) = s).  All staging loads are scalar: no operand needs an alignment beyond its element's.
//
// Tiles: four waves per workgroup, one 32 x 32 accumulator block each.  linear / gradfeat: 64 x 64 outputs per workgroup
// (2048 x 512 -> 256 workgroups, one per CU, per mesh); the contraction is staged 32 deep through LDS, the next stage is
// in registers while the current one is multiplied.  diffuse: one workgroup per (mesh, 32 channels); its K x 32 spectrum stays in LDS.
#include <math.h>

#include "dm_dnet_common.h"

typedef float dl_f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int DL_T = 64;          // outputs per workgroup side (linear, gradfeat)
constexpr int DL_KC = 32;         // contraction depth per stage
constexpr int DL_LD = DL_T + 1;   // LDS row stride of a stage [kk][row]
constexpr int DL_CT = 32;         // channels per workgroup (diffuse)
constexpr int DL_KG = 128;        // spectrum rows per pass over the vertices (diffuse): one 32-row block per wave
constexpr int DL_VT = 128;        // vertices per tile of the product back (diffuse)
constexpr int DL_KMAX = 1024;     // largest K whose K x 32 spectrum (+ staging) fits in 160 KB of LDS
constexpr int GF_ELL_MAX = 64;    // widest ELL rows that gradfeat keeps in LDS (dm_dnet_ell writes at most 64 entries per row): 48 KB per tile

__device__ __forceinline__ int dl_nv(const int32_t* nv, int b, int N) { return nv ? nv[b] : N; }
// row of the 32 x 32 accumulator block that register `reg` of a lane in half `h` holds (the column is lane & 31)
__device__ __forceinline__ int dl_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ---------------------------------------------------------------------------------------------------------------- linear
struct lin_args {
    int N, Cout, Ktot;
    const float* src[3]; int w[3]; int ld[3];
    const float* W; int ldw;
    const float* bias; const float* resid; int ldr; int act;
    const int32_t* nv; float* out; int ldo;
};

__global__ __launch_bounds__(256) void dnet_linear_kernel(lin_args a) {
    __shared__ float As[DL_KC * DL_LD], Bs[DL_KC * DL_LD];
    const int b = blockIdx.z, row0 = blockIdx.y * DL_T, col0 = blockIdx.x * DL_T;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int nvb = dl_nv(a.nv, b, a.N);
    const int kk = t & 31, r8 = t >> 5;
    float ra[8], rb[8];
    // a thread stages column kk of rows / weight rows r8 + 8 i: which of them exist is fixed for the kernel, and the source that
    // holds a column of the concatenation is one per thread and stage
    unsigned rmask = 0, cmask = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (row0 + r8 + 8 * i < nvb) rmask |= 1u << i;
        if (col0 + r8 + 8 * i < a.Cout) cmask |= 1u << i;
    }
    const long long brow0 = (long long)b * a.N + row0 + r8, wrow0 = (long long)(col0 + r8) * a.ldw, wstep = 8LL * a.ldw;
    auto fetch = [&](int k0) {
        int k = k0 + kk;
        const bool kin = k < a.Ktot;
        const long long wo = wrow0 + k;
        int s = 0;
        if (k >= a.w[0]) { k -= a.w[0]; s = 1; if (k >= a.w[1]) { k -= a.w[1]; s = 2; } }
        const float* sp = s == 0 ? a.src[0] : (s == 1 ? a.src[1] : a.src[2]);
        const long long ld = s == 0 ? a.ld[0] : (s == 1 ? a.ld[1] : a.ld[2]);
        const long long ao = brow0 * ld + k, astep = 8 * ld;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ra[i] = (kin && ((rmask >> i) & 1u)) ? sp[ao + i * astep] : 0.f;
            rb[i] = (kin && ((cmask >> i) & 1u)) ? a.W[wo + i * wstep] : 0.f;
        }
    };
    dl_f32x16 acc = {0};
    fetch(0);
    for (int k0 = 0; k0 < a.Ktot; k0 += DL_KC) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            As[kk * DL_LD + r8 + 8 * i] = ra[i];
            Bs[kk * DL_LD + r8 + 8 * i] = rb[i];
        }
        __syncthreads();
        if (k0 + DL_KC < a.Ktot) fetch(k0 + DL_KC);
#pragma unroll
        for (int s = 0; s < DL_KC / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * s + h) * DL_LD + 32 * wr + r], Bs[(2 * s + h) * DL_LD + 32 * wc + r], acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = col0 + 32 * wc + r;
    if (col >= a.Cout) return;
    const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = row0 + 32 * wr + dl_row(reg, h);
        if (row >= a.N) continue;
        const long long brow = (long long)b * a.N + row;
        float v = 0.f;
        if (row < nvb) {
            v = acc[reg] + bv;
            if (a.act) v = fmaxf(v, 0.f);
            if (a.resid) v += a.resid[brow * a.ldr + col];
        }
        a.out[brow * a.ldo + col] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- diffuse
struct dif_args {
    int N, K, C, Kpad;
    const float* x; int ldx; const float* mass; const float* evals; const float* evecs; int lde; const float* times;
    const int32_t* nv; float* out; int ldo;
};

__global__ __launch_bounds__(256) void dnet_diffuse_kernel(dif_args a) {
    extern __shared__ float dl_lds[];
    float* spec = dl_lds;                                  // [Kpad][32]
    float* Ps = spec + (size_t)a.Kpad * DL_CT;             // pass 1: [32 vertices][128 k]; pass 2: [128 vertices][33]
    float* Xs = Ps + DL_VT * (DL_KC + 1);                  // [32 vertices][32 channels] of mass * x
    const int b = blockIdx.y, c0 = blockIdx.x * DL_CT;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int nvb = dl_nv(a.nv, b, a.N);
    const long long bN = (long long)b * a.N;
    // ---- pass 1: spec = coef * (evecs^T (mass * x)), 128 rows of it per sweep over the vertices in ascending order
    for (int kg = 0; kg < a.Kpad; kg += DL_KG) {
        float rp[16], rx[4];
        auto fetch = [&](int v0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int e = t + 256 * i, k = kg + (e & 127), v = v0 + (e >> 7);
                rp[i] = (v < nvb && k < a.K) ? a.evecs[(bN + v) * a.lde + k] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = t + 256 * i, c = c0 + (e & 31), v = v0 + (e >> 5);
                rx[i] = (v < nvb && c < a.C) ? a.mass[bN + v] * a.x[(bN + v) * a.ldx + c] : 0.f;
            }
        };
        dl_f32x16 acc = {0};
        const bool live = kg + 32 * wave < a.Kpad;
        fetch(0);
        for (int v0 = 0; v0 < nvb; v0 += 32) {
#pragma unroll
            for (int i = 0; i < 16; ++i) Ps[t + 256 * i] = rp[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) Xs[t + 256 * i] = rx[i];
            __syncthreads();
            if (v0 + 32 < nvb) fetch(v0 + 32);
            if (live) {
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ps[(2 * s + h) * DL_KG + 32 * wave + r], Xs[(2 * s + h) * DL_CT + r], acc, 0, 0, 0);
            }
            __syncthreads();
        }
        if (live) {
            const int c = c0 + r;
            // the reference clamps the times in fp32 (torch.clamp(diffusion_time, min=1e-8)); the exponent and exp() are float64
            const double tc = c < a.C ? (double)fmaxf(a.times[c], 1e-8f) : 0.0;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int k = kg + 32 * wave + dl_row(reg, h);
                float v = 0.f;
                if (k < a.K && c < a.C) v = (float)exp(-(double)a.evals[(long long)b * a.K + k] * tc) * acc[reg];
                spec[k * DL_CT + r] = v;
            }
        }
    }
    __syncthreads();
    // ---- pass 2: out = evecs spec, 128 vertices per tile, k ascending
    const int nk = a.Kpad / DL_KC, nt = dm_cdiv(a.N, DL_VT), total = nk * nt;
    float rp[16];
    auto fetch2 = [&](int it) {
        const int v0 = (it / nk) * DL_VT, k0 = (it % nk) * DL_KC;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = t + 256 * i, k = k0 + (e & 31), v = v0 + (e >> 5);
            rp[i] = (v < nvb && k < a.K) ? a.evecs[(bN + v) * a.lde + k] : 0.f;
        }
    };
    dl_f32x16 acc = {0};
    fetch2(0);
    for (int it = 0; it < total; ++it) {
        const int v0 = (it / nk) * DL_VT, k0 = (it % nk) * DL_KC;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = t + 256 * i;
            Ps[(e >> 5) * (DL_KC + 1) + (e & 31)] = rp[i];
        }
        __syncthreads();
        if (it + 1 < total) fetch2(it + 1);
#pragma unroll
        for (int s = 0; s < 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ps[(32 * wave + r) * (DL_KC + 1) + 2 * s + h], spec[(k0 + 2 * s + h) * DL_CT + r], acc, 0, 0, 0);
        __syncthreads();
        if (k0 + DL_KC == a.Kpad) {
            const int c = c0 + r;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int v = v0 + 32 * wave + dl_row(reg, h);
                if (v < a.N && c < a.C) a.out[(bN + v) * a.ldo + c] = v < nvb ? acc[reg] : 0.f;
                acc[reg] = 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- gradient features
struct gf_args {
    int N, C, nnz;
    const int32_t* row_len; const int32_t* cols; const float* gx; const float* gy;
    const float* x; int ldx; const float* Are; const float* Aim; int lda;
    const int32_t* nv; float* out; int ldo;
    int ell_lds;                                           // the tile's ELL rows fit in LDS next to the stages
};

// (G_x x)[row][ch], (G_y x)[row][ch]: the row's entries in stored order, one fmaf each; slots q >= row_len are not touched, a column
// outside the mesh contributes nothing
__device__ __forceinline__ void gf_gather(const gf_args& a, int b, int row, int ch, int nvb, float& sx, float& sy) {
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

// the same chain from the tile's rows in LDS (gf_stage_rows): `len` entries, a column outside the mesh stored as -1
__device__ __forceinline__ void gf_gather_lds(const gf_args& a, const int32_t* ec, const float* ex, const float* ey, int len, const float* xb,
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

__global__ __launch_bounds__(256) void dnet_gradfeat_kernel(gf_args a) {
    extern __shared__ float gf_lds[];
    float* Xs = gf_lds;
    float* Ys = Xs + DL_KC * DL_LD;
    float* Rs = Ys + DL_KC * DL_LD;
    float* Is = Rs + DL_KC * DL_LD;
    int32_t* El = (int32_t*)(Is + DL_KC * DL_LD);          // [64] entries of each row of the tile (0 behind the mesh's rows)
    int32_t* Ec = El + DL_T;                               // [64][nnz] columns, then the two value planes (ell_lds only)
    float* Ex = (float*)(Ec + DL_T * a.nnz);
    float* Ey = Ex + DL_T * a.nnz;
    const int b = blockIdx.z, row0 = blockIdx.y * DL_T, col0 = blockIdx.x * DL_T;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int nvb = dl_nv(a.nv, b, a.N);
    const bool rot = a.Aim != nullptr;
    const int kk = t & 31, r8 = t >> 5;
    float rgx[8], rgy[8], rre[8], rim[8];
    unsigned rmask = 0, cmask = 0;                         // which of the rows / matrix rows r8 + 8 i this thread stages exist
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (row0 + r8 + 8 * i < nvb) rmask |= 1u << i;
        if (col0 + r8 + 8 * i < a.C) cmask |= 1u << i;
    }
    const long long arow0 = (long long)(col0 + r8) * a.lda, astep = 8LL * a.lda;
    const float* xmesh = a.x + (long long)b * a.N * a.ldx;
    // The gather reads a row's (column, gx, gy) once per channel: the column tiles of a row tile and the 32-channel stages would
    // fetch them from global memory C / 2 times per row.  They go to LDS once per workgroup instead, where they fit.
    if (a.ell_lds) {
        if (t < DL_T) El[t] = row0 + t < nvb ? min(max(a.row_len[(long long)b * a.N + row0 + t], 0), a.nnz) : 0;
        __syncthreads();
        for (int e = t; e < DL_T * a.nnz; e += 256) {
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
        if (a.ell_lds) gf_gather_lds(a, Ec + rl * a.nnz, Ex + rl * a.nnz, Ey + rl * a.nnz, El[rl], xmesh + ch, sx, sy);
        else gf_gather(a, b, row0 + rl, ch, nvb, sx, sy);
    };
    auto fetch = [&](int k0) {
        const int k = k0 + kk;
        const bool kin = k < a.C;
        const long long ao = arow0 + k;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            rgx[i] = 0.f; rgy[i] = 0.f;
            if (kin && ((rmask >> i) & 1u)) gather(r8 + 8 * i, k, rgx[i], rgy[i]);
            const bool in = kin && ((cmask >> i) & 1u);
            rre[i] = in ? a.Are[ao + i * astep] : 0.f;
            rim[i] = (in && rot) ? a.Aim[ao + i * astep] : 0.f;
        }
    };
    dl_f32x16 p1 = {0}, p2 = {0}, p3 = {0}, p4 = {0};
    fetch(0);
    for (int k0 = 0; k0 < a.C; k0 += DL_KC) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = kk * DL_LD + r8 + 8 * i;
            Xs[o] = rgx[i]; Ys[o] = rgy[i]; Rs[o] = rre[i]; Is[o] = rim[i];
        }
        __syncthreads();
        if (k0 + DL_KC < a.C) fetch(k0 + DL_KC);
#pragma unroll
        for (int s = 0; s < DL_KC / 2; ++s) {
            const int oa = (2 * s + h) * DL_LD + 32 * wr + r, ob = (2 * s + h) * DL_LD + 32 * wc + r;
            const float ax = Xs[oa], ay = Ys[oa], bre = Rs[ob];
            p1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, bre, p1, 0, 0, 0);
            p3 = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, bre, p3, 0, 0, 0);
            if (rot) {
                const float bim = Is[ob];
                p2 = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, bim, p2, 0, 0, 0);
                p4 = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, bim, p4, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    const int col = col0 + 32 * wc + r;
    if (col >= a.C) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = row0 + 32 * wr + dl_row(reg, h);
        if (row >= a.N) continue;
        float v = 0.f;
        if (row < nvb) {
            float sx, sy;
            gather(row - row0, col, sx, sy);
            const float bre = rot ? p1[reg] - p2[reg] : p1[reg];
            const float bim = rot ? p3[reg] + p4[reg] : p3[reg];
            v = tanhf(fmaf(sx, bre, __fmul_rn(sy, bim)));
        }
        a.out[((long long)b * a.N + row) * a.ldo + col] = v;
    }
}
}  // namespace

extern "C" int dm_dnet_linear_f32(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* src0, int w0, int ld0, const float* src1, int w1,
                                  int ld1, const float* src2, int w2, int ld2, const float* W, int ldw, const float* bias /*nullable*/,
                                  const float* resid /*nullable*/, int ldr, int act, const int32_t* n_verts /*nullable*/, float* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && C_out > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, n_src >= 1 && n_src <= 3, "one to three sources");
    DM_REQUIRE(ctx, act == 0 || act == 1, "act: 0 none, 1 ReLU");
    const float* src[3] = {src0, src1, src2};
    int w[3] = {w0, w1, w2}, ld[3] = {ld0, ld1, ld2};
    long long ktot = 0;
    for (int s = 0; s < 3; ++s) {
        if (s >= n_src) { src[s] = nullptr; w[s] = 0; ld[s] = 0; continue; }
        DM_REQUIRE(ctx, src[s] != nullptr, "null source");
        DM_REQUIRE(ctx, w[s] > 0 && ld[s] >= w[s], "a source needs width > 0 and ld >= width");
        ktot += w[s];
    }
    DM_REQUIRE(ctx, ktot <= (1 << 24), "summed source width");
    DM_REQUIRE(ctx, W && out, "null pointer");
    DM_REQUIRE(ctx, ldw >= (int)ktot && ldo >= C_out, "ldw >= summed widths, ldo >= C_out");
    DM_REQUIRE(ctx, !resid || ldr >= C_out, "ldr >= C_out");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "dm_dnet_linear_f32", B, N, n_verts)) return rc;
    lin_args a{N, C_out, (int)ktot, {src[0], src[1], src[2]}, {w[0], w[1], w[2]}, {ld[0], ld[1], ld[2]}, W, ldw, bias, resid, ldr, act, n_verts, out, ldo};
    DM_LAUNCH(ctx, "dnet_linear", dnet_linear_kernel, dim3(dm_cdiv(C_out, DL_T), dm_cdiv(N, DL_T), B), dim3(256), 0, a);
    return DM_OK;
}

extern "C" int dm_dnet_diffuse_f32(dm_ctx* ctx, int B, int N, int K, int C, const float* x, int ldx, const float* mass, const float* evals,
                                   const float* evecs, int lde, const float* times, const int32_t* n_verts /*nullable*/, float* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && K > 0 && C > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, K <= DL_KMAX, "K <= 1024: the K x 32 spectrum of a workgroup has to fit in LDS");
    DM_REQUIRE(ctx, x && mass && evals && evecs && times && out, "null pointer");
    DM_REQUIRE(ctx, ldx >= C && ldo >= C && lde >= K, "ldx >= C, ldo >= C, lde >= K");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "dm_dnet_diffuse_f32", B, N, n_verts)) return rc;
    const int Kpad = dm_cdiv(K, DL_KC) * DL_KC;
    const size_t lds = ((size_t)Kpad * DL_CT + DL_VT * (DL_KC + 1) + 32 * DL_CT) * sizeof(float);
    if (int rc = dm_grant_lds(ctx, (const void*)dnet_diffuse_kernel, lds)) return rc;
    dif_args a{N, K, C, Kpad, x, ldx, mass, evals, evecs, lde, times, n_verts, out, ldo};
    DM_LAUNCH(ctx, "dnet_diffuse", dnet_diffuse_kernel, dim3(dm_cdiv(C, DL_CT), B), dim3(256), lds, a);
    return DM_OK;
}

extern "C" int dm_dnet_gradfeat_f32(dm_ctx* ctx, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx,
                                    const float* gy, const float* x, int ldx, const float* A_re, const float* A_im /*nullable*/, int lda,
                                    const int32_t* n_verts /*nullable*/, float* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && C > 0 && nnz > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, row_len && cols && gx && gy && x && A_re && out, "null pointer");
    DM_REQUIRE(ctx, ldx >= C && ldo >= C && lda >= C, "ldx >= C, ldo >= C, lda >= C");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dm_dnet_check_counts(ctx, "dm_dnet_gradfeat_f32", B, N, n_verts)) return rc;
    // the four stages, the row lengths and -- up to GF_ELL_MAX entries per row -- the tile's ELL rows (12 bytes per entry)
    const int ell_lds = nnz <= GF_ELL_MAX;
    const size_t lds = (size_t)(4 * DL_KC * DL_LD + DL_T) * 4 + (ell_lds ? (size_t)DL_T * nnz * 12 : 0);
    if (int rc = dm_grant_lds(ctx, (const void*)dnet_gradfeat_kernel, lds)) return rc;
    gf_args a{N, C, nnz, row_len, cols, gx, gy, x, ldx, A_re, A_im, lda, n_verts, out, ldo, ell_lds};
    DM_LAUNCH(ctx, "dnet_gradfeat", dnet_gradfeat_kernel, dim3(dm_cdiv(C, DL_T), dm_cdiv(N, DL_T), B), dim3(256), lds, a);
    return DM_OK;
}

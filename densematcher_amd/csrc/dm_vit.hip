// DINOv2 ViT encoder (inference) on the fp16 matrix cores: dm_vit_patch_rows_f16 (resize, normalise and lay the 14 x 14 patches out as
// GEMM rows), dm_vit_layernorm_f16, dm_vit_linear_f16 (out = resid + scale * act(A W^T + bias), dense output) and dm_vit_attention_f16
// (flash-style softmax(q k^T / 8) v per image and head; the T x T scores are never stored).
//
// Reference computation replaced: the DINOv2 ViT-B/14 that densematcher/featurizers/SDDINO.py:27 builds through
//   third_party/featup/featup/model_utils/extractor_dino.py:24-53   ViTExtractor('dinov2_vitb14', stride=14)
//   extractor_dino.py:181-190                                        resize_and_normalize (bilinear, align_corners=False; Normalize)
//   SDDINO.py:49-51                                                  the tokens of block 11 without the cls token as (bs, 768, P, P)
// and the encoder itself: patch embedding (Conv2d 14 x 14, stride 14), pre-norm blocks x + ls1(attn(norm1 x)), x + ls2(mlp(norm2 x)).
//
// Every product is a fixed-order sum: v_mfma_f32_32x32x16_f16 (exact fp16 products, fp32 accumulation) over ascending chunks of the
// contraction index, no split along it, no atomics.  An output element depends on its own row (linear, LayerNorm) or its own image and
// head (attention) only, so an image has the same bits alone and in any batch.
//
// linear: a workgroup of four waves owns 128 x 128 outputs, a wave 64 x 64 (2 x 2 accumulator blocks); stages of 64 contraction indices
// go global -> registers -> LDS (16-byte loads, the next stage fetched while the current one is multiplied).  Lane (r = lane & 31,
// h = lane >> 5) of a 32x32x16 step holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r], j = 0 .. 7: eight adjacent halves of a row of
// A and of a row of W.  Accumulator register `reg` is row (reg & 3) + 8 (reg >> 2) + 4 h, column r.
// attention: a workgroup owns 128 queries of one (image, head), a wave 32 of them.  S^T = K Q^T is computed (keys on the accumulator
// rows, the query on the lane), so a query's maximum and sum are reductions over a lane's registers and one exchange between the two
// half-waves, and the rounded P^T is, as it lies in the registers, the B operand of O^T = V^T P^T: the 16 keys of an MFMA step are
// taken in the order the accumulator holds them, and V is staged transposed in LDS so that the A operand follows the same order.
// All memory operations are vector loads and stores.
#include <math.h>

#include <hip/hip_fp16.h>

#include "dm_internal.h"

typedef float vt_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 vt_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 vt_f16x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int VT_PATCH = 14, VT_PATCH_K = 3 * VT_PATCH * VT_PATCH;   // 588
constexpr int VL_T = 128, VL_KC = 64, VL_LD = VL_KC + 8;             // output tile, contraction stage (the K granule), LDS row in halves
constexpr int VA_QT = 128, VA_KT = 64, VA_HD = 64, VA_LD = 72;        // query tile, key tile, head dimension, LDS row in halves
constexpr double VT_LN_EPS = 1e-6;

__device__ __forceinline__ int vt_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
__device__ __forceinline__ float vt_load(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float vt_load(const float* p) { return *p; }
__device__ __forceinline__ void vt_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void vt_store(_Float16* p, float v) { *p = (_Float16)v; }

// ---------------------------------------------------------------------------------------------------------------- patch rows
struct patch_args {
    int S, P, Kp, ldo;
    long long total, si, sc, sy, sx;
    const void* img; _Float16* out;
    float mean[3], std[3];
};

// F.interpolate(bilinear, align_corners=False) from (S, S) to (Z, Z) at (ty, tx), the convention of dm_agg_gather_f32
template <typename T>
__device__ __forceinline__ float vt_interp(const T* base, const patch_args& a, int Z, int ty, int tx) {
    if (a.S == Z) return vt_load(base + ty * a.sy + tx * a.sx);
    double fy = ((double)ty + 0.5) * ((double)a.S / (double)Z) - 0.5, fx = ((double)tx + 0.5) * ((double)a.S / (double)Z) - 0.5;
    fy = fy < 0.0 ? 0.0 : fy;
    fx = fx < 0.0 ? 0.0 : fx;
    const int y0 = min((int)fy, a.S - 1), x0 = min((int)fx, a.S - 1);
    const int y1 = y0 + (y0 < a.S - 1 ? 1 : 0), x1 = x0 + (x0 < a.S - 1 ? 1 : 0);
    const float ly = (float)(fy - (double)y0), lx = (float)(fx - (double)x0);
    const float p = vt_load(base + y0 * a.sy + x0 * a.sx), q = vt_load(base + y0 * a.sy + x1 * a.sx);
    const float r = vt_load(base + y1 * a.sy + x0 * a.sx), s = vt_load(base + y1 * a.sy + x1 * a.sx);
    return (1.0f - ly) * ((1.0f - lx) * p + lx * q) + ly * ((1.0f - lx) * r + lx * s);
}

template <typename T>
__global__ void __launch_bounds__(256) vit_patch_rows_kernel(patch_args a) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.total) return;
    const long long row = e / a.Kp;
    const int k = (int)(e - row * a.Kp);
    float v = 0.0f;                                          // the padding columns k >= 588 are zeros
    if (k < VT_PATCH_K) {
        const int npatch = a.P * a.P, img = (int)(row / npatch), p = (int)(row - (long long)img * npatch);
        const int c = k / (VT_PATCH * VT_PATCH), rem = k - c * VT_PATCH * VT_PATCH, dy = rem / VT_PATCH, dx = rem - dy * VT_PATCH;
        const int py = p / a.P, px = p - py * a.P;
        const T* base = reinterpret_cast<const T*>(a.img) + img * a.si + c * a.sc;
        const float x = vt_interp(base, a, VT_PATCH * a.P, VT_PATCH * py + dy, VT_PATCH * px + dx);
        v = __fdiv_rn(__fsub_rn(x, a.mean[c]), a.std[c]);
    }
    a.out[row * a.ldo + k] = (_Float16)v;
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm
// one wave per row: the fp64 sum, then the fp64 sum of squared deviations from the fp64 mean; a lane's elements ascending, the 64
// partial sums through the xor tree (the same value in every lane)
__device__ __forceinline__ double vt_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <typename TO>
__global__ void __launch_bounds__(256) vit_layernorm_kernel(int M, int D, const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, TO* __restrict__ out, int ldo) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;                                    // a whole wave leaves; the kernel has no barrier
    const float* xr = x + row * ldx;
    double s = 0.0;
    for (int c = lane; c < D; c += 64) s += (double)xr[c];
    const double mean = vt_wave_sum(s) / (double)D;
    double q = 0.0;
    for (int c = lane; c < D; c += 64) {
        const double d = (double)xr[c] - mean;
        q += d * d;
    }
    const double rstd = 1.0 / sqrt(vt_wave_sum(q) / (double)D + VT_LN_EPS);
    TO* orow = out + row * ldo;
    for (int c = lane; c < D; c += 64) {
        const float n = (float)(((double)xr[c] - mean) * rstd);
        vt_store(orow + c, fmaf(n, gamma[c], beta[c]));
    }
}

// ---------------------------------------------------------------------------------------------------------------- linear
struct lin_args {
    int Mb, N, K, act;
    const _Float16* A; int lda; long long sA;
    const _Float16* W; int ldw;
    const float *bias, *scale, *resid; int ldr; long long sR;
    void* out; int ldo; long long sO;
};

__device__ __forceinline__ float vt_gelu(float v) { return __fmul_rn(__fmul_rn(0.5f, v), __fadd_rn(1.0f, erff(__fmul_rn(v, 0.70710678118654752440f)))); }

template <typename TO>
__global__ void __launch_bounds__(256) vit_linear_kernel(lin_args a) {
    __shared__ __attribute__((aligned(16))) _Float16 As[VL_T * VL_LD], Bs[VL_T * VL_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;
    const int row0 = blockIdx.y * VL_T, col0 = blockIdx.x * VL_T;
    const long long blk = blockIdx.z;
    const _Float16* Ab = a.A + blk * a.sA;
    // a thread stages the halves kq .. kq + 7 of the rows sr + 32 i of both tiles
    const int sr = t >> 3, kq = (t & 7) * 8;
    vt_f16x8 ra[4], rb[4];
    const vt_f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gr = row0 + sr + 32 * i, gc = col0 + sr + 32 * i;
            ra[i] = gr < a.Mb ? *reinterpret_cast<const vt_f16x8*>(Ab + (long long)gr * a.lda + k0 + kq) : zero8;
            rb[i] = gc < a.N ? *reinterpret_cast<const vt_f16x8*>(a.W + (long long)gc * a.ldw + k0 + kq) : zero8;
        }
    };
    vt_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    fetch(0);
    for (int k0 = 0; k0 < a.K; k0 += VL_KC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<vt_f16x8*>(&As[(sr + 32 * i) * VL_LD + kq]) = ra[i];
            *reinterpret_cast<vt_f16x8*>(&Bs[(sr + 32 * i) * VL_LD + kq]) = rb[i];
        }
        __syncthreads();
        if (k0 + VL_KC < a.K) fetch(k0 + VL_KC);
#pragma unroll
        for (int s = 0; s < VL_KC / 16; ++s) {
            vt_f16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const vt_f16x8*>(&As[(64 * wr + 32 * i + r) * VL_LD + 16 * s + 8 * h]);
                fb[i] = *reinterpret_cast<const vt_f16x8*>(&Bs[(64 * wc + 32 * i + r) * VL_LD + 16 * s + 8 * h]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // epilogue: + bias, act, * scale, + resid, each rounded on its own; an element is read (resid) and written by the same lane
    TO* ob = reinterpret_cast<TO*>(a.out) + blk * a.sO;
    const float* rbk = a.resid ? a.resid + blk * a.sR : nullptr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = col0 + 64 * wc + 32 * j + r;
        if (col >= a.N) continue;
        const float bv = a.bias ? a.bias[col] : 0.0f, sv = a.scale ? a.scale[col] : 1.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = row0 + 64 * wr + 32 * i + vt_row(reg, h);
                if (row >= a.Mb) continue;
                float v = acc[i][j][reg];
                if (a.bias) v = __fadd_rn(v, bv);
                if (a.act) v = vt_gelu(v);
                if (a.scale) v = __fmul_rn(sv, v);
                if (rbk) v = __fadd_rn(rbk[(long long)row * a.ldr + col], v);
                vt_store(ob + (long long)row * a.ldo + col, v);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- attention
struct attn_args {
    int T, H;
    const _Float16* qkv; int ldq; long long sq;
    _Float16* out; int ldo; long long so;
};

__global__ void __launch_bounds__(256) vit_attention_kernel(attn_args a) {
    __shared__ __attribute__((aligned(16))) _Float16 Ks[VA_KT * VA_LD], Vt[VA_HD * VA_LD];      // K [key][d], V transposed [d][key]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, D = a.H * VA_HD, q = blockIdx.x * VA_QT + wave * 32 + r;
    const _Float16* base = a.qkv + (long long)blockIdx.z * a.sq + head * VA_HD;
    const vt_f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    // the query as the B operand of S^T = K Q^T: lane (r, h) holds q[16 s + 8 h + j], scaled by 1 / 8 (exact)
    vt_f16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        qf[s] = q < a.T ? *reinterpret_cast<const vt_f16x8*>(base + (long long)q * a.ldq + 16 * s + 8 * h) : zero8;
        qf[s] = qf[s] * (_Float16)0.125f;
    }
    vt_f32x16 o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[0][e] = o[1][e] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const int skey = t >> 3, sdq = (t & 7) * 8;               // staging: halves sdq .. sdq + 7 of the keys skey, skey + 32
    for (int k0 = 0; k0 < a.T; k0 += VA_KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = skey + 32 * i, gk = k0 + key;
            vt_f16x8 kv = zero8, vv = zero8;                  // keys at positions >= T are staged as zeros
            if (gk < a.T) {
                kv = *reinterpret_cast<const vt_f16x8*>(base + (long long)gk * a.ldq + D + sdq);
                vv = *reinterpret_cast<const vt_f16x8*>(base + (long long)gk * a.ldq + 2 * D + sdq);
            }
            *reinterpret_cast<vt_f16x8*>(&Ks[key * VA_LD + sdq]) = kv;
#pragma unroll
            for (int j = 0; j < 8; ++j) Vt[(sdq + j) * VA_LD + key] = vv[j];
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int kb = k0 + 32 * sub;
            if (kb >= a.T) break;                             // uniform: the whole half tile lies behind the last key
            vt_f32x16 sc;
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[e] = 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const vt_f16x8 kf = *reinterpret_cast<const vt_f16x8*>(&Ks[(32 * sub + r) * VA_LD + 16 * s + 8 * h]);
                sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], sc, 0, 0, 0);
            }
            // register reg: key kb + vt_row(reg, h), query q; a key >= T scores -inf and weighs exactly 0
            float tmax = -INFINITY;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                if (kb + vt_row(reg, h) >= a.T) sc[reg] = -INFINITY;
                tmax = fmaxf(tmax, sc[reg]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float m_new = fmaxf(m_run, tmax);           // finite: key 0 lies in the first half tile
            const float alpha = expf(m_run - m_new);
            float lsum = 0.0f;
            vt_f16x8 pf[2];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float p = expf(sc[reg] - m_new);
                lsum = __fadd_rn(lsum, p);
                pf[reg >> 3][reg & 7] = (_Float16)p;
            }
            l_run = __fadd_rn(__fmul_rn(l_run, alpha), lsum);
            m_run = m_new;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                o[0][e] = __fmul_rn(o[0][e], alpha);
                o[1][e] = __fmul_rn(o[1][e], alpha);
            }
            // O^T += V^T P^T: element j of step s2 is the key 32 sub + 16 s2 + 8 (j >> 2) + 4 h + (j & 3), as the accumulator holds it
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const _Float16* vrow = &Vt[(32 * db + r) * VA_LD + 32 * sub + 16 * s2 + 4 * h];
                    const vt_f16x4 lo = *reinterpret_cast<const vt_f16x4*>(vrow), hi = *reinterpret_cast<const vt_f16x4*>(vrow + 8);
                    const vt_f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[s2], o[db], 0, 0, 0);
                }
        }
    }
    if (q >= a.T) return;                                     // query rows >= T are not written
    const float l = __fadd_rn(l_run, __shfl_xor(l_run, 32));
    _Float16* orow = a.out + (long long)blockIdx.z * a.so + (long long)q * a.ldo + head * VA_HD;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            vt_f16x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = (_Float16)__fdiv_rn(o[db][4 * g + j], l);
            *reinterpret_cast<vt_f16x4*>(orow + 32 * db + 8 * g + 4 * h) = w;
        }
}

bool vt_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int dm_vit_patch_rows_f16(dm_ctx* ctx, int n, int S, int P, int src_dtype, const void* img, long long s_img, long long s_chan,
                                     long long s_row, long long s_col, const double* mean, const double* std, int Kp, void* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, n > 0 && S > 0 && P > 0 && S <= 16384 && P <= 1024, "sizes must be positive, S <= 16384, P <= 1024");
    DM_REQUIRE(ctx, src_dtype == DM_F16 || src_dtype == DM_F32, "source dtype: DM_F16 or DM_F32");
    DM_REQUIRE(ctx, img && mean && std && out, "null pointer");
    DM_REQUIRE(ctx, s_img >= 0 && s_chan >= 0 && s_row >= 0 && s_col >= 0, "source strides must not be negative");
    DM_REQUIRE(ctx, Kp >= VT_PATCH_K && Kp % VL_KC == 0 && Kp <= 4096, "Kp: 588 padded to a multiple of 64");
    DM_REQUIRE(ctx, ldo >= Kp, "ldo >= Kp");
    patch_args a{};
    a.S = S; a.P = P; a.Kp = Kp; a.ldo = ldo;
    a.total = (long long)n * P * P * Kp;
    a.si = s_img; a.sc = s_chan; a.sy = s_row; a.sx = s_col;
    a.img = img; a.out = reinterpret_cast<_Float16*>(out);
    for (int c = 0; c < 3; ++c) {
        DM_REQUIRE(ctx, isfinite(mean[c]) && isfinite(std[c]) && std[c] > 0.0, "mean finite, std positive");
        a.mean[c] = (float)mean[c];
        a.std[c] = (float)std[c];
    }
    DM_REQUIRE(ctx, (a.total + 255) / 256 < (1LL << 31), "n * P * P * Kp");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((a.total + 255) / 256));
    if (src_dtype == DM_F16) DM_LAUNCH(ctx, "vit_patch_rows", vit_patch_rows_kernel<__half>, grid, dim3(256), 0, a);
    else DM_LAUNCH(ctx, "vit_patch_rows", vit_patch_rows_kernel<float>, grid, dim3(256), 0, a);
    return DM_OK;
}

extern "C" int dm_vit_layernorm_f16(dm_ctx* ctx, int M, int D, const float* x, int ldx, const float* gamma, const float* beta, int out_dtype,
                                    void* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, M > 0 && D > 0, "sizes must be positive");
    DM_REQUIRE(ctx, out_dtype == DM_F16 || out_dtype == DM_F32, "output dtype: DM_F16 or DM_F32");
    DM_REQUIRE(ctx, ldx >= D && ldo >= D, "ldx >= D, ldo >= D");
    DM_REQUIRE(ctx, x && gamma && beta && out, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid(dm_cdiv(M, 4));
    if (out_dtype == DM_F16) DM_LAUNCH(ctx, "vit_layernorm", vit_layernorm_kernel<_Float16>, grid, dim3(256), 0, M, D, x, ldx, gamma, beta, reinterpret_cast<_Float16*>(out), ldo);
    else DM_LAUNCH(ctx, "vit_layernorm", vit_layernorm_kernel<float>, grid, dim3(256), 0, M, D, x, ldx, gamma, beta, reinterpret_cast<float*>(out), ldo);
    return DM_OK;
}

extern "C" int dm_vit_linear_f16(dm_ctx* ctx, int B, int Mb, int N, int K, const void* A, int lda, long long strideA, const void* W, int ldw,
                                 const float* bias, const float* scale, const float* resid, int ldr, long long strideR, int act, int out_dtype,
                                 void* out, int ldo, long long strideO) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && Mb > 0 && N > 0 && K > 0, "sizes must be positive");
    DM_REQUIRE(ctx, B <= 65535 && dm_cdiv(Mb, VL_T) <= 65535, "B <= 65535, Mb <= 65535 * 128");
    DM_REQUIRE(ctx, K % VL_KC == 0, "K must be a multiple of the granule 64");
    DM_REQUIRE(ctx, act == 0 || act == 1, "act: 0 none, 1 erf-GELU");
    DM_REQUIRE(ctx, out_dtype == DM_F16 || out_dtype == DM_F32, "output dtype: DM_F16 or DM_F32");
    DM_REQUIRE(ctx, A && W && out, "null pointer");
    DM_REQUIRE(ctx, lda >= K && ldw >= K && ldo >= N && (!resid || ldr >= N), "lda >= K, ldw >= K, ldo >= N, ldr >= N");
    DM_REQUIRE(ctx, strideA >= 0 && strideR >= 0 && strideO >= 0, "block strides must not be negative");
    DM_REQUIRE(ctx, B == 1 || strideO >= (long long)(Mb - 1) * ldo + N, "output blocks must not overlap");
    DM_REQUIRE(ctx, vt_aligned16(A) && vt_aligned16(W) && lda % 8 == 0 && ldw % 8 == 0 && strideA % 8 == 0,
               "A and W: 16-byte aligned, leading dimensions and block stride multiples of 8 halves");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    lin_args a{Mb, N, K, act, reinterpret_cast<const _Float16*>(A), lda, strideA, reinterpret_cast<const _Float16*>(W), ldw,
               bias, scale, resid, ldr, strideR, out, ldo, strideO};
    const dim3 grid(dm_cdiv(N, VL_T), dm_cdiv(Mb, VL_T), B);
    if (out_dtype == DM_F16) DM_LAUNCH(ctx, "vit_linear", vit_linear_kernel<_Float16>, grid, dim3(256), 0, a);
    else DM_LAUNCH(ctx, "vit_linear", vit_linear_kernel<float>, grid, dim3(256), 0, a);
    return DM_OK;
}

extern "C" int dm_vit_attention_f16(dm_ctx* ctx, int n, int T, int heads, int head_dim, const void* qkv, int ldq, long long stride_q, void* out,
                                    int ldo, long long stride_o) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, n > 0 && T > 0 && heads > 0, "sizes must be positive");
    DM_REQUIRE(ctx, head_dim == VA_HD, "head dimension 64 only");
    DM_REQUIRE(ctx, n <= 65535 && heads <= 65535 && T <= (1 << 24), "n, heads <= 65535, T <= 2^24");
    DM_REQUIRE(ctx, qkv && out, "null pointer");
    DM_REQUIRE(ctx, ldq >= 3 * heads * VA_HD && ldo >= heads * VA_HD, "ldq >= 3 D, ldo >= D");
    DM_REQUIRE(ctx, stride_q >= 0 && stride_o >= 0 && (n == 1 || stride_o >= (long long)(T - 1) * ldo + heads * VA_HD), "image strides");
    DM_REQUIRE(ctx, vt_aligned16(qkv) && vt_aligned16(out) && ldq % 8 == 0 && ldo % 8 == 0 && stride_q % 8 == 0 && stride_o % 8 == 0,
               "qkv and out: 16-byte aligned, leading dimensions and image strides multiples of 8 halves");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    attn_args a{T, heads, reinterpret_cast<const _Float16*>(qkv), ldq, stride_q, reinterpret_cast<_Float16*>(out), ldo, stride_o};
    DM_LAUNCH(ctx, "vit_attention", vit_attention_kernel, dim3(dm_cdiv(T, VA_QT), heads, n), dim3(256), 0, a);
    return DM_OK;
}

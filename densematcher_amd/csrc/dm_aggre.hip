// Aggregation network of the 2D backbone (inference), fp32 on rows = pixels, channels last: dm_agg_gather_f32 (interpolation to the
// patch grid, rotation back, mean over the rotations and concatenation of the backbone's raw outputs in one pass),
// dm_groupnorm_stats_f32 / dm_groupnorm_relu_f32, dm_conv3x3_f32 (implicit GEMM on the matrix cores) and dm_agg_mix_f32 (the last
// GroupNorms of the bottleneck blocks, the shortcut -- projected and normalised, or the block's input where it has as many channels as
// the output --, ReLU and the softmax mixture).  The 1x1 convolutions are dm_dnet_linear_f32.
//
// Reference computation replaced: densematcher/featurizers
//   SDDINO.py:53-57                      F.interpolate(s4 | s5, bilinear, align_corners=False), torch.cat([s3, s4, s5, dino], 1)
//   SDDINO.py:67-90                      rotate(features[idx], -idx * angle, BILINEAR) summed over idx, / num_rotations
//   modules/resnet.py:271-287            BottleneckBlock.forward (GN after every convolution, projection shortcut, ReLU)
//   modules/projection_network.py:89-123 AggregationNetwork.forward (softmax mixing weights, first term assigned, the rest added)
//
// Every output element is computed by one thread (or one accumulator register of one wave) in a fixed order from its own image: no
// atomics, no sums across workgroups other than the (image, group) statistics, which one workgroup reduces through a fixed tree.  An
// image therefore has the same bits alone and in any batch.
//
// gather: a workgroup owns 32 pixels x 32 channels of one source; it reads with the lanes along whichever of pixel / channel is
// adjacent in the source's memory, stages the tile in LDS and writes it with the lanes along the channels (the output is channels-last).
// conv3x3: dnet_linear_kernel's 64 x 64 x 32 tiling (four waves, one 32 x 32 accumulator block each, v_mfma_f32_32x32x2_f32: an exact
// fp32 fmaf chain in ascending order of the contraction index k = (3 dy + dx) C_in + c); a row of the left operand is a pixel of ONE
// image, column k of it the input at (y + dy - 1, x + dx - 1, c) or zero outside the image, gathered while the stage is fetched.
// All memory operations are vector loads and stores.
#include <math.h>

#include <hip/hip_fp16.h>

#include "dm_internal.h"

typedef float ag_f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int AG_MAX_SRC = 8, AG_MAX_ROT = 16;
constexpr int AG_TILE = 32;               // pixels and channels of a gather tile
constexpr double AG_EPS = 1e-5;           // nn.GroupNorm's default, which the reference's get_norm leaves in place
constexpr int CV_T = 64, CV_KC = 32, CV_LD = CV_T + 1;

__device__ __forceinline__ float ag_load(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float ag_load(const float* p) { return *p; }

// ---------------------------------------------------------------------------------------------------------------- gather
struct ag_src {
    const void* p; int C, h, w, dtype, off, tiles;
    long long si, sc, sy, sx;             // element strides (image, channel, row, col)
};
struct gather_args {
    int n_src, R, B, Ph, Pw, ld, identity;          // identity: step = 0, every rotation takes the pixel itself
    float* out;
    double cs[AG_MAX_ROT], sn[AG_MAX_ROT];          // cos / sin of radians(-r step)
    ag_src s[AG_MAX_SRC];
};

// interp_s(src[img, c])(ty, tx): F.interpolate(bilinear, align_corners=False) to (Ph, Pw); `base` points at (img, c, 0, 0)
template <typename T>
__device__ __forceinline__ float ag_interp(const T* base, const ag_src& s, int Ph, int Pw, int ty, int tx) {
    if (s.h == Ph && s.w == Pw) return ag_load(base + ty * s.sy + tx * s.sx);
    double fy = ((double)ty + 0.5) * ((double)s.h / (double)Ph) - 0.5, fx = ((double)tx + 0.5) * ((double)s.w / (double)Pw) - 0.5;
    fy = fy < 0.0 ? 0.0 : fy;
    fx = fx < 0.0 ? 0.0 : fx;
    const int y0 = min((int)fy, s.h - 1), x0 = min((int)fx, s.w - 1);
    const int y1 = y0 + (y0 < s.h - 1 ? 1 : 0), x1 = x0 + (x0 < s.w - 1 ? 1 : 0);
    const float ly = (float)(fy - (double)y0), lx = (float)(fx - (double)x0);
    const float a = ag_load(base + y0 * s.sy + x0 * s.sx), b = ag_load(base + y0 * s.sy + x1 * s.sx);
    const float c = ag_load(base + y1 * s.sy + x0 * s.sx), d = ag_load(base + y1 * s.sy + x1 * s.sx);
    return (1.0f - ly) * ((1.0f - lx) * a + lx * b) + ly * ((1.0f - lx) * c + lx * d);
}

// out[b, p, off + c] of one source: the rotations in ascending order, summed from zero, divided by R
template <typename T>
__device__ __forceinline__ float ag_value(const gather_args& a, const ag_src& s, int b, int c, int y, int x) {
    float sum = 0.0f;
    for (int r = 0; r < a.R; ++r) {
        const T* base = reinterpret_cast<const T*>(s.p) + (long long)(r * a.B + b) * s.si + (long long)c * s.sc;
        float v;
        if (r == 0 || a.identity) {
            v = ag_interp(base, s, a.Ph, a.Pw, y, x);
        } else {
            const double xb = (double)x - 0.5 * a.Pw + 0.5, yb = (double)y - 0.5 * a.Ph + 0.5;
            const double ix = a.cs[r] * xb - a.sn[r] * yb + 0.5 * a.Pw - 0.5, iy = a.sn[r] * xb + a.cs[r] * yb + 0.5 * a.Ph - 0.5;
            const double fx0 = floor(ix), fy0 = floor(iy);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const float tx = (float)(ix - fx0), ty = (float)(iy - fy0);
            const bool xin0 = x0 >= 0 && x0 < a.Pw, xin1 = x0 + 1 >= 0 && x0 + 1 < a.Pw;
            const bool yin0 = y0 >= 0 && y0 < a.Ph, yin1 = y0 + 1 >= 0 && y0 + 1 < a.Ph;
            v = 0.0f;                                    // nw, ne, sw, se; a tap outside the map is not read
            if (yin0 && xin0) v = ag_interp(base, s, a.Ph, a.Pw, y0, x0) * ((1.0f - tx) * (1.0f - ty));
            if (yin0 && xin1) v += ag_interp(base, s, a.Ph, a.Pw, y0, x0 + 1) * (tx * (1.0f - ty));
            if (yin1 && xin0) v += ag_interp(base, s, a.Ph, a.Pw, y0 + 1, x0) * ((1.0f - tx) * ty);
            if (yin1 && xin1) v += ag_interp(base, s, a.Ph, a.Pw, y0 + 1, x0 + 1) * (tx * ty);
        }
        sum += v;
    }
    return sum / (float)a.R;
}

__global__ void __launch_bounds__(256) agg_gather_kernel(gather_args a) {
    __shared__ float tile[AG_TILE * (AG_TILE + 1)];          // [pixel][channel]
    const int t = threadIdx.x, lo = t & 31, hi = t >> 5, b = blockIdx.z, npix = a.Ph * a.Pw;
    int si = 0, ct = blockIdx.y;
    while (si < a.n_src - 1 && ct >= a.s[si].tiles) { ct -= a.s[si].tiles; ++si; }
    const ag_src& s = a.s[si];
    const int p0 = blockIdx.x * AG_TILE, c0 = ct * AG_TILE;
    const bool chan_fastest = s.sc == 1;
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int pl = chan_fastest ? hi + 8 * i : lo, cl = chan_fastest ? lo : hi + 8 * i;
        const int p = p0 + pl, c = c0 + cl;
        float v = 0.0f;
        if (p < npix && c < s.C) {
            const int y = p / a.Pw, x = p - y * a.Pw;
            v = s.dtype == DM_F16 ? ag_value<__half>(a, s, b, c, y, x) : ag_value<float>(a, s, b, c, y, x);
        }
        tile[pl * (AG_TILE + 1) + cl] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pl = hi + 8 * i, p = p0 + pl, c = c0 + lo;
        if (p < npix && c < s.C) a.out[((long long)b * npix + p) * a.ld + s.off + c] = tile[pl * (AG_TILE + 1) + lo];
    }
}

// ---------------------------------------------------------------------------------------------------------------- GroupNorm
// the sum of the 256 partial sums through a fixed tree; every thread returns it
__device__ __forceinline__ double ag_block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    const double total = sh[0];
    __syncthreads();
    return total;
}

// one workgroup per (image, group): float64 sum, then the float64 sum of squared deviations from the float64 mean
__global__ void __launch_bounds__(256) groupnorm_stats_kernel(int npix, int C, int G, const float* __restrict__ x, int ld,
                                                              float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ double sh[256];
    const int g = blockIdx.x, img = blockIdx.y, cg = C / G, n = npix * cg, t = threadIdx.x;
    const float* xb = x + (long long)img * npix * ld + g * cg;
    double s = 0.0;
    for (int e = t; e < n; e += 256) {
        const int p = e / cg, c = e - p * cg;
        s += (double)xb[(long long)p * ld + c];
    }
    const double m = ag_block_sum(s, sh) / (double)n;
    double q = 0.0;
    for (int e = t; e < n; e += 256) {
        const int p = e / cg, c = e - p * cg;
        const double d = (double)xb[(long long)p * ld + c] - m;
        q += d * d;
    }
    const double var = ag_block_sum(q, sh) / (double)n;
    if (t == 0) {
        mean[img * G + g] = (float)m;
        rstd[img * G + g] = (float)(1.0 / sqrt(var + AG_EPS));
    }
}

__device__ __forceinline__ float ag_norm(float x, float m, float r, float gamma, float beta) { return fmaf((x - m) * r, gamma, beta); }

__global__ void __launch_bounds__(256) groupnorm_relu_kernel(long long total, int B, int npix, int C, int G, const float* __restrict__ x,
                                                             int ldx, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ out, int ldo) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long row = e / C;
    const int c = (int)(e - row * C), img = (int)(row / npix), level = img / B, g = c / (C / G);
    const float v = ag_norm(x[row * ldx + c], mean[img * G + g], rstd[img * G + g], gamma[level * C + c], beta[level * C + c]);
    out[row * ldo + c] = fmaxf(v, 0.0f);
}

// ---------------------------------------------------------------------------------------------------------------- mix
struct mix_args {
    int L, B, npix, C, G;
    unsigned identity;                                      // bit l: level l has no shortcut convolution, ys[l] is added as it is
    const float* y3; int ld3; const float* ys; int lds;
    const float *mean3, *rstd3, *gamma3, *beta3, *means, *rstds, *gammas, *betas, *mix;
    float* out; int ldo;
};

__global__ void __launch_bounds__(256) agg_mix_kernel(long long total, mix_args a) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long row = e / a.C;                          // b * npix + p
    const int c = (int)(e - row * a.C), b = (int)(row / a.npix), g = c / (a.C / a.G);
    const long long level_rows = (long long)a.B * a.npix;
    float acc = 0.0f;
    for (int l = 0; l < a.L; ++l) {
        const int sg = (l * a.B + b) * a.G + g, pc = l * a.C + c;
        const long long r = l * level_rows + row;
        const float v3 = ag_norm(a.y3[r * a.ld3 + c], a.mean3[sg], a.rstd3[sg], a.gamma3[pc], a.beta3[pc]);
        const float ys = a.ys[r * a.lds + c];
        const float vs = ((a.identity >> l) & 1u) ? ys : ag_norm(ys, a.means[sg], a.rstds[sg], a.gammas[pc], a.betas[pc]);
        const float term = __fmul_rn(a.mix[l], fmaxf(__fadd_rn(v3, vs), 0.0f));
        acc = l == 0 ? term : __fadd_rn(acc, term);         // the first term is assigned, the rest are added
    }
    a.out[row * a.ldo + c] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- conv3x3
struct conv_args {
    int B, Ph, Pw, Cin, Cout, K;
    const float* x; int ldx; const float* w; float* out; int ldo;
};

// row of the 32 x 32 accumulator block that register `reg` of a lane in half `h` holds (the column is lane & 31)
__device__ __forceinline__ int cv_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__global__ void __launch_bounds__(256) conv3x3_kernel(conv_args a) {
    __shared__ float As[CV_KC * CV_LD], Bs[CV_KC * CV_LD];
    const int img = blockIdx.z, level = img / a.B, row0 = blockIdx.y * CV_T, col0 = blockIdx.x * CV_T, npix = a.Ph * a.Pw;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int kk = t & 31, r8 = t >> 5;
    float ra[8], rb[8];
    // a thread stages column kk of the pixels / weight rows r8 + 8 i: their coordinates are fixed for the kernel
    int py[8], px[8];
    unsigned rmask = 0, cmask = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = row0 + r8 + 8 * i;
        py[i] = px[i] = 0;
        if (p < npix) { rmask |= 1u << i; py[i] = p / a.Pw; px[i] = p - py[i] * a.Pw; }
        if (col0 + r8 + 8 * i < a.Cout) cmask |= 1u << i;
    }
    const float* xi = a.x + (long long)img * npix * a.ldx;
    const float* wl = a.w + ((long long)level * a.Cout + col0 + r8) * a.K;
    const long long wstep = 8LL * a.K;
    auto fetch = [&](int k0) {
        const int k = k0 + kk;
        const bool kin = k < a.K;
        const int tap = kin ? k / a.Cin : 0, c = k - tap * a.Cin, dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int yy = py[i] + dy, xx = px[i] + dx;
            const bool in = kin && ((rmask >> i) & 1u) && yy >= 0 && yy < a.Ph && xx >= 0 && xx < a.Pw;
            ra[i] = in ? xi[((long long)yy * a.Pw + xx) * a.ldx + c] : 0.f;          // a padding tap contributes nothing
            rb[i] = (kin && ((cmask >> i) & 1u)) ? wl[i * wstep + k] : 0.f;
        }
    };
    ag_f32x16 acc = {0};
    fetch(0);
    for (int k0 = 0; k0 < a.K; k0 += CV_KC) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            As[kk * CV_LD + r8 + 8 * i] = ra[i];
            Bs[kk * CV_LD + r8 + 8 * i] = rb[i];
        }
        __syncthreads();
        if (k0 + CV_KC < a.K) fetch(k0 + CV_KC);
#pragma unroll
        for (int s = 0; s < CV_KC / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * s + h) * CV_LD + 32 * wr + r], Bs[(2 * s + h) * CV_LD + 32 * wc + r], acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = col0 + 32 * wc + r;
    if (col >= a.Cout) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = row0 + 32 * wr + cv_row(reg, h);
        if (row < npix) a.out[((long long)img * npix + row) * a.ldo + col] = acc[reg];
    }
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int dm_agg_gather_f32(dm_ctx* ctx, int n_src, const long long* desc, const void* src0, const void* src1, const void* src2,
                                 const void* src3, const void* src4, const void* src5, const void* src6, const void* src7, int R, int B,
                                 int P_h, int P_w, double step_deg, float* out, int ld) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, n_src >= 1 && n_src <= AG_MAX_SRC, "one to eight sources");
    DM_REQUIRE(ctx, R >= 1 && R <= AG_MAX_ROT, "1 <= R <= 16 rotations");
    DM_REQUIRE(ctx, B > 0 && B <= 65535 && P_h > 0 && P_w > 0 && P_h <= 16384 && P_w <= 16384, "sizes must be positive, B <= 65535, P <= 16384");
    DM_REQUIRE(ctx, desc && out, "null pointer");
    DM_REQUIRE(ctx, isfinite(step_deg), "the rotation step must be finite");
    const void* src[AG_MAX_SRC] = {src0, src1, src2, src3, src4, src5, src6, src7};
    gather_args a{};
    a.n_src = n_src; a.R = R; a.B = B; a.Ph = P_h; a.Pw = P_w; a.ld = ld; a.identity = step_deg == 0.0; a.out = out;
    for (int r = 0; r < R; ++r) {
        const double th = (-(double)r * step_deg) * (M_PI / 180.0);
        a.cs[r] = cos(th);
        a.sn[r] = sin(th);
    }
    long long width = 0, tiles = 0;
    for (int s = 0; s < n_src; ++s) {
        const long long* d = desc + 8 * s;
        DM_REQUIRE(ctx, src[s] != nullptr, "null source");
        DM_REQUIRE(ctx, d[0] > 0 && d[1] > 0 && d[2] > 0 && d[0] <= (1 << 24) && d[1] <= 16384 && d[2] <= 16384, "a source needs C, h, w > 0");
        DM_REQUIRE(ctx, d[3] >= 0 && d[4] >= 0 && d[5] >= 0 && d[6] >= 0, "source strides must not be negative");
        DM_REQUIRE(ctx, d[7] == DM_F16 || d[7] == DM_F32, "source dtype: DM_F16 or DM_F32");
        ag_src& q = a.s[s];
        q.p = src[s]; q.C = (int)d[0]; q.h = (int)d[1]; q.w = (int)d[2]; q.dtype = (int)d[7]; q.off = (int)width;
        q.tiles = dm_cdiv(q.C, AG_TILE);
        q.si = d[3]; q.sc = d[4]; q.sy = d[5]; q.sx = d[6];
        width += q.C;
        tiles += q.tiles;
    }
    DM_REQUIRE(ctx, width <= (1 << 24) && ld >= (int)width, "ld >= the summed source widths");
    DM_REQUIRE(ctx, tiles <= 65535, "too many channel tiles");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DM_LAUNCH(ctx, "agg_gather", agg_gather_kernel, dim3(dm_cdiv(P_h * P_w, AG_TILE), (int)tiles, B), dim3(256), 0, a);
    return DM_OK;
}

extern "C" int dm_groupnorm_stats_f32(dm_ctx* ctx, int n_img, int npix, int C, int G, const float* x, int ld, float* mean, float* rstd) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, n_img > 0 && npix > 0 && C > 0 && G > 0 && n_img <= 65535, "sizes must be positive, n_img <= 65535");
    DM_REQUIRE(ctx, C % G == 0, "C must be a multiple of G");
    DM_REQUIRE(ctx, (long long)npix * (C / G) < (1LL << 31), "npix * C / G < 2^31");
    DM_REQUIRE(ctx, ld >= C, "ld >= C");
    DM_REQUIRE(ctx, x && mean && rstd, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DM_LAUNCH(ctx, "groupnorm_stats", groupnorm_stats_kernel, dim3(G, n_img), dim3(256), 0, npix, C, G, x, ld, mean, rstd);
    return DM_OK;
}

extern "C" int dm_groupnorm_relu_f32(dm_ctx* ctx, int n_img, int B, int npix, int C, int G, const float* x, int ldx, const float* mean,
                                     const float* rstd, const float* gamma, const float* beta, float* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, n_img > 0 && B > 0 && npix > 0 && C > 0 && G > 0, "sizes must be positive");
    DM_REQUIRE(ctx, n_img % B == 0, "n_img = L * B");
    DM_REQUIRE(ctx, C % G == 0, "C must be a multiple of G");
    DM_REQUIRE(ctx, ldx >= C && ldo >= C, "ldx >= C, ldo >= C");
    DM_REQUIRE(ctx, x && mean && rstd && gamma && beta && out, "null pointer");
    const long long total = (long long)n_img * npix * C;
    DM_REQUIRE(ctx, (total + 255) / 256 < (1LL << 31), "n_img * npix * C");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DM_LAUNCH(ctx, "groupnorm_relu", groupnorm_relu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, total, B, npix, C, G, x, ldx,
              mean, rstd, gamma, beta, out, ldo);
    return DM_OK;
}

extern "C" int dm_conv3x3_f32(dm_ctx* ctx, int L, int B, int P_h, int P_w, int C_in, int C_out, const float* x, int ldx, const float* w,
                              float* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, L > 0 && B > 0 && P_h > 0 && P_w > 0 && C_in > 0 && C_out > 0, "sizes must be positive");
    DM_REQUIRE(ctx, (long long)L * B <= 65535 && P_h <= 16384 && P_w <= 16384 && C_in <= (1 << 24) && C_out <= (1 << 24), "L * B <= 65535, P <= 16384");
    DM_REQUIRE(ctx, 9LL * C_in < (1LL << 28), "9 C_in");
    DM_REQUIRE(ctx, ldx >= C_in && ldo >= C_out, "ldx >= C_in, ldo >= C_out");
    DM_REQUIRE(ctx, x && w && out, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    conv_args a{B, P_h, P_w, C_in, C_out, 9 * C_in, x, ldx, w, out, ldo};
    DM_LAUNCH(ctx, "conv3x3", conv3x3_kernel, dim3(dm_cdiv(C_out, CV_T), dm_cdiv(P_h * P_w, CV_T), L * B), dim3(256), 0, a);
    return DM_OK;
}

extern "C" int dm_agg_mix_f32(dm_ctx* ctx, int L, int B, int npix, int C, int G, const float* y3, int ld3, const float* ys, int lds,
                              const float* mean3, const float* rstd3, const float* gamma3, const float* beta3, const float* means,
                              const float* rstds, const float* gammas, const float* betas, unsigned identity_mask, const float* mix,
                              float* out, int ldo) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, L > 0 && B > 0 && npix > 0 && C > 0 && G > 0, "sizes must be positive");
    DM_REQUIRE(ctx, L <= 32 && (L == 32 || (identity_mask >> L) == 0), "at most 32 levels, identity_mask within them");
    DM_REQUIRE(ctx, C % G == 0, "C must be a multiple of G");
    DM_REQUIRE(ctx, ld3 >= C && lds >= C && ldo >= C, "ld3 >= C, lds >= C, ldo >= C");
    DM_REQUIRE(ctx, y3 && ys && mean3 && rstd3 && gamma3 && beta3 && means && rstds && gammas && betas && mix && out, "null pointer");
    const long long total = (long long)B * npix * C;
    DM_REQUIRE(ctx, (total + 255) / 256 < (1LL << 31) && (long long)L * B * G < (1LL << 31) && (long long)L * C < (1LL << 31), "B * npix * C");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    mix_args a{L, B, npix, C, G, identity_mask, y3, ld3, ys, lds, mean3, rstd3, gamma3, beta3, means, rstds, gammas, betas, mix, out, ldo};
    DM_LAUNCH(ctx, "agg_mix", agg_mix_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, total, a);
    return DM_OK;
}

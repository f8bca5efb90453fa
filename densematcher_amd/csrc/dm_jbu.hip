// Guided (joint bilateral) feature upsampling, one 2x stage of FeatUp's JBUStack: dm_jbu_filters_f32 (the combined 7 x 7 kernel of
// every output pixel from the guidance image) and dm_jbu_apply (bicubic 2x upsampling of the source, reflect padding by 3 and the
// adaptive convolution with those kernels, fused: neither the upsampled nor the padded source is ever stored).
//
// Reference computation replaced: third_party/featup/featup/upsamplers.py
//   213-221   get_range_kernel: range_proj (1x1 conv 3 -> 32, GELU, 1x1 conv 32 -> 32), reflect padding, the 49 products of the centre
//             key with its neighbourhood, temperature, softmax
//   223-228   get_spatial_kernel (evaluated on the host with the reference's expressions, passed as 49 numbers)
//   238-243   times the spatial kernel, normalisation with the 1e-7 clamp, + 0.1 fixup_proj(cat[kernel, guidance])
//   245-249   bicubic upsampling (align_corners=False, A = -0.75), reflect padding, AdaptiveConv (adaptive_conv_cuda: tap order i, j)
//
// Filters: two passes.  jbu_keys writes the 32-wide key of every pixel ONCE to the workspace (128 bytes per pixel, pixel-major);
// jbu_filters, one thread per pixel, re-reads its 49 reflected neighbours from there as float4 (they come from L2: a pixel's key is read
// by 49 threads of the same or a neighbouring workgroup).  Staging the key map with its halo in LDS instead would recompute
// (22 / 16)^2 = 1.9 x the keys for a 16 x 16 tile and cost 62 KB of LDS.  The fixup network runs as ONE rolled loop over its 49 hidden
// units: unit k is 52 FMAs on the thread's statically indexed inputs, one GELU, and 49 FMAs into the statically indexed outputs
// (the second layer is stored transposed), so no per-thread array is indexed at run time.  Weights are read from LDS at a
// wave-uniform address (broadcast).
//
// Apply: one workgroup per (view, 16 x 32 output pixels, chunk of channels), 256 threads, each thread the two pixels (2 ty, tx) and
// (2 ty + 1, tx) and FOUR channels at a time.  The 2 x 49 filter values of a thread stay in registers for the whole channel loop.
// Per four channels the workgroup (1) loads the source window (at most 16 x 24 texels, clamped indices) into LDS as float4 (the four
// channels of a texel side by side), (2) interpolates along x into the 38 padded columns, (3) along y into the 22 padded rows --
// P[22][38] float4, the reflect padding being a remap of the row / column read -- and (4) every thread walks its 8 x 7 window of P:
// 56 ds_read_b128 feed 2 x 49 x 4 = 392 FMAs, 7 FMAs per LDS instruction.  A pixel's sum is the fmaf chain over i (outer), j (inner)
// in its own thread: no atomics, no sums across threads, so its bits depend on its own view alone, whatever the batch, the chunking
// of the channels or the layout of source and output.
// All memory operations are vector loads and stores.
#include <math.h>

#include "dm_jbu_common.h"

namespace {
constexpr int JB_KEY = 32;          // key_dim of JBULearnedRange
// the packed parameter block of one stage, in floats (densematch.h)
constexpr int PB_RP_W1 = 0, PB_RP_B1 = 96, PB_RP_W2 = 128, PB_RP_B2 = 1152, PB_FX_W1 = 1184, PB_FX_B1 = 3732, PB_FX_W2T = 3784,
              PB_FX_B2 = 6332, PB_SPATIAL = 6384, PB_TEMP = 6436, PB_SIZE = 6440;
constexpr int PB_KEYS_SIZE = PB_FX_W1;      // what jbu_keys reads of it

constexpr int AP_TY = 16, AP_TX = 32;                       // output pixels of a workgroup
constexpr int AP_PR = AP_TY + 2 * JB_R, AP_PC = AP_TX + 2 * JB_R;      // the padded window: 22 x 38
constexpr int AP_SR = AP_TY / 2 + 8, AP_SC = AP_TX / 2 + 8;            // the source window: at most 16 x 24
constexpr int AP_CB = 4;                                    // channels per pass

__device__ __forceinline__ float jb_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// ---------------------------------------------------------------------------------------------------------------- keys
// keys[b][p][:] = W2 gelu(W1 g + b1) + b2, g = guidance[b][:, p]
__global__ void __launch_bounds__(256) jbu_keys_kernel(int HW, const float* __restrict__ guid, const float* __restrict__ params,
                                                       float* __restrict__ keys) {
    __shared__ float pb[PB_KEYS_SIZE];
    for (int q = threadIdx.x; q < PB_KEYS_SIZE; q += blockDim.x) pb[q] = params[q];
    __syncthreads();
    const int p = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (p >= HW) return;
    const float* g = guid + (size_t)b * 3 * HW + p;
    const float g0 = g[0], g1 = g[HW], g2 = g[2 * (size_t)HW];
    float hid[JB_KEY];
#pragma unroll
    for (int o = 0; o < JB_KEY; ++o)
        hid[o] = jb_gelu(fmaf(pb[PB_RP_W1 + 3 * o + 2], g2, fmaf(pb[PB_RP_W1 + 3 * o + 1], g1, fmaf(pb[PB_RP_W1 + 3 * o], g0, pb[PB_RP_B1 + o]))));
    float4* out = reinterpret_cast<float4*>(keys + ((size_t)b * HW + p) * JB_KEY);
    for (int o4 = 0; o4 < JB_KEY / 4; ++o4) {
        float r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float* w = pb + PB_RP_W2 + (o4 * 4 + q) * JB_KEY;
            float s = pb[PB_RP_B2 + o4 * 4 + q];
#pragma unroll
            for (int k = 0; k < JB_KEY; ++k) s = fmaf(w[k], hid[k], s);
            r[q] = s;
        }
        out[o4] = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- filters
__global__ void __launch_bounds__(256) jbu_filters_kernel(int H, int W, const float* __restrict__ guid, const float* __restrict__ params,
                                                          const float* __restrict__ keys, float* __restrict__ filt) {
    __shared__ float pb[PB_SIZE - PB_FX_W1];                 // fixup weights, spatial kernel, temperature
    for (int q = threadIdx.x; q < PB_SIZE - PB_FX_W1; q += blockDim.x) pb[q] = params[PB_FX_W1 + q];
    __syncthreads();
    const float* fx_w1 = pb;
    const float* fx_b1 = pb + (PB_FX_B1 - PB_FX_W1);
    const float* fx_w2t = pb + (PB_FX_W2T - PB_FX_W1);
    const float* fx_b2 = pb + (PB_FX_B2 - PB_FX_W1);
    const float* spatial = pb + (PB_SPATIAL - PB_FX_W1);
    const float temp = pb[PB_TEMP - PB_FX_W1];
    const int HW = H * W, p = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (p >= HW) return;
    const int y = p / W, x = p % W;
    const float* kb = keys + (size_t)b * HW * JB_KEY;
    float4 kc[JB_KEY / 4];
    {
        const float4* c = reinterpret_cast<const float4*>(kb + (size_t)p * JB_KEY);
#pragma unroll
        for (int q = 0; q < JB_KEY / 4; ++q) kc[q] = c[q];
    }
    // in[0..48]: the kernel; in[49..51]: the guidance
    float in[JB_T + 3];
    float top = -INFINITY;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int yy = jb_reflect(y + i - JB_R, H);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int xx = jb_reflect(x + j - JB_R, W);
            const float4* n = reinterpret_cast<const float4*>(kb + ((size_t)yy * W + xx) * JB_KEY);
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;      // four chains over c = 0, 1, 2, 3 mod 4, then (s0 + s1) + (s2 + s3)
#pragma unroll
            for (int q = 0; q < JB_KEY / 4; ++q) {
                const float4 v = n[q];
                s0 = fmaf(v.x, kc[q].x, s0); s1 = fmaf(v.y, kc[q].y, s1); s2 = fmaf(v.z, kc[q].z, s2); s3 = fmaf(v.w, kc[q].w, s3);
            }
            float s = ((s0 + s1) + (s2 + s3)) * temp;
            in[i * 7 + j] = s;
            top = fmaxf(top, s);
        }
    }
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < JB_T; ++t) { in[t] = expf(in[t] - top); sum += in[t]; }
    float total = 0.0f;
#pragma unroll
    for (int t = 0; t < JB_T; ++t) { in[t] = (in[t] / sum) * spatial[t]; total += in[t]; }
    total = fmaxf(total, 1e-7f);
#pragma unroll
    for (int t = 0; t < JB_T; ++t) in[t] /= total;
    const float* g = guid + (size_t)b * 3 * HW + p;
    in[JB_T] = g[0]; in[JB_T + 1] = g[HW]; in[JB_T + 2] = g[2 * (size_t)HW];
    float acc[JB_T];
#pragma unroll
    for (int t = 0; t < JB_T; ++t) acc[t] = fx_b2[t];
    for (int k = 0; k < JB_T; ++k) {                         // hidden unit k of fixup_proj, then its column of the second layer
        const float* w1 = fx_w1 + k * (JB_T + 3);
        float h = fx_b1[k];
#pragma unroll
        for (int t = 0; t < JB_T + 3; ++t) h = fmaf(w1[t], in[t], h);
        h = jb_gelu(h);
        const float* w2 = fx_w2t + k * (JB_T + 3);
#pragma unroll
        for (int t = 0; t < JB_T; ++t) acc[t] = fmaf(w2[t], h, acc[t]);
    }
    float* o = filt + ((size_t)b * HW + p) * JB_T;
#pragma unroll
    for (int t = 0; t < JB_T; ++t) o[t] = fmaf(0.1f, acc[t], in[t]);
}

// ---------------------------------------------------------------------------------------------------------------- apply
struct apply_args {
    int C, h, w, H, W, tiles_x, c_chunk;
    const void* src; long long sb, sc, sy, sx;      // element strides (view, channel, row, col)
    const float* filt;
    void* out; long long ob, oc, oy, ox;
};

template <typename TS, typename TO>
__global__ void __launch_bounds__(256, 3) jbu_apply_kernel(apply_args a) {
    __shared__ float4 S[AP_SR * AP_SC];       // source window, four channels per texel
    __shared__ float4 Hx[AP_SR * AP_PC];      // interpolated along x
    __shared__ float4 P[AP_PR * AP_PC];       // the padded, upsampled window
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int b = blockIdx.z, Y0 = (blockIdx.x / a.tiles_x) * AP_TY, X0 = (blockIdx.x % a.tiles_x) * AP_TX;
    const int c_first = blockIdx.y * a.c_chunk, c_last = min(a.C, c_first + a.c_chunk);
    // padded rows / columns that hold something: pr < n_pr, pc < n_pc; the rest of P is zero
    const int n_pr = min(AP_TY, a.H - Y0) + 2 * JB_R, n_pc = min(AP_TX, a.W - X0) + 2 * JB_R;
    // upsampled rows read, after reflection, lie in [u_lo, u_hi]; their source taps in [s_lo, s_hi], at most AP_SR (AP_SC) of them
    const int uy_lo = max(0, Y0 - JB_R), uy_hi = min(a.H - 1, Y0 + n_pr - 1 - JB_R);
    const int ux_lo = max(0, X0 - JB_R), ux_hi = min(a.W - 1, X0 + n_pc - 1 - JB_R);
    const int sy_lo = max(0, (uy_lo >> 1) - 2), sy_n = min(min(a.h - 1, (uy_hi >> 1) + 2) - sy_lo + 1, AP_SR);
    const int sx_lo = max(0, (ux_lo >> 1) - 2), sx_n = min(min(a.w - 1, (ux_hi >> 1) + 2) - sx_lo + 1, AP_SC);

    // the thread's two pixels and their kernels
    const int x = X0 + tx, y0 = Y0 + 2 * ty;
    const bool live0 = x < a.W && y0 < a.H, live1 = x < a.W && y0 + 1 < a.H;
    float f0[JB_T], f1[JB_T];
    {
        const float* fb = a.filt + ((size_t)b * a.H * a.W) * JB_T;
        const float* q0 = fb + ((size_t)(live0 ? y0 : 0) * a.W + (live0 ? x : 0)) * JB_T;
        const float* q1 = fb + ((size_t)(live1 ? y0 + 1 : 0) * a.W + (live1 ? x : 0)) * JB_T;
#pragma unroll
        for (int t = 0; t < JB_T; ++t) { f0[t] = live0 ? q0[t] : 0.0f; f1[t] = live1 ? q1[t] : 0.0f; }
    }
    const TS* src = reinterpret_cast<const TS*>(a.src) + (long long)b * a.sb;
    TO* out = reinterpret_cast<TO*>(a.out) + (long long)b * a.ob;
    float* Sf = reinterpret_cast<float*>(S);

    // the source window of a pass, AP_SR * AP_SC * AP_CB / 256 = 6 values per thread at most: element e = tid + 256 k is channel
    // e & 3 of texel e >> 2 where the channels lie side by side in memory (channels-last), else texel e % n_tex of channel e / n_tex.
    // The values of the NEXT pass are fetched into registers while this pass computes.
    constexpr int AP_PRE = AP_SR * AP_SC * AP_CB / 256;
    const int n_tex = sy_n * sx_n;
    const bool chan_fastest = a.sc == 1;
    float pre[AP_PRE];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int k = 0; k < AP_PRE; ++k) {
            const int e = tid + 256 * k;
            const int ch = chan_fastest ? (e & 3) : e / n_tex, t = chan_fastest ? (e >> 2) : e % n_tex, r = t / sx_n, q = t % sx_n;
            float v = 0.0f;
            if (e < n_tex * AP_CB && c0 + ch < c_last)
                v = jb_load(src + (long long)(c0 + ch) * a.sc + (long long)(sy_lo + r) * a.sy + (long long)(sx_lo + q) * a.sx);
            pre[k] = v;
        }
    };
    fetch(c_first);
    for (int c0 = c_first; c0 < c_last; c0 += AP_CB) {
        // (1) source window: S[r][q].ch = src[c0 + ch][sy_lo + r][sx_lo + q], zero for a channel past the end
#pragma unroll
        for (int k = 0; k < AP_PRE; ++k) {
            const int e = tid + 256 * k;
            const int ch = chan_fastest ? (e & 3) : e / n_tex, t = chan_fastest ? (e >> 2) : e % n_tex, r = t / sx_n, q = t % sx_n;
            if (e < n_tex * AP_CB) Sf[(r * AP_SC + q) * 4 + ch] = pre[k];
        }
        if (c0 + AP_CB < c_last) fetch(c0 + AP_CB);
        __syncthreads();
        // (2) along x: Hx[r][pc] = sum_q w_q S[r][tap_q(u)], u = reflect(X0 + pc - 3)
#pragma unroll 1
        for (int e = tid; e < sy_n * AP_PC; e += 256) {
            const int r = e / AP_PC, pc = e % AP_PC;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (pc < n_pc) {
                int tap[4]; float wt[4];
                jb_taps(jb_reflect(X0 + pc - JB_R, a.W), a.w, tap, wt);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 s = S[r * AP_SC + min(max(tap[q] - sx_lo, 0), AP_SC - 1)];
                    if (q == 0) v = make_float4(wt[0] * s.x, wt[0] * s.y, wt[0] * s.z, wt[0] * s.w);
                    else v = make_float4(fmaf(wt[q], s.x, v.x), fmaf(wt[q], s.y, v.y), fmaf(wt[q], s.z, v.z), fmaf(wt[q], s.w, v.w));
                }
            }
            Hx[r * AP_PC + pc] = v;
        }
        __syncthreads();
        // (3) along y: P[pr][pc] = sum_q w_q Hx[tap_q(u)][pc], u = reflect(Y0 + pr - 3)
#pragma unroll 1
        for (int e = tid; e < AP_PR * AP_PC; e += 256) {
            const int pr = e / AP_PC, pc = e % AP_PC;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (pr < n_pr && pc < n_pc) {
                int tap[4]; float wt[4];
                jb_taps(jb_reflect(Y0 + pr - JB_R, a.H), a.h, tap, wt);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 s = Hx[min(max(tap[q] - sy_lo, 0), AP_SR - 1) * AP_PC + pc];
                    if (q == 0) v = make_float4(wt[0] * s.x, wt[0] * s.y, wt[0] * s.z, wt[0] * s.w);
                    else v = make_float4(fmaf(wt[q], s.x, v.x), fmaf(wt[q], s.y, v.y), fmaf(wt[q], s.z, v.z), fmaf(wt[q], s.w, v.w));
                }
            }
            P[e] = v;
        }
        __syncthreads();
        // (4) the two pixels of the thread: rows 2 ty .. 2 ty + 7 of P, columns tx .. tx + 6
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const float4 v = P[(2 * ty + i) * AP_PC + tx + j];
                if (i < 7) {
                    const float f = f0[i * 7 + j];
                    r0.x = fmaf(f, v.x, r0.x); r0.y = fmaf(f, v.y, r0.y); r0.z = fmaf(f, v.z, r0.z); r0.w = fmaf(f, v.w, r0.w);
                }
                if (i > 0) {
                    const float f = f1[(i - 1) * 7 + j];
                    r1.x = fmaf(f, v.x, r1.x); r1.y = fmaf(f, v.y, r1.y); r1.z = fmaf(f, v.z, r1.z); r1.w = fmaf(f, v.w, r1.w);
                }
            }
            // pin this row's sums here: without it the compiler sinks all 392 FMAs into the guarded stores below and keeps the 56
            // reads (224 registers) in flight
            asm volatile("" : "+v"(r0.x), "+v"(r0.y), "+v"(r0.z), "+v"(r0.w), "+v"(r1.x), "+v"(r1.y), "+v"(r1.z), "+v"(r1.w) : : "memory");
        }
        const float o0[4] = {r0.x, r0.y, r0.z, r0.w}, o1[4] = {r1.x, r1.y, r1.z, r1.w};
#pragma unroll
        for (int ch = 0; ch < AP_CB; ++ch) {
            if (c0 + ch >= c_last) break;
            TO* oc = out + (long long)(c0 + ch) * a.oc + (long long)x * a.ox;
            if (live0) jb_store(oc + (long long)y0 * a.oy, o0[ch]);
            if (live1) jb_store(oc + (long long)(y0 + 1) * a.oy, o1[ch]);
        }
        // the next pass overwrites S and Hx before its first barrier, P only after two more: no barrier is needed here for S and Hx
        // (every thread is past (3)), and P is rewritten only after the barriers of (1) and (2), which every thread reaches after (4)
    }
}

// true when no two index tuples of a tensor of these extents and element strides address the same element
bool jb_strides_distinct(const long long* ext, const long long* st, int n) {
    int order[4] = {0, 1, 2, 3};
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (st[order[j]] < st[order[i]]) { int t = order[i]; order[i] = order[j]; order[j] = t; }
    long long span = 1;                                       // elements covered by the dimensions seen so far
    for (int i = 0; i < n; ++i) {
        const int d = order[i];
        if (ext[d] == 1) continue;
        if (st[d] < span) return false;
        span = st[d] * (ext[d] - 1) + span;
    }
    return true;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int dm_jbu_filters_f32(dm_ctx* ctx, int B, int H, int W, const float* guidance, const float* params, float* filters) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && B <= 65535, "1 <= B <= 65535");
    DM_REQUIRE(ctx, H >= 4 && W >= 4 && H <= 16384 && W <= 16384, "4 <= H, W <= 16384: the reflection by 3 must stay inside the image");
    DM_REQUIRE(ctx, guidance && params && filters, "null pointer");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t key_bytes = (size_t)B * H * W * JB_KEY * sizeof(float);
    if (int rc = dm_ws_reserve(ctx, dm_align_up(key_bytes))) return rc;
    float* keys = (float*)dm_ws_take(ctx, key_bytes);
    if (!keys) return dm_fail(ctx, DM_ENOMEM, "dm_jbu_filters_f32: the key map does not fit the workspace");
    const dim3 grid(dm_cdiv(H * W, 256), B);
    DM_LAUNCH(ctx, "jbu_keys", jbu_keys_kernel, grid, dim3(256), 0, H * W, guidance, params, keys);
    DM_LAUNCH(ctx, "jbu_filters", jbu_filters_kernel, grid, dim3(256), 0, H, W, guidance, params, (const float*)keys, filters);
    return DM_OK;
}

extern "C" int dm_jbu_apply(dm_ctx* ctx, int B, int C, int h, int w, int src_dtype, const void* src, long long s_view, long long s_chan,
                            long long s_row, long long s_col, const float* filters, int out_dtype, void* out, long long o_view,
                            long long o_chan, long long o_row, long long o_col) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && C > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, h >= 2 && w >= 2 && h <= 8192 && w <= 8192, "2 <= h, w <= 8192: the output (2h, 2w) needs H, W >= 4");
    DM_REQUIRE(ctx, src_dtype == DM_F16 || src_dtype == DM_F32, "src_dtype: DM_F16 or DM_F32");
    DM_REQUIRE(ctx, out_dtype == DM_F16 || out_dtype == DM_F32, "out_dtype: DM_F16 or DM_F32");
    DM_REQUIRE(ctx, src && filters && out, "null pointer");
    DM_REQUIRE(ctx, s_view >= 0 && s_chan >= 0 && s_row >= 0 && s_col >= 0, "source strides must not be negative");
    const int H = 2 * h, W = 2 * w;
    const long long ext[4] = {B, C, H, W}, ost[4] = {o_view, o_chan, o_row, o_col};
    DM_REQUIRE(ctx, o_view > 0 && o_chan > 0 && o_row > 0 && o_col > 0 && jb_strides_distinct(ext, ost, 4),
               "output strides must be positive and give every element its own address");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int tiles_x = dm_cdiv(W, AP_TX), tiles = tiles_x * dm_cdiv(H, AP_TY);
    // channels per workgroup: all of them when the tiles alone fill the chip (the kernels of a tile are then read once), else chunks
    // of a multiple of four so that about 2048 workgroups exist; a pixel's bits do not depend on the choice
    int quads = dm_cdiv(C, AP_CB), chunks = 1;
    if ((long long)tiles * B < 2048) chunks = (int)min((long long)quads, (2048 + (long long)tiles * B - 1) / ((long long)tiles * B));
    chunks = min(chunks, 65535);
    const int c_chunk = dm_cdiv(quads, chunks) * AP_CB;
    chunks = dm_cdiv(C, c_chunk);
    apply_args a{C, h, w, H, W, tiles_x, c_chunk, src, s_view, s_chan, s_row, s_col, filters, out, o_view, o_chan, o_row, o_col};
    const dim3 grid(tiles, chunks, B);
    if (src_dtype == DM_F16 && out_dtype == DM_F32) DM_LAUNCH(ctx, "jbu_apply", (jbu_apply_kernel<__half, float>), grid, dim3(256), 0, a);
    else if (src_dtype == DM_F32 && out_dtype == DM_F32) DM_LAUNCH(ctx, "jbu_apply", (jbu_apply_kernel<float, float>), grid, dim3(256), 0, a);
    else if (src_dtype == DM_F16) DM_LAUNCH(ctx, "jbu_apply", (jbu_apply_kernel<__half, __half>), grid, dim3(256), 0, a);
    else DM_LAUNCH(ctx, "jbu_apply", (jbu_apply_kernel<float, __half>), grid, dim3(256), 0, a);
    return DM_OK;
}

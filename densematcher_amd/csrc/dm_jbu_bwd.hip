// Backward of dm_jbu_apply (dm_jbu.hip), the two kernels FeatUp ships next to its forward (third_party/featup/featup/adaptive_conv_cuda/
// adaptive_conv_kernel.cu: adaptive_conv_grad_filters_kernel, adaptive_conv_grad_input_kernel), here fused with the adjoint of the
// reflect padding and of the bicubic upsampling, as the forward fuses those: neither P = reflect_pad_3(bicubic_2x(src)) nor its
// gradient ever reaches memory.  Per axis P = A src with A of (2 n + 6) x n and at most four non-zeros per row; out = filters * P.
//
// dm_jbu_apply_bwd_filters_f32: gfilt[b,y,x,7i+j] = sum_c gout[b,c,y,x] P[b,c,y+i,x+j].  The forward's workgroup: 16 x 32 output
// pixels, 256 threads, each thread the pixels (2 ty, tx) and (2 ty + 1, tx); P of four channels is rebuilt in LDS exactly as
// jbu_apply_kernel builds it (same taps, same fmaf chains, so the same bits), and the thread's 2 x 49 sums stay in registers for the
// whole channel loop, each an fmaf chain over ascending channels.  Small stages are a handful of tiles: below BF_MIN_TILES tiles the
// channels are split into chunks -- a function of (C, h, w) alone --, every chunk writes its partial sums to the workspace and
// jbu_bwdf_reduce_kernel adds them in ascending chunk order.  A pixel's bits therefore depend on (C, h, w) and its own view only.
//
// dm_jbu_apply_bwd_source_f32: gsrc = Ay^T gP Ax per (view, channel), gP[u,v] = sum_{i,j} gout[u-i,v-j] filters[u-i,v-j,7i+j] on the
// padded grid (the reference's grad_input).  One workgroup per (view, tile of BS_T x BS_T source texels, chunk of channels), 1024
// threads, FOUR channels per pass.  The texels s0 .. s0 + 9 of an axis are fed by the upsampled indices 2 s0 - 3 .. 2 s0 + 22 (at
// most 26), those by the padded indices u + 3 and, at a border, by the reflected 3 - u (u = 1 .. 3) and 2 N + 1 - u (u = N - 4 ..
// N - 2): a CONTIGUOUS run of at most 32 padded indices (bs_window: the worst case is the first tile of an image of 13 texels).  Each
// thread owns one pixel of that 32 x 32 padded window and keeps its 49 "transposed" kernel values filters[u-i,v-j,7i+j] in registers
// across the channel loop.  Per pass: (1) the 38 x 38 window of gout into LDS as float4 of four channels, zero outside the image;
// (2) gP, 49 ds_read_b128 and 196 FMAs per thread, an fmaf chain over i (outer), j (inner); (3), (4) the reflection folded as a
// gather along y, then along x: every upsampled index adds its one to three padded indices in ascending order; (5), (6) the bicubic
// adjoint as a gather along x, then y: a texel adds its eight candidate upsampled indices 2 s - 3 .. 2 s + 4 in ascending order with
// the weight table built once per workgroup (the sum of the weights of the clamped taps that land on the texel; exact, the weights
// being multiples of 2^-8).  Everything is a gather inside LDS with a fixed order: no atomics, no sums across workgroups, so a
// texel's bits depend on its own view alone, whatever the batch and the chunking of the channels.  LDS: 23.1 KB (gout window, then
// the row fold) + 16 KB (gP, then the x adjoint) + 10.6 KB (the folded window) + 0.6 KB of weights.
// All memory operations are vector loads and stores.
#include "dm_jbu_common.h"

namespace {
// ---------------------------------------------------------------------------------------------------------------- gfilt
constexpr int AP_TY = 16, AP_TX = 32;                       // output pixels of a workgroup: the forward's tile
constexpr int AP_PR = AP_TY + 2 * JB_R, AP_PC = AP_TX + 2 * JB_R;
constexpr int AP_SR = AP_TY / 2 + 8, AP_SC = AP_TX / 2 + 8;
constexpr int AP_CB = 4;                                    // channels per pass
constexpr int BF_MIN_TILES = 64, BF_MAX_CHUNKS = 16;        // the channel split of the small stages

struct bwdf_args {
    int C, h, w, H, W, tiles_x, c_chunk;
    const void* src; long long sb, sc, sy, sx;      // element strides (view, channel, row, col)
    const float* gout; long long gb, gc, gy, gx;
    float* dst; long long dst_chunk;                // gfilt itself, or the partial sums: chunk q at dst + q * dst_chunk
};

template <typename TS>
__global__ void __launch_bounds__(256, 2) jbu_bwd_filters_kernel(bwdf_args a) {
    __shared__ float4 S[AP_SR * AP_SC];       // source window, four channels per texel
    __shared__ float4 Hx[AP_SR * AP_PC];      // interpolated along x
    __shared__ float4 P[AP_PR * AP_PC];       // the padded, upsampled window
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int b = blockIdx.z, Y0 = (blockIdx.x / a.tiles_x) * AP_TY, X0 = (blockIdx.x % a.tiles_x) * AP_TX;
    const int c_first = blockIdx.y * a.c_chunk, c_last = min(a.C, c_first + a.c_chunk);
    // the windows of jbu_apply_kernel
    const int n_pr = min(AP_TY, a.H - Y0) + 2 * JB_R, n_pc = min(AP_TX, a.W - X0) + 2 * JB_R;
    const int uy_lo = max(0, Y0 - JB_R), uy_hi = min(a.H - 1, Y0 + n_pr - 1 - JB_R);
    const int ux_lo = max(0, X0 - JB_R), ux_hi = min(a.W - 1, X0 + n_pc - 1 - JB_R);
    const int sy_lo = max(0, (uy_lo >> 1) - 2), sy_n = min(min(a.h - 1, (uy_hi >> 1) + 2) - sy_lo + 1, AP_SR);
    const int sx_lo = max(0, (ux_lo >> 1) - 2), sx_n = min(min(a.w - 1, (ux_hi >> 1) + 2) - sx_lo + 1, AP_SC);

    const int x = X0 + tx, y0 = Y0 + 2 * ty;
    const bool live0 = x < a.W && y0 < a.H, live1 = x < a.W && y0 + 1 < a.H;
    float f0[JB_T], f1[JB_T];                 // the sums of the thread's two pixels
#pragma unroll
    for (int t = 0; t < JB_T; ++t) { f0[t] = 0.0f; f1[t] = 0.0f; }
    const TS* src = reinterpret_cast<const TS*>(a.src) + (long long)b * a.sb;
    const float* gout = a.gout + (long long)b * a.gb + (long long)x * a.gx;
    float* Sf = reinterpret_cast<float*>(S);

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
        // the upstream gradient of the two pixels, four channels; zero for a dead pixel and for a channel past the end
        float g0[AP_CB], g1[AP_CB];
#pragma unroll
        for (int ch = 0; ch < AP_CB; ++ch) {
            const bool c_ok = c0 + ch < c_last;
            const float* gc = gout + (long long)(c0 + ch) * a.gc;
            g0[ch] = (live0 && c_ok) ? gc[(long long)y0 * a.gy] : 0.0f;
            g1[ch] = (live1 && c_ok) ? gc[(long long)(y0 + 1) * a.gy] : 0.0f;
        }
        // (1) source window
#pragma unroll
        for (int k = 0; k < AP_PRE; ++k) {
            const int e = tid + 256 * k;
            const int ch = chan_fastest ? (e & 3) : e / n_tex, t = chan_fastest ? (e >> 2) : e % n_tex, r = t / sx_n, q = t % sx_n;
            if (e < n_tex * AP_CB) Sf[(r * AP_SC + q) * 4 + ch] = pre[k];
        }
        if (c0 + AP_CB < c_last) fetch(c0 + AP_CB);
        __syncthreads();
        // (2) along x
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
        // (3) along y
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
        // (4) the 2 x 49 sums: rows 2 ty .. 2 ty + 7 of P, columns tx .. tx + 6; channels in ascending order
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const float4 v = P[(2 * ty + i) * AP_PC + tx + j];
                if (i < 7) f0[i * 7 + j] = fmaf(g0[3], v.w, fmaf(g0[2], v.z, fmaf(g0[1], v.y, fmaf(g0[0], v.x, f0[i * 7 + j]))));
                if (i > 0) f1[(i - 1) * 7 + j] = fmaf(g1[3], v.w, fmaf(g1[2], v.z, fmaf(g1[1], v.y, fmaf(g1[0], v.x, f1[(i - 1) * 7 + j]))));
            }
        }
        // as in the forward, no barrier here: S and Hx are rewritten before the next pass's first barrier by threads that are past
        // (3), P only after two more barriers
    }
    float* d = a.dst + (long long)blockIdx.y * a.dst_chunk + ((size_t)b * a.H * a.W) * JB_T;
    if (live0) {
        float* o = d + ((size_t)y0 * a.W + x) * JB_T;
#pragma unroll
        for (int t = 0; t < JB_T; ++t) o[t] = f0[t];
    }
    if (live1) {
        float* o = d + ((size_t)(y0 + 1) * a.W + x) * JB_T;
#pragma unroll
        for (int t = 0; t < JB_T; ++t) o[t] = f1[t];
    }
}

// gfilt = ((part_0 + part_1) + part_2) + ..., n4 float4 per chunk
__global__ void __launch_bounds__(256) jbu_bwdf_reduce_kernel(long long n4, int chunks, const float4* __restrict__ part, float4* __restrict__ gfilt) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n4) return;
    float4 s = part[e];
    for (int q = 1; q < chunks; ++q) {
        const float4 v = part[q * n4 + e];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    gfilt[e] = s;
}

// ---------------------------------------------------------------------------------------------------------------- gsrc
constexpr int BS_T = 10;                      // source texels of a workgroup, per axis
constexpr int BS_NU = 2 * BS_T + 6;           // upsampled indices that feed them: at most 26
constexpr int BS_NP = 2 * BS_T + 12;          // padded indices that feed those: at most 32
constexpr int BS_NG = BS_NP + 2 * JB_R;       // output pixels whose kernels reach those: 38
constexpr int BS_THREADS = BS_NP * BS_NP;     // one thread per padded pixel
constexpr int BS_CB = 4;                      // channels per pass

struct bwds_args {
    int C, h, w, H, W, tiles_x, c_chunk;
    const float* gout; long long gb, gc, gy, gx;    // element strides (view, channel, row, col)
    const float* filt;
    float* gsrc;
};

// One axis of a tile: the texels s0 .. s0 + ns - 1 of n, the upsampled indices u_lo .. u_lo + nu - 1 of N = 2 n that feed them and
// the first padded index p_lo of the run that feeds those.  The run ends at u_hi + 3, or at N + 5 when u_hi >= N - 4 (the reflected
// far border); it starts at u_lo + 3, or at 0 when u_lo <= 3 (only the first tile, BS_T being above 3).  At most BS_NP long: the first
// tile reaches N + 5 only for n <= 13 (2 n + 6 <= 32), a later one only for n <= s0 + 13 (2 n + 6 - 2 s0 <= 32), any other run is 26.
struct bs_axis { int s0, ns, u_lo, nu, p_lo; };
__device__ __forceinline__ bs_axis bs_window(int tile, int n) {
    bs_axis r;
    r.s0 = tile * BS_T;
    r.ns = min(BS_T, n - r.s0);
    r.u_lo = max(0, 2 * r.s0 - 3);
    r.nu = min(2 * n - 1, 2 * (r.s0 + r.ns - 1) + 4) - r.u_lo + 1;
    r.p_lo = r.u_lo <= 3 ? 0 : r.u_lo + 3;
    return r;
}

__device__ __forceinline__ float4 bs_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 bs_fma(float w, float4 v, float4 s) {
    return make_float4(fmaf(w, v.x, s.x), fmaf(w, v.y, s.y), fmaf(w, v.z, s.z), fmaf(w, v.w, s.w));
}

// the padded indices that land on upsampled index u of N (forward: P[p] = U[reflect(p - 3)]), in ascending order, relative to p_lo
__device__ __forceinline__ int bs_folds(int u, int N, int p_lo, int* p) {
    int n = 0;
    if (u >= 1 && u <= 3) p[n++] = 3 - u - p_lo;
    p[n++] = u + 3 - p_lo;
    if (u >= N - 4 && u <= N - 2) p[n++] = 2 * N + 1 - u - p_lo;
    return n;
}

__global__ void __launch_bounds__(BS_THREADS) jbu_bwd_source_kernel(bwds_args a) {
    __shared__ float4 A[BS_NG * BS_NG];       // (1) the window of gout; (3) the row fold, BS_NU x BS_NP
    __shared__ float4 Bf[BS_NP * BS_NP];      // (2) gP; (5) the adjoint along x, BS_NU x BS_T
    __shared__ float4 U[BS_NU * BS_NU];       // (4) the gradient of the upsampled window
    __shared__ float wgt[2][BS_T][8];         // [axis][texel][k]: the weight of upsampled index 2 s - 3 + k on texel s
    const int tid = threadIdx.x, lx = tid % BS_NP, ly = tid / BS_NP;
    const int b = blockIdx.z;
    const bs_axis wy = bs_window(blockIdx.x / a.tiles_x, a.h), wx = bs_window(blockIdx.x % a.tiles_x, a.w);
    const int c_first = blockIdx.y * a.c_chunk, c_last = min(a.C, c_first + a.c_chunk);

    if (tid < 2 * BS_T * 8) {
        const int axis = tid / (BS_T * 8), sl = (tid / 8) % BS_T, k = tid % 8;
        const int n = axis ? a.w : a.h, s = (axis ? wx.s0 : wy.s0) + sl, u = 2 * s - 3 + k;
        float sum = 0.0f;
        if (s < n && u >= 0 && u < 2 * n) {
            int tap[4]; float wt[4];
            jb_taps(u, n, tap, wt);
#pragma unroll
            for (int q = 0; q < 4; ++q) sum += tap[q] == s ? wt[q] : 0.0f;
        }
        wgt[axis][sl][k] = sum;
    }
    // the thread's padded pixel (py, px) and the kernel values that reach it: tap (i, j) of output pixel (py - i, px - j)
    float tf[JB_T];
    {
        const int py = wy.p_lo + ly, px = wx.p_lo + lx;
        const float* fb = a.filt + ((size_t)b * a.H * a.W) * JB_T;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const int y = py - i, x = px - j;
                const bool ok = y >= 0 && y < a.H && x >= 0 && x < a.W;
                tf[i * 7 + j] = ok ? fb[((size_t)y * a.W + x) * JB_T + i * 7 + j] : 0.0f;
            }
        }
    }
    const float* gout = a.gout + (long long)b * a.gb;
    float* Af = reinterpret_cast<float*>(A);
    const bool chan_fastest = a.gc == 1;
    const int gy0 = wy.p_lo - 2 * JB_R, gx0 = wx.p_lo - 2 * JB_R;      // the output pixel of A[0][0]

    for (int c0 = c_first; c0 < c_last; c0 += BS_CB) {
        // (1) A[r][q].ch = gout[c0 + ch][gy0 + r][gx0 + q], zero outside the image and for a channel past the end
#pragma unroll 1
        for (int e = tid; e < BS_NG * BS_NG * BS_CB; e += BS_THREADS) {
            const int ch = chan_fastest ? (e & 3) : e / (BS_NG * BS_NG), t = chan_fastest ? (e >> 2) : e % (BS_NG * BS_NG);
            const int y = gy0 + t / BS_NG, x = gx0 + t % BS_NG;
            float v = 0.0f;
            if (y >= 0 && y < a.H && x >= 0 && x < a.W && c0 + ch < c_last)
                v = gout[(long long)(c0 + ch) * a.gc + (long long)y * a.gy + (long long)x * a.gx];
            Af[t * 4 + ch] = v;
        }
        __syncthreads();
        // (2) gP of the thread's pixel
        {
            float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int i = 0; i < 7; ++i) {
#pragma unroll
                for (int j = 0; j < 7; ++j) s = bs_fma(tf[i * 7 + j], A[(ly + 2 * JB_R - i) * BS_NG + lx + 2 * JB_R - j], s);
                // pin this row's sums here: 1024 threads leave 128 registers each, 49 of them hold tf, and without it the compiler
                // keeps all 49 reads (196 registers) in flight and spills
                asm volatile("" : "+v"(s.x), "+v"(s.y), "+v"(s.z), "+v"(s.w) : : "memory");
            }
            Bf[tid] = s;
        }
        __syncthreads();
        // (3) the reflection along y: A[lu][q] = sum of the padded rows that land on upsampled row u_lo + lu
        for (int e = tid; e < wy.nu * BS_NP; e += BS_THREADS) {
            const int lu = e / BS_NP, q = e % BS_NP;
            int p[3];
            const int n = bs_folds(wy.u_lo + lu, a.H, wy.p_lo, p);
            float4 s = Bf[p[0] * BS_NP + q];
            for (int k = 1; k < n; ++k) s = bs_add(s, Bf[p[k] * BS_NP + q]);
            A[e] = s;
        }
        __syncthreads();
        // (4) the reflection along x
        for (int e = tid; e < wy.nu * wx.nu; e += BS_THREADS) {
            const int lu = e / wx.nu, lv = e % wx.nu;
            int p[3];
            const int n = bs_folds(wx.u_lo + lv, a.W, wx.p_lo, p);
            float4 s = A[lu * BS_NP + p[0]];
            for (int k = 1; k < n; ++k) s = bs_add(s, A[lu * BS_NP + p[k]]);
            U[lu * BS_NU + lv] = s;
        }
        __syncthreads();
        // (5) the bicubic adjoint along x: Bf[lu][sl] = sum_k wgt[1][sl][k] U[lu][2 s - 3 + k]; a zero weight stands for an index
        // outside the image, whose read is clamped into the window
        for (int e = tid; e < wy.nu * wx.ns; e += BS_THREADS) {
            const int lu = e / wx.ns, sl = e % wx.ns, first = 2 * (wx.s0 + sl) - 3 - wx.u_lo;
            float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int k = 0; k < 8; ++k) s = bs_fma(wgt[1][sl][k], U[lu * BS_NU + min(max(first + k, 0), wx.nu - 1)], s);
            Bf[lu * BS_T + sl] = s;
        }
        __syncthreads();
        // (6) along y, and the texels of four channels
        for (int e = tid; e < wy.ns * wx.ns; e += BS_THREADS) {
            const int sly = e / wx.ns, slx = e % wx.ns, first = 2 * (wy.s0 + sly) - 3 - wy.u_lo;
            float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int k = 0; k < 8; ++k) s = bs_fma(wgt[0][sly][k], Bf[min(max(first + k, 0), wy.nu - 1) * BS_T + slx], s);
            const float o[4] = {s.x, s.y, s.z, s.w};
            float* g = a.gsrc + (((size_t)b * a.C + c0) * a.h + wy.s0 + sly) * a.w + wx.s0 + slx;
#pragma unroll
            for (int ch = 0; ch < BS_CB; ++ch)
                if (c0 + ch < c_last) g[(size_t)ch * a.h * a.w] = o[ch];
        }
        // the next pass rewrites A after (4) read it, Bf after (6) read it and U after (5) read it, each behind at least one barrier
        // that every thread passes after those reads: A behind (4)'s and (5)'s, Bf behind the next (1)'s, U behind the next three
    }
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int dm_jbu_apply_bwd_filters_f32(dm_ctx* ctx, int B, int C, int h, int w, int src_dtype, const void* src, long long s_view,
                                            long long s_chan, long long s_row, long long s_col, const float* gout, long long g_view,
                                            long long g_chan, long long g_row, long long g_col, float* gfilt) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && C > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, h >= 2 && w >= 2 && h <= 8192 && w <= 8192, "2 <= h, w <= 8192: the output (2h, 2w) needs H, W >= 4");
    DM_REQUIRE(ctx, src_dtype == DM_F16 || src_dtype == DM_F32, "src_dtype: DM_F16 or DM_F32");
    DM_REQUIRE(ctx, src && gout && gfilt, "null pointer");
    DM_REQUIRE(ctx, s_view >= 0 && s_chan >= 0 && s_row >= 0 && s_col >= 0, "source strides must not be negative");
    DM_REQUIRE(ctx, g_view >= 0 && g_chan >= 0 && g_row >= 0 && g_col >= 0, "gout strides must not be negative");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int H = 2 * h, W = 2 * w;
    const int tiles_x = dm_cdiv(W, AP_TX), tiles = tiles_x * dm_cdiv(H, AP_TY);
    // the channel split: a function of (C, h, w) alone
    const int quads = dm_cdiv(C, AP_CB);
    int chunks = tiles >= BF_MIN_TILES ? 1 : min(min(quads, dm_cdiv(BF_MIN_TILES, tiles)), BF_MAX_CHUNKS);
    const int c_chunk = dm_cdiv(quads, chunks) * AP_CB;
    chunks = dm_cdiv(C, c_chunk);
    const long long n = (long long)B * H * W * JB_T;             // a multiple of four: H and W are even
    float* dst = gfilt;
    if (chunks > 1) {
        const size_t bytes = (size_t)chunks * n * sizeof(float);
        if (int rc = dm_ws_reserve(ctx, dm_align_up(bytes))) return rc;
        dst = (float*)dm_ws_take(ctx, bytes);
        if (!dst) return dm_fail(ctx, DM_ENOMEM, "dm_jbu_apply_bwd_filters_f32: the partial sums do not fit the workspace");
    }
    bwdf_args a{C, h, w, H, W, tiles_x, c_chunk, src, s_view, s_chan, s_row, s_col, gout, g_view, g_chan, g_row, g_col, dst, chunks > 1 ? n : 0};
    const dim3 grid(tiles, chunks, B);
    if (src_dtype == DM_F16) DM_LAUNCH(ctx, "jbu_bwd_filters", (jbu_bwd_filters_kernel<__half>), grid, dim3(256), 0, a);
    else DM_LAUNCH(ctx, "jbu_bwd_filters", (jbu_bwd_filters_kernel<float>), grid, dim3(256), 0, a);
    if (chunks > 1)
        DM_LAUNCH(ctx, "jbu_bwd_filters_reduce", jbu_bwdf_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, n / 4, chunks,
                  (const float4*)dst, (float4*)gfilt);
    return DM_OK;
}

extern "C" int dm_jbu_apply_bwd_source_f32(dm_ctx* ctx, int B, int C, int h, int w, const float* gout, long long g_view, long long g_chan,
                                           long long g_row, long long g_col, const float* filters, float* gsrc) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && C > 0 && B <= 65535, "sizes must be positive, B <= 65535");
    DM_REQUIRE(ctx, h >= 2 && w >= 2 && h <= 8192 && w <= 8192, "2 <= h, w <= 8192: the output (2h, 2w) needs H, W >= 4");
    DM_REQUIRE(ctx, gout && filters && gsrc, "null pointer");
    DM_REQUIRE(ctx, g_view >= 0 && g_chan >= 0 && g_row >= 0 && g_col >= 0, "gout strides must not be negative");
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int tiles_x = dm_cdiv(w, BS_T), tiles = tiles_x * dm_cdiv(h, BS_T);
    // channels per workgroup: chunks of a multiple of four so that about 1024 workgroups exist; a texel's bits do not depend on it
    int quads = dm_cdiv(C, BS_CB), chunks = 1;
    if ((long long)tiles * B < 1024) chunks = (int)min((long long)quads, (1024 + (long long)tiles * B - 1) / ((long long)tiles * B));
    chunks = min(chunks, 65535);
    const int c_chunk = dm_cdiv(quads, chunks) * BS_CB;
    chunks = dm_cdiv(C, c_chunk);
    bwds_args a{C, h, w, 2 * h, 2 * w, tiles_x, c_chunk, gout, g_view, g_chan, g_row, g_col, filters, gsrc};
    DM_LAUNCH(ctx, "jbu_bwd_source", jbu_bwd_source_kernel, dim3(tiles, chunks, B), dim3(BS_THREADS), 0, a);
    return DM_OK;
}

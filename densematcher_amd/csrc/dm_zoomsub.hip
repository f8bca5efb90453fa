// Subsampled ("fast") ZoomOut: what dm_zoomout_sub adds to the loop of dm_zoomout.hip.
//
// Reference: pyFM/refine/zoomout.py:95-113 with subsample = (sub1, sub2): the iterations run on Phi1[sub1], Phi2[sub2] with the
// least-squares p2p_to_FM (no mass, convert.py:51), the final vertex map on all vertices.
//   C_{k+step} = argmin |Phi2s[:, :k'] X - Phi1s[p21, :k']|_F   <=>   (Phi2s^T Phi2s)[:k', :k'] X = Phi2s[:, :k']^T Phi1s[p21, :k']
// Phi2s does not change during a call, so the Gram matrix G is formed once at the final size kf, and because the Cholesky factor
// of a leading principal block is the leading block of the Cholesky factor, ONE factorisation G = L L^T serves every iteration:
// iteration k' solves with L[:k', :k'].  The same holds for the inverses of the 16 x 16 diagonal blocks of L (the inverse of a
// leading block of a triangular matrix is the leading block of its inverse), so a partial last block needs nothing but a mask.
//
//   zo_sub_gather     Phi1[sub1], Phi2[sub2] -> contiguous (B, ns, Kpad) copies; an index outside the mesh sets info bit 2 (and is
//                     clamped: nothing downstream reads outside its arrays)
//   zo_sub_factor     in-place blocked right-looking Cholesky of the B Gram matrices in global memory, one workgroup per pair,
//                     the current panel staged in LDS; keeps W_J = L_JJ^-1.  info bit 1: a pivot at or below 1e-10 of its
//                     diagonal entry (fewer samples than kf, duplicated samples: cond(Phi2s) beyond 1e5 is refused, not solved)
//   zo_sub_pack       the factor and the W_J once more, block by block in the lane order the solve's matrix instructions read
//   zo_sub_solve      per iteration: L_k L_k^T C = R on the float64 matrix cores, one wave per 16 right-hand sides; the solution
//                     blocks never leave the wave's registers (a 16 x 16 result block of v_mfma_f64_16x16x4_f64 is, register by
//                     register, the B operand of the next product when the contraction index is walked as (lane >> 4) + 4 r)
// Every sum runs in an order fixed by the sizes alone: a pair's numbers do not depend on the batch it is in.
#include "dm_gemm_f64.h"
#include "dm_internal.h"

namespace {

template <typename TR>
__global__ __launch_bounds__(256) void zo_sub_gather_kernel(int N, int ns, int kf, int Kpad, const TR* __restrict__ Phi, int ld,
                                                           const int32_t* __restrict__ sub, TR* __restrict__ out, int32_t* __restrict__ info) {
    const int b = blockIdx.y;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)ns * Kpad) return;
    const int r = (int)(e / Kpad), c = (int)(e - (long long)r * Kpad);
    int v = sub[(long long)b * ns + r];
    if (v < 0 || v >= N) {
        if (c == 0) atomicOr(info + b, 2);
        v = min(max(v, 0), N - 1);
    }
    out[((long long)b * ns + r) * Kpad + c] = c < kf ? Phi[((long long)b * N + v) * ld + c] : (TR)0;
}

__global__ __launch_bounds__(256) void zo_sub_iota_ones_kernel(int ns, int B, int32_t* __restrict__ iota, double* __restrict__ ones) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)B * ns) return;
    iota[e] = (int32_t)(e % ns);
    ones[e] = 1.0;
}

constexpr int ZS_MAXK = 256;           // largest final map size
constexpr double ZS_PIVOT_REL = 1e-10;

// G (B, Kpad, Kpad) in place: on return its lower triangle holds L (the strict upper triangle keeps what the product left
// there and is never read), W (B, Kpad / 16, 256) the inverses of L's diagonal blocks, row-major.
__global__ __launch_bounds__(256) void zo_sub_factor_kernel(int kf, int Kpad, double* G, double* __restrict__ W, int32_t* __restrict__ info) {
    __shared__ double a[16][17];
    __shared__ double x[16][17];
    __shared__ double pan[ZS_MAXK][17];
    __shared__ double gd[ZS_MAXK];
    __shared__ int flag;
    const int b = blockIdx.x, t = threadIdx.x;
    double* A = G + (size_t)b * Kpad * Kpad;
    double* Wb = W + (size_t)b * Kpad * 16;
    const int NB = Kpad / 16;
    if (t == 0) flag = 0;
    // rows / columns beyond kf: identity (they decouple exactly)
    for (int e = t; e < Kpad * Kpad; e += 256) {
        const int i = e / Kpad, c = e - i * Kpad;
        if (i >= kf || c >= kf) A[e] = (i == c) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (t < Kpad) gd[t] = A[(size_t)t * Kpad + t];
    __syncthreads();
    for (int J = 0; J < NB; ++J) {
        const int j0 = 16 * J;
        {   // diagonal block: factor in LDS (one column per barrier), then invert
            const int i = t >> 4, c = t & 15;
            a[i][c] = A[(size_t)(j0 + i) * Kpad + j0 + c];
            __syncthreads();
            for (int j = 0; j < 16; ++j) {
                double d = a[j][j];
                const bool ok = d > ZS_PIVOT_REL * gd[j0 + j] && d < DM_INF_F64;
                if (!ok) { d = 1.0; if (t == 0) flag = 1; }
                const double r = 1.0 / sqrt(d);
                const double lij = a[i][j] * r, lcj = a[c][j] * r;
                __syncthreads();
                if (i > j && c > j && c <= i) a[i][c] -= lij * lcj;
                if (c == j && i > j) a[i][j] = lij;
                if (i == j && c == j) a[j][j] = sqrt(d);
                __syncthreads();
            }
            if (t < 16) {                                          // X = L_JJ^-1, column t by forward substitution
                for (int r = 0; r < t; ++r) x[r][t] = 0.0;
                for (int r = t; r < 16; ++r) {
                    double s = (r == t) ? 1.0 : 0.0;
                    for (int m = t; m < r; ++m) s -= a[r][m] * x[m][t];
                    x[r][t] = s / a[r][r];
                }
            }
            __syncthreads();
            A[(size_t)(j0 + i) * Kpad + j0 + c] = c <= i ? a[i][c] : 0.0;
            Wb[(size_t)J * 256 + i * 16 + c] = x[i][c];
        }
        const int rem = Kpad - j0 - 16;                            // rows below the block
        // panel: L_IJ = A_IJ L_JJ^-T, i.e. L[i][j0 + c] = sum_m A[i][j0 + m] W[c][m]
        for (int e = t; e < rem * 16; e += 256) {
            const int i = e >> 4, c = e & 15;
            const double* row = A + (size_t)(j0 + 16 + i) * Kpad + j0;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 16; ++m) s = fma(row[m], x[c][m], s);
            pan[i][c] = s;
        }
        __syncthreads();
        for (int e = t; e < rem * 16; e += 256) {
            const int i = e >> 4, c = e & 15;
            A[(size_t)(j0 + 16 + i) * Kpad + j0 + c] = pan[i][c];
        }
        // trailing update of the lower triangle: A[i][c] -= sum_m L[i][j0 + m] L[c][j0 + m]
        for (int e = t; e < rem * rem; e += 256) {
            const int i = e / rem, c = e - i * rem;
            if (c > i) continue;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 16; ++m) s = fma(pan[i][m], pan[c][m], s);
            A[(size_t)(j0 + 16 + i) * Kpad + j0 + 16 + c] -= s;
        }
        __syncthreads();
    }
    if (t == 0 && flag) atomicOr(info + b, 1);
}

// The factor as the solve reads it: one 2 KiB slot per 16 x 16 block of the lower block triangle, block (I, J) at slot I (I + 1) / 2 + J,
// holding for lane l its four A-operand entries of v_mfma_f64_16x16x4_f64 side by side (one 32-byte load per lane and block, the
// whole slot one contiguous run), with the contraction index walked as kk = (l >> 4) + 4 r so that a result block feeds the next
// product register by register:
//   Lf  forward substitution:  block (I, J), I > J: A[m][kk] = L[16 I + m][16 J + kk];   (J, J): W_J[m][kk]      (m = l & 15)
//   Lb  back substitution:     block (J, K), J > K: A[m][kk] = L[16 J + kk][16 K + m];   (J, J): W_J[kk][m]
__global__ __launch_bounds__(256) void zo_sub_pack_kernel(int Kpad, int nslots, const double* __restrict__ L, const double* __restrict__ W,
                                                         double* __restrict__ Lf, double* __restrict__ Lb) {
    const int slot = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= slot) ++I;
    const int J = slot - I * (I + 1) / 2;
    const int lane = t >> 2, r = t & 3, m = lane & 15, kk = (lane >> 4) + 4 * r;
    const double* Lp = L + (size_t)b * Kpad * Kpad;
    const double* Wp = W + (size_t)b * Kpad * 16 + (size_t)I * 256;
    const size_t o = ((size_t)b * nslots + slot) * 256 + t;
    if (I == J) {
        Lf[o] = Wp[m * 16 + kk];
        Lb[o] = Wp[kk * 16 + m];
    } else {
        Lf[o] = Lp[(size_t)(16 * I + m) * Kpad + 16 * J + kk];
        Lb[o] = Lp[(size_t)(16 * I + kk) * Kpad + 16 * J + m];
    }
}

// C[:k, :k] = (L_k L_k^T)^-1 R[:k, :k].  grid (ceil(k / 16), B), one wave each: 16 columns of the right-hand side.
// Block J of the wave's columns is x[J]: register r of lane l holds row 16 J + (l >> 4) + 4 r, column l & 15.
// Only the last block row can be partial (k not a multiple of 16): its operand entries beyond k are masked to zero.
template <int NBMAX>
__global__ __launch_bounds__(64) void zo_sub_solve_kernel(int k, int Kpad, int nslots, const double* __restrict__ Lf, const double* __restrict__ Lb,
                                                         const double* __restrict__ R, double* __restrict__ C, int ldc, long long strideC) {
    const int b = blockIdx.y, lane = threadIdx.x, l15 = lane & 15, g = lane >> 4;
    const int NB = (k + 15) >> 4;
    const f64x4* F = reinterpret_cast<const f64x4*>(Lf + (size_t)b * nslots * 256) + lane;
    const f64x4* Bk = reinterpret_cast<const f64x4*>(Lb + (size_t)b * nslots * 256) + lane;
    const double* Rb = R + (size_t)b * Kpad * Kpad;
    const int col = blockIdx.x * 16 + l15;
    const int last = 16 * (NB - 1);
    const bool m_ok = last + l15 < k;                              // this lane's m in the last block row
    bool kk_ok[4];                                                 // this lane's kk = g + 4 r in the last block row
#pragma unroll
    for (int r = 0; r < 4; ++r) kk_ok[r] = last + g + 4 * r < k;
    f64x4 x[NBMAX];
#pragma unroll
    for (int J = 0; J < NBMAX; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * J + g + 4 * r;
            x[J][r] = (row < k && col < k) ? Rb[(size_t)row * Kpad + col] : 0.0;
        }
    // forward: y_J = W_J x_J, then x_I -= L_IJ y_J for I > J
#pragma unroll
    for (int J = 0; J < NBMAX; ++J) {
        if (J < NB) {
            f64x4 w = F[(J * (J + 1) / 2 + J) * 64];
            if (J == NB - 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (m_ok && kk_ok[r]) ? w[r] : 0.0;
            }
            f64x4 y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r) y = mfma_f64_16x16x4(w[r], x[J][r], y);
            x[J] = y;
#pragma unroll
            for (int I = J + 1; I < NBMAX; ++I) {
                if (I < NB) {
                    f64x4 a = F[(I * (I + 1) / 2 + J) * 64];
                    if (I == NB - 1) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) a[r] = m_ok ? a[r] : 0.0;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[I] = mfma_f64_16x16x4(-a[r], y[r], x[I]);
                }
            }
        }
    }
    // back: c_J = W_J^T x_J, then x_K -= L_JK^T c_J for K < J
#pragma unroll
    for (int J = NBMAX - 1; J >= 0; --J) {
        if (J < NB) {
            f64x4 w = Bk[(J * (J + 1) / 2 + J) * 64];
            if (J == NB - 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (m_ok && kk_ok[r]) ? w[r] : 0.0;
            }
            f64x4 y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r) y = mfma_f64_16x16x4(w[r], x[J][r], y);
            x[J] = y;
#pragma unroll
            for (int K = 0; K < J; ++K) {
                f64x4 a = Bk[(J * (J + 1) / 2 + K) * 64];
                if (J == NB - 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[r] = kk_ok[r] ? a[r] : 0.0;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) x[K] = mfma_f64_16x16x4(-a[r], y[r], x[K]);
            }
        }
    }
    double* Cb = C + (size_t)b * strideC;
#pragma unroll
    for (int J = 0; J < NBMAX; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * J + g + 4 * r;
            if (row < k && col < k) Cb[(size_t)row * ldc + col] = x[J][r];
        }
}

static inline int zs_pad16(int v) { return (v + 15) / 16 * 16; }

}  // namespace

size_t dm_zo_sub_ws_bytes(int B, int n1s, int n2s, int kf, int real_bytes) {
    const int Kpad = zs_pad16(kf);
    return dm_align_up((size_t)B * n1s * Kpad * real_bytes) + dm_align_up((size_t)B * n2s * Kpad * real_bytes) +
           2 * dm_align_up((size_t)B * Kpad * Kpad * 8) + dm_align_up((size_t)B * Kpad * 16 * 8) + dm_align_up((size_t)B * n2s * 8) +
           dm_align_up((size_t)B * n2s * 4) + dm_p2pfm_ws_bytes(B, n2s, kf, kf) + 8192 +
           2 * dm_align_up((size_t)B * ((Kpad / 16) * (Kpad / 16 + 1) / 2) * 256 * 8);
}

template <typename TR>
int dm_zo_sub_setup(dm_ctx* ctx, int B, int n1s, int n2s, int kf, const TR* Phi1, int ld1, const TR* Phi2, int ld2, dm_zo_sub* s,
                    const TR** Phi1s, const TR** Phi2s) {
    const int Kpad = zs_pad16(kf);
    TR* P1 = (TR*)dm_ws_take(ctx, (size_t)B * n1s * Kpad * sizeof(TR));
    TR* P2 = (TR*)dm_ws_take(ctx, (size_t)B * n2s * Kpad * sizeof(TR));
    double* L = (double*)dm_ws_take(ctx, (size_t)B * Kpad * Kpad * 8);
    double* R = (double*)dm_ws_take(ctx, (size_t)B * Kpad * Kpad * 8);
    double* W = (double*)dm_ws_take(ctx, (size_t)B * Kpad * 16 * 8);
    double* ones = (double*)dm_ws_take(ctx, (size_t)B * n2s * 8);
    int32_t* iota = (int32_t*)dm_ws_take(ctx, (size_t)B * n2s * 4);
    const int nslots = (Kpad / 16) * (Kpad / 16 + 1) / 2;
    double* Lf = (double*)dm_ws_take(ctx, (size_t)B * nslots * 256 * 8);
    double* Lb = (double*)dm_ws_take(ctx, (size_t)B * nslots * 256 * 8);
    if (!P1 || !P2 || !L || !R || !W || !ones || !iota || !Lf || !Lb) return dm_fail(ctx, DM_ENOMEM, "zoomout_sub: workspace not reserved");
    DM_LAUNCH(ctx, "zo_sub_gather", zo_sub_gather_kernel<TR>, dim3((unsigned)(((long long)n1s * Kpad + 255) / 256), B), dim3(256), 0, s->N1, n1s, kf,
              Kpad, Phi1, ld1, s->sub1, P1, s->info);
    DM_LAUNCH(ctx, "zo_sub_gather", zo_sub_gather_kernel<TR>, dim3((unsigned)(((long long)n2s * Kpad + 255) / 256), B), dim3(256), 0, s->N2, n2s, kf,
              Kpad, Phi2, ld2, s->sub2, P2, s->info);
    DM_LAUNCH(ctx, "zo_sub_iota_ones", zo_sub_iota_ones_kernel, dim3((unsigned)(((long long)B * n2s + 255) / 256)), dim3(256), 0, n2s, B, iota, ones);
    DM_CHECK_HIP(ctx, hipMemsetAsync(L, 0, (size_t)B * Kpad * Kpad * 8, ctx->stream));
    DM_CHECK_HIP(ctx, hipMemsetAsync(R, 0, (size_t)B * Kpad * Kpad * 8, ctx->stream));
    const size_t mark = ctx->ws_off;
    int rc = dm_launch_p2p_to_fm<TR>(ctx, B, n2s, n2s, kf, kf, iota, P2, Kpad, P2, Kpad, ones, L, Kpad, (long long)Kpad * Kpad);
    if (rc) return rc;
    ctx->ws_off = mark;                                            // (the product's scratch is free again: stream order)
    DM_LAUNCH(ctx, "zo_sub_factor", zo_sub_factor_kernel, dim3(B), dim3(256), 0, kf, Kpad, L, W, s->info);
    DM_LAUNCH(ctx, "zo_sub_pack", zo_sub_pack_kernel, dim3(nslots, B), dim3(256), 0, Kpad, nslots, (const double*)L, (const double*)W, Lf, Lb);
    s->Lf = Lf; s->Lb = Lb; s->nslots = nslots; s->R = R; s->ones = ones; s->Kpad = Kpad;
    *Phi1s = P1; *Phi2s = P2;
    return DM_OK;
}
template int dm_zo_sub_setup<float>(dm_ctx*, int, int, int, int, const float*, int, const float*, int, dm_zo_sub*, const float**, const float**);
template int dm_zo_sub_setup<double>(dm_ctx*, int, int, int, int, const double*, int, const double*, int, dm_zo_sub*, const double**, const double**);

int dm_zo_sub_solve(dm_ctx* ctx, int B, int k, const dm_zo_sub& s, double* C, int ldc, long long strideC) {
    const int NB = dm_cdiv(k, 16);
    const dim3 grid(NB, B);
#define ZS_CASE(M_)                                                                                                                       \
    if (NB <= M_) {                                                                                                                       \
        DM_LAUNCH(ctx, "zo_sub_solve", zo_sub_solve_kernel<M_>, grid, dim3(64), 0, k, s.Kpad, s.nslots, (const double*)s.Lf, (const double*)s.Lb, \
                  (const double*)s.R, C, ldc, strideC);                                                                                   \
        return DM_OK;                                                                                                                     \
    }
    ZS_CASE(4) ZS_CASE(8) ZS_CASE(13) ZS_CASE(16)
#undef ZS_CASE
    return dm_fail(ctx, DM_EINVAL, "zoomout_sub: map size %d beyond 256", k);
}

// Heat and wave kernel signatures on the device (dm_spectral_signatures[_f64]): the spectral descriptors of
// FunctionalMapping.preprocess (reference functional.py:308-334) for a batch of meshes.
//
//   S[n, t]   = sum_k w[t,k] Phi[n,k]^2       / sum_k w[t,k]       (plain block)
//   S_p[n, t] = sum_k w[t,k] Phi[p,k] Phi[n,k] / sum_k w[t,k]       (one block per landmark p, HKS_functions.py:73: landmark-major columns)
//   HKS: w[t,k] = exp(-t lambda_k)                                   HKS_functions.py:97-98
//   WKS: w[e,k] = exp(-(e - ln lambda_k)^2 / (2 sigma^2))            WKS_functions.py:29,71,118-126
//
// The times / energies, the sorted |lambda| (or their logarithms), 2 sigma^2 and the first kept eigen-column come from the host
// (pyFM/signatures.py: signature_tables, the reference's own NumPy calls), so the arguments of exp are the host's bit for bit:
// -(t mu) and -((e - mu)(e - mu)) / denom, every operation rounded on its own (__d*_rn: no contraction).  What may differ from
// the host is exp itself (OCML against libm) and the order of the two sums.
//
// Two launches:
//   sig_weights_kernel   W (B, nk, T, Kw) and 1 / sum_k w (B, nk, T) into the workspace; nk block kinds in use (plain, landmark:
//                        WKS drops a different number of leading eigen-columns for the two), columns before k0 and past K are 0
//   gemm_nt_f64          one (N x T x K) product per mesh and BLOCK (grid z = B (plain + P)) on the float64 matrix cores: the A
//                        operand delivers Phi[n,k] Phi[p,k] (one float64 rounding, like the host's evects * evects[p]), the Out
//                        functor applies the column scale -- (A @ w^T) * (1 / sum w), as the host writes it: a column whose weights
//                        all underflow is 0 * inf = NaN in every row, like the reference's -- and the output type.
// Bound: the output, (plain + P) T values per vertex written once (WKS-2048 of 2048 vertices: 32 MiB in float64 for 0.4 GFLOP).
// A mesh's values depend on nothing but its own rows and table: bit-identical whatever shares the call or however N is padded.
#include <vector>

#include "dm_gemm_f64.h"
#include "dm_internal.h"

// slot of the weights a block reads: with both kinds in use the plain block reads slot 0, landmark blocks slot 1
__device__ __forceinline__ int sig_slot(int q, int plain, int nk) { return (nk == 2 && q >= plain) ? 1 : 0; }

// grid (T, nk, B), one wave per (mesh, kind, t)
__global__ __launch_bounds__(64) void sig_weights_kernel(int wks, int T, int K, int Kw, int nk, int plain, const double* __restrict__ tt,
                                                          const double* __restrict__ mu, const double* __restrict__ denom,
                                                          const int32_t* __restrict__ k0, double* __restrict__ W, double* __restrict__ rs) {
    const int it = blockIdx.x, s = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int kb = (nk == 2) ? s : (plain ? 0 : 1);                  // block kind of this slot: 0 plain, 1 landmark
    const int kfirst = k0[b * 2 + kb];
    const double tv = tt[(long long)b * T + it];
    const double dn = wks ? denom[b] : 1.0;
    double* row = W + (((long long)b * nk + s) * T + it) * Kw;
    double part = 0.0;
    for (int k = lane; k < Kw; k += 64) {
        double w = 0.0;
        if (k >= kfirst && k < K) {
            const double m = mu[(long long)b * K + k];
            double arg;
            if (wks) {
                const double d = __dsub_rn(tv, m);
                arg = __ddiv_rn(-__dmul_rn(d, d), dn);
            } else {
                arg = -__dmul_rn(tv, m);
            }
            w = exp(arg);
            part += w;
        }
        row[k] = w;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) rs[((long long)b * nk + s) * T + it] = 1.0 / part;
}

// A operand: row n of block q of mesh b is Phi[n, k] * Phi[p_q, k] (p_q = n for the plain block); the product is formed in float64
// when the staged pair is written to LDS
template <typename TR>
struct SigPair {
    TR a, p;
    __device__ __forceinline__ operator double() const { return (double)a * (double)p; }
};
template <typename TR>
struct SigRows {
    typedef SigPair<TR> elem_t;
    const TR* Phi; long long stride_b; int ld; int N; int K;
    const int32_t* lm; int P; int plain; int nblk;
    __device__ __forceinline__ void load8(int bv, int row, int k0, elem_t (&v)[8]) const {
        const int b = bv / nblk, q = bv - b * nblk;
        const bool in = row < N;
        const int rc = min(row, N - 1);
        const int pr = (q < plain) ? rc : min(max(lm[(long long)b * P + (q - plain)], 0), N - 1);
        const TR* r = Phi + b * stride_b + (long long)rc * ld;
        const TR* rp = Phi + b * stride_b + (long long)pr * ld;
        if (k0 + 7 < K && dm_rows_aligned<TR>(Phi, stride_b, ld)) {
            TR a0[4], a1[4], p0[4], p1[4];
            dm_load_row4<TR>(r, k0, K, true, a0);
            dm_load_row4<TR>(r, k0 + 4, K, true, a1);
            dm_load_row4<TR>(rp, k0, K, true, p0);
            dm_load_row4<TR>(rp, k0 + 4, K, true, p1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = elem_t{in ? a0[e] : (TR)0, p0[e]};
                v[4 + e] = elem_t{in ? a1[e] : (TR)0, p1[e]};
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool ok = in && k0 + e < K;
                v[e] = elem_t{ok ? r[k0 + e] : (TR)0, ok ? rp[k0 + e] : (TR)0};
            }
        }
    }
};

// B operand: row t of the block's weights (Kw = K rounded up to 8, zero behind K: every 8-wide piece is whole and 16-byte aligned)
struct SigWeights {
    const double* W; int T; int Kw; int nk; int plain; int nblk;
    __device__ __forceinline__ void load8(int bv, int row, int k0, double (&v)[8]) const {
        const int b = bv / nblk, q = bv - b * nblk;
        const bool in = row < T && k0 < Kw;
        const f64x2* r = reinterpret_cast<const f64x2*>(W + (((long long)b * nk + sig_slot(q, plain, nk)) * T + min(row, T - 1)) * Kw + (in ? k0 : 0));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f64x2 x = r[e];
            v[2 * e] = in ? x[0] : 0.0;
            v[2 * e + 1] = in ? x[1] : 0.0;
        }
    }
};

// out[b][i][q T + j] = acc * (1 / sum_k w[j, k]); rows past the mesh's vertex count are 0
template <typename TO>
struct SigOut {
    TO* out; long long stride_b; int ldo; int T; const double* rs; int nk; int plain; int nblk; const int32_t* nv;
    __device__ __forceinline__ void store(int bv, int i, int j, double v) const {
        const int b = bv / nblk, q = bv - b * nblk;
        const double sc = rs[((long long)b * nk + sig_slot(q, plain, nk)) * T + j];
        const double r = (i < nv[b]) ? v * sc : 0.0;
        out[b * stride_b + (long long)i * ldo + (long long)q * T + j] = (TO)r;
    }
};

template <typename TR>
static int signatures_impl(dm_ctx* ctx, int B, int N, const int32_t* n_verts, int K, const TR* Phi, int ld, int kind, int T, const double* t,
                           const double* mu, const double* denom, const int32_t* k0, int P, const int32_t* landmarks, int plain, int out_f32,
                           void* out) {
    if (!ctx) return DM_EINVAL;
    DM_REQUIRE(ctx, B > 0 && N > 0 && K > 0, "sizes must be positive");
    DM_REQUIRE(ctx, T >= 1, "at least one time / energy");
    DM_REQUIRE(ctx, kind == 0 || kind == 1, "kind: 0 = HKS, 1 = WKS");
    DM_REQUIRE(ctx, (plain == 0 || plain == 1) && P >= 0 && plain + P >= 1, "nothing to compute: plain = 0 and no landmark");
    DM_REQUIRE(ctx, Phi && t && mu && k0 && out && (kind == 0 || denom) && (P == 0 || landmarks), "null pointer");
    DM_REQUIRE(ctx, ld >= K, "eigenvector row stride smaller than the number of eigenpairs");
    const int nblk = plain + P, nk = (plain && P > 0) ? 2 : 1;
    DM_REQUIRE(ctx, (long long)B * nblk <= 65535, "more than 65535 (mesh, block) products in one call");
    DM_REQUIRE(ctx, (long long)nblk * T <= 0x7fffffff, "output row longer than 2^31 - 1");
    // the small integers of the call, checked here and uploaded in one piece: [n_verts (B) | k0 (B, 2) | landmarks (B, P)]
    std::vector<int32_t> ints((size_t)B * (3 + P));
    for (int b = 0; b < B; ++b) {
        const int nv = n_verts ? n_verts[b] : N;
        if (nv < 0 || nv > N) return dm_fail(ctx, DM_EINVAL, "dm_spectral_signatures: n_verts[%d] = %d outside [0, %d]", b, nv, N);
        ints[b] = nv;
        for (int c = 0; c < 2; ++c) {
            const int kf = k0[b * 2 + c];
            const bool used = c == 0 ? plain != 0 : P > 0;
            if (used && (kf < 0 || kf >= K))
                return dm_fail(ctx, DM_EINVAL, "dm_spectral_signatures: mesh %d keeps no eigenpair (k0 = %d of K = %d)", b, kf, K);
            ints[(size_t)B + b * 2 + c] = used ? kf : 0;
        }
        for (int p = 0; p < P; ++p) {
            const int v = landmarks[(size_t)b * P + p];
            if (v < 0 || v >= nv) return dm_fail(ctx, DM_EINVAL, "dm_spectral_signatures: landmark %d of mesh %d outside [0, %d)", v, b, nv);
            ints[(size_t)3 * B + (size_t)b * P + p] = v;
        }
    }
    DM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int Kw = (K + 7) / 8 * 8;
    const size_t bW = (size_t)B * nk * T * Kw * 8, bR = (size_t)B * nk * T * 8, bI = ints.size() * 4;
    int rc = dm_ws_reserve(ctx, dm_align_up(bW) + dm_align_up(bR) + dm_align_up(bI) + 1024);
    if (rc) return rc;
    double* W = (double*)dm_ws_take(ctx, bW);
    double* rs = (double*)dm_ws_take(ctx, bR);
    int32_t* di = (int32_t*)dm_ws_take(ctx, bI);
    if (!W || !rs || !di) return dm_fail(ctx, DM_ENOMEM, "spectral signatures: workspace not reserved");
    DM_CHECK_HIP(ctx, hipMemcpyAsync(di, ints.data(), bI, hipMemcpyHostToDevice, ctx->stream));
    DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));         // (the host vector goes away with this call)
    const int32_t* d_nv = di;
    const int32_t* d_k0 = di + B;
    const int32_t* d_lm = di + (size_t)3 * B;
    DM_LAUNCH(ctx, "sig_weights", sig_weights_kernel, dim3(T, nk, B), dim3(64), 0, kind, T, K, Kw, nk, plain, t, mu, denom, d_k0, W, rs);
    SigRows<TR> opa{Phi, (long long)N * ld, ld, N, K, d_lm, P, plain, nblk};
    SigWeights opb{W, T, Kw, nk, plain, nblk};
    const dim3 grid(dm_cdiv(N, NT_T) * dm_cdiv(T, NT_T), 1, B * nblk);
    const long long so = (long long)N * nblk * T;
    if (out_f32) {
        SigOut<float> o{(float*)out, so, nblk * T, T, rs, nk, plain, nblk, d_nv};
        DM_LAUNCH(ctx, "signatures_nt_f64", (gemm_nt_f64<SigRows<TR>, SigWeights, SigOut<float>>), grid, dim3(256), 0, opa, opb, o, N, T, K);
    } else {
        SigOut<double> o{(double*)out, so, nblk * T, T, rs, nk, plain, nblk, d_nv};
        DM_LAUNCH(ctx, "signatures_nt_f64", (gemm_nt_f64<SigRows<TR>, SigWeights, SigOut<double>>), grid, dim3(256), 0, opa, opb, o, N, T, K);
    }
    return DM_OK;
}

extern "C" int dm_spectral_signatures(dm_ctx* ctx, int B, int N, const int32_t* n_verts, int K, const float* Phi, int ld, int kind, int T,
                                      const double* t, const double* mu, const double* denom, const int32_t* k0, int P,
                                      const int32_t* landmarks, int plain, int out_f32, void* out) {
    return signatures_impl<float>(ctx, B, N, n_verts, K, Phi, ld, kind, T, t, mu, denom, k0, P, landmarks, plain, out_f32, out);
}
extern "C" int dm_spectral_signatures_f64(dm_ctx* ctx, int B, int N, const int32_t* n_verts, int K, const double* Phi, int ld, int kind, int T,
                                          const double* t, const double* mu, const double* denom, const int32_t* k0, int P,
                                          const int32_t* landmarks, int plain, int out_f32, void* out) {
    return signatures_impl<double>(ctx, B, N, n_verts, K, Phi, ld, kind, T, t, mu, denom, k0, P, landmarks, plain, out_f32, out);
}

/*
 * densematch.h -- C ABI of libdensematch (MI355X / gfx950 native).
 *
 * The drop-in boundary for DenseMatcher's matching hot path.  The reference
 * has no FFI on this path: the seam is the Python call level
 * (densematcher/functional_map.py:9 `compute_surface_map` and the
 * densematcher/pyFM functions it calls).  Each entry point below replaces the
 * arithmetic of one of those reference functions; the Python mirror in
 * `densematcher_amd/` keeps the reference signatures and binds these symbols
 * with ctypes (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - every array argument is a DEVICE pointer owned by the caller (hipMalloc /
 *     torch tensor.data_ptr()), row-major, batch-major, contiguous unless an
 *     `ld` (row stride in elements) is given.  The library never frees or
 *     retains caller pointers past return.
 *   - B = number of mesh pairs in the batch.  Pairs are independent.
 *   - mesh 1 = source, mesh 2 = target.  Phi1 (N1 x ld1) / Phi2 (N2 x ld2) are
 *     mass-orthonormal Laplace-Beltrami eigenvectors, mass1/mass2 the diagonals
 *     of the lumped mass matrices, C is (k2 x k1) and maps basis-1
 *     coefficients to basis 2 (reference convention, pyFM/functional.py:482).
 *   - eigenvectors and masses are fp32 in the plain entry points and fp64 in the `*_f64` ones (same argument lists,
 *     `const double*` for Phi1 / Phi2 / mass): float64 is what the reference holds (pyFM/mesh/trimesh.py:118 float64
 *     vertices -> float64 spectrum) and what its FM_to_p2p / p2p_to_FM / ICP / ZoomOut consume
 *     (pyFM/spectral/convert.py:134-144), so the integer outputs of the `*_f64` forms equal the reference's on ITS inputs;
 *     fp32 halves the operand traffic and is exact for bases that were rounded to fp32 anyway.
 *   - integer maps are int32 on the device (the Python layer widens to int64).
 *   - calls are asynchronous on the context's stream; the caller synchronises
 *     the stream before reading results.  A context is not thread-safe;
 *     contexts are independent of one another.
 *   - return value: DM_OK or a negative dm_status; no exceptions cross the ABI.
 */
#ifndef DENSEMATCH_H
#define DENSEMATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dm_ctx dm_ctx;

typedef enum dm_status {
    DM_OK = 0,
    DM_EINVAL = -1,     /* bad argument (shape, null pointer, unsupported size)  -> Python ValueError   */
    DM_ENOMEM = -2,     /* workspace allocation failed                           -> Python MemoryError  */
    DM_EHIP = -3,       /* a HIP runtime call failed (see dm_last_error)         -> Python RuntimeError */
    DM_ESINGULAR = -4   /* a linear system was not positive definite (info[] says which pair) */
} dm_status;

/* feature dtypes for dm_project; OR in DM_PROJECT_F64 to force the float64 matrix-core path */
enum { DM_F16 = 0, DM_F32 = 1, DM_PROJECT_F64 = 0x10 };

/* ---- context ---------------------------------------------------------- */
/* One context per (device, stream).  hip_stream may be NULL (default stream). */
int dm_create(int device, void* hip_stream, dm_ctx** out);
int dm_destroy(dm_ctx* ctx);
/* ctx-owned string describing the last failure; valid until the next call on ctx. */
const char* dm_last_error(const dm_ctx* ctx);
const char* dm_version(void);
/* bytes of ctx-owned scratch currently allocated (grown lazily, never shrunk). */
size_t dm_workspace_bytes(const dm_ctx* ctx);
/* Choose between equivalent code paths (every value of every option returns the same, exact results; the
 * defaults are the fast paths).  No reference counterpart: the reference has one CPU path.  Options:
 *   "simnn_pipe"    1 | 0   feature-similarity tiles: LDS-DMA ring kernel | bounds-checked register-staged kernel
 *   "simnn_persist" 1 | 0 | n>1   one persistent workgroup per CU walking its tiles | one workgroup per tile | exactly n workgroups
 *   "knn_split"     1 | 0   knn21 of dm_zoomout / dm_icp / dm_knn_query_f64: fp16-split first pass | float64 G kernel
 *   "p2p_split" 2 | 3 | 4 | 1 | 0 dm_fm_to_p2p: one fp16 pass reducing in both directions, tile shape by size (4 waves, 128 x 256
 *                           tiles, two workgroups per CU while a pair's operands fit an XCD's L2, else 8 waves, 256 x 256) |
 *                           always the 4-wave shape | always the 8-wave shape | two two-key passes | float64 G kernel
 *                           (all + exact float64 re-evaluation of the ambiguous rows; identical results)
 *   "solve_packed"  0 | 1   dm_fmap_solve: blocked LDS Cholesky when it fits | packed-storage solver always
 *   "simnn_band"    4 | n   tile order of the similarity kernels: bands of n tile rows, column-major inside (0: row-major)
 *   "simnn_big"     0 | 1   tile kernels as four waves of 128 x 128 (accumulators in AGPRs) instead of eight waves of 128 x 64
 *   "lsa_reg"       2 | 1 | 0   dm_linear_sum_assignment: column state in registers, started from a column reduction (kept per
 *                           matrix only when its optimum is provably unique, else redone) | the same in SciPy's order | LDS state
 *   "solve_reg"     1 | 0   dm_fmap_solve, k1 <= 129: register-resident solver (one wave per system) | the LDS-resident blocked one
 *   "zoomout_fused" 1 | 0   dm_zoomout on meshes of at least 256 vertices, maps up to 208: five launches per iteration (embedding + split
 *                           rows, biased-key search, merge, exact, p2p_to_FM) | six (seven with the reduce) through K-major copies
 *   "zoomout_sub_fused" 1 | 0   subsampled ZoomOut in the Python layer (refine.zoomout_refine(subsample=...), square map, one step size):
 *                           dm_zoomout_sub, one device loop on one Cholesky factor | the host-chained search + dm_p2p_to_fm_lstsq per
 *                           iteration.  The library only keeps the value.  The two settings agree to 1e-9, not bit for bit.
 *   "fps_heat_route" 0 | 1 | 2   dm_fps_heat: the all-pairs rows when their work space fits, else one solve per sample | always the
 *                           all-pairs rows | always one solve per sample.  Same indices.
 *   "graph_geod_device" 1 | 0   shortest paths along the mesh edges in the Python layer (the default TriMesh.extract_fps / extract_fps_many,
 *                           get_geodesic(dijkstra=True), geometry.geodesic_distmat_dijkstra): dm_fps_graph / dm_graph_geodesic | SciPy's
 *                           Dijkstra on the host.  The library only keeps the value.  The two settings agree bit for bit.
 *   "fmn_eig_route" 0 | 1 | 2   the eigenproblem of a functional map network in the Python layer (MatchEngine.eigh_smallest, FMN.compute_CLB):
 *                           by the sizes (Jacobi where the filtered iteration has no room, 2 (k + guard) > n, or n <= 128) | always the
 *                           full Jacobi eigendecomposition (n <= 512) | always the Chebyshev-filtered iteration.  The library only keeps
 *                           the value.  The routes agree on eigenvalues and invariant subspaces, not on bits.
 *   "p2pfm_direct"  1 | 0   dm_p2p_to_fm (and the p2p_to_FM steps of dm_zoomout / dm_icp): register-resident tiles, operands straight
 *                           from global memory, fixed-order in-workgroup reduction | LDS-staged 64 x 64 tiles + split-K partials + reduce
 *   "simnn1_wt"     4 | 2   tile shape of the fused ZoomOut search: 8 waves, 256 x 256 | 4 waves, 128 x 256 (two workgroups per CU)
 *   "solve_pcg"     1 | 0   dm_fmap_solve / dm_fmap_fit, 66 <= k1 <= 200 (any batch: the choice follows the sizes only, a pair's result
 *                           does not depend on its batch): the k2 systems of a pair by a batched Jacobi-preconditioned
 *                           conjugate-gradient iteration on the float64 matrix cores (stops at a 1e-11 relative reduction: C within 1e-9 of
 *                           the direct solution; ill-conditioned pairs leave it after six steps and take the direct solver) | direct
 *                           solvers only.  The two settings agree to 1e-9, not bit for bit.
 *   "basis_stats"   1 | 0   dm_fm_to_p2p: keep the maximum of |Phi2| per basis tensor between calls (a checked hint: the target operand's
 *                           fp16 rows are then written while the basis streams through the second embedding) | every call takes its own
 *                           pass over the basis.  Same results.
 *   "fit_mfma"      1 | 0   the fp32 element loop for maps up to 16 x 16: the two 16-deep products of an entry (the entry itself and the
 *                           back-product of its derivative) on v_mfma_f32_16x16x4_f32, the element-wise terms alone on the vector ALU | both
 *                           on the packed vector FMA.  Different summation orders of the same fp32 arithmetic: both within 1e-7 (energy) /
 *                           1e-6 (gradient) of the float64 oracle, fitted maps within 1e-6 of each other.
 * Unknown names return DM_EINVAL.  The library never reads environment variables. */
int dm_set_option(dm_ctx* ctx, const char* name, int value);
/* Diagnostics of the LAST dm_fm_to_p2p[_f64] / dm_simnn_f16 call on ctx (synchronises the stream): out[q] = rows of reduction q
 * whose fp32 margin fell inside the error bound and were re-evaluated in float64 (q = knn21 | ind21 | knn12 | ind12 for the four
 * maps, q = 0 for dm_simnn_f16; -1 where the call ran the float64 kernel).  bench.py reports them for its hard input
 * distributions: the cost of the exact pass depends on the data.  No reference counterpart. */
int dm_last_requeued_rows(dm_ctx* ctx, int out[4]);

/* ---- kernel timing (HIP events on the ctx stream) ----------------------- */
/* Bracket every launch of the kernel called `name` (see DESIGN.md for names)
 * with a hipEvent pair.  Pass NULL to stop.  dm_profile_read synchronises the
 * stream and returns the number of launches and their summed duration since
 * the last dm_profile_kernel call. */
int dm_profile_kernel(dm_ctx* ctx, const char* name);
int dm_profile_read(dm_ctx* ctx, int* launches, double* total_ms);
/* dm_profile_kernel(ctx, "*") brackets EVERY launch; dm_profile_report then writes one line per kernel name,
 * "name\tlaunches\ttotal_ms\tkernels\n" in order of first launch, into buf (NUL-terminated; DM_EINVAL if cap is too small) and
 * resets the record.  `kernels` lists the distinct kernel expressions launched under that name, ';'-separated (several kernels
 * share a name: every direct solver is "fmap_solve_chol").  (The event pairs add a few microseconds between launches: bench.py times its K steps with one kernel
 * bracketed and collects the per-kernel table in a separate, untimed pass.) */
int dm_profile_report(dm_ctx* ctx, char* buf, size_t cap);

/* ---- on-box peak probes (bench.py: measured peak beside the spec peak of the roofline block) -------------------
 * value = FLOP/s (matrix-core probes) or bytes/s read + written (copy).  The fp16 probe comes in two flavours because the
 * part is power-limited: all-zero operands run at the full 2.4 GHz (the instruction-issue ceiling, ~2.48 PFLOP/s), N(0,1)
 * operands pull the shader clock to ~1.7 GHz (~1.72 PFLOP/s): the ceiling of a kernel that multiplies real data. */
enum { DM_PEAK_MFMA_F16_ZERO = 0, DM_PEAK_MFMA_F16_RANDOM = 1, DM_PEAK_MFMA_F64 = 2, DM_PEAK_HBM_COPY = 3 };
int dm_measure_peak(dm_ctx* ctx, int which, double* value);

/* ---- config 3: feature-similarity nearest neighbour ---------------------
 * nn21[b,i] = argmax_j <Ftgt[b,i,:], Fsrc[b,j,:]>   (lowest j on ties)
 * No reference symbol; defined by oracle/dm_oracle.py:simnn.
 * The products are exact (fp16 x fp16 in fp32), accumulated in fp32 on the
 * matrix cores; rows whose top-2 margin is within the fp32 accumulation bound
 * are re-evaluated in float64, so nn21 equals the float64 argmax.
 * Ftgt (B,N2,D), Fsrc (B,N1,D) fp16.  best/margin (B,N2) fp32 are optional
 * (fp32-accumulated best score and best - second best). */
int dm_simnn_f16(dm_ctx* ctx, int B, int N2, int N1, int D,
                 const void* Ftgt, const void* Fsrc,
                 int32_t* nn21, float* best /*nullable*/, float* margin /*nullable*/);

/* ---- spectral projection ------------------------------------------------
 * Ared[b] = Phi[b][:, :k]^T (mass[b] * F[b])        (k x D), fp32 out.
 * Replaces pyFM/optimize/base_functions.py:526-532 (descr{1,2}_red) and
 * pyFM/mesh/trimesh.py:533-556 (TriMesh.project).
 * Phi (B,N,ld) fp32, mass (B,N) fp32, F (B,N,D) fp16 or fp32 (f_dtype).
 * fp16 descriptors run on the fp16 matrix cores with the basis split into two fp16 pieces (relative error
 * ~1e-6, the class of the reference's own fp32 projection); fp32 descriptors, or f_dtype | DM_PROJECT_F64,
 * run on the float64 matrix cores (error = the final fp32 rounding only). */
int dm_project(dm_ctx* ctx, int B, int N, int D, int k,
               const float* Phi, int ld, const float* mass,
               const void* F, int f_dtype, float* Ared /* B*k*D */);
/* float64 basis and masses: rounded to fp32 as they are loaded by the fp16-split path (exactly what the reference's fit does
 * before it projects, pyFM/functional.py:410-414: same result as converting first, without the extra pass over Phi); the
 * DM_PROJECT_F64 path uses them unrounded (TriMesh.project, pyFM/mesh/trimesh.py:533-556, is float64 NumPy). */
int dm_project_f64(dm_ctx* ctx, int B, int N, int D, int k,
                   const double* Phi, int ld, const double* mass,
                   const void* F, int f_dtype, float* Ared /* B*k*D */);

/* ---- pinned first column ---------------------------------------------------
 * c00[b] = sign(Phi1[b][0,0] * Phi2[b][0,0]) * sqrt(sum(mass2[b]) / sum(mass1[b]))
 * Replaces FunctionalMapping.get_x0 (pyFM/functional.py:654-658; mesh.area =
 * A.sum(), pyFM/mesh/trimesh.py:206-221): the only non-zero entry of column 0
 * of the initial map, which the optimiser never changes (base_functions.py:759). */
int dm_fmap_c00(dm_ctx* ctx, int B, int N1, int N2,
                const float* Phi1, int ld1, const float* Phi2, int ld2,
                const float* mass1, const float* mass2, double* c00 /* B */);
int dm_fmap_c00_f64(dm_ctx* ctx, int B, int N1, int N2,
                    const double* Phi1, int ld1, const double* Phi2, int ld2,
                    const double* mass1, const double* mass2, double* c00 /* B */);

/* ---- functional-map solve -----------------------------------------------
 * Minimiser of  w_descr/2 |C A - Bm|^2 + w_lap/2 sum C_ij^2 ev_ij  with column
 * 0 pinned to (c00, 0, ..., 0)^T, ev_ij = ((lam1_j - lam2_i)/max(lam))^2.
 * Replaces the L-BFGS-B loop of pyFM/functional.py:352-487 over
 * pyFM/optimize/base_functions.py:480-763 (w_descr / w_lap terms), i.e.
 * FunctionalMapping.fit; c00 is get_x0()[0,0] (functional.py:654-658).
 * A (B,k1,D), Bm (B,k2,D) fp32; lam1 (B,k1), lam2 (B,k2), c00 (B) fp64;
 * C (B,k2,k1) fp64 out; info (B) int32 out, 0 = ok, r+1 = row r not SPD. */
int dm_fmap_solve(dm_ctx* ctx, int B, int k1, int k2, int D,
                  const float* A, const float* Bm,
                  const double* lam1, const double* lam2, const double* c00,
                  double w_descr, double w_lap, double* C, int32_t* info);

/* The same fit in ONE call: FunctionalMapping.fit with w_descr, w_lap > 0 and every other weight 0
 * (pyFM/functional.py:352-487) = the two projections (dm_project), the pinned column (dm_fmap_c00) and dm_fmap_solve.
 * Same C, bit for bit, as the three calls; the projected descriptors are not returned, which lets the library skip their
 * split-K reduction pass (the Gram kernel adds the chunks up as it reads them).  F1 (B,N1,D), F2 (B,N2,D) fp16. */
int dm_fmap_fit(dm_ctx* ctx, int B, int N1, int N2, int D, int k1, int k2,
                const float* Phi1, int ld1, const float* Phi2, int ld2,
                const float* mass1, const float* mass2, const void* F1, const void* F2,
                const double* lam1, const double* lam2, double w_descr, double w_lap,
                double* C, int32_t* info);
int dm_fmap_fit_f64(dm_ctx* ctx, int B, int N1, int N2, int D, int k1, int k2,
                    const double* Phi1, int ld1, const double* Phi2, int ld2,
                    const double* mass1, const double* mass2, const void* F1, const void* F2,
                    const double* lam1, const double* lam2, double w_descr, double w_lap,
                    double* C, int32_t* info);

/* ---- general functional-map energy and gradient -----------------------------------
 * What scipy's L-BFGS-B evaluates in FunctionalMapping.fit when energy terms beyond w_descr / w_lap are switched on:
 * replaces energy_func_std / grad_energy_std (pyFM/optimize/base_functions.py:480-763) for the terms
 *   weights[0..9] = w_descr, w_lap, w_dcomm, w_p2p, w_stochastic, w_ent, w_range01, w_sumto1, w_area, w_conformal   (HOST array of 10 doubles)
 *   (w_area 1/2 |C^T C - I|^2, w_conformal 1/2 |C^T D2 C - D1|^2 with D = diag(lam / max lam): base_functions.py:228-294.  The
 *    orientation term w_orient, base_functions.py:567-600, is a commutation term like w_dcomm: the host appends its operator pairs,
 *    scaled by sqrt(w_orient / w_dcomm), to ops1 / ops2 -- densematcher_amd/pyFM/functional.py.)
 * i.e. descr_preservation :31, LB_commutation :79, oplist_commutation :168 (descriptor multiplication operators),
 * p2p :296, doubly_stochastic :324, entropy :363, range01 :374, sumto1 :387 (eta == 1, v = None).
 * energy (B) fp64 = the reference's energy value; grad (B,k2,k1) fp64 = its gradient with column 0 zeroed (:759).
 * A (B,k1,D), Bm (B,k2,D) fp32 = the projections (dm_project); ops1 (B,n_ops,k1,k1), ops2 (B,n_ops,k2,k2) fp64 =
 * dm_fmap_descr_ops of the two meshes (needed only when w_dcomm > 0; n_ops = number of descriptors).  The terms in the
 * mapped indicator (last five weights) need Phi1, Phi2, mass1; the indicator itself is never stored (its tiles are formed twice on
 * the float64 matrix cores, statistics then derivative): workspace O(B N k), k1 <= 256. */
int dm_fmap_energy_grad(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2, int D,
                        const float* Phi1, int ld1, const float* Phi2, int ld2, const float* mass1,
                        const float* A, const float* Bm, const double* lam1, const double* lam2,
                        const double* ops1 /*nullable*/, const double* ops2 /*nullable*/, int n_ops,
                        const double* weights /*host, 10*/, const double* C, double* energy, double* grad);
/* What dm_fmap_energy_grad will do for these sizes: host only, launches nothing. ctx may be NULL, then n_cu is used (<= 0: 256).
 * out[12]: rg, ncs, cchunk, ngroups, stats_route, cp_inline, e2_inline, nt2, kc_m, nsplit_m, nsplit_d, m_terms
 *   rg          rows of the mapped indicator per workgroup of the statistics tile pass (64, 128, 256, 512)
 *   ncs, cchunk column splits of both tile passes and the columns of one split (trailing splits may be empty); ngroups = ceil(N2 / rg)
 *   stats_route 0: no row / column statistics; 1: from the basis sums (w_sumto1 without w_stochastic, k2 <= 256); 2: the tile pass
 *   cp_inline, e2_inline   maps up to 32 x 32: C A A^T / Phi2 C are formed inside another kernel instead of by a product launch
 *   nt2         16-column tiles of the derivative pass per wave: 1, 2, 4 for k1 <= 64, 128, 256
 *   kc_m, nsplit_m   split-K chunk and splits of Phi2^T Y; nsplit_d: splits of the commutativity back product (0: no such term)
 *   m_terms     1 when an indicator term is weighted; otherwise the indicator fields (all but cp_inline, nsplit_d) are 0
 * rg, ncs, cchunk and ngroups depend on the batch size and the CU count, the others on the map's sizes and the weights alone.  Two
 * evaluations of a pair under the same plan give the same bits.  Returns what dm_fmap_energy_grad returns for sizes and weights
 * it refuses (DM_EINVAL). */
int dm_fmap_energy_plan(const dm_ctx* ctx, int n_cu, int B, int N1, int N2, int k1, int k2, const double* weights /*host, 10*/, int n_ops,
                        int32_t out[12]);

/* ---- batched L-BFGS on the device --------------------------------------------------------------------------------
 * The optimiser FunctionalMapping.fit runs for the non-quadratic terms: replaces scipy.optimize.minimize(method = "L-BFGS-B")
 * of pyFM/functional.py:477 (no bounds are set there: plain limited-memory BFGS with L-BFGS-B's line-search constants and
 * stopping tests).  The state of every pair (iterate, gradient, direction, m history pairs, line-search bracket, counters)
 * lives in `state` (dm_lbfgs_state_bytes bytes of device memory owned by the caller); pairs are independent of one another.
 *   dm_lbfgs_init     x0 (B,n) -> state, x_trial = x0
 *   dm_lbfgs_advance  energy (B) and grad (B,n) of x_trial (dm_fmap_energy_grad) -> the pairs' next trial points in x_trial;
 *                     ftol: stop when (f_k - f_k+1) <= ftol max(|f_k|, |f_k+1|, 1) (SciPy: factr * eps = 2.2e-9), pgtol: max |g_i|
 *                     (SciPy 1e-5), maxiter, maxfun (SciPy 15000), maxls (SciPy 20).  Finished pairs keep x_trial at their result.
 *   dm_lbfgs_result   x (B,n), f (B), info (B,4) = status (0 running, 1 gradient, 2 energy decrease, 3 maxiter, 4 maxfun, 5 line
 *                     search failed), iterations, evaluations, history length
 * The host alternates dm_fmap_energy_grad and dm_lbfgs_advance and reads info every few evaluations.
 * All three take 1 <= m <= 64 (B, n >= 1, no null pointer) and return DM_EINVAL otherwise. */
size_t dm_lbfgs_state_bytes(int B, int n, int m);
int dm_lbfgs_init(dm_ctx* ctx, int B, int n, int m, const double* x0, void* state, double* x_trial);
int dm_lbfgs_advance(dm_ctx* ctx, int B, int n, int m, void* state, const double* energy, const double* grad, double* x_trial,
                     double ftol, double pgtol, int maxiter, int maxfun, int maxls);
int dm_lbfgs_result(dm_ctx* ctx, int B, int n, int m, const void* state, double* x, double* f, int32_t* info);
/* `nsteps` rounds of (dm_fmap_energy_grad at x_trial -> dm_lbfgs_advance) without returning to the caller in between: the loop
 * of one scipy.optimize.minimize call (pyFM/functional.py:477), nsteps evaluations at a time.  `energy` (B) and `grad` (B,k2,k1)
 * are scratch the caller owns; x_trial (B,k2,k1) is the trial point dm_lbfgs_init / the last advance left.  Pairs that have
 * stopped are not moved by further steps.  (A Python loop around the two calls costs more host time per evaluation than the
 * evaluation takes on the device for one small pair.)
 *   keep (nullable)     dm_fmap_fit_keep_bytes(B, k1, k2) bytes of device memory the caller owns, for what an evaluation computes
 *                       that does not depend on the map: A A^T and Bm A^T stacked (B, k1 + k2, k1) fp64, then the mass-weighted
 *                       column sums of the bases, p (B, k1) and s2 (B, k2).  NULL: every evaluation recomputes them in the workspace,
 *                       as dm_fmap_energy_grad does.  The same bits either way.
 *   keep_valid 0 | 1    0: the first evaluation of this call writes the block (the evaluations after it read it).  1: the block is
 *                       read as it is; it must have been written by an earlier call of the same fit, with the same operands and weights.
 *   n_running (host, nullable)   the number of pairs whose status is still 0 (running) after the call's last advance; asking for it
 *                       is the call's one synchronisation with the device. */
size_t dm_fmap_fit_keep_bytes(int B, int k1, int k2);
int dm_fmap_fit_steps(dm_ctx* ctx, int nsteps, int B, int N1, int N2, int k1, int k2, int D,
                      const float* Phi1, int ld1, const float* Phi2, int ld2, const float* mass1,
                      const float* A, const float* Bm, const double* lam1, const double* lam2,
                      const double* ops1 /*nullable*/, const double* ops2 /*nullable*/, int n_ops,
                      const double* weights /*host, 10*/, int m, void* state, double* x_trial, double* energy, double* grad,
                      double ftol, double pgtol, int maxiter, int maxfun, int maxls,
                      double* keep /*nullable*/, int keep_valid, int* n_running /*host, nullable*/);

/* The WHOLE iterative fit of small maps in one call: FunctionalMapping.fit (pyFM/functional.py:352-487) for maps up to 32 x 32 whose
 * energy has, besides w_descr / w_lap, only element-wise indicator terms and the sum-to-one term (w_p2p, w_ent, w_range01, w_sumto1:
 * base_functions.py:296, 363, 374, 387) -- the notebook's call (example.ipynb cell 11).  One launch per energy evaluation: the
 * workgroup that delivers a pair's last partial sum also adds up, evaluates the O(k^3) terms and advances that pair's L-BFGS
 * (same optimiser, constants and stopping rules as dm_lbfgs_advance); the status words are read every 16 launches.  A pair's
 * result does not depend on the batch it is in (the additions follow a tree fixed by N1, N2 alone).
 *   dm_fmap_fit_fused_ok  1 when the sizes / weights (host array of 10, order of dm_fmap_energy_grad) are taken, else 0 (the caller
 *                         then runs dm_fmap_fit_steps)
 *   x0 (B,k2,k1) start (first column = the pinned one); x_out (B,k2,k1), f_out (B), info_out (B,4) as dm_lbfgs_result;
 *   evaluations_out (host, nullable): launches issued.
 *   maxfun <= 0: ONE evaluation at x0, no optimiser: f_out (B) energy, grad_out (B,k2,k1) gradient (x_out / info_out unused).
 *   element_f32 0 | 1 (both modes): the element loop over the N2 x N1 entries of the mapped indicator in float64 | in fp32, the
 *                         precision the reference evaluates these terms in (pyFM/functional.py:379-383).  The two differ in the result:
 *                         energy / gradient within 1e-6 relative, the fitted map within 3e-6 under SciPy's stopping rule.  The Python
 *                         layer chooses it from the stopping rule (engine.py: _fit_fused).
 *   dm_fmap_fit_fused takes no operator lists, so it has no commutativity term: weights[2] (w_dcomm) must be 0, DM_EINVAL otherwise
 *   (a fit with operators goes through dm_fmap_fit_steps; dm_fmap_fit_fused_ok(..., n_ops > 0) says so). */
int dm_fmap_fit_fused_ok(int k1, int k2, const double* weights /*host, 10*/, int n_ops);
int dm_fmap_fit_fused(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2, int D,
                      const float* Phi1, int ld1, const float* Phi2, int ld2, const float* mass1,
                      const float* A, const float* Bm, const double* lam1, const double* lam2,
                      const double* weights /*host, 10*/, int m, const double* x0,
                      double ftol, double pgtol, int maxiter, int maxfun, int maxls, int element_f32,
                      double* x_out, double* f_out, int32_t* info_out, double* grad_out /*nullable*/, int* evaluations_out /*host, nullable*/);

/* ops[b][d] = Phi[b][:, :k]^T diag(mass[b] * F[b][:, d]) Phi[b][:, :k]   (B, D, k, k) fp64: the multiplication operator
 * of descriptor d in the reduced basis.  Replaces commute_left / commute_right of base_functions.py:550-555
 * (pinv @ (descr[:, i, None] * evects), pinv = evects^T A, pyFM/functional.py:416-417).  B * D <= 65535 per call. */
int dm_fmap_descr_ops(dm_ctx* ctx, int B, int N, int D, int k, const float* Phi, int ld, const float* mass,
                      const void* F, int f_dtype, double* ops);

/* ops[b][p] (B, D, k, k) fp64: the orientation operator of descriptor p in the reduced basis of mesh b,
 *   pinv diag(1 / area) W_p Phi,   W_p the sparse operator g -> <n x grad f_p, grad g> summed over the faces around a vertex
 * (pyFM/mesh/geometry.py:919-985 get_orientation_op; one operand of FunctionalMapping.compute_orientation_op, pyFM/functional.py:686-728,
 * and of orientation_op_torch inside energy_func_std, base_functions.py:430-478).  With left = Phi * row_scale[:, None]:
 *   row_scale = mass / vertex_areas: compute_orientation_op's form;  row_scale = null (ones): energy_func_std's (area = diag(A) cancels).
 * verts (B,N,3) fp64, faces (B,M,3) int32 with every index of a used face in [0, N) (the caller checks; the kernels clamp), n_faces
 * (HOST, B; null: M each): faces beyond n_faces[b] are padding and contribute nothing.  F (B,N,D) fp16 | fp32 as staged for the fit.
 * All descriptors of a mesh are ONE float64 matrix-core product (D k) x 3M times 3M x k, split-K into workspace partials added in a fixed
 * order; the split follows from (D, k) alone: a mesh's operators are the same bits in every batch it is part of.  B <= 65535. */
int dm_fmap_orient_ops(dm_ctx* ctx, int B, int N, int M, int D, int k, const double* verts, const int32_t* faces,
                       const int32_t* n_faces, const float* Phi, int ld, const double* row_scale /*nullable*/,
                       const void* F, int f_dtype, double* ops);
int dm_fmap_orient_ops_f64(dm_ctx* ctx, int B, int N, int M, int D, int k, const double* verts, const int32_t* faces,
                           const int32_t* n_faces, const double* Phi, int ld, const double* row_scale /*nullable*/,
                           const void* F, int f_dtype, double* ops);

/* ---- functional map -> vertex maps ---------------------------------------
 * With G = Phi2[:, :k2] C Phi1[:, :k1]^T (never materialised):
 *   knn21[i] = argmin_j |C Phi1_j|^2 - 2 G_ij      (pyFM/spectral/convert.py:138-140)
 *   knn12[j] = argmin_i |Phi2_i C|^2 - 2 G_ij      (pyFM/spectral/convert.py:134-136)
 *   ind21[i] = argmax_j G_ij mass1_j               (convert.py:144 + functional_map.py:49)
 *   ind12[j] = argmax_i G_ij mass1_j               (convert.py:144 + functional_map.py:50)
 * The returned indices are those of the float64 arithmetic above, lowest index on ties.  When all four maps are
 * asked for, N1, N2 >= 256 (any values: operands are padded to whole tiles internally) and k2 >= 65, they come from one pass
 * on the fp16 matrix cores over split operands with a rigorous error bound, every row inside the bound re-evaluated in
 * float64; otherwise from a fused kernel on the f64 matrix cores ("p2p_split" option).
 * Any of the four outputs may be NULL.  knn21/ind21 (B,N2); knn12/ind12 (B,N1). */
int dm_fm_to_p2p(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
                 const float* Phi1, int ld1, const float* Phi2, int ld2,
                 const float* mass1, const double* C,
                 int32_t* knn21, int32_t* knn12, int32_t* ind21, int32_t* ind12);
/* float64 eigenvectors and masses: the reference's own inputs (convert.py:134-144 runs on float64 evects and a float64
 * sparse A1).  The fp16 first pass splits the float64 values directly; its error bound and the exact float64
 * re-evaluation are the same, the masses enter the re-evaluation unrounded. */
int dm_fm_to_p2p_f64(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
                     const double* Phi1, int ld1, const double* Phi2, int ld2,
                     const double* mass1, const double* C,
                     int32_t* knn21, int32_t* knn12, int32_t* ind21, int32_t* ind12);

/* The "p2p_split" mode (1, 2, 3) dm_fm_to_p2p would take for these sizes with the context's options when all four maps
 * are requested, else 0 (the float64 G kernel).  Informational (bench.py reports the dominant kernel of the step); no
 * reference counterpart. */
int dm_fm_to_p2p_uses_split(const dm_ctx* ctx, int N2, int N1, int k);

/* ---- exact nearest neighbour, k = 1 -----------------------------------------
 * out[b,i] = argmin_j |X[b,j,:] - Y[b,i,:]|^2 (lowest j on ties); X (B,nx,p), Y (B,ny,p) fp64.
 * Replaces pyFM/spectral/nn_utils.py:4-38 (knn_query: sklearn kd-tree, k = 1).
 * Exact: a first pass on the fp16 matrix cores with a rigorous error bound, every row inside the bound
 * re-evaluated in float64 from the original operands (also the search inside dm_zoomout / dm_icp;
 * dm_set_option("knn_split", 0) selects the float64 matrix-core kernel for all of it instead). */
int dm_knn_query_f64(dm_ctx* ctx, int B, int nx, int ny, int p,
                     const double* X, const double* Y, int32_t* out /* B*ny */);

/* ---- k nearest neighbours, k > 1 -------------------------------------------------------
 * idx[b,i,r] = index of the r-th nearest row of X[b] to Y[b,i] (ascending distance, lowest index on equal distances),
 * dist (nullable) = the Euclidean distances; idx / dist (B,ny,k).  Replaces pyFM/spectral/nn_utils.py:4-38 for k > 1
 * (sklearn kneighbors).  The k = 1 searches of the matching path use dm_knn_query_f64. */
int dm_knn_query_topk_f64(dm_ctx* ctx, int B, int nx, int ny, int p, int k,
                          const double* X, const double* Y, int32_t* idx, double* dist /*nullable*/);

/* ---- dense mapped indicator --------------------------------------------------
 * M[b] = ((Phi2[:, :k2] C) Phi1[:, :k1]^T) * mass1[None, :]   (B,N2,N1) fp64.
 * Replaces the matrix returned by FM_to_p2p (pyFM/spectral/convert.py:144) for
 * callers that want it; the arg-max maps come from dm_fm_to_p2p without it. */
int dm_mapped_indicator(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
                        const float* Phi1, int ld1, const float* Phi2, int ld2,
                        const float* mass1, const double* C, double* M);
int dm_mapped_indicator_f64(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
                            const double* Phi1, int ld1, const double* Phi2, int ld2,
                            const double* mass1, const double* C, double* M);

/* ---- vertex map -> functional map -----------------------------------------
 * C[b] = Phi2[b][:, :k2]^T (mass2[b] * Phi1[b][p21[b], :k1])   (k2 x k1) fp64.
 * Replaces pyFM/spectral/convert.py:14-51 (p2p_to_FM, A2 given). */
int dm_p2p_to_fm(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
                 const int32_t* p21, const float* Phi1, int ld1, const float* Phi2, int ld2,
                 const float* mass2, double* C);
int dm_p2p_to_fm_f64(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
                     const int32_t* p21, const double* Phi1, int ld1, const double* Phi2, int ld2,
                     const double* mass2, double* C);

/* ---- Laplace-Beltrami eigenbasis -----------------------------------------------------
 * The k smallest eigenpairs of  W phi = lambda A phi  (Phi^T A Phi = I) for B meshes of N vertices each.
 * Replaces the eigensolve of TriMesh.process / laplacian_spectrum (pyFM/mesh/trimesh.py:440-531 -> pyFM/mesh/laplacian.py:
 * 143-182: scipy.sparse.linalg.eigsh(W, k, M=A, sigma=-0.01), ARPACK) by a Chebyshev-filtered subspace iteration.
 * Input: L = A^-1/2 W A^-1/2 in ELL format -- ell_cols (B,N,nnz) int32, ell_vals (B,N,nnz) fp64, padded with (col = row,
 * val = 0) -- and mass (B,N) fp32 = diag(A).  X (B,N,k+guard) fp64: in, a random block (warm_start = 0) or the block a
 * previous call returned (warm_start = 1); out, the orthonormal Ritz vectors of L.  n_iter filtered iterations of
 * polynomial degree `degree` (<= 64; a cold start ramps 4, 8, 16, ... up to it).
 * Output: lam (B,k) fp64 ascending, Phi (B,N,k) fp64 (sign: largest entry of a column positive), resid (B) fp64 =
 * max_j |L x_j - lam_j x_j| over the k wanted pairs -- the caller iterates (warm_start = 1) until it is small enough.
 * ARPACK's output is not reproducible either (random start vector, arbitrary basis of multiple eigenvalues): parity is
 * stated on eigenvalues and invariant subspaces, never on bits.  k + guard <= min(N, 512).
 * warm_start = 2: the dense route for small meshes (where ARPACK, laplacian.py:165, works for any k < N): X = the identity (k + guard =
 * N <= 512), no filter, one Rayleigh-Ritz step = the Jacobi eigendecomposition of L; n_iter / degree are ignored. */
int dm_eigenbasis(dm_ctx* ctx, int B, int N, int nnz, const int32_t* ell_cols, const double* ell_vals, const float* mass,
                  int k, int guard, int n_iter, int degree, int warm_start,
                  double* X, double* lam, double* Phi, double* resid);

/* ---- dense symmetric eigenproblem ---------------------------------------------------------------------------------------
 * The k smallest eigenpairs of B dense symmetric matrices A (B,n,lda) fp64 (only the symmetric part is meaningful: the Gershgorin bound
 * reads columns as rows).  Replaces scipy.sparse.linalg.eigsh(W, k, which='LM', sigma=-1e-6) of the functional map network
 * (pyFM/FMN/FMN.py:293-334), whose W is block-dense.  Same contract as dm_eigenbasis -- Chebyshev-filtered subspace iteration, Rayleigh-Ritz
 * by the Jacobi eigensolver, Cholesky-QR / polar orthonormalisation -- without mass scaling: X (B,n,k+guard) in/out (warm_start = 0: a random
 * block, 1: the block a previous call returned, 2: the identity with k + guard = n <= 512, one Jacobi eigendecomposition of A itself),
 * lam (B,k) ascending, V (B,n,k) orthonormal columns (sign: largest entry of a column positive), resid (B) = max_j |A x_j - lam_j x_j|.
 * Limits: n <= 4096, k + guard <= min(n, 512); anything else is DM_EINVAL. */
int dm_eigh_smallest(dm_ctx* ctx, int B, int n, const double* A, int lda, int k, int guard, int n_iter, int degree, int warm_start,
                     double* X, double* lam, double* V, double* resid);

/* ---- functional map networks (pyFM/FMN/FMN.py) -----------------------------------------------------------------------------
 * A network has n shapes and E directed edges; edge e = (i, j) carries the map maps[e] (stored ldm x ldm, row stride ldm, fp64), of which
 * the leading M x M block is used (M <= ldm, M <= 256).  Every sum runs in a fixed order and an edge's / cycle's result does not depend
 * on what else is in the call.
 *   dm_fmn_orth_defect  out[e] = |FM^T FM - I|_F of the cropped map (FMN.set_isometries, :234-270).
 *   dm_fmn_cycle_costs  cyc_edges (n_cyc,3) int32 = the edge indices (e_ij, e_jk, e_ki) of a three-cycle; cost[c] = the maximum over the
 *                       three rotations of |C_a C_b C_c - I|_F (FMN.get_cycle_weight, :559-594).  The caller validates the indices (MatchEngine.fmn_cycle_costs raises
 *                       ValueError); the kernel clamps an index outside [0, E) so that it never reads outside maps.
 *   dm_fmn_quad_form    W (n M x n M, row stride n M) = the quadratic form of the consistent latent basis (CLB_quad_form, :690-738): per
 *                       edge e = (i, j) with weight w[e], block (i,i) += w FM^T FM, (j,j) += w I, (i,j) -= w FM^T, (j,i) -= w FM, the edges
 *                       added in index order; every block is written, zeros included.  edges (E,2) int32; the caller validates the ends (MatchEngine.fmn_quad_form
 *                       raises ValueError); an edge with an end outside [0, n) writes nothing.
 *   dm_fmn_cclb         canonical consistent latent basis (FMN.compute_CCLB, :336-369): E = sum_i Y_i^T diag(evals[i][:M]) Y_i with
 *                       Y_i = CLB[i][:, :m] (CLB (n,M,M), evals (n,ldl)), symmetrised; (theta, Q) = eigenpairs of E / n ascending (Jacobi, theta as
 *                       Rayleigh quotients of the computed vectors; sign: largest entry of a column of Q positive); cclb[i] = Y_i Q (n,M,m), cclb_evals (m).  m <= M <= 256. */
int dm_fmn_orth_defect(dm_ctx* ctx, int E, int M, const double* maps, int ldm, double* out);
int dm_fmn_cycle_costs(dm_ctx* ctx, int E, int M, const double* maps, int ldm, int n_cyc, const int32_t* cyc_edges, double* cost);
int dm_fmn_quad_form(dm_ctx* ctx, int n, int E, int M, const double* maps, int ldm, const int32_t* edges, const double* w, double* W);
int dm_fmn_cclb(dm_ctx* ctx, int n, int M, int m, const double* CLB, const double* evals, int ldl, double* cclb, double* cclb_evals);

/* The linear assignments of mapped indicators WITHOUT the dense matrices (functional_map.py:57, 78 call
 * scipy.optimize.linear_sum_assignment(mapped_indicator, maximize=True) on the N2 x N1 matrix of pyFM/spectral/convert.py:144).  For maps
 * up to 32 x 32 the kernel evaluates a cost row from the factors E2 = Phi2 C and Phi1, a1 -- the same arithmetic, bit for bit, as
 * dm_mapped_indicator's entries (csrc/dm_indicator_dev.h), so the result is the assignment of that matrix -- and n_dense dense N2 x N1
 * matrices (the precise map, functional_map.py:66) ride in the same launch.  Phi1 (n_ind,N1,ld1), Phi2 (n_ind,N2,ld2), mass1 (n_ind,N1),
 * C (n_ind,k2,k1) fp64; col_of_row (n_ind + n_dense, N2), info (n_ind + n_dense): the indicators first.  dm_lsa_indicator_ok: 1 when
 * the sizes are taken (k1, k2 <= 32, N2 <= N1 <= 2048). */
int dm_lsa_indicator_ok(dm_ctx* ctx, int N1, int N2, int k1, int k2);
int dm_lsa_indicator(dm_ctx* ctx, int n_ind, int N1, int N2, int k1, int k2, const float* Phi1, int ld1, const float* Phi2, int ld2,
                     const float* mass1, const double* C, int n_dense, const double* dense /*nullable*/, int maximize,
                     int32_t* col_of_row, int32_t* info);
int dm_lsa_indicator_f64(dm_ctx* ctx, int n_ind, int N1, int N2, int k1, int k2, const double* Phi1, int ld1, const double* Phi2, int ld2,
                         const double* mass1, const double* C, int n_dense, const double* dense /*nullable*/, int maximize,
                         int32_t* col_of_row, int32_t* info);

/* ---- Laplace-Beltrami operators ---------------------------------------------------------------------------------------
 * What TriMesh.process assembles before its eigensolve (pyFM/mesh/trimesh.py:440-482).
 *   dm_tufted_cover   HOST function (no device, no context, thread safe): the tufted intrinsic-Delaunay cover of one mesh -- the
 *                     construction behind robust_laplacian.mesh_laplacian(V, F, mollify_factor) (external C++ wheel of the reference,
 *                     trimesh.py:465-470): mollified edge lengths, front / back copy of every face glued around every edge,
 *                     intrinsic edge flips until every cover edge is Delaunay.  T (2 nf, 3) int32 corner vertices and L (2 nf, 3)
 *                     fp64 side lengths (side s runs from corner s to corner s + 1) of the cover's triangles; info = [flips,
 *                     converged]; mollify_eps (nullable) = what was added to every length.  Its Laplacian = dm_laplacian_* of
 *                     (T, L) with scale 1/2.
 *   dm_laplacian_rows cotangent stiffness rows and lumped masses of B meshes of N vertices and nt triangles each, on the device, in a
 *                     fixed order of additions.  tri (B,nt,3) int32; len (B,nt,3) fp64 intrinsic side lengths (Heron) or null: from
 *                     verts (B,N,3) fp64 with the reference's arithmetic (laplacian.py:88-140, 5-40).  n_verts (B, nullable): meshes
 *                     with fewer vertices / triangles ride along padded (triangles (-1,-1,-1); vertices >= n_verts[b] become decoupled
 *                     rows at the top of the spectrum).  rows: dm_laplacian_rows_bytes of device memory; max_row (host): longest row.
 *   dm_laplacian_ell  the operands of dm_eigenbasis from those rows: L = A^-1/2 W A^-1/2 in ELL (ell_cols, ell_vals (B,N,nnz), nnz >=
 *                     max_row, padded with (col = row, val = 0)) and mass32 (B,N) = fp32(diag A); optional w_vals (B,N,nnz) = the
 *                     entries of W itself and mass64 (B,N) fp64 (what TriMesh.W / TriMesh.A hold). */
int dm_tufted_cover(int n, int nf, const double* verts /*host*/, const int32_t* faces /*host*/, double mollify_factor,
                    int32_t* T /*host, 2 nf x 3*/, double* L /*host, 2 nf x 3*/, int32_t* info /*host, 2, nullable*/, double* mollify_eps /*host, nullable*/);
/* dm_tufted_cover for `count` meshes on n_threads host threads (<= 0: one per hardware thread); arrays of per-mesh sizes and pointers */
int dm_tufted_cover_batch(int count, const int32_t* n, const int32_t* nf, const double* const* verts, const int32_t* const* faces,
                          double mollify_factor, int32_t* const* T, double* const* L, int32_t* info /*count x 2*/,
                          double* mollify_eps /*count, nullable*/, int n_threads);
size_t dm_laplacian_rows_bytes(int B, int N, int nt);
int dm_laplacian_rows(dm_ctx* ctx, int B, int N, int nt, const int32_t* tri, const double* len /*nullable*/, const double* verts /*nullable*/,
                      double scale, const int32_t* n_verts /*nullable*/, void* rows, int* max_row /*host*/);
int dm_laplacian_ell(dm_ctx* ctx, int B, int N, int nt, const void* rows, int nnz, const int32_t* n_verts /*nullable*/,
                     int32_t* ell_cols, double* ell_vals, float* mass32, double* w_vals /*nullable*/, double* mass64 /*nullable*/);

/* ---- DiffusionNet operators ----------------------------------------------------------------------------------------------
 * What diffusion_net.geometry.compute_operators builds besides its eigensolve (diffusion_net/geometry.py:151-391), for B meshes padded
 * to N vertices and nt triangles (triangles (-1,-1,-1) pad tri; n_verts (B, nullable): the real vertex count of each), float64:
 *   frames (B,N,3,3)  rows bx, by, n.  n = the normalised sum over the incident corners of the unit face normals raw / (|raw| + 1e-6),
 *                     or normals (B,N,3) when given; bx = c - (c.n) n over (norm + 1e-6) with c = e_x where |n.e_x| < 0.9, else e_y;
 *                     by = n x bx.  A vertex whose sum has no direction (unreferenced, exactly cancelling faces) gets a zero frame and
 *                     sets bit 1 of info[b] (device, (B)): the caller repairs the normals and calls again with them.
 *   L                 the weak cotangent Laplacian: for each corner k opposite the edge (i, j), cot = (v_i - v_k).(v_j - v_k) /
 *                     (|(v_i - v_k) x (v_j - v_k)| + denom_eps); L_ii, L_jj += cot / 2, L_ij, L_ji -= cot / 2.  An entry exists for every
 *                     pair of vertices that share a face, whatever its value.
 *   mass              a third of the incident areas + mass_eps * mean over the mesh.
 *   gradX, gradY      per vertex i over the off-diagonal columns j of its row of L: t_j = ((v_j - v_i).bx_i, (v_j - v_i).by_i),
 *                     M = sum_j t_j t_j^T + grad_eps I, g_j = M^-1 t_j (first / second component), g_self = -sum_j g_j in the
 *                     diagonal slot; a vertex without neighbours keeps the single entry g_self = 0.
 * A vertex's contributions are summed in a fixed order: a mesh gives the same bits whatever else shares the call.
 *   dm_dnet_rows  assembly into rows (dm_dnet_rows_bytes of device memory); writes frames and info, reports max_row (host): the longest
 *                 row (<= 64 entries: a vertex of more than 63 neighbours is DM_EINVAL, as in dm_laplacian_rows).
 *   dm_dnet_ell   the rows at the ELL width nnz >= max_row: row_len (B,N); ell_cols (B,N,nnz) sorted by column and padded with (col = row,
 *                 val = 0), the layout dm_laplacian_ell writes; l_vals, gx_vals, gy_vals on those columns; ell_vals = M'^-1/2 (L + shift I)
 *                 M'^-1/2 with M' = the masses rounded to fp32 (mass32), the operand of dm_eigenbasis; mass64.  Padding vertices: zero
 *                 frames and gradient rows, unit mass, a decoupled row at the Gershgorin bound of their mesh's operand.
 * Both calls refuse (DM_EINVAL) an n_verts[b] outside [1, N]; dm_dnet_ell also an nnz below the longest row that dm_dnet_rows left in
 * `rows`.  The checks read a few words back from the device: dm_dnet_rows synchronises the stream twice, dm_dnet_ell once (twice with
 * n_verts). */
size_t dm_dnet_rows_bytes(int B, int N, int nt);
int dm_dnet_rows(dm_ctx* ctx, int B, int N, int nt, const int32_t* tri, const double* verts, const double* normals /*nullable*/,
                 const int32_t* n_verts /*nullable*/, double denom_eps, double grad_eps, void* rows, double* frames, int32_t* info /*device*/,
                 int* max_row /*host*/);
int dm_dnet_ell(dm_ctx* ctx, int B, int N, int nt, const void* rows, int nnz, const int32_t* n_verts /*nullable*/, double mass_eps, double shift,
                int32_t* row_len, int32_t* ell_cols, double* l_vals, double* ell_vals, double* gx_vals, double* gy_vals, double* mass64, float* mass32);

/* ---- DiffusionNet forward pass (inference) --------------------------------------------
 * Replaces the network of diffusion_net/layers.py (LearnedTimeDiffusion with method 'spectral', SpatialGradientFeatures, MiniMLP,
 * DiffusionNetBlock, first_lin / last_lin) for padded batches of B meshes with N vertices.  Every operand is fp32 and every product an
 * fp32 fmaf chain on v_mfma_f32_32x32x2_f32 in ascending order of the contraction index: an output element depends on its own row and
 * column of the operands only, so a mesh has the same bits alone and in any batch.  Matrix operands are row-major with a leading
 * dimension (batch stride N * ld); no pointer needs more than 4-byte alignment.
 *   dm_dnet_linear_f32    out[b,i,:] = act(concat(src_0[b,i,:w_0], .., src_{n_src-1}[b,i,:w]) W^T + bias) + resid[b,i,:]; W (C_out, sum w)
 *                         as nn.Linear stores it; bias, resid nullable; act 0 none, 1 ReLU (applied before resid).  The concatenation
 *                         is never formed.  Order: the chain over the concatenated index, then + bias, act, + resid.
 *   dm_dnet_diffuse_f32   out = evecs (coef * (evecs^T (mass * x))), x (B,N,C), mass (B,N), evals (B,K), evecs (B,N,K), times (C);
 *                         coef[k,c] = exp(-evals[k] max(times[c], 1e-8f)) evaluated in float64 and rounded once.  mass * x is rounded to
 *                         fp32 (as the reference's expression), the sum over the vertices ascends, then the sum over k.  One workgroup
 *                         per (mesh, 32 channels) keeps its K x 32 spectrum in LDS: K <= 1024.
 *   dm_dnet_gradfeat_f32  gX = G_x x, gY = G_y x from ELL rows (row_len (B,N); cols, gx, gy (B,N,nnz): the layout of dm_dnet_ell in
 *                         fp32), entries in stored order; B_re = gX A_re^T - gY A_im^T, B_im = gY A_re^T + gX A_im^T (A_im null:
 *                         B_re = gX A_re^T, B_im = gY A_re^T); out = tanhf(gX * B_re + gY * B_im).  gX / gY are recomputed where a tile
 *                         needs them and never stored.  A stored column outside [0, n_verts) contributes nothing.
 * n_verts (device, nullable): rows i >= n_verts[b] are never read and are written as zeros; ELL slots q >= row_len[i] are never read.
 * DM_EINVAL: B, N, C, K, nnz <= 0, a leading dimension below its width, a null operand, n_verts[b] outside [1, N] (read back: one
 * stream synchronisation per call that passes n_verts). */
int dm_dnet_linear_f32(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* src0, int w0, int ld0, const float* src1, int w1, int ld1,
                       const float* src2, int w2, int ld2, const float* W, int ldw, const float* bias /*nullable*/, const float* resid /*nullable*/,
                       int ldr, int act, const int32_t* n_verts /*nullable*/, float* out, int ldo);
int dm_dnet_diffuse_f32(dm_ctx* ctx, int B, int N, int K, int C, const float* x, int ldx, const float* mass, const float* evals,
                        const float* evecs, int lde, const float* times, const int32_t* n_verts /*nullable*/, float* out, int ldo);
int dm_dnet_gradfeat_f32(dm_ctx* ctx, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx, const float* gy,
                         const float* x, int ldx, const float* A_re, const float* A_im /*nullable*/, int lda, const int32_t* n_verts /*nullable*/,
                         float* out, int ldo);

/* ---- DiffusionNet forward pass (inference), fp16 operands ------------------------------
 * The same network for a module after .half(), as the reference's driver runs it (model.half() under torch.autocast): the three
 * entries above with fp16 matrix operands.  Every product is exact fp16 x fp16 accumulated in fp32 on v_mfma_f32_32x32x16_f16 over
 * ascending chunks of 16 of the contraction index, never split, no atomics; the residual stream and everything one kernel hands to
 * the next stay fp32.  An output element depends on its own row and column of the operands only: a mesh has the same bits alone and
 * in any batch, whatever tile shape the launch picked.  A value is rounded to fp16 (to nearest even) exactly once, at the places
 * named below and nowhere else; a magnitude beyond 65504 becomes infinite there, as in the reference's half route.  fp16 operands
 * need 2-byte alignment only (nn.Linear's (C_out, 835) weight is read where it lies); dtype flags are DM_F16 | DM_F32.
 *   dm_dnet_linear_f16    the expression of dm_dnet_linear_f32.  Each source is fp32 or fp16 (dtype_s); an fp32 source element is
 *                         ROUNDED as it is staged.  W (C_out, sum w) fp16.  bias fp16 or fp32 (bias_dtype), widened exactly; resid fp32.
 *                         Order: the accumulation, + bias, act, + resid, in fp32.  out fp32, or fp16 (out_dtype): that value ROUNDED
 *                         once more.  Tiles: 128 x 128 outputs per workgroup when ceil(C_out / 128) ceil(N / 128) B >= 256 (one for
 *                         every CU), 64 x 64 below; the bits do not depend on it.
 *   dm_dnet_diffuse_f16   evecs_h = fp16(2^e1[b] evecs), mevecs_h = fp16(2^e2[b] mass * evecs) (B,N,K), prepared once per mesh with
 *                         per-mesh integer exponents that put each operand's largest magnitude in [2^14, 2^15)
 *                         (PackedOperators.half_operands): the vertex masses, at the bottom of fp16's normal range, are never rounded
 *                         on their own.  x fp32, ROUNDED as it is staged.  acc = mevecs_h^T x over ascending vertices in fp32;
 *                         coef[k,c] = exp(-evals[k] max(times[c], 1e-8f)) in float64, rounded once to fp32 (times fp16 or fp32, widened
 *                         exactly); d = coef * acc * 2^(14 - e1 - e2), the exact float64 product ROUNDED once to fp16 -- the spectrum at
 *                         the scale of the product back, so that evecs -> s evecs, mass -> mass / s^2 (s a power of two) moves no bit;
 *                         out = 2^-14 (evecs_h d) over ascending k, fp32.  One workgroup per (mesh, 32 channels) keeps d in LDS: K <= 1024.
 *   dm_dnet_gradfeat_f16  gX = G_x x, gY = G_y x in fp32 from the fp32 ELL rows and the fp32 x, as dm_dnet_gradfeat_f32 (the reference
 *                         keeps this product in fp32 under autocast).  gX, gY are ROUNDED only as operands of the products with A_re /
 *                         A_im (fp16, A_im nullable); out = tanhf(gX * B_re + gY * B_im) with the unrounded gX, gY; out fp32.
 *                         Where the rounded gradients of 32 rows fit in LDS for every channel (C <= 768) and ceil(N / 32) B >= 256, a
 *                         workgroup owns 32 rows and gathers them once for all columns; else 64 x 64 tiles gather per column tile,
 *                         as the fp32 kernel.  The bits do not depend on it.
 * n_verts, the leading dimensions and DM_EINVAL as for the fp32 entries; also an unknown dtype flag or an operand not aligned to its
 * element. */
int dm_dnet_linear_f16(dm_ctx* ctx, int B, int N, int C_out, int n_src, const void* src0, int w0, int ld0, int dtype0, const void* src1, int w1,
                       int ld1, int dtype1, const void* src2, int w2, int ld2, int dtype2, const void* W, int ldw, const void* bias /*nullable*/,
                       int bias_dtype, const float* resid /*nullable*/, int ldr, int act, const int32_t* n_verts /*nullable*/, int out_dtype,
                       void* out, int ldo);
int dm_dnet_diffuse_f16(dm_ctx* ctx, int B, int N, int K, int C, const float* x, int ldx, const void* evecs_h, int lde, const void* mevecs_h,
                        int ldm, const int32_t* e1, const int32_t* e2, const float* evals, const void* times, int times_dtype,
                        const int32_t* n_verts /*nullable*/, float* out, int ldo);
int dm_dnet_gradfeat_f16(dm_ctx* ctx, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx, const float* gy,
                         const float* x, int ldx, const void* A_re, const void* A_im /*nullable*/, int lda, const int32_t* n_verts /*nullable*/,
                         float* out, int ldo);

/* ---- DiffusionNet backward pass (training) ---------------------------------------------
 * The gradients of the three fp32 forward entries with respect to their activations and parameters (the operators of a mesh -- mass,
 * evals, evecs, the gradient rows -- are constants).  Everything is fp32; every product is an fp32 fmaf chain on
 * v_mfma_f32_32x32x2_f32 that starts at +0 and runs in ascending order of the contraction index; no atomics.  Operands beyond a mesh's
 * rows, columns or ELL slots are staged as zeros.  Matrix operands are row-major with a leading dimension (batch stride N * ld); no
 * pointer needs more than 4-byte alignment.  n_verts (device, nullable): rows i >= n_verts[b] are never read, and are written as zeros
 * in every gradient of an activation.
 * Order guarantees.
 *   - A gradient with respect to an activation (B,N,.) depends on its own mesh only: the same bits alone and in any batch.
 *   - A gradient with respect to a parameter contracts over the vertices: ONE chain per mesh and element over the mesh's vertices in
 *     ascending order (into the workspace), then the meshes are added in ascending order, ((P_0 + P_1) + P_2) + ..  With B = 1 the
 *     result is P_0.  Neither depends on the CU count or on a tile shape.
 * Workspace: caller-owned device memory of at least the matching dm_dnet_*_bwd_bytes, 4-byte aligned; its contents afterwards are
 * unspecified.  An output that is null is not computed.
 *   dm_dnet_linear_bwd_data_f32    dZ = dY * [Y > 0] for act = 1 (Y: the saved output of the forward call WITHOUT its resid term;
 *                         applied while a tile is staged, never stored), dZ = dY for act = 0 (Y not read).  With resid the forward
 *                         adds it after the activation: its gradient is dY itself, no kernel.
 *                         d_s[b,i,:] = dZ[b,i,:] W[:, off_s : off_s + w_s], the chain over o = 0 .. C_out-1; W is read where it lies.
 *                         Every source has its own output and leading dimension; a null d_s skips that source.
 *   dm_dnet_linear_bwd_weight_f32  P_b[o, off_s + k] = sum_i dZ[b,i,o] src_s[b,i,k] and P_b[o, K_tot] = sum_i dZ[b,i,o] (the chain
 *                         fma(dZ, 1, s)), i ascending over the mesh; dW (C_out, K_tot), db (C_out) = the meshes added in ascending
 *                         order.  Workspace dm_dnet_linear_bwd_bytes(B, C_out, K_tot): the partials (B, C_out, K_tot + 1).
 *   dm_dnet_diffuse_bwd_f32        g = evecs^T dO, s = evecs^T (mass * x) (mass * x rounded to fp32 as in the forward), both over
 *                         ascending vertices; coef as in the forward (float64 exp, rounded once).  H = fl(coef g);
 *                         dx = fl(mass * (evecs H)), the chain over ascending k.  T = fl(fl(fl(evals coef) g) s);
 *                         dtimes[c] = -((m_0 + m_1) + ..), m_b the running sum of T[b,k,c] over ascending k from +0.  The gradient
 *                         is with respect to the clamped time (the caller clamps the parameter in place before the forward).  x is
 *                         read for dtimes only.  Workspace dm_dnet_diffuse_bwd_bytes(B, K, C): H and T (B,K,C) in global memory, no
 *                         spectrum in LDS; K <= 1024, the limit of dm_dnet_diffuse_f32.
 *   dm_dnet_gradfeat_bwd_f32       recomputes gX, gY (the forward's gather chain), B_re, B_im and out = tanhf(gX B_re + gY B_im) with
 *                         the forward's operations; p = fl(dO fl(1 - out^2)), U = fl(p gX), V = fl(p gY).
 *                         dgX = (fl(p B_re) + U A_re) + V A_im, dgY = (fl(p B_im) - U A_im) + V A_re, each product one chain over
 *                         ascending c (A_im null: dgX = fl(p B_re) + U A_re, dgY = fl(p B_im) + V A_re).
 *                         dx = G_x^T dgX + G_y^T dgY as a gather over the rows of the transposed operators (row_len_t (B,N); cols_t,
 *                         gx_t, gy_t (B,N,nnz_t), the union pattern of G_x^T and G_y^T in the layout of the forward's rows): entry
 *                         q of row j adds gx_t dgX[col], then gy_t dgY[col], one fmaf each, q ascending.  The transposed rows are
 *                         read only when dx is asked for.
 *                         Per mesh dA_re_b = U^T gX + V^T gY, dA_im_b = V^T gX - U^T gY: four chains over ascending vertices, one
 *                         sum or difference; then the meshes in ascending order.  Workspace dm_dnet_gradfeat_bwd_bytes(B, N, C):
 *                         gX, gY, U, V, dgX, dgY (B,N,C) and the partials 2 (B,C,C).
 * DM_EINVAL: the conditions of the forward counterpart; act = 1 without Y; K > 1024; dtimes without x; dx (gradfeat) without the
 * transposed rows; dA_im without A_im; a null workspace. */
int dm_dnet_linear_bwd_data_f32(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/, int ldy,
                                int act, const float* W, int ldw, const int32_t* n_verts /*nullable*/, float* d0 /*nullable*/, int w0, int ld0,
                                float* d1 /*nullable*/, int w1, int ld1, float* d2 /*nullable*/, int w2, int ld2);
size_t dm_dnet_linear_bwd_bytes(int B, int C_out, int k_tot);
int dm_dnet_linear_bwd_weight_f32(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/, int ldy,
                                  int act, const float* src0, int w0, int ld0, const float* src1, int w1, int ld1, const float* src2, int w2,
                                  int ld2, const int32_t* n_verts /*nullable*/, void* ws, float* dW /*nullable*/, int lddw, float* db /*nullable*/);
size_t dm_dnet_diffuse_bwd_bytes(int B, int K, int C);
int dm_dnet_diffuse_bwd_f32(dm_ctx* ctx, int B, int N, int K, int C, const float* dO, int lddo, const float* x /*nullable*/, int ldx,
                            const float* mass, const float* evals, const float* evecs, int lde, const float* times,
                            const int32_t* n_verts /*nullable*/, void* ws, float* dx /*nullable*/, int lddx, float* dtimes /*nullable*/);
size_t dm_dnet_gradfeat_bwd_bytes(int B, int N, int C);
int dm_dnet_gradfeat_bwd_f32(dm_ctx* ctx, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx,
                             const float* gy, int nnz_t, const int32_t* row_len_t, const int32_t* cols_t, const float* gx_t, const float* gy_t,
                             const float* dO, int lddo, const float* x, int ldx, const float* A_re, const float* A_im /*nullable*/, int lda,
                             const int32_t* n_verts /*nullable*/, void* ws, float* dx /*nullable*/, int lddx, float* dA_re /*nullable*/,
                             float* dA_im /*nullable*/, int ldda);

/* ---- DiffusionNet backward pass (training), fp16 operands ------------------------------
 * Mixed-precision training: the gradients of the three fp16 forward entries with respect to their activations and to the fp32 MASTER
 * parameters whose fp16 roundings the forward multiplied (W, A_re, A_im fp16 here, rounded by the caller once per step).  Every product
 * is exact fp16 x fp16 accumulated in fp32 on v_mfma_f32_32x32x16_f16, the contraction index in ascending chunks of 16 from a zero
 * accumulator, never split, no atomics.  Operands behind a mesh's rows, a matrix's columns or a row's ELL slots are staged as zeros.  A
 * value is rounded to fp16 (to nearest even; beyond 65504 infinite) once, at the places marked ROUNDED below and nowhere else: a
 * gradient entry below fp16's range is lost there and one beyond it becomes infinite -- loss scaling is the caller's.  Gradients of
 * activations travel between the kernels in fp32.
 * Order guarantees.
 *   - A gradient with respect to an activation depends on its own row and column of the operands only: the same bits alone and in any
 *     batch, whatever tile the element falls in (every product runs in 64 x 64 tiles; no launch picks another shape).
 *   - A gradient with respect to a parameter is ONE fp32 chain per mesh over ascending vertices (into the workspace); then the meshes
 *     are added ((P_0 + P_1) + P_2) + .. in fp32.  It is fp32 and belongs to the fp32 master parameter: the rounding of the matrix is
 *     passed straight through.
 * Workspace, n_verts and null outputs as for the fp32 entries.  fp16 operands need 2-byte alignment only; dtype flags are DM_F16 | DM_F32.
 *   dm_dnet_linear_bwd_data_f16    dZ = dY * [Y > 0] (act = 1, Y the saved fp32 output) or dZ = dY, ROUNDED as it is staged.
 *                         d_s = dZ W_h[:, off_s : off_s + w_s] over ascending o; W_h (C_out, K_tot) fp16 is read where it lies.  Outputs
 *                         fp32, one per source with its own leading dimension; a null d_s skips that source.
 *   dm_dnet_linear_bwd_weight_f16  P_b[o, off_s + k] = sum_i fp16(dZ[b,i,o]) fp16(src_s[b,i,k]): an fp32 source (dtype_s) is ROUNDED as
 *                         it is staged -- the value the forward multiplied -- and an fp16 source is read as it is.  Column K_tot is the
 *                         bias: the same product against the constant 1.  The loads of two stages of the vertex contraction are in
 *                         flight.  dW (C_out, K_tot), db (C_out) fp32.  Workspace dm_dnet_linear_bwd_f16_bytes(B, C_out, K_tot).
 *   dm_dnet_diffuse_bwd_f16        dx = M Phi (coef * Phi^T dO): dm_dnet_diffuse_f16 itself with evecs_h / mevecs_h and e1 / e2
 *                         exchanged -- its roundings (dO as staged; the spectrum once, at the scale 2^(14 - e1 - e2), from the exact
 *                         float64 product) and its bits.  dtimes: g = evecs_h^T fp16(dO), s = mevecs_h^T fp16(x), fp32 accumulators
 *                         over ascending vertices; T[b,k,c] = evals coef g s 2^-(e1 + e2) formed in float64 and rounded once to fp32;
 *                         dtimes[c] = -((m_0 + m_1) + ..), m_b the ascending-k sum of T[b,.,c]; with respect to the clamped time.  x
 *                         is read for dtimes only.  Workspace dm_dnet_diffuse_bwd_f16_bytes(B, K, C): T.  K <= 1024.
 *   dm_dnet_gradfeat_bwd_f16       gX, gY from the fp32 gather chain; B_re, B_im and out recomputed with dm_dnet_gradfeat_f16's
 *                         operations; p = fl(dO fl(1 - out^2)), U = fl(p gX), V = fl(p gY) in fp32.  U, V, gX, gY are ROUNDED only as
 *                         matrix operands: of the products with A_h (dgX = (fl(p B_re) + U A_re) + V A_im,
 *                         dgY = (fl(p B_im) - U A_im) + V A_re, assembled in fp32 in the fp32 entry's order) and of
 *                         dA_re_b = U^T gX + V^T gY, dA_im_b = V^T gX - U^T gY.  dx is the fp32 gather over the transposed rows.
 *                         A_im nullable.  Workspace dm_dnet_gradfeat_bwd_f16_bytes(B, N, C).
 * DM_EINVAL: the conditions of the fp32 entries; also an unknown dtype flag, an operand not aligned to its element, a null workspace. */
int dm_dnet_linear_bwd_data_f16(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/, int ldy,
                                int act, const void* W, int ldw, const int32_t* n_verts /*nullable*/, float* d0 /*nullable*/, int w0, int ld0,
                                float* d1 /*nullable*/, int w1, int ld1, float* d2 /*nullable*/, int w2, int ld2);
size_t dm_dnet_linear_bwd_f16_bytes(int B, int C_out, int k_tot);
int dm_dnet_linear_bwd_weight_f16(dm_ctx* ctx, int B, int N, int C_out, int n_src, const float* dY, int lddy, const float* Y /*nullable*/, int ldy,
                                  int act, const void* src0, int w0, int ld0, int dtype0, const void* src1, int w1, int ld1, int dtype1,
                                  const void* src2, int w2, int ld2, int dtype2, const int32_t* n_verts /*nullable*/, void* ws,
                                  float* dW /*nullable*/, int lddw, float* db /*nullable*/);
size_t dm_dnet_diffuse_bwd_f16_bytes(int B, int K, int C);
int dm_dnet_diffuse_bwd_f16(dm_ctx* ctx, int B, int N, int K, int C, const float* dO, int lddo, const float* x /*nullable*/, int ldx,
                            const void* evecs_h, int lde, const void* mevecs_h, int ldm, const int32_t* e1, const int32_t* e2, const float* evals,
                            const float* times, const int32_t* n_verts /*nullable*/, void* ws, float* dx /*nullable*/, int lddx,
                            float* dtimes /*nullable*/);
size_t dm_dnet_gradfeat_bwd_f16_bytes(int B, int N, int C);
int dm_dnet_gradfeat_bwd_f16(dm_ctx* ctx, int B, int N, int C, int nnz, const int32_t* row_len, const int32_t* cols, const float* gx,
                             const float* gy, int nnz_t, const int32_t* row_len_t, const int32_t* cols_t, const float* gx_t, const float* gy_t,
                             const float* dO, int lddo, const float* x, int ldx, const void* A_re, const void* A_im /*nullable*/, int lda,
                             const int32_t* n_verts /*nullable*/, void* ws, float* dx /*nullable*/, int lddx, float* dA_re /*nullable*/,
                             float* dA_im /*nullable*/, int ldda);

/* ---- heat-method geodesic distances ------------------------------------------------
 * Replaces pyFM's heat method (pyFM/mesh/geometry.py:587-740 heat_geodesic_from / heat_geodmat, behind
 * TriMesh.get_geodesic(robust=False) / geod_from(i, robust=False), pyFM/mesh/trimesh.py:612-738), where SciPy's SuperLU factors
 * A + tW and W (sparse.linalg.factorized) and solves for the sources.  Here, for B meshes padded to N vertices (n_verts, nullable:
 * the real count of each; triangles (-1,-1,-1) pad tri), both systems are assembled dense and factored once (blocked Cholesky in
 * float64, W grounded at vertex 0: row and column 0 replaced by the identity), then solved for any set of sources.
 *   dm_heat_geodesic_bytes   device memory of the factors of B meshes (0 for an invalid size; N <= 16384).
 *   dm_heat_geodesic_factor  tri (B,nt,3) int32, verts (B,N,3) fp64, the stiffness rows of W in ELL (ell_cols (B,N,nnz) int32,
 *                            w_vals (B,N,nnz) fp64: what dm_laplacian_ell writes as w_vals, or rows of a host W; entries outside
 *                            [0, n_verts) must be 0), mass64 (B,N) = diag A, t (B) the heat time of each mesh (trimesh.py:661-665:
 *                            the squared mean edge length).  info (B): 0 ok, else a sum of 1 (A + tW not positive definite), 2 (W not
 *                            positive definite once grounded: more than one connected component), 4 (a face of zero area), 8 (a face
 *                            index or a W column outside [0, n_verts)), 16 (a vertex that no face references).  mass64 must be
 *                            one third of the adjacent face areas (the cotangent lumped mass): only then does A div h lie in W's
 *                            range, so that grounding W changes nothing but the constant the min-shift removes (not checked here:
 *                            the Python layer refuses other masses).
 *   dm_heat_geodesic_solve   D (B,ns,N) fp64: row s of mesh b = the distances FROM vertex sources[b][s] (geometry.py:660-668: phi of
 *                            the heat method minus its minimum, 0 at the source; column j of the reference's matrix); sources (B,ns)
 *                            int32 device, -1 = no source (a row of zeros).  A row's bits do not depend on the other sources or meshes
 *                            of the call.  info (B): 1 if a source lies outside [-1, n_verts).  Work space: 2 B ns ceil64(N) doubles. */
size_t dm_heat_geodesic_bytes(int B, int N, int nt);
int dm_heat_geodesic_factor(dm_ctx* ctx, int B, int N, int nt, const int32_t* tri, const double* verts, const int32_t* ell_cols,
                            const double* w_vals, int nnz, const double* mass64, const double* t, const int32_t* n_verts /*nullable*/,
                            void* factors, int32_t* info);
int dm_heat_geodesic_solve(dm_ctx* ctx, int B, int N, int nt, const void* factors, int ns, const int32_t* sources, double* D,
                           int32_t* info);

/* ---- precise (barycentric) map ----------------------------------------------------
 * For every vertex i of mesh 2 the face of mesh 1 its spectral embedding projects onto and the barycentric coordinates
 * of the projection: face_match (B,N2) int32, bary (B,N2,3) fp64; dense (B,N2,N1) fp64 optional = the same map as a
 * matrix with three weights per row (what get_precise_map().toarray() returns).  faces1 (B,nf,3) int32.
 * Replaces FunctionalMapping.get_precise_map (pyFM/functional.py:221-251 -> pyFM/spectral/convert.py:185-229 with
 * use_adj = True -> pyFM/spectral/projection_utils.py:16-115).  info (B): 1 if some point of the pair had more than 4096
 * candidate faces (such a point re-tests every face instead of walking a list: slower, same result).  Face indices must lie in
 * [0, N1) (the caller checks; the kernel indexes LDS with them).  N1 + k1 <= about 17000. */
int dm_precise_map(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2, int nf,
                   const float* Phi1, int ld1, const float* Phi2, int ld2, const double* C,
                   const int32_t* faces1, int32_t* face_match, double* bary, double* dense /*nullable*/, int32_t* info);
int dm_precise_map_f64(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2, int nf,
                       const double* Phi1, int ld1, const double* Phi2, int ld2, const double* C,
                       const int32_t* faces1, int32_t* face_match, double* bary, double* dense /*nullable*/, int32_t* info);

/* ---- linear assignment ------------------------------------------------------------
 * col_of_row[b][r] = column assigned to row r of cost[b] (nr x nc fp64, device), -1 for an unassigned row (nr > nc).
 * Replaces scipy.optimize.linear_sum_assignment(mapped_indicator, maximize=True) of densematcher/functional_map.py:57,66,78
 * (the `hungarian`, `hungarian_precise`, `hungarian_icp` outputs).  Same algorithm as SciPy's (Crouse 2016, shortest
 * augmenting paths), same floating-point steps and tie rules: the assignment equals SciPy's, not merely its objective.
 * One workgroup per matrix; matrices of a batch run concurrently.  info (B): 0 ok; 1 the matrix is infeasible (no complete
 * assignment of finite cost: SciPy raises ValueError("cost matrix is infeasible")), 2 it holds NaN or an infinity of the
 * rejected sign (SciPy: "matrix contains invalid numeric entries"); col_of_row of such a matrix is not meaningful. */
int dm_linear_sum_assignment(dm_ctx* ctx, int B, int nr, int nc, const double* cost, int maximize,
                             int32_t* col_of_row /* B*nr */, int32_t* info /* B */);

/* ---- many ragged assignments gathered from one matrix -----------------------------
 * Replaces the loop of densematcher/utils.py:115-143 (get_distance_between_groups / get_groups_dmtx: the semantic distance matrix
 * between vertex groups): for every problem p,  scipy.optimize.linear_sum_assignment(S_p)  with  S_p[r][c] = D[b][rows[r]][cols[c]]
 * and the mean of the matched entries.  D (B,N,ld) fp64 device, row stride ld >= N (the padded batches of the geodesic calls), is
 * read where it is.  idx (n_idx) int32 device: every index list of the call, concatenated.  problems (P,6) int32 in HOST memory
 * (the library orders the problems by work, largest first, and uploads the table): mesh b, offset and length nr of the row list in
 * idx, offset and length nc of the column list, offset of the problem's nr outputs in col_of_row.  Lists may repeat indices and
 * overlap.  Indices must lie in [0, N) (the caller checks, as for dm_precise_map; the kernels index D with them).
 * Outputs (device): col_of_row (nullable) packed by the output offsets, -1 for an unassigned row (nr > nc); mean (P) = the matched
 * entries S_p[r][col_of_row[r]] summed over the assigned rows r in ascending order, divided by min(nr, nc); info (P) with the codes
 * of dm_linear_sum_assignment: 0 ok, 1 infeasible, 2 NaN or an infinity of the rejected sign (mean = NaN, col_of_row = -1 there).
 * Same algorithm, floating-point steps and tie rules as SciPy's (the transposed problem is solved when nr > nc, as SciPy does): the
 * assignment equals SciPy's, ties included.  One wavefront per problem for up to 1024 entries on the longer side, the
 * workgroup-per-matrix search of dm_linear_sum_assignment on a gathered copy above; a problem's results do not depend on what else
 * shares the call.  P = 0 is legal (nothing is launched); nr = 0 or nc = 0 is DM_EINVAL.  The call synchronises the stream once
 * (the table's upload). */
int dm_lsa_gather(dm_ctx* ctx, int B, int N, int ld, const double* D, int n_idx, const int32_t* idx, int P,
                  const int32_t* problems /* host, P*6 */, int maximize, int32_t* col_of_row /*nullable*/, double* mean /* P */,
                  int32_t* info /* P */);

/* ---- map quality measures on the geodesic matrices --------------------------------------
 * Replaces the host fancy-indexing of pyFM/eval/evaluate.py: accuracy (:29-36), continuity (:63-66), coverage (:89-91), for P
 * problems on the matrices of a padded batch in ONE launch, and np.max of a distance matrix (the geodesic diameter that
 * diffusion_net/geometry.py:773 normalises by).  No N x N matrix crosses to the host.
 *   dm_map_metrics  D (B,N,ld) fp64 device, read in place (ld >= N: a view with a row stride is accepted, as dm_lsa_gather does;
 *     nullable when every problem is a coverage); D2 (B2,N2,ld2) nullable = D (the matrices that a continuity's edges index);
 *     n_verts (B) / n_verts2 (B2) HOST, nullable = N / N2: the vertex counts of a padded batch; area (B,N) fp64 device, nullable
 *     (the vertex areas of a coverage); idx (n_idx) int32 device: every index list of the call once, lists may be shared between
 *     problems; table (P,8) int32 HOST (the library sorts it by length, longest first, and uploads it), a row being
 *         kind, mesh, mesh2, offset a, offset b, length, aux, flags
 *       kind 0 accuracy:   d[i] = D[mesh][idx[a + i]][idx[b + i]], i < length -- the row from the map, the column from the ground
 *                          truth -- d[i] /= scale[p] element by element when flags & 1, value = sum(d) / length; when flags & 2 the
 *                          d[i] are also written to all[aux + i] (the reference's return_all)
 *       kind 1 continuity: the map is idx[a : a + aux], the edges are (idx[b + e], idx[b + length + e]), e < length;
 *                          value = mean_e( D[mesh][map[e0]][map[e1]] / D2[mesh2][e0][e1] ), IEEE division with no guards (a zero
 *                          length gives inf or NaN and the mean carries it, as NumPy's does)
 *       kind 2 coverage:   value = sum of area[mesh][v] over the DISTINCT values v of idx[a : a + length], divided by the sum of
 *                          area[mesh][:n_verts[mesh]]; length 0 is legal (0 / total)
 *     scale (P) fp64 HOST, nullable; n_all = the elements of `all`.  Outputs (device): value (P), all (nullable), info (P): 0, or 1
 *     where an index lies outside [0, n_verts) of its mesh (value NaN; such an index is never used as an address; the caller
 *     checks its lists, as for dm_lsa_gather).
 *     One workgroup per problem; a sum is taken in an order fixed by the problem alone (256 strided partial sums in ascending
 *     order, then a binary tree), the coverage sums in ascending vertex order (np.unique's): a problem's bits do not depend on
 *     what shares the call, on B, on the padding or on ld.  No floating-point atomics.  N, N2 <= 16384.  P = 0 is legal.
 *     DM_EINVAL for a kind, mesh, offset or length outside its range and for a coverage without `area`.  The call synchronises
 *     the stream once (the table's upload).
 *   dm_geodesic_diameter  out[b] = np.max(D[b, :n, :n]), n = n_verts[b] (HOST, nullable = N): NaN if any entry is NaN (np.max's
 *     rule); rows / columns past n and the columns N..ld are never read.  A two-stage max reduction. */
int dm_map_metrics(dm_ctx* ctx, int B, int N, int ld, const double* D, int B2, int N2, int ld2, const double* D2 /*nullable*/,
                   const int32_t* n_verts /*host, nullable*/, const int32_t* n_verts2 /*host, nullable*/, const double* area /*nullable*/,
                   int n_idx, const int32_t* idx, int P, const int32_t* table /* host, P*8 */, const double* scale /*host, nullable*/,
                   int n_all, double* value /* P */, double* all /*nullable*/, int32_t* info /* P */);
int dm_geodesic_diameter(dm_ctx* ctx, int B, int N, int ld, const double* D, const int32_t* n_verts /*host, nullable*/, double* out /* B */);

/* ---- vertex map -> functional map, least squares -------------------------------
 * C[b] = argmin_X |Phi2[b][:, :k2] X - Phi1[b][p21[b], :k1]|_F   (k2 x k1) fp64, no mass matrix.
 * Replaces pyFM/spectral/convert.py:51 (p2p_to_FM with A2 = None: scipy.linalg.lstsq), the form ICP and ZoomOut on
 * subsampled vertices use.  Normal equations (Phi2^T Phi2) C = Phi2^T Phi1[p21] with one step of iterative refinement; info (B):
 * 0 ok, else the Gram matrix was not positive definite / its inverse did not converge.  Needs N2 >= k2 and Phi2 of full column
 * rank, cond(Phi2) up to ~1e4 (the reference's SVD-based lstsq also returns the minimum-norm solution of rank-deficient
 * problems: those are reported here, not solved).  k2 <= 256.  Phi1 rows may be any (N1 x ld1)
 * matrix (a pulled-back basis P Phi1 with p21 = identity gives the sparse-map form of convert.py:39). */
int dm_p2p_to_fm_lstsq(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
                       const int32_t* p21, const float* Phi1, int ld1, const float* Phi2, int ld2,
                       double* C, int32_t* info);
int dm_p2p_to_fm_lstsq_f64(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
                           const int32_t* p21, const double* Phi1, int ld1, const double* Phi2, int ld2,
                           double* C, int32_t* info);

/* ---- ZoomOut ----------------------------------------------------------------
 * nit times: p21 = knn21(C_k); C_{k+step} = p2p_to_fm(p21) with k+step columns.
 * Replaces pyFM/refine/zoomout.py:7-44,47-115 (with upstream FM_to_p2p
 * semantics).  C0 (B,k0,k0); Cout (B,kf,kf), kf = k0+nit*step;
 * p21_out (B,N2) optional = knn21(Cout).  Needs ld1, ld2 >= kf. */
int dm_zoomout(dm_ctx* ctx, int B, int N1, int N2, int k0, int nit, int step,
               const float* Phi1, int ld1, const float* Phi2, int ld2,
               const float* mass2, const double* C0, double* Cout, int32_t* p21_out /*nullable*/);
int dm_zoomout_f64(dm_ctx* ctx, int B, int N1, int N2, int k0, int nit, int step,
                   const double* Phi1, int ld1, const double* Phi2, int ld2,
                   const double* mass2, const double* C0, double* Cout, int32_t* p21_out /*nullable*/);

/* ---- subsampled ("fast") ZoomOut --------------------------------------------------
 * zoomout.py:95-113 with subsample = (sub1, sub2): the nit iterations run on the rows Phi1[sub1] (n1s), Phi2[sub2] (n2s) with the
 * least-squares p2p_to_FM (no mass, convert.py:51); p21_out (B,N2) optional = knn21(Cout) on ALL vertices (zoomout.py:111-113).
 * sub1 (B,n1s), sub2 (B,n2s) int32 device.  Square map, one step size; kf = k0 + nit*step <= 256.  One device loop without host
 * synchronisation: the rows are gathered and the Gram matrix Phi2s[:, :kf]^T Phi2s[:, :kf] is formed and Cholesky-factored ONCE (the
 * factor of a leading block is the leading block of the factor), every iteration then costs the search of dm_zoomout on the
 * samples, one product and one triangular-solve launch.  info (B): 0 ok, else a sum of 1 (the Gram matrix is not positive definite
 * to 1e-10 of its diagonal: fewer distinct samples than kf, cond(Phi2s) beyond 1e5) and 2 (a sample index outside its mesh; it is
 * clamped, nothing reads outside its arrays).  The results of a flagged pair are meaningless.  A pair's result does not depend on
 * the other pairs of the call. */
int dm_zoomout_sub(dm_ctx* ctx, int B, int N1, int N2, int n1s, int n2s, const int32_t* sub1, const int32_t* sub2,
                   int k0, int nit, int step, const float* Phi1, int ld1, const float* Phi2, int ld2,
                   const double* C0, double* Cout, int32_t* p21_out /*nullable*/, int32_t* info);
int dm_zoomout_sub_f64(dm_ctx* ctx, int B, int N1, int N2, int n1s, int n2s, const int32_t* sub1, const int32_t* sub2,
                       int k0, int nit, int step, const double* Phi1, int ld1, const double* Phi2, int ld2,
                       const double* C0, double* Cout, int32_t* p21_out /*nullable*/, int32_t* info);

/* ---- farthest-point sampling --------------------------------------------------------
 * geometry.py:839-848 (behind TriMesh.extract_fps): out[b][0] = start[b], dists = d(start); size - 1 times new = argmax(dists) (the
 * LOWEST index among equal maxima, like np.argmax), dists = min(dists, d(new)).  out (B,size) int32; vertices >= n_verts[b] are
 * never chosen; with size > n_verts the indices repeat as the reference's do (all distances 0 -> vertex 0).  The whole loop of a
 * mesh runs on the device without host synchronisation, a batch is one call.  N <= 16384.
 *   dm_fps_euclid  d(i) = |V - V[i]| as np.linalg.norm(V - V[i], axis=1) rounds it: sqrt((dx dx + dy dy) + dz dz) in float64 without
 *                  fused multiply-add, correctly rounded square root: the reference's indices.  verts (B,N,3); start is clamped
 *                  into the mesh.
 *   dm_fps_heat    d(i) = row i of dm_heat_geodesic_solve for these factors (TriMesh.geod_from(i, robust=False)); info (B): 1 a
 *                  start outside [0, n_verts), 2 a distance that is not finite. */
int dm_fps_euclid(dm_ctx* ctx, int B, int N, const double* verts, const int32_t* n_verts /*nullable*/, int size,
                  const int32_t* start, int32_t* out);
int dm_fps_heat(dm_ctx* ctx, int B, int N, int nt, const void* factors, int size, const int32_t* start, int32_t* out, int32_t* info);

/* ---- shortest paths along the edges of a mesh -------------------------------------------
 * Replaces scipy.sparse.csgraph.dijkstra on the edge graph of a mesh: all pairs in pyFM/mesh/geometry.py:524-556
 * (geodesic_distmat_dijkstra, behind TriMesh.get_geodesic(dijkstra=True), pyFM/mesh/trimesh.py:612-692, the matrix pyFM.eval.accuracy
 * consumes), and one run per sample in the default TriMesh.extract_fps of this package.  The distances are Dijkstra's BIT FOR BIT:
 * d[v] = the minimum over the paths s -> v of the left-folded float64 sum of the weights, reached by relaxing every edge until a
 * whole sweep changes nothing -- for weights >= 0 that fixed point is unique, whatever the order of the relaxations (DESIGN.md
 * section 4), so a row's bits depend neither on the other sources or meshes of a call nor on how the work is spread over threads.
 * The graph of B meshes padded to N vertices (n_verts, nullable: the real count of each), ELL in VERTEX-MINOR layout:
 * cols (B,nnz,N) int32, w (B,nnz,N) fp64; entry (b,e,v) is an edge INTO vertex v from vertex cols[b][e][v] of weight w[b][e][v]
 * (an undirected graph stores every edge at both ends; a stored weight 0 is an edge), col = -1 pads.  N <= 16384 (8 N bytes of LDS
 * hold the distances of one source).
 *   dm_graph_geodesic  D (B,ns,N) fp64: row s of mesh b = the distances FROM vertex sources[b][s] (row i of csgraph.dijkstra's matrix);
 *                      +inf for a vertex no path reaches; sources (B,ns) int32 device, -1 = no source (a row of zeros); columns past
 *                      n_verts are 0.  One workgroup per source.
 *   dm_fps_graph       farthest-point sampling (see above) with d(i) = row i of dm_graph_geodesic: out (B,size) int32, out[b][0] =
 *                      start[b]; +inf counts as a maximum (the lowest-index vertex of an unreached component is taken next).  One
 *                      workgroup per mesh runs the whole loop in ONE launch; the running minimum stays in LDS and every sample
 *                      relaxes from it (min(m, d_new) exactly), which only touches the new sample's Voronoi region.
 * info (B, zeroed by the caller), a sum of: 1 a source outside [-1, n_verts) / a start outside [0, n_verts) (a row of zeros / clamped);
 * 2 a weight that is negative or NaN (the argument needs w >= 0; such an edge is skipped); 4 a column outside [-1, n_verts) (skipped).
 * The results of a flagged mesh are not meaningful. */
int dm_graph_geodesic(dm_ctx* ctx, int B, int N, int nnz, const int32_t* cols, const double* w, const int32_t* n_verts /*nullable*/,
                      int ns, const int32_t* sources, double* D, int32_t* info);
int dm_fps_graph(dm_ctx* ctx, int B, int N, int nnz, const int32_t* cols, const double* w, const int32_t* n_verts /*nullable*/,
                 int size, const int32_t* start, int32_t* out, int32_t* info);

/* ---- heat / wave kernel signatures -------------------------------------------------
 * The spectral descriptors of FunctionalMapping.preprocess (reference functional.py:308-334; HKS_functions.py:73,97-98,
 * WKS_functions.py:29,71,118-126), scaled form, for B meshes padded to N vertices (n_verts: HOST array (B), nullable = all N):
 *   plain block       S[n, t]   = (sum_k w[t,k] Phi[n,k]^2)        * (1 / sum_k w[t,k])
 *   landmark block p  S_p[n, t] = (sum_k w[t,k] Phi[p,k] Phi[n,k]) * (1 / sum_k w[t,k])
 *   kind 0 (HKS): w[t,k] = exp(-(t[t] mu[k]))      kind 1 (WKS): w[t,k] = exp(-((t[t] - mu[k]) (t[t] - mu[k])) / denom)
 * over the eigen-columns k0 <= k < K of Phi (B,N,ld).  The table is prepared on the host (pyFM/signatures.py: signature_tables):
 *   t (B,T) fp64 DEVICE: times / energies;  mu (B,K) fp64 DEVICE: sorted |lambda| (HKS), their logarithms (WKS; entries before k0
 *   are never read);  denom (B) fp64 DEVICE: 2 sigma^2 (WKS; nullable for HKS);  k0 (B,2) int32 HOST: first column kept by the plain
 *   block and by the landmark blocks (WKS drops lambda <= 1e-5 / <= 1e-2);  landmarks (B,P) int32 HOST, P >= 0;  plain 0 | 1.
 * out (B, N, (plain + P) T), fp64 or (out_f32) fp32 rounded once from the fp64 value; columns [plain | p0 | p1 | ...], T each; rows
 * past n_verts are 0.  Every operation in the argument of exp is rounded on its own, so the arguments are the host's bits; a column
 * whose weights all underflow comes out NaN in every row (0 * inf), as in the reference.  A mesh's result does not depend on the
 * other meshes of the call.  DM_EINVAL: T < 1, k0 >= K for a block kind in use, a landmark outside [0, n_verts), plain + P = 0. */
int dm_spectral_signatures(dm_ctx* ctx, int B, int N, const int32_t* n_verts /*host, nullable*/, int K, const float* Phi, int ld,
                           int kind, int T, const double* t, const double* mu, const double* denom /*nullable for HKS*/,
                           const int32_t* k0 /*host*/, int P, const int32_t* landmarks /*host, nullable when P = 0*/, int plain,
                           int out_f32, void* out);
int dm_spectral_signatures_f64(dm_ctx* ctx, int B, int N, const int32_t* n_verts /*host, nullable*/, int K, const double* Phi, int ld,
                               int kind, int T, const double* t, const double* mu, const double* denom /*nullable for HKS*/,
                               const int32_t* k0 /*host*/, int P, const int32_t* landmarks /*host, nullable when P = 0*/, int plain,
                               int out_f32, void* out);

/* ---- spectral ICP -------------------------------------------------------------
 * nit times: p21 = knn21(C); Chat = argmin |Phi2[:, :k2] X - Phi1[p21, :k1]|_F (no mass);
 * C = U eye(k2,k1) V^T with U S V^T = svd(Chat), i.e. the orthogonal polar factor of Chat.
 * Replaces pyFM/refine/icp.py:10-40,43-107 (fixed nit; functional.py:564 uses nit = 10).
 * C0, Cout (B,k2,k1) fp64; resid (B) fp64 optional = max |Cout^T Cout - I| (convergence of the
 * polar iteration); info (B): 0 ok, c+1 = normal equations not SPD.  k1 <= k2 <= 256 (k2 <= 176: in-LDS Cholesky of
 * Phi2^T Phi2; above: Newton-Schulz inverse on the float64 matrix cores). */
int dm_icp(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
           const float* Phi1, int ld1, const float* Phi2, int ld2,
           const double* C0, int nit, double* Cout, double* resid /*nullable*/, int32_t* info);
int dm_icp_f64(dm_ctx* ctx, int B, int N1, int N2, int k1, int k2,
               const double* Phi1, int ld1, const double* Phi2, int ld2,
               const double* C0, int nit, double* Cout, double* resid /*nullable*/, int32_t* info);

/* ---- shape difference operators ---------------------------------------------------
 * Replaces pyFM/spectral/shape_difference.py:6-98 (area_SD, conformal_SD, compute_SD), batched: B pairs (or B candidate maps) per call.
 * In both entry points inv1 stands for np.linalg.pinv(np.diag(lam1[:k1])) (shape_difference.py:44, :96), which is diagonal:
 *   inv1[i] = 1 / lam1[i]  if |lam1[i]| > 1e-15 max_j<k1 |lam1[j]|,  else exactly 0      (pinv's cut-off at its default rcond)
 * and a cut row leaves as exact +0.
 *   dm_shape_diff_f64      from a functional map FM (B,k2,ldf) fp64, ldf >= k1 (the 'spectral' form):
 *                            SDa = FM^T FM                                              (B,k1,k1)   shape_difference.py:20
 *                            SDc[i][j] = inv1[i] sum_l FM[l][i] (lam2[l] FM[l][j])      (B,k1,k1)   shape_difference.py:44
 *                          lam1 (B,ld_l1), lam2 (B,ld_l2) fp64 device, ld_l1 >= k1, ld_l2 >= k2 (read only for SDc).  Either output may
 *                          be null.  One workgroup per pair and 64 x 64 tile on the f64 matrix cores, l = 0 .. k2 - 1 in order.
 *                          Limits: k1 <= 256, k2 <= 768 (3 k1 at k1 = 256), else DM_EINVAL.
 *   dm_pullback_forms_f64  from a vertex map p21 (B,N2) int32 (the 'semican' form, shape_difference.py:94-96), X = Phi1[p21, :k1]:
 *                            Ga = X^T diag(mass2) X                                     (B,k1,k1)
 *                            Gw = X^T (W2 X),  or diag(inv1) X^T (W2 X) when lam1 is given (the conformal operator itself)
 *                          Phi1 (B,N1,ld1) fp64; W2 as stiffness rows in ELL: ell_cols (B,N2,nnz) int32, w_vals (B,N2,nnz) fp64, the
 *                          layout dm_laplacian_ell writes (`w`, padded with col = row, val = 0) or a host CSR padded with col = -1: a
 *                          column outside [0, n_verts2[b]) contributes nothing.  mass2 (B,N2) fp64.  n_verts1 / n_verts2 (B) HOST,
 *                          nullable = N1 / N2: the vertex counts of a padded batch; rows of p21, mass2 and W2 past n_verts2[b] and
 *                          rows of Phi1 past n_verts1[b] are never read.  lam1 (B,ld_l1) fp64 device, nullable.  Either output may be
 *                          null.  A p21 entry outside [0, n_verts1[b]) is clamped -- nothing is read outside Phi1; callers check
 *                          their maps.  A row of W2 X is formed in registers inside the contraction kernel (nnz gathered rows in
 *                          ELL order), not written to memory.  Limit: k1 <= 256, else DM_EINVAL.  With n_verts1 / n_verts2 the call
 *                          synchronises the stream once (their upload).
 * Every sum runs in a fixed order that depends on the pair alone (vertices in index order inside 512-vertex partials, the partials in
 * order): a pair's bits do not depend on B, on what shares the call, on the padding or on the row strides.  No floating-point
 * atomics. */
int dm_shape_diff_f64(dm_ctx* ctx, int B, int k1, int k2, const double* FM, int ldf, const double* lam1 /*nullable*/, int ld_l1,
                      const double* lam2 /*nullable*/, int ld_l2, double* SDa /*nullable*/, double* SDc /*nullable*/);
int dm_pullback_forms_f64(dm_ctx* ctx, int B, int N1, int N2, int k1, const int32_t* p21, const double* Phi1, int ld1,
                          const int32_t* ell_cols, const double* w_vals, int nnz, const double* mass2,
                          const int32_t* n_verts1 /*host, nullable*/, const int32_t* n_verts2 /*host, nullable*/,
                          const double* lam1 /*nullable*/, int ld_l1, double* Ga /*nullable*/, double* Gw /*nullable*/);

/* ---- multi-view feature lifting -----------------------------------------------------
 * The back-projection of get_features_per_vertex (reference densematcher/projection.py:27-130 with fts given; the simplified mesh's
 * pix2face of render.py:31-53), for B meshes padded to N vertices and nt faces, each seen from up to `views` cameras
 * (n_verts, n_views (B) int32 DEVICE, nullable = N / views).
 *   Cameras: R (B,views,3,3), T (B,views,3) fp64 in the row-vector convention X_view = X_world R + T; x = focal X / Z, y = focal Y / Z
 *   in NDC with +x left, +y up (the defaults of PerspectiveCameras, render.py:31).  Square images only (H == W).
 *   dm_raster_pix2face  (projection.py:60-62,94-101)
 *     proj (B,views,N,4) fp64 out: (x, y, Z, in-frame) per vertex, in-frame = 1 where -1 < x < 1 and -1 < y < 1 (projection.py:100).
 *     pix2face (B,views,H,W) int32: the face nearest to the camera at the centre of pixel (r, c), x_c = 1 - (2c+1)/W, y_r = 1 - (2r+1)/H,
 *       or -1.  A face is skipped when a vertex has Z <= 1e-6 or a non-finite projection, when |signed area| <= 1e-8, or when an index
 *       lies outside [0, n_verts) (-1 pads tri).  A centre is inside where all three barycentric coordinates w_i / area are > 0; depth
 *       z = 1 / sum b_i / Z_i in fp64, rounded to fp32 for the comparison; the smallest z wins, equal z goes to the lowest face index
 *       (a 64-bit integer minimum over (depth bits << 32 | face): independent of the order of faces and workgroups).
 *       given (B) int32 DEVICE, nullable: a mesh with given[b] != 0 keeps the pix2face the caller wrote (any rasteriser's; a face
 *       index outside [0, nt) owns nothing) and only the marks below are made from it.
 *     vis (B,views,N) bytes: 1 for every vertex of a face that owns a pixel (projection.py:94-97), else 0.
 *   dm_lift_features  (projection.py:103-121)
 *     maps (B,5) int64 DEVICE: per mesh the device address of its feature maps and their strides (view, channel, row, col) in
 *     elements, f_dtype DM_F16 | DM_F32: NCHW and channels-last tensors are read where they lie.  For every vertex and every view
 *     (ascending) with vis and in-frame set: grid_sample(ft, -(x, y), align_corners=True), bilinear, zero padding -- taps
 *     ix = (1 - x)/2 (W-1), iy = (1 - y)/2 (H-1), fp32 weights, summed in the order nw, ne, sw, se; a tap outside the image is not
 *     read.  out (B,N,ldo) fp32 = the sum over those views / their number, 0 where no view sees the vertex (projection.py:119-121)
 *     and in rows past n_verts; count (B,N) int32, nullable: the number of views.  At most 64 views.  A vertex's bits depend on its
 *     own mesh only: no floating-point atomics, no sums across workgroups. */
int dm_raster_pix2face(dm_ctx* ctx, int B, int N, int nt, int views, int H, int W, const double* verts, const int32_t* tri,
                       const int32_t* n_verts /*nullable*/, const double* R, const double* T, const int32_t* n_views /*nullable*/,
                       double focal, const int32_t* given /*nullable*/, double* proj, int32_t* pix2face, unsigned char* vis);
int dm_lift_features(dm_ctx* ctx, int B, int N, int views, int C, int H, int W, int f_dtype, const long long* maps,
                     const double* proj, const unsigned char* vis, const int32_t* n_verts /*nullable*/,
                     const int32_t* n_views /*nullable*/, float* out, int ldo, int32_t* count /*nullable*/);

/* ---- textured-mesh rendering ----------------------------------------------------------
 * The hard-Phong views of the raw, textured meshes (reference densematcher/render.py:13-54: pytorch3d's MeshRasterizer with
 * blur_radius 0 and one face per pixel, HardPhongShader, one point light per view, default Materials and BlendParams), for B meshes
 * padded to N vertices and nt faces, each seen from up to `views` <= 64 cameras.  Cameras, pixel centres, the face-skipping rule and
 * ownership are those of dm_raster_pix2face above (the same projection and key-image kernels).  This library's restatement of
 * pytorch3d's defaults, not pinned against pytorch3d:
 *   normals (B,N,3) fp64, in/out: s / max(|s|, 1e-6) with s = the sum over the incident faces, in ascending face order, of
 *     cross(v1 - v0, v2 - v0).  inc_ptr (B,N+1), inc_face (B,n_inc) int32: per vertex the faces of its corners (CSR, one entry per
 *     corner, ascending; entries outside [0, nt) are skipped).  normals_given (B) int32, nullable: a mesh with normals_given[b] != 0
 *     keeps the normals the caller wrote.
 *   per covered pixel: the owner's screen-space barycentrics b_i (the raster's expressions) are perspective-corrected in fp64,
 *     b'_i = (b_i / Z_i) / sum_j (b_j / Z_j), and rounded to fp32; position p, normal n (normalised again, eps 1e-6) and texel are
 *     b'-interpolated in fp32.
 *   tex (B,8) int64 DEVICE per mesh: kind (0 none = white, 1 vertex colours, 2 UV map), the address of the colours (n,3) fp32 or of the
 *     map (Ht,Wt,3) fp32, Ht (kind 1: the number of colour rows), Wt, the address of verts_uvs (n_uv,2) fp32, of faces_uvs (n_fuv,3)
 *     int32, n_uv, n_fuv.  UV: the sample position x = u (Wt-1), y = (1-v)(Ht-1) is clamped to the map; four taps nw, ne, sw, se
 *     (grid_sample of the row-flipped map at 2 uv - 1, bilinear, align_corners, border padding).  A face or UV index outside its
 *     array leaves the texel white.
 *   light (B,views,3) fp64, nullable = the camera centre C = -T R^T.  l = unit(L - p), cos = n.l, v = unit(C - p), r = -l + 2 cos n,
 *     alpha = relu(v.r) [cos > 0]; rgb = (ambient + diffuse relu(cos)) texel + specular alpha^shininess, unit(a) = a / max(|a|, 1e-6).
 *     shade (HOST, 13 floats): ambient, diffuse, specular, background (3 each), shininess.
 *   rgba (B,views,H,W,4) fp32: (rgb, 1) on covered pixels, (background, 0) elsewhere and in views past n_views; no clamping.
 *   zbuf (B,views,H,W) fp32: 1 / sum b_i / Z_i, the fp32 value of the key, -1 on background.  pix2face (B,views,H,W) int32, -1 on
 *     background.  planes (B,views,3,H,W), nullable, p_dtype DM_F16 | DM_F32: the RGB planes in the backbone's layout.
 * No floating-point atomics; a mesh's bits do not depend on what shares the call. */
int dm_render_phong(dm_ctx* ctx, int B, int N, int nt, int views, int H, int W, const double* verts, const int32_t* tri,
                    const int32_t* n_verts /*nullable*/, const double* R, const double* T, const int32_t* n_views /*nullable*/,
                    double focal, const int32_t* inc_ptr, const int32_t* inc_face, int n_inc,
                    const int32_t* normals_given /*nullable*/, double* normals, const long long* tex,
                    const double* light /*nullable*/, const float* shade /*host, 13*/, float* rgba, float* zbuf,
                    int32_t* pix2face, void* planes /*nullable*/, int p_dtype);

/* ---- guided feature upsampling (FeatUp's JBU) -----------------------------------------
 * One 2x stage of JBUStack (reference third_party/featup/featup/upsamplers.py:184-250, JBULearnedRange with guidance_dim 3, key_dim 32,
 * radius 3, inference: the dropouts are identities), for B views.  The guidance is already pooled to the output size (H, W) = (2h, 2w).
 *   dm_jbu_filters_f32  (upsamplers.py:213-243)
 *     guidance (B,3,H,W) fp32, dense.  filters (B,H,W,49) fp32 out: per pixel the combined 7 x 7 kernel, tap t = 7 i + j at offset
 *     (i - 3, j - 3): key = W2 gelu(W1 g + b1) + b2 per pixel (exact-erf GELU); logit_t = temp * <key(reflect(y+i-3), reflect(x+j-3)),
 *     key(y, x)>; softmax over t with the maximum subtracted; times spatial_t; divided by max(sum, 1e-7); then
 *     + 0.1 * (V2 gelu(V1 [kernel, g] + c1) + c2).  Everything fp32: fmaf chains in ascending index order starting from the bias; the
 *     product of two keys as four chains over the channels 0, 1, 2, 3 mod 4, added as (s0 + s1) + (s2 + s3).
 *     params: PACKED block of 6440 floats, offsets in floats:
 *          0  W1 (32,3)      96  b1 (32)     128  W2 (32,32)    1152  b2 (32)                      range_proj.0 / range_proj.3
 *       1184  V1 (49,52): columns 0..48 the kernel, 49..51 the guidance        3732  c1 (49)     fixup_proj.0
 *       3784  V2 TRANSPOSED, (49 in, 52): row k holds V2[:, k], 3 floats of padding             6332  c2 (49)     fixup_proj.3
 *       6384  spatial (49): get_spatial_kernel evaluated by the caller     6436  temp: exp(range_temp) clamped to [1e-4, 1e4]
 *     The key map (B,H,W,32) fp32 is written once to the workspace and re-read.
 *   dm_jbu_apply  (upsamplers.py:245-249)
 *     out[b,c,y,x] = sum_{i,j} filters[b,y,x,7i+j] * P[b,c,y+i,x+j], an fp32 fmaf chain in the order i (outer), j (inner) starting from
 *     zero, P = reflect_pad_3(bicubic_2x(src)) never stored: bicubic with align_corners=False, A = -0.75 and clamped indices; at exactly
 *     2x the weights are (-0.03515625, 0.26171875, 0.87890625, -0.10546875) on texels k-2..k+1 for output 2k and the reverse on k-1..k+2
 *     for 2k+1, applied along x first, then along y, each an fmaf chain over ascending texels.
 *     src (B,C,h,w) fp16 | fp32 and out (B,C,2h,2w) fp32 | fp16 (rounded to nearest even) are addressed through ELEMENT strides (view,
 *     channel, row, col): NCHW, channels-last and views of larger buffers are read and written where they lie.  No atomics; a
 *     view's bits depend on that view alone.
 * DM_EINVAL: H or W below 4 (h or w below 2), a null operand, a negative source stride, output strides that are not positive or that
 * give two elements one address. */
int dm_jbu_filters_f32(dm_ctx* ctx, int B, int H, int W, const float* guidance, const float* params, float* filters);
int dm_jbu_apply(dm_ctx* ctx, int B, int C, int h, int w, int src_dtype, const void* src, long long s_view, long long s_chan,
                 long long s_row, long long s_col, const float* filters, int out_dtype, void* out, long long o_view, long long o_chan,
                 long long o_row, long long o_col);

/* ---- backward of dm_jbu_apply ------------------------------------------------------------
 * The two gradients of out = filters * P, P = reflect_pad_3(bicubic_2x(src)) (reference third_party/featup/featup/adaptive_conv_cuda/
 * adaptive_conv_kernel.cu: adaptive_conv_grad_filters_kernel, adaptive_conv_grad_input_kernel, and the backward of F.pad reflect and
 * F.interpolate bicubic that autograd chains behind the latter), for B views.  Per axis P = A src with A of (2n + 6) x n: row p holds
 * the four bicubic weights of upsampled index reflect(p - 3) on its clamped texels.  All arithmetic is fp32 fmaf; neither P nor its
 * gradient is stored.  gout (B,C,2h,2w) fp32 is addressed through ELEMENT strides (view, channel, row, col) and only read: NCHW,
 * channels-last, views of larger buffers and the all-zero strides of an expanded scalar are read where they lie.
 *   dm_jbu_apply_bwd_filters_f32
 *     gfilt[b,y,x,7i+j] = sum_c gout[b,c,y,x] * P[b,c,y+i,x+j], gfilt (B,2h,2w,49) fp32 dense, 16-byte aligned.  P has the bits
 *     dm_jbu_apply computes; the sum is one fmaf chain over ascending c starting from zero.  Only where the output has fewer than 64
 *     tiles of 16 x 32 pixels the channels are cut into n = min(ceil(C / 4), ceil(64 / tiles), 16) chunks of 4 ceil(ceil(C / 4) / n)
 *     channels -- a function of (C, h, w) alone --, whose chains are added in ascending chunk order by a second launch; the partial
 *     sums (n, B, 2h, 2w, 49) fp32 live in the workspace (at most 127 tiles' worth per chunk set: 12.7 MB per view).
 *     src (B,C,h,w) fp16 | fp32 through element strides, as dm_jbu_apply reads it.
 *   dm_jbu_apply_bwd_source_f32
 *     gsrc = Ay^T gP Ax per (view, channel), gsrc (B,C,h,w) fp32 dense; gP[u,v] = sum_{i,j} gout[u-i,v-j] * filters[u-i,v-j,7i+j]
 *     over the output pixels inside the image, an fmaf chain in the order i (outer), j (inner) starting from zero.  The transposes
 *     are gathers in a fixed order: an upsampled index adds the padded indices that reflect onto it in ascending order, along y then
 *     along x; a texel s adds the upsampled indices 2s-3 .. 2s+4 in ascending order (fmaf from zero), each with the sum of the weights
 *     of its taps that clamp onto s, along x then along y.  filters (B,2h,2w,49) fp32 dense.  No workspace.
 * No atomics, no sum whose order depends on scheduling; a view's bits depend on that view alone, whatever B.
 * DM_EINVAL: h or w below 2 or above 8192, B or C not positive, B above 65535, a null operand, a dtype other than DM_F16 | DM_F32, a
 * negative stride. */
int dm_jbu_apply_bwd_filters_f32(dm_ctx* ctx, int B, int C, int h, int w, int src_dtype, const void* src, long long s_view,
                                 long long s_chan, long long s_row, long long s_col, const float* gout, long long g_view,
                                 long long g_chan, long long g_row, long long g_col, float* gfilt);
int dm_jbu_apply_bwd_source_f32(dm_ctx* ctx, int B, int C, int h, int w, const float* gout, long long g_view, long long g_chan,
                                long long g_row, long long g_col, const float* filters, float* gsrc);

/* ---- aggregation network of the 2D backbone --------------------------------------------
 * The part of the reference between the raw outputs of the frozen backbones and features_lr (densematcher/featurizers/SDDINO.py:53-57,
 * 67-90; modules/projection_network.py:89-123; modules/resnet.py:271-287), inference.  Everything fp32 on rows = pixels, channels
 * last: L levels and B images lie as (L, B, npix, C) with a leading dimension, npix = P_h * P_w, pixel p = y * P_w + x.  The 1x1
 * convolutions are dm_dnet_linear_f32.  No atomics; an image has the same bits alone and in any batch.
 *   dm_agg_gather_f32  (SDDINO.py:53-57, 76-88)
 *     n_src <= 8 sources src0 .. (the rest null), each of R * B images in the order r * B + b, read where they lie.  desc HOST
 *     (n_src, 8) int64: C_s, h_s, w_s, the element strides (image, channel, row, col) and the dtype DM_F16 | DM_F32 of source s.
 *     out (B, npix, ld) fp32: out[b, p, off_s + c] = (sum over r ascending of rot_{-r step}(interp_s(src_s[r B + b, c]))(p)) / R with
 *     off_s the summed widths of the sources in front; the sum starts from zero, the division is a true division.
 *     interp: F.interpolate(bilinear, align_corners=False) to (P_h, P_w) -- source coordinate max(0, (t + 1/2) h_s / P_h - 1/2) in
 *     fp64, weights rounded to fp32, (1-ly)((1-lx) a + lx b) + ly((1-lx) c + lx d); the identity when the sizes agree.
 *     rot_angle: output pixel (y, x) samples at ix = cos xb - sin yb + P_w/2 - 1/2, iy = sin xb + cos yb + P_h/2 - 1/2,
 *     xb = x - P_w/2 + 1/2, yb = y - P_h/2 + 1/2, theta = radians(angle) (torchvision's rotate: positive angles turn counter-clockwise),
 *     bilinear with zero padding: coordinates in fp64, weights in fp32, taps in the order nw, ne, sw, se, a tap outside the map is not
 *     read.  r = 0 or step_deg = 0 takes the pixel itself.  R = 1, step_deg = 0 is the concatenation laid out as rows.
 *   dm_groupnorm_stats_f32
 *     per (image, group) over the npix * C/G values x[img, :, g C/G .. (g+1) C/G): the fp64 sum, then the fp64 sum of squared
 *     deviations from the fp64 mean -- two passes, each thread's elements ascending, the 256 partial sums through a fixed tree --
 *     biased variance, rstd = 1 / sqrt(var + 1e-5); mean, rstd (n_img, G) fp32, each rounded once.
 *   dm_groupnorm_relu_f32
 *     out[img, p, c] = max(0, fmaf((x - mean) * rstd, gamma[level, c], beta[level, c])), level = img / B; gamma, beta (n_img / B, C).
 *   dm_conv3x3_f32
 *     3 x 3, stride 1, zero padding 1, x (L, B, P_h, P_w, C_in) -> out (L, B, P_h, P_w, C_out); w (L, C_out, 9 C_in) with contraction
 *     index k = (3 dy + dx) C_in + c for the input at (y + dy - 1, x + dx - 1, c).  An exact fp32 fmaf chain over ascending k starting
 *     from zero (v_mfma_f32_32x32x2_f32, like dm_dnet_linear_f32); a tap outside the image contributes nothing.
 *   dm_agg_mix_f32
 *     out[b, p, c] = sum over l ascending of mix[l] * max(0, GN3(y3[l, b, p, c]) + GNs(ys[l, b, p, c])), GN as in dm_groupnorm_relu_f32
 *     with the statistics (L * B, G) and affine parameters (L, C) of each branch; the first term is assigned, the rest are added, every
 *     product and sum rounded on its own.  y3, ys (L, B, npix, ld); mix (L) fp32; out (B, npix, ldo).  identity_mask, bit l: level l
 *     has no shortcut convolution (a block with as many channels in as out, resnet.py:280-283): ys[l] holds the block's input and is
 *     added as it is.  L <= 32.
 * DM_EINVAL: a size that is not positive, C not a multiple of G, a leading dimension below its width, a null operand, a negative
 * stride, R > 16, more than 8 sources, more than 32 levels. */
int dm_agg_gather_f32(dm_ctx* ctx, int n_src, const long long* desc, const void* src0, const void* src1 /*nullable*/,
                      const void* src2 /*nullable*/, const void* src3 /*nullable*/, const void* src4 /*nullable*/,
                      const void* src5 /*nullable*/, const void* src6 /*nullable*/, const void* src7 /*nullable*/, int R, int B, int P_h,
                      int P_w, double step_deg, float* out, int ld);
int dm_groupnorm_stats_f32(dm_ctx* ctx, int n_img, int npix, int C, int G, const float* x, int ld, float* mean, float* rstd);
int dm_groupnorm_relu_f32(dm_ctx* ctx, int n_img, int B, int npix, int C, int G, const float* x, int ldx, const float* mean,
                          const float* rstd, const float* gamma, const float* beta, float* out, int ldo);
int dm_conv3x3_f32(dm_ctx* ctx, int L, int B, int P_h, int P_w, int C_in, int C_out, const float* x, int ldx, const float* w,
                   float* out, int ldo);
int dm_agg_mix_f32(dm_ctx* ctx, int L, int B, int npix, int C, int G, const float* y3, int ld3, const float* ys, int lds,
                   const float* mean3, const float* rstd3, const float* gamma3, const float* beta3, const float* means,
                   const float* rstds, const float* gammas, const float* betas, unsigned identity_mask, const float* mix, float* out,
                   int ldo);

/* ---- DINOv2 ViT encoder (inference) --------------------------------------------------------
 * The frozen ViT behind the reference's `dino` tokens (featup/model_utils/extractor_dino.py through densematcher/featurizers/
 * SDDINO.py:27, 49-51): patch embedding, pre-norm blocks with LayerScale, exact GELU.  fp16 operands on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation; the residual stream and the LayerNorm input stay fp32.  Every product is a fixed-order sum over ascending chunks of
 * the contraction index, never split along it, no atomics: an image has the same bits alone and in any batch.  fp16 operands that a
 * kernel reads with 16-byte loads (A, W, qkv, the attention output) are 16-byte aligned with leading dimensions and block strides that
 * are multiples of 8 halves; everything else needs its natural alignment only.
 *   dm_vit_patch_rows_f16
 *     img (n, 3, S, S) fp16 | fp32 through ELEMENT strides (image, channel, row, col) -> out (n P P, Kp) fp16 rows with leading
 *     dimension ldo: row i P P + py P + px, column k = 196 c + 14 dy + dx (Conv2d's flattening) holds (v - mean[c]) / std[c] in fp32
 *     (mean, std: three HOST doubles each, rounded to fp32), rounded once to fp16, v the image resized to (14 P, 14 P) at
 *     (14 py + dy, 14 px + dx): F.interpolate(bilinear, align_corners=False) with the coordinate and weight convention of
 *     dm_agg_gather_f32, the pixel itself when S = 14 P.  Columns 588 .. Kp - 1 are zeros; Kp a multiple of 64.
 *   dm_vit_layernorm_f16
 *     x (M, D) fp32 -> out (M, D) fp16 (out_dtype DM_F16) or fp32: per row the fp64 sum, then the fp64 sum of squared deviations from
 *     the fp64 mean (a lane's elements ascending, 64 partial sums through a fixed tree), biased variance, eps 1e-6;
 *     out = fmaf((float)((x - mean) rstd), gamma, beta), rounded once more for an fp16 output.
 *   dm_vit_linear_f16
 *     out[b] = resid[b] + scale * act(A[b] W^T + bias) for B blocks of Mb rows: A (Mb, K) fp16 rows lda, blocks strideA apart; W (N, K)
 *     fp16 as nn.Linear stores it; bias, scale (N) fp32 and resid (Mb, N) fp32 rows ldr, blocks strideR apart (0 broadcasts one
 *     block), all three nullable; act 0 none, 1 erf-GELU 0.5 v (1 + erff(v / sqrt 2)); out fp32 | fp16, rows ldo, blocks strideO
 *     apart.  Order: the fp32 accumulation, + bias, act, * scale, + resid, each rounded on its own.  out may alias resid.  Any Mb
 *     and N; K a multiple of 64 (the granule).  No operand is read past a row's width.
 *   dm_vit_attention_f16
 *     qkv (n, T, 3 D) fp16, D = 64 heads, row t of image i at qkv + i stride_q + t ldq: q | k | v, heads adjacent within each.
 *     out (n, T, D) fp16: softmax(q k^T / 8) v per (image, head).  Keys in ascending tiles of 32; q scaled by 0.125 in fp16; running
 *     maximum and sum in fp32 (the sum of the unrounded weights), the weights rounded to fp16 for the second product, the output
 *     rescaled at every tile and divided by the sum at the end.  Keys at positions >= T weigh exactly nothing.
 * DM_EINVAL, checked on the host before any launch: a size that is not positive, a null operand, a leading dimension below its width,
 * K not on the granule, a head dimension other than 64, a misaligned 16-byte operand, output blocks that overlap. */
int dm_vit_patch_rows_f16(dm_ctx* ctx, int n, int S, int P, int src_dtype, const void* img, long long s_img, long long s_chan,
                          long long s_row, long long s_col, const double* mean /*host*/, const double* std /*host*/, int Kp, void* out,
                          int ldo);
int dm_vit_layernorm_f16(dm_ctx* ctx, int M, int D, const float* x, int ldx, const float* gamma, const float* beta, int out_dtype,
                         void* out, int ldo);
int dm_vit_linear_f16(dm_ctx* ctx, int B, int Mb, int N, int K, const void* A, int lda, long long strideA, const void* W, int ldw,
                      const float* bias /*nullable*/, const float* scale /*nullable*/, const float* resid /*nullable*/, int ldr,
                      long long strideR, int act, int out_dtype, void* out, int ldo, long long strideO);
int dm_vit_attention_f16(dm_ctx* ctx, int n, int T, int heads, int head_dim, const void* qkv, int ldq, long long stride_q, void* out,
                         int ldo, long long stride_o);

#ifdef __cplusplus
}
#endif
#endif /* DENSEMATCH_H */

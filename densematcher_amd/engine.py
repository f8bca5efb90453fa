"""
MatchEngine: batched matching hot path on one MI355X, bound to libdensematch through ctypes.

PyTorch is used for device memory and streams only: every method takes / returns
torch tensors that live on the engine's GPU and hands their `data_ptr()` to the
C ABI (include/densematch.h).  All arithmetic of the path runs in the HIP kernels.

Batch layout (B pairs; pairs are independent):
    Phi1 (B,N1,ld1) f32|f64  Phi2 (B,N2,ld2) f32|f64   eigenvectors (first k columns are used)
    lam1 (B,k1) f64          lam2 (B,k2) f64           eigenvalues
    a1 (B,N1) f32|f64        a2 (B,N2) f32|f64         lumped masses
  (float64 eigenvectors / masses -- the reference's own dtype, pyFM/mesh/trimesh.py:118 -- take the *_f64 entry points
   of the vertex-map, refinement and conversion calls; the projection consumes fp32 like the reference's fit does)
    F1 (B,N1,D) f16|f32   F2 (B,N2,D) f16|f32    descriptors
    C  (B,k2,k1) f64                              functional maps
    maps int32 on the device
"""
import ctypes as C

import torch

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class _KeepAlive(tuple):
    """an argument tuple that also holds the tensors its raw pointers refer to"""


def heat_geodesic_check(V, F, mass, b=0):
    """Host checks of one mesh of MatchEngine.heat_geodesic_factor; ValueError where the reference's SuperLU fails or returns
    numbers that depend on its pivoting:
    * more than one connected component (vertices that no face references included): W is singular beyond its constant;
    * lumped masses that are not one third of the adjacent face areas (e.g. those of process(robust=True), the intrinsic
      Laplacian's): W phi = A div h is then inconsistent -- sum_i A_i div_i = 0 holds only for A_i = va_i, since
      sum_i va_i div_i = sum_f area_f (sum_c grad phi_c) . h_f = 0 -- and its solution depends on where W is grounded."""
    import numpy as np
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    n = V.shape[0]
    if V.ndim != 2 or V.shape[1] != 3:
        raise ValueError(f"heat_geodesic_factor: mesh {b}: vertices must be (n, 3)")
    if F.ndim != 2 or F.shape[1] != 3 or F.size == 0 or F.min() < 0 or F.max() >= n:
        raise ValueError(f"heat_geodesic_factor: mesh {b}: faces must be (m, 3) indices into the {n} vertices")
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]]])
    G = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    ncomp = connected_components(G, directed=False)[0]
    if ncomp != 1:
        raise ValueError(f"heat_geodesic_factor: mesh {b} has {ncomp} connected components (vertices that no face references "
                         "count as components of their own): the heat method's W is singular beyond its constant there "
                         "(the reference's SuperLU fails or returns pivot-dependent numbers)")
    mass = np.asarray(mass, np.float64).ravel()
    if len(mass) != n:
        raise ValueError(f"heat_geodesic_factor: mesh {b}: {len(mass)} masses for {n} vertices")
    area = 0.5 * np.linalg.norm(np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]), axis=1)
    va = np.zeros(n)
    np.add.at(va, F.ravel(), np.repeat(area / 3.0, 3))
    dev = np.abs(mass - va)
    if not np.all(dev <= 1e-8 * va):
        i = int(np.argmax(np.where(va > 0, dev / np.maximum(va, 1e-300), np.inf)))
        raise ValueError(f"heat_geodesic_factor: mesh {b}: the lumped mass A is not one third of the adjacent face areas (vertex {i}: "
                         f"{mass[i]:.6g} against {va[i]:.6g}), as after process(robust=True): W phi = A div h is then inconsistent, "
                         "and its solution depends on the solver's pivoting (the reference's SuperLU) or on the ground vertex.  Use "
                         "the cotangent Laplacian's W and A (process(robust=False) on a fresh mesh)")


class GraphTooWide(ValueError):
    """a graph outside what dm_graph_geodesic / dm_fps_graph take (more than 16384 vertices, a degree above
    MatchEngine.GRAPH_MAX_DEGREE): the mesh layer answers it with SciPy's Dijkstra on the host, the same bits"""


class MatchEngine:
    def __init__(self, device=None, lib_path=None):
        if not torch.cuda.is_available():
            raise RuntimeError("MatchEngine needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.lib = _lib.load(lib_path)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   (device if isinstance(device, int) else torch.device(device).index or 0))
        self.stream = torch.cuda.current_stream(self.device)
        ctx = C.c_void_p()
        rc = self.lib.dm_create(self.device.index, C.c_void_p(self.stream.cuda_stream), C.byref(ctx))
        if rc != 0:
            raise _lib.DenseMatchError(f"dm_create failed with status {rc}: {self.lib.dm_last_error(None).decode()}")
        self.ctx = ctx
        self._options = dict(self.OPTION_DEFAULTS)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.dm_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _chk(self, rc):
        _lib.raise_for(rc, self.lib, self.ctx)

    def _dev(self, t, dtype, name):
        # The context launches on the stream it was created on; temporaries and outputs come from torch's caching
        # allocator, which recycles a block as soon as the *current* stream is done with it.  Using an engine under
        # another stream would let blocks be reused while our kernels still run: refuse it.
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:
            raise RuntimeError("MatchEngine is bound to the stream it was created on; create one engine per stream "
                               "(default_engine() does) instead of calling it under torch.cuda.stream(other)")
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            t = t.to(device=self.device, dtype=dtype).contiguous()
        return t

    def _reals(self, *arrays):
        """Eigenvector / mass arrays of one call on the device in ONE dtype: float64 if any of them is float64 (then the
        *_f64 entry points run: the reference's arithmetic on its own inputs), else float32.  None entries pass through.
        Returns (suffix, arrays...) with suffix "" or "_f64"."""
        def dt(a):
            return a.dtype if isinstance(a, torch.Tensor) else getattr(a, "dtype", None)
        f64 = any(a is not None and str(dt(a)).endswith("float64") for a in arrays)
        tdt = torch.float64 if f64 else torch.float32
        return ("_f64" if f64 else "",) + tuple(None if a is None else self._dev(a, tdt, "real") for a in arrays)

    def synchronize(self):
        self.stream.synchronize()

    OPTION_DEFAULTS = {"simnn_pipe": 1, "simnn_persist": 1, "knn_split": 1, "p2p_split": 2, "solve_packed": 0, "solve_reg": 1, "simnn_band": 4, "lsa_reg": 2, "simnn_big": 0, "energy_keep_gram": 0,
                       "p2pfm_direct": 1, "zoomout_fused": 1, "proj_onepass": 1, "fit_mfma": 1, "basis_stats": 1, "solve_pcg": 1,
                       "zoomout_sub_fused": 1, "fps_heat_route": 0, "graph_geod_device": 1, "fmn_eig_route": 0}

    def set_option(self, name, value):
        """Choose between code paths of the library (include/densematch.h: dm_set_option).  Most settings return the same
        results bit for bit; four change bits -- "solve_pcg", "fit_mfma", "zoomout_sub_fused" and "fmn_eig_route".  "solve_pcg" (the
        batched iteration in front of the direct solvers): its C agrees with
        solve_pcg = 0 to max(1e-9, 4 (n + D) u kappa) relative per system of condition number kappa (u = 2^-53,
        tests/test_gpu_solver_conditioning.py); "fit_mfma" chooses the summation order of the products in the fused fit's fp32
        element loop (fitted maps within 1e-6 of each other); "zoomout_sub_fused" chooses
        between the one-factor device loop of subsampled ZoomOut (1) and the host-chained least-squares steps (0): the maps agree
        to 1e-9, not bit for bit; "graph_geod_device" chooses between the device kernels (1) and SciPy's Dijkstra on the host (0) for
        shortest paths along mesh edges (the default extract_fps / extract_fps_many, get_geodesic(dijkstra=True)): the two settings
        agree bit for bit; "fmn_eig_route" chooses the route of eigh_smallest (0 by the sizes, 1 the full Jacobi eigendecomposition, 2 the
        filtered iteration): eigenvalues and invariant subspaces agree to the residual, not bit for bit."""
        self._chk(self.lib.dm_set_option(self.ctx, name.encode(), int(value)))
        self._options[name] = int(value)

    def get_option(self, name):
        """the value set_option last gave `name` on this engine (its default otherwise)"""
        return self._options[name]

    def reset_options(self):
        for k, v in self.OPTION_DEFAULTS.items():
            self.set_option(k, v)

    @staticmethod
    def split_depth(k):
        """fp16 contraction depth of the split features for a float64 depth k (dm_knnsplit.hip: 3 entries per index + 8
        bias slots, padded to the 32-wide stage, at least 96)."""
        return max(96, -(-(8 + 3 * k) // 32) * 32)

    def p2p_split_active(self, N2, N1, k):
        """0 when fm_to_p2p runs the float64 kernel for these sizes, 1: two passes of the two-key fp16 tile kernel, 2: one
        pass in both directions (bench.py names its dominant kernel accordingly)."""
        return int(self.lib.dm_fm_to_p2p_uses_split(self.ctx, int(N2), int(N1), int(k)))

    def last_requeued_rows(self):
        """rows of the last fm_to_p2p / simnn call that took the exact float64 path, per reduction (knn21, ind21, knn12, ind12;
        -1: not applicable) -- include/densematch.h: dm_last_requeued_rows"""
        out = (C.c_int * 4)()
        self._chk(self.lib.dm_last_requeued_rows(self.ctx, out))
        return [int(x) for x in out]

    def workspace_bytes(self):
        return int(self.lib.dm_workspace_bytes(self.ctx))

    def profile_kernel(self, name):
        self._chk(self.lib.dm_profile_kernel(self.ctx, name.encode() if name else None))

    def profile_read(self):
        n, ms = C.c_int(0), C.c_double(0.0)
        self._chk(self.lib.dm_profile_read(self.ctx, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    PEAK_PROBES = {"mfma_f16_zero_operands": 0, "mfma_f16_random_operands": 1, "mfma_f64": 2, "hbm_copy": 3}

    def measure_peak(self, which):
        """on-box peak probe (include/densematch.h: dm_measure_peak): FLOP/s, or bytes/s for "hbm_copy" """
        v = C.c_double(0.0)
        self._chk(self.lib.dm_measure_peak(self.ctx, self.PEAK_PROBES[which], C.byref(v)))
        return v.value

    def profile_report(self, kernels=False):
        """after profile_kernel("*"): {kernel name: (launches, total ms)} of every launch since, in order of first launch;
        kernels=True adds a third entry, the tuple of distinct kernel expressions launched under that name (e.g.
        "fmap_solve_reg_kernel<8>" under "fmap_solve_chol")"""
        buf = C.create_string_buffer(1 << 16)
        self._chk(self.lib.dm_profile_report(self.ctx, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms, syms = line.split("\t")
            out[name] = (int(n), float(ms), tuple(syms.split(";"))) if kernels else (int(n), float(ms))
        return out

    # ------------------------------------------------------------------ ops
    def simnn(self, Ftgt, Fsrc, return_scores=False):
        """nn[b,i] = argmax_j <Ftgt[b,i], Fsrc[b,j]> (float64-exact, lowest index on ties)."""
        Ftgt = self._dev(Ftgt, torch.float16, "Ftgt")
        Fsrc = self._dev(Fsrc, torch.float16, "Fsrc")
        if Ftgt.dim() != 3 or Fsrc.dim() != 3 or Ftgt.shape[0] != Fsrc.shape[0] or Ftgt.shape[2] != Fsrc.shape[2]:
            raise ValueError("simnn expects Ftgt (B,N2,D) and Fsrc (B,N1,D)")
        B, N2, D = Ftgt.shape
        N1 = Fsrc.shape[1]
        nn = torch.empty((B, N2), dtype=torch.int32, device=self.device)
        best = torch.empty((B, N2), dtype=torch.float32, device=self.device) if return_scores else None
        margin = torch.empty((B, N2), dtype=torch.float32, device=self.device) if return_scores else None
        self._chk(self.lib.dm_simnn_f16(self.ctx, B, N2, N1, D, _ptr(Ftgt), _ptr(Fsrc), _ptr(nn), _ptr(best), _ptr(margin)))
        return (nn, best, margin) if return_scores else nn

    def project(self, Phi, mass, F, k=None, out=None, exact=False):
        """Phi[:, :k]^T (mass * F)  ->  (B,k,D) f32.  fp16 descriptors use the fp16 matrix cores (split basis,
        relative error ~1e-6); exact=True or fp32 descriptors use the float64 matrix cores.
        The one-pass kernel ("proj_onepass" = 1) reads descriptor rows in dwords: fp16 descriptors that start at an odd element (a view
        cut at an odd offset) take the two-launch kernels instead -- the same result to 2e-6 of sum |mass Phi| |F|, not the same bits."""
        sfx, Phi, mass = self._reals(Phi, mass)
        if not isinstance(F, torch.Tensor):
            F = torch.as_tensor(F)
        fdt = torch.float16 if F.dtype == torch.float16 else torch.float32
        F = self._dev(F, fdt, "F")
        B, N, ld = Phi.shape
        k = ld if k is None else k
        if F.shape[:2] != (B, N) or mass.shape != (B, N):
            raise ValueError("project: Phi (B,N,ld), mass (B,N), F (B,N,D) do not agree")
        D = F.shape[2]
        if out is None:
            out = torch.empty((B, k, D), dtype=torch.float32, device=self.device)
        self._chk(getattr(self.lib, "dm_project" + sfx)(self.ctx, B, N, D, k, _ptr(Phi), ld, _ptr(mass), _ptr(F),
                                      (_lib.DM_F16 if fdt == torch.float16 else _lib.DM_F32) |
                                      (_lib.DM_PROJECT_F64 if exact else 0), _ptr(out)))
        return out

    def c00(self, Phi1, Phi2, a1, a2):
        sfx, Phi1, Phi2, a1, a2 = self._reals(Phi1, Phi2, a1, a2)
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        out = torch.empty((B,), dtype=torch.float64, device=self.device)
        self._chk(getattr(self.lib, "dm_fmap_c00" + sfx)(self.ctx, B, N1, N2, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(a1), _ptr(a2), _ptr(out)))
        return out

    def fmap_fit(self, Phi1, Phi2, a1, a2, F1, F2, lam1, lam2, w_descr, w_lap, k1=None, k2=None, check=True):
        """project(mesh 1) + project(mesh 2) + c00 + fmap_solve in one library call (dm_fmap_fit): the same C bit for bit; the
        projected descriptors are not returned.  fp16 descriptors (on a dword boundary for the one-pass projection, see project: a view that
        starts at an odd element takes the two-launch kernels, C within 1e-6, not the same bits)."""
        sfx, Phi1, Phi2, a1, a2 = self._reals(Phi1, Phi2, a1, a2)
        F1 = self._dev(F1, torch.float16, "F1")
        F2 = self._dev(F2, torch.float16, "F2")
        lam1 = self._dev(lam1, torch.float64, "lam1")
        lam2 = self._dev(lam2, torch.float64, "lam2")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        k1 = lam1.shape[1] if k1 is None else k1
        k2 = lam2.shape[1] if k2 is None else k2
        D = F1.shape[2]
        if (F1.shape[:2] != (B, N1) or F2.shape != (B, N2, D) or a1.shape != (B, N1) or a2.shape != (B, N2) or lam1.shape != (B, k1)
                or lam2.shape != (B, k2)):
            raise ValueError("fmap_fit: shapes do not agree")
        Cm = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        info = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(getattr(self.lib, "dm_fmap_fit" + sfx)(self.ctx, B, N1, N2, D, k1, k2, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(a1), _ptr(a2),
                                                         _ptr(F1), _ptr(F2), _ptr(lam1), _ptr(lam2), float(w_descr), float(w_lap),
                                                         _ptr(Cm), _ptr(info)))
        if check:
            bad = torch.nonzero(info).flatten()
            if bad.numel():
                raise _lib.DenseMatchError(
                    f"functional-map system not positive definite for pairs {bad.tolist()[:8]} "
                    f"(row {int(info[bad[0]]) - 1}): descriptors are rank deficient in the basis and w_lap cannot fix it")
        return Cm

    def fmap_solve(self, A, Bm, lam1, lam2, c00, w_descr, w_lap, check=True, return_info=False):
        """Closed-form minimiser of the w_descr / w_lap energy -> C (B,k2,k1) f64; return_info=True: (C, info (B,) int32), info[b] =
        1 + the index of a row of C whose system is not positive definite (0: every system of pair b was solved)."""
        A = self._dev(A, torch.float32, "A")
        Bm = self._dev(Bm, torch.float32, "Bm")
        lam1 = self._dev(lam1, torch.float64, "lam1")
        lam2 = self._dev(lam2, torch.float64, "lam2")
        c00 = self._dev(c00, torch.float64, "c00")
        B, k1, D = A.shape
        k2 = Bm.shape[1]
        if Bm.shape[0] != B or Bm.shape[2] != D or lam1.shape != (B, k1) or lam2.shape != (B, k2) or c00.shape != (B,):
            raise ValueError("fmap_solve: shapes do not agree")
        Cm = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        info = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_fmap_solve(self.ctx, B, k1, k2, D, _ptr(A), _ptr(Bm), _ptr(lam1), _ptr(lam2), _ptr(c00),
                                         float(w_descr), float(w_lap), _ptr(Cm), _ptr(info)))
        if check:
            bad = torch.nonzero(info).flatten()
            if bad.numel():
                raise _lib.DenseMatchError(
                    f"functional-map system not positive definite for pairs {bad.tolist()[:8]} "
                    f"(row {int(info[bad[0]]) - 1}): descriptors are rank deficient in the basis and w_lap cannot fix it")
        return (Cm, info) if return_info else Cm

    WEIGHT_ORDER = ("w_descr", "w_lap", "w_dcomm", "w_p2p", "w_stochastic", "w_ent", "w_range01", "w_sumto1", "w_area", "w_conformal")

    def descr_ops(self, Phi, mass, F, k=None):
        """Multiplication operators of the descriptors in the reduced basis, Phi^T diag(mass * f_d) Phi -> (B,D,k,k) f64
        (reference base_functions.py:550-555)."""
        Phi = self._dev(Phi, torch.float32, "Phi")
        mass = self._dev(mass, torch.float32, "mass")
        if not isinstance(F, torch.Tensor):
            F = torch.as_tensor(F)
        fdt = torch.float16 if F.dtype == torch.float16 else torch.float32
        F = self._dev(F, fdt, "F")
        B, N, ld = Phi.shape
        k = ld if k is None else k
        D = F.shape[2]
        ops = torch.empty((B, D, k, k), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_fmap_descr_ops(self.ctx, B, N, D, k, _ptr(Phi), ld, _ptr(mass), _ptr(F),
                                             _lib.DM_F16 if fdt == torch.float16 else _lib.DM_F32, _ptr(ops)))
        return ops

    def orientation_ops(self, verts, faces, Phi, F, k=None, row_scale=None, n_faces=None):
        """Orientation operators of the descriptors in the reduced basis -> (B,D,k,k) f64 on the device: per descriptor p
        pinv diag(1 / area) W_p Phi with W_p the sparse operator g -> <n x grad f_p, grad g> (reference geometry.py:919-985; what
        FunctionalMapping.compute_orientation_op assembles per descriptor on the host).  All descriptors of a mesh are one float64
        matrix-core product (dm_fmap_orient_ops); a mesh's result does not depend on the batch it is in.
        verts (B,N,3) f64, faces (B,M,3) integer, Phi (B,N,ld) f32 | f64 (the first k columns are used), F (B,N,D) f16 | f32.
        row_scale (B,N) f64: the rows of the left factor are row_scale * Phi -- mass / vertex_areas gives compute_orientation_op's
        operators (area="vertex"), None (ones) those of area="mass", which energy_func_std builds (base_functions.py:567-597).
        n_faces (B): meshes with fewer faces are padded to M rows; rows beyond n_faces[b] are not read as faces.
        A face index outside [0, N) is a ValueError, checked on the host before anything is uploaded."""
        import numpy as np
        fh = faces.cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        if fh.ndim != 3 or fh.shape[2] != 3 or fh.shape[1] == 0 or not np.issubdtype(fh.dtype, np.integer):
            raise ValueError("orientation_ops: faces must be (B, M, 3) integers")
        B, M = fh.shape[:2]
        sfx, Phi = self._reals(Phi)
        if Phi.dim() != 3 or Phi.shape[0] != B:
            raise ValueError("orientation_ops: Phi must be (B, N, ld)")
        _, N, ld = Phi.shape
        k = ld if k is None else int(k)
        nf = None
        if n_faces is not None:
            nf = np.ascontiguousarray(np.asarray(n_faces).reshape(-1), dtype=np.int32)
            if nf.shape != (B,) or nf.min() < 0 or nf.max() > M:
                raise ValueError(f"orientation_ops: n_faces must be (B,) counts in [0, {M}]")
        used = fh if nf is None else fh[np.arange(M)[None, :] < nf[:, None]]
        if used.size and (used.min() < 0 or used.max() >= N):
            raise ValueError(f"orientation_ops: face index outside [0, {N})")
        verts = self._dev(verts, torch.float64, "verts")
        if verts.shape != (B, N, 3):
            raise ValueError("orientation_ops: verts must be (B, N, 3) for the N rows of Phi")
        faces_d = self._dev(np.ascontiguousarray(fh, dtype=np.int32), torch.int32, "faces")
        if not isinstance(F, torch.Tensor):
            F = torch.as_tensor(F)
        fdt = torch.float16 if F.dtype == torch.float16 else torch.float32
        F = self._dev(F, fdt, "F")
        if F.dim() != 3 or F.shape[:2] != (B, N):
            raise ValueError("orientation_ops: F must be (B, N, D)")
        D = F.shape[2]
        if row_scale is not None:
            row_scale = self._dev(row_scale, torch.float64, "row_scale")
            if row_scale.shape != (B, N):
                raise ValueError("orientation_ops: row_scale must be (B, N)")
        ops = torch.empty((B, D, k, k), dtype=torch.float64, device=self.device)
        fn = getattr(self.lib, "dm_fmap_orient_ops" + sfx)
        self._chk(fn(self.ctx, B, N, M, D, k, _ptr(verts), _ptr(faces_d), None if nf is None else nf.ctypes.data_as(C.c_void_p), _ptr(Phi), ld,
                     _ptr(row_scale), _ptr(F), _lib.DM_F16 if fdt == torch.float16 else _lib.DM_F32, _ptr(ops)))
        return ops

    def energy_grad(self, Cm, A, Bm, lam1, lam2, weights, Phi1=None, Phi2=None, a1=None, ops1=None, ops2=None):
        """Energy (B,) and gradient (B,k2,k1) of the functional-map objective for the weights in `weights` (dict with keys
        of WEIGHT_ORDER; reference energy_func_std / grad_energy_std, base_functions.py:480-763)."""
        ev = self._energy_grad_args(Cm, A, Bm, lam1, lam2, weights, Phi1, Phi2, a1, ops1, ops2)
        Cm = ev[-1]
        B, k2, k1 = Cm.shape
        energy = torch.empty((B,), dtype=torch.float64, device=self.device)
        grad = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_fmap_energy_grad(self.ctx, *ev[:-1], _ptr(Cm), _ptr(energy), _ptr(grad)))
        return energy, grad

    def _energy_grad_args(self, Cm, A, Bm, lam1, lam2, weights, Phi1=None, Phi2=None, a1=None, ops1=None, ops2=None):
        """the argument list dm_fmap_energy_grad and dm_fmap_fit_steps share (B ... weights), followed by the map tensor; the tensors
        behind the pointers are kept alive by the tuple"""
        Cm = self._dev(Cm, torch.float64, "C")
        A = self._dev(A, torch.float32, "A")
        Bm = self._dev(Bm, torch.float32, "Bm")
        lam1 = self._dev(lam1, torch.float64, "lam1")
        lam2 = self._dev(lam2, torch.float64, "lam2")
        B, k2, k1 = Cm.shape
        D = A.shape[2]
        if A.shape != (B, k1, D) or Bm.shape != (B, k2, D) or lam1.shape != (B, k1) or lam2.shape != (B, k2):
            raise ValueError("energy_grad: shapes do not agree")
        unknown = set(weights) - set(self.WEIGHT_ORDER)
        if unknown:
            raise ValueError(f"energy_grad: unknown weights {sorted(unknown)}")
        w = (C.c_double * 10)(*[float(weights.get(n, 0.0)) for n in self.WEIGHT_ORDER])
        N1 = N2 = ld1 = ld2 = 1
        if Phi1 is not None:
            Phi1 = self._dev(Phi1, torch.float32, "Phi1")
            Phi2 = self._dev(Phi2, torch.float32, "Phi2")
            a1 = self._dev(a1, torch.float32, "a1")
            _, N1, ld1 = Phi1.shape
            _, N2, ld2 = Phi2.shape
        n_ops = 0
        if ops1 is not None:
            ops1 = self._dev(ops1, torch.float64, "ops1")
            ops2 = self._dev(ops2, torch.float64, "ops2")
            n_ops = ops1.shape[1]
            if ops1.shape != (B, n_ops, k1, k1) or ops2.shape != (B, n_ops, k2, k2):
                raise ValueError("energy_grad: descriptor operators must be (B,D,k1,k1) and (B,D,k2,k2)")
        keep = (Phi1, Phi2, a1, A, Bm, lam1, lam2, ops1, ops2, w)
        args = _KeepAlive((B, N1, N2, k1, k2, D, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(a1), _ptr(A), _ptr(Bm), _ptr(lam1), _ptr(lam2),
                           _ptr(ops1), _ptr(ops2), n_ops, C.cast(w, C.c_void_p), Cm))
        args.keep = keep
        return args

    # SciPy's L-BFGS-B defaults, i.e. what the reference's `minimize(..., options={'maxiter': maxiter})` runs with (functional.py:477)
    LBFGS_REFERENCE = {"maxcor": 10, "ftol": 2.220446049250313e-09, "gtol": 1e-5, "maxfun": 15000, "maxls": 20}
    LBFGS_STATUS = {0: "running", 1: "CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL", 2: "CONVERGENCE: REL_REDUCTION_OF_F <= FACTR*EPSMCH",
                    3: "STOP: TOTAL NO. of ITERATIONS REACHED LIMIT", 4: "STOP: TOTAL NO. of f AND g EVALUATIONS EXCEEDS LIMIT",
                    5: "ABNORMAL_TERMINATION_IN_LNSRCH (or a non-finite energy / gradient)"}

    def _fit_inputs(self, batch, weights, k, orient_ops):
        """projected descriptors, spectra, operator lists and the weight dictionary dm_fmap_energy_grad takes: the orientation term is
        a commutation term like w_dcomm (base_functions.py:567-600), its operator pairs ride in the same lists scaled by
        sqrt(w_orient / w_dcomm) (w_dcomm = 1 when only w_orient is set)"""
        k1 = k if k is not None else batch["lam1"].shape[1]
        k2 = k if k is not None else batch["lam2"].shape[1]
        Phi1, Phi2 = batch["Phi1"], batch["Phi2"]
        A = self.project(Phi1, batch["a1"], batch["F1"], k1)
        Bm = self.project(Phi2, batch["a2"], batch["F2"], k2)
        lam1 = self._dev(batch["lam1"], torch.float64, "lam1")[:, :k1].contiguous()
        lam2 = self._dev(batch["lam2"], torch.float64, "lam2")[:, :k2].contiguous()
        import numpy as np
        w = {n: float(v) for n, v in weights.items() if n != "w_orient"}
        # w_orient: one weight for the batch, or (B,) -- every pair of a batched fit has its own rescaled weight (functional.py:448-456)
        w_orient = np.asarray(weights.get("w_orient", 0.0), dtype=np.float64)
        w_dcomm = float(weights.get("w_dcomm", 0.0))
        if w_orient.ndim > 1:
            raise ValueError("w_orient must be a number or (B,) weights")
        ops1 = ops2 = None
        if w_dcomm > 0:
            ops1 = self.descr_ops(Phi1, batch["a1"], batch["F1"], k1)
            ops2 = self.descr_ops(Phi2, batch["a2"], batch["F2"], k2)
        if (w_orient > 0).any():
            if orient_ops is None:
                raise ValueError("w_orient > 0 needs the orientation operators (FunctionalMapping.compute_orientation_op)")
            scale = lambda wo: (wo / w_dcomm) ** 0.5 if w_dcomm > 0 else wo ** 0.5
            o1 = self._dev(orient_ops[0], torch.float64, "orient_ops1")
            o2 = self._dev(orient_ops[1], torch.float64, "orient_ops2")
            if w_orient.ndim == 0:
                sc = scale(float(w_orient))
            else:                                       # (per pair the same float64 product as the scalar form)
                if w_orient.shape[0] != o1.shape[0]:
                    raise ValueError("w_orient: one weight per pair of the batch")
                sc = torch.tensor([scale(max(float(wo), 0.0)) for wo in w_orient], dtype=torch.float64, device=self.device).view(-1, 1, 1, 1)
            o1, o2 = o1 * sc, o2 * sc
            ops1 = o1 if ops1 is None else torch.cat([ops1, o1], dim=1).contiguous()
            ops2 = o2 if ops2 is None else torch.cat([ops2, o2], dim=1).contiguous()
            if w_dcomm <= 0:
                w["w_dcomm"] = 1.0
        P1 = self._dev(Phi1, torch.float32, "Phi1")[:, :, :k1].contiguous()
        P2 = self._dev(Phi2, torch.float32, "Phi2")[:, :, :k2].contiguous()
        a1 = self._dev(batch["a1"], torch.float32, "a1")
        return A, Bm, lam1, lam2, w, P1, P2, a1, ops1, ops2, k1, k2

    def fit_energy(self, batch, weights, x, k=None, orient_ops=None):
        """energy (B,) of the fit's objective at the maps x (B,k2,k1) -- what FunctionalMapping.fit evaluates at x0 to rescale the
        orientation weight (functional.py:448-456)"""
        A, Bm, lam1, lam2, w, P1, P2, a1, ops1, ops2, k1, k2 = self._fit_inputs(batch, weights, k, orient_ops)
        w.setdefault("w_descr", 0.0)
        e, _ = self.energy_grad(self._dev(x, torch.float64, "x"), A, Bm, lam1, lam2, w, P1, P2, a1, ops1, ops2)
        return e.cpu().numpy()

    def _weight_array(self, weights):
        return (C.c_double * 10)(*[float(weights.get(n, 0.0)) for n in self.WEIGHT_ORDER])

    def fit_fused_ok(self, k1, k2, weights, ops1=None):
        """does dm_fmap_fit_fused take this fit (maps up to 32 x 32; w_descr, w_lap, w_p2p, w_ent, w_range01, w_sumto1 only)?"""
        w = self._weight_array(weights)
        return bool(self.lib.dm_fmap_fit_fused_ok(int(k1), int(k2), C.cast(w, C.c_void_p), 0 if ops1 is None else int(ops1.shape[1])))

    def _fit_fused(self, A, Bm, lam1, lam2, weights, P1, P2, a1, x0, opts, maxiter, precision="auto"):
        """the whole fit in one library call (dm_fmap_fit_fused: one launch per evaluation, the optimiser inside the kernel).
        precision: the element loop over the N2 x N1 entries of the mapped indicator (product, entropy / range terms, back-product):
        "f32" = the reference's precision (pyFM/functional.py:379-383 moves every tensor to float32), "f64", or "auto" (default): fp32
        under SciPy's stopping rule -- what the reference runs: the same iterations, the map within 3e-6 of the float64 loop's, 1.7 x
        faster per evaluation -- and float64 when the caller asks for a tighter one (ftol < 1e-10 is below the fp32 noise floor of the
        energy: the line search then ends in ABNORMAL_TERMINATION, like SciPy's does on a noisy function).  Everything around the
        element loop (Phi2 C, partial sums, quadratic and sum-to-one terms, L-BFGS) is float64 either way."""
        import types
        import numpy as np
        if precision not in ("auto", "f32", "f64"):
            raise ValueError("precision must be 'auto', 'f32' or 'f64'")
        f32 = precision == "f32" or (precision == "auto" and float(opts["ftol"]) >= 1e-10)
        B, k1, D = A.shape
        k2 = Bm.shape[1]
        _, N1, ld1 = P1.shape
        _, N2, ld2 = P2.shape
        w = self._weight_array(dict(weights, w_dcomm=0.0))      # (reached only without operator lists: the commutativity term is off)
        x0d = self._dev(x0, torch.float64, "x0")
        xo = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        fo = torch.empty((B,), dtype=torch.float64, device=self.device)
        info = torch.empty((B, 4), dtype=torch.int32, device=self.device)
        nev = C.c_int(0)
        self._chk(self.lib.dm_fmap_fit_fused(self.ctx, B, N1, N2, k1, k2, D, _ptr(P1), ld1, _ptr(P2), ld2, _ptr(a1), _ptr(A), _ptr(Bm), _ptr(lam1),
                                             _ptr(lam2), C.cast(w, C.c_void_p), int(opts["maxcor"]), _ptr(x0d), float(opts["ftol"]), float(opts["gtol"]),
                                             int(maxiter), int(opts["maxfun"]), int(opts["maxls"]), 1 if f32 else 0, _ptr(xo), _ptr(fo), _ptr(info),
                                             C.c_void_p(0), C.byref(nev)))
        info = info.cpu().numpy()
        info[:, 0] = np.where(info[:, 0] == 0, 4, info[:, 0])
        res = types.SimpleNamespace(x=xo.cpu().numpy(), fun=fo.cpu().numpy(), status=info[:, 0].copy(), nit=info[:, 1].copy(),
                                    nfev=info[:, 2].copy(), message=[self.LBFGS_STATUS.get(int(q), "?") for q in info[:, 0]],
                                    success=bool(np.all((info[:, 0] == 1) | (info[:, 0] == 2))), evaluations=int(nev.value), path="fused",
                                    element_loop="f32" if f32 else "f64")
        return res.x, res

    def energy_grad_fused(self, Cm, A, Bm, lam1, lam2, weights, Phi1, Phi2, a1, precision="f64"):
        """energy (B,) and gradient (B,k2,k1) at the maps Cm through the arithmetic of dm_fmap_fit_fused (its single-evaluation mode):
        what the fused fit minimises, for tests and diagnostics.  precision "f64" | "f32": the element loop's (see _fit_fused)"""
        Cm = self._dev(Cm, torch.float64, "C")
        A = self._dev(A, torch.float32, "A")
        Bm = self._dev(Bm, torch.float32, "Bm")
        lam1 = self._dev(lam1, torch.float64, "lam1")
        lam2 = self._dev(lam2, torch.float64, "lam2")
        P1 = self._dev(Phi1, torch.float32, "Phi1")
        P2 = self._dev(Phi2, torch.float32, "Phi2")
        a1 = self._dev(a1, torch.float32, "a1")
        B, k2, k1 = Cm.shape
        D = A.shape[2]
        _, N1, ld1 = P1.shape
        _, N2, ld2 = P2.shape
        w = self._weight_array(dict(weights, w_dcomm=0.0))
        energy = torch.empty((B,), dtype=torch.float64, device=self.device)
        grad = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        if precision not in ("f32", "f64"):
            raise ValueError("precision must be 'f32' or 'f64'")
        self._chk(self.lib.dm_fmap_fit_fused(self.ctx, B, N1, N2, k1, k2, D, _ptr(P1), ld1, _ptr(P2), ld2, _ptr(a1), _ptr(A), _ptr(Bm), _ptr(lam1),
                                             _ptr(lam2), C.cast(w, C.c_void_p), 0, _ptr(Cm), 0.0, 0.0, 0, 0, 0, 1 if precision == "f32" else 0,
                                             C.c_void_p(0), _ptr(energy), C.c_void_p(0), _ptr(grad), None))
        return energy, grad

    def fit_general(self, batch, weights, x0, k=None, maxiter=15000, lbfgs_options=None, driver="device", check_every=4, orient_ops=None, fused=True,
                    precision="auto"):
        """FunctionalMapping.fit for any of the implemented energy terms, a whole batch at once (reference: L-BFGS-B through
        scipy.optimize.minimize, one pair per call, functional.py:477).  Every pair runs its OWN limited-memory BFGS iteration --
        history, step length, stopping test -- so a pair's result does not depend on the batch it is in; the optimiser state
        lives on the device (dm_lbfgs_*), energy and gradient of all pairs come from one dm_fmap_energy_grad call per
        evaluation, and the host reads the status words every `check_every` evaluations.
        lbfgs_options: maxcor, ftol, gtol, maxfun, maxls with SciPy's names; default = SciPy's defaults (LBFGS_REFERENCE).
        driver="scipy" (single pair only): the same evaluations driven by scipy.optimize.minimize on the host, as the reference.
        x0 (B,k2,k1): start, its first column is the pinned one.  Returns (C (B,k2,k1) numpy, result) with result.x, .fun (B),
        .status (B), .nit (B), .nfev (B), .message (list)."""
        import types
        import numpy as np
        A, Bm, lam1, lam2, weights, P1, P2, a1, ops1, ops2, k1, k2 = self._fit_inputs(batch, weights, k, orient_ops)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        B = x0.shape[0]
        opts = dict(self.LBFGS_REFERENCE)
        opts.update(lbfgs_options or {})
        if driver == "scipy":
            import scipy.optimize
            if B != 1:
                raise ValueError("driver='scipy' optimises one pair per call (the summed energy of a batch would couple the pairs)")
            cache = {}

            def fg(x):
                key = x.tobytes()
                if key not in cache:
                    cache.clear()
                    e, g = self.energy_grad(torch.from_numpy(x.reshape(B, k2, k1)), A, Bm, lam1, lam2, weights, P1, P2, a1, ops1, ops2)
                    cache[key] = (float(e.sum().item()), g.cpu().numpy().ravel())
                return cache[key]
            res = scipy.optimize.minimize(lambda x: fg(x)[0], x0.ravel(), jac=lambda x: fg(x)[1], method="L-BFGS-B",
                                          options={"maxiter": maxiter, **opts})
            return res.x.reshape(B, k2, k1), res
        n, m = k2 * k1, int(opts["maxcor"])
        if self.fit_fused_ok(k1, k2, weights, ops1) and fused:
            return self._fit_fused(A, Bm, lam1, lam2, weights, P1, P2, a1, x0, opts, maxiter, precision=precision)
        nbytes = int(self.lib.dm_lbfgs_state_bytes(B, n, m))
        state = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        xt = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        x0d = self._dev(x0, torch.float64, "x0")
        self._chk(self.lib.dm_lbfgs_init(self.ctx, B, n, m, _ptr(x0d), _ptr(state), _ptr(xt)))
        # the per-pair integer state (status first) sits behind the float64 blocks of the state buffer
        n_f64 = 3 * B * n + 2 * B * m * n + 2 * B * m + 16 * B
        ints = state[n_f64:n_f64 + (8 * B * 4 + 7) // 8].view(torch.int32)[:8 * B].view(B, 8)
        nev, maxfun = 0, int(opts["maxfun"])
        # the projected descriptors A, Bm are fixed during the fit: their Gram blocks are computed by the first evaluation only
        keep_gram = self.get_option("energy_keep_gram")
        self.set_option("energy_keep_gram", 1)
        # the evaluation loop itself runs behind the ABI, `check_every` evaluations per call (dm_fmap_fit_steps): a Python round per
        # evaluation cost more host time than the evaluation takes on the device for one small pair
        ev = self._energy_grad_args(xt, A, Bm, lam1, lam2, weights, P1, P2, a1, ops1, ops2)
        energy = torch.empty((B,), dtype=torch.float64, device=self.device)
        grad = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        try:
            while True:
                self._chk(self.lib.dm_fmap_fit_steps(self.ctx, int(check_every), *ev[:-1], m, _ptr(state), _ptr(xt), _ptr(energy), _ptr(grad),
                                                     float(opts["ftol"]), float(opts["gtol"]), int(maxiter), maxfun, int(opts["maxls"])))
                nev += int(check_every)
                if bool((ints[:, 0] != 0).all()) or nev > maxfun + 2:        # (one host synchronisation per check_every evaluations)
                    break
        finally:
            self.set_option("energy_keep_gram", keep_gram)         # (the caller's setting; setting it drops what this fit kept)
        xo = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        fo = torch.empty((B,), dtype=torch.float64, device=self.device)
        info = torch.empty((B, 4), dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_lbfgs_result(self.ctx, B, n, m, _ptr(state), _ptr(xo), _ptr(fo), _ptr(info)))
        info = info.cpu().numpy()
        info[:, 0] = np.where(info[:, 0] == 0, 4, info[:, 0])      # (the host loop ended at the evaluation limit: report it as such)
        res = types.SimpleNamespace(x=xo.cpu().numpy(), fun=fo.cpu().numpy(), status=info[:, 0].copy(), nit=info[:, 1].copy(),
                                    nfev=info[:, 2].copy(), message=[self.LBFGS_STATUS.get(int(q), "?") for q in info[:, 0]],
                                    success=bool(np.all((info[:, 0] == 1) | (info[:, 0] == 2))), evaluations=nev)
        return res.x, res

    def fm_to_p2p(self, Phi1, Phi2, a1, Cm, k1=None, k2=None, knn=True, ind=True):
        """Returns dict with knn21, knn12 (kd-tree maps of the reference) and ind21, ind12 (indicator arg-max)."""
        sfx, Phi1, Phi2, a1 = self._reals(Phi1, Phi2, a1)
        Cm = self._dev(Cm, torch.float64, "C")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        k2_, k1_ = Cm.shape[1], Cm.shape[2]
        if (k1 is not None and k1 != k1_) or (k2 is not None and k2 != k2_) or Cm.shape[0] != B:
            raise ValueError("fm_to_p2p: C must be (B,k2,k1)")
        if k1_ > ld1 or k2_ > ld2:
            raise AssertionError(f"At least {k1_}/{k2_} eigenvectors should be provided, here only {ld1}/{ld2} are given")
        mk = lambda n: torch.empty((B, n), dtype=torch.int32, device=self.device)
        out = {"knn21": mk(N2) if knn else None, "knn12": mk(N1) if knn else None,
               "ind21": mk(N2) if ind else None, "ind12": mk(N1) if ind else None}
        self._chk(getattr(self.lib, "dm_fm_to_p2p" + sfx)(self.ctx, B, N1, N2, k1_, k2_, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(a1), _ptr(Cm),
                                        _ptr(out["knn21"]), _ptr(out["knn12"]), _ptr(out["ind21"]), _ptr(out["ind12"])))
        return out

    def p2p_to_fm(self, p21, Phi1, Phi2, a2, k1, k2):
        sfx, Phi1, Phi2, a2 = self._reals(Phi1, Phi2, a2)
        p21 = self._dev(p21, torch.int32, "p21")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        if p21.shape != (B, N2):
            raise ValueError("p2p_to_fm: p21 must be (B,N2)")
        Cm = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        self._chk(getattr(self.lib, "dm_p2p_to_fm" + sfx)(self.ctx, B, N1, N2, k1, k2, _ptr(p21), _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(a2), _ptr(Cm)))
        return Cm

    def tufted_covers(self, meshes, mollify_factor=1e-5, n_threads=0):
        """The tufted intrinsic-Delaunay cover of every (verts, faces) in `meshes` (dm_tufted_cover_batch: host C++ on a thread pool,
        like the reference's robust_laplacian wheel).  Returns [(T (2 nf, 3) int32, L (2 nf, 3) f64, flips, converged, eps)]."""
        import numpy as np
        cnt = len(meshes)
        V = [np.ascontiguousarray(v, dtype=np.float64) for v, _ in meshes]
        F = [np.ascontiguousarray(f, dtype=np.int32) for _, f in meshes]
        for v, f in zip(V, F):
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
                raise ValueError("tufted_covers: meshes are (verts (n, 3), faces (m, 3)) with at least one face")
        T = [np.empty((2 * f.shape[0], 3), np.int32) for f in F]
        L = [np.empty((2 * f.shape[0], 3), np.float64) for f in F]
        info = np.zeros((cnt, 2), np.int32)
        eps = np.zeros(cnt, np.float64)
        n = np.array([v.shape[0] for v in V], np.int32)
        nf = np.array([f.shape[0] for f in F], np.int32)
        ptrs = lambda arrs: C.cast((C.c_void_p * cnt)(*[a.ctypes.data for a in arrs]), C.c_void_p)
        rc = self.lib.dm_tufted_cover_batch(cnt, n.ctypes.data, nf.ctypes.data, ptrs(V), ptrs(F), float(mollify_factor), ptrs(T), ptrs(L),
                                            info.ctypes.data, eps.ctypes.data, int(n_threads))
        if rc != 0:
            raise ValueError("tufted cover: face indices must lie in [0, n)")
        return [(T[i], L[i], int(info[i, 0]), bool(info[i, 1]), float(eps[i])) for i in range(cnt)]

    def laplacian_ell(self, tris, lens=None, verts=None, scale=1.0, want_w=True):
        """Cotangent Laplacians of a batch of meshes assembled on the device (dm_laplacian_rows + dm_laplacian_ell).
        tris: list of (nt_b, 3) int arrays; lens: list of (nt_b, 3) intrinsic side lengths, or None with verts: list of (n_b, 3)
        coordinates (the reference's cotangent_weights / dia_area_mat arithmetic); meshes of different sizes are padded to the
        largest (padding vertices become decoupled rows at the top of the spectrum).  n_verts of a mesh = len(verts[b]) or, with
        lens, max index + 1 unless `verts` gives it.
        Returns dict(cols (B,N,nnz) int32, vals (B,N,nnz) f64 [A^-1/2 W A^-1/2], mass32 (B,N), w (B,N,nnz) f64 [W] or None,
        mass64 (B,N), nnz, n_verts (list))."""
        import numpy as np
        Bn = len(tris)
        if lens is None and verts is None:
            raise ValueError("laplacian_ell: pass intrinsic lengths or vertex coordinates")
        n_verts = [int(np.asarray(v).shape[0]) for v in verts] if verts is not None else [int(np.max(t)) + 1 for t in tris]
        N, nt = max(n_verts), max(int(np.asarray(t).shape[0]) for t in tris)
        tri_h = np.full((Bn, nt, 3), -1, np.int32)
        for b, t in enumerate(tris):
            tri_h[b, :len(t)] = t
        tri_d = torch.as_tensor(tri_h).to(self.device)
        len_d = vert_d = None
        if lens is not None:
            len_h = np.ones((Bn, nt, 3), np.float64)
            for b, l in enumerate(lens):
                len_h[b, :len(l)] = l
            len_d = torch.as_tensor(len_h).to(self.device)
        else:
            vert_h = np.zeros((Bn, N, 3), np.float64)
            for b, v in enumerate(verts):
                vert_h[b, :len(v)] = v
            vert_d = torch.as_tensor(vert_h).to(self.device)
        ragged = min(n_verts) < N
        nv_d = torch.as_tensor(np.asarray(n_verts, np.int32)).to(self.device) if ragged else None
        rows = torch.empty(int(self.lib.dm_laplacian_rows_bytes(Bn, N, nt)), dtype=torch.uint8, device=self.device)
        mx = C.c_int(0)
        self._chk(self.lib.dm_laplacian_rows(self.ctx, Bn, N, nt, _ptr(tri_d), _ptr(len_d), _ptr(vert_d), float(scale), _ptr(nv_d), _ptr(rows), C.byref(mx)))
        nnz = int(mx.value)
        cols = torch.empty((Bn, N, nnz), dtype=torch.int32, device=self.device)
        vals = torch.empty((Bn, N, nnz), dtype=torch.float64, device=self.device)
        mass32 = torch.empty((Bn, N), dtype=torch.float32, device=self.device)
        w = torch.empty((Bn, N, nnz), dtype=torch.float64, device=self.device) if want_w else None
        mass64 = torch.empty((Bn, N), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_laplacian_ell(self.ctx, Bn, N, nt, _ptr(rows), nnz, _ptr(nv_d), _ptr(cols), _ptr(vals), _ptr(mass32), _ptr(w), _ptr(mass64)))
        return {"cols": cols, "vals": vals, "mass32": mass32, "w": w, "mass64": mass64, "nnz": nnz, "n_verts": n_verts}

    # ------------------------------------------------------------- DiffusionNet operators (dm_dnet_*)
    def _dnet_assemble(self, V, F, normals):
        """dm_dnet_rows + dm_dnet_ell of the meshes (V[b] (n_b, 3) float64, F[b] (m_b, 3) int32 NumPy arrays; normals: a list of
        (n_b, 3) arrays or None), padded as laplacian_ell pads.  Returns the dict of device tensors."""
        import numpy as np
        from .diffusion_net import _host
        Bn = len(V)
        n_verts = [int(v.shape[0]) for v in V]
        N, nt = max(n_verts), max(int(f.shape[0]) for f in F)
        tri_h = np.full((Bn, nt, 3), -1, np.int32)
        vert_h = np.zeros((Bn, N, 3), np.float64)
        nrm_h = np.zeros((Bn, N, 3), np.float64) if normals is not None else None
        for b in range(Bn):
            tri_h[b, :len(F[b])] = F[b]
            vert_h[b, :n_verts[b]] = V[b]
            if nrm_h is not None:
                nrm_h[b, :n_verts[b]] = normals[b]
        # (through _dev: it refuses a call under another stream than the engine's, where the allocator could recycle the scratch below
        #  while the context's stream still uses it)
        tri_d = self._dev(tri_h, torch.int32, "tri")
        vert_d = self._dev(vert_h, torch.float64, "verts")
        nrm_d = self._dev(nrm_h, torch.float64, "normals") if nrm_h is not None else None
        nv_d = self._dev(np.asarray(n_verts, np.int32), torch.int32, "n_verts") if min(n_verts) < N else None
        rows = torch.empty(int(self.lib.dm_dnet_rows_bytes(Bn, N, nt)), dtype=torch.uint8, device=self.device)
        frames = torch.empty((Bn, N, 3, 3), dtype=torch.float64, device=self.device)
        info = torch.empty((Bn,), dtype=torch.int32, device=self.device)
        mx = C.c_int(0)
        self._chk(self.lib.dm_dnet_rows(self.ctx, Bn, N, nt, _ptr(tri_d), _ptr(vert_d), _ptr(nrm_d), _ptr(nv_d), _host.DENOM_EPS, _host.GRAD_EPS,
                                        _ptr(rows), _ptr(frames), _ptr(info), C.byref(mx)))
        nnz = int(mx.value)
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
        out = {"frames": frames, "info": info, "nnz": nnz, "n_verts": n_verts,
               "row_len": torch.empty((Bn, N), dtype=torch.int32, device=self.device),
               "cols": torch.empty((Bn, N, nnz), dtype=torch.int32, device=self.device),
               "l": f64(Bn, N, nnz), "vals": f64(Bn, N, nnz), "gx": f64(Bn, N, nnz), "gy": f64(Bn, N, nnz), "mass64": f64(Bn, N),
               "mass32": torch.empty((Bn, N), dtype=torch.float32, device=self.device)}
        self._chk(self.lib.dm_dnet_ell(self.ctx, Bn, N, nt, _ptr(rows), nnz, _ptr(nv_d), _host.MASS_EPS, _host.MASS_EPS, _ptr(out["row_len"]),
                                       _ptr(out["cols"]), _ptr(out["l"]), _ptr(out["vals"]), _ptr(out["gx"]), _ptr(out["gy"]), _ptr(out["mass64"]),
                                       _ptr(out["mass32"])))
        return out

    def diffusion_operators(self, verts_list, faces_list, k_eig, normals=None):
        """What diffusion_net.geometry.compute_operators precomputes (reference diffusion_net/geometry.py:275-391), for a batch of
        meshes in one device call: dm_dnet_rows / dm_dnet_ell, then eigenbasis(ell=...) on M'^-1/2 (L + 1e-8 I) M'^-1/2.
        verts_list / faces_list: (n_b, 3) / (m_b, 3) arrays; normals: None or a list with an (n_b, 3) array or None per mesh.
        A mesh for which the device reports an undefined normal (bit 1 of info) gets its normals from the host -- the reference's
        repair sequence, literally -- and runs again with them.
        Returns a list with, per mesh, the dict frames (n,3,3), mass (n), row_len (n) int32, cols (n,nnz) int32, l / gx / gy (n,nnz),
        evals (k), evecs (n,k): float64 tensors on the device, padding rows cut off, entries q < row_len[i] of row i real; and
        info: the first pass's info word of the mesh."""
        import numpy as np
        from .diffusion_net import _host
        Bn = len(verts_list)
        if Bn == 0:
            return []
        V = [np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64) for v in verts_list]
        F = [np.ascontiguousarray(f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else f) for f in faces_list]
        for b in range(Bn):
            if V[b].ndim != 2 or V[b].shape[1] != 3 or V[b].shape[0] == 0:
                raise ValueError(f"diffusion_operators: mesh {b}: vertices must be (n, 3)")
            if F[b].size == 0:
                raise NotImplementedError("diffusion_operators: point clouds (no faces) are not built")
            if F[b].ndim != 2 or F[b].shape[1] != 3 or F[b].min() < 0 or F[b].max() >= V[b].shape[0]:
                raise ValueError(f"diffusion_operators: mesh {b}: faces must be (m, 3) indices into the {V[b].shape[0]} vertices")
            F[b] = F[b].astype(np.int32)
        given = [None] * Bn if normals is None else [None if g is None else np.asarray(g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else g, np.float64)
                                                      for g in normals]
        have, lack = [b for b in range(Bn) if given[b] is not None], [b for b in range(Bn) if given[b] is None]
        parts, first_info = [None] * Bn, [0] * Bn

        def run(idx, nrm):
            out = self._dnet_assemble([V[b] for b in idx], [F[b] for b in idx], nrm)
            info = out["info"].cpu().numpy()
            for q, b in enumerate(idx):
                parts[b] = (out, q)
                if nrm is None:
                    first_info[b] = int(info[q])
            return info

        if lack:
            info = run(lack, None)
            redo = [b for q, b in enumerate(lack) if info[q] & 1]
            for b in redo:
                given[b] = _host.vertex_normals(V[b], F[b].astype(np.int64))
            have = sorted(have + redo)
        if have:
            run(have, [given[b] for b in have])
        res = [None] * Bn
        groups = {}
        for b in range(Bn):
            groups.setdefault(id(parts[b][0]), []).append(b)
        # eigenbasis() chooses between the filtered iteration and the dense route from the SMALLEST mesh of its batch (and the dense
        # route takes at most 2048 padded vertices): meshes are solved with the partners that take the same route as they would alone,
        # each group cut to its own largest mesh, so a small mesh neither drags a large one to the dense route nor changes its own
        guard = next((g for g in range(12, 33) if (int(k_eig) + g) % 32 == 0), 32)
        by_route = {}
        for key, idx in groups.items():
            for b in idx:
                by_route.setdefault((key, 2 * (int(k_eig) + guard) > V[b].shape[0]), []).append(b)
        for idx in by_route.values() if k_eig > 0 else groups.values():
            out = parts[idx[0]][0]
            if k_eig > 0:
                sel = torch.as_tensor([parts[b][1] for b in idx], device=self.device)
                Ng = max(V[b].shape[0] for b in idx)
                cut = lambda t: t[sel, :Ng].contiguous()
                out = {key: cut(out[key]) for key in ("frames", "mass64", "row_len", "cols", "l", "gx", "gy", "vals", "mass32")}
                out["nnz"], out["n_verts"] = parts[idx[0]][0]["nnz"], [V[b].shape[0] for b in idx]
                for q, b in enumerate(idx):
                    parts[b] = (out, q)
                ell = {"cols": out["cols"], "vals": out["vals"], "mass32": out["mass32"], "nnz": out["nnz"], "n_verts": out["n_verts"]}
                lam, Phi, _, _ = self.eigenbasis(None, None, int(k_eig), guard=guard, ell=ell)
                # dm_eigenbasis solves the problem of the fp32-rounded masses M' (Phi^T M' Phi = I).  The operators carry the float64
                # masses M: Phi <- Phi (Phi^T M Phi)^-1/2, the symmetric orthonormalisation, with G = I + E, |E| ~ 1e-8:
                # G^-1/2 = I - E/2 + 3/8 E^2 to 1e-24.  The eigenvalues move by E's second order; they stay as returned.
                G = torch.matmul(Phi.transpose(1, 2), out["mass64"].unsqueeze(-1) * Phi)
                E = G - torch.eye(G.shape[-1], dtype=G.dtype, device=G.device)
                Phi = Phi - torch.matmul(Phi, 0.5 * E - 0.375 * torch.matmul(E, E))
                lam = torch.clamp(lam, min=0.0)
            for b in idx:
                q, n = parts[b][1], V[b].shape[0]
                res[b] = {"frames": out["frames"][q, :n], "mass": out["mass64"][q, :n], "row_len": out["row_len"][q, :n], "cols": out["cols"][q, :n],
                          "l": out["l"][q, :n], "gx": out["gx"][q, :n], "gy": out["gy"][q, :n], "info": first_info[b],
                          "evals": lam[q] if k_eig > 0 else torch.zeros((0,), dtype=torch.float64, device=self.device),
                          "evecs": Phi[q, :n] if k_eig > 0 else torch.zeros((n, 0), dtype=torch.float64, device=self.device)}
        return res

    # ------------------------------------------------------------- DiffusionNet forward (dm_dnet_*_f32)
    def _dnet_mat(self, t, name):
        """(tensor, ld) of an fp32 matrix operand, (B, N, W) or (R, W).  It is passed as it lies in memory when its elements of a row are
        adjacent and its rows evenly spaced (row stride ld >= W, batch stride N ld) -- a parameter, a column slice of a wider buffer,
        a padded view --, and copied otherwise."""
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float32:
            t = self._dev(t, torch.float32, name)
        elif torch.cuda.current_stream(self.device).cuda_stream != self.stream.cuda_stream:
            raise RuntimeError("MatchEngine is bound to the stream it was created on; create one engine per stream")
        if t.dim() == 2:
            R, W = t.shape
            ld = t.stride(0) if R > 1 else max(W, 1)
            if (W == 1 or t.stride(1) == 1) and ld >= W:
                return t, int(ld)
            return t.contiguous(), int(W)
        if t.dim() != 3:
            raise ValueError(f"{name}: expected a (B, N, W) or (N, W) tensor, got {tuple(t.shape)}")
        Bn, N, W = t.shape
        ld = t.stride(1) if N > 1 else (t.stride(0) if Bn > 1 else W)
        if (W == 1 or t.stride(2) == 1) and ld >= W and (Bn == 1 or t.stride(0) == N * ld):
            return t, int(ld)
        return t.contiguous(), int(W)

    def _dnet_counts(self, n_verts, Bn):
        if n_verts is None:
            return None
        nv = self._dev(n_verts, torch.int32, "n_verts")
        if nv.shape != (Bn,):
            raise ValueError(f"n_verts: expected {Bn} counts, got {tuple(nv.shape)}")
        return nv

    def _dnet_out(self, out, Bn, N, C, name):
        if out is None:
            return torch.empty((Bn, N, C), dtype=torch.float32, device=self.device), C
        if out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != (Bn, N, C):
            raise ValueError(f"{name}: out must be a float32 ({Bn}, {N}, {C}) tensor on {self.device}")
        o, ld = self._dnet_mat(out, name)
        if o is not out:
            raise ValueError(f"{name}: out must have adjacent elements in a row and evenly spaced rows")
        return out, ld

    def dnet_linear(self, srcs, weight, bias=None, resid=None, relu=False, n_verts=None, out=None):
        """out[b,i,:] = act(concat(srcs)[b,i,:] weight^T + bias) + resid[b,i,:] (dm_dnet_linear_f32): srcs one tensor or up to three
        (B, N, w_s) (or all (N, w_s)), weight (C_out, sum w_s) as nn.Linear stores it; the concatenation is never formed.  n_verts
        (B) int32: rows behind a mesh's count are not read and come out as zeros."""
        srcs = [srcs] if isinstance(srcs, torch.Tensor) else list(srcs)
        if not 1 <= len(srcs) <= 3:
            raise ValueError("dnet_linear: one to three sources")
        flat = srcs[0].dim() == 2
        if flat:
            srcs = [s.unsqueeze(0) for s in srcs]
            resid = None if resid is None else resid.unsqueeze(0)
        mats = [self._dnet_mat(s, "src") for s in srcs]
        Bn, N = mats[0][0].shape[:2]
        if any(m.shape[:2] != (Bn, N) for m, _ in mats):
            raise ValueError("dnet_linear: the sources differ in their leading dimensions")
        W, ldw = self._dnet_mat(weight, "weight")
        if W.dim() != 2 or W.shape[1] != sum(m.shape[2] for m, _ in mats):
            raise ValueError(f"dnet_linear: weight {tuple(W.shape)} does not match the summed source widths {sum(m.shape[2] for m, _ in mats)}")
        C_out = W.shape[0]
        bias = None if bias is None else self._dev(bias, torch.float32, "bias")
        if bias is not None and bias.shape != (C_out,):
            raise ValueError("dnet_linear: bias must be (C_out,)")
        R, ldr = (None, 0) if resid is None else self._dnet_mat(resid, "resid")
        if R is not None and tuple(R.shape) != (Bn, N, C_out):
            raise ValueError("dnet_linear: resid must have the shape of the output")
        nv = self._dnet_counts(n_verts, Bn)
        out, ldo = self._dnet_out(out, Bn, N, C_out, "dnet_linear")
        a = [(m, m.shape[2], ld) for m, ld in mats] + [(None, 0, 0)] * (3 - len(mats))
        self._chk(self.lib.dm_dnet_linear_f32(self.ctx, Bn, N, C_out, len(mats), _ptr(a[0][0]), a[0][1], a[0][2], _ptr(a[1][0]), a[1][1], a[1][2],
                                              _ptr(a[2][0]), a[2][1], a[2][2], _ptr(W), ldw, _ptr(bias), _ptr(R), ldr, 1 if relu else 0, _ptr(nv),
                                              _ptr(out), ldo))
        return out[0] if flat else out

    def dnet_diffuse(self, x, mass, evals, evecs, times, n_verts=None, out=None):
        """evecs (exp(-evals max(times, 1e-8)) * (evecs^T (mass * x))) (dm_dnet_diffuse_f32): x (B,N,C), mass (B,N), evals (B,K),
        evecs (B,N,K), times (C); the spectrum stays on chip."""
        X, ldx = self._dnet_mat(x, "x")
        E, lde = self._dnet_mat(evecs, "evecs")
        Bn, N, Cw = X.shape
        K = E.shape[2]
        mass = self._dev(mass, torch.float32, "mass")
        evals = self._dev(evals, torch.float32, "evals")
        times = self._dev(times, torch.float32, "times")
        if tuple(E.shape[:2]) != (Bn, N) or tuple(mass.shape) != (Bn, N) or tuple(evals.shape) != (Bn, K) or tuple(times.shape) != (Cw,):
            raise ValueError("dnet_diffuse: x (B,N,C), mass (B,N), evals (B,K), evecs (B,N,K), times (C)")
        nv = self._dnet_counts(n_verts, Bn)
        out, ldo = self._dnet_out(out, Bn, N, Cw, "dnet_diffuse")
        self._chk(self.lib.dm_dnet_diffuse_f32(self.ctx, Bn, N, K, Cw, _ptr(X), ldx, _ptr(mass), _ptr(evals), _ptr(E), lde, _ptr(times), _ptr(nv),
                                               _ptr(out), ldo))
        return out

    def dnet_gradient_features(self, x, row_len, cols, gx, gy, A_re, A_im=None, n_verts=None, out=None):
        """tanh(gX * B_re + gY * B_im) of SpatialGradientFeatures (dm_dnet_gradfeat_f32) from the ELL rows of the gradient operators
        (row_len (B,N) int32; cols int32, gx, gy float32 (B,N,nnz)) and x (B,N,C); A_im None: one matrix, no rotation."""
        X, ldx = self._dnet_mat(x, "x")
        Bn, N, Cw = X.shape
        row_len = self._dev(row_len, torch.int32, "row_len")
        cols = self._dev(cols, torch.int32, "cols")
        gx = self._dev(gx, torch.float32, "gx")
        gy = self._dev(gy, torch.float32, "gy")
        if cols.dim() != 3 or tuple(cols.shape[:2]) != (Bn, N) or gx.shape != cols.shape or gy.shape != cols.shape or tuple(row_len.shape) != (Bn, N):
            raise ValueError("dnet_gradient_features: row_len (B,N), cols / gx / gy (B,N,nnz)")
        Are, lda = self._dnet_mat(A_re, "A_re")
        Aim = None
        if A_im is not None:
            Aim, lda2 = self._dnet_mat(A_im, "A_im")
            if lda2 != lda:
                Are, Aim, lda = Are.contiguous(), Aim.contiguous(), Cw
        if tuple(Are.shape) != (Cw, Cw) or (Aim is not None and tuple(Aim.shape) != (Cw, Cw)):
            raise ValueError("dnet_gradient_features: A_re / A_im must be (C, C)")
        nv = self._dnet_counts(n_verts, Bn)
        out, ldo = self._dnet_out(out, Bn, N, Cw, "dnet_gradient_features")
        self._chk(self.lib.dm_dnet_gradfeat_f32(self.ctx, Bn, N, Cw, cols.shape[2], _ptr(row_len), _ptr(cols), _ptr(gx), _ptr(gy), _ptr(X), ldx,
                                                _ptr(Are), _ptr(Aim), lda, _ptr(nv), _ptr(out), ldo))
        return out

    def diffusion_net_forward(self, weights, packed, x):
        """A whole DiffusionNet (inference) on a padded batch: first_lin, per block diffuse -> gradient features -> the MLP (its first
        layer reads (x, x_diffuse, x_grad) as three sources, its last adds the skip), last_lin.
        weights  {"first": (W, b), "last": (W, b), "blocks": [{"times": t, "A_re": A or None, "A_im": A or None, "mlp": [(W, b), ...]}]},
                 the module's parameters as they lie in memory (A_re None: no gradient features)
        packed   fp32 padded operators with the attributes mass (B,N), evals (B,K), evecs (B,N,K), row_len, cols, gx, gy, n_verts_dev
                 ((B) int32 or None when no mesh is padded) -- diffusion_net.layers.PackedOperators
        x        (B, N, C_in), or up to three tensors read as concatenated along the channels.
        Returns (B, N, C_out); rows behind a mesh's count are zero.  Intermediates live in buffers that the blocks share."""
        nv = packed.n_verts_dev
        W0, b0 = weights["first"]
        cur = self.dnet_linear(x, W0, b0, n_verts=nv)
        Bn, N, Cw = cur.shape
        buf = lambda c=Cw: torch.empty((Bn, N, c), dtype=torch.float32, device=self.device)
        nxt, xd, xg, hidden = buf(), buf(), None, {}
        for blk in weights["blocks"]:
            self.dnet_diffuse(cur, packed.mass, packed.evals, packed.evecs, blk["times"], n_verts=nv, out=xd)
            src = [cur, xd]
            if blk.get("A_re") is not None:
                xg = buf() if xg is None else xg
                self.dnet_gradient_features(xd, packed.row_len, packed.cols, packed.gx, packed.gy, blk["A_re"], blk.get("A_im"), n_verts=nv, out=xg)
                src.append(xg)
            mlp = blk["mlp"]
            for i, (W, b) in enumerate(mlp):
                if i + 1 == len(mlp):
                    self.dnet_linear(src, W, b, resid=cur, n_verts=nv, out=nxt)
                else:
                    key = (i % 2, W.shape[0])
                    if key not in hidden:
                        hidden[key] = buf(W.shape[0])
                    src = [self.dnet_linear(src, W, b, relu=True, n_verts=nv, out=hidden[key])]
            cur, nxt = nxt, cur
        W1, b1 = weights["last"]
        return self.dnet_linear(cur, W1, b1, n_verts=nv)

    # ------------------------------------------------------------- heat-method geodesics (dm_heat_geodesic_*)
    _GEOD_INFO = ((1, "A + tW is not positive definite"),
                  (2, "the grounded stiffness matrix W is not positive definite (more than one connected component?)"),
                  (4, "the mesh has a face of zero area"),
                  (8, "a face index or a column of W lies outside the mesh's vertices"),
                  (16, "a vertex that no face references"))

    def _stiffness_rows(self, W, n, who, b):
        """the stiffness matrix of mesh b (n vertices) as ELL rows (cols (n, nnz) int32, w (n, nnz) float64) on the device: a SciPy
        sparse matrix is converted row by row in CSR order and padded with col = -1, val = 0; (cols, w) device rows (those of
        laplacian_ell) pass through"""
        import numpy as np
        import scipy.sparse as sp
        if sp.issparse(W):
            Wc = sp.csr_matrix(W)
            if Wc.shape != (n, n):
                raise ValueError(f"{who}: mesh {b}: W is {Wc.shape}, expected {(n, n)}")
            rl = np.diff(Wc.indptr)
            w = max(1, int(rl.max()))
            cols_h = np.full((n, w), -1, np.int32)
            vals_h = np.zeros((n, w), np.float64)
            pos = np.arange(Wc.nnz) - np.repeat(Wc.indptr[:-1], rl)
            r = np.repeat(np.arange(n), rl)
            cols_h[r, pos] = Wc.indices
            vals_h[r, pos] = Wc.data
            return torch.as_tensor(cols_h).to(self.device), torch.as_tensor(vals_h).to(self.device)
        cols_d, w_d = W
        if cols_d.shape[0] != n or w_d.shape != cols_d.shape:
            raise ValueError(f"{who}: mesh {b}: device rows of shape {tuple(cols_d.shape)} for {n} vertices")
        return cols_d, w_d

    def heat_geodesic_factor(self, meshes, t):
        """Factor the two systems of the heat method (pyFM geometry.heat_geodmat: A + tW and W, geometry.py:716-718) for a batch
        of meshes, on the device (dm_heat_geodesic_factor: dense float64 Cholesky, W grounded at vertex 0).
        meshes: list of (verts (n,3), faces (m,3), W, mass (n,)) with W the stiffness matrix as a SciPy sparse matrix or as the
        (cols, w) device rows (n, nnz) of laplacian_ell; t: the heat time, one float or one per mesh.  Fails closed (ValueError)
        on a mesh of more than one connected component (vertices that no face references included), masses that are not one
        third of the adjacent face areas (heat_geodesic_check), a face of zero area or a system that is not positive definite.  Returns the factors (a dict holding the device buffer) for heat_geodesic."""
        import numpy as np
        Bn = len(meshes)
        if Bn == 0:
            raise ValueError("heat_geodesic_factor: no meshes")
        ts = np.broadcast_to(np.asarray(t, np.float64), (Bn,)).copy()
        n_verts, rows = [], []
        for b, (V, F, W, mass) in enumerate(meshes):
            heat_geodesic_check(V, F, mass, b)
            n = len(V)
            rows.append(self._stiffness_rows(W, n, "heat_geodesic_factor", b))
            n_verts.append(n)
        N = max(n_verts)
        nt = max(len(m[1]) for m in meshes)
        nnz = max(int(c.shape[1]) for c, _ in rows)
        tri_h = np.full((Bn, nt, 3), -1, np.int32)
        vert_h = np.zeros((Bn, N, 3), np.float64)
        mass_h = np.zeros((Bn, N), np.float64)
        for b, (V, F, _, mass) in enumerate(meshes):
            tri_h[b, :len(F)] = F
            vert_h[b, :len(V)] = V
            mass_h[b, :len(V)] = np.asarray(mass, np.float64).ravel()
        cols = torch.full((Bn, N, nnz), -1, dtype=torch.int32, device=self.device)
        wv = torch.zeros((Bn, N, nnz), dtype=torch.float64, device=self.device)
        for b, (c, w) in enumerate(rows):
            cols[b, :c.shape[0], :c.shape[1]] = c.to(self.device, torch.int32)
            wv[b, :w.shape[0], :w.shape[1]] = w.to(self.device, torch.float64)
        tri_d, vert_d, mass_d = (torch.as_tensor(x).to(self.device) for x in (tri_h, vert_h, mass_h))
        t_d = torch.as_tensor(ts).to(self.device)
        nv_d = torch.as_tensor(np.asarray(n_verts, np.int32)).to(self.device)
        nbytes = int(self.lib.dm_heat_geodesic_bytes(Bn, N, nt))
        if nbytes == 0:
            raise ValueError(f"heat_geodesic_factor: meshes of up to 16384 vertices (got {N})")
        buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_heat_geodesic_factor(self.ctx, Bn, N, nt, _ptr(tri_d), _ptr(vert_d), _ptr(cols), _ptr(wv), nnz, _ptr(mass_d),
                                                   _ptr(t_d), _ptr(nv_d), _ptr(buf), _ptr(info)))
        info_h = info.cpu().numpy()
        for b in np.flatnonzero(info_h):
            why = "; ".join(msg for bit, msg in self._GEOD_INFO if info_h[b] & bit)
            raise ValueError(f"heat_geodesic_factor: mesh {b}: {why}")
        return {"buf": buf, "B": Bn, "N": N, "nt": nt, "n_verts": n_verts, "t": ts}

    def heat_geodesic(self, factors, sources=None, sym=False):
        """Heat-method geodesic distances from the factors of heat_geodesic_factor (dm_heat_geodesic_solve): the reference's
        heat_geodesic_from / heat_geodmat (geometry.py:587-740) for robust=False.
        sources: None = all pairs; a 1-D list of vertex indices shared by every mesh; or one list per mesh (the same length, -1 = none).
        Returns a device tensor D (B, N, ns) float64 with D[b, :, s] = the distances FROM sources[s] (a column of the reference's
        matrix; rows past a mesh's vertex count are 0).  sym=True (all pairs only): (D + D^T) / 2 as the reference forms it
        (trimesh.py:677-679).  A column's bits do not depend on the other sources or meshes of the call."""
        import numpy as np
        Bn, N = factors["B"], factors["N"]
        nv = factors["n_verts"]
        if sources is None:
            src = np.full((Bn, N), -1, np.int32)
            for b, n in enumerate(nv):
                src[b, :n] = np.arange(n)
        else:
            if sym:
                raise ValueError("heat_geodesic: sym=True needs all pairs (sources=None)")
            src = np.asarray(sources)
            src = np.broadcast_to(src, (Bn, src.shape[-1])) if src.ndim == 1 else src
            if src.ndim != 2 or src.shape[0] != Bn or src.shape[1] == 0:
                raise ValueError(f"heat_geodesic: sources must be (ns,) or ({Bn}, ns)")
            for b, n in enumerate(nv):
                if src[b].min() < -1 or src[b].max() >= n:
                    raise ValueError(f"heat_geodesic: mesh {b}: source indices must lie in [0, {n})")
            src = np.ascontiguousarray(src, np.int32)
        ns = src.shape[1]
        src_d = torch.as_tensor(src).to(self.device)
        rows = torch.empty((Bn, ns, N), dtype=torch.float64, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_heat_geodesic_solve(self.ctx, Bn, N, factors["nt"], _ptr(factors["buf"]), ns, _ptr(src_d), _ptr(rows),
                                                  _ptr(info)))
        bad = np.flatnonzero(info.cpu().numpy())
        if len(bad):
            raise ValueError(f"heat_geodesic: mesh {int(bad[0])}: a source lies outside [-1, n_verts)")
        D = rows.transpose(1, 2)
        if sym:
            D = D * 0.5
            D = D + D.transpose(1, 2)
        return D.contiguous()

    # ------------------------------------------------------------- farthest-point sampling (dm_fps_*)
    def fps(self, verts, size, start, n_verts=None):
        """Farthest-point sampling on Euclidean distances (geometry.py:839-848 with the distance of trimesh.py:872-873), the
        reference's indices.  verts (B,N,3) or (N,3) float64; start: one index or (B,); n_verts (B,) for padded batches.
        Returns (B,size) int32 on the device."""
        import numpy as np
        verts = self._dev(verts, torch.float64, "verts")
        if verts.dim() == 2:
            verts = verts[None]
        if verts.dim() != 3 or verts.shape[2] != 3:
            raise ValueError("fps: verts must be (B,N,3)")
        Bn, N = int(verts.shape[0]), int(verts.shape[1])
        if N > 16384:
            raise ValueError(f"fps: meshes of up to 16384 vertices (got {N})")
        st = np.broadcast_to(np.asarray(start, np.int64), (Bn,))
        nv = np.full((Bn,), N, np.int64) if n_verts is None else np.broadcast_to(np.asarray(n_verts, np.int64), (Bn,))
        if nv.min() < 1 or nv.max() > N or st.min() < 0 or np.any(st >= nv):
            raise ValueError("fps: start indices must lie in [0, n_verts), n_verts in [1, N]")
        st_d = torch.as_tensor(np.ascontiguousarray(st, np.int32)).to(self.device)
        nv_d = torch.as_tensor(np.ascontiguousarray(nv, np.int32)).to(self.device)
        out = torch.empty((Bn, int(size)), dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_fps_euclid(self.ctx, Bn, N, _ptr(verts), _ptr(nv_d), int(size), _ptr(st_d), _ptr(out)))
        return out

    def fps_heat(self, factors, size, start):
        """Farthest-point sampling on the heat-method distances of heat_geodesic_factor's factors: d(i) = geod_from(i, robust=False).
        start: one index or one per mesh.  Returns (B,size) int32 on the device.  The whole sampling is one call without host
        synchronisation ("fps_heat_route": all-pairs rows + one sampling launch, or one single-source solve per sample)."""
        import numpy as np
        Bn, N = factors["B"], factors["N"]
        st = np.broadcast_to(np.asarray(start, np.int64), (Bn,))
        for b, n in enumerate(factors["n_verts"]):
            if st[b] < 0 or st[b] >= n:
                raise ValueError(f"fps_heat: mesh {b}: the start vertex must lie in [0, {n})")
        st_d = torch.as_tensor(np.ascontiguousarray(st, np.int32)).to(self.device)
        out = torch.empty((Bn, int(size)), dtype=torch.int32, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_fps_heat(self.ctx, Bn, N, factors["nt"], _ptr(factors["buf"]), int(size), _ptr(st_d), _ptr(out), _ptr(info)))
        info_h = info.cpu().numpy()
        for b in np.flatnonzero(info_h):
            raise ValueError(f"fps_heat: mesh {int(b)}: " + ("a start vertex outside the mesh" if info_h[b] & 1 else "a distance that is not finite"))
        return out

    # ------------------------------------------------------------- shortest paths along mesh edges (dm_graph_geodesic / dm_fps_graph)
    GRAPH_MAX_DEGREE = 64
    _GRAPH_INFO = ((1, "a source or start vertex outside the mesh"),
                   (2, "an edge weight that is negative or NaN (shortest paths by relaxation need weights >= 0)"),
                   (4, "a column outside the mesh's vertices"))

    def _graph_ell(self, graphs, who):
        """the ELL operands of dm_graph_geodesic / dm_fps_graph for a list of SciPy sparse matrices: G[i, j] stored = an edge i -> j
        of that weight (explicit zeros included, as csgraph reads a sparse matrix).  Vertex-minor layout (B, nnz, N), vertex v's
        entries = the edges INTO v, meshes padded to the largest, the width = the largest in-degree of the batch.  A degree above
        GRAPH_MAX_DEGREE = 64 raises GraphTooWide (a ValueError): every vertex of every mesh walks the padded width in every sweep, so
        one hub vertex would set the cost of the whole batch; mesh edge graphs stay far below (valence 6 on average)."""
        import numpy as np
        import scipy.sparse as sp
        Bn = len(graphs)
        if Bn == 0:
            raise ValueError(f"{who}: no graphs")
        ins, n_verts = [], []
        for b, G in enumerate(graphs):
            if not sp.issparse(G) or G.shape[0] != G.shape[1] or G.shape[0] < 1:
                raise ValueError(f"{who}: mesh {b}: a square SciPy sparse matrix is expected")
            Gi = sp.csc_matrix(G)                                                # column v = the edges into v (no entry is dropped or summed)
            ins.append(Gi)
            n_verts.append(Gi.shape[0])
        N = max(n_verts)
        if N > 16384:
            raise GraphTooWide(f"{who}: meshes of up to 16384 vertices (got {N})")
        nnz = max(1, max(int(np.diff(Gi.indptr).max()) for Gi in ins))
        if nnz > self.GRAPH_MAX_DEGREE:
            raise GraphTooWide(f"{who}: a vertex of degree {nnz}: the device route takes degrees up to {self.GRAPH_MAX_DEGREE}")
        cols_h = np.full((Bn, nnz, N), -1, np.int32)
        w_h = np.zeros((Bn, nnz, N), np.float64)
        for b, Gi in enumerate(ins):
            rl = np.diff(Gi.indptr)
            pos = np.arange(Gi.nnz) - np.repeat(Gi.indptr[:-1], rl)
            v = np.repeat(np.arange(Gi.shape[0]), rl)
            cols_h[b, pos, v] = Gi.indices
            w_h[b, pos, v] = Gi.data
        nv_d = torch.as_tensor(np.asarray(n_verts, np.int32)).to(self.device)
        return {"B": Bn, "N": N, "nnz": nnz, "n_verts": n_verts, "nv_d": nv_d,
                "cols": torch.as_tensor(cols_h).to(self.device), "w": torch.as_tensor(w_h).to(self.device)}

    def _graph_info(self, info, who):
        import numpy as np
        info_h = info.cpu().numpy()
        for b in np.flatnonzero(info_h):
            raise ValueError(f"{who}: mesh {int(b)}: " + "; ".join(msg for bit, msg in self._GRAPH_INFO if info_h[b] & bit))

    def graph_geodesic(self, graphs, sources=None):
        """Shortest-path distances on weighted graphs (dm_graph_geodesic): scipy.sparse.csgraph.dijkstra(G, indices=sources) BIT FOR
        BIT, the reference's geodesic_distmat_dijkstra (geometry.py:524-556) when G is the edge graph of a mesh.
        graphs: list of square SciPy sparse matrices, G[i, j] stored = an edge i -> j (store both directions of an undirected edge;
        explicit zeros are edges), weights >= 0 (negative or NaN: ValueError); up to 16384 vertices, degrees up to GRAPH_MAX_DEGREE
        (GraphTooWide, a ValueError, beyond either).
        sources: None = all pairs; a 1-D list of vertex indices shared by every mesh; or one list per mesh (the same length, -1 = none).
        Returns a device tensor D (B, ns, N) float64 with D[b, s] = the distances FROM sources[s] (row s of csgraph.dijkstra's
        matrix; +inf where no path leads; columns past a mesh's vertex count and rows without a source are 0).  A row's bits do not
        depend on the other sources or meshes of the call."""
        import numpy as np
        ell = self._graph_ell(graphs, "graph_geodesic")
        Bn, N, nv = ell["B"], ell["N"], ell["n_verts"]
        if sources is None:
            src = np.full((Bn, N), -1, np.int32)
            for b, n in enumerate(nv):
                src[b, :n] = np.arange(n)
        else:
            src = np.asarray(sources)
            src = np.broadcast_to(src, (Bn, src.shape[-1])) if src.ndim == 1 else src
            if src.ndim != 2 or src.shape[0] != Bn or src.shape[1] == 0:
                raise ValueError(f"graph_geodesic: sources must be (ns,) or ({Bn}, ns)")
            for b, n in enumerate(nv):
                if src[b].min() < -1 or src[b].max() >= n:
                    raise ValueError(f"graph_geodesic: mesh {b}: source indices must lie in [0, {n})")
            src = np.ascontiguousarray(src, np.int32)
        ns = src.shape[1]
        src_d = torch.as_tensor(src).to(self.device)
        D = torch.empty((Bn, ns, N), dtype=torch.float64, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_graph_geodesic(self.ctx, Bn, N, ell["nnz"], _ptr(ell["cols"]), _ptr(ell["w"]), _ptr(ell["nv_d"]), ns,
                                             _ptr(src_d), _ptr(D), _ptr(info)))
        self._graph_info(info, "graph_geodesic")
        return D

    def fps_graph(self, graphs, size, start):
        """Farthest-point sampling on the shortest-path distances of graph_geodesic (dm_fps_graph): the loop of geometry.py:839-848 with
        d(i) = csgraph.dijkstra(G, indices=i), the same indices (+inf is a maximum, the lowest index among equal maxima).
        graphs as for graph_geodesic; start: one index or one per mesh.  Returns (B,size) int32 on the device.  The whole sampling
        of the batch is ONE launch without host synchronisation."""
        import numpy as np
        ell = self._graph_ell(graphs, "fps_graph")
        Bn = ell["B"]
        if int(size) < 1:
            raise ValueError("fps_graph: size must be positive")
        st = np.broadcast_to(np.asarray(start, np.int64), (Bn,))
        for b, n in enumerate(ell["n_verts"]):
            if st[b] < 0 or st[b] >= n:
                raise ValueError(f"fps_graph: mesh {b}: the start vertex must lie in [0, {n})")
        st_d = torch.as_tensor(np.ascontiguousarray(st, np.int32)).to(self.device)
        out = torch.empty((Bn, int(size)), dtype=torch.int32, device=self.device)
        info = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_fps_graph(self.ctx, Bn, ell["N"], ell["nnz"], _ptr(ell["cols"]), _ptr(ell["w"]), _ptr(ell["nv_d"]), int(size),
                                        _ptr(st_d), _ptr(out), _ptr(info)))
        self._graph_info(info, "fps_graph")
        return out

    def eigenbasis(self, W_list, mass, k, guard=None, degree=30, tol=1e-9, max_rounds=12, seed=0, ell=None):
        """k smallest eigenpairs of W phi = lambda A phi for a batch of meshes (reference TriMesh.process ->
        laplacian_spectrum: ARPACK on the host, one mesh at a time).
        ell = the dict laplacian_ell returns (operands already on the device; W_list / mass are ignored), or
        W_list: sparse stiffness matrices (host, SciPy) with mass (B,N) lumped masses, or a list of 1-D arrays when the vertex
        counts differ (Phi is then padded to the largest) -- the ELL layout of A^-1/2 W A^-1/2 is then built on the host.
        The iteration runs on the GPU (dm_eigenbasis) until max_j |L x_j - lam_j x_j| <= tol * lam_k.  Meshes too small for the
        filtered subspace iteration (2 (k + guard) > N) take the dense route: the whole space as the subspace, one Rayleigh-Ritz
        step (a Jacobi eigensolve of the N x N operator, N <= 2048: one workgroup per mesh, ~0.3 s at N = 1024).
        Returns (lam (B,k) f64, Phi (B,N,k) f64, resid (B,), rounds)."""
        import numpy as np
        import scipy.sparse as sp
        # (dm_eigenbasis takes the lumped masses as fp32: the problem solved is the one with the ROUNDED masses, and Phi^T A Phi = I
        #  holds for those.  The float64 entry points downstream receive the caller's unrounded mesh.A: the basis is orthonormal
        #  for a mass vector that differs from theirs by <= 6e-8 relative -- far inside the 1e-4 bar on C, and the reason the
        #  eigenbasis tests compare with SciPy on the rounded masses.)
        # Meshes of DIFFERENT vertex counts share a call too: the smaller ones are padded with decoupled vertices whose only entry
        # is a diagonal one AT the Gershgorin bound of the mesh's own operator (max_i sum_q |L_iq| >= lambda_max: the upper end of
        # the interval the Chebyshev filter damps), so the spurious eigenvalue can never fall inside the wanted part of the
        # spectrum.  Their rows of Phi come back ~0 and the caller slices them off.
        if guard is None:
            # guard vectors: 12 .. 32, so that the block k + guard is a multiple of 32 columns where that is possible -- the sparse
            # product gathers whole rows of the block, and 32 doubles are two aligned 128-byte lines (measured, 128 meshes of 2048
            # vertices, k = 20: 79 ms with 32 guard vectors = 52 columns, 46 ms with 12 = 32 columns, one more round, same eigenpairs
            # to 1e-15: tools/eig_sweep.py)
            guard = next((g for g in range(12, 33) if (k + g) % 32 == 0), 32)
        if ell is not None:
            cols_d, vals_d, mass_d, nnz = ell["cols"], ell["vals"], ell["mass32"], int(ell["nnz"])
            B, N = mass_d.shape
            nmin = min(ell["n_verts"])
        else:
            masses = [np.ascontiguousarray(a, dtype=np.float32).astype(np.float64).ravel() for a in mass]
            B, N = len(masses), max(a.shape[0] for a in masses)
            if any(np.any(a <= 0) for a in masses):
                raise ValueError("eigenbasis: every vertex needs a positive lumped mass (isolated or degenerate vertices?)")
            mats = []
            for b in range(B):
                d = sp.diags(1.0 / np.sqrt(masses[b]))
                mats.append((d @ sp.csr_matrix(W_list[b]) @ d).tocsr())
            nnz = max(int(np.diff(Lm.indptr).max()) for Lm in mats)
            cols = np.tile(np.arange(N, dtype=np.int32)[None, :, None], (B, 1, nnz))
            vals = np.zeros((B, N, nnz))
            mass_h = np.ones((B, N))
            for b, Lm in enumerate(mats):
                nb = Lm.shape[0]
                cnt = np.diff(Lm.indptr)
                pos = np.arange(Lm.nnz) - np.repeat(Lm.indptr[:-1], cnt)
                rows = np.repeat(np.arange(nb), cnt)
                cols[b, rows, pos] = Lm.indices
                vals[b, rows, pos] = Lm.data
                mass_h[b, :nb] = masses[b]
                if nb < N:
                    vals[b, nb:, 0] = float(abs(Lm).sum(axis=1).max())
            nmin = min(a.shape[0] for a in masses)
            cols_d = torch.as_tensor(cols).to(self.device)
            vals_d = torch.as_tensor(vals).to(self.device)
            mass_d = torch.as_tensor(mass_h.astype(np.float32)).to(self.device)
        lam = torch.empty((B, k), dtype=torch.float64, device=self.device)
        Phi = torch.empty((B, N, k), dtype=torch.float64, device=self.device)
        resid = torch.empty((B,), dtype=torch.float64, device=self.device)
        if k > nmin:
            raise ValueError(f"eigenbasis: {k} eigenpairs asked of a mesh with {nmin} vertices")
        if 2 * (k + guard) > nmin:
            # (measured: with the wanted range reaching into the upper half of a spectrum the filtered block loses rank and the Ritz step
            #  returns spurious zero pairs whose residual looks converged.)  Dense route: X = I, no filter -- the Rayleigh-Ritz step IS the
            # eigendecomposition of L; the padding rows of a ragged batch sit at their Gershgorin bound, above every wanted pair.
            if N > 2048:
                raise ValueError(f"eigenbasis: k + guard = {k + guard} vectors need a mesh of at least {2 * (k + guard)} vertices "
                                 f"(the smallest has {nmin}); the dense route takes meshes up to 2048 vertices, this batch has {N}")
            X = torch.eye(N, dtype=torch.float64, device=self.device).repeat(B, 1, 1).contiguous()
            self._chk(self.lib.dm_eigenbasis(self.ctx, B, N, nnz, _ptr(cols_d), _ptr(vals_d), _ptr(mass_d), k, N - k, 1, 2, 2,
                                             _ptr(X), _ptr(lam), _ptr(Phi), _ptr(resid)))
            return lam, Phi, resid, 0
        m = min(k + guard, N)
        # A mesh's result must not depend on the batch it is solved in: its start block is drawn for ITS vertex count (one draw per
        # distinct count, the same seed; padding rows start at zero), and its outputs are latched the first time its own residual
        # passes -- the batch iterates on until the last mesh has, but a mesh that was done keeps what it had.
        nvs = ell["n_verts"] if ell is not None else [a.shape[0] for a in masses]
        X = torch.zeros((B, N, m), dtype=torch.float64, device=self.device)
        draws = {}
        for b, nb in enumerate(nvs):
            if nb not in draws:
                g = torch.Generator(device=self.device).manual_seed(seed)
                draws[nb] = torch.randn((nb, m), dtype=torch.float64, device=self.device, generator=g)
            X[b, :nb] = draws[nb]
        lam_w, Phi_w, resid_w = torch.empty_like(lam), torch.empty_like(Phi), torch.empty_like(resid)
        done = torch.zeros((B,), dtype=torch.bool, device=self.device)
        rounds = 0
        for rounds in range(1, max_rounds + 1):
            n_iter = 5 if rounds == 1 else 2
            self._chk(self.lib.dm_eigenbasis(self.ctx, B, N, nnz, _ptr(cols_d), _ptr(vals_d), _ptr(mass_d), k, m - k, n_iter, degree,
                                             0 if rounds == 1 else 1, _ptr(X), _ptr(lam_w), _ptr(Phi_w), _ptr(resid_w)))
            scale = torch.clamp(lam_w[:, -1].abs(), min=1e-300)
            ok = resid_w <= tol * scale
            take = ~done if rounds == max_rounds else (ok & ~done)        # (the last round: whatever is there, the caller judges the residual)
            if B == 1:
                if bool(take[0]):
                    lam, Phi, resid = lam_w, Phi_w, resid_w
            else:
                lam[take], Phi[take], resid[take] = lam_w[take], Phi_w[take], resid_w[take]
            done |= ok
            if bool(done.all()):
                break
        return lam, Phi, resid, rounds

    # ------------------------------------------------------------------ functional map networks (pyFM/FMN)
    FMN_MAX_DIM, FMN_MAX_M = 4096, 256

    def eigh_smallest(self, A, k, guard=None, tol=1e-9, max_rounds=12, degree=30):
        """k smallest eigenpairs of dense symmetric matrices A (n, n) or (B, n, n), n <= 4096 (dm_eigh_smallest; the functional map
        network's scipy.sparse.linalg.eigsh(W, k, sigma=-1e-6)).  Iterates as eigenbasis does, until max_j |A x_j - lam_j x_j| <= tol * d
        with d = max_i |A_ii| -- for a symmetric matrix d <= max |lambda|, so the test is at least as strict as tol * lambda_max -- and
        raises DenseMatchError when max_rounds pass without that.  Route ("fmn_eig_route" 0): the full Jacobi eigendecomposition (n <= 512,
        one call) where n <= 128 or the filtered iteration has no room (2 (k + guard) > n), else the Chebyshev-filtered iteration; 1 / 2
        force one.  Either route reads the residual back: one synchronisation per call on the Jacobi route, one per round on the filtered.
        The start block of the filtered route is drawn from a fixed seed.
        Returns (lam (B,k), V (B,n,k) orthonormal columns, largest entry of each positive, resid (B,), rounds); B dropped for a 2-D A."""
        A = self._dev(A, torch.float64, "A")
        single = A.dim() == 2
        if single:
            A = A[None]
        if A.dim() != 3 or A.shape[1] != A.shape[2]:
            raise ValueError("eigh_smallest: A must be (n, n) or (B, n, n)")
        B, n, _ = A.shape
        k = int(k)
        if not 0 < k <= n:
            raise ValueError(f"eigh_smallest: {k} eigenpairs asked of a {n} x {n} matrix")
        if n > self.FMN_MAX_DIM:
            raise ValueError(f"eigh_smallest: n = {n} is above the limit of {self.FMN_MAX_DIM}")
        if guard is None:
            guard = next((g for g in range(12, 33) if (k + g) % 32 == 0), 32)
        route = self.get_option("fmn_eig_route")
        jacobi = route == 1 or (route == 0 and n <= 512 and (2 * (k + guard) > n or n <= 128))
        bound = torch.clamp(torch.diagonal(A, dim1=1, dim2=2).abs().amax(dim=1), min=1e-300)
        lam = torch.empty((B, k), dtype=torch.float64, device=self.device)
        V = torch.empty((B, n, k), dtype=torch.float64, device=self.device)
        resid = torch.empty((B,), dtype=torch.float64, device=self.device)

        def refuse(rounds):
            return _lib.DenseMatchError(f"eigh_smallest: residual {resid.max().item():.3e} above {tol:g} * max |A_ii| = "
                                        f"{tol * bound.min().item():.3e} after {rounds} rounds")
        if jacobi:
            if n > 512:
                raise ValueError(f"eigh_smallest: the Jacobi route takes n <= 512, not {n}")
            X = torch.eye(n, dtype=torch.float64, device=self.device).repeat(B, 1, 1).contiguous()
            self._chk(self.lib.dm_eigh_smallest(self.ctx, B, n, _ptr(A), n, k, n - k, 1, 2, 2, _ptr(X), _ptr(lam), _ptr(V), _ptr(resid)))
            if not bool((resid <= tol * bound).all()):
                raise refuse(0)
            return (lam[0], V[0], resid[0], 0) if single else (lam, V, resid, 0)
        if 2 * (k + guard) > n:                     # (the block may not reach past the middle of the spectrum: see eigenbasis)
            guard = n // 2 - k
        if guard < 4 or k + guard > 512:
            raise ValueError(f"eigh_smallest: the filtered route needs 2 (k + 4) <= n and k + guard <= 512 (k = {k}, n = {n})")
        m = k + guard
        g = torch.Generator(device=self.device).manual_seed(0)
        X = torch.randn((n, m), dtype=torch.float64, device=self.device, generator=g).repeat(B, 1, 1).contiguous()
        lam_w, V_w, resid_w = torch.empty_like(lam), torch.empty_like(V), torch.empty_like(resid)
        done = torch.zeros((B,), dtype=torch.bool, device=self.device)
        rounds = 0
        for rounds in range(1, max_rounds + 1):
            n_iter = 5 if rounds == 1 else 2
            self._chk(self.lib.dm_eigh_smallest(self.ctx, B, n, _ptr(A), n, k, guard, n_iter, degree, 0 if rounds == 1 else 1, _ptr(X),
                                                _ptr(lam_w), _ptr(V_w), _ptr(resid_w)))
            ok = resid_w <= tol * bound
            take = ~done if rounds == max_rounds else (ok & ~done)
            if B == 1:
                if bool(take[0]):
                    lam, V, resid = lam_w.clone(), V_w.clone(), resid_w.clone()
            else:
                lam[take], V[take], resid[take] = lam_w[take], V_w[take], resid_w[take]
            done |= ok
            if bool(done.all()):
                break
        if not bool(done.all()):
            raise refuse(max_rounds)
        return (lam[0], V[0], resid[0], rounds) if single else (lam, V, resid, rounds)

    def _fmn_maps(self, maps, M, who):
        maps = self._dev(maps, torch.float64, "maps")
        if maps.dim() != 3 or maps.shape[1] != maps.shape[2] or maps.shape[0] == 0:
            raise ValueError(f"{who}: maps must be (E, ldm, ldm) with E >= 1")
        if not 0 < M <= maps.shape[1]:
            raise ValueError(f"{who}: M = {M} must lie in [1, {maps.shape[1]}]")
        return maps

    def fmn_orth_defect(self, maps, M):
        """|FM^T FM - I|_F of the leading M x M block of every map (E, ldm, ldm) -> (E,) f64 (dm_fmn_orth_defect; FMN.set_isometries)"""
        maps = self._fmn_maps(maps, int(M), "fmn_orth_defect")
        out = torch.empty((maps.shape[0],), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_fmn_orth_defect(self.ctx, maps.shape[0], int(M), _ptr(maps), maps.shape[1], _ptr(out)))
        return out

    def fmn_cycle_costs(self, maps, M, cyc_edges):
        """cost of every three-cycle (n_cyc, 3) int32 = edge indices (e_ij, e_jk, e_ki): the maximum over its three rotations of
        |C_a C_b C_c - I|_F on the leading M x M blocks -> (n_cyc,) f64 (dm_fmn_cycle_costs; FMN.get_cycle_weight)"""
        maps = self._fmn_maps(maps, int(M), "fmn_cycle_costs")
        if not isinstance(cyc_edges, torch.Tensor):
            cyc_edges = torch.as_tensor(cyc_edges)
        if cyc_edges.dim() != 2 or cyc_edges.shape[1] != 3:
            raise ValueError("fmn_cycle_costs: cyc_edges must be (n_cyc, 3)")
        bad = cyc_edges.shape[0] and (int(cyc_edges.min()) < 0 or int(cyc_edges.max()) >= maps.shape[0])   # (read where the list is)
        cyc = self._dev(cyc_edges, torch.int32, "cyc_edges")
        if bad:
            raise ValueError(f"fmn_cycle_costs: cycle edge indices must lie in [0, {maps.shape[0]})")
        out = torch.empty((cyc.shape[0],), dtype=torch.float64, device=self.device)
        if cyc.shape[0]:
            self._chk(self.lib.dm_fmn_cycle_costs(self.ctx, maps.shape[0], int(M), _ptr(maps), maps.shape[1], cyc.shape[0], _ptr(cyc), _ptr(out)))
        return out

    def fmn_quad_form(self, n, M, maps, edges, w):
        """the quadratic form of the consistent latent basis, dense (n M, n M) f64 (dm_fmn_quad_form; CLB_quad_form): edges (E, 2) int32,
        w (E,) f64 weights, maps (E, ldm, ldm)"""
        n, M = int(n), int(M)
        maps = self._fmn_maps(maps, M, "fmn_quad_form")
        if not isinstance(edges, torch.Tensor):
            edges = torch.as_tensor(edges)
        if edges.numel() and (int(edges.min()) < 0 or int(edges.max()) >= n):       # (read where the edge list is: the host's for FMN)
            raise ValueError(f"fmn_quad_form: edge ends must lie in [0, {n})")
        edges = self._dev(edges, torch.int32, "edges")
        w = self._dev(w, torch.float64, "w")
        E = maps.shape[0]
        if edges.shape != (E, 2) or w.shape != (E,):
            raise ValueError("fmn_quad_form: edges must be (E, 2) and w (E,)")
        if n * M > self.FMN_MAX_DIM or M > self.FMN_MAX_M:
            raise ValueError(f"fmn_quad_form: n M = {n * M} (limit {self.FMN_MAX_DIM}), M = {M} (limit {self.FMN_MAX_M})")
        W = torch.empty((n * M, n * M), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_fmn_quad_form(self.ctx, n, E, M, _ptr(maps), maps.shape[1], _ptr(edges), _ptr(w), _ptr(W)))
        return W

    def fmn_cclb(self, CLB, evals, m):
        """canonical consistent latent basis (dm_fmn_cclb; FMN.compute_CCLB): CLB (n, M, M), evals (n, >= M) the meshes' eigenvalues ->
        (CCLB (n, M, m), cclb_eigenvalues (m,)) f64"""
        CLB = self._dev(CLB, torch.float64, "CLB")
        evals = self._dev(evals, torch.float64, "evals")
        n, M, _ = CLB.shape
        m = int(m)
        if CLB.shape[2] != M or evals.dim() != 2 or evals.shape[0] != n or evals.shape[1] < M or not 0 < m <= M:
            raise ValueError("fmn_cclb: CLB must be (n, M, M), evals (n, >= M) and 1 <= m <= M")
        cclb = torch.empty((n, M, m), dtype=torch.float64, device=self.device)
        ev = torch.empty((m,), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_fmn_cclb(self.ctx, n, M, m, _ptr(CLB), _ptr(evals), evals.shape[1], _ptr(cclb), _ptr(ev)))
        return cclb, ev

    def scratch(self, name, shape, dtype):
        """a device tensor that belongs to this engine and is handed out again by the next call with the same name, shape and dtype: for
        large intermediates of a call that never reach the user (a gigabyte of precise maps per chunk: allocated per call, the caching
        allocator of a process with other tensors around kept going back to hipMalloc, which stalls every stream)"""
        cache = self.__dict__.setdefault("_scratch", {})
        t = cache.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(tuple(shape), dtype=dtype, device=self.device)
            cache[name] = t
        return t

    def precise_map(self, Phi1, Phi2, Cm, faces1, dense=False, scratch=False, return_info=False):
        """Barycentric projection of every vertex of mesh 2 onto the faces of mesh 1 in the spectral embedding (reference
        get_precise_map, functional.py:221-251).  Returns (face_match (B,N2) int32, bary (B,N2,3) f64[, dense (B,N2,N1) f64]
        [, info (B,) int32]).  return_info=True appends the route word of every pair: 1 if some point of the pair had more
        candidate faces than the kernel lists and every face was re-tested for it, else 0 (same results either way)."""
        sfx, Phi1, Phi2 = self._reals(Phi1, Phi2)
        Cm = self._dev(Cm, torch.float64, "C")
        faces1 = self._dev(faces1, torch.int32, "faces1")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        k2, k1 = Cm.shape[1], Cm.shape[2]
        nf = faces1.shape[1]
        if faces1.shape != (B, nf, 3) or Cm.shape[0] != B:
            raise ValueError("precise_map: faces1 must be (B,nf,3) and C (B,k2,k1)")
        if nf and (int(faces1.min()) < 0 or int(faces1.max()) >= N1):
            raise ValueError("precise_map: face indices must lie in [0, N1)")
        fm = torch.empty((B, N2), dtype=torch.int32, device=self.device)
        bary = torch.empty((B, N2, 3), dtype=torch.float64, device=self.device)
        # (scratch=True: the dense matrices live in this engine's scratch and are overwritten by its next such call)
        M = (self.scratch("precise_dense", (B, N2, N1), torch.float64) if scratch else
             torch.empty((B, N2, N1), dtype=torch.float64, device=self.device)) if dense else None
        info = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(getattr(self.lib, "dm_precise_map" + sfx)(self.ctx, B, N1, N2, k1, k2, nf, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(Cm), _ptr(faces1),
                                          _ptr(fm), _ptr(bary), _ptr(M), _ptr(info)))
        out = (fm, bary, M) if dense else (fm, bary)
        return out + (info,) if return_info else out

    def linear_sum_assignment(self, cost, maximize=False, defer=False):
        """Optimal assignment of every matrix of the batch `cost` (B,nr,nc) f64 -> col_of_row (B,nr) int32, -1 = unassigned
        (identical to scipy.optimize.linear_sum_assignment, reference functional_map.py:57,66,78).
        defer=True: the launches go out and a function is returned that waits for them, raises SciPy's errors and hands back the result
        (a search is a single workgroup busy for milliseconds: a caller with other work for the GPU queues it on another stream meanwhile)."""
        cost = self._dev(cost, torch.float64, "cost")
        if cost.dim() != 3:
            raise ValueError("linear_sum_assignment expects (B,nr,nc)")
        B, nr, nc = cost.shape
        out = torch.empty((B, nr), dtype=torch.int32, device=self.device)
        info = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_linear_sum_assignment(self.ctx, B, nr, nc, _ptr(cost), 1 if maximize else 0, _ptr(out), _ptr(info)))

        def finish(keep=cost):                               # (`keep`: the matrix stays alive until the search has read it)
            worst = int(info.max())                          # (the caller reads the result next: this synchronisation is not extra)
            if worst == 2:
                raise ValueError("matrix contains invalid numeric entries")      # SciPy's messages
            if worst == 1:
                raise ValueError("cost matrix is infeasible")
            return out
        return finish if defer else finish()

    # ------------------------------------------------------------- ragged assignments gathered from one matrix (dm_lsa_gather)
    def _lsa_gather_D(self, D, who):
        """D as the (B, N, ld) float64 device operand of dm_lsa_gather: a device tensor is used where it is when its strides fit the
        ABI (unit stride along a row, one row stride ld >= N, meshes N ld apart); anything else is copied.  Returns (tensor, B, N, ld)."""
        if not isinstance(D, torch.Tensor):
            import warnings
            with warnings.catch_warnings():                  # (a read-only array is only read)
                warnings.simplefilter("ignore", UserWarning)
                D = torch.as_tensor(D)
        if D.dim() == 2:
            D = D[None]
        if D.dim() != 3 or D.shape[1] != D.shape[2] or D.shape[1] < 1:
            raise ValueError(f"{who}: D must be (N, N) or (B, N, N)")
        B, N = int(D.shape[0]), int(D.shape[1])
        fits = (D.device == self.device and D.dtype == torch.float64 and D.stride(2) == 1 and D.stride(1) >= N and
                D.stride(1) < 2 ** 31 and (B == 1 or D.stride(0) == N * D.stride(1)))
        if not fits:
            D = self._dev(D, torch.float64, "D")
        else:
            self._dev(D[:0], torch.float64, "D")              # (the stream check)
        return D, B, N, int(D.stride(1))

    def _lsa_gather_run(self, D, idx, table, maximize, return_assignment, n_out):
        """dm_lsa_gather on a prepared index array (n_idx,) and problem table (P, 6), both int32 NumPy; the means (P,) float64 and,
        on request, the packed col_of_row (n_out,) int32, as NumPy arrays.  Raises SciPy's errors."""
        import numpy as np
        Dd, B, N, ld = D
        P = int(table.shape[0])
        if P == 0:
            return np.zeros(0, np.float64), (np.zeros(0, np.int32) if return_assignment else None)
        idx_d = torch.as_tensor(np.ascontiguousarray(idx, np.int32)).to(self.device)
        table = np.ascontiguousarray(table, np.int32)
        mean = torch.empty((P,), dtype=torch.float64, device=self.device)
        info = torch.empty((P,), dtype=torch.int32, device=self.device)
        out = torch.empty((max(1, n_out),), dtype=torch.int32, device=self.device) if return_assignment else None
        self._chk(self.lib.dm_lsa_gather(self.ctx, B, N, ld, _ptr(Dd), int(idx_d.numel()), _ptr(idx_d), P,
                                         C.c_void_p(table.ctypes.data), 1 if maximize else 0, _ptr(out), _ptr(mean), _ptr(info)))
        worst = int(info.max())
        if worst == 2:
            raise ValueError("matrix contains invalid numeric entries")      # SciPy's messages
        if worst == 1:
            raise ValueError("cost matrix is infeasible")
        return mean.cpu().numpy(), (out.cpu().numpy() if return_assignment else None)

    @staticmethod
    def _index_list(lst, n, who):
        import numpy as np
        a = np.asarray(lst)
        if a.ndim != 1:
            raise ValueError(f"{who}: an index list must be one-dimensional")
        if a.size and not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.bool_)):
            raise ValueError(f"{who}: an index list must hold integers")
        if a.size and (int(a.min()) < 0 or int(a.max()) >= n):
            raise ValueError(f"{who}: vertex indices must lie in [0, {n})")
        return a.astype(np.int32)

    def lsa_gather(self, D, row_lists, col_lists, mesh=None, maximize=False, return_assignment=False, n_verts=None):
        """Many assignments on sub-blocks of one matrix in ONE device call (dm_lsa_gather): problem p is
        scipy.optimize.linear_sum_assignment(D[mesh[p]][np.ix_(row_lists[p], col_lists[p])], maximize) -- the same assignment, ties
        included -- and the mean of its matched entries (the reference's get_distance_between_groups, densematcher/utils.py:115-127).
        D: (N, N) or (B, N, N), NumPy or torch; a float64 device tensor is read in place (a padded batch as heat_geodesic /
        graph_geodesic return it, or a view of one with a row stride).  row_lists / col_lists: P sequences of vertex indices
        (repeats and overlaps allowed, none empty); mesh: the mesh of every problem (default 0); n_verts (B,): the vertex counts of a
        padded batch, for the index check (default N).
        Returns the means (P,) float64 (NumPy); with return_assignment=True also the list of col_of_row arrays (int32, -1 for an
        unassigned row when a problem has more rows than columns).  ValueError with SciPy's texts for an infeasible problem and for
        NaN / the rejected infinity; ValueError for an index outside its mesh and for an empty list."""
        import numpy as np
        Dt = self._lsa_gather_D(D, "lsa_gather")
        B, N = Dt[1], Dt[2]
        P = len(row_lists)
        if len(col_lists) != P:
            raise ValueError("lsa_gather: as many column lists as row lists")
        mesh = np.zeros(P, np.int64) if mesh is None else np.broadcast_to(np.asarray(mesh, np.int64), (P,))
        if P and (mesh.min() < 0 or mesh.max() >= B):
            raise ValueError(f"lsa_gather: mesh indices must lie in [0, {B})")
        nv = np.full(B, N, np.int64) if n_verts is None else np.broadcast_to(np.asarray(n_verts, np.int64), (B,))
        if nv.min() < 1 or nv.max() > N:
            raise ValueError("lsa_gather: n_verts must lie in [1, N]")
        parts, table, off, ooff = [], np.zeros((P, 6), np.int32), 0, 0
        for p in range(P):
            r = self._index_list(row_lists[p], int(nv[mesh[p]]), "lsa_gather")
            c = self._index_list(col_lists[p], int(nv[mesh[p]]), "lsa_gather")
            if r.size == 0 or c.size == 0:
                raise ValueError(f"lsa_gather: problem {p}: an empty index list")
            table[p] = (mesh[p], off, r.size, off + r.size, c.size, ooff)
            parts += [r, c]
            off += r.size + c.size
            ooff += r.size
        idx = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        means, packed = self._lsa_gather_run(Dt, idx, table, maximize, return_assignment, ooff)
        if not return_assignment:
            return means
        return means, [packed[table[p, 5]:table[p, 5] + table[p, 2]] for p in range(P)]

    def groups_dmtx(self, D, groups, n_verts=None):
        """The semantic distance matrices between vertex groups (the reference's get_groups_dmtx, densematcher/utils.py:129-143) of
        a batch of meshes in ONE lsa_gather call: out[i, j] = out[j, i] (i < j) = the mean matched distance of the assignment on
        D[np.ix_(groups[i], groups[j])], 0 on the diagonal and for a pair with an empty group.
        D (N, N) with one list of groups -> one (G, G) float64 NumPy array; D (B, N, N) (meshes padded to the largest, n_verts (B,)
        their vertex counts) with one list of groups per mesh (any numbers of groups) -> a list of B arrays."""
        import numpy as np
        single = (D.dim() if isinstance(D, torch.Tensor) else np.ndim(D)) == 2
        Dt = self._lsa_gather_D(D, "groups_dmtx")
        B, N = Dt[1], Dt[2]
        per_mesh = [groups] if single else list(groups)
        if len(per_mesh) != B:
            raise ValueError(f"groups_dmtx: {len(per_mesh)} lists of groups for {B} meshes")
        nv = np.full(B, N, np.int64) if n_verts is None else np.broadcast_to(np.asarray(n_verts, np.int64), (B,))
        if nv.min() < 1 or nv.max() > N:
            raise ValueError("groups_dmtx: n_verts must lie in [1, N]")
        parts, off, rows, where = [], 0, [], []
        for b, gs in enumerate(per_mesh):
            lists = [self._index_list(g, int(nv[b]), f"groups_dmtx: mesh {b}") for g in gs]
            offs = []
            for g in lists:                                  # every group once in the index array, whatever the number of its pairs
                offs.append(off)
                parts.append(g)
                off += g.size
            for i in range(len(lists)):
                for j in range(i + 1, len(lists)):
                    if lists[i].size and lists[j].size:
                        rows.append((b, offs[i], lists[i].size, offs[j], lists[j].size, 0))
                        where.append((b, i, j))
        table = np.asarray(rows, np.int32).reshape(-1, 6)
        idx = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        means, _ = self._lsa_gather_run(Dt, idx, table, False, False, 0)
        out = [np.zeros((len(gs), len(gs)), np.float64) for gs in per_mesh]
        for (b, i, j), m in zip(where, means):
            out[b][i, j] = out[b][j, i] = m
        return out[0] if single else out

    # ------------------------------------------------------------- map quality measures on the geodesic matrices (dm_map_metrics)
    MM_ACCURACY, MM_CONTINUITY, MM_COVERAGE = 0, 1, 2

    @staticmethod
    def _numpy_index(lst, n, who):
        """an index list with NumPy's rules against an axis of length n: integers in [-n, n), negatives counted from the end
        (IndexError otherwise, NumPy's text); returned as non-negative int32"""
        import numpy as np
        a = np.asarray(lst.cpu() if isinstance(lst, torch.Tensor) else lst)
        if a.ndim != 1:
            raise ValueError(f"{who}: an index list must be one-dimensional")
        if a.size == 0:
            return np.zeros(0, np.int32)
        if not np.issubdtype(a.dtype, np.integer):
            raise IndexError(f"{who}: arrays used as indices must be of integer type")
        lo, hi = int(a.min()), int(a.max())
        if lo < -n or hi >= n:
            raise IndexError(f"{who}: index {lo if lo < -n else hi} is out of bounds for axis 0 with size {n}")
        return np.where(a < 0, a + n, a).astype(np.int32)

    def _mm_batch(self, P, B, N, mesh, n_verts, who):
        """the mesh of every problem (P,) and the vertex counts (B,) of a call, checked"""
        import numpy as np
        mesh = np.zeros(P, np.int64) if mesh is None else np.broadcast_to(np.asarray(mesh, np.int64), (P,))
        if P and (mesh.min() < 0 or mesh.max() >= B):
            raise ValueError(f"{who}: mesh indices must lie in [0, {B})")
        nv = np.full(B, N, np.int64) if n_verts is None else np.broadcast_to(np.asarray(n_verts, np.int64), (B,))
        if nv.min() < 1 or nv.max() > N:
            raise ValueError(f"{who}: n_verts must lie in [1, N]")
        return mesh, np.ascontiguousarray(nv, np.int32)

    class _IndexPool:
        """the index array of one call: a list object that several problems pass is stored once"""

        def __init__(self):
            self.parts, self.off, self.seen = [], 0, {}

        def add(self, obj, extra, make):
            key = (id(obj),) + extra
            if key not in self.seen:
                a = make()
                self.seen[key] = (self.off, a, obj)          # (obj is held: its id stays its own for the call)
                self.parts.append(a)
                self.off += a.size
            return self.seen[key][:2]

        def array(self):
            import numpy as np
            return np.concatenate(self.parts) if self.parts else np.zeros(0, np.int32)

    def _map_metrics_run(self, D, D2, nv, nv2, area, idx, table, scale, n_all):
        """ONE dm_map_metrics launch on a prepared index array and table (P, 8); the values (P,) and `all` (n_all,) as NumPy arrays.
        D / D2: the tuples of _lsa_gather_D or None; area: (B, N) float64 device or None."""
        import numpy as np
        P = int(table.shape[0])
        if P == 0:
            return np.zeros(0, np.float64), np.zeros(0, np.float64)
        if D is not None:
            Dd, B, N, ld = D
        else:
            Dd, B, N, ld = None, int(area.shape[0]), int(area.shape[1]), int(area.shape[1])
        D2d, B2, N2, ld2 = D2 if D2 is not None else (None, 0, 0, 0)
        idx_d = torch.as_tensor(np.ascontiguousarray(idx, np.int32)).to(self.device) if len(idx) else torch.zeros(1, dtype=torch.int32, device=self.device)
        table = np.ascontiguousarray(table, np.int32)
        scale = None if scale is None else np.ascontiguousarray(scale, np.float64)
        value = torch.empty((P,), dtype=torch.float64, device=self.device)
        info = torch.empty((P,), dtype=torch.int32, device=self.device)
        every = torch.empty((n_all,), dtype=torch.float64, device=self.device) if n_all else None
        self._chk(self.lib.dm_map_metrics(self.ctx, B, N, ld, _ptr(Dd), B2, N2, ld2, _ptr(D2d), C.c_void_p(nv.ctypes.data),
                                          C.c_void_p(nv2.ctypes.data) if nv2 is not None else C.c_void_p(0), _ptr(area),
                                          int(len(idx)), _ptr(idx_d), P, C.c_void_p(table.ctypes.data),
                                          C.c_void_p(scale.ctypes.data) if scale is not None else C.c_void_p(0), int(n_all),
                                          _ptr(value), _ptr(every), _ptr(info)))
        if int(info.max()) != 0:                             # (the lists were checked here: not reached through this class)
            raise IndexError("map metrics: an index outside its mesh")
        return value.cpu().numpy(), (every.cpu().numpy() if n_all else np.zeros(0, np.float64))

    def map_metrics_table(self, idx, table, D=None, D2=None, area=None, scale=None, n_verts=None, n_verts2=None, n_all=0):
        """dm_map_metrics as the header states it, for callers that build the table themselves (problems of all three kinds in one
        launch): idx (n_idx,) int32 non-negative indices, table (P, 8) int32 rows (kind, mesh, mesh2, offset a, offset b, length,
        aux, flags), scale (P,) or None; D / D2 as in lsa_gather, area (B, N).  Returns (values (P,), all (n_all,)) as NumPy arrays;
        ValueError for a table the library refuses, IndexError for an index outside its mesh."""
        import numpy as np
        Dt = None if D is None else self._lsa_gather_D(D, "map_metrics_table")
        D2t = None if D2 is None else self._lsa_gather_D(D2, "map_metrics_table")
        if area is not None:
            area = self._dev(area if isinstance(area, torch.Tensor) else torch.as_tensor(np.asarray(area, np.float64)), torch.float64, "area")
            area = area[None] if area.dim() == 1 else area
        if Dt is None and area is None:
            raise ValueError("map_metrics_table: D or area is needed")
        if Dt is not None and area is not None and tuple(area.shape) != (Dt[1], Dt[2]):
            raise ValueError("map_metrics_table: area must be (B, N) like D")
        B, N = (Dt[1], Dt[2]) if Dt is not None else (int(area.shape[0]), int(area.shape[1]))
        _, nv = self._mm_batch(0, B, N, None, n_verts, "map_metrics_table")
        nv2 = None if (D2t is None or n_verts2 is None) else self._mm_batch(0, D2t[1], D2t[2], None, n_verts2, "map_metrics_table")[1]
        table = np.asarray(table, np.int32).reshape(-1, 8)
        return self._map_metrics_run(Dt, D2t, nv, nv2, area, np.asarray(idx, np.int32).reshape(-1), table, scale, int(n_all))

    def geodesic_diameter(self, D, n_verts=None):
        """np.max(D[b, :n_verts[b], :n_verts[b]]) of every mesh of a padded batch (dm_geodesic_diameter; the diameter that the
        reference's geodesic_label_errors normalises by, diffusion_net/geometry.py:773): (B,) float64 NumPy, NaN where an entry is
        NaN.  D: (N, N) or (B, N, N), NumPy or torch; a float64 device tensor is read in place."""
        import numpy as np
        Dd, B, N, ld = self._lsa_gather_D(D, "geodesic_diameter")
        _, nv = self._mm_batch(0, B, N, None, n_verts, "geodesic_diameter")
        out = torch.empty((B,), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_geodesic_diameter(self.ctx, B, N, ld, _ptr(Dd), C.c_void_p(nv.ctypes.data), _ptr(out)))
        return out.cpu().numpy()

    def map_accuracy(self, D, p2p_list, gt_list, mesh=None, scale=None, return_all=False, n_verts=None):
        """The reference's accuracy (pyFM/eval/evaluate.py:29-36) for P maps in ONE device call: problem p is
        d = D[mesh[p]][(p2p_list[p], gt_list[p])] -- the row from the map, the column from the ground truth --, d /= scale[p] element
        by element where a scale is given, and d.mean().  D as in lsa_gather (a float64 device tensor is read in place); index lists
        with NumPy's rules (-n <= i < n, IndexError otherwise); a list object passed for several problems is uploaded once.
        scale: None, one number, one number per problem, or "diameter" (geodesic_diameter, once for the batch).  An empty list gives
        NumPy's nan without a launch.  Returns the means (P,) float64 NumPy; with return_all=True also the list of the d arrays."""
        import numpy as np
        Dt = self._lsa_gather_D(D, "map_accuracy")
        B, N = Dt[1], Dt[2]
        p2p_list, gt_list = list(p2p_list), list(gt_list)
        P = len(p2p_list)
        if len(gt_list) != P:
            raise ValueError("map_accuracy: as many ground-truth lists as maps")
        mesh, nv = self._mm_batch(P, B, N, mesh, n_verts, "map_accuracy")
        if isinstance(scale, str):
            if scale != "diameter":
                raise ValueError("map_accuracy: scale must be None, numbers or 'diameter'")
            sc = self.geodesic_diameter(Dt[0], nv)[mesh]
        elif scale is not None:
            sc = np.array(np.broadcast_to(np.asarray(scale, np.float64), (P,)))
        else:
            sc = None
        pool, rows, where, n_all = self._IndexPool(), [], [], 0
        values = np.full(P, np.nan)
        for p in range(P):
            n = int(nv[mesh[p]])
            oa, a = pool.add(p2p_list[p], (n,), lambda: self._numpy_index(p2p_list[p], n, "map_accuracy"))
            ob, b = pool.add(gt_list[p], (n,), lambda: self._numpy_index(gt_list[p], n, "map_accuracy"))
            if a.size != b.size:
                raise ValueError(f"map_accuracy: problem {p}: a map of {a.size} and a ground truth of {b.size} entries")
            if a.size == 0:
                values[p] = np.zeros(0).mean()               # (NumPy's nan and its warning)
                continue
            flags = (1 if sc is not None else 0) | (2 if return_all else 0)
            rows.append((self.MM_ACCURACY, mesh[p], 0, oa, ob, a.size, n_all, flags))
            where.append(p)
            n_all += a.size if return_all else 0
        table = np.asarray(rows, np.int32).reshape(-1, 8)
        where = np.asarray(where, np.int64)
        got, every = self._map_metrics_run(Dt, None, nv, None, None, pool.array(), table, None if sc is None else sc[where], n_all)
        values[where] = got
        if not return_all:
            return values
        dists = [np.zeros(0) for _ in range(P)]
        for row, p in zip(table, where):
            dists[p] = every[row[6]:row[6] + row[5]].copy()
        return values, dists

    def map_continuity(self, D1, D2, p2p_list, edges_list, mesh1=None, mesh2=None, n_verts1=None, n_verts2=None):
        """The reference's continuity (pyFM/eval/evaluate.py:63-66) for P maps in ONE device call: problem p is
        np.mean(D1[mesh1[p]][(p2p[e0], p2p[e1])] / D2[mesh2[p]][(e0, e1)]) over the edges (e0, e1) = edges_list[p] (E, 2) of the
        target mesh, p2p = p2p_list[p] its map into the source mesh.  D2=None: both sides are meshes of D1.  IEEE division without
        guards: an edge of length zero gives inf or nan and the mean carries it, as NumPy's does.  Index rules, sharing of list
        objects, empty lists and the return as in map_accuracy."""
        import numpy as np
        D1t = self._lsa_gather_D(D1, "map_continuity")
        D2t = D1t if D2 is None else self._lsa_gather_D(D2, "map_continuity")
        p2p_list, edges_list = list(p2p_list), list(edges_list)
        P = len(p2p_list)
        if len(edges_list) != P:
            raise ValueError("map_continuity: as many edge lists as maps")
        mesh1, nv1 = self._mm_batch(P, D1t[1], D1t[2], mesh1, n_verts1, "map_continuity")
        mesh2, nv2 = self._mm_batch(P, D2t[1], D2t[2], mesh2, n_verts1 if (D2 is None and n_verts2 is None) else n_verts2, "map_continuity")
        pool, rows, where = self._IndexPool(), [], []
        values = np.full(P, np.nan)

        def edge_lists(edges, n_map, n2):
            e = np.asarray(edges.cpu() if isinstance(edges, torch.Tensor) else edges)
            if e.ndim != 2 or e.shape[1] != 2:
                raise ValueError("map_continuity: edges must be (E, 2)")
            flat = e.T.reshape(-1)                           # every e0, then every e1
            in_map = self._numpy_index(flat, n_map, "map_continuity")
            if n_map != n2 and not np.array_equal(in_map, self._numpy_index(flat, n2, "map_continuity")):
                raise ValueError("map_continuity: negative edge indices need a map with one entry per target vertex")
            return in_map

        for p in range(P):
            n1, n2 = int(nv1[mesh1[p]]), int(nv2[mesh2[p]])
            oa, a = pool.add(p2p_list[p], (n1,), lambda: self._numpy_index(p2p_list[p], n1, "map_continuity"))
            if a.size == 0 and np.size(edges_list[p]):
                raise IndexError("map_continuity: index 0 is out of bounds for axis 0 with size 0")
            ob, e = pool.add(edges_list[p], (a.size, n2), lambda: edge_lists(edges_list[p], a.size, n2))
            if e.size == 0:
                values[p] = np.zeros(0).mean()
                continue
            rows.append((self.MM_CONTINUITY, mesh1[p], mesh2[p], oa, ob, e.size // 2, a.size, 0))
            where.append(p)
        table = np.asarray(rows, np.int32).reshape(-1, 8)
        got, _ = self._map_metrics_run(D1t, D2t, nv1, nv2, None, pool.array(), table, None, 0)
        values[np.asarray(where, np.int64)] = got
        return values

    def map_coverage(self, area, p2p_list, mesh=None, n_verts=None):
        """The reference's coverage (pyFM/eval/evaluate.py:89-91) for P maps in ONE device call: problem p is
        area[mesh[p]][np.unique(p2p_list[p])].sum() / area[mesh[p]][:n].sum().  area: (N,) or (B, N) vertex areas, NumPy or torch.
        Index rules, sharing of list objects and the return as in map_accuracy; an empty map covers nothing (0.0, as NumPy gives)."""
        import numpy as np
        if not isinstance(area, torch.Tensor):
            area = torch.as_tensor(np.asarray(area, np.float64))
        if area.dim() == 1:
            area = area[None]
        if area.dim() != 2 or area.shape[1] < 1:
            raise ValueError("map_coverage: area must be (N,) or (B, N)")
        area = self._dev(area, torch.float64, "area")
        B, N = int(area.shape[0]), int(area.shape[1])
        p2p_list = list(p2p_list)
        P = len(p2p_list)
        mesh, nv = self._mm_batch(P, B, N, mesh, n_verts, "map_coverage")
        pool, rows = self._IndexPool(), []
        for p in range(P):
            n = int(nv[mesh[p]])
            oa, a = pool.add(p2p_list[p], (n,), lambda: self._numpy_index(p2p_list[p], n, "map_coverage"))
            rows.append((self.MM_COVERAGE, mesh[p], 0, oa, 0, a.size, 0, 0))
        table = np.asarray(rows, np.int32).reshape(-1, 8)
        return self._map_metrics_run(None, None, nv, None, area, pool.array(), table, None, 0)[0]

    def lsa_indicator_ok(self, N1, N2, k1, k2):
        return bool(self.lib.dm_lsa_indicator_ok(self.ctx, int(N1), int(N2), int(k1), int(k2)))

    def lsa_indicator(self, Phi1, Phi2, a1, Cm, dense=None, maximize=True, defer=False):
        """Optimal assignments of the mapped indicators Phi2 C Phi1^T diag(a1) given by their factors (no N2 x N1 matrix is formed: the
        kernel evaluates cost rows from the factors with dm_mapped_indicator's arithmetic, bit for bit) and of the dense (n, N2, N1)
        matrices `dense` in the same launch.  Returns col_of_row (n_ind + n_dense, N2) int32, the indicators first.
        (reference functional_map.py:57, 66, 78: scipy.optimize.linear_sum_assignment(..., maximize=True))"""
        sfx, Phi1, Phi2, a1 = self._reals(Phi1, Phi2, a1)
        Cm = self._dev(Cm, torch.float64, "C")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        k2, k1 = Cm.shape[1], Cm.shape[2]
        nd = 0
        if dense is not None:
            dense = self._dev(dense, torch.float64, "dense")
            if dense.dim() != 3 or dense.shape[1:] != (N2, N1):
                raise ValueError("lsa_indicator: dense matrices must be (n, N2, N1)")
            nd = dense.shape[0]
        out = torch.empty((B + nd, N2), dtype=torch.int32, device=self.device)
        info = torch.empty((B + nd,), dtype=torch.int32, device=self.device)
        self._chk(getattr(self.lib, "dm_lsa_indicator" + sfx)(self.ctx, B, N1, N2, k1, k2, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(a1), _ptr(Cm), nd, _ptr(dense),
                                                             1 if maximize else 0, _ptr(out), _ptr(info)))

        def finish(keep=(Phi1, Phi2, a1, Cm, dense)):        # (defer=True: see linear_sum_assignment)
            worst = int(info.max())
            if worst == 2:
                raise ValueError("matrix contains invalid numeric entries")
            if worst == 1:
                raise ValueError("cost matrix is infeasible")
            return out
        return finish if defer else finish()

    def p2p_to_fm_lstsq(self, p21, Phi1, Phi2, k1, k2):
        """argmin_X |Phi2[:, :k2] X - Phi1[p21, :k1]|_F (reference convert.py:51, no mass matrix) -> (B,k2,k1) f64."""
        sfx, Phi1, Phi2 = self._reals(Phi1, Phi2)
        p21 = self._dev(p21, torch.int32, "p21")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        if p21.shape != (B, N2):
            raise ValueError("p2p_to_fm_lstsq: p21 must be (B,N2)")
        Cm = torch.empty((B, k2, k1), dtype=torch.float64, device=self.device)
        info = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(getattr(self.lib, "dm_p2p_to_fm_lstsq" + sfx)(self.ctx, B, N1, N2, k1, k2, _ptr(p21), _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(Cm),
                                              _ptr(info)))
        bad = torch.nonzero(info).flatten()
        if bad.numel():
            raise _lib.DenseMatchError(f"least-squares map: Phi2^T Phi2 is not positive definite for pairs {bad.tolist()[:8]}")
        return Cm

    def _sub_indices(self, sub, B, name):
        sub = self._dev(sub, torch.int32, name)
        if sub.dim() == 1:
            sub = sub[None].expand(B, -1).contiguous()
        if sub.dim() != 2 or sub.shape[0] != B or sub.shape[1] == 0:
            raise ValueError(f"zoomout: {name} must be (n,) or ({B}, n)")
        return sub

    def zoomout(self, Phi1, Phi2, a2, C0, nit, step=1, return_p2p=False, subsample=None):
        """ZoomOut (dm_zoomout): C0 (B,k0,k0) -> (B,kf,kf), kf = k0 + nit*step [, knn21 of the result (B,N2)].
        subsample = (sub1, sub2), index arrays (n,) shared by the batch or (B, n): the subsampled form (reference
        zoomout_refine(subsample=...), dm_zoomout_sub): the iterations on Phi1[sub1], Phi2[sub2] with the least-squares map (a2 is
        not used and may be None), the returned vertex map on all vertices.  Raises DenseMatchError where Phi2[sub2][:, :kf] has
        no full column rank (fewer distinct samples than kf), ValueError for a sample index outside its mesh."""
        sfx, Phi1, Phi2, a2 = self._reals(Phi1, Phi2, None if subsample is not None else a2)
        C0 = self._dev(C0, torch.float64, "C0")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        if C0.dim() != 3 or C0.shape[0] != B or C0.shape[1] != C0.shape[2]:
            raise ValueError("zoomout: C0 must be (B,k0,k0)")
        k0 = C0.shape[1]
        kf = k0 + nit * step
        assert kf <= ld1, f"Not enough eigenvectors on source : {kf} are needed when {ld1} are provided"
        assert kf <= ld2, f"Not enough eigenvectors on target : {kf} are needed when {ld2} are provided"
        Cout = torch.empty((B, kf, kf), dtype=torch.float64, device=self.device)
        p21 = torch.empty((B, N2), dtype=torch.int32, device=self.device) if return_p2p else None
        if subsample is not None:
            sub1 = self._sub_indices(subsample[0], B, "sub1")
            sub2 = self._sub_indices(subsample[1], B, "sub2")
            info = torch.zeros((B,), dtype=torch.int32, device=self.device)
            self._chk(getattr(self.lib, "dm_zoomout_sub" + sfx)(self.ctx, B, N1, N2, sub1.shape[1], sub2.shape[1], _ptr(sub1), _ptr(sub2),
                                                               k0, nit, step, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(C0), _ptr(Cout),
                                                               _ptr(p21), _ptr(info)))
            info_h = info.cpu()
            bad = torch.nonzero(info_h & 2).flatten()
            if bad.numel():
                raise ValueError(f"zoomout: sample indices outside the mesh for pairs {bad.tolist()[:8]}")
            bad = torch.nonzero(info_h & 1).flatten()
            if bad.numel():
                raise _lib.DenseMatchError(f"subsampled zoomout: Phi2[sub2]^T Phi2[sub2] is not positive definite for pairs {bad.tolist()[:8]} "
                                           f"({sub2.shape[1]} samples for {kf} eigenvectors; duplicated samples?)")
            return (Cout, p21) if return_p2p else Cout
        self._chk(getattr(self.lib, "dm_zoomout" + sfx)(self.ctx, B, N1, N2, k0, nit, step, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(a2),
                                      _ptr(C0), _ptr(Cout), _ptr(p21)))
        return (Cout, p21) if return_p2p else Cout

    def icp(self, Phi1, Phi2, C0, nit=10, return_resid=False):
        """Spectral ICP (reference pyFM/refine/icp.py) -> C (B,k2,k1) f64 with orthonormal columns."""
        sfx, Phi1, Phi2 = self._reals(Phi1, Phi2)
        C0 = self._dev(C0, torch.float64, "C0")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        k2, k1 = C0.shape[1], C0.shape[2]
        Cout = torch.empty_like(C0)
        resid = torch.empty((B,), dtype=torch.float64, device=self.device)
        info = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(getattr(self.lib, "dm_icp" + sfx)(self.ctx, B, N1, N2, k1, k2, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(C0), int(nit), _ptr(Cout),
                                  _ptr(resid), _ptr(info)))
        return (Cout, resid, info) if return_resid else Cout

    def knn_query(self, X, Y):
        """For every row of Y the index of the nearest row of X (float64, exact, lowest index on ties)."""
        X = self._dev(X, torch.float64, "X")
        Y = self._dev(Y, torch.float64, "Y")
        if X.dim() != 3 or Y.dim() != 3 or X.shape[0] != Y.shape[0] or X.shape[2] != Y.shape[2]:
            raise ValueError("knn_query expects X (B,nx,p) and Y (B,ny,p)")
        B, nx, p = X.shape
        ny = Y.shape[1]
        out = torch.empty((B, ny), dtype=torch.int32, device=self.device)
        self._chk(self.lib.dm_knn_query_f64(self.ctx, B, nx, ny, p, _ptr(X), _ptr(Y), _ptr(out)))
        return out

    def knn_query_topk(self, X, Y, k):
        """the k nearest rows of X for every row of Y, nearest first -> (idx (B,ny,k) int32, dist (B,ny,k) f64)"""
        X = self._dev(X, torch.float64, "X")
        Y = self._dev(Y, torch.float64, "Y")
        B, nx, p = X.shape
        ny = Y.shape[1]
        idx = torch.empty((B, ny, k), dtype=torch.int32, device=self.device)
        dist = torch.empty((B, ny, k), dtype=torch.float64, device=self.device)
        self._chk(self.lib.dm_knn_query_topk_f64(self.ctx, B, nx, ny, p, k, _ptr(X), _ptr(Y), _ptr(idx), _ptr(dist)))
        return idx, dist

    def mapped_indicator(self, Phi1, Phi2, a1, Cm):
        """Dense (B,N2,N1) float64 indicator ((Phi2 C) Phi1^T) * a1 -- only for callers that want the matrix."""
        sfx, Phi1, Phi2, a1 = self._reals(Phi1, Phi2, a1)
        Cm = self._dev(Cm, torch.float64, "C")
        B, N1, ld1 = Phi1.shape
        _, N2, ld2 = Phi2.shape
        k2, k1 = Cm.shape[1], Cm.shape[2]
        M = torch.empty((B, N2, N1), dtype=torch.float64, device=self.device)
        self._chk(getattr(self.lib, "dm_mapped_indicator" + sfx)(self.ctx, B, N1, N2, k1, k2, _ptr(Phi1), ld1, _ptr(Phi2), ld2, _ptr(a1),
                                               _ptr(Cm), _ptr(M)))
        return M

    # ------------------------------------------------------------------ spectral descriptors
    def signatures(self, Phi, lam, kind, num, landmarks=None, plain=True, k=None, n_verts=None, out_dtype=torch.float64):
        """Heat / wave kernel signatures (pyFM/signatures.py: mesh_HKS / mesh_WKS, reference functional.py:308-334) of a batch of
        meshes: Phi (B,N,ld) f32|f64 eigenvectors, lam (B,>=k) eigenvalues, kind "HKS" | "WKS", num times / energies, landmarks
        None | (B,P) vertex indices, plain: the vertex's own block leads, k: eigenpairs used (default: all of lam), n_verts (B):
        vertex counts of meshes padded to N.  Returns (B, N, (plain + P) num) on the device, float64 or float32 (rounded once
        from the float64 value), columns [plain | landmark 0 | landmark 1 | ...]; rows past n_verts are 0."""
        import numpy as np
        from .pyFM.signatures import signature_tables
        if out_dtype not in (torch.float64, torch.float32):
            raise ValueError("signatures: out_dtype must be torch.float64 or torch.float32")
        sfx, Phi = self._reals(Phi)
        if Phi.dim() != 3:
            raise ValueError("signatures: Phi must be (B,N,ld)")
        B, N, ld = Phi.shape
        lam = np.asarray(lam.detach().cpu() if isinstance(lam, torch.Tensor) else lam, dtype=np.float64)
        if lam.ndim != 2 or lam.shape[0] != B:
            raise ValueError("signatures: lam must be (B,k)")
        K = lam.shape[1] if k is None else min(int(k), lam.shape[1])
        if K < 2 or K > ld:
            raise ValueError(f"signatures: {K} eigenpairs with {ld} eigenvector columns (at least 2 are needed)")
        num = int(num)
        if num < 1:
            raise ValueError("signatures: at least one time / energy (num >= 1)")
        plain = 1 if plain else 0
        lm = np.zeros((B, 0), np.int32) if landmarks is None else np.ascontiguousarray(np.asarray(landmarks).reshape(B, -1), dtype=np.int32)
        P = lm.shape[1]
        if plain + P < 1:
            raise ValueError("signatures: nothing to compute (plain=False and no landmark)")
        nv = None if n_verts is None else np.ascontiguousarray(np.asarray(n_verts).reshape(B), dtype=np.int32)
        if nv is not None and (nv.min() < 0 or nv.max() > N):
            raise ValueError("signatures: n_verts must lie in [0, N]")
        if P and (lm.min() < 0 or (lm >= (N if nv is None else nv[:, None])).any()):
            raise ValueError("signatures: landmarks must lie in [0, n_verts)")
        tabs = [(signature_tables(lam[b, :K], kind, num, False), signature_tables(lam[b, :K], kind, num, True)) for b in range(B)]
        t = self._dev(np.stack([tb[0][0] for tb in tabs]), torch.float64, "t")
        mu = self._dev(np.stack([tb[0][1] for tb in tabs]), torch.float64, "mu")
        denom = self._dev(np.array([tb[0][2] for tb in tabs], dtype=np.float64), torch.float64, "denom")
        k0 = np.ascontiguousarray([[tb[0][3], tb[1][3]] for tb in tabs], dtype=np.int32)
        out = torch.empty((B, N, (plain + P) * num), dtype=out_dtype, device=self.device)
        ip = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)
        self._chk(getattr(self.lib, "dm_spectral_signatures" + sfx)(
            self.ctx, B, N, ip(nv), K, _ptr(Phi), ld, {"HKS": 0, "WKS": 1}[kind], num, _ptr(t), _ptr(mu), _ptr(denom), ip(k0), P, ip(lm),
            plain, 1 if out_dtype == torch.float32 else 0, _ptr(out)))
        return out

    # ------------------------------------------------------------- shape difference operators (dm_shape_diff_f64, dm_pullback_forms_f64)
    SD_MAX_K1, SD_MAX_K2 = 256, 768

    def shape_difference(self, FM, lam1=None, lam2=None, k1=None):
        """Area and conformal shape difference operators of B functional maps (pyFM shape_difference.py:20, :44), one call:
        SD_a = FM^T FM and SD_c = pinv(diag(lam1[:k1])) FM^T (lam2[:k2, None] * FM), both (B, k1, k1) float64 on the device
        (SD_c is None when the eigenvalues are not given).
        FM (B, k2, ldf) with k1 <= ldf columns in use (k1: default all), lam1 (B, >= k1), lam2 (B, >= k2); NumPy arrays or GPU
        tensors.  k1 <= 256, k2 <= 768 (ValueError otherwise).  No host synchronisation."""
        FM = self._dev(FM, torch.float64, "FM")
        if FM.dim() != 3:
            raise ValueError("shape_difference: FM must be (B,k2,k1)")
        B, k2, ldf = FM.shape
        k1 = ldf if k1 is None else int(k1)
        if not 0 < k1 <= ldf:
            raise ValueError(f"shape_difference: k1 = {k1} with {ldf} columns")
        if (lam1 is None) != (lam2 is None):
            raise ValueError("shape_difference: the conformal operator needs the eigenvalues of both meshes")
        SDa = torch.empty((B, k1, k1), dtype=torch.float64, device=self.device)
        SDc, l1, l2 = None, 0, 0
        if lam1 is not None:
            lam1, lam2 = self._dev(lam1, torch.float64, "lam1"), self._dev(lam2, torch.float64, "lam2")
            if lam1.dim() != 2 or lam2.dim() != 2 or lam1.shape[0] != B or lam2.shape[0] != B or lam1.shape[1] < k1 or lam2.shape[1] < k2:
                raise ValueError(f"shape_difference: a ({k2},{k1}) map needs lam1 (B,>={k1}) and lam2 (B,>={k2})")
            SDc, l1, l2 = torch.empty((B, k1, k1), dtype=torch.float64, device=self.device), lam1.shape[1], lam2.shape[1]
        self._chk(self.lib.dm_shape_diff_f64(self.ctx, B, k1, k2, _ptr(FM), ldf, _ptr(lam1), l1, _ptr(lam2), l2, _ptr(SDa), _ptr(SDc)))
        return SDa, SDc

    def _vertex_maps(self, p21, B, N2, N1, nv1, nv2, who):
        """B vertex maps (B, N2) into meshes of N1 (nv1[b]) vertices as a non-negative int32 device tensor, with NumPy's index rules
        -- integers in [-n1, n1), negatives counted from the end, IndexError otherwise -- checked on the device (one synchronisation);
        entries past nv2[b] are not looked at and come out 0"""
        import numpy as np
        p = p21 if isinstance(p21, torch.Tensor) else torch.as_tensor(np.asarray(p21))
        if p.dtype.is_floating_point or p.dtype == torch.bool:
            raise IndexError(f"{who}: arrays used as indices must be of integer type")
        if tuple(p.shape) != (B, N2):
            raise ValueError(f"{who}: p21 must be (B,N2)")
        p = p.to(self.device)
        n1 = torch.full((B, 1), N1, dtype=torch.int64, device=self.device) if nv1 is None else torch.as_tensor(nv1.astype(np.int64)).to(self.device)[:, None]
        live = None if nv2 is None else (torch.arange(N2, device=self.device)[None, :] < torch.as_tensor(nv2.astype(np.int64)).to(self.device)[:, None])
        bad = (p < -n1) | (p >= n1)
        if live is not None:
            bad &= live
        if bool(bad.any()):
            b, i = (int(x) for x in bad.nonzero()[0])
            raise IndexError(f"{who}: pair {b}: index {int(p[b, i])} is out of bounds for axis 0 with size {int(n1[b, 0])}")
        p = torch.where(p < 0, p + n1, p)
        if live is not None:
            p = torch.where(live, p, torch.zeros_like(p))
        return p.to(torch.int32).contiguous()

    def pullback_forms(self, p21, Phi1, W, mass2, k1, lam1=None, n_verts1=None, n_verts2=None):
        """The quadratic forms of the target mesh pulled back through vertex maps (pyFM shape_difference.py:94-96, the 'semican'
        operators), B pairs in one launch: with X = Phi1[p21, :k1]
            Ga = X^T diag(mass2) X,    Gw = X^T (W X)   -- or pinv(diag(lam1[:k1])) X^T (W X), the conformal operator, when lam1 is given.
        p21 (B, N2) integers with NumPy's index rules (IndexError for an entry outside [-n1, n1)), Phi1 (B, N1, ld1 >= k1) float64,
        mass2 (B, N2), lam1 (B, >= k1); NumPy arrays or GPU tensors.  W: per pair a SciPy sparse matrix or the (cols, w) device rows
        (n, nnz) of laplacian_ell, as heat_geodesic_factor takes them -- or one (cols (B, N2, nnz), w (B, N2, nnz)) pair of tensors for
        the whole batch.  n_verts1 / n_verts2 (B,): the vertex counts of padded batches.  Returns (Ga, Gw), (B, k1, k1) float64 on the
        device.  A pair's bits do not depend on the other pairs or on the padding.  One host synchronisation: the check of p21."""
        import numpy as np
        Phi1 = self._dev(Phi1, torch.float64, "Phi1")
        mass2 = self._dev(mass2, torch.float64, "mass2")
        if Phi1.dim() != 3 or mass2.dim() != 2 or mass2.shape[0] != Phi1.shape[0]:
            raise ValueError("pullback_forms: Phi1 must be (B,N1,ld1), mass2 (B,N2)")
        B, N1, ld1 = Phi1.shape
        N2 = mass2.shape[1]
        k1 = int(k1)
        if not 0 < k1 <= ld1:
            raise ValueError(f"pullback_forms: k1 = {k1} with {ld1} eigenvector columns")
        nv = []
        for name, n_verts, N in (("n_verts1", n_verts1, N1), ("n_verts2", n_verts2, N2)):
            a = None if n_verts is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_verts, np.int64), (B,)), dtype=np.int32)
            if a is not None and (a.min() < 1 or a.max() > N):
                raise ValueError(f"pullback_forms: {name} must lie in [1, {N}]")
            nv.append(a)
        nv1, nv2 = nv
        # the vertex maps: NumPy's rules against each pair's own source mesh, checked before anything is launched
        p = self._vertex_maps(p21, B, N2, N1, nv1, nv2, "pullback_forms")
        # ---- the stiffness rows
        if isinstance(W, tuple) and len(W) == 2 and isinstance(W[0], torch.Tensor) and W[0].dim() == 3:
            cols, wv = self._dev(W[0], torch.int32, "cols"), self._dev(W[1], torch.float64, "w")
            if cols.shape[:2] != (B, N2) or wv.shape != cols.shape:
                raise ValueError(f"pullback_forms: batched device rows must be (B,N2,nnz), got {tuple(cols.shape)}")
            nnz = int(cols.shape[2])
        else:
            if len(W) != B:
                raise ValueError(f"pullback_forms: {len(W)} stiffness matrices for {B} pairs")
            rows = [self._stiffness_rows(Wb, N2 if nv2 is None else int(nv2[b]), "pullback_forms", b) for b, Wb in enumerate(W)]
            nnz = max(int(c.shape[1]) for c, _ in rows)
            cols = torch.full((B, N2, nnz), -1, dtype=torch.int32, device=self.device)
            wv = torch.zeros((B, N2, nnz), dtype=torch.float64, device=self.device)
            for b, (c, w) in enumerate(rows):
                cols[b, :c.shape[0], :c.shape[1]] = c.to(self.device, torch.int32)
                wv[b, :w.shape[0], :w.shape[1]] = w.to(self.device, torch.float64)
        if nnz < 1:
            raise ValueError("pullback_forms: empty stiffness rows")
        ld_l1 = 0
        if lam1 is not None:
            lam1 = self._dev(lam1, torch.float64, "lam1")
            if lam1.dim() != 2 or lam1.shape[0] != B or lam1.shape[1] < k1:
                raise ValueError(f"pullback_forms: lam1 must be (B,>={k1})")
            ld_l1 = lam1.shape[1]
        Ga = torch.empty((B, k1, k1), dtype=torch.float64, device=self.device)
        Gw = torch.empty((B, k1, k1), dtype=torch.float64, device=self.device)
        ip = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.dm_pullback_forms_f64(self.ctx, B, N1, N2, k1, _ptr(p), _ptr(Phi1), ld1, _ptr(cols), _ptr(wv), nnz, _ptr(mass2),
                                                 ip(nv1), ip(nv2), _ptr(lam1), ld_l1, _ptr(Ga), _ptr(Gw)))
        return Ga, Gw

    # ------------------------------------------------------------------ the hot path, one batch
    def match(self, batch, k=None, w_descr=1e4, w_lap=1e3, knn=True, ind=True, check=False):
        """project -> pinned column -> solve -> vertex maps for a batch of pairs (BASELINE config 2).

        `batch` is a dict with Phi1, Phi2, lam1, lam2, a1, a2, F1, F2 (device tensors).
        Returns dict(C, knn21, knn12, ind21, ind12).  No host synchronisation inside
        (unless check=True)."""
        Phi1, Phi2 = batch["Phi1"], batch["Phi2"]
        k1 = k if k is not None else batch["lam1"].shape[1]
        k2 = k if k is not None else batch["lam2"].shape[1]
        lam1 = batch["lam1"][:, :k1].contiguous()
        lam2 = batch["lam2"][:, :k2].contiguous()
        if batch["F1"].dtype == torch.float16 and batch["F2"].dtype == torch.float16:
            Cm = self.fmap_fit(Phi1, Phi2, batch["a1"], batch["a2"], batch["F1"], batch["F2"], lam1, lam2, w_descr, w_lap, k1, k2, check=check)
        else:
            A = self.project(Phi1, batch["a1"], batch["F1"], k1)
            Bm = self.project(Phi2, batch["a2"], batch["F2"], k2)
            c00 = self.c00(Phi1, Phi2, batch["a1"], batch["a2"])
            Cm = self.fmap_solve(A, Bm, lam1, lam2, c00, w_descr, w_lap, check=check)
        out = self.fm_to_p2p(Phi1, Phi2, batch["a1"], Cm, knn=knn, ind=ind)
        out["C"] = Cm
        return out


_default_engines = {}


def default_engine(device=None):
    """One engine per (device, current stream), created on first use."""
    if not torch.cuda.is_available():
        raise RuntimeError("densematcher_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
    dev = torch.cuda.current_device() if device is None else (device if isinstance(device, int) else torch.device(device).index or 0)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _default_engines:
        _default_engines[key] = MatchEngine(dev)
    return _default_engines[key]

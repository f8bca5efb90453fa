"""
MatchEngine, mesh operators: tufted covers, cotangent Laplacians, eigenbases, dense eigenpairs, spectral signatures.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._operands import counts, csr_to_ell, host_ptr, pad_stack, ptr as _ptr


class _MeshOps:
    def tufted_covers(self, meshes, mollify_factor=1e-5, n_threads=0):
        """The tufted intrinsic-Delaunay cover of every (verts, faces) in `meshes` (dm_tufted_cover_batch: host C++ on a thread pool,
        like the reference's robust_laplacian wheel).  Returns [(T (2 nf, 3) int32, L (2 nf, 3) f64, flips, converged, eps)]."""
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
        Bn = len(tris)
        if lens is None and verts is None:
            raise ValueError("laplacian_ell: pass intrinsic lengths or vertex coordinates")
        n_verts = [int(np.asarray(v).shape[0]) for v in verts] if verts is not None else [int(np.max(t)) + 1 for t in tris]
        N, nt = max(n_verts), max(int(np.asarray(t).shape[0]) for t in tris)
        tri_d = torch.as_tensor(pad_stack(tris, (nt, 3), -1, np.int32)).to(self.device)
        len_d = vert_d = None
        if lens is not None:
            len_d = torch.as_tensor(pad_stack(lens, (nt, 3), 1.0, np.float64)).to(self.device)
        else:
            vert_d = torch.as_tensor(pad_stack(verts, (N, 3), 0.0, np.float64)).to(self.device)
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
            cols = np.tile(np.arange(N, dtype=np.int32)[None, :, None], (B, 1, nnz))     # (a padding entry: the row's own index, value 0)
            vals = np.zeros((B, N, nnz))
            mass_h = np.ones((B, N))
            for b, Lm in enumerate(mats):
                nb = Lm.shape[0]
                cols[b, :nb], vals[b, :nb] = csr_to_ell(Lm.indptr, Lm.indices, Lm.data, nb, nnz, np.arange(nb)[:, None])
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

    # ------------------------------------------------------------------ spectral descriptors
    def signatures(self, Phi, lam, kind, num, landmarks=None, plain=True, k=None, n_verts=None, out_dtype=torch.float64):
        """Heat / wave kernel signatures (pyFM/signatures.py: mesh_HKS / mesh_WKS, reference functional.py:308-334) of a batch of
        meshes: Phi (B,N,ld) f32|f64 eigenvectors, lam (B,>=k) eigenvalues, kind "HKS" | "WKS", num times / energies, landmarks
        None | (B,P) vertex indices, plain: the vertex's own block leads, k: eigenpairs used (default: all of lam), n_verts (B):
        vertex counts of meshes padded to N.  Returns (B, N, (plain + P) num) on the device, float64 or float32 (rounded once
        from the float64 value), columns [plain | landmark 0 | landmark 1 | ...]; rows past n_verts are 0."""
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
        nv = None if n_verts is None else counts(n_verts, B, N, 0, "signatures")
        if P and (lm.min() < 0 or (lm >= (N if nv is None else nv[:, None])).any()):
            raise ValueError("signatures: landmarks must lie in [0, n_verts)")
        tabs = [(signature_tables(lam[b, :K], kind, num, False), signature_tables(lam[b, :K], kind, num, True)) for b in range(B)]
        t = self._dev(np.stack([tb[0][0] for tb in tabs]), torch.float64, "t")
        mu = self._dev(np.stack([tb[0][1] for tb in tabs]), torch.float64, "mu")
        denom = self._dev(np.array([tb[0][2] for tb in tabs], dtype=np.float64), torch.float64, "denom")
        k0 = np.ascontiguousarray([[tb[0][3], tb[1][3]] for tb in tabs], dtype=np.int32)
        out = torch.empty((B, N, (plain + P) * num), dtype=out_dtype, device=self.device)
        self._chk(getattr(self.lib, "dm_spectral_signatures" + sfx)(
            self.ctx, B, N, host_ptr(nv), K, _ptr(Phi), ld, {"HKS": 0, "WKS": 1}[kind], num, _ptr(t), _ptr(mu), _ptr(denom), host_ptr(k0), P, host_ptr(lm),
            plain, 1 if out_dtype == torch.float32 else 0, _ptr(out)))
        return out

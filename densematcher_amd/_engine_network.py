"""
MatchEngine, networks of maps: functional map networks (pyFM FMN) and shape difference operators.
"""
import numpy as np
import torch

from ._operands import counts, host_ptr, ptr as _ptr, stack_ell


class _NetworkOps:
    # ------------------------------------------------------------------ functional map networks (pyFM/FMN)
    FMN_MAX_DIM, FMN_MAX_M = 4096, 256

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
        Phi1 = self._dev(Phi1, torch.float64, "Phi1")
        mass2 = self._dev(mass2, torch.float64, "mass2")
        if Phi1.dim() != 3 or mass2.dim() != 2 or mass2.shape[0] != Phi1.shape[0]:
            raise ValueError("pullback_forms: Phi1 must be (B,N1,ld1), mass2 (B,N2)")
        B, N1, ld1 = Phi1.shape
        N2 = mass2.shape[1]
        k1 = int(k1)
        if not 0 < k1 <= ld1:
            raise ValueError(f"pullback_forms: k1 = {k1} with {ld1} eigenvector columns")
        nv1 = None if n_verts1 is None else counts(n_verts1, B, N1, 1, "pullback_forms", "n_verts1", N1)
        nv2 = None if n_verts2 is None else counts(n_verts2, B, N2, 1, "pullback_forms", "n_verts2", N2)
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
            cols, wv = stack_ell(rows, N2, self.device)
            nnz = int(cols.shape[2])
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
        self._chk(self.lib.dm_pullback_forms_f64(self.ctx, B, N1, N2, k1, _ptr(p), _ptr(Phi1), ld1, _ptr(cols), _ptr(wv), nnz, _ptr(mass2),
                                                 host_ptr(nv1), host_ptr(nv2), _ptr(lam1), ld_l1, _ptr(Ga), _ptr(Gw)))
        return Ga, Gw

"""
MatchEngine, DiffusionNet: the operators of a batch of meshes, the forward pass, fp32 or -- for a halved module -- fp16 operands, and
the backward pass of the fp32 kernels and of the fp16 kernels (mixed precision: fp16 operands, float32 gradients).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._operands import pad_stack, ptr as _ptr

_HALF_OR_SINGLE = (torch.float16, torch.float32)


def _flag(t):
    return _lib.DM_F16 if t.dtype == torch.float16 else _lib.DM_F32


def _kept(t):
    """the dtype in which a floating-point operand goes to the fp16 kernels: its own when it is float16 or float32, else float32"""
    dtype = t.dtype if isinstance(t, torch.Tensor) else torch.as_tensor(t).dtype
    return dtype if dtype in _HALF_OR_SINGLE else torch.float32


class _DiffusionNetOps:
    # ------------------------------------------------------------- DiffusionNet operators (dm_dnet_*)
    def _dnet_assemble(self, V, F, normals):
        """dm_dnet_rows + dm_dnet_ell of the meshes (V[b] (n_b, 3) float64, F[b] (m_b, 3) int32 NumPy arrays; normals: a list of
        (n_b, 3) arrays or None), padded as laplacian_ell pads.  Returns the dict of device tensors."""
        from .diffusion_net import _host
        Bn = len(V)
        n_verts = [int(v.shape[0]) for v in V]
        N, nt = max(n_verts), max(int(f.shape[0]) for f in F)
        # (through _dev: it refuses a call under another stream than the engine's, where the allocator could recycle the scratch below
        #  while the context's stream still uses it)
        tri_d = self._dev(pad_stack(F, (nt, 3), -1, np.int32), torch.int32, "tri")
        vert_d = self._dev(pad_stack(V, (N, 3), 0.0, np.float64), torch.float64, "verts")
        nrm_d = self._dev(pad_stack(normals, (N, 3), 0.0, np.float64), torch.float64, "normals") if normals is not None else None
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

    # ------------------------------------------------------------- DiffusionNet layers: what the fp32 and the fp16 family share
    # (`who` is the public method an error message names; `half` picks the dm_dnet_*_f16 family)
    def _dnet_counts(self, n_verts, Bn):
        if n_verts is None:
            return None
        nv = self._dev(n_verts, torch.int32, "n_verts")
        if nv.shape != (Bn,):
            raise ValueError(f"n_verts: expected {Bn} counts, got {tuple(nv.shape)}")
        return nv

    def _dnet_out(self, out, Bn, N, C, name, dtype=torch.float32):
        if out is None:
            return torch.empty((Bn, N, C), dtype=dtype, device=self.device), C
        if out.dtype != dtype or out.device != self.device or tuple(out.shape) != (Bn, N, C):
            raise ValueError(f"{name}: out must be a {str(dtype)[6:]} ({Bn}, {N}, {C}) tensor on {self.device}")
        o, ld = self._strided(out, dtype, name)
        if o is not out:
            raise ValueError(f"{name}: out must have adjacent elements in a row and evenly spaced rows")
        return out, ld

    def _dnet_ws(self, nbytes):
        return torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=self.device)

    def _dnet_ell_rows(self, who, Bn, N, rows, t=""):
        """(row_len, cols, gx, gy) of the gradient operators (t = "_t": of their transposes) on the device, held to (B,N) and (B,N,nnz)"""
        row_len, cols = self._dev(rows[0], torch.int32, "row_len" + t), self._dev(rows[1], torch.int32, "cols" + t)
        gx, gy = self._dev(rows[2], torch.float32, "gx" + t), self._dev(rows[3], torch.float32, "gy" + t)
        if cols.dim() != 3 or tuple(cols.shape[:2]) != (Bn, N) or gx.shape != cols.shape or gy.shape != cols.shape or tuple(row_len.shape) != (Bn, N):
            raise ValueError(f"{who}: row_len{t} (B,N), cols{t} / gx{t} / gy{t} (B,N,nnz{t})")
        return row_len, cols, gx, gy

    def _dnet_matrices(self, who, A_re, A_im, dtype, Cw):
        """A_re and A_im (or None) as (C, C) operands that share one leading dimension: (A_re, A_im, lda)"""
        Are, lda = self._strided(A_re, dtype, "A_re")
        Aim = None
        if A_im is not None:
            Aim, lda2 = self._strided(A_im, dtype, "A_im")
            if lda2 != lda:
                Are, Aim, lda = Are.contiguous(), Aim.contiguous(), Cw
        if tuple(Are.shape) != (Cw, Cw) or (Aim is not None and tuple(Aim.shape) != (Cw, Cw)):
            raise ValueError(f"{who}: A_re / A_im must be (C, C)")
        return Are, Aim, lda

    @staticmethod
    def _dnet_src_args(mats, half):
        """the (pointer, width, ld[, dtype flag]) argument groups of up to three sources, absent ones null"""
        a = [(_ptr(m), m.shape[2], ld) + ((_flag(m),) if half else ()) for m, ld in mats]
        return a + [(_ptr(None), 0, 0) + ((_lib.DM_F32,) if half else ())] * (3 - len(a))

    def _dnet_linear_operands(self, who, half, srcs, weight, bias, resid):
        """The operands of a linear layer, checked against each other.  fp16 family: a source or a bias keeps its dtype when that is
        float16 or float32, the weight is float16.  Returns (flat, mats, W, ldw, bias, R, ldr)."""
        srcs = [srcs] if isinstance(srcs, torch.Tensor) else list(srcs)
        if not 1 <= len(srcs) <= 3:
            raise ValueError(f"{who}: one to three sources")
        flat = srcs[0].dim() == 2
        if flat:
            srcs = [s.unsqueeze(0) for s in srcs]
            resid = None if resid is None else resid.unsqueeze(0)
        mats = [self._strided(s, _kept(s) if half else torch.float32, "src") for s in srcs]
        Bn, N = mats[0][0].shape[:2]
        if any(m.shape[:2] != (Bn, N) for m, _ in mats):
            raise ValueError(f"{who}: the sources differ in their leading dimensions")
        W, ldw = self._strided(weight, torch.float16 if half else torch.float32, "weight")
        if W.dim() != 2 or W.shape[1] != sum(m.shape[2] for m, _ in mats):
            raise ValueError(f"{who}: weight {tuple(W.shape)} does not match the summed source widths {sum(m.shape[2] for m, _ in mats)}")
        bias = None if bias is None else self._dev(bias, _kept(bias) if half else torch.float32, "bias")
        if bias is not None and bias.shape != (W.shape[0],):
            raise ValueError(f"{who}: bias must be (C_out,)")
        R, ldr = (None, 0) if resid is None else self._strided(resid, torch.float32, "resid")
        if R is not None and tuple(R.shape) != (Bn, N, W.shape[0]):
            raise ValueError(f"{who}: resid must have the shape of the output")
        return flat, mats, W, ldw, bias, R, ldr

    def _dnet_gradient_features(self, who, half, x, row_len, cols, gx, gy, A_re, A_im, n_verts, out):
        X, ldx = self._strided(x, torch.float32, "x")
        Bn, N, Cw = X.shape
        row_len, cols, gx, gy = self._dnet_ell_rows(who, Bn, N, (row_len, cols, gx, gy))
        Are, Aim, lda = self._dnet_matrices(who, A_re, A_im, torch.float16 if half else torch.float32, Cw)
        nv = self._dnet_counts(n_verts, Bn)
        out, ldo = self._dnet_out(out, Bn, N, Cw, who)
        fn = self.lib.dm_dnet_gradfeat_f16 if half else self.lib.dm_dnet_gradfeat_f32
        self._chk(fn(self.ctx, Bn, N, Cw, cols.shape[2], _ptr(row_len), _ptr(cols), _ptr(gx), _ptr(gy), _ptr(X), ldx, _ptr(Are), _ptr(Aim), lda, _ptr(nv),
                     _ptr(out), ldo))
        return out

    def _dnet_linear_backward(self, who, half, grad_out, srcs, weight, y, n_verts, need_src, need_weight, need_bias, out):
        lib, sfx = self.lib, "_f16" if half else "_f32"
        G, ldg = self._strided(grad_out, torch.float32, "grad_out")
        flat = G.dim() == 2
        if flat:
            G = G.unsqueeze(0)
        Bn, N, C_out = G.shape
        srcs = [srcs] if isinstance(srcs, (torch.Tensor, int)) else list(srcs)
        if not 1 <= len(srcs) <= 3:
            raise ValueError(f"{who}: one to three sources")
        widths = [int(s) if isinstance(s, int) else int(s.shape[-1]) for s in srcs]
        need_src = [bool(need_src)] * len(srcs) if isinstance(need_src, bool) else [bool(f) for f in need_src]
        if len(need_src) != len(srcs):
            raise ValueError(f"{who}: need_src has one flag per source")
        W, ldw = (None, 0)
        if any(need_src):
            if weight is None:
                raise ValueError(f"{who}: the gradient of a source reads the weight")
            W, ldw = self._strided(weight, torch.float16 if half else torch.float32, "weight")
            if W.dim() != 2 or tuple(W.shape) != (C_out, sum(widths)):
                raise ValueError(f"{who}: weight {tuple(W.shape)} does not match grad_out ({C_out}) and the summed source widths {sum(widths)}")
        Y, ldy = (None, 0)
        if y is not None:
            Y, ldy = self._strided(y.unsqueeze(0) if flat else y, torch.float32, "y")
            if tuple(Y.shape) != (Bn, N, C_out):
                raise ValueError(f"{who}: y must have the shape of grad_out")
        nv = self._dnet_counts(n_verts, Bn)
        act = 0 if Y is None else 1
        d_src = [None] * len(srcs)
        if any(need_src):
            outs = [None] * len(srcs) if out is None else list(out)
            a = []
            for s, (w, need) in enumerate(zip(widths, need_src)):
                if need:
                    d_src[s], ld = self._dnet_out(None if outs[s] is None else (outs[s].unsqueeze(0) if flat else outs[s]), Bn, N, w, who)
                    a.append((d_src[s], w, ld))
                else:
                    a.append((None, w, w))
            a += [(None, 0, 0)] * (3 - len(a))
            self._chk(getattr(lib, "dm_dnet_linear_bwd_data" + sfx)(self.ctx, Bn, N, C_out, len(srcs), _ptr(G), ldg, _ptr(Y), ldy, act, _ptr(W), ldw,
                                                                    _ptr(nv), _ptr(a[0][0]), a[0][1], a[0][2], _ptr(a[1][0]), a[1][1], a[1][2],
                                                                    _ptr(a[2][0]), a[2][1], a[2][2]))
        dW = db = None
        if need_weight or need_bias:
            if any(isinstance(s, int) for s in srcs):
                raise ValueError(f"{who}: the weight and bias gradients read the sources")
            mats = [self._strided(s.unsqueeze(0) if flat else s, _kept(s) if half else torch.float32, "src") for s in srcs]
            if any(tuple(m.shape[:2]) != (Bn, N) for m, _ in mats):
                raise ValueError(f"{who}: the sources differ from grad_out in their leading dimensions")
            a = self._dnet_src_args(mats, half)
            dW = torch.empty((C_out, sum(widths)), dtype=torch.float32, device=self.device) if need_weight else None
            db = torch.empty((C_out,), dtype=torch.float32, device=self.device) if need_bias else None
            ws = self._dnet_ws((lib.dm_dnet_linear_bwd_f16_bytes if half else lib.dm_dnet_linear_bwd_bytes)(Bn, C_out, sum(widths)))
            self._chk(getattr(lib, "dm_dnet_linear_bwd_weight" + sfx)(self.ctx, Bn, N, C_out, len(mats), _ptr(G), ldg, _ptr(Y), ldy, act, *a[0], *a[1], *a[2],
                                                                      _ptr(nv), _ptr(ws), _ptr(dW), sum(widths), _ptr(db)))
        if flat:
            d_src = [None if d is None else d[0] for d in d_src]
        return d_src, dW, db

    def _dnet_gradient_features_backward(self, who, half, grad_out, x, row_len, cols, gx, gy, rows_t, A_re, A_im, n_verts, need_x, need_A, out):
        lib = self.lib
        G, ldg = self._strided(grad_out, torch.float32, "grad_out")
        X, ldx = self._strided(x, torch.float32, "x")
        Bn, N, Cw = X.shape
        if tuple(G.shape) != (Bn, N, Cw):
            raise ValueError(f"{who}: grad_out must have the shape of x")
        row_len, cols, gx, gy = self._dnet_ell_rows(who, Bn, N, (row_len, cols, gx, gy))
        rl_t = cols_t = gx_t = gy_t = None
        nnz_t = 0
        if need_x:
            if rows_t is None:
                raise ValueError(f"{who}: the gradient of x reads the transposed rows")
            rl_t, cols_t, gx_t, gy_t = self._dnet_ell_rows(who, Bn, N, rows_t, "_t")
            nnz_t = cols_t.shape[2]
        Are, Aim, lda = self._dnet_matrices(who, A_re, A_im, torch.float16 if half else torch.float32, Cw)
        nv = self._dnet_counts(n_verts, Bn)
        dx, lddx = self._dnet_out(out, Bn, N, Cw, who) if need_x else (None, 0)
        dAre = torch.empty((Cw, Cw), dtype=torch.float32, device=self.device) if need_A else None
        dAim = torch.empty((Cw, Cw), dtype=torch.float32, device=self.device) if need_A and Aim is not None else None
        ws = self._dnet_ws((lib.dm_dnet_gradfeat_bwd_f16_bytes if half else lib.dm_dnet_gradfeat_bwd_bytes)(Bn, N, Cw))
        fn = lib.dm_dnet_gradfeat_bwd_f16 if half else lib.dm_dnet_gradfeat_bwd_f32
        self._chk(fn(self.ctx, Bn, N, Cw, cols.shape[2], _ptr(row_len), _ptr(cols), _ptr(gx), _ptr(gy), nnz_t, _ptr(rl_t), _ptr(cols_t), _ptr(gx_t),
                     _ptr(gy_t), _ptr(G), ldg, _ptr(X), ldx, _ptr(Are), _ptr(Aim), lda, _ptr(nv), _ptr(ws), _ptr(dx), lddx, _ptr(dAre), _ptr(dAim), Cw))
        return dx, dAre, dAim

    # ------------------------------------------------------------- DiffusionNet forward (dm_dnet_*_f32)
    def dnet_linear(self, srcs, weight, bias=None, resid=None, relu=False, n_verts=None, out=None):
        """out[b,i,:] = act(concat(srcs)[b,i,:] weight^T + bias) + resid[b,i,:] (dm_dnet_linear_f32): srcs one tensor or up to three
        (B, N, w_s) (or all (N, w_s)), weight (C_out, sum w_s) as nn.Linear stores it; the concatenation is never formed.  n_verts
        (B) int32: rows behind a mesh's count are not read and come out as zeros."""
        flat, mats, W, ldw, bias, R, ldr = self._dnet_linear_operands("dnet_linear", False, srcs, weight, bias, resid)
        (Bn, N), C_out = mats[0][0].shape[:2], W.shape[0]
        nv = self._dnet_counts(n_verts, Bn)
        out, ldo = self._dnet_out(out, Bn, N, C_out, "dnet_linear")
        a = self._dnet_src_args(mats, False)
        self._chk(self.lib.dm_dnet_linear_f32(self.ctx, Bn, N, C_out, len(mats), *a[0], *a[1], *a[2], _ptr(W), ldw, _ptr(bias), _ptr(R), ldr,
                                              1 if relu else 0, _ptr(nv), _ptr(out), ldo))
        return out[0] if flat else out

    def dnet_diffuse(self, x, mass, evals, evecs, times, n_verts=None, out=None):
        """evecs (exp(-evals max(times, 1e-8)) * (evecs^T (mass * x))) (dm_dnet_diffuse_f32): x (B,N,C), mass (B,N), evals (B,K),
        evecs (B,N,K), times (C); the spectrum stays on chip."""
        X, ldx = self._strided(x, torch.float32, "x")
        E, lde = self._strided(evecs, torch.float32, "evecs")
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
        return self._dnet_gradient_features("dnet_gradient_features", False, x, row_len, cols, gx, gy, A_re, A_im, n_verts, out)

    # ------------------------------------------------------------- DiffusionNet backward (dm_dnet_*_bwd_f32)
    def dnet_linear_backward(self, grad_out, srcs, weight, y=None, n_verts=None, need_src=True, need_weight=True, need_bias=True, out=None):
        """The gradients of dnet_linear (dm_dnet_linear_bwd_data_f32, dm_dnet_linear_bwd_weight_f32).  grad_out (B, N, C_out); srcs the
        forward's sources; weight (C_out, sum w_s); y: the saved output of a relu=True call made WITHOUT resid (its mask y > 0 is
        applied to grad_out), None for relu=False.  The gradient of resid is grad_out itself.  need_src: one flag, or one per source;
        out: a list with a (B, N, w_s) tensor or None per source.  Only the weight and bias gradients read the sources: without
        them a source may be given as its width (an int).
        Returns (list of source gradients or None each, grad_weight or None, grad_bias or None)."""
        return self._dnet_linear_backward("dnet_linear_backward", False, grad_out, srcs, weight, y, n_verts, need_src, need_weight, need_bias, out)

    def dnet_diffuse_backward(self, grad_out, x, mass, evals, evecs, times, n_verts=None, need_x=True, need_times=True, out=None):
        """The gradients of dnet_diffuse (dm_dnet_diffuse_bwd_f32) with respect to x and to the clamped times: grad_out, x (B,N,C) (x
        may be None with need_times=False), the operators as in dnet_diffuse.  Returns (grad_x or None, grad_times or None)."""
        G, ldg = self._strided(grad_out, torch.float32, "grad_out")
        E, lde = self._strided(evecs, torch.float32, "evecs")
        Bn, N, Cw = G.shape
        K = E.shape[2]
        X, ldx = (None, 0)
        if need_times:
            X, ldx = self._strided(x, torch.float32, "x")
            if tuple(X.shape) != (Bn, N, Cw):
                raise ValueError("dnet_diffuse_backward: x must have the shape of grad_out")
        mass = self._dev(mass, torch.float32, "mass")
        evals = self._dev(evals, torch.float32, "evals")
        times = self._dev(times, torch.float32, "times")
        if tuple(E.shape[:2]) != (Bn, N) or tuple(mass.shape) != (Bn, N) or tuple(evals.shape) != (Bn, K) or tuple(times.shape) != (Cw,):
            raise ValueError("dnet_diffuse_backward: grad_out (B,N,C), mass (B,N), evals (B,K), evecs (B,N,K), times (C)")
        nv = self._dnet_counts(n_verts, Bn)
        dx, lddx = self._dnet_out(out, Bn, N, Cw, "dnet_diffuse_backward") if need_x else (None, 0)
        dt = torch.empty((Cw,), dtype=torch.float32, device=self.device) if need_times else None
        ws = self._dnet_ws(self.lib.dm_dnet_diffuse_bwd_bytes(Bn, K, Cw))
        self._chk(self.lib.dm_dnet_diffuse_bwd_f32(self.ctx, Bn, N, K, Cw, _ptr(G), ldg, _ptr(X), ldx, _ptr(mass), _ptr(evals), _ptr(E), lde, _ptr(times),
                                                   _ptr(nv), _ptr(ws), _ptr(dx), lddx, _ptr(dt)))
        return dx, dt

    def dnet_gradient_features_backward(self, grad_out, x, row_len, cols, gx, gy, rows_t, A_re, A_im=None, n_verts=None, need_x=True, need_A=True,
                                        out=None):
        """The gradients of dnet_gradient_features (dm_dnet_gradfeat_bwd_f32): grad_out and the saved x (B,N,C), the forward's rows,
        rows_t = (row_len_t, cols_t, gx_t, gy_t), the rows of the transposed operators (PackedOperators.transposed_rows(); None with
        need_x=False).  Returns (grad_x or None, grad_A_re or None, grad_A_im or None)."""
        return self._dnet_gradient_features_backward("dnet_gradient_features_backward", False, grad_out, x, row_len, cols, gx, gy, rows_t, A_re, A_im,
                                                     n_verts, need_x, need_A, out)

    # ------------------------------------------------------------- DiffusionNet backward, fp16 operands (dm_dnet_*_bwd_f16)
    def dnet_linear_backward_f16(self, grad_out, srcs, weight_h, y=None, n_verts=None, need_src=True, need_weight=True, need_bias=True, out=None):
        """dnet_linear_backward on fp16 operands (dm_dnet_linear_bwd_data_f16, dm_dnet_linear_bwd_weight_f16): grad_out and y float32;
        weight_h (C_out, sum w_s) float16, the rounded matrix the forward multiplied; every source float16 or float32 in its own dtype
        (float32 elements are rounded as they are staged).  The gradients are float32; grad_weight belongs to the float32 master of
        weight_h.  Arguments and the returned triple as dnet_linear_backward."""
        return self._dnet_linear_backward("dnet_linear_backward_f16", True, grad_out, srcs, weight_h, y, n_verts, need_src, need_weight, need_bias, out)

    def dnet_diffuse_backward_f16(self, grad_out, x, evecs_h, mevecs_h, e1, e2, evals, times, n_verts=None, need_x=True, need_times=True, out=None):
        """The gradients of dnet_diffuse_f16 (dm_dnet_diffuse_bwd_f16) with respect to x and to the clamped times: grad_out, x (B,N,C)
        float32 (x may be None with need_times=False), the operands as in dnet_diffuse_f16, times float32.  grad_x is dnet_diffuse_f16
        of grad_out with the two matrix operands exchanged.  Returns (grad_x or None, grad_times or None), float32."""
        G, ldg = self._strided(grad_out, torch.float32, "grad_out")
        E, lde = self._strided(evecs_h, torch.float16, "evecs_h")
        M, ldm = self._strided(mevecs_h, torch.float16, "mevecs_h")
        Bn, N, Cw = G.shape
        K = E.shape[2]
        X, ldx = (None, 0)
        if need_times:
            X, ldx = self._strided(x, torch.float32, "x")
            if tuple(X.shape) != (Bn, N, Cw):
                raise ValueError("dnet_diffuse_backward_f16: x must have the shape of grad_out")
        evals = self._dev(evals, torch.float32, "evals")
        times = self._dev(times, torch.float32, "times")
        e1, e2 = self._dev(e1, torch.int32, "e1"), self._dev(e2, torch.int32, "e2")
        if (tuple(E.shape[:2]) != (Bn, N) or M.shape != E.shape or tuple(evals.shape) != (Bn, K) or tuple(times.shape) != (Cw,)
                or tuple(e1.shape) != (Bn,) or tuple(e2.shape) != (Bn,)):
            raise ValueError("dnet_diffuse_backward_f16: grad_out (B,N,C), evecs_h / mevecs_h (B,N,K), e1 / e2 (B), evals (B,K), times (C)")
        nv = self._dnet_counts(n_verts, Bn)
        dx, lddx = self._dnet_out(out, Bn, N, Cw, "dnet_diffuse_backward_f16") if need_x else (None, 0)
        dt = torch.empty((Cw,), dtype=torch.float32, device=self.device) if need_times else None
        ws = self._dnet_ws(self.lib.dm_dnet_diffuse_bwd_f16_bytes(Bn, K, Cw))
        self._chk(self.lib.dm_dnet_diffuse_bwd_f16(self.ctx, Bn, N, K, Cw, _ptr(G), ldg, _ptr(X), ldx, _ptr(E), lde, _ptr(M), ldm, _ptr(e1), _ptr(e2),
                                                   _ptr(evals), _ptr(times), _ptr(nv), _ptr(ws), _ptr(dx), lddx, _ptr(dt)))
        return dx, dt

    def dnet_gradient_features_backward_f16(self, grad_out, x, row_len, cols, gx, gy, rows_t, A_re_h, A_im_h=None, n_verts=None, need_x=True,
                                            need_A=True, out=None):
        """The gradients of dnet_gradient_features_f16 (dm_dnet_gradfeat_bwd_f16): A_re_h / A_im_h float16, the rounded matrices the forward
        multiplied; everything else as dnet_gradient_features_backward.  Returns (grad_x or None, grad_A_re or None, grad_A_im or None),
        float32; the matrix gradients belong to the float32 masters."""
        return self._dnet_gradient_features_backward("dnet_gradient_features_backward_f16", True, grad_out, x, row_len, cols, gx, gy, rows_t, A_re_h,
                                                     A_im_h, n_verts, need_x, need_A, out)

    # ------------------------------------------------------------- DiffusionNet forward, fp16 operands (dm_dnet_*_f16)
    def dnet_linear_f16(self, srcs, weight, bias=None, resid=None, relu=False, n_verts=None, out=None, out_dtype=torch.float32):
        """dnet_linear on fp16 operands (dm_dnet_linear_f16): every source float16 or float32 in its own dtype (float32 elements are
        rounded as they are staged), weight (C_out, sum w_s) float16 read where it lies, bias float16 or float32, resid float32;
        fp32 accumulation, + bias, act, + resid; out float32 or float16 (out_dtype, or the dtype of out)."""
        flat, mats, W, ldw, bias, R, ldr = self._dnet_linear_operands("dnet_linear_f16", True, srcs, weight, bias, resid)
        (Bn, N), C_out = mats[0][0].shape[:2], W.shape[0]
        nv = self._dnet_counts(n_verts, Bn)
        out_dtype = out_dtype if out is None else out.dtype
        if out_dtype not in _HALF_OR_SINGLE:
            raise ValueError("dnet_linear_f16: the output is float32 or float16")
        out, ldo = self._dnet_out(out, Bn, N, C_out, "dnet_linear_f16", out_dtype)
        a = self._dnet_src_args(mats, True)
        self._chk(self.lib.dm_dnet_linear_f16(self.ctx, Bn, N, C_out, len(mats), *a[0], *a[1], *a[2], _ptr(W), ldw, _ptr(bias),
                                              _lib.DM_F32 if bias is None else _flag(bias), _ptr(R), ldr, 1 if relu else 0, _ptr(nv), _flag(out),
                                              _ptr(out), ldo))
        return out[0] if flat else out

    def dnet_diffuse_f16(self, x, evecs_h, mevecs_h, e1, e2, evals, times, n_verts=None, out=None):
        """evecs (exp(-evals max(times, 1e-8)) * (evecs^T (mass * x))) on fp16 operands (dm_dnet_diffuse_f16): x (B,N,C) float32;
        evecs_h, mevecs_h (B,N,K) float16 and e1, e2 (B) int32 as PackedOperators.half_operands() returns them; evals (B,K) float32;
        times (C) float16 or float32.  Returns float32."""
        X, ldx = self._strided(x, torch.float32, "x")
        E, lde = self._strided(evecs_h, torch.float16, "evecs_h")
        M, ldm = self._strided(mevecs_h, torch.float16, "mevecs_h")
        Bn, N, Cw = X.shape
        K = E.shape[2]
        evals = self._dev(evals, torch.float32, "evals")
        times = self._dev(times, _kept(times), "times")
        e1, e2 = self._dev(e1, torch.int32, "e1"), self._dev(e2, torch.int32, "e2")
        if (tuple(E.shape[:2]) != (Bn, N) or M.shape != E.shape or tuple(evals.shape) != (Bn, K) or tuple(times.shape) != (Cw,)
                or tuple(e1.shape) != (Bn,) or tuple(e2.shape) != (Bn,)):
            raise ValueError("dnet_diffuse_f16: x (B,N,C), evecs_h / mevecs_h (B,N,K), e1 / e2 (B), evals (B,K), times (C)")
        nv = self._dnet_counts(n_verts, Bn)
        out, ldo = self._dnet_out(out, Bn, N, Cw, "dnet_diffuse_f16")
        self._chk(self.lib.dm_dnet_diffuse_f16(self.ctx, Bn, N, K, Cw, _ptr(X), ldx, _ptr(E), lde, _ptr(M), ldm, _ptr(e1), _ptr(e2), _ptr(evals),
                                               _ptr(times), _flag(times), _ptr(nv), _ptr(out), ldo))
        return out

    def dnet_gradient_features_f16(self, x, row_len, cols, gx, gy, A_re, A_im=None, n_verts=None, out=None):
        """dnet_gradient_features with float16 A_re / A_im (dm_dnet_gradfeat_f16): the gradients come from the float32 rows and the
        float32 x in float32 and are rounded only as operands of the products with the matrices.  Returns float32."""
        return self._dnet_gradient_features("dnet_gradient_features_f16", True, x, row_len, cols, gx, gy, A_re, A_im, n_verts, out)

    def diffusion_net_forward(self, weights, packed, x, out_dtype=None):
        """A whole DiffusionNet (inference) on a padded batch: first_lin, per block diffuse -> gradient features -> the MLP (its first
        layer reads (x, x_diffuse, x_grad) as three sources, its last adds the skip), last_lin.
        weights  {"first": (W, b), "last": (W, b), "blocks": [{"times": t, "A_re": A or None, "A_im": A or None, "mlp": [(W, b), ...]}]},
                 the module's parameters as they lie in memory (A_re None: no gradient features)
        packed   fp32 padded operators with the attributes mass (B,N), evals (B,K), evecs (B,N,K), row_len, cols, gx, gy, n_verts_dev
                 ((B) int32 or None when no mesh is padded) -- diffusion_net.layers.PackedOperators
        x        (B, N, C_in), or up to three tensors read as concatenated along the channels.
        Returns (B, N, C_out); rows behind a mesh's count are zero.  Intermediates live in buffers that the blocks share.
        The dtype of weights["first"][0] picks the kernels: float32 the dm_dnet_*_f32 family, float16 (a module after .half()) the
        dm_dnet_*_f16 family on packed.half_operands(), with float32 intermediates.  out_dtype: float32, or for float16 weights
        float16 (their default, the reference's return dtype: the float32 result rounded once)."""
        nv = packed.n_verts_dev
        W0, b0 = weights["first"]
        half = W0.dtype == torch.float16
        if out_dtype is None:
            out_dtype = torch.float16 if half else torch.float32
        if out_dtype != torch.float32 and not (half and out_dtype == torch.float16):
            raise ValueError("diffusion_net_forward: out_dtype is float32, or float16 with float16 weights")
        if half:
            evecs_h, mevecs_h, e1, e2 = packed.half_operands()
            linear, gradfeat = self.dnet_linear_f16, self.dnet_gradient_features_f16
            diffuse = lambda x, times, out: self.dnet_diffuse_f16(x, evecs_h, mevecs_h, e1, e2, packed.evals, times, n_verts=nv, out=out)
        else:
            linear, gradfeat = self.dnet_linear, self.dnet_gradient_features
            diffuse = lambda x, times, out: self.dnet_diffuse(x, packed.mass, packed.evals, packed.evecs, times, n_verts=nv, out=out)
        cur = linear(x, W0, b0, n_verts=nv)
        Bn, N, Cw = cur.shape
        buf = lambda c=Cw: torch.empty((Bn, N, c), dtype=torch.float32, device=self.device)
        nxt, xd, xg, hidden = buf(), buf(), None, {}
        for blk in weights["blocks"]:
            diffuse(cur, blk["times"], xd)
            src = [cur, xd]
            if blk.get("A_re") is not None:
                xg = buf() if xg is None else xg
                gradfeat(xd, packed.row_len, packed.cols, packed.gx, packed.gy, blk["A_re"], blk.get("A_im"), n_verts=nv, out=xg)
                src.append(xg)
            mlp = blk["mlp"]
            for i, (W, b) in enumerate(mlp):
                if i + 1 == len(mlp):
                    linear(src, W, b, resid=cur, n_verts=nv, out=nxt)
                else:
                    key = (i % 2, W.shape[0])
                    if key not in hidden:
                        hidden[key] = buf(W.shape[0])
                    src = [linear(src, W, b, relu=True, n_verts=nv, out=hidden[key])]
            cur, nxt = nxt, cur
        W1, b1 = weights["last"]
        return linear(cur, W1, b1, n_verts=nv, out_dtype=out_dtype) if half else linear(cur, W1, b1, n_verts=nv)

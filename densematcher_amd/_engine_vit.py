"""
MatchEngine, the DINOv2 ViT encoder behind the `dino` tokens (the reference's SDDINO.py:27, 49-51 through featup's ViTExtractor):
the patch rows (dm_vit_patch_rows_f16), LayerNorm (dm_vit_layernorm_f16), the dense fp16 GEMM with its epilogue (dm_vit_linear_f16),
flash-style attention (dm_vit_attention_f16), and `vit_tokens`, the whole encoder: two launches for the embedding, seven per block.
fp16 operands on the matrix cores, fp32 accumulation, an fp32 residual stream.
"""
import ctypes as C

import torch

from . import _lib
from ._operands import fits_abi, ptr as _ptr

VIT_PATCH, VIT_PATCH_K, VIT_GRANULE, VIT_HEAD_DIM = 14, 588, 64, 64


def vit_pad_k(k):
    """a contraction depth padded to the GEMM's granule"""
    return -(-int(k) // VIT_GRANULE) * VIT_GRANULE


class _VitOps:
    def _vit_half(self, t, name, vec=True):
        """(tensor, ld, block stride) of an fp16 operand (B, M, W) or (M, W), read where it lies when its strides fit the ABI and -- vec:
        the kernel reads it with 16-byte loads -- its address, leading dimension and block stride are multiples of 8 halves"""
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float16:
            t = self._dev(t, torch.float16, name)
        else:
            self._check_stream()
        if t.dim() not in (2, 3):
            raise ValueError(f"{name}: expected a (B, M, W) or (M, W) tensor, got {tuple(t.shape)}")
        ld = None
        if t.dim() == 2:
            ld = fits_abi(t)
            sb = 0
        elif t.stride(2) == 1 or t.shape[2] == 1:
            ld = t.stride(1) if t.shape[1] > 1 else t.shape[2]
            sb = t.stride(0) if t.shape[0] > 1 else 0
            if ld < t.shape[2] or ld >= 2 ** 31 or sb < 0:
                ld = None
        if ld is not None and vec and (t.data_ptr() % 16 or ld % 8 or sb % 8):
            ld = None
        if ld is None:
            t = t.contiguous()
            if vec and t.data_ptr() % 16:                            # contiguous already, but off the 16-byte grid: a fresh block is on it
                t = t.clone()
            ld, sb = int(t.shape[-1]), (int(t.shape[1] * t.shape[2]) if t.dim() == 3 else 0)
        return t, int(ld), int(sb)

    @staticmethod
    def _vit_rows(t, dtype, name, device):
        """(ld, block stride) of an output / residual (B, M, W) or (M, W) that must be used where it lies"""
        if not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype or t.dim() not in (2, 3):
            raise ValueError(f"{name}: expected a {dtype} (B, M, W) or (M, W) tensor on {device}")
        if t.shape[-1] > 1 and t.stride(-1) != 1:
            raise ValueError(f"{name}: the elements of a row must be adjacent")
        ld = t.stride(-2) if t.shape[-2] > 1 else t.shape[-1]
        sb = t.stride(0) if t.dim() == 3 and t.shape[0] > 1 else 0
        if ld < t.shape[-1] or sb < 0:
            raise ValueError(f"{name}: strides {t.stride()} do not describe rows with a leading dimension")
        return int(ld), int(sb)

    def vit_patch_rows(self, images, P, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out=None):
        """dm_vit_patch_rows_f16: images (n, 3, S, S) fp16 | fp32 in any non-negative strides -> (n P P, Kp) fp16 rows, Kp = 588 padded to
        the granule: the image resized (bilinear, align_corners=False) to 14 P, (v - mean_c) / std_c, column 196 c + 14 dy + dx."""
        x = images if isinstance(images, torch.Tensor) else torch.as_tensor(images)
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError(f"vit_patch_rows: images must be (n, 3, S, S), got {tuple(x.shape)}")
        self._check_stream()
        if x.dtype not in (torch.float16, torch.float32):
            x = x.to(torch.float32)
        if x.device != self.device:
            x = x.to(self.device)
        if any(s < 0 for s in x.stride()):
            x = x.contiguous()
        n, S, P = x.shape[0], x.shape[2], int(P)
        Kp = vit_pad_k(VIT_PATCH_K)
        if out is None:
            out = torch.empty((n * P * P, Kp), dtype=torch.float16, device=self.device)
        ldo, _ = self._vit_rows(out, torch.float16, "vit_patch_rows out", self.device)
        if out.dim() != 2 or tuple(out.shape) != (n * P * P, Kp):
            raise ValueError(f"vit_patch_rows: out must be ({n * P * P}, {Kp})")
        m3, s3 = (C.c_double * 3)(*[float(v) for v in mean]), (C.c_double * 3)(*[float(v) for v in std])
        self._chk(self.lib.dm_vit_patch_rows_f16(self.ctx, n, S, P, _lib.DM_F16 if x.dtype == torch.float16 else _lib.DM_F32, _ptr(x), *x.stride(),
                                                 m3, s3, Kp, _ptr(out), ldo))
        return out

    def vit_layernorm(self, x, gamma, beta, out=None, out_dtype=torch.float16):
        """dm_vit_layernorm_f16: x (M, D) or (B, M, D) fp32 rows -> the same shape in fp16 (or fp32): fp64 two-pass statistics, eps 1e-6"""
        X, ldx = self._strided(x, torch.float32, "vit_layernorm x")
        D = X.shape[-1]
        M = X.numel() // D
        gamma, beta = self._dev(gamma, torch.float32, "gamma"), self._dev(beta, torch.float32, "beta")
        if gamma.numel() != D or beta.numel() != D:
            raise ValueError(f"vit_layernorm: gamma and beta must hold {D} values")
        if out is None:
            out = torch.empty(X.shape, dtype=out_dtype, device=self.device)
        if out.dtype not in (torch.float16, torch.float32) or out.shape != X.shape:
            raise ValueError(f"vit_layernorm: out must be fp16 | fp32 of shape {tuple(X.shape)}")
        ldo = fits_abi(out)
        if ldo is None:
            raise ValueError("vit_layernorm: out must be rows with a leading dimension, blocks M ld apart")
        self._chk(self.lib.dm_vit_layernorm_f16(self.ctx, M, D, _ptr(X), ldx, _ptr(gamma), _ptr(beta),
                                                _lib.DM_F16 if out.dtype == torch.float16 else _lib.DM_F32, _ptr(out), ldo))
        return out

    def vit_linear(self, A, W, bias=None, scale=None, resid=None, gelu=False, out=None, out_dtype=torch.float32):
        """dm_vit_linear_f16: out = resid + scale * act(A W^T + bias).  A (M, K) or (B, Mb, K) fp16, W (N, K) fp16, K a multiple of 64;
        bias, scale (N) fp32; resid fp32 of out's shape, or (Mb, N) for a batched A (one block for every image); out fp32 | fp16, given
        or allocated; out may be resid itself."""
        A, lda, sA = self._vit_half(A, "vit_linear A")
        W, ldw, _ = self._vit_half(W, "vit_linear W")
        if W.dim() != 2 or W.shape[1] != A.shape[-1]:
            raise ValueError(f"vit_linear: W must be (N, {A.shape[-1]}), got {tuple(W.shape)}")
        K, N = A.shape[-1], W.shape[0]
        B, Mb = (A.shape[0], A.shape[1]) if A.dim() == 3 else (1, A.shape[0])
        if K % VIT_GRANULE:
            raise ValueError(f"vit_linear: K = {K} must be a multiple of {VIT_GRANULE}")
        bias = None if bias is None else self._dev(bias, torch.float32, "bias")
        scale = None if scale is None else self._dev(scale, torch.float32, "scale")
        if any(v is not None and v.numel() != N for v in (bias, scale)):
            raise ValueError(f"vit_linear: bias and scale must hold {N} values")
        shape = (B, Mb, N) if A.dim() == 3 else (Mb, N)
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=self.device)
        if out.dtype not in (torch.float16, torch.float32) or tuple(out.shape) != shape:
            raise ValueError(f"vit_linear: out must be fp16 | fp32 of shape {shape}")
        ldo, sO = self._vit_rows(out, out.dtype, "vit_linear out", self.device)
        ldr = sR = 0
        if resid is not None:
            if tuple(resid.shape) not in (shape, (Mb, N)):
                raise ValueError(f"vit_linear: resid must be {shape} or ({Mb}, {N})")
            ldr, sR = self._vit_rows(resid, torch.float32, "vit_linear resid", self.device)
        self._chk(self.lib.dm_vit_linear_f16(self.ctx, B, Mb, N, K, _ptr(A), lda, sA, _ptr(W), ldw, _ptr(bias), _ptr(scale), _ptr(resid), ldr, sR,
                                             1 if gelu else 0, _lib.DM_F16 if out.dtype == torch.float16 else _lib.DM_F32, _ptr(out), ldo, sO))
        return out

    def vit_attention(self, qkv, heads, out=None):
        """dm_vit_attention_f16: qkv (n, T, 3 D) fp16, D = 64 heads, q | k | v with the heads adjacent within each -> (n, T, D) fp16,
        softmax(q k^T / 8) v per image and head"""
        if not isinstance(qkv, torch.Tensor) or qkv.dim() != 3:
            raise ValueError("vit_attention: qkv must be (n, T, 3 D)")
        Q, ldq, sq = self._vit_half(qkv, "vit_attention qkv")
        n, T, W3 = Q.shape
        H = int(heads)
        if H <= 0 or W3 != 3 * VIT_HEAD_DIM * H:
            raise ValueError(f"vit_attention: qkv must be (n, T, {3 * VIT_HEAD_DIM} heads): head dimension {VIT_HEAD_DIM} only")
        if out is None:
            out = torch.empty((n, T, VIT_HEAD_DIM * H), dtype=torch.float16, device=self.device)
        if tuple(out.shape) != (n, T, VIT_HEAD_DIM * H):
            raise ValueError(f"vit_attention: out must be ({n}, {T}, {VIT_HEAD_DIM * H})")
        ldo, so = self._vit_rows(out, torch.float16, "vit_attention out", self.device)
        self._chk(self.lib.dm_vit_attention_f16(self.ctx, n, T, H, W3 // (3 * H), _ptr(Q), ldq, sq, _ptr(out), ldo, so))
        return out

    def vit_tokens(self, packed, images, P, layer, norm=False, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        """The output of block `layer` of a DINOv2 encoder on images (n, 3, S, S), resized to 14 P and normalised on the way in: packed
        (featurizers.dinov2.PackedViT), returns (n, 1 + P P, D) fp32 -- the residual stream itself, fp32 throughout; norm: the final
        LayerNorm applied (fp32).  Launches: patch rows, the embedding GEMM (writes rows 1 .. P P of every image's block and adds
        pos_embed[1:]; the constant cls row is copied in), then per block LayerNorm, qkv, attention, proj (+ LayerScale + residual, in
        place), LayerNorm, fc1 (+ GELU), fc2 (+ LayerScale + residual, in place)."""
        n, P = images.shape[0], int(P)
        T, D = 1 + P * P, packed.dim
        if not 0 <= layer < len(packed.blocks):
            raise ValueError(f"vit_tokens: layer {layer} outside the {len(packed.blocks)} blocks")
        pos = packed.pos(P)                                          # (T, D) fp32: row 0 the cls token + pos_embed[0]
        rows = self.vit_patch_rows(images, P, mean, std)
        x = torch.empty((n, T, D), dtype=torch.float32, device=self.device)
        x[:, 0].copy_(pos[0])
        self.vit_linear(rows.view(n, P * P, -1), packed.w_patch, bias=packed.b_patch, resid=pos[1:], out=x[:, 1:])
        h = torch.empty((n, T, D), dtype=torch.float16, device=self.device)
        qkv = torch.empty((n, T, 3 * D), dtype=torch.float16, device=self.device)
        att = torch.empty((n, T, D), dtype=torch.float16, device=self.device)
        mid = torch.empty((n, T, packed.hidden), dtype=torch.float16, device=self.device)
        flat = lambda t: t.view(n * T, t.shape[-1])
        for blk in packed.blocks[:layer + 1]:
            self.vit_layernorm(x, blk.g1, blk.b1, out=h)
            self.vit_linear(flat(h), blk.w_qkv, bias=blk.b_qkv, out=flat(qkv))
            self.vit_attention(qkv, packed.heads, out=att)
            self.vit_linear(flat(att), blk.w_proj, bias=blk.b_proj, scale=blk.ls1, resid=flat(x), out=flat(x))
            self.vit_layernorm(x, blk.g2, blk.b2, out=h)
            self.vit_linear(flat(h), blk.w_fc1, bias=blk.b_fc1, gelu=True, out=flat(mid))
            self.vit_linear(flat(mid), blk.w_fc2, bias=blk.b_fc2, scale=blk.ls2, resid=flat(x), out=flat(x))
        return self.vit_layernorm(x, packed.g_norm, packed.b_norm, out_dtype=torch.float32) if norm else x

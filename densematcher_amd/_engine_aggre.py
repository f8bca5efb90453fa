"""
MatchEngine, the aggregation network behind the 2D backbones (the reference's SDDINO.py:53-90 and AggregationNetwork at inference): the
fused interpolation / rotation / mean / concatenation of the backbones' raw outputs (dm_agg_gather_f32), GroupNorm statistics and
normalisation (dm_groupnorm_stats_f32, dm_groupnorm_relu_f32), the 3 x 3 convolution (dm_conv3x3_f32), the mixture of the bottleneck
blocks (dm_agg_mix_f32), and `aggregate`, the whole network in 17 launches for four levels.  Everything is fp32 on rows = pixels, channels last;
the 1x1 convolutions are dm_dnet_linear_f32 on those rows.
"""
import ctypes as C

import torch

from . import _lib
from ._operands import ptr as _ptr

MAX_SOURCES, MAX_ROTATIONS = 8, 16


class _AggreOps:
    def agg_gather(self, sources, num_rotations=1, step_deg=0.0, size=None):
        """dm_agg_gather_f32: sources, up to 8 tensors (R B, C_s, h_s, w_s) fp16 | fp32 in any strides (read where they lie), image
        r B + b the b-th image turned by r step_deg.  size (P_h, P_w): the patch grid (None: the first source's).  Returns the rows
        (B, P_h P_w, sum C_s) fp32: every source interpolated to the grid, turned back by -r step_deg, averaged over r, side by side."""
        sources = [sources] if isinstance(sources, torch.Tensor) else list(sources)
        if not 1 <= len(sources) <= MAX_SOURCES:
            raise ValueError(f"agg_gather: one to {MAX_SOURCES} sources")
        R = int(num_rotations)
        if not 1 <= R <= MAX_ROTATIONS:
            raise ValueError(f"agg_gather: 1 <= num_rotations <= {MAX_ROTATIONS}")
        self._check_stream()
        srcs = []
        for s in sources:
            s = s if isinstance(s, torch.Tensor) else torch.as_tensor(s)
            if s.dim() != 4:
                raise ValueError(f"agg_gather: a source must be (R B, C, h, w), got {tuple(s.shape)}")
            if s.dtype not in (torch.float16, torch.float32):
                s = s.to(torch.float32)
            if s.device != self.device:
                s = s.to(self.device)
            srcs.append(s)
        n_img = srcs[0].shape[0]
        if n_img % R or any(s.shape[0] != n_img for s in srcs):
            raise ValueError(f"agg_gather: every source needs the same number of images, a multiple of num_rotations = {R}")
        Bn = n_img // R
        P_h, P_w = (int(v) for v in (srcs[0].shape[2:] if size is None else size))
        width = sum(s.shape[1] for s in srcs)
        out = torch.empty((Bn, P_h * P_w, width), dtype=torch.float32, device=self.device)
        desc = (C.c_longlong * (8 * len(srcs)))()
        for i, s in enumerate(srcs):
            desc[8 * i:8 * i + 8] = [s.shape[1], s.shape[2], s.shape[3], *s.stride(), _lib.DM_F16 if s.dtype == torch.float16 else _lib.DM_F32]
        ptrs = [_ptr(s) for s in srcs] + [_ptr(None)] * (MAX_SOURCES - len(srcs))
        self._chk(self.lib.dm_agg_gather_f32(self.ctx, len(srcs), C.cast(desc, C.c_void_p), *ptrs, R, Bn, P_h, P_w, float(step_deg), _ptr(out), width))
        return out

    def _agg_rows(self, x, name):
        """(tensor, ld) of (n_img, npix, C) fp32 rows, read where they lie"""
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError(f"{name}: expected (n_img, npix, C) rows")
        return self._strided(x, torch.float32, name)

    def groupnorm_stats(self, x, num_groups):
        """dm_groupnorm_stats_f32: x (n_img, npix, C) fp32 rows (a column slice is read in place) -> (mean, rstd), each (n_img, G) fp32:
        two float64 passes per (image, group), biased variance, eps 1e-5."""
        X, ld = self._agg_rows(x, "groupnorm_stats")
        n_img, npix, Cw = X.shape
        G = int(num_groups)
        mean = torch.empty((n_img, max(G, 1)), dtype=torch.float32, device=self.device)
        rstd = torch.empty_like(mean)
        self._chk(self.lib.dm_groupnorm_stats_f32(self.ctx, n_img, npix, Cw, G, _ptr(X), ld, _ptr(mean), _ptr(rstd)))
        return mean, rstd

    def groupnorm_relu(self, x, mean, rstd, gamma, beta):
        """dm_groupnorm_relu_f32: relu(fmaf((x - mean) rstd, gamma, beta)); x (L B, npix, C), mean / rstd (L B, G), gamma / beta (L, C):
        image i takes the parameters of level i // B."""
        X, ldx = self._agg_rows(x, "groupnorm_relu")
        n_img, npix, Cw = X.shape
        mean, rstd = self._dev(mean, torch.float32, "mean"), self._dev(rstd, torch.float32, "rstd")
        gamma, beta = self._dev(gamma, torch.float32, "gamma"), self._dev(beta, torch.float32, "beta")
        if mean.dim() != 2 or mean.shape[0] != n_img or rstd.shape != mean.shape:
            raise ValueError(f"groupnorm_relu: mean and rstd must be ({n_img}, G)")
        if gamma.dim() != 2 or gamma.shape[1] != Cw or beta.shape != gamma.shape or n_img % gamma.shape[0]:
            raise ValueError(f"groupnorm_relu: gamma and beta must be (L, {Cw}) with L dividing the {n_img} images")
        out = torch.empty((n_img, npix, Cw), dtype=torch.float32, device=self.device)
        self._chk(self.lib.dm_groupnorm_relu_f32(self.ctx, n_img, n_img // gamma.shape[0], npix, Cw, mean.shape[1], _ptr(X), ldx, _ptr(mean),
                                                 _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(out), Cw))
        return out

    def conv3x3(self, x, weight):
        """dm_conv3x3_f32: x (L, B, P_h, P_w, C_in) fp32 channels-last, weight (L, C_out, 9 C_in) packed with contraction index
        (3 dy + dx) C_in + c -> (L, B, P_h, P_w, C_out); stride 1, zero padding 1."""
        x = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
        if x.dim() != 5:
            raise ValueError(f"conv3x3: x must be (L, B, P_h, P_w, C_in), got {tuple(x.shape)}")
        L, Bn, P_h, P_w, Cin = x.shape
        W = self._dev(weight, torch.float32, "weight")
        if W.dim() != 3 or W.shape[0] != L or W.shape[2] != 9 * Cin:
            raise ValueError(f"conv3x3: weight must be ({L}, C_out, {9 * Cin}), got {tuple(W.shape)}")
        X, ldx = self._strided(x.reshape(L * Bn, P_h * P_w, Cin), torch.float32, "x")
        out = torch.empty((L, Bn, P_h, P_w, W.shape[1]), dtype=torch.float32, device=self.device)
        self._chk(self.lib.dm_conv3x3_f32(self.ctx, L, Bn, P_h, P_w, Cin, W.shape[1], _ptr(X), ldx, _ptr(W), _ptr(out), W.shape[1]))
        return out

    def agg_mix(self, y3, ys, stats3, stats_s, affine3, affine_s, mix, identity=()):
        """dm_agg_mix_f32: out[b, p, c] = sum_l mix[l] relu(GN(y3[l]) + GN(ys[l])); y3, ys (L B, npix, C) fp32 rows (ys may be a column
        slice of a wider buffer), stats (mean, rstd) each (L B, G), affine (gamma, beta) each (L, C), mix (L) -> (B, npix, C).
        identity: the levels without a shortcut convolution, whose ys is the block's input and is added as it is."""
        Y3, ld3 = self._agg_rows(y3, "agg_mix y3")
        Ys, lds = self._agg_rows(ys, "agg_mix ys")
        mix = self._dev(mix, torch.float32, "mix")
        L = mix.numel()
        n_img, npix, Cw = Y3.shape
        if mix.dim() != 1 or L == 0 or n_img % L or Ys.shape != Y3.shape:
            raise ValueError("agg_mix: y3 and ys must be (L B, npix, C) rows for the L mixing weights")
        ops = [self._dev(t, torch.float32, "agg_mix") for t in (*stats3, *affine3, *stats_s, *affine_s)]
        G = ops[0].shape[-1]
        if any(tuple(t.shape) != (n_img, G) for t in (ops[0], ops[1], ops[4], ops[5])) or any(tuple(t.shape) != (L, Cw) for t in (ops[2], ops[3], ops[6], ops[7])):
            raise ValueError(f"agg_mix: statistics must be ({n_img}, G), affine parameters ({L}, {Cw})")
        Bn = n_img // L
        mask = 0
        for l in identity:
            if not 0 <= int(l) < min(L, 32):
                raise ValueError(f"agg_mix: identity level {l} outside the {L} levels (at most 32)")
            mask |= 1 << int(l)
        out = torch.empty((Bn, npix, Cw), dtype=torch.float32, device=self.device)
        self._chk(self.lib.dm_agg_mix_f32(self.ctx, L, Bn, npix, Cw, G, _ptr(Y3), ld3, _ptr(Ys), lds, *[_ptr(t) for t in ops], mask, _ptr(mix), _ptr(out), Cw))
        return out

    def aggregate(self, packed, rows, P_h, P_w):
        """AggregationNetwork.forward at inference on gathered rows: packed (featurizers.modules.projection_network.PackedAggre), rows
        (B, P_h P_w, sum feature_dims) fp32 as agg_gather returns them.  Per level one dm_dnet_linear_f32 feeds conv1 and the shortcut
        (the level's columns of `rows` are read in place; a level with as many channels in as out has no shortcut convolution: its
        columns are copied beside conv1's output and added as they are); then for all levels at once GroupNorm + ReLU, the 3 x 3 convolution,
        GroupNorm + ReLU; one dm_dnet_linear_f32 per level for conv3; the last GroupNorms, the shortcut, ReLU and the mixture in
        dm_agg_mix_f32.  Returns (B, projection_dim, P_h, P_w) fp32, NCHW-shaped over channels-last memory."""
        X, _ = self._agg_rows(rows, "aggregate")
        Bn, npix, width = X.shape
        dims, Cb, Co, G, L = packed.feature_dims, packed.bottleneck, packed.out_channels, packed.groups, len(packed.feature_dims)
        if npix != P_h * P_w or width != sum(dims):
            raise ValueError(f"aggregate: rows must be (B, {P_h * P_w}, {sum(dims)}), got {tuple(X.shape)}")
        y1 = torch.empty((L, Bn, npix, Cb + Co), dtype=torch.float32, device=self.device)
        start = 0
        for l, Cl in enumerate(dims):
            if l in packed.identity:
                self.dnet_linear(X[:, :, start:start + Cl], packed.w1[l], out=y1[l, :, :, :Cb])
                y1[l, :, :, Cb:].copy_(X[:, :, start:start + Cl])
            else:
                self.dnet_linear(X[:, :, start:start + Cl], packed.w1[l], out=y1[l])
            start += Cl
        y1 = y1.view(L * Bn, npix, Cb + Co)
        main, short = y1[:, :, :Cb], y1[:, :, Cb:]
        stats_s = self.groupnorm_stats(short, G)
        a1 = self.groupnorm_relu(main, *self.groupnorm_stats(main, G), packed.g1, packed.b1)
        y2 = self.conv3x3(a1.view(L, Bn, P_h, P_w, Cb), packed.w2).view(L * Bn, npix, Cb)
        a2 = self.groupnorm_relu(y2, *self.groupnorm_stats(y2, G), packed.g2, packed.b2).view(L, Bn, npix, Cb)
        y3 = torch.empty((L, Bn, npix, Co), dtype=torch.float32, device=self.device)
        for l in range(L):
            self.dnet_linear(a2[l], packed.w3[l], out=y3[l])
        y3 = y3.view(L * Bn, npix, Co)
        out = self.agg_mix(y3, short, self.groupnorm_stats(y3, G), stats_s, (packed.g3, packed.b3), (packed.gs, packed.bs), packed.mix, packed.identity)
        return out.view(Bn, P_h, P_w, Co).permute(0, 3, 1, 2)

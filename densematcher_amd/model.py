"""
densematcher.model of the reference: MeshFeaturizer, the module that turns a simplified mesh, its spectral operators and the per-view
2D feature maps into normalised per-vertex descriptors (reference model.py:14-173).  extractor_3d and reconstructor are built as the
reference builds them, so `model.extractor_3d.load_state_dict(...)` of the notebook loads with strict=True.

The SD half of the 2D backbone is outside this package: forward takes the per-view feature maps as fts=
together with the cameras they were rendered with -- or, with an upsampler= (featup.upsamplers.JBUStack, extractor.load_upsampler),
the backbone's low-resolution features fts_lr= and the images= they came from, which it upsamples 16x on the way into lifting; with
an aggre_net= as well (featurizers.AggregationNetwork, extractor.load_aggre_net), the raw outputs of the two frozen backbones raw=
(s3, s4, s5, dino); or a backbone= callable, images (views, 3, H, W) -> (s3, s4, s5, dino), for the views of mesh_raw that render.py
renders here (extractor's module docstring shows one that chains the caller's SD model with this package's DINOv2 encoder,
featurizers.dino_features).  From there on -- back-projection (projection.get_features_per_vertex), positional encoding, heat kernel signatures, DiffusionNet, the row normalisation -- everything runs here, on the device with
route="device" (or "auto", see projection.AUTO_DEVICE and diffusion_net.layers.AUTO_DEVICE).
"""
import numpy as np
import torch
from torch import nn

from . import _routes, diffusion_net
from .diffusion_net.layers import PackedOperators
from .projection import get_features_per_vertex, lift_features_many, mesh_arrays

NORM_FLOOR = 1e-5


def _reconstructor(layers, width, num_features, num_blocks):
    """the head that maps the 3D features back to the 2D ones: layers = 1 one Linear, layers > 1 that many Linears with ReLU between
    them (an nn.Sequential: the checkpoint's keys are its positions), layers = -1 a second DiffusionNet of the same depth"""
    if layers == -1:
        return diffusion_net.layers.DiffusionNet(C_in=width, C_out=num_features, C_width=width, N_block=num_blocks, dropout=True)
    if layers == 1:
        return nn.Linear(width, num_features)
    hidden = [m for _ in range(layers - 1) for m in (nn.Linear(width, width), nn.ReLU())]
    return nn.Sequential(*hidden, nn.Linear(width, num_features))


class MeshFeaturizer(nn.Module):
    def __init__(self, pretrained_upsampler_path=None, num_views=(3, 1), num_blocks=8, width=512, aggre_net_weights_folder=None,
                 reconstructor_layers=1, num_encoding_functions=8, num_hks=16, *, num_features=768, extractor_2d=None, upsampler=None,
                 use_unitnorm=False, use_channelnorm=False, aggre_net=None, rot_inv=False, num_rotations=4):
        """num_views: (num_azimuth, num_elevation) of the reference's camera placement; kept, the cameras come with every call.
        pretrained_upsampler_path / aggre_net_weights_folder: kept for the reference's call signature, nothing is loaded from them.
        extractor_2d: an optional 2D feature extractor (num_patches, featurizer.num_features); without one the width of the maps is
        num_features and forward needs fts=, or fts_lr= and images= when an upsampler is given.
        upsampler: an optional JBUStack (a submodule: its parameters move and save with the model, under `upsampler.*`);
        use_unitnorm / use_channelnorm: the normalisations of the low-resolution features in front of it (extractor.upsample_features).
        aggre_net: an optional AggregationNetwork (a submodule, under `aggre_net.*`) for raw= calls; rot_inv / num_rotations: whether the
        raw outputs hold num_rotations rotated copies per view (extractor.features_from_backbone)."""
        super().__init__()
        self.upsampler = upsampler
        self.aggre_net = aggre_net
        self.rot_inv, self.num_rotations = rot_inv, num_rotations
        self.use_unitnorm, self.use_channelnorm = use_unitnorm, use_channelnorm
        self.pretrained_upsampler_path = pretrained_upsampler_path
        self.extractor_2d = extractor_2d
        if extractor_2d is not None:
            num_features = extractor_2d.featurizer.num_features
            self.H = self.W = extractor_2d.num_patches * 16
        else:
            self.H = self.W = None          # taken from the maps of a call
        self.num_features = num_features
        self.num_views = num_views
        self.reconstructor_layers = reconstructor_layers
        self.num_encoding_functions = num_encoding_functions
        self.num_hks = num_hks
        self.pos_enc_size = 3 * (2 * num_encoding_functions + 1)
        self.diffusion_in_channels = num_features + self.num_hks + self.pos_enc_size
        self.extractor_3d = diffusion_net.layers.DiffusionNet(C_in=self.diffusion_in_channels, C_out=width, C_width=width, N_block=num_blocks,
                                                              dropout=True)
        self.reconstructor = _reconstructor(reconstructor_layers, width, num_features, num_blocks)
        self.use_lr_features = False

    @property
    def device(self):
        return next(self.parameters()).device

    def positional_encoding(self, tensor, include_input=True, log_sampling=True):
        """[..., d] -> [..., d (2 n + 1)], n = num_encoding_functions: the input (include_input), then per frequency band sin and cos of
        the input times the band; the bands are 2^0 .. 2^(n-1) (log_sampling) or n values spaced evenly between those two"""
        n, d = self.num_encoding_functions, tensor.shape[-1]
        if log_sampling:
            bands = torch.exp2(torch.arange(n, dtype=tensor.dtype, device=tensor.device))
        else:
            bands = torch.linspace(1.0, 2.0 ** (n - 1), n, dtype=tensor.dtype, device=tensor.device)
        phase = tensor.unsqueeze(-2) * bands.unsqueeze(-1)                                   # (..., n, d)
        waves = torch.stack((torch.sin(phase), torch.cos(phase)), dim=-2)                   # (..., n, 2, d): band, then sin | cos
        waves = waves.reshape(tensor.shape[:-1] + (2 * n * d,))
        return torch.cat((tensor, waves), dim=-1) if include_input else waves

    # ------------------------------------------------------------------ the neck
    def _neck(self, verts, evals, evecs):
        """(pos_enc (V, 51), hks (V, 16)) of a mesh: model.py:155,158"""
        pos_enc = self.positional_encoding(verts * np.pi * 6)
        hks = diffusion_net.geometry.compute_hks_autoscale(evals.contiguous(), evecs.contiguous(), self.num_hks)
        return pos_enc, hks

    @staticmethod
    def _normalize(out_features):
        return out_features / out_features.norm(dim=-1, keepdim=True).clamp(min=NORM_FLOOR)

    def _verts(self, mesh_simp):
        verts = mesh_arrays(mesh_simp)[0]
        verts = verts if isinstance(verts, torch.Tensor) else torch.as_tensor(np.asarray(verts))
        return verts.to(device=self.device, dtype=torch.float32)

    def _need_maps(self, fts):
        if fts is None and self.extractor_2d is None:
            raise ValueError("MeshFeaturizer was built without extractor_2d: pass the per-view feature maps as fts= (or, with an "
                             "upsampler, the low-resolution features and their images as fts_lr= and images=)")

    def _maps(self, fts, fts_lr, images, route, raw=None):
        """the per-view maps of a mesh: fts as given, else fts_lr (views, C, h, w) upsampled under images (views, 3, H, W), else raw
        (s3, s4, s5, dino) through the aggregation network and the upsampler"""
        if fts is None and fts_lr is None and raw is not None:
            if self.aggre_net is None or self.upsampler is None or images is None:
                raise ValueError("raw= needs a MeshFeaturizer built with aggre_net= and upsampler= and the images the features came from as images=")
            from .extractor import features_from_backbone
            with torch.no_grad():
                return features_from_backbone(self.aggre_net, self.upsampler, *[t.to(self.device) for t in raw], images.to(self.device),
                                              self.num_rotations, self.rot_inv, self.use_unitnorm, self.use_channelnorm,
                                              route=_routes.torch_route(route))
        if fts is not None or fts_lr is None:
            return fts
        if self.upsampler is None or images is None:
            raise ValueError("fts_lr= needs a MeshFeaturizer built with upsampler= and the images the features came from as images=")
        from .extractor import upsample_features
        with torch.no_grad():
            return upsample_features(self.upsampler, fts_lr.to(self.device), images.to(self.device), self.use_unitnorm, self.use_channelnorm,
                                     route=_routes.torch_route(route))

    def _render_views(self, meshes_raw, cameras_list, route, image_size):
        """the views of the raw meshes for a backbone: per mesh the RGB planes (views, 3, H, W) fp32 and the cameras (R, T) they were
        rendered with (generated from num_views around the origin where None, as the reference's get_features_per_vertex does)"""
        from .render import render_many
        size = int(image_size or self.H or 512)
        outs = render_many(self.device, meshes_raw, self.num_views, size, size, cameras_list, [torch.zeros((1, 3))] * len(meshes_raw), route=route,
                           planes=torch.float32)
        return [o[5] for o in outs], [(o[1].R, o[1].T) for o in outs]

    def forward(self, mesh_raw, mesh_simp, operators, cameras, return_mvfeatures=False, *, fts=None, pix2face=None, route="auto", fts_lr=None,
                images=None, raw=None, backbone=None, image_size=None, differentiable=False, compute_dtype=None):
        """mesh_simp: the simplified mesh (verts_list()[0] / faces_list()[0], or a (verts, faces) pair); mesh_raw is the rendering half's
        and is not read.  operators: the tuple of get_operators (frames, massvec, L, evals, evecs, gradX, gradY), or a PackedOperators of
        this one mesh.  cameras (R, T): the cameras the maps fts (views, C, H, W) were rendered with; pix2face: optional, another
        rasteriser's.  route: 'host' (CPU raster, torch expressions), 'device' (HIP), 'auto'.  Without fts: fts_lr (views, C, h, w) and
        images (views, 3, H, W) go through the upsampler (same route) and its maps straight into lifting; or raw = (s3, s4, s5, dino), the
        backbones' outputs for those images, through the aggregation network first.  With none of fts / fts_lr / raw and a backbone=
        (images (views, 3, H, W) -> (s3, s4, s5, dino)): mesh_raw (verts_list / faces_list, optional .textures) is rendered with
        `cameras` (generated from num_views when None) at image_size (default: the extractor's size, else 512), the images go to the
        backbone and the result takes the raw= route with images=.
        differentiable: passed to extractor_3d (DiffusionNet.forward): with route='device' the refiner records its autograd graph
        through the backward kernels, so a training step stays on the device route.  compute_dtype: passed along with it; torch.float16
        selects the mixed-precision kernels (float32 master parameters, fp16 matrix operands; use torch.amp.GradScaler as with autocast).
        Returns the row-normalised features (V, width); with return_mvfeatures also the unnormalised ones and the (V, C) multi-view features."""
        _routes.check(route, _routes.HOST)
        if fts is None and fts_lr is None and raw is None and backbone is not None:
            with torch.no_grad():
                (images,), (cameras,) = self._render_views([mesh_raw], [cameras], route, image_size)
                raw = backbone(images)
        fts = self._maps(fts, fts_lr, images, route, raw)
        self._need_maps(fts)
        size = {} if self.H is None else {"H": self.H, "W": self.W}
        if fts is not None:
            size = {"H": fts.shape[2], "W": fts.shape[3]}
        with torch.no_grad():
            lifted = get_features_per_vertex(self.device, self.extractor_2d, mesh_raw, mesh_simp, self.num_views, ft_dim=self.num_features,
                                             cameras=cameras, fts=fts, use_lr_features=self.use_lr_features, pix2face=pix2face, route=route, **size)
        verts = self._verts(mesh_simp)
        net_route = _routes.torch_route(route)
        if isinstance(operators, PackedOperators):
            if len(operators.n_verts) != 1:
                raise ValueError("forward takes one mesh: a PackedOperators of several meshes goes to forward_many")
            packed = operators.to(self.device) if operators.device != self.device else operators
            sources = (lifted,) + self._neck(verts, packed.evals[0], packed.evecs[0, :verts.shape[0]])
            raw = self.extractor_3d(sources, route=net_route, operators=packed, differentiable=differentiable, compute_dtype=compute_dtype)
        else:
            ops = [None if op is None else op.to(self.device) for op in operators]       # frames, mass, L, evals, evecs, gradX, gradY
            sources = (lifted,) + self._neck(verts, ops[3], ops[4])
            raw = self.extractor_3d(sources, ops[1], ops[2], ops[3], ops[4], ops[5], ops[6], route=net_route, differentiable=differentiable,
                                    compute_dtype=compute_dtype)
        unit = self._normalize(raw)
        return (unit, raw, lifted) if return_mvfeatures else unit

    def forward_many(self, meshes_raw, meshes_simp, packed, cameras_list, return_mvfeatures=False, *, fts_list=None, pix2face_list=None,
                     fts_lr=None, images=None, raw=None, backbone=None, image_size=None, differentiable=False, compute_dtype=None):
        """forward for a ragged list of meshes on the device: ONE batched lifting call and ONE batched DiffusionNet call.  packed: the
        PackedOperators of the same meshes (diffusion_net.layers.pack_operators).  Returns the list of what forward returns per mesh.
        Without fts_list: fts_lr / images, lists of (views_b, C, h, w) and (views_b, 3, H, W), go through the upsampler on the device; or raw, a list of (s3, s4, s5, dino) per mesh, through the aggregation network first;
        or backbone=, as in forward: the raw meshes are rendered in ONE device call (cameras_list entries may be None).
        differentiable, compute_dtype: passed to extractor_3d.forward_many, as in forward."""
        if fts_list is None and fts_lr is None and raw is None and backbone is not None:
            with torch.no_grad():
                images, cameras_list = self._render_views(list(meshes_raw), list(cameras_list), "device", image_size)
                raw = [backbone(i) for i in images]
        if fts_list is None and fts_lr is None and raw is not None:
            if images is None or len(raw) != len(meshes_simp) or len(images) != len(meshes_simp):
                raise ValueError("forward_many: raw= and images= are lists with one entry per mesh")
            fts_list = [self._maps(None, None, i, "device", r) for r, i in zip(raw, images)]
        if fts_list is None and fts_lr is not None:
            if images is None or len(fts_lr) != len(meshes_simp) or len(images) != len(meshes_simp):
                raise ValueError("forward_many: fts_lr= and images= are lists with one entry per mesh")
            fts_list = [self._maps(None, f, i, "device") for f, i in zip(fts_lr, images)]
        if fts_list is None:
            self._need_maps(None)
            raise NotImplementedError("rendering and the 2D backbone are outside this package: pass the per-view feature maps as fts_list=")
        if not isinstance(packed, PackedOperators) or len(packed.n_verts) != len(meshes_simp):
            raise ValueError("forward_many: packed must be the PackedOperators of the same meshes")
        packed = packed.to(self.device) if packed.device != self.device else packed
        with torch.no_grad():
            mv = lift_features_many(fts_list, meshes_simp, cameras_list, pix2face_list, route="device", device=self.device)
        xs = []
        for b, mesh in enumerate(meshes_simp):
            verts = self._verts(mesh)
            if verts.shape[0] != packed.n_verts[b]:
                raise ValueError(f"forward_many: mesh {b} has {verts.shape[0]} vertices, its packed operators {packed.n_verts[b]}")
            xs.append((mv[b],) + self._neck(verts, packed.evals[b], packed.evecs[b, :verts.shape[0]]))
        outs = self.extractor_3d.forward_many(xs, packed, differentiable=differentiable, compute_dtype=compute_dtype)
        if return_mvfeatures:
            return [(self._normalize(o), o, m) for o, m in zip(outs, mv)]
        return [self._normalize(o) for o in outs]

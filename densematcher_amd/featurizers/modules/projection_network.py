"""
densematcher.featurizers.modules.projection_network of the reference: AggregationNetwork, the trained network between the concatenated
backbone features and features_lr -- one bottleneck block per feature level, their outputs mixed by softmax weights.  Constructor
arguments, parameters and state_dict keys are the reference's: a state dict of the reference class loads with strict=True (the released
best_<size>.PTH through load_pretrained_weights, as the reference loads it).

Routes (forward(..., route=)):
  torch    the reference's expressions on PyTorch, any device: training, autograd, dropout.
  device   inference in HIP on rows = pixels (MatchEngine.agg_gather lays the NCHW input out as rows, MatchEngine.aggregate runs the
           network: dm_dnet_linear_f32, dm_groupnorm_*_f32, dm_conv3x3_f32, dm_agg_mix_f32).  Refused with ValueError in training mode,
           when a gradient is required, and for a network the kernels are not built for (kernels other than 1, 3, 1; several
           timesteps); RuntimeError without a GPU.  A level whose in_channels == out_channels has no shortcut convolution -- the DINO
           level of the released network, 768 in and out -- and adds its input as it is, on both routes.
  auto     the device route where its conditions hold and tools/aggre_time.py measured it faster (AUTO_DEVICE), else torch.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ... import _routes
from .resnet import BottleneckBlock, ResNet

# whether tools/aggre_time.py measured the device route faster than the torch route of the same process on an MI355X (README.md,
# DESIGN.md section 4): 1.08 ms against 29.8 ms (5 views, 4 rotations, 24 x 24 patches, the released dims, projection 768, fp16 sources)
AUTO_DEVICE = True


def route_of(module, route, tensors):
    """'torch' or 'device' for a call of `module` (an AggregationNetwork) on `tensors`: what it hands to the one picker"""
    operands = lambda: list(tensors) + list(module.parameters())
    return _routes.pick_torch(route, "AggregationNetwork", lambda: module.device_obstacle() or _routes.grad_obstacle(operands()), AUTO_DEVICE,
                              lambda: all(t.is_cuda for t in operands()))


class PackedAggre:
    """what MatchEngine.aggregate reads of an AggregationNetwork, fp32 on the device: w1[l] (C_b + C_o, C_l) conv1 over shortcut (conv1
    alone, (C_b, C_l), for the levels in `identity`, which have no shortcut convolution; their rows of gs / bs are not read), w2
    (L, C_b, 9 C_b) with contraction index (3 dy + dx) C_b + c, w3 (L, C_o, C_b), the affine parameters of the four GroupNorms as
    (L, C) and mix, the softmax of the mixing weights"""

    def __init__(self, feature_dims, bottleneck, out_channels, groups, **tensors):
        self.feature_dims, self.bottleneck, self.out_channels, self.groups = tuple(feature_dims), bottleneck, out_channels, groups
        self.__dict__.update(tensors)


class AggregationNetwork(nn.Module):
    def __init__(self, feature_dims=(640, 1280, 1280, 768), projection_dim=384, num_norm_groups=32, save_timestep=(1,), kernel_size=(1, 3, 1),
                 contrastive_temp=10, feat_map_dropout=0.0):
        super().__init__()
        self.skip_connection = True
        self.feat_map_dropout = feat_map_dropout
        self.azimuth_embedding = None
        self.pos_embedding = None
        self.feature_dims = list(feature_dims)
        self.projection_dim, self.num_norm_groups, self.kernel_size = projection_dim, num_norm_groups, tuple(kernel_size)
        self.save_timestep = list(save_timestep)
        # the temperatures of the contrastive losses the network is trained with
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.self_logit_scale = nn.Parameter(torch.ones([]) * np.log(contrastive_temp))
        self.bottleneck_layers = nn.ModuleList()
        self.mixing_weights_names = []
        for l, dim in enumerate(self.feature_dims):
            self.bottleneck_layers.append(nn.Sequential(*ResNet.make_stage(
                BottleneckBlock, num_blocks=1, in_channels=dim, bottleneck_channels=projection_dim // 4, out_channels=projection_dim, norm="GN",
                num_norm_groups=num_norm_groups, kernel_size=self.kernel_size)))
            self.mixing_weights_names += [f"timestep-{self.save_timestep}_layer-{l + 1}" for _ in self.save_timestep]
        self.last_layer = None
        self.mixing_weights = nn.Parameter(torch.ones(len(self.bottleneck_layers) * len(self.save_timestep)))
        self._packed = None

    def load_pretrained_weights(self, pretrained_dict):
        """the reference's rule: the first four mixing weights are copied (a fifth, where this network has one and the checkpoint's
        shape differs, starts at zero), every other key this network has is taken, the rest ignored"""
        own = self.state_dict()
        theirs = pretrained_dict.get("mixing_weights")
        if theirs is not None:
            theirs = torch.as_tensor(theirs)
            own["mixing_weights"][:4] = theirs[:4]
            if own["mixing_weights"].shape != theirs.shape and own["mixing_weights"].numel() > 4:
                own["mixing_weights"][4] = 0
        own.update({k: torch.as_tensor(v) for k, v in pretrained_dict.items() if k in own and k != "mixing_weights"})
        self.load_state_dict(own, strict=False)

    # ------------------------------------------------------------------ torch route
    def _forward_torch(self, batch):
        if self.feat_map_dropout > 0 and self.training:
            batch = F.dropout(batch, p=self.feat_map_dropout)
        mix = F.softmax(self.mixing_weights, dim=0)
        if self.pos_embedding is not None:
            batch = torch.cat((batch, self.pos_embedding), dim=1)
        out, start, n = None, 0, len(self.feature_dims)
        for i in range(len(mix)):                                  # (the blocks are shared across timesteps)
            end = start + self.feature_dims[i % n]
            term = mix[i] * self.bottleneck_layers[i % n](batch[:, start:end])
            start = end
            if out is None:
                out = term
            else:
                out += term
        if self.last_layer is not None:
            after = self.last_layer(out)
            if self.skip_connection:
                out = out + after
        return out

    # ------------------------------------------------------------------ device route
    def device_obstacle(self):
        """why the device route cannot run this network, or None"""
        if self.training:
            return "the module is in training mode (the device route is inference only: call .eval())"
        if self.kernel_size != (1, 3, 1) or len(self.save_timestep) != 1 or self.last_layer is not None or self.pos_embedding is not None:
            return "the device route is built for kernels (1, 3, 1), one timestep, no last layer and no position embedding"
        if len(self.bottleneck_layers) > 32:
            return "the device route mixes at most 32 levels"
        if any(m.eps != 1e-5 for m in self.modules() if isinstance(m, nn.GroupNorm)):
            return "the device route is built for GroupNorm's eps = 1e-5"
        return None

    def packed(self, device):
        """the device-side weight blocks (PackedAggre) on `device`, rebuilt when a parameter changed"""
        why = self.device_obstacle()
        if why is not None:
            raise ValueError(f"AggregationNetwork.packed: {why}")
        stamp = (torch.device(device),) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed is None or self._packed[0] != stamp:
            with torch.no_grad():
                f = lambda t: t.detach().to(device=device, dtype=torch.float32)
                blocks = [layer[0] for layer in self.bottleneck_layers]
                Cb, Co = self.projection_dim // 4, self.projection_dim
                stack = lambda get: torch.stack([f(get(b)) for b in blocks]).contiguous()
                tensors = dict(
                    w1=[torch.cat([f(b.conv1.weight).reshape(Cb, -1)] + ([] if b.shortcut is None else [f(b.shortcut.weight).reshape(Co, -1)])).contiguous()
                        for b in blocks],
                    w2=stack(lambda b: b.conv2.weight.permute(0, 2, 3, 1).reshape(Cb, 9 * Cb)),
                    w3=stack(lambda b: b.conv3.weight.reshape(Co, Cb)),
                    g1=stack(lambda b: b.conv1.norm.weight), b1=stack(lambda b: b.conv1.norm.bias),
                    g2=stack(lambda b: b.conv2.norm.weight), b2=stack(lambda b: b.conv2.norm.bias),
                    g3=stack(lambda b: b.conv3.norm.weight), b3=stack(lambda b: b.conv3.norm.bias),
                    gs=stack(lambda b: b.conv3.norm.weight if b.shortcut is None else b.shortcut.norm.weight),
                    bs=stack(lambda b: b.conv3.norm.bias if b.shortcut is None else b.shortcut.norm.bias),
                    identity=tuple(l for l, b in enumerate(blocks) if b.shortcut is None),
                    mix=F.softmax(f(self.mixing_weights), dim=0).contiguous())
            self._packed = (stamp, PackedAggre(self.feature_dims, Cb, Co, self.num_norm_groups, **tensors))
        return self._packed[1]

    def forward(self, batch, pose=None, route="auto"):
        """batch (B, sum feature_dims, H, W): the levels' features side by side -> (B, projection_dim, H, W); on the device route
        NCHW-shaped over channels-last memory.  pose is not read (the reference's signature)."""
        if route_of(self, route, (batch,)) == "torch":
            return self._forward_torch(batch)
        eng = _routes.engine_or_none()
        rows = eng.agg_gather([batch])
        return eng.aggregate(self.packed(eng.device), rows, batch.shape[2], batch.shape[3])

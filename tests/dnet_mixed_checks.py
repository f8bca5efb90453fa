"""Shared by tests/test_dnet_mixed_cpu.py and tests/test_gpu_dnet_mixed.py: the whole-network cases of the mixed-precision route (fixtures a
to d of dnet_layers_checks and a ragged forward_many), the loss scale of each, the recording of a run's ReLU masks and the figures
against the masked oracle (tests/dnet_mixed_restate.py)."""
import numpy as np
import torch

import dnet_backward_restate as br
import dnet_layers_checks as lc
import dnet_mixed_restate as mr
from densematcher_amd.diffusion_net import layers

# The loss is 2^s sum (y * g).  s per case: the largest integer for which, in the masked oracle, the largest gradient a backward kernel
# stages as an fp16 operand (oracle_gradients' second result, `top`) stays below 2^13 -- one binade of headroom under the 2^14 that the
# tests assert -- and every gradient of a parameter or of the input stays below 2^16 (fp16 ends at 65504), so that the fp16 parameter gradients of the
# autocast yardstick stay finite too (case c, a global mean: its bias gradients are 2^7 times its largest operand).
# test_dnet_mixed_cpu.py::test_the_loss_scales recomputes both on the CPU.
SCALE = {"a": 11, "b": 11, "c": 14, "d": 11, "many": 10}
MANY = ("t", "r", "f")            # forward_many's ragged list: 160, 96, 81 vertices


def rnd(seed, *shape, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


class Case:
    """network, inputs per mesh, the reference's call arguments, the packed operators and the cotangents g of a case, on `device`"""

    def __init__(self, case, device):
        self.case, self.device = case, device
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        if case == "many":
            self.net = lc.network("a", device)
            self.keys = MANY
            self.packed = layers.pack_operators([lc.operators(k) for k in MANY]).to(device)
            std = float(lc.golden()["a_x"].std())
            self.xs = [dev(std * rnd(100 + 1000 * b, n, 19)) for b, n in enumerate(self.packed.n_verts)]
            self.gs = [dev(rnd(91 + b, n, 24)) for b, n in enumerate(self.packed.n_verts)]
            self.kw, self.x, self.batched, self.faces = None, None, True, None
            return
        self.net = lc.network(case, device)
        self.keys = lc.config(case)["meshes"]
        self.x, self.kw = lc.call_arguments(case, device)
        self.packed = layers.pack_operators([lc.operators(k) for k in self.keys]).to(device)
        self.batched = self.x.dim() == 3
        with torch.no_grad():
            shape = self.net(self.x, route="torch", **self.kw).shape
        g = dev(rnd(90, *shape))
        self.xs = [self.x[b] for b in range(self.x.shape[0])] if self.batched else [self.x]
        self.gs = [g[b] for b in range(g.shape[0])] if self.batched else [g]
        self.g = g
        self.faces = [self.kw["faces"]] if "faces" in self.kw else None

    @property
    def scale(self):
        return 2.0 ** SCALE[self.case]

    def torch_call(self, x_or_list):
        """the torch route on the reference's tensors: the case's own call; the ragged list one mesh at a time.  Returns the outputs per mesh"""
        if self.case == "many":
            outs = []
            for x, k in zip(x_or_list, self.keys):
                _, mass, _, evals, evecs, gX, gY = lc.operators(k, self.device)
                outs.append(self.net(x, mass=mass, evals=evals, evecs=evecs, gradX=gX, gradY=gY, route="torch"))
            return outs
        y = self.net(x_or_list, route="torch", **self.kw)
        return [y[b] for b in range(y.shape[0])] if self.batched else [y]

    def leaf(self):
        """a fresh input that requires grad, as the case's call takes it"""
        if self.case == "many":
            return [x.clone().requires_grad_() for x in self.xs]
        return self.x.clone().requires_grad_()

    def loss(self, ys):
        return self.scale * sum((y * g).sum() for y, g in zip(ys, self.gs))

    def collect(self, leaf):
        """name -> gradient of the module's parameters and 'x' (B, N, C) padded, or (N, C) for a flat case"""
        out = {name: p.grad.detach().clone() for name, p in self.net.named_parameters() if p.grad is not None}
        if self.case == "many":
            N = max(x.shape[0] for x in leaf)
            out["x"] = torch.stack([torch.nn.functional.pad(x.grad, (0, 0, 0, N - x.shape[0])) for x in leaf])
        else:
            out["x"] = leaf.grad.detach().clone()
        return out

    def split_masks(self, recorded, per_mesh_calls=False):
        """recorded: the (B, N, C) (or (1, n, C)) bool outputs of the ReLU layers in the order in which they ran -> per layer a list over
        the meshes of (n_b, C).  per_mesh_calls: the run called the network once per mesh (mesh-major), not once for the batch"""
        n = self.packed.n_verts
        if per_mesh_calls:
            per = len(recorded) // len(n)
            return [[recorded[b * per + l][0, :n[b]] for b in range(len(n))] for l in range(per)]
        return [[m[b, :n[b]] for b in range(len(n))] for m in recorded]

    def oracle(self, relu_masks, drop_masks=None):
        """(gradients in the layout of collect, the largest staged gradient operand) of the masked oracle under these masks"""
        grads, top, _ = mr.oracle_gradients(self.net, self.xs, br.dense_operators(self.packed, torch.float64, device="cpu"), self.gs, relu_masks,
                                            scale=self.scale, drop_masks=drop_masks, faces=self.faces)
        flat = br_flat(grads)
        if self.case != "many" and not self.batched:
            flat["x"] = flat["x"][0]
        return flat, top


def br_flat(grads):
    out = dict(grads)
    xs = out.pop("x")
    N = max(x.shape[0] for x in xs)
    out["x"] = torch.stack([torch.nn.functional.pad(x.grad, (0, 0, 0, N - x.shape[0])) for x in xs])
    return out


def relu_hooks(net, into):
    """forward hooks on the nn.ReLU modules of net that append (output > 0) to `into`; returns the handles"""
    return [m.register_forward_hook(lambda mod, inp, out: into.append(out.detach() > 0)) for m in net.modules() if isinstance(m, torch.nn.ReLU)]


def emulated_run(c):
    """the route restated on the CPU: (gradients in Case.collect's layout, its ReLU masks)"""
    params = br.leaf_parameters(c.net, torch.float64)
    leaves = [x.double().requires_grad_() for x in c.xs]
    ys, masks = mr.emulated_network(c.net, params, leaves, br.dense_operators(c.packed, torch.float64), faces=c.faces)
    (c.scale * sum((y * g.double()).sum() for y, g in zip(ys, c.gs))).backward()
    grads = {name: p.grad for name, p in params.items()}
    grads["x"] = leaves
    flat = br_flat(grads)
    if c.case != "many" and not c.batched:
        flat["x"] = flat["x"][0]
    return flat, masks


def autocast_run(c, device_type):
    """the same fp32 module on route='torch' under torch.autocast(device_type, dtype=torch.float16): (gradients, its ReLU masks)"""
    recorded = []
    hooks = relu_hooks(c.net, recorded)
    try:
        c.net.zero_grad()
        leaf = c.leaf()
        with torch.autocast(device_type, dtype=torch.float16):
            ys = c.torch_call(leaf)
        c.loss([y.float() for y in ys]).backward()
    finally:
        for h in hooks:
            h.remove()
    return c.collect(leaf), c.split_masks(recorded, per_mesh_calls=c.case == "many")


def report(tag, device_figs, yard_figs, columns=("device", "torch autocast")):
    """prints every per-tensor pair and the largest of each; returns (largest device figure, largest yardstick figure)"""
    assert set(device_figs) == set(yard_figs)
    for name in sorted(device_figs):
        d, y = device_figs[name], yard_figs[name]
        note = "   <- its own ratio exceeds 1" if d > y else ""
        print(f"{tag} {name}: {columns[0]} {d:.3e}, {columns[1]} {y:.3e}, ratio {d / max(y, 1e-300):.3f}{note}")
    top_d, top_y = max(device_figs.values()), max(yard_figs.values())
    print(f"{tag}: largest {columns[0]} figure {top_d:.3e}, largest {columns[1]} figure {top_y:.3e}, ratio {top_d / max(top_y, 1e-300):.3f}")
    return top_d, top_y

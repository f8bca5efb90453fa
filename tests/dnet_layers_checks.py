"""Shared by tests/test_dnet_layers_cpu.py and tests/test_gpu_dnet_layers.py: the fixture tests/golden/fx_dnet_layers.npz (the reference's
DiffusionNet run on the CPU, tools/make_golden_dnet_layers.py), the networks and operators its cases name, and the whole-network bound."""
import functools
import json
import os

import numpy as np
import torch

from densematcher_amd.diffusion_net import layers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_dnet_layers.npz")
CASES = ("a", "b", "c", "d")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def log_softmax(x):
    return torch.nn.functional.log_softmax(x, dim=-1)


def config(case):
    return json.loads(str(golden()[f"{case}_cfg"]))


def names(case):
    return [str(n) for n in golden()[f"{case}_names"]]


def state(case):
    fx = golden()
    return {n: torch.from_numpy(fx[f"{case}_p{i}"].copy()) for i, n in enumerate(names(case))}


def network(case, device="cpu", load=True):
    kw = {k: v for k, v in config(case).items() if k != "meshes"}
    if kw.get("last_activation") == "log_softmax":
        kw["last_activation"] = log_softmax
    net = layers.DiffusionNet(**kw)
    if load:
        net.load_state_dict(state(case), strict=True)
    return net.to(device).eval()


def operators(key, device="cpu"):
    """mesh `key` of the fixture as the tuple get_operators returns (frames and L are None), float32"""
    fx = golden()
    n = fx[f"mass_{key}"].shape[0]
    t = lambda name: torch.from_numpy(fx[f"{name}_{key}"]).to(device)
    sp = lambda name: torch.sparse_coo_tensor(torch.from_numpy(np.stack((fx[f"{name}_row_{key}"], fx[f"{name}_col_{key}"])).astype(np.int64)),
                                              torch.from_numpy(fx[f"{name}_val_{key}"]), (n, n)).coalesce().to(device)
    return (None, t("mass"), None, t("evals"), t("evecs"), sp("gradX"), sp("gradY"))


def faces(key, device="cpu"):
    return torch.from_numpy(golden()[f"faces_{key}"].astype(np.int64)).to(device)


def call_arguments(case, device="cpu"):
    """(x, keyword arguments) of DiffusionNet.forward for the case, in the reference's tensors"""
    fx, keys = golden(), config(case)["meshes"]
    x = torch.from_numpy(fx[f"{case}_x"]).to(device)
    ops = [operators(k, device) for k in keys]
    if len(keys) == 1:
        _, mass, _, evals, evecs, gX, gY = ops[0]
        return x, dict(mass=mass, evals=evals, evecs=evecs, gradX=gX, gradY=gY, faces=faces(keys[0], device))
    st = lambda i: torch.stack([o[i] for o in ops])
    return x, dict(mass=st(1), evals=st(3), evecs=st(4))


def check_output(case, got, tag):
    """|got - ref| <= (4 f32_floor + 2^-23) max |ref|: the floor is one fp32 evaluation's distance from exact arithmetic, the factor 4
    covers another evaluation order, 2^-23 the final rounding.  Returns the measured figure (printed before it is asserted)."""
    fx = golden()
    ref = fx[f"{case}_y_ref32"].astype(np.float64)
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    figure = np.abs(got - ref).max() / np.abs(ref).max()
    bound = 4.0 * float(fx[f"{case}_f32_floor"]) + 2.0 ** -23
    print(f"{tag} case {case}: max |got - ref| / max |ref| = {figure:.3e} (bound {bound:.3e})")
    assert figure <= bound, (case, figure, bound)
    return figure

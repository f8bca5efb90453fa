"""Shared by tests/test_dnet_operators_cpu.py and tests/test_gpu_dnet_operators.py: the fixture tests/golden/fx_dnet.npz (the reference's
own frames / gradients, tools/make_golden_dnet.py) and the comparisons both routes must pass."""
import functools
import os

import numpy as np
import scipy.sparse as sp
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_dnet.npz")
NAMES = ("frames", "massvec", "L", "evals", "evecs", "gradX", "gradY")
# entrywise on the densified matrices, relative to max |ref|: the bars tests/test_gpu_laplacian.py:63-65 uses for the same kind of assembly
BOUNDS = {"frames": 1e-13, "massvec": 1e-13, "L": 1e-11, "gradX": 1e-11, "gradY": 1e-11}


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def mesh(key, dtype=torch.float64, device="cpu"):
    fx = golden()
    return (torch.from_numpy(fx[f"verts_{key}"].astype(np.float64)).to(device=device, dtype=dtype),
            torch.from_numpy(fx[f"faces_{key}"].astype(np.int64)).to(device))


def ref_array(key, name):
    """the stored array `name` of mesh `key`, sparse ones densified, float64"""
    fx = golden()
    if name in ("L", "gradX", "gradY"):
        n = fx[f"verts_{key}"].shape[0]
        return sp.coo_matrix((fx[f"{name}_val_{key}"].astype(np.float64), (fx[f"{name}_row_{key}"], fx[f"{name}_col_{key}"])), shape=(n, n)).toarray()
    return fx[{"massvec": "mass"}.get(name, name) + f"_{key}"].astype(np.float64)


def dense(t):
    t = t.detach().cpu()
    return (t.to_dense() if t.is_sparse else t).double().numpy()


def check_against_golden(ops, key, bounds=BOUNDS, tag=""):
    """every figure is printed before it is asserted"""
    got = dict(zip(NAMES, ops))
    figures = {}
    for name, bound in bounds.items():
        ref = ref_array(key, name)
        figures[name] = np.abs(dense(got[name]) - ref).max() / np.abs(ref).max()
        print(f"{tag} mesh {key}: {name}: max |got - ref| / max |ref| = {figures[name]:.3e} (bound {bound:.3e})")
    for name, bound in bounds.items():
        assert figures[name] <= bound, (key, name, figures[name], bound)


def check_spectrum(ops, ref_evals=None, tag=""):
    """eigenvalues against the reference's, mass-orthonormality to 1e-9, residual max |(L + 1e-8 I) phi - lambda M phi| <= 1e-7 max(lambda_k, 1)
    (tests/test_gpu_laplacian.py:128, 163-165); eigenvectors are never compared entry by entry"""
    got = {k: dense(v) for k, v in zip(NAMES, ops)}
    lam, Phi, mass, L = got["evals"], got["evecs"], got["massvec"], got["L"]
    G = Phi.T @ (mass[:, None] * Phi)
    orth = np.abs(G - np.eye(len(lam))).max()
    R = (L + 1e-8 * np.eye(L.shape[0])) @ Phi - (mass[:, None] * Phi) * lam[None, :]
    res = np.abs(R).max() / max(lam[-1], 1.0)
    dev = np.abs(lam - ref_evals).max() / ref_evals[-1] if ref_evals is not None else 0.0
    print(f"{tag} spectrum: |evals - ref| / ref_k = {dev:.3e} (1e-7), orthonormality {orth:.3e} (1e-9), residual {res:.3e} (1e-7)")
    assert lam.shape == (Phi.shape[1],) and np.all(lam >= 0) and np.all(np.diff(lam) >= 0)
    assert dev <= 1e-7 and orth <= 1e-9 and res <= 1e-7, (dev, orth, res)

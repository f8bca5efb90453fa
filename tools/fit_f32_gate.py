#!/usr/bin/env python
"""the fused fit's element loop in fp32 (precision="f32" of fit_general / energy_grad_fused; the reference evaluates these terms in fp32,
pyFM/functional.py:379-383) against the float64 loop.  Gate: energy / gradient within 1e-6 relative of the oracle, the tight fit
within 1e-4 of the oracle's float64 minimiser, bit-identical across batch sizes; then the time per evaluation at 64 pairs.
usage: python tools/fit_f32_gate.py"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import dm_oracle as orc  # noqa: E402
from densematcher_amd.engine import default_engine  # noqa: E402
from densematcher_amd.pyFM.functional import LBFGS_OPTIONS  # noqa: E402
import test_gpu_fitfuse as tf  # noqa: E402

eng = default_engine()
PREC = ("f64", "f32")               # (the printed lines keep the name fit_f32 = 0 | 1 of the earlier records)
NB = tf.NOTEBOOK_W
GOLD = os.path.join(REPO, "tests", "golden")
fx = dict(np.load(os.path.join(GOLD, "fx_cfg1.npz")))
fits = dict(np.load(os.path.join(GOLD, "oracle_cfg1_fits.npz")))

print("== one evaluation against the oracle (relative to |E|, max |G|)")
for (N1, N2, k1, k2) in [(300, 517, 15, 13), (1000, 777, 20, 30), (129, 65, 32, 32), (2048, 2048, 15, 15)]:
    rng = np.random.default_rng(N1 + 3 * N2 + k1)
    e1, e2, a1, C, A, Bm, lam1, lam2 = tf._random_problem(rng, 2, N1, N2, k1, k2)
    C[1] *= 40.0
    for w in ({"w_ent": 0.3}, dict(NB), {"w_p2p": 0.5, "w_ent": 0.3, "w_range01": 1.5, "w_sumto1": 2.0, "w_descr": 1.0, "w_lap": 0.1}):
        row = []
        for f32 in (0, 1):
            E, G = eng.energy_grad_fused(C, A, Bm, lam1, lam2, w, e1, e2, a1, precision=PREC[f32])
            worst_e = worst_g = 0.0
            for b in range(2):
                ev = orc.ev_sqdiff(lam1[b], lam2[b])
                Eo, Go = orc.energy_grad_general(C[b], A[b].astype(np.float64), Bm[b].astype(np.float64), ev, e1[b], e2[b], a1[b], w)
                worst_e = max(worst_e, abs(float(E[b]) - Eo) / abs(Eo))
                worst_g = max(worst_g, np.abs(G[b].cpu().numpy() - Go).max() / np.abs(Go).max())
            row.append((worst_e, worst_g))
        print(f"N1={N1:5d} N2={N2:5d} k=({k1},{k2}) terms={sorted(w)}: f64 dE {row[0][0]:.1e} dG {row[0][1]:.1e} | f32 dE {row[1][0]:.1e} dG {row[1][1]:.1e}", flush=True)

print("== the notebook's energy at a fitted map of the fixture (where the optimiser works)")
k = 15
e1, e2 = fx["Phi1"][:, :k], fx["Phi2"][:, :k]
A, Bq = orc.project(e1, fx["a1"], fx["F1"]), orc.project(e2, fx["a2"], fx["F2"])
ev = orc.ev_sqdiff(fx["lam1"][:k], fx["lam2"][:k])
x0 = orc.get_x0(k, k, float(fx["Phi1"][0, 0]), float(fx["Phi2"][0, 0]), float(fx["a1"].astype(np.float64).sum()), float(fx["a2"].astype(np.float64).sum()))
one = {n: v[:1] for n, v in tf._fit_batch(fx, k, 1, None).items()}
res = {}
for f32 in (0, 1):
    for name, opts in (("tight", dict(LBFGS_OPTIONS)), ("reference", None)):
        C1, r1 = eng.fit_general(one, NB, x0[None], lbfgs_options=opts, precision=PREC[f32])
        Ef, Gf = orc.energy_grad_general(C1[0], A, Bq, ev, e1, e2, fx["a1"], NB)
        res[(f32, name)] = C1[0]
        print(f"fit_f32={f32} stopping={name:9s}: nit {int(r1.nit[0]):4d} nfev {int(r1.nfev[0]):4d} status {int(r1.status[0])} oracle energy {Ef:.12e} max|grad| {np.abs(Gf).max():.2e}", flush=True)
print("|C_f32 - C_f64| tight:", np.abs(res[(1, 'tight')] - res[(0, 'tight')]).max(), " reference:", np.abs(res[(1, 'reference')] - res[(0, 'reference')]).max())

print("== k = 30 tight fit against the oracle's minimiser (bar 1e-4)")
k = int(fx["k"])
x30 = orc.get_x0(k, k, float(fx["Phi1"][0, 0]), float(fx["Phi2"][0, 0]), float(fx["a1"].astype(np.float64).sum()), float(fx["a2"].astype(np.float64).sum()))
one30 = {n: v[:1] for n, v in tf._fit_batch(fx, k, 1, None).items()}
for f32 in (0, 1):
    C1, r1 = eng.fit_general(one30, NB, x30[None], lbfgs_options=dict(LBFGS_OPTIONS), precision=PREC[f32])
    print(f"fit_f32={f32}: nit {int(r1.nit[0])} nfev {int(r1.nfev[0])} status {int(r1.status[0])} |C - C_oracle| = {np.abs(C1[0] - fits['C_nb']).max():.3e}", flush=True)

print("== batch invariance (fp32 loop): a pair in batches of 1, 3, 140")
k = 15
b3 = tf._fit_batch(fx, k, 3, None)
C3, r3 = eng.fit_general(b3, NB, np.stack([x0] * 3), lbfgs_options=dict(LBFGS_OPTIONS), precision="f32")
C1, r1 = eng.fit_general({n: v[:1] for n, v in b3.items()}, NB, x0[None], lbfgs_options=dict(LBFGS_OPTIONS), precision="f32")
big = tf._fit_batch(fx, k, 140, None)
Cb, rb = eng.fit_general(big, NB, np.stack([x0] * 140), lbfgs_options=dict(LBFGS_OPTIONS), precision="f32")
print("1 vs 3:", np.array_equal(C1[0], C3[0]), " 140 vs 3:", all(np.array_equal(Cb[b], C3[b % 3]) for b in (0, 1, 2, 137, 139)))

print("== time per evaluation, 64 pairs of N = 2048, k = 15 (the batched documented call's fit)")
from densematcher_amd import synth  # noqa: E402
B = 64
batch = synth.make_pair_batch(B, 64, 32, 512, 15, sigma=0.3, n_distinct_meshes=2)
dev = {n: torch.as_tensor(v).to(eng.device) for n, v in batch.items()}
x0b = np.zeros((B, 15, 15)); x0b[:, 0, 0] = 1.0
for f32 in (0, 1, 0, 1):
    torch.cuda.synchronize()
    eng.profile_kernel("fit_fused_eval")
    t0 = time.time()
    Cf, rf = eng.fit_general(dev, NB, x0b, k=15, precision=PREC[f32])
    torch.cuda.synchronize()
    dt = time.time() - t0
    n, ms = eng.profile_read()
    eng.profile_kernel("")
    print(f"fit_f32={f32}: fit {1e3 * dt:7.1f} ms, {n} launches, {1e3 * ms / max(n, 1):7.1f} us per launch (mean; late launches hold few pairs), nfev max {int(rf.nfev.max())}", flush=True)

#!/usr/bin/env python
"""
bench.py -- mesh-pairs/s of the matching hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload fmap|simnn|zoomout|stress|icp] [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path over one batch of synthetic mesh pairs that is
already resident in HBM.  A plain run sets up, warms up, times exactly K steps, writes the
last step's outputs (--dump-outputs DIR: DIR/<name>.npy, float32 / float64, at most 64 MB;
the seeded inputs are the same from run to run) and prints the line.  Everything else below
(roofline, per-kernel tables, parity, the other configs, cpu_baseline) needs --full.
Default workload = BASELINE.json configs[1]:
    batch = 64 pairs per GPU, N = 2048 vertices (64x32 torus), D = 768 fp16 descriptors,
    k = 128 eigenfunctions:  project -> pinned column -> functional-map solve -> four vertex maps.
Pairs are independent: with N GPUs every rank processes its own 64 pairs (weak scaling, no
data-path collective); the process group (RCCL) is used only for the timing barrier / max.

`--gpus N` with N > 1 and no launcher in the environment: bench.py launches its N ranks itself
(python -m torch.distributed.run, one process per GPU, rendezvous on 127.0.0.1).  Under an
external torchrun it reads RANK / LOCAL_RANK / WORLD_SIZE as usual.

Prints ONE JSON line (rank 0): metric, value, unit, higher_is_better, dtype, ms_per_step, steps, config ...; --full adds
    roofline      the kernel that takes the largest share of the step (per-kernel HIP-event table of an untimed pass of the
                  same step; its launch time inside the timed region), priced on SURVEY 8(d)'s ALGORITHMIC flops against the
                  spec peak of the arithmetic it runs in, with
                    .peak_measured     on-box probes (dm_measure_peak): fp16 MFMA on zero and on N(0,1) operands, f64 MFMA, copy
                    .kernels[]         every kernel above 2 % of the step: avg ms, share, algorithmic / executed flops, frac
                    .config3_simnn     (default workload) the feature-similarity kernel of configs[2], same method:
                                       north_star's ">= 60 % of the 16-bit MFMA roofline" target refers to that kernel
                    .config5_stress    (default workload) configs[4] (N = 8192, k = 200), 3 steps
    parity        (default workload only) |C_gpu - C_f64| and |C_gpu - C_fit| on the committed config-2 fixture
    cpu_baseline  the NumPy oracle timed on this box's host cores on a bounded sample of the same workload:
                  the closed-form port and a reference-faithful variant (kd-tree NN, dense indicator, L-BFGS-B)
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md; f64 MFMA = half the f32 MFMA rate, AMD spec 78.6 TF)
PEAK_TFLOPS = {"f64": 78.6, "f32": 157.3, "f16": 2500.0}

WORKLOADS = {
    # name: (nu, nv, D, k, pairs per GPU)
    "fmap": dict(nu=64, nv=32, D=768, k=128, B=64, cfg="configs[1]: batch=64 pairs, N=2048, D=768, k=128 functional-map solve"),
    "simnn": dict(nu=64, nv=32, D=768, k=0, B=64, cfg="configs[2]: batch=64 pairs, N=2048, D=768 brute-force NN feature similarity + argmax"),
    "zoomout": dict(nu=64, nv=32, D=0, k=200, B=32, cfg="configs[3]: 32 pairs/GPU, N=2048, k=50->200 ZoomOut refinement"),
    "stress": dict(nu=128, nv=64, D=384, k=200, B=64, cfg="configs[4]: batch=64 pairs, N=8192, D=384, k=200 (HBM-bound stress)"),
    "icp": dict(nu=64, nv=32, D=0, k=128, B=64, cfg="SURVEY 8(f) next #1: spectral ICP, 10 iterations, 64 pairs/GPU, N=2048, k=128"),
    "surface_map": dict(nu=64, nv=32, D=512, k=15, B=1,
                        cfg="the reference's one documented call: compute_surface_map with the notebook's parameters (example.ipynb cell 11: "
                            "n_ev=15, w_descr=1e4, w_lap=1e3, w_ent=0.1, w_sumto1=10, compute_extra=True) on one raw mesh pair, N=2048, D=512 "
                            "(BASELINE.md section 2: 39.8 s/pair for the reference on 8 CPU cores)"),
}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 20; surface_map: 3 calls)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps before them (default 3; surface_map: 1 call)")
    ap.add_argument("--workload", default="fmap", choices=list(WORKLOADS))
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0) as DIR/<name>.npy: float64 for float64 results and integer maps, "
                         "float32 otherwise; a seeded sample of the pairs where the whole exceeds 64 MB")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: roofline and per-kernel tables, timing blocks, parity, PCIe-inclusive "
                         "rate, the other configs, the CPU baseline")
    ap.add_argument("--batch", type=int, default=0, help="pairs per GPU (default: the config's)")
    ap.add_argument("--basis", default="f64", choices=["f64", "f32"],
                    help="dtype of the eigenvectors and masses handed to the path: f64 = what the reference holds and consumes "
                         "(TriMesh / FM_to_p2p run on float64; the *_f64 entry points), f32 = pre-rounded inputs (round-1/2 benches)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the other configs' blocks of the default workload")
    ap.add_argument("--p2p-split", type=int, default=None,
                    help="code path of the four maps (dm_set_option p2p_split): 0 float64 kernel, 1 two fp16 passes, 2 one pass in both "
                         "directions (3: its 4-wave shape); default: the library's")
    ap.add_argument("--dist-backend", default="nccl", help="process-group backend (nccl = RCCL)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the process group (RCCL) and run the barrier / max-over-ranks through it even with ONE rank: "
                         "the N > 1 branch of the timing code on a 1-GPU box (tests/test_gpu_shard.py)")
    ap.add_argument("--single-device", action="store_true",
                    help="rehearsal of the N > 1 path on a 1-GPU box: every rank uses cuda:0, gloo carries the barrier")
    args = ap.parse_args()
    one_pair = args.workload == "surface_map"
    if args.steps is None:
        args.steps = 3 if one_pair else 20
    if args.warmup is None:
        args.warmup = 1 if one_pair else 3
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks (one process per GPU) and relay rank 0's line."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    return subprocess.call(cmd, env=env)


def make_batch(w, rank, basis="f64"):
    from threadpoolctl import threadpool_limits
    from densematcher_amd import synth
    n = w["nu"] * w["nv"]
    rdt = np.float64 if basis == "f64" else np.float32
    if w["k"]:
        # N = 8192: a mass-orthonormalised seeded Gaussian stands in for the eigenbasis (throughput-only
        # runs; an ARPACK solve per mesh would dominate the set-up and the arithmetic does not depend on it).
        # One BLAS thread: the unperturbed torus has repeated eigenvalues, and which basis of such an eigenspace the solver
        # returns depends on how its products are split over threads; the inputs must not change with the thread count.
        with threadpool_limits(limits=1, user_api="blas"):
            batch = synth.make_pair_batch(w["B"], w["nu"], w["nv"], max(w["D"], 8), w["k"], sigma=0.1, n_distinct_meshes=2,
                                          seed0=100 * rank, basis="eig" if n <= 4096 else "random", real_dtype=rdt)
    else:
        batch = simnn_features(w["B"], n, w["D"], rank)
    return batch


def simnn_features(B, n, D, rank):
    from densematcher_amd import synth
    batch = {"F1": np.empty((B, n, D), np.float16), "F2": np.empty((B, n, D), np.float16)}
    for i in range(B):
        batch["F1"][i], batch["F2"][i], _ = synth.feature_pair(n, n, D, 1000 + i + 1000 * rank, 2000 + i + 1000 * rank, sigma=1.0)
    return batch


PREHEAT_S = 0.25


def kernel_models(N, D, k, B, eng):
    """SURVEY.md 8(d) algorithmic work of the step's kernels, per LAUNCH (B pairs), keyed by the DM_LAUNCH name.
    dtype = the arithmetic the kernel runs in (its spec peak prices `frac`); executed = what the matrix cores actually
    issue where that differs from the algorithmic count (fp16 split: three products per float64 index, padded)."""
    n = k - 1
    kd = 3 * 16 * (-(-k // 16)) if k else 0        # split rows: three fp16 products per index, indices padded to 16
    return {
        "fmap_solve_chol": dict(dtype="f64", bound="mfma", what="k2 SPD solves of order k1-1 per pair: k (n^3/3 + 2 n^2)",
                                flops=B * k * (n ** 3 / 3.0 + 2.0 * n * n)),
        # r06: the same k2 solves by the batched Jacobi-preconditioned conjugate-gradient iteration (csrc/dm_pcg.h).  `flops` stays SURVEY
        # 8(d)'s algorithmic count of the solves (what a direct method spends); the iteration issues 2 n^2 k per step and pair on the
        # matrix cores (about 24 steps to its tolerance: 0.8 of the algorithmic count at n = 127) -- not quoted as `executed` because the
        # step count is data dependent
        "fmap_solve_pcg": dict(dtype="f64", bound="mfma", what="k2 SPD solves of order k1-1 per pair (batched PCG on the matrix cores): k (n^3/3 + 2 n^2)",
                               flops=B * k * (n ** 3 / 3.0 + 2.0 * n * n)),
        "simnn4_f16_mfma": dict(dtype="f16", bound="mfma", what="G = Phi2 C Phi1^T and its four arg-reductions: 2 N^2 k (float64 flops of the reference)",
                                flops=2.0 * N * N * k * B, executed=2.0 * N * N * kd * B),
        "simnn2_f16_mfma": dict(dtype="f16", bound="mfma", what="one direction of G: 2 N^2 k", flops=2.0 * N * N * k * B, executed=2.0 * N * N * kd * B),
        "gred_f64": dict(dtype="f64", bound="mfma", what="G = Phi2 C Phi1^T: 2 N^2 k", flops=2.0 * N * N * k * B),
        "simnn_f16_mfma": dict(dtype="f16", bound="mfma", what="S = Ftgt Fsrc^T: 2 N^2 D", flops=2.0 * N * N * D * B),
        "embed_nt_f64": dict(dtype="f64", bound="mfma", what="one embedding Phi C^T (or Phi C): 2 N k^2", flops=2.0 * N * k * k * B),
        "project_f16split_mfma": dict(dtype="f16", bound="mfma", what="one projection Phi^T (a F): 2 k N D", flops=2.0 * k * N * D * B,
                                      executed=4.0 * k * N * D * B),
        "gram_nt_f64": dict(dtype="f64", bound="mfma", what="[A; B] A^T: 2 (2 k^2 D)", flops=4.0 * k * k * D * B),
        "p2pfm_tn_f64": dict(dtype="f64", bound="mfma", what="Phi2^T (a2 Phi1[p]): 2 N k^2", flops=2.0 * N * k * k * B),
    }


def kernel_table(eng, step, n_steps, models, workload, min_share=0.02, step_ms=None):
    """Per kernel name: launches per step, average launch duration, share of the step and -- where SURVEY 8(d) gives the kernel's
    algorithmic work -- achieved rate and fraction of the spec peak.  Two passes of the same step: ONE step with every launch
    bracketed by HIP events (dm_profile_kernel "*") finds the names and the launch counts; then every kernel above min_share is
    timed on its own (only its launches bracketed, n_steps steps) -- with all launches bracketed the event pairs perturb the
    step by ~6 %, with one kernel bracketed the step runs as in the timed region.
    share_of_step = launches x avg / (step_ms, or the sum over the kernels when step_ms is not given)."""
    import torch
    step()
    torch.cuda.synchronize()
    eng.profile_kernel("*")
    step()
    rep = eng.profile_report()
    eng.profile_kernel("")
    total_all = sum(ms for _, ms in rep.values()) or 1.0
    rows, kernel_ms = [], 0.0
    for name, (n, ms) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
        if ms / total_all >= min_share:
            eng.profile_kernel(name)
            for _ in range(n_steps):
                step()
            n1, ms1 = eng.profile_read()
            eng.profile_kernel("")
            avg, per_step = ms1 / max(n1, 1), n1 / n_steps
        else:
            avg, per_step = ms / n, float(n)
        kernel_ms += avg * per_step
        row = {"name": name, "launches_per_step": round(per_step, 2), "avg_launch_ms": round(avg, 4), "_ms_per_step": avg * per_step}
        m = models.get(name)
        if m:
            peak = PEAK_TFLOPS[m["dtype"]]
            ach = m["flops"] / (avg * 1e-3) / 1e12
            row.update(bound=m["bound"], dtype=m["dtype"], algorithmic_flops_per_launch=m["flops"], achieved=round(ach, 3),
                       peak=peak, frac=round(ach / peak, 4), algorithmic_work=m["what"])
            if "executed" in m:
                row["executed_flops_per_launch"] = m["executed"]
                row["frac_executed"] = round(m["executed"] / (avg * 1e-3) / 1e12 / peak, 4)
        traffic, tfile = pmc_traffic_bytes(name, workload) if workload else (None, None)
        if traffic:
            row["traffic"] = traffic
            row["traffic_file"] = "profiles/" + tfile
        if ms / total_all >= min_share:
            rows.append(row)
    denom = step_ms if step_ms else kernel_ms
    for r in rows:
        r["share_of_step"] = round(r.pop("_ms_per_step") / denom, 4)
    rows.sort(key=lambda r: -r["share_of_step"])
    return rows, kernel_ms, float(sum(n for n, _ in rep.values()))


_PEAKS = {}


def measured_peaks(eng):
    """on-box probes, once per process (about 0.2 s): TFLOP/s and GB/s"""
    if not _PEAKS:
        for nm in ("mfma_f16_zero_operands", "mfma_f16_random_operands", "mfma_f64"):
            _PEAKS[nm + "_tflops"] = round(eng.measure_peak(nm) / 1e12, 1)
        _PEAKS["hbm_copy_gbs"] = round(eng.measure_peak("hbm_copy") / 1e9, 0)
        _PEAKS["note"] = ("fp16 MFMA: zero operands run at 2.4 GHz (issue ceiling = the guide's 2.5 PF), N(0,1) operands at ~1.7 GHz "
                          "(power): the second is the ceiling of a kernel that multiplies real data (tools/ubench_mfma_clock.hip)")
    return dict(_PEAKS)


N_BLOCKS = 5


def timed_kernel(eng, step, kernel, steps, warmup, barrier, n_blocks=N_BLOCKS, max_over_ranks=None, local_out=None):
    """W untimed steps, then n_blocks blocks of EXACTLY K steps, each bracketed by barrier() (barrier + device synchronisation) on
    both sides; the MEDIAN block is the reported one (a 28 ms region varies by a few % with the box's clocks; the other blocks
    come back too).  Returns (elapsed s of the median block -- the max over ranks of each block first --, launches of `kernel`
    in it, their summed ms, [every block's elapsed s]).
    Before the warm-up the same step runs untimed for PREHEAT_S seconds: the part raises its clocks only after some tens of
    milliseconds of sustained load (the first launches of a process run ~20 % slower)."""
    warm_up(step, warmup)
    blocks = []
    for _ in range(n_blocks):
        barrier()
        eng.profile_kernel(kernel)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        barrier()
        elapsed = time.perf_counter() - t0
        launches, kernel_ms = eng.profile_read()
        eng.profile_kernel("")
        if local_out is not None:
            local_out.append(elapsed)                     # (this rank's own time, before the max over ranks)
        if max_over_ranks is not None:
            elapsed = max_over_ranks(elapsed)
        blocks.append((elapsed, launches, kernel_ms))
    order = sorted(range(n_blocks), key=lambda i: blocks[i][0])
    med = blocks[order[n_blocks // 2]]
    return med[0], med[1], med[2], [b[0] for b in blocks]


def warm_up(step, warmup):
    """PREHEAT_S seconds of the step (clocks up), then `warmup` steps, all untimed"""
    import torch
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < PREHEAT_S:
        step()
        torch.cuda.synchronize()
    for _ in range(warmup):
        step()


def timed_steps(step, steps, warmup, barrier, max_over_ranks):
    """The headline: after warm_up, exactly `steps` steps bracketed by barrier() (barrier + device synchronisation) on both sides,
    nothing else inside.  Returns (elapsed s, the max over ranks; what the last step returned)."""
    warm_up(step, warmup)
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps - 1):
        step()
    last = step()
    barrier()
    return max_over_ranks(time.perf_counter() - t0), last


DUMP_LIMIT_BYTES = 64 << 20


def output_arrays(obj, name, out):
    """every tensor / array in a result into out[name] as a host array: dicts by key, tuples and lists by position"""
    import torch
    if isinstance(obj, dict):
        for key, v in obj.items():
            output_arrays(v, f"{name}_{key}" if name else str(key), out)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            output_arrays(v, f"{name}_{i}", out)
    elif isinstance(obj, torch.Tensor):
        t = obj.detach()
        out[name] = (t if t.dtype == torch.float64 or not t.is_floating_point() else t.float()).cpu().numpy()
    elif isinstance(obj, np.ndarray) and obj.dtype.kind in "fiub":
        out[name] = obj
    return out


def dump_outputs(dirname, arrays):
    """--dump-outputs: DIR/<name>.npy per array, float64 for float64 results and integer maps (exact), float32 for narrower floats.
    Above DUMP_LIMIT_BYTES in all, every array keeps the same seeded sample of its leading-axis rows (the pairs).  Returns the names."""
    arrays = {n: (a if a.dtype == np.float64 else a.astype(np.float32 if a.dtype.kind == "f" else np.float64)) for n, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        for n, a in arrays.items():
            if a.ndim:
                rows = np.random.default_rng(0).permutation(a.shape[0])[:max(1, int(a.shape[0] * DUMP_LIMIT_BYTES / total))]
                arrays[n] = a[np.sort(rows)]
    os.makedirs(dirname, exist_ok=True)
    for n, a in arrays.items():
        np.save(os.path.join(dirname, n + ".npy"), np.ascontiguousarray(a))
    return sorted(arrays)


NOTEBOOK_FIT = dict(w_descr=1e4, w_lap=1e3, w_dcomm=0, w_ent=1e-1, w_sumto1=1e1, optinit="zeros", maxiter=5000)   # example.ipynb cell 11


class _Duck:
    """what compute_surface_map needs of a pytorch3d Meshes object (functional_map.py:17-18)"""
    def __init__(self, v, f):
        self.v, self.f = v, f

    def verts_list(self):
        return [self.v]

    def faces_list(self):
        return [self.f]


def surface_map_workload(args):
    """Latency of the API the reference exposes: one compute_surface_map call (raw meshes in, 14-tuple out), per-stage times.
    value = calls per second of ONE pair at a time (the reference's own use); a step is one call."""
    import torch
    from densematcher_amd import functional_map as fmod, synth
    from densematcher_amd.pyFM.functional import FunctionalMapping
    from densematcher_amd.pyFM.mesh import laplacian as _lap
    _lap.set_robust_backend("restated")       # (no robust_laplacian wheel on the box: the call opts into the package's restatement)
    w = WORKLOADS["surface_map"]
    nu, nv, D, k = w["nu"], w["nv"], w["D"], w["k"]
    (v1, f1), (v2, f2) = synth.torus_mesh(nu, nv, perturb=0.03, seed=3), synth.torus_mesh(nu, nv, perturb=0.08, seed=1)
    F1, F2, _ = synth.feature_pair(nu * nv, nu * nv, D, 1000, 2000, sigma=0.5, perm="identity")
    stages = {}

    def timed(name, fn):
        def wrapper(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
            return out
        return wrapper
    patched = [(FunctionalMapping, "preprocess", "eigenbases (2 meshes: assembly + eigensolve on the GPU)"),
               (FunctionalMapping, "fit", "fit (L-BFGS, notebook energy terms)"), (FunctionalMapping, "get_p2p", "vertex maps (2 x 4 maps)"),
               (FunctionalMapping, "_precise_map_device", "precise map"), (FunctionalMapping, "icp_refine", "ICP (10 iterations)"),
               (fmod, "_assign_many", "linear assignment (3 matrices, one batched call)")]
    import warnings

    def one_call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res_ = fmod.compute_surface_map(_Duck(v1, f1), _Duck(v2, f2), F1, F2, n_ev=k, compute_extra=True, optimizer="L-BFGS-B",
                                            fit_params=dict(NOTEBOOK_FIT))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res_
    # the call as a user makes it (the assignments overlap the later stages on side streams): this is `value`
    times = []
    for rep in range(args.warmup + args.steps):
        dt, res = one_call()
        times.append(dt)
    t = float(np.median(times[args.warmup:]))
    model = res[7]
    out = {"metric": "compute_surface_map calls/sec (one pair at a time, notebook parameters)", "value": round(1.0 / t, 4), "unit": "mesh-pairs/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * t, 2), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": w["cfg"], "pairs_per_gpu": 1, "N": nu * nv, "D": D, "k": k},
           "fit": {"iterations": int(model.fit_result.nit[0]), "evaluations": int(model.fit_result.nfev[0]), "status": model.fit_result.message[0]},
           "roofline": {"bound": "latency", "kernel": None, "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None,
                        "note": "a single pair cannot fill the chip: this workload reports the latency of the API; the throughput kernels are in the default workload"}}
    if args.dump_outputs:
        names = ("p2p_21", "p2p_12", "hungarian", "hungarian_precise", "p2p_21_icp", "p2p_12_icp", "hungarian_icp", "model", "mesh1", "mesh2",
                 "p2p_21_adjoint", "p2p_12_adjoint", "p2p_21_icp_adjoint", "p2p_12_icp_adjoint")
        arrays = output_arrays(dict(zip(names, res)), "", {})
        output_arrays(model.FM, "FM", arrays)
        out["outputs"] = dump_outputs(args.dump_outputs, arrays)
    del res, model
    if args.full:
        # per-stage times from a separate instrumented call: every stage bracketed by device synchronisations, the three assignments as one
        # batched call at the end (the stages add up to more than the clean call: nothing overlaps there)
        saved = [(o, n, getattr(o, n)) for o, n, _ in patched]
        for o, n, label in patched:
            setattr(o, n, timed(label, getattr(o, n)))
        fmod.EARLY_ASSIGNMENTS = False
        try:
            stages.clear()
            t_instr, _ = one_call()
            last_stages = dict(stages)
        finally:
            fmod.EARLY_ASSIGNMENTS = True
            for o, n, fn in saved:
                setattr(o, n, fn)
        out["stages_ms"] = {n: round(1e3 * v, 2) for n, v in last_stages.items()}
        out["stages_note"] = ("from a separate instrumented call (%.1f ms: every stage bracketed by device synchronisations, the three assignments as "
                              "one batched call at the end); in the timed calls the fitted map's and the precise map's assignments run on side streams "
                              "beside the later stages" % (1e3 * t_instr))
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_surface_map(v1, f1, v2, f2, F1, F2, k)
    print(json.dumps(out), flush=True)


def cpu_surface_map(v1, f1, v2, f2, F1, F2, k):
    """the same call restated on the host with the oracle (one pair): dense eigensolve of the same Laplacians, float64 L-BFGS-B
    with SciPy's default stopping rule (the reference's), kd-tree-free maps, SciPy's linear_sum_assignment x 3, precise map, ICP"""
    import scipy.linalg
    import scipy.optimize
    from densematcher_amd import synth
    from oracle import dm_oracle as orc
    t_all = time.perf_counter()
    st = {}

    def tick(name, t0):
        st[name] = round(1e3 * (time.perf_counter() - t0), 1)
    t0 = time.perf_counter()
    bases = []
    for v, f in ((v1, f1), (v2, f2)):
        W, m = synth.cotan_laplacian(v, f)
        lam, phi = scipy.linalg.eigh(W.toarray(), np.diag(m), subset_by_index=[0, max(20, k) - 1])
        bases.append((lam[:k], phi[:, :k], m))
    tick("eigenbases (dense eigh)", t0)
    (l1, e1, m1), (l2, e2, m2) = bases
    t0 = time.perf_counter()
    wts = {n: v for n, v in NOTEBOOK_FIT.items() if n.startswith("w_")}
    C, _ = orc.fit_general(e1, e2, l1, l2, m1, m2, F1, F2, wts, tight=False)
    tick("fit", t0)
    t0 = time.perf_counter()
    orc.fm_to_p2p_all(C, e1, e2, m1)
    M0 = orc.mapped_indicator(C, e1, e2, m1)
    tick("vertex maps + indicator", t0)
    t0 = time.perf_counter()
    scipy.optimize.linear_sum_assignment(M0, maximize=True)
    P0, _, _ = orc.precise_map_dense(C, e1, e2, f1)
    scipy.optimize.linear_sum_assignment(P0, maximize=True)
    tick("assignment x 2 + precise map", t0)
    t0 = time.perf_counter()
    Ci = orc.icp_refine(C, e1, e2, nit=10)
    orc.fm_to_p2p_all(Ci, e1, e2, m1)
    scipy.optimize.linear_sum_assignment(orc.mapped_indicator(Ci, e1, e2, m1), maximize=True)
    tick("ICP + maps + assignment", t0)
    tot = time.perf_counter() - t_all
    return {"value": round(1.0 / tot, 4), "unit": "mesh-pairs/s", "cores": os.cpu_count() or 1, "kind": "port", "stages_ms": st,
            "sample": f"one pair, the same call on the oracle (NumPy / SciPy float64, BLAS threads on {os.cpu_count()} cores), {tot:.1f} s"}


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    if args.workload == "surface_map":
        return surface_map_workload(args)

    import torch
    from densematcher_amd.engine import MatchEngine

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    backend = args.dist_backend
    if args.single_device:
        local_rank, backend = 0, "gloo"
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or args.force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    w = dict(WORKLOADS[args.workload])
    if args.batch:
        w["B"] = args.batch
    host = make_batch(w, rank, args.basis)
    eng = MatchEngine(local_rank)
    if args.p2p_split is not None:
        eng.set_option("p2p_split", args.p2p_split)
    dev = {n: torch.as_tensor(v).to(eng.device) for n, v in host.items()}
    N = w["nu"] * w["nv"]
    B, D, k = w["B"], w["D"], w["k"]
    extra = {}

    models = kernel_models(N, max(D, 1), k, B, eng)
    # Every workload goes through the library's sharded entry point (densematcher_amd/shard.py: run_sharded): this rank holds block
    # [rank B, (rank + 1) B) of a world x B batch (weak scaling: no rank builds the whole batch), results stay on the rank's device
    # (gather=False), no data-path collective.  With one rank this is the plain engine call.
    from densematcher_amd import shard
    blk = (rank * B, (rank + 1) * B, world * B)

    def sharded(method, local, **kw):
        return shard.run_sharded(method, local, lambda: eng, rank, world, gather=False, block=blk, **kw)
    if args.workload in ("fmap", "stress"):
        def step():
            return sharded("match", dev, k=k)
        out_name = ""
        split = eng.p2p_split_active(N, N, k)
        maps_kernel = ("simnn4_f16_mfma" if split >= 2 else "simnn2_f16_mfma") if split else "gred_f64"
        dtype = "f16" if split else "f64"
    elif args.workload == "simnn":
        sim_in = {"F2": dev["F2"], "F1": dev["F1"]}

        def step():
            return sharded("simnn", sim_in)["nn21"]
        out_name = "nn21"
        dtype = "f16"
    elif args.workload == "icp":
        gen = torch.Generator(device=eng.device).manual_seed(1 + rank)
        C0 = torch.eye(k, dtype=torch.float64, device=eng.device).repeat(B, 1, 1) \
            + 0.01 * torch.randn(B, k, k, dtype=torch.float64, device=eng.device, generator=gen)
        icp_in = {"Phi1": dev["Phi1"], "Phi2": dev["Phi2"], "C0": C0}

        def step():
            return sharded("icp", icp_in, nit=10)["C"]
        out_name = "C"
        dtype = "f16"
        models.update(refine_models("icp", N, k, B, eng))
    else:
        k0, nit = 50, 150
        C0 = torch.eye(k0, dtype=torch.float64, device=eng.device).repeat(B, 1, 1)
        zo_in = {"Phi1": dev["Phi1"], "Phi2": dev["Phi2"], "a2": dev["a2"], "C0": C0}

        def step():
            return sharded("zoomout", zo_in, nit=nit, step=1)["C"]
        out_name = "C"
        dtype = "f16"
        models.update(refine_models("zoomout", N, k, B, eng))

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if dist is None:
            return x
        tt = torch.tensor([x], dtype=torch.float64, device=eng.device if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    # which kernel dominates the step (its arithmetic is the line's dtype): untimed steps with every launch bracketed by HIP events
    wl_tag = args.workload if not args.batch else None
    dominant = dominant_kernel(eng, step)
    if models.get(dominant):
        dtype = models[dominant]["dtype"]          # the arithmetic type of the kernel that dominates the step
    # the headline: exactly `steps` steps, nothing bracketed inside
    elapsed, last = timed_steps(step, args.steps, args.warmup, barrier, max_over_ranks)
    value = B * world * args.steps / elapsed
    group_size = dist.get_world_size() if dist is not None else 1
    out = {
        "metric": "mesh-pairs/sec at N=2048 D=768 k=128" if args.workload == "fmap" else f"mesh-pairs/sec ({args.workload})",
        "value": round(value, 2), "unit": "mesh-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4), "ms_per_pair": round(1e3 * elapsed / (B * args.steps), 5),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
        "inputs": "device-resident (uploaded before the timed region; outputs stay on the device)",
        "config": {"workload": w["cfg"], "pairs_per_gpu": B, "N": N, "D": D, "k": k,
                   "basis_dtype": str(host["Phi1"].dtype) if "Phi1" in host else None,
                   "parallelism": f"pairs sharded over {world} GPU(s), one process per GPU, no data-path collective",
                   "process_group": (backend if dist is not None else None), "process_group_size": group_size},
        "timing": {"reported": "one block of exactly `steps` steps after `warmup` untimed ones, bracketed by barrier + synchronize (max over ranks)"},
    }
    if args.dump_outputs and rank == 0:
        out["outputs"] = dump_outputs(args.dump_outputs, output_arrays(last, out_name, {}))
    del last
    if not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return

    # --full: five more blocks of `steps` steps with the dominant kernel's launches bracketed by HIP events (the roofline's kernel time;
    # the median block prices the tables' share of the step)
    blocks_local = []
    median_s, launches, kernel_ms, blocks = timed_kernel(eng, step, dominant, args.steps, args.warmup, barrier, max_over_ranks=max_over_ranks,
                                                         local_out=blocks_local)
    # the per-kernel table, every kernel timed on its own, after the timed region
    table_steps = 2 if args.workload == "zoomout" else 10
    table, kernel_ms_per_step, launches_per_step = kernel_table(eng, step, table_steps, models, wl_tag, step_ms=1e3 * median_s / args.steps)
    avg_ms = kernel_ms / max(launches, 1)
    roof = roofline_block(dominant, models.get(dominant), launches, avg_ms, wl_tag, table, kernel_ms_per_step, launches_per_step, eng)
    kernels_table = roof.pop("kernels")
    # per-rank figures: every rank's five timed blocks, gathered over the process group when there is one
    my_blocks = [round(1e3 * b_ / args.steps, 4) for b_ in blocks_local]
    per_rank = {str(rank): my_blocks}
    if dist is not None:
        gathered = [None] * group_size
        dist.all_gather_object(gathered, my_blocks)
        per_rank = {str(r): g for r, g in enumerate(gathered)}
    details = {"kernels": kernels_table}
    summary = {}
    pcie = None
    if args.workload == "fmap" and not args.batch:
        if world == 1:
            pcie = pcie_inclusive(eng, host, dev, k, barrier)
        if not args.no_secondary:
            c3 = secondary_simnn(eng, rank, barrier, max_over_ranks, world)
            summary["config3_simnn"] = {q: c3[q] for q in ("value", "unit", "ms_per_step", "kernel", "avg_launch_ms", "achieved", "peak", "frac",
                                                           "frac_of_step", "frac_of_measured_peak_random_operands")}
            details["config3_simnn"] = c3
            if world == 1:
                hard = secondary_hard(eng, host, dev, k, barrier)
                details["config2_hard"] = hard
                summary["config2_hard_pairs_per_s"] = {n.split(" ")[0]: v["value"] for n, v in hard.items()}
                d64 = secondary_distinct(eng, k, barrier)
                details["config2_distinct64"] = d64
                summary["config2_distinct64"] = {q: d64.get(q) for q in ("value", "ms_per_step", "requeued_rows_fraction", "error") if q in d64}
                del dev
                torch.cuda.empty_cache()
                for key, which in (("config4_zoomout", "zoomout"), ("icp", "icp")):
                    blk = secondary_refine(eng, rank, barrier, which)
                    details[key] = blk
                    summary[key] = {q: blk[q] for q in ("value", "unit", "ms_per_step", "launches_per_step", "step10_nit15") if q in blk}
                blk = secondary_stress(eng, rank, barrier)
                details["config5_stress"] = blk
                summary["config5_stress"] = {q: blk[q] for q in ("value", "unit", "ms_per_step", "launches_per_step", "workspace_bytes")}
                sm = secondary_surface_map()
                details["surface_map"] = sm
                summary["surface_map"] = {"single_call_ms": sm.get("ms_per_call"), "single_stages_ms": sm.get("stages_ms"), "single_stages_note": sm.get("stages_note"),
                                          "batched_pairs_per_s": (sm.get("batched") or {}).get("value"),
                                          "batched_s_per_call": (sm.get("batched") or {}).get("s_per_call"),
                                          "batched_pairs_per_call": (sm.get("batched") or {}).get("pairs_per_call"),
                                          "batched_streams": (sm.get("batched") or {}).get("streams"),
                                          "robust_laplacian": "restated (opt-in: the robust_laplacian wheel is not installed on the box)",
                                          "error": sm.get("error") or (sm.get("batched") or {}).get("error")}
    # ---- the rest of the line.  Only its LAST 2 000 characters may be kept: the contract's keys come first, the long tables (`details`) in
    # the middle, and `roofline`, `cpu_baseline` and a compact `summary` (every secondary figure, <= 1 500 characters) at the very end
    out["pcie_inclusive_value"] = pcie["value"] if pcie else None
    out["timing"].update({"blocks": N_BLOCKS, "blocks_reported": "after the headline: blocks of exactly `steps` steps with the dominant kernel's "
                                                                  "launches bracketed by HIP events, each bracketed by barrier + synchronize (max over ranks per block)",
                          "blocks_ms_per_step": [round(1e3 * b_ / args.steps, 4) for b_ in blocks], "blocks_ms_per_step_by_rank": per_rank,
                          "kernel_ms_per_step_note": "kernel_ms_per_step in `roofline` is a sum of single-kernel HIP-event brackets taken after the timed "
                                                     "region: the brackets add about 2 %, so it can exceed ms_per_step"})
    if pcie:
        out["pcie_inclusive"] = pcie
    if args.workload == "fmap" and not args.batch and rank == 0:
        out["parity"] = parity_block(eng)
    details["summary_long"] = summary
    out["details"] = details
    out["roofline"] = roof
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args.workload, host, k)
    out["summary"] = compact_summary(summary, pcie)
    # (the headline's own figures once more, so that the kept tail of the line stands alone)
    out["summary"]["headline"] = {"pairs_s": out["value"], "step_ms": out["ms_per_step"], "kernel": roof.get("kernel"),
                                  "kernel_ms": roof.get("avg_launch_ms"), "frac": roof.get("frac"), "frac_executed": roof.get("frac_executed"),
                                  "traffic_B": roof.get("traffic"), "cpu_pairs_s": (out.get("cpu_baseline") or {}).get("value")}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def compact_summary(summary, pcie):
    """The secondary figures in <= 1 500 characters, printed as the LAST key of the line (the driver keeps the end of it).  Short keys:
    c3 = config 3 (feature NN), c4 = config 4 (ZoomOut 50 -> 200), c5 = config 5 (N = 8192 stress), sm = compute_surface_map."""
    def rnd(x, n=4):
        return round(x, n) if isinstance(x, float) else x
    s = {}
    c3 = summary.get("config3_simnn")
    if c3:
        s["c3"] = {"pairs_s": rnd(c3.get("value"), 1), "step_ms": rnd(c3.get("ms_per_step")), "kernel_ms": rnd(c3.get("avg_launch_ms")),
                   "frac": rnd(c3.get("frac")), "frac_step": rnd(c3.get("frac_of_step")),
                   "frac_meas_peak": rnd(c3.get("frac_of_measured_peak_random_operands"))}
    for key, short in (("config4_zoomout", "c4"), ("config5_stress", "c5"), ("icp", "icp")):
        blk = summary.get(key)
        if blk:
            s[short] = {"pairs_s": rnd(blk.get("value"), 1), "step_ms": rnd(blk.get("ms_per_step"), 3), "launches": blk.get("launches_per_step")}
            if blk.get("step10_nit15"):
                s[short]["step10_pairs_s"] = rnd(blk["step10_nit15"].get("value"), 1)
    sm = summary.get("surface_map")
    if sm:
        s["sm"] = {"single_ms": rnd(sm.get("single_call_ms"), 2), "batch_pairs_s": rnd(sm.get("batched_pairs_per_s"), 1),
                   "batch_s_per_call": rnd(sm.get("batched_s_per_call")), "pairs_per_call": sm.get("batched_pairs_per_call"),
                   "robust_laplacian": "restated"}
        if sm.get("error"):
            s["sm"]["error"] = str(sm["error"])[:120]
    d64 = summary.get("config2_distinct64")
    if d64:
        s["c2_distinct64"] = {"pairs_s": rnd(d64.get("value"), 1), "step_ms": rnd(d64.get("ms_per_step"))}
    hard = summary.get("config2_hard_pairs_per_s")
    if hard:
        s["c2_hard_pairs_s"] = {k_: rnd(v, 0) for k_, v in hard.items()}
    if pcie:
        s["pcie_inclusive_pairs_s"] = rnd(pcie.get("value"), 1)
    return s


def pcie_inclusive(eng, host, dev, k, barrier, steps=10):
    """The same step fed from HOST memory: every step's batch (0.67 GB) is uploaded from pinned host buffers on a second stream into
    the other of two device buffer sets while the current one is matched (double buffering).  value = pairs/s over `steps` steps,
    measured; never the headline (the contract's value has its inputs resident in HBM)."""
    import torch
    names = list(host)
    pinned = {n: torch.as_tensor(host[n]).pin_memory() for n in names}
    sets = [dev, {n: torch.empty_like(dev[n]) for n in names}]
    copy_stream = torch.cuda.Stream(device=eng.device)
    main = torch.cuda.current_stream(eng.device)
    ready = [torch.cuda.Event(), torch.cuda.Event()]
    freed = [torch.cuda.Event(), torch.cuda.Event()]
    B = host["F1"].shape[0]
    nbytes = sum(v.numel() * v.element_size() for v in pinned.values())

    def upload(slot):
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(freed[slot])
            for n in names:
                sets[slot][n].copy_(pinned[n], non_blocking=True)
            ready[slot].record(copy_stream)
    for slot in (0, 1):
        freed[slot].record(main)
    upload(0)
    barrier()
    t0 = time.perf_counter()
    for s in range(steps):
        slot = s & 1
        if s + 1 < steps:
            upload(slot ^ 1)
        main.wait_event(ready[slot])
        eng.match(sets[slot], k=k)
        freed[slot].record(main)
    barrier()
    dt = time.perf_counter() - t0
    # the upload alone
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for s in range(3):
        upload(s & 1)
        freed[s & 1].record(copy_stream)
    copy_stream.synchronize()
    up = (time.perf_counter() - t1) / 3
    return {"value": round(B * steps / dt, 2), "unit": "mesh-pairs/s", "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps,
            "upload_ms_per_batch": round(1e3 * up, 3), "upload_gb_per_s": round(nbytes / up / 1e9, 1), "bytes_per_batch": nbytes,
            "method": "pinned host buffers, upload of batch i + 1 on a second stream into the other of two device buffer sets while batch i is matched"}


def secondary_distinct(eng, k, barrier):
    """configs[1] once more on 64 DISTINCT mesh pairs (the headline's batch cycles two geometries: VERDICT r04 #8): 128 torus meshes with
    their own perturbations, cotangent Laplacians assembled on the device, eigenbases through dm_eigenbasis; value and the fraction of
    rows that took the exact path."""
    import torch
    try:
        from densematcher_amd import synth
        from densematcher_amd.pyFM.mesh import TriMesh
        w = WORKLOADS["fmap"]
        B, nu, nv, D = w["B"], w["nu"], w["nv"], w["D"]
        n = nu * nv
        t0 = time.perf_counter()
        meshes = [TriMesh(*synth.torus_mesh(nu, nv, perturb=0.02 + 0.06 * ((7 * q) % 10) / 10.0, seed=500 + q)) for q in range(2 * B)]
        half = B // 2
        for lo in range(0, 2 * B, half):                      # (k + guard = 160 vectors x 2048 vertices x 32 meshes per call)
            TriMesh.process_many(meshes[lo:lo + half], [k] * half, robust=False)
        setup = time.perf_counter() - t0
        host = {"Phi1": np.stack([m.eigenvectors for m in meshes[0::2]]), "Phi2": np.stack([m.eigenvectors for m in meshes[1::2]]),
                "lam1": np.stack([m.eigenvalues for m in meshes[0::2]]), "lam2": np.stack([m.eigenvalues for m in meshes[1::2]]),
                "a1": np.stack([m.A.diagonal() for m in meshes[0::2]]), "a2": np.stack([m.A.diagonal() for m in meshes[1::2]]),
                "F1": np.empty((B, n, D), np.float16), "F2": np.empty((B, n, D), np.float16)}
        for i in range(B):
            host["F1"][i], host["F2"][i], _ = synth.feature_pair(n, n, D, 1000 + i, 2000 + i, sigma=0.1, perm="identity")
        d = {q: torch.as_tensor(v).to(eng.device) for q, v in host.items()}

        def step():
            return eng.match(d, k=k)
        steps = 10
        elapsed, _, _, _ = timed_kernel(eng, step, "fm_split_exact_f64", steps, 2, barrier, n_blocks=3)
        step()
        rows = eng.last_requeued_rows()
        return {"value": round(B * steps / elapsed, 2), "unit": "mesh-pairs/s", "ms_per_step": round(1e3 * elapsed / steps, 4), "distinct_mesh_pairs": B,
                "requeued_rows_fraction": {nm: (round(r / (B * n), 5) if r >= 0 else None) for nm, r in zip(("knn21", "ind21", "knn12", "ind12"), rows)},
                "setup_s": round(setup, 2), "eigenbases": "128 cotangent Laplacians assembled on the device, dm_eigenbasis (k = 128 + 32 guard vectors)"}
    except Exception as e:       # informational block
        return {"error": repr(e)}


def dominant_kernel(eng, step, reps=3):
    """name of the kernel with the largest summed duration over `reps` steps (every launch bracketed, untimed); a few steps run
    first: the two largest kernels of config 2 are within 8 % of each other and a single cold step has named either"""
    import torch
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    eng.profile_kernel("*")
    for _ in range(reps):
        step()
    rep = eng.profile_report()
    eng.profile_kernel("")
    return max(rep.items(), key=lambda kv: kv[1][1])[0]


def refine_models(workload, N, k, B, eng):
    """SURVEY 8(d) work of the refinement loops' kernels per launch (mean over the iterations for ZoomOut's growing map)"""
    if workload == "icp":
        return {"simnn_f16_mfma": dict(dtype="f16", bound="mfma", what="nearest-neighbour search of one ICP iteration: 2 N^2 k (float64 flops of the reference)",
                                       flops=2.0 * N * N * k * B, executed=2.0 * N * N * eng.split_depth(k) * B),
                "p2pfm_tn_f64": dict(dtype="f64", bound="mfma", what="Phi2^T Phi1[p]: 2 N k^2", flops=2.0 * N * k * k * B),
                "embed_nt_f64": dict(dtype="f64", bound="mfma", what="embedding Phi1 C^T: 2 N k^2", flops=2.0 * N * k * k * B)}
    ks = range(50, 200)
    sd = lambda kk: 3 * 16 * (-(-kk // 16))          # split rows: three fp16 products per index, indices padded to 16 (depth >= 80 indices)
    return {
        "simnn1_f16_mfma": dict(dtype="f16", bound="mfma", what="nearest-neighbour search of one ZoomOut iteration: 2 N^2 k, mean over k = 50 .. 199",
                                flops=sum(2.0 * N * N * kk * B for kk in ks) / 150.0, executed=sum(2.0 * N * N * max(sd(kk), 240) * B for kk in ks) / 150.0),
        "simnn_f16_mfma": dict(dtype="f16", bound="mfma", what="nearest-neighbour search of one ZoomOut iteration: 2 N^2 k, mean over k = 50 .. 199",
                               flops=sum(2.0 * N * N * kk * B for kk in ks) / 150.0, executed=sum(2.0 * N * N * eng.split_depth(kk) * B for kk in ks) / 150.0),
        "p2pfm_tn_f64": dict(dtype="f64", bound="mfma", what="p2p_to_FM of one iteration: 2 N (k+1)^2, mean over k",
                             flops=sum(2.0 * N * (kk + 1) ** 2 * B for kk in ks) / 150.0),
        "zo_embed_split": dict(dtype="f64", bound="mfma", what="embedding Phi1 C^T of one iteration (+ split rows, norms): 2 N k^2, mean over k",
                               flops=sum(2.0 * N * kk * kk * B for kk in ks) / 150.0),
        "embed_nt_f64": dict(dtype="f64", bound="mfma", what="embedding of one iteration: 2 N k^2, mean over k",
                             flops=sum(2.0 * N * kk * kk * B for kk in ks) / 150.0)}


def secondary_refine(eng, rank, barrier, which):
    """configs[3] (ZoomOut 50 -> 200, step 1, 32 pairs per GPU) / spectral ICP (10 iterations, 64 pairs) in the same process:
    value (median of 3 blocks), launches and kernel time per step, the per-kernel table."""
    import torch
    w = dict(WORKLOADS[which])
    host = make_batch(w, rank)
    dev = {n: torch.as_tensor(v).to(eng.device) for n, v in host.items()}
    N, B, k = w["nu"] * w["nv"], w["B"], w["k"]
    if which == "zoomout":
        C0 = torch.eye(50, dtype=torch.float64, device=eng.device).repeat(B, 1, 1)

        def step():
            return eng.zoomout(dev["Phi1"], dev["Phi2"], dev["a2"], C0, nit=150, step=1)
        steps, tsteps = 3, 1
    else:
        gen = torch.Generator(device=eng.device).manual_seed(1 + rank)
        C0 = torch.eye(k, dtype=torch.float64, device=eng.device).repeat(B, 1, 1) \
            + 0.01 * torch.randn(B, k, k, dtype=torch.float64, device=eng.device, generator=gen)

        def step():
            return eng.icp(dev["Phi1"], dev["Phi2"], C0, nit=10)
        steps, tsteps = 5, 3
    models = refine_models(which, N, k, B, eng)
    elapsed, launches, kernel_ms, blocks = timed_kernel(eng, step, dominant_kernel(eng, step, reps=1), steps, 1, barrier, n_blocks=3)
    table, kms, nl = kernel_table(eng, step, tsteps, models, which, step_ms=1e3 * elapsed / steps)
    out = {"value": round(B * steps / elapsed, 2), "unit": "mesh-pairs/s", "ms_per_step": round(1e3 * elapsed / steps, 3), "steps": steps,
           "blocks_ms_per_step": [round(1e3 * b_ / steps, 3) for b_ in blocks],
           "config": {"workload": w["cfg"], "pairs_per_gpu": B, "N": N, "k": k, "basis_dtype": str(host["Phi1"].dtype)},
           "kernel_ms_per_step": round(kms, 3), "launches_per_step": round(nl, 1),
           "launches_per_iteration": round(nl / (150 if which == "zoomout" else 10), 2), "kernels": table}
    if which == "zoomout":
        # the same refinement in steps of ten (15 iterations: the maps of sizes 50, 60, ... 200), reported beside step 1
        def step10():
            return eng.zoomout(dev["Phi1"], dev["Phi2"], dev["a2"], C0, nit=15, step=10)
        el10, _, _, bl10 = timed_kernel(eng, step10, "simnn1_f16_mfma", 10, 2, barrier, n_blocks=3)
        out["step10_nit15"] = {"value": round(B * 10 / el10, 1), "unit": "mesh-pairs/s", "ms_per_step": round(1e3 * el10 / 10, 3), "steps": 10,
                               "blocks_ms_per_step": [round(1e3 * b_ / 10, 3) for b_ in bl10]}
    del dev
    torch.cuda.empty_cache()
    return out


def secondary_hard(eng, host, dev, k, barrier):
    """configs[1] on the HARD input distributions of SURVEY 8(d): sigma = 1.0 descriptors and the smooth (spectrally decaying)
    descriptors.  The exact float64 repair of the vertex maps is data dependent: value, the rows of each map that took it, and
    the time of the exact kernel, next to the default distribution (sigma = 0.1)."""
    import torch
    from densematcher_amd import synth
    B, n, D = host["F1"].shape
    out = {}

    def variant(name, F1, F2):
        d = dict(dev)
        d["F1"] = torch.as_tensor(F1).to(eng.device)
        d["F2"] = torch.as_tensor(F2).to(eng.device)

        def step():
            return eng.match(d, k=k)
        steps = 10
        elapsed, launches, kernel_ms, _ = timed_kernel(eng, step, "fm_split_exact_f64", steps, 2, barrier, n_blocks=3)
        step()
        rows = eng.last_requeued_rows()
        out[name] = {"value": round(B * steps / elapsed, 2), "unit": "mesh-pairs/s", "ms_per_step": round(1e3 * elapsed / steps, 4),
                     "requeued_rows_fraction": {nm: (round(r / (B * n), 5) if r >= 0 else None) for nm, r in zip(("knn21", "ind21", "knn12", "ind12"), rows)},
                     "fm_split_exact_f64_ms": round(kernel_ms / max(launches, 1), 4)}

    variant("sigma_0.1 (the headline's inputs)", host["F1"], host["F2"])
    F1 = np.empty_like(host["F1"]); F2 = np.empty_like(host["F2"])
    for i in range(B):
        F1[i], F2[i], _ = synth.feature_pair(n, n, D, 1000 + i, 2000 + i, sigma=1.0, perm="identity")
    variant("sigma_1.0", F1, F2)
    for i in range(B):
        F1[i], F2[i] = synth.smooth_feature_pair(host["Phi1"][i].astype(np.float64), host["Phi2"][i].astype(np.float64), D, 1000 + i, 2000 + i)
    variant("smooth (spectral coefficients ~ 1/sqrt(j), 5 % noise)", F1, F2)
    return out


def secondary_surface_map():
    """the documented call (compute_surface_map, notebook parameters) on one raw pair: GPU side only (the CPU restatement runs
    with --workload surface_map), median of 3 calls"""
    import io
    import contextlib
    buf = io.StringIO()
    a = argparse.Namespace(steps=3, warmup=1, no_cpu_baseline=True, full=True, dump_outputs=None)
    try:
        with contextlib.redirect_stdout(buf):
            surface_map_workload(a)
        r = json.loads(buf.getvalue().strip().splitlines()[-1])
        out = {"value": r["value"], "unit": "calls/s (one pair at a time)", "ms_per_call": r["ms_per_step"], "stages_ms": r["stages_ms"], "stages_note": r.get("stages_note"), "fit": r["fit"],
               "config": r["config"]}
    except Exception as e:       # informational block
        return {"error": repr(e)}
    try:
        out["batched"] = surface_map_batch_rate(64)
    except Exception as e:
        out["batched"] = {"error": repr(e)}
    return out


def surface_map_batch_rate(B):
    """throughput of the documented call through compute_surface_map_batch: B raw pairs (N = 2048, D = 512, notebook parameters,
    compute_extra=True) per call, every pair its own meshes and descriptors; one warm-up call, one timed call, stage times of the
    timed one.  Host work inside the call (Laplacian assembly of 2 B meshes, as in the reference) is part of the figure."""
    import warnings
    import torch
    from densematcher_amd import functional_map as fmod, synth
    from densematcher_amd.engine import MatchEngine
    from densematcher_amd.pyFM.mesh import TriMesh, laplacian as _lap
    _lap.set_robust_backend("restated")
    w = WORKLOADS["surface_map"]
    nu, nv, D, k = w["nu"], w["nv"], w["D"], w["k"]
    m1, m2, F1s, F2s = [], [], [], []
    for i in range(B):
        v1, f1 = synth.torus_mesh(nu, nv, perturb=0.03, seed=3 + 2 * i)
        v2, f2 = synth.torus_mesh(nu, nv, perturb=0.08, seed=4 + 2 * i)
        F1, F2, _ = synth.feature_pair(nu * nv, nu * nv, D, 1000 + i, 2000 + i, sigma=0.5, perm="identity")
        m1.append(_Duck(v1, f1)); m2.append(_Duck(v2, f2)); F1s.append(F1); F2s.append(F2)
    stages = {}

    def timed(name, fn):
        def wrapper(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(*a, **kw)
            torch.cuda.synchronize()
            stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
            return res
        return wrapper
    patched = [(TriMesh, "process_many", "eigenbases (2 B meshes: covers on host threads, assembly + one batched eigensolve on the device)", True),
               (MatchEngine, "fit_general", "fit (device L-BFGS over B maps)", False), (MatchEngine, "fm_to_p2p", "vertex maps (2 x 4 maps x B)", False),
               (MatchEngine, "precise_map", "precise maps", False), (MatchEngine, "icp", "ICP (10 iterations)", False),
               (MatchEngine, "mapped_indicator", "indicator matrices (2 B)", False),
               (MatchEngine, "lsa_indicator", "linear assignment (3 B matrices, one launch)", False),
               (MatchEngine, "linear_sum_assignment", "linear assignment (3 B matrices, one launch)", False)]
    def call(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = fmod.compute_surface_map_batch(m1, m2, F1s, F2s, n_ev=k, compute_extra=True, optimizer="L-BFGS-B", fit_params=dict(NOTEBOOK_FIT), **kw)
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    # the figure: the call as a user makes it (its default: one chunk stream per 64 pairs), no instrumentation; six warm-ups (the first call of a
    # process creates the chunk streams' engines and their workspaces, and the caching allocator takes a few calls to hold every block a
    # call needs: until then calls alternate between 305 and 340-375 ms), then the median of seven
    for _ in range(6):
        call()
    times = []
    for rep in range(7):
        res, dt = call()
        times.append(dt)
    t_call = float(np.median(times))
    # the stage times: one more call on ONE stream with every stage bracketed by device synchronisations (they would serialise the chunk
    # streams of the default call: this call is slower than the figure above and says where the time goes, not how long the call takes)
    saved = [(o, n, o.__dict__[n]) for o, n, _, _ in patched]
    for o, n, label, static in patched:
        fn = getattr(o, n)
        setattr(o, n, staticmethod(timed(label, fn)) if static else timed(label, fn))
    fmod.EARLY_ASSIGNMENTS = False          # (the instrumented call: all assignments in one launch at the end, nothing on side streams)
    try:
        stages.clear()
        _, t_one = call(streams=1)
    finally:
        fmod.EARLY_ASSIGNMENTS = True
        for o, n, fn in saved:
            setattr(o, n, fn)
    fr = res[0][7].fit_result
    return {"value": round(B / t_call, 2), "unit": "mesh-pairs/s", "pairs_per_call": B, "s_per_call": round(t_call, 3),
            "calls_s": [round(t, 3) for t in times], "streams": min(4, -(-B // 64)),
            "one_stream_instrumented_s_per_call": round(t_one, 3),
            "stages_ms_one_stream": {n: round(1e3 * v, 1) for n, v in stages.items()},
            "fit_evaluations_of_pair_0": int(getattr(fr, "nfev", [0])[0]),
            "timing_note": "median of seven calls after six warm-up calls (a process's first calls create the chunk streams' engines and let the caching "
                           "allocator collect the blocks a call needs: they alternate between the steady time and 30-70 ms more)",
            "note": "compute_surface_map_batch: the documented call (example.ipynb cell 11) for B raw pairs at once; every pair's 14-tuple equals the "
                    "single call's (tests/test_gpu_api.py::test_compute_surface_map_batch_equals_single_calls)"}


def roofline_block(kernel, model, launches, avg_ms, workload, table, kernel_ms_per_step, launches_per_step, eng):
    """`achieved` = SURVEY 8(d) ALGORITHMIC flops of one launch / its average duration inside the timed region; `peak` = the spec
    peak of the arithmetic the kernel runs in (MI355X_MICROARCH.md); the flops the matrix cores really execute (fp16 split) and
    the on-box measured peaks are separate keys."""
    traffic, traffic_file = pmc_traffic_bytes(kernel, workload) if workload else (None, None)
    out = {"bound": "mfma", "kernel": kernel, "launches": launches, "avg_launch_ms": round(avg_ms, 4),
           "kernel_ms_per_step": round(kernel_ms_per_step, 4), "launches_per_step": round(launches_per_step, 1)}
    if model and launches:
        peak = PEAK_TFLOPS[model["dtype"]]
        ach = model["flops"] / (avg_ms * 1e-3) / 1e12
        out.update(achieved=round(ach, 3), peak=peak, unit="TFLOP/s", frac=round(ach / peak, 4), dtype=model["dtype"],
                   algorithmic_flops_per_launch=model["flops"], algorithmic_work=model["what"])
        if "executed" in model:
            out["executed_flops_per_launch"] = model["executed"]
            out["frac_executed"] = round(model["executed"] / (avg_ms * 1e-3) / 1e12 / peak, 4)
    else:
        out.update(achieved=None, peak=None, unit="TFLOP/s", frac=None)
    out["traffic"] = traffic
    out["traffic_source"] = (f"HBM bytes per launch from the rocprofv3 PMC passes of this command on this code (profiles/{traffic_file}, "
                             f"csrc_sha16 {_SHA[0] if _SHA else None}: 2 x FETCH_SIZE + WRITE_SIZE, gfx950 correction)") if traffic else \
        "no PMC summary of this code under profiles/ (tools/prof_all_r06.sh writes one): not quoted"
    out["peak_measured"] = measured_peaks(eng)
    if out.get("achieved") and model["dtype"] == "f16":
        out["frac_of_measured_peak_random_operands"] = round(out["achieved"] / out["peak_measured"]["mfma_f16_random_operands_tflops"], 4)
    if out.get("achieved") and model["dtype"] == "f64":
        out["frac_of_measured_peak"] = round(out["achieved"] / out["peak_measured"]["mfma_f64_tflops"], 4)
    out["kernels"] = table
    return out


def secondary_simnn(eng, rank, barrier, max_over_ranks, world):
    """configs[2] (64 pairs, N = 2048, D = 768 feature-similarity NN) measured in the same process with the same method:
    the kernel north_star's MFMA-roofline target is about."""
    import torch
    w = WORKLOADS["simnn"]
    n, D, B = w["nu"] * w["nv"], w["D"], w["B"]
    feats = simnn_features(B, n, D, rank)
    F1 = torch.as_tensor(feats["F1"]).to(eng.device)
    F2 = torch.as_tensor(feats["F2"]).to(eng.device)
    steps, warmup = 10, 2
    elapsed, launches, kernel_ms, _ = timed_kernel(eng, lambda: eng.simnn(F2, F1), "simnn_f16_mfma", steps, warmup, barrier, n_blocks=3,
                                                   max_over_ranks=max_over_ranks)
    avg_ms = kernel_ms / max(launches, 1)
    flops = 2.0 * n * n * D * B
    ach = flops / (avg_ms * 1e-3) / 1e12
    traffic, tfile = pmc_traffic_bytes("simnn_f16_mfma", "simnn")
    pk = measured_peaks(eng)
    return {"value": round(B * world * steps / elapsed, 2), "unit": "mesh-pairs/s", "ms_per_step": round(1e3 * elapsed / steps, 4),
            "steps": steps, "warmup": warmup, "dtype": "f16", "config": {"workload": w["cfg"], "pairs_per_gpu": B, "N": n, "D": D},
            "kernel": "simnn_f16_mfma", "avg_launch_ms": round(avg_ms, 4), "algorithmic_flops_per_launch": flops, "achieved": round(ach, 3),
            "peak": PEAK_TFLOPS["f16"], "unit_roofline": "TFLOP/s", "frac": round(ach / PEAK_TFLOPS["f16"], 4),
            "frac_of_measured_peak_random_operands": round(ach / pk["mfma_f16_random_operands_tflops"], 4),
            "frac_of_step": round(flops / (elapsed / steps) / 1e12 / PEAK_TFLOPS["f16"], 4),   # the same flops over the whole step (kernel + merge + exact repair)
            "traffic": traffic, "traffic_file": ("profiles/" + tfile) if tfile else None}


def secondary_stress(eng, rank, barrier):
    """configs[4] (64 pairs, N = 8192, D = 384, k = 200), 3 timed steps in the same process: value and its kernel table."""
    import torch
    w = dict(WORKLOADS["stress"])
    host = make_batch(w, rank)
    dev = {n: torch.as_tensor(v).to(eng.device) for n, v in host.items()}
    N, B, D, k = w["nu"] * w["nv"], w["B"], w["D"], w["k"]

    def step():
        return eng.match(dev, k=k)
    models = kernel_models(N, D, k, B, eng)
    steps = 3
    elapsed, launches, kernel_ms, _ = timed_kernel(eng, step, dominant_kernel(eng, step, reps=1), steps, 1, barrier, n_blocks=3)
    table, kms, nl = kernel_table(eng, step, 2, models, "stress", step_ms=1e3 * elapsed / steps)
    out = {"value": round(B * steps / elapsed, 2), "unit": "mesh-pairs/s", "ms_per_step": round(1e3 * elapsed / steps, 3), "steps": steps,
           "config": {"workload": w["cfg"], "pairs_per_gpu": B, "N": N, "D": D, "k": k}, "kernel_ms_per_step": round(kms, 3),
           "launches_per_step": round(nl, 1), "workspace_bytes": eng.workspace_bytes(), "kernels": table}
    del dev
    torch.cuda.empty_cache()
    return out


def parity_block(eng):
    """C of the committed config-2 fixture (reference-generated, tools/make_golden.py) through the GPU path."""
    try:
        from densematcher_amd import synth
        fx = dict(np.load(os.path.join(REPO, "tests", "golden", "fx_cfg2.npz"), allow_pickle=False))
        n, kk = fx["Phi1"].shape[0], int(fx["k"])
        s1, s2 = (int(x) for x in fx["feat_seeds"])
        F1, F2, _ = synth.feature_pair(n, n, int(fx["D"]), s1, s2, sigma=float(fx["feat_sigma"]), perm="identity")
        b = {"Phi1": fx["Phi1"][None], "Phi2": fx["Phi2"][None], "lam1": fx["lam1"][None], "lam2": fx["lam2"][None],
             "a1": fx["a1"][None], "a2": fx["a2"][None], "F1": F1[None], "F2": F2[None]}
        import torch
        dev = {k_: torch.as_tensor(v).to(eng.device) for k_, v in b.items()}
        res = eng.match(dev, k=kk, w_descr=float(fx["w_descr"]), w_lap=float(fx["w_lap"]))
        C = res["C"][0].cpu().numpy()
        agree = {nm: float((res[nm][0].cpu().numpy() == fx["f64_" + nm]).mean()) for nm in ("knn21", "knn12", "ind21", "ind12")}
        return {"fixture": "tests/golden/fx_cfg2.npz (N=2048, D=768, k=128; outputs of the reference, tools/make_golden.py)",
                "max_abs_C_minus_C_f64": float(np.abs(C - fx["C_f64"]).max()), "bar": 1e-4,
                "max_abs_C_minus_C_fit_reference_fp32_lbfgs": float(np.abs(C - fx["C_fit"]).max()),
                "map_agreement_with_oracle_maps_of_C_f64": agree}
    except Exception as e:       # the bench line must not die on the informational block
        return {"error": repr(e)}


ROUND = "r06"


def csrc_sha16():
    """sha256 (16 hex digits) over the kernel sources: a committed PMC summary is only quoted while it belongs to this code"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(REPO, "densematcher_amd", "csrc")
    for f in sorted(os.listdir(d)):
        h.update(f.encode())
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


_SHA = []


def pmc_traffic_bytes(kernel, workload):
    """HBM bytes per launch of a kernel, measured in separate rocprofv3 --pmc passes of this same command (PMC collection cannot
    run inside the timed region; tools/prof_all_r06.sh), summaries committed under profiles/.  Only THIS round's summary is read,
    and only when its `# csrc_sha16:` line equals the hash of the kernel sources now in the tree: a number measured on other code
    is not quoted -- the caller then reports traffic = null."""
    import csv
    import re

    def dual_of(name):           # third template argument of simnn_pipe_kernel<XV, WT, DUAL, ...>: 0 one key, 1 two keys, 3 both directions, 4 one biased key
        mt = re.search(r"simnn_pipe_kernel<\d+, \d+, (\d+)", name)
        return int(mt.group(1)) if mt else None
    match = {"gred_f64": lambda n: "gred_kernel" in n,
             "fmap_solve_chol": lambda n: "fmap_solve" in n and "pcg" not in n,
             "fmap_solve_pcg": lambda n: "fmap_solve_pcg" in n,
             "embed_nt_f64": lambda n: "embed_tile_kernel" in n,
             "project_f16split_mfma": lambda n: "proj_f16split_kernel" in n,
             "gram_nt_f64": lambda n: "gemm_nt_f64" in n and "OutScaled" in n,
             "p2pfm_tn_f64": lambda n: "p2pfm_direct_kernel" in n,
             "simnn_f16_mfma": lambda n: dual_of(n) == 0,
             "simnn2_f16_mfma": lambda n: dual_of(n) == 1,
             "simnn4_f16_mfma": lambda n: dual_of(n) == 3,
             "simnn1_f16_mfma": lambda n: dual_of(n) == 4}.get(kernel, lambda n: kernel in n)
    if not _SHA:
        _SHA.append(csrc_sha16())
    fname = f"{ROUND}_{workload}_hbm_traffic_pmc.csv"
    path = os.path.join(REPO, "profiles", fname)
    try:
        lines = open(path).read().splitlines()
        sha = [ln.split(":", 1)[1].strip() for ln in lines if ln.startswith("# csrc_sha16:")]
        if not sha or sha[0] != _SHA[0]:
            return None, None
        rows = [r for r in csv.reader(ln for ln in lines if not ln.startswith("#"))]
        hdr = rows[0]
        tot, cnt = 0.0, 0
        for r in rows[1:]:
            if match(r[0]):                     # (a kernel name may cover several instantiations: dispatch-weighted mean)
                d = dict(zip(hdr, r))
                nd = int(d["dispatches"])
                tot += nd * (float(d["fetch_MB_corrected"]) + float(d["write_MB"]))
                cnt += nd
        if cnt:
            return int(tot / cnt * 1e6), fname
    except Exception:
        pass
    return None, None


def _median_rate(fn, budget_s, min_reps=3):
    """fn() processes one pair; repeat for about budget_s (at least min_reps), return (median pairs/s, reps, total s)."""
    times = []
    t_all = time.perf_counter()
    while len(times) < min_reps or (time.perf_counter() - t_all) < budget_s:
        t0 = time.perf_counter()
        fn(len(times))
        times.append(time.perf_counter() - t0)
        if len(times) >= 64:
            break
    return 1.0 / float(np.median(times)), len(times), time.perf_counter() - t_all


def cpu_baseline(workload, host, k):
    """The NumPy float64 oracle on the host cores, bounded sample.  "port" = the arithmetic the GPU path uses (closed-form
    solve, brute-force GEMM nearest neighbour, no N x N matrix kept); "reference_faithful" = the reference's own algorithm
    choices restated (iterative L-BFGS-B on the energy, sklearn kd-tree nearest neighbours, dense N2 x N1 indicator + two
    arg-maxes), BASELINE.md section 3.  Medians over >= 3 repetitions, one pair per repetition."""
    from oracle import dm_oracle as orc
    ncores = os.cpu_count() or 1
    nb = host["F1"].shape[0] if "F1" in host else host["Phi1"].shape[0]
    faithful = None
    if workload in ("fmap", "stress"):
        def pair(i):
            i %= nb
            orc.match_pair(host["Phi1"][i][:, :k], host["Phi2"][i][:, :k], host["lam1"][i][:k], host["lam2"][i][:k],
                           host["a1"][i], host["a2"][i], host["F1"][i], host["F2"][i])

        def pair_faithful(i):
            i %= nb
            orc.match_pair_reference_faithful(host["Phi1"][i][:, :k], host["Phi2"][i][:, :k], host["lam1"][i][:k],
                                              host["lam2"][i][:k], host["a1"][i], host["a2"][i], host["F1"][i], host["F2"][i])
        rate, reps, dt = _median_rate(pair, 8.0)
        what = "project + closed-form solve + 4 maps (oracle.match_pair)"
        if workload == "fmap":
            frate, freps, fdt = _median_rate(pair_faithful, 10.0)
            faithful = {"value": round(frate, 4), "unit": "mesh-pairs/s", "cores": ncores, "kind": "port",
                        "sample": f"median of {freps} pairs, project + L-BFGS-B (float64 energy / analytic gradient, SciPy defaults of "
                                  f"the reference call) + 2 sklearn kd-tree queries + dense 2048 x 2048 indicator + 2 arg-maxes "
                                  f"(oracle.match_pair_reference_faithful), {fdt:.1f} s"}
    elif workload == "simnn":
        rate, reps, dt = _median_rate(lambda i: orc.simnn(host["F2"][i % nb], host["F1"][i % nb]), 10.0)
        what = "float64 GEMM + argmax (oracle.simnn)"
    elif workload == "icp":
        rate, reps, dt = _median_rate(lambda i: orc.icp_refine(np.eye(k), host["Phi1"][i % nb][:, :k], host["Phi2"][i % nb][:, :k], nit=10), 10.0)
        what = "spectral ICP, 10 iterations (oracle.icp_refine: brute-force NN, lstsq, SVD)"
    else:
        rate, reps, dt = _median_rate(lambda i: orc.zoomout_refine(np.eye(50), host["Phi1"][i % nb], host["Phi2"][i % nb], nit=150,
                                                                   step=1, a2=host["a2"][i % nb]), 10.0, min_reps=1)
        what = "ZoomOut 50->200 step 1 (oracle.zoomout_refine)"
    out = {"value": round(rate, 4), "unit": "mesh-pairs/s", "cores": ncores, "kind": "port",
           "sample": f"median of {reps} pairs of the same workload, {what}, NumPy/BLAS threads on {ncores} host cores, {dt:.1f} s"}
    if faithful:
        out["reference_faithful"] = faithful
    return out


if __name__ == "__main__":
    main()

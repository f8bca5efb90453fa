#!/usr/bin/env python
"""
Fixture of the map quality measures, produced by RUNNING THE REFERENCE's three functions (densematcher/pyFM/eval/evaluate.py:
accuracy, continuity, coverage) on the CPU:

    python tools/make_golden_eval.py <checkout of the reference>

evaluate.py imports only NumPy, so the file is loaded by its path (not through the package, whose other modules import rendering
packages).  Nothing of its text is stored: the fixture holds inputs made here and the numbers the functions returned.

    tests/golden/fx_eval.npz
      case a, on small_D of fx_geod.npz (160 vertices, heat method, asymmetric):
        a_p2p, a_gt            seeded maps of 160 entries, with repeats (a_p2p reaches 102 of the 160 vertices)
        a_p2p_long, a_gt_long  the same with 257 entries
        a_acc, a_dists                 accuracy(a_p2p, a_gt, small_D, return_all=True)
        a_acc_scaled, a_dists_scaled   the same with sqrt_area = a_sqrt_area
        a_acc_long, a_dists_long, a_acc_long_scaled, a_dists_long_scaled    the 257-entry maps
        a_cont                 continuity(a_p2p, small_D, small_D, small_edges): inf -- the heat method gives some neighbours the
                               distance 0 (its phi -= min phi puts the zero at the minimum, which is not always the source)
        a_edges_pos, a_cont_pos    the edges of small_edges with a positive length, and the continuity on them (finite)
        a_area                 a seeded positive diagonal; a_cov, a_cov_long = coverage(map, diag(a_area))
      case b, on b_D of fx_groups.npz (96 x 96 small integers, zeros off the diagonal):
        b_p2p, b_edges_inf, b_edges_nan    a map and two edge lists: one holds an edge of target length 0 whose image has a
                               positive length (the reference returns inf), the other also one whose image has length 0 (nan)
        b_cont_inf, b_cont_nan continuity(b_p2p, b_D, b_D, edges)
        b_acc_p2p, b_acc_gt, b_acc, b_dists    an accuracy whose elements tie
"""
import importlib.util
import os
import sys

import numpy as np
import scipy.sparse as sparse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_module(root):
    path = os.path.join(root, "densematcher", "pyFM", "eval", "evaluate.py")
    spec = importlib.util.spec_from_file_location("reference_evaluate", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DENSEMATCHER_REFERENCE")
    if not root:
        raise SystemExit(__doc__)
    ref = reference_module(root)
    golden = os.path.join(REPO, "tests", "golden")
    geod = dict(np.load(os.path.join(golden, "fx_geod.npz")))
    D, edges = geod["small_D"], geod["small_edges"].astype(np.int64)
    n = D.shape[0]
    out = {}

    rng = np.random.default_rng(160)
    out["a_sqrt_area"] = np.float64(1.7320508075688772)
    for tag, length in (("", n), ("_long", 257)):
        p2p, gt = rng.integers(0, n, length), rng.integers(0, n, length)
        assert len(np.unique(p2p)) < min(n, length)
        out["a_p2p" + tag], out["a_gt" + tag] = p2p, gt
        out["a_acc" + tag], out["a_dists" + tag] = ref.accuracy(p2p, gt, D, return_all=True)
        out["a_acc" + tag + "_scaled"], out["a_dists" + tag + "_scaled"] = ref.accuracy(p2p, gt, D, return_all=True,
                                                                                       sqrt_area=out["a_sqrt_area"])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["a_cont"] = ref.continuity(out["a_p2p"], D, D, edges)
    out["a_edges_pos"] = edges[D[edges[:, 0], edges[:, 1]] > 0]
    out["a_cont_pos"] = ref.continuity(out["a_p2p"], D, D, out["a_edges_pos"])
    assert np.isfinite(out["a_cont_pos"]) and 400 < len(out["a_edges_pos"]) < len(edges)
    out["a_area"] = rng.uniform(0.5, 2.0, n)
    A = sparse.diags(out["a_area"]).tocsr()
    out["a_cov"], out["a_cov_long"] = ref.coverage(out["a_p2p"], A), ref.coverage(out["a_p2p_long"], A)

    bD = dict(np.load(os.path.join(golden, "fx_groups.npz")))["b_D"]
    m = bD.shape[0]
    rng = np.random.default_rng(96)
    p2p = rng.permutation(m)
    img = bD[p2p[:, None], p2p[None, :]]                      # length of the image of the edge (i, j)
    off = ~np.eye(m, dtype=bool)
    pos = np.argwhere(off & (bD > 0))
    zero_inf = np.argwhere(off & (bD == 0) & (img > 0))
    zero_nan = np.argwhere(off & (bD == 0) & (img == 0))
    assert len(zero_inf) and len(zero_nan)
    plain = pos[rng.permutation(len(pos))[:70]]
    e_inf = np.concatenate([plain[:35], zero_inf[:2], plain[35:]])
    e_nan = np.concatenate([plain[:20], zero_inf[:1], zero_nan[:1], plain[20:]])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["b_cont_inf"], out["b_cont_nan"] = ref.continuity(p2p, bD, bD, e_inf), ref.continuity(p2p, bD, bD, e_nan)
    assert np.isposinf(out["b_cont_inf"]) and np.isnan(out["b_cont_nan"])
    out["b_p2p"], out["b_edges_inf"], out["b_edges_nan"] = p2p, e_inf, e_nan
    out["b_acc_p2p"], out["b_acc_gt"] = rng.integers(0, m, 130), rng.integers(0, m, 130)
    out["b_acc"], out["b_dists"] = ref.accuracy(out["b_acc_p2p"], out["b_acc_gt"], bD, return_all=True)
    assert len(np.unique(out["b_dists"])) <= 4

    path = os.path.join(golden, "fx_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

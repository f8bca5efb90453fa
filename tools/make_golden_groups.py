#!/usr/bin/env python
"""
Fixture of the semantic group distances, produced by RUNNING THE REFERENCE's two functions (densematcher/utils.py:115-143:
get_distance_between_groups, get_groups_dmtx) on the CPU:

    python tools/make_golden_groups.py <checkout of the reference>

That module imports pytorch3d, meshplot and other rendering packages at its top; only the two function definitions are taken
from it (parsed with `ast`, executed in a namespace that provides np, os and scipy's linear_sum_assignment).  Nothing of its text
is stored: the fixture holds inputs made here and the numbers the functions returned.

    tests/golden/fx_groups.npz
        a_flat, a_off   six groups on the 160-vertex mesh of fx_geod.npz (its heat-method matrix small_D, asymmetric): Voronoi
                        groups of five farthest-point seeds, with an EMPTY group inserted at position 2; group g is
                        a_flat[a_off[g]:a_off[g + 1]]
        a_dmtx          get_groups_dmtx(small_D, groups)  (6, 6)
        b_D             (96, 96) matrix of small integers (0..3) as float64: ties everywhere, not symmetric
        b_flat, b_off   five groups with repeated indices, overlapping each other, not covering every vertex
        b_dmtx          get_groups_dmtx(b_D, groups)  (5, 5)
"""
import ast
import os
import sys

import numpy as np
from scipy.optimize import linear_sum_assignment

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import groups_restate as gr  # noqa: E402

NAMES = ("get_distance_between_groups", "get_groups_dmtx")


def reference_functions(root):
    path = os.path.join(root, "densematcher", "utils.py")
    tree = ast.parse(open(path).read(), path)
    keep = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in NAMES]
    assert sorted(n.name for n in keep) == sorted(NAMES), [n.name for n in keep]
    ns = {"np": np, "os": os, "linear_sum_assignment": linear_sum_assignment}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["get_distance_between_groups"], ns["get_groups_dmtx"]


def pack(groups):
    off = np.cumsum([0] + [len(g) for g in groups]).astype(np.int64)
    flat = np.asarray([i for g in groups for i in g], np.int64)
    return flat, off


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DENSEMATCHER_REFERENCE")
    if not root:
        raise SystemExit(__doc__)
    _, ref_dmtx = reference_functions(root)
    geod = dict(np.load(os.path.join(REPO, "tests", "golden", "fx_geod.npz")))
    D = geod["small_D"]
    groups_a = gr.voronoi_groups(D, 5)
    groups_a.insert(2, [])
    a_dmtx = ref_dmtx(D, groups_a)

    rng = np.random.default_rng(96)
    b_D = rng.integers(0, 4, (96, 96)).astype(np.float64)
    groups_b = [rng.integers(0, 40, 30).tolist(),            # repeats inside a group
                list(range(20, 60)),                          # overlaps the first and the third
                rng.permutation(np.arange(50, 90))[:17].tolist(),
                [5, 5, 5, 70, 71],
                rng.integers(30, 80, 64).tolist()]
    assert len(set(i for g in groups_b for i in g)) < 96
    b_dmtx = ref_dmtx(b_D, groups_b)

    a_flat, a_off = pack(groups_a)
    b_flat, b_off = pack(groups_b)
    out = os.path.join(REPO, "tests", "golden", "fx_groups.npz")
    np.savez_compressed(out, a_flat=a_flat, a_off=a_off, a_dmtx=a_dmtx, b_D=b_D, b_flat=b_flat, b_off=b_off, b_dmtx=b_dmtx)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

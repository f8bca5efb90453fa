"""Shared by tests/test_energy_plan_cpu.py and tests/test_gpu_energy_routes.py (no GPU needed to import this).

dm_fmap_energy_grad (densematcher_amd/csrc/dm_energy.hip) chooses its work decomposition at run time from
(B, N1, N2, k1, k2, weights, n_cu).  This module holds
  * plan(): a Python restatement of that choice, written from the description in include/densematch.h (dm_fmap_energy_plan) --
    an independent definition, not a ctypes call -- so that a test can say which route a case takes on any CU count;
  * pick_B(): the smallest batch whose plan has a wanted (rg, ncs);
  * make_case(): random operands with the scaling of test_energy_indicator_terms_ragged (tests/test_gpu_api.py);
  * the case table: the smallest shapes at which each route exists.
"""
import numpy as np

WEIGHT_ORDER = ("w_descr", "w_lap", "w_dcomm", "w_p2p", "w_stochastic", "w_ent", "w_range01", "w_sumto1", "w_area", "w_conformal")
PLAN_FIELDS = ("rg", "ncs", "cchunk", "ngroups", "stats_route", "cp_inline", "e2_inline", "nt2", "kc_m", "nsplit_m", "nsplit_d", "m_terms")
# fields that follow from the map's sizes and the weights alone: the same for every batch size and CU count
SIZE_ONLY_FIELDS = ("kc_m", "nsplit_m", "cp_inline", "e2_inline", "nt2", "nsplit_d", "stats_route", "m_terms")
M_TERMS = ("w_p2p", "w_stochastic", "w_ent", "w_range01", "w_sumto1")


def cdiv(a, b):
    return -(-a // b)


def weight_array(w):
    return [float(w.get(n, 0.0)) for n in WEIGHT_ORDER]


def plan(n_cu, B, N1, N2, k1, k2, weights, n_ops=0):
    """The plan as a dict of PLAN_FIELDS, or ValueError for what dm_fmap_energy_grad refuses."""
    w = {n: float(weights.get(n, 0.0)) for n in WEIGHT_ORDER}
    if min(B, N1, N2, k1, k2) <= 0 or any(v < 0 for v in w.values()):
        raise ValueError("sizes must be positive, weights >= 0")
    m_terms = any(w[n] > 0 for n in M_TERMS)
    if w["w_dcomm"] > 0 and (n_ops <= 0 or B * n_ops > 65535):
        raise ValueError("w_dcomm needs 1 <= B * n_ops <= 65535")
    if B > 65535:
        raise ValueError("batch too large")
    if m_terms and k1 > 256:
        raise ValueError("the indicator terms need k1 <= 256")
    out = dict.fromkeys(PLAN_FIELDS, 0)
    out["m_terms"] = int(m_terms)
    out["cp_inline"] = int(k1 <= 32 and k2 <= 32)
    out["nsplit_d"] = cdiv(n_ops * k2, 512) if w["w_dcomm"] > 0 else 0
    if not m_terms:
        return out
    target = 4 * (n_cu if n_cu > 0 else 256)            # workgroups wanted: four per CU
    rg = 512
    while rg > 64 and B * cdiv(N2, rg) < target:        # whole-row sweeps for a batch, one 64-row block for a single pair
        rg //= 2
    ncs, max_split = 1, max(1, cdiv(N1, 128))           # a split keeps at least two 64-column tiles
    while ncs < max_split and B * cdiv(N2, 64) * ncs < target:
        ncs *= 2
    stats = w["w_stochastic"] > 0 or w["w_sumto1"] > 0
    route = 0 if not stats else (1 if w["w_stochastic"] == 0 and k2 <= 256 else 2)
    kc_m = 128 if (k1 <= 64 and k2 <= 64) else 512
    out.update(rg=rg, ncs=ncs, cchunk=cdiv(cdiv(N1, ncs), 64) * 64, ngroups=cdiv(N2, rg), stats_route=route,
               e2_inline=int(route == 1 and k1 <= 32 and k2 <= 32), nt2=1 if k1 <= 64 else 2 if k1 <= 128 else 4,
               kc_m=kc_m, nsplit_m=cdiv(N2, kc_m))
    return out


def pick_B(target_rg, target_ncs, N1, N2, n_cu, cap=1024):
    """the smallest B <= cap whose plan has (rg, ncs) = the target on a device of n_cu CUs; None if there is none"""
    w = {"w_stochastic": 1.0}
    for B in range(1, cap + 1):
        p = plan(n_cu, B, N1, N2, 16, 16, w)
        if (p["rg"], p["ncs"]) == (target_rg, target_ncs):
            return B
    return None


def make_case(seed, B, N1, N2, k1, k2, D, n_ops=0):
    """Operands of B different pairs (the scaling of test_energy_indicator_terms_ragged): bases / sqrt(N), masses uniform in
    [0.5, 1.5] / N, C = 3 randn, sorted spectra in [0, 50]; n_ops > 0 adds random operator lists (B, n_ops, k, k) / sqrt(k).
    Pair b is the same whatever B is asked for with the same seed and sizes (each pair has its own generator)."""
    keys = ("e1", "e2", "a1", "C", "A", "Bm", "lam1", "lam2", "ops1", "ops2")
    rows = {n: [] for n in keys}
    for b in range(B):
        rng = np.random.default_rng([seed, b, N1, N2, k1, k2])
        rows["e1"].append((rng.standard_normal((N1, k1)) / np.sqrt(N1)).astype(np.float32))
        rows["e2"].append((rng.standard_normal((N2, k2)) / np.sqrt(N2)).astype(np.float32))
        rows["a1"].append((rng.uniform(0.5, 1.5, N1) / N1).astype(np.float32))
        rows["C"].append(rng.standard_normal((k2, k1)) * 3.0)
        rows["A"].append(rng.standard_normal((k1, D)).astype(np.float32))
        rows["Bm"].append(rng.standard_normal((k2, D)).astype(np.float32))
        rows["lam1"].append(np.sort(rng.uniform(0, 50, k1)))
        rows["lam2"].append(np.sort(rng.uniform(0, 50, k2)))
        rows["ops1"].append(rng.standard_normal((n_ops, k1, k1)) / np.sqrt(k1))
        rows["ops2"].append(rng.standard_normal((n_ops, k2, k2)) / np.sqrt(k2))
    out = {n: np.stack(v) for n, v in rows.items()}
    if n_ops == 0:
        out["ops1"] = out["ops2"] = None
    return out


# ---- weight sets -----------------------------------------------------------------------------------------------------
W_ENT = {"w_ent": 0.3}
W_SUM = {"w_sumto1": 2.0}
W_STO = {"w_stochastic": 0.7}
W_P2P_RANGE = {"w_p2p": 0.5, "w_range01": 1.5}
W_FULL = {"w_p2p": 0.5, "w_stochastic": 0.7, "w_ent": 0.3, "w_range01": 1.5, "w_sumto1": 2.0, "w_descr": 1.0, "w_lap": 0.1}
W_STO_SUM = {"w_stochastic": 0.7, "w_sumto1": 2.0}
W_QUAD = {"w_descr": 1.0, "w_lap": 0.1}
W_DCOMM = {"w_dcomm": 0.8}
W_DCOMM_QUAD = {"w_dcomm": 0.8, "w_descr": 1.0, "w_lap": 0.1}
W_AREA = {"w_area": 2.0}
W_CONF = {"w_conformal": 3.0}
W_SHAPE_ENT = {"w_area": 2.0, "w_conformal": 3.0, "w_ent": 0.3}
RAGGED_SETS = (W_ENT, W_SUM, W_STO, W_P2P_RANGE, W_FULL)          # the five of test_energy_indicator_terms_ragged; the last is the full mix
SWEEP_SETS = (W_STO, W_STO_SUM, W_FULL)                           # rg only matters on the tile statistics route
INLINE_SETS = (W_SUM, W_STO_SUM, W_ENT)
SHAPE_SETS = (W_AREA, W_CONF, W_SHAPE_ENT)
ALL_WEIGHT_SETS = (W_ENT, W_SUM, W_STO, W_P2P_RANGE, W_FULL, W_STO_SUM, W_QUAD, W_DCOMM, W_DCOMM_QUAD, W_AREA, W_CONF, W_SHAPE_ENT)

# ---- the case table --------------------------------------------------------------------------------------------------
# id, sizes, the batch (a number, or the (rg, ncs) target pick_B finds a batch for), the weight sets, and what the plan must say
# (`expect`: plan fields that hold on any device; targets are reached through pick_B with the device's CU count).
SWEEP_SHAPE = dict(N1=200, N2=600, k1=20, k2=17, D=8)             # two groups at rg = 512 (the second: 88 rows = two blocks, the last
SWEEP_TARGETS = ((64, 2), (64, 1), (128, 1), (256, 1), (512, 1))  # ragged); four column tiles, the last with 8 columns
SWEEP_FIRST_B_256CU = {(64, 2): 1, (64, 1): 103, (128, 1): 205, (256, 1): 342, (512, 1): 512}


def _case(id, N1, N2, k1, k2, D, B, sets, n_ops=0, expect=None, target=None):
    return dict(id=id, N1=N1, N2=N2, k1=k1, k2=k2, D=D, B=B, sets=sets, n_ops=n_ops, expect=expect or {}, target=target)


CASES = [_case("sweep_rg%d_ncs%d" % t, B=None, target=t, sets=SWEEP_SETS, expect={"stats_route": 2, "nt2": 1}, **SWEEP_SHAPE)
         for t in SWEEP_TARGETS]
CASES += [
    # one full 512-row group, max_split = 1 (ncs = 1 at any batch)
    _case("exact_multiples_rg512", 128, 512, 16, 12, 4, None, (W_STO, W_FULL), target=(512, 1), expect={"stats_route": 2, "ngroups": 1, "cchunk": 128}),
    # ncs = 4, cchunk = 128: split 3 starts at column 384 >= N1
    _case("empty_trailing_split", 300, 517, 20, 33, 8, 1, RAGGED_SETS, expect={"cchunk": 128}, target=(64, 4)),
]
for _B in (1, 2):
    CASES += [
        _case("nt2_k64_B%d" % _B, 70, 65, 64, 64, 8, _B, RAGGED_SETS, expect={"nt2": 1, "kc_m": 128}),
        _case("nt2_k65_B%d" % _B, 70, 65, 65, 40, 8, _B, RAGGED_SETS, expect={"nt2": 2, "kc_m": 512}),
        _case("nt2_k128_B%d" % _B, 130, 129, 128, 128, 8, _B, RAGGED_SETS, expect={"nt2": 2}),
        _case("nt2_k129_B%d" % _B, 130, 129, 129, 60, 8, _B, RAGGED_SETS, expect={"nt2": 4}),
        _case("nt2_k256_B%d" % _B, 200, 130, 256, 40, 8, _B, RAGGED_SETS, expect={"nt2": 4}),
        _case("quad_only_k300_B%d" % _B, 1, 1, 300, 280, 8, _B, (W_QUAD,), expect={"m_terms": 0, "cp_inline": 0}),
    ]
CASES += [
    _case("inline_32x32", 129, 65, 32, 32, 8, 2, INLINE_SETS, expect={"cp_inline": 1}),
    _case("inline_33x32", 129, 65, 33, 32, 8, 2, INLINE_SETS, expect={"cp_inline": 0, "e2_inline": 0}),
    _case("inline_32x33", 129, 65, 32, 33, 8, 2, INLINE_SETS, expect={"cp_inline": 0, "e2_inline": 0}),
    _case("wide_k2_260", 150, 300, 8, 260, 8, 2, (W_SUM,), expect={"stats_route": 2}),
    _case("wide_k2_256", 150, 300, 8, 256, 8, 2, (W_SUM,), expect={"stats_route": 1, "e2_inline": 0}),
    _case("dcomm_split", 70, 65, 30, 200, 8, 2, (W_DCOMM, W_DCOMM_QUAD), n_ops=3, expect={"nsplit_d": 2}),
    _case("dcomm_tiny", 70, 65, 5, 7, 8, 2, (W_DCOMM, W_DCOMM_QUAD), n_ops=1, expect={"nsplit_d": 1, "cp_inline": 1}),
    _case("shape_12x20", 70, 65, 12, 20, 8, 3, SHAPE_SETS, expect={"cp_inline": 1}),
    _case("shape_40x25", 70, 65, 40, 25, 8, 3, SHAPE_SETS, expect={"cp_inline": 0}),
]
CASE_IDS = [c["id"] for c in CASES]
SAME_PLAN_SHAPE = dict(N1=300, N2=517, k1=20, k2=33, D=8)         # B = 1, 2, 3 all plan (rg, ncs) = (64, 4) on 256 CUs

# every (N1, N2, k1, k2, n_ops) of the table, for the plan grid of the CPU test
SIZES = sorted({(c["N1"], c["N2"], c["k1"], c["k2"], c["n_ops"]) for c in CASES})


def case_B(case, n_cu):
    """the batch a case runs with on a device of n_cu CUs (None: its target cannot be reached with B <= 1024)"""
    if case["B"] is not None:
        return case["B"]
    return pick_B(case["target"][0], case["target"][1], case["N1"], case["N2"], n_cu)


def sample_pairs(B, seed):
    """which pairs of a batch are held to the oracle: all up to 8, else 0, 1, B - 1 and five drawn by the seed"""
    if B <= 8:
        return list(range(B))
    drawn = np.random.default_rng(seed).choice(np.arange(2, B - 1), size=5, replace=False)
    return [0, 1] + sorted(int(x) for x in drawn) + [B - 1]

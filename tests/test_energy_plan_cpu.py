"""CPU: dm_fmap_energy_plan (the host function dm_fmap_energy_grad launches from) against the independent restatement in
tests/energy_cases.py, on a grid of CU counts, batch sizes, the sizes of the GPU case table and every weight set it uses; and
that the batches the GPU cases rely on exist on a 256-CU device.  Nothing here launches a kernel or needs a context."""
import ctypes as C

import pytest

import energy_cases as ec

N_CUS = (64, 128, 228, 256, 304)
BATCHES = (1, 2, 3, 64, 103, 205, 342, 512, 1024)


@pytest.fixture(scope="module")
def lib():
    from densematcher_amd import _build, _lib
    _build.build()
    return _lib.load()


def lib_plan(lib, n_cu, B, N1, N2, k1, k2, weights, n_ops=0):
    """(rc, dict) from the library with a NULL context"""
    out = (C.c_int32 * 12)(*([-7] * 12))
    w = (C.c_double * 10)(*ec.weight_array(weights))
    rc = lib.dm_fmap_energy_plan(None, n_cu, B, N1, N2, k1, k2, C.cast(w, C.c_void_p), n_ops, out)
    return rc, dict(zip(ec.PLAN_FIELDS, (int(v) for v in out)))


def test_plan_fields_match_the_engine():
    from densematcher_amd.engine import MatchEngine
    assert tuple(MatchEngine.ENERGY_PLAN_FIELDS) == ec.PLAN_FIELDS
    assert tuple(MatchEngine.WEIGHT_ORDER) == ec.WEIGHT_ORDER


def test_plan_equals_restatement_on_the_grid(lib):
    n = 0
    s = ec.SAME_PLAN_SHAPE
    assert (s["N1"], s["N2"], s["k1"], s["k2"], 0) in ec.SIZES
    for (N1, N2, k1, k2, n_ops) in ec.SIZES:
        for w in ec.ALL_WEIGHT_SETS:
            ops = max(n_ops, 1) if w.get("w_dcomm", 0) > 0 else n_ops
            for n_cu in N_CUS:
                for B in BATCHES:
                    try:
                        want = ec.plan(n_cu, B, N1, N2, k1, k2, w, ops)
                    except ValueError:
                        want = None
                    rc, got = lib_plan(lib, n_cu, B, N1, N2, k1, k2, w, ops)
                    if want is None:
                        assert rc == -1, (n_cu, B, N1, N2, k1, k2, w, ops, rc)
                    else:
                        assert rc == 0 and got == want, (n_cu, B, N1, N2, k1, k2, w, ops, rc, got, want)
                    n += 1
    assert n >= len(ec.SIZES) * len(ec.ALL_WEIGHT_SETS) * len(N_CUS) * len(BATCHES)


def test_n_cu_default_is_256(lib):
    s = ec.SWEEP_SHAPE
    for B in BATCHES:
        for n_cu in (0, -3):
            rc, got = lib_plan(lib, n_cu, B, s["N1"], s["N2"], s["k1"], s["k2"], ec.W_FULL)
            assert rc == 0 and got == ec.plan(256, B, s["N1"], s["N2"], s["k1"], s["k2"], ec.W_FULL)


def test_sweep_targets_first_batches_on_256_cus(lib):
    """the table of the row-group sweep: the first B of every (rg, ncs) at N1 = 200, N2 = 600 on 256 CUs, by the restatement and by
    the library"""
    s = ec.SWEEP_SHAPE
    for target, first in ec.SWEEP_FIRST_B_256CU.items():
        assert ec.pick_B(target[0], target[1], s["N1"], s["N2"], 256) == first
        for B, hit in ((first, True), (first - 1, False)):
            if B < 1:
                continue
            rc, got = lib_plan(lib, 256, B, s["N1"], s["N2"], s["k1"], s["k2"], ec.W_STO)
            assert rc == 0 and ((got["rg"], got["ncs"]) == target) == hit, (target, B, got)
    rc, got = lib_plan(lib, 256, 512, s["N1"], s["N2"], s["k1"], s["k2"], ec.W_STO)
    assert (got["ngroups"], got["cchunk"]) == (2, 256)          # two groups (512 + 88 rows), four column tiles in one split


def test_every_case_of_the_table_has_its_batch_on_256_cus(lib):
    for case in ec.CASES:
        B = ec.case_B(case, 256)
        assert B is not None and B <= (1024 if case["id"].startswith("exact_multiples") else 512), (case["id"], B)
        for w in case["sets"]:
            rc, got = lib_plan(lib, 256, B, case["N1"], case["N2"], case["k1"], case["k2"], w, case["n_ops"])
            assert rc == 0, (case["id"], w)
            if case["target"] and got["m_terms"]:
                assert (got["rg"], got["ncs"]) == case["target"], (case["id"], B, got)
            for name, v in case["expect"].items():
                if name in ("m_terms", "cp_inline", "nsplit_d") or got["m_terms"]:
                    assert got[name] == v, (case["id"], w, name, got)
    s = ec.SAME_PLAN_SHAPE
    for B in (1, 2, 3):
        rc, got = lib_plan(lib, 256, B, s["N1"], s["N2"], s["k1"], s["k2"], ec.W_FULL)
        assert rc == 0 and (got["rg"], got["ncs"], got["cchunk"]) == (64, 4, 128)
    assert ec.pick_B(64, 1, s["N1"], s["N2"], 256) is not None


def test_size_only_fields_do_not_depend_on_the_batch_or_the_device(lib):
    """what the source chooses "by the map's size only": equal for every B and CU count of the grid"""
    for (N1, N2, k1, k2, n_ops) in ec.SIZES:
        for w in ec.ALL_WEIGHT_SETS:
            ops = max(n_ops, 1) if w.get("w_dcomm", 0) > 0 else n_ops
            seen = set()
            for n_cu in N_CUS:
                for B in BATCHES:
                    rc, got = lib_plan(lib, n_cu, B, N1, N2, k1, k2, w, ops)
                    if rc == 0:
                        seen.add(tuple(got[f] for f in ec.SIZE_ONLY_FIELDS))
            assert len(seen) <= 1, (N1, N2, k1, k2, w, seen)


def test_refusals_stay_refusals(lib):
    """sizes and weights the launcher refuses are refused by the plan with the same code (DM_EINVAL), and the output is left alone"""
    for w in (ec.W_ENT, ec.W_SUM, ec.W_STO, ec.W_P2P_RANGE, ec.W_FULL):
        rc, got = lib_plan(lib, 256, 1, 70, 65, 257, 8, w)
        assert rc == -1 and set(got.values()) == {-7}, (w, rc, got)
        rc, got = lib_plan(lib, 256, 1, 70, 65, 256, 8, w)
        assert rc == 0 and got["nt2"] == 4
    rc, _ = lib_plan(lib, 256, 1, 70, 65, 257, 8, ec.W_QUAD)                 # no indicator term: any k1
    assert rc == 0
    assert lib_plan(lib, 256, 2, 70, 65, 5, 7, ec.W_DCOMM, 32768)[0] == -1   # B * n_ops > 65535
    assert lib_plan(lib, 256, 1, 70, 65, 5, 7, ec.W_DCOMM, 65535)[0] == 0
    assert lib_plan(lib, 256, 1, 70, 65, 5, 7, ec.W_DCOMM, 0)[0] == -1       # w_dcomm without operators
    assert lib_plan(lib, 256, 65536, 70, 65, 5, 7, ec.W_QUAD)[0] == -1
    assert lib_plan(lib, 256, 0, 70, 65, 5, 7, ec.W_QUAD)[0] == -1
    assert lib_plan(lib, 256, 1, 70, 65, 5, 7, {"w_ent": -1.0})[0] == -1
    assert lib.dm_fmap_energy_plan(None, 256, 1, 70, 65, 5, 7, None, 0, (C.c_int32 * 12)()) == -1
    w = (C.c_double * 10)(*ec.weight_array(ec.W_QUAD))
    assert lib.dm_fmap_energy_plan(None, 256, 1, 70, 65, 5, 7, C.cast(w, C.c_void_p), 0, None) == -1

"""GPU: every work decomposition dm_fmap_energy_grad chooses from its sizes (densematcher_amd/csrc/dm_energy.hip: energy_plan_make),
each at the smallest shape where it exists, value and gradient against the float64 oracle.

Reference: oracle.dm_oracle.energy_grad_general.  Bound: the one of test_energy_indicator_terms_ragged (tests/test_gpu_api.py),
|E - Eo| <= 1e-11 |Eo| and max |G - Go| <= 1e-11 max |Go|.  (The oracle's own deviation from an np.longdouble restatement on these
shapes: at most 4e-14 of max |G| (k1 = 256) and 3e-16 of |E|.)

Every case first asserts the route it claims -- through MatchEngine.energy_plan with the device's real CU count, against the
restatement in tests/energy_cases.py -- and then checks the plan against the kernels that were launched (profile_report).  A case
whose route cannot be reached fails; it does not skip.  In batches above 8 pairs the pairs 0, 1, B - 1 and five drawn by the seed
are compared (energy_cases.sample_pairs); all pairs otherwise.  Each case prints its plan and its worst ratio to the bound.
"""
import numpy as np
import pytest

import energy_cases as ec
from oracle import dm_oracle as orc

pytestmark = pytest.mark.gpu

BOUND = 1e-11


@pytest.fixture(scope="module")
def eng():
    from densematcher_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def n_cu(eng):
    import torch
    return int(torch.cuda.get_device_properties(eng.device).multi_processor_count)


def oracle_pair(ops, b, w):
    o1 = None if ops["ops1"] is None else ops["ops1"][b]
    o2 = None if ops["ops2"] is None else ops["ops2"][b]
    return orc.energy_grad_general(ops["C"][b], ops["A"][b].astype(np.float64), ops["Bm"][b].astype(np.float64),
                                   orc.ev_sqdiff(ops["lam1"][b], ops["lam2"][b]), ops["e1"][b], ops["e2"][b], ops["a1"][b], w, o1, o2,
                                   ops["lam1"][b], ops["lam2"][b])


def evaluate(eng, ops, w, B=None):
    """energy (B,), gradient (B, k2, k1) as NumPy arrays, and the launch report of this one evaluation"""
    cut = (lambda a: a) if B is None else (lambda a: None if a is None else a[:B])
    eng.profile_kernel("*")
    try:
        E, G = eng.energy_grad(cut(ops["C"]), cut(ops["A"]), cut(ops["Bm"]), cut(ops["lam1"]), cut(ops["lam2"]), w, cut(ops["e1"]), cut(ops["e2"]),
                               cut(ops["a1"]), cut(ops["ops1"]), cut(ops["ops2"]))
        rep = eng.profile_report(kernels=True)
    finally:
        eng.profile_kernel("")
    return E.cpu().numpy(), G.cpu().numpy(), rep


def check_launches(plan, rep, tag):
    """the plan against what was launched"""
    m = bool(plan["m_terms"])
    want = {"energy_stats_tiles": plan["stats_route"] == 2, "energy_finish_stats": plan["stats_route"] == 2,
            "energy_stats_linear": plan["stats_route"] == 1, "energy_sum_splits": m and plan["ncs"] > 1,
            "energy_cp_nt_f64": not plan["cp_inline"], "energy_quad": not plan["cp_inline"], "emb2_nt_f64": m and not plan["e2_inline"],
            "splitk_reduce": plan["nsplit_d"] > 1, "dcomm_rt_tn_f64": plan["nsplit_d"] > 0, "energy_deriv_tiles": m, "energy_back_tn_f64": m,
            "energy_combine": True}
    for name, present in want.items():
        assert (name in rep) == present, (tag, name, present, sorted(rep))
        if present:
            assert rep[name][0] == 1, (tag, name, rep[name])
    if m:
        assert rep["energy_deriv_tiles"][2] == ("em_deriv_kernel<%d>" % plan["nt2"],), (tag, rep["energy_deriv_tiles"])


def worst_ratio(E, G, ops, w, pairs, tag):
    """max over the pairs of |E - Eo| / (BOUND |Eo|) and max |G - Go| / (BOUND max |Go|); column 0 of the gradient is zero"""
    worst = 0.0
    for b in pairs:
        Eo, Go = oracle_pair(ops, b, w)
        assert np.isfinite(E[b]) and np.isfinite(G[b]).all(), (tag, b)
        assert np.all(G[b][:, 0] == 0), (tag, b)
        assert abs(Eo) > 0 and np.abs(Go).max() > 0, (tag, b)
        rE = abs(float(E[b]) - Eo) / (BOUND * abs(Eo))
        rG = np.abs(G[b] - Go).max() / (BOUND * np.abs(Go).max())
        assert rE <= 1.0, (tag, b, "energy", float(E[b]), Eo, rE)
        assert rG <= 1.0, (tag, b, "gradient", rG)
        worst = max(worst, rE, rG)
    return worst


@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_energy_route(eng, n_cu, case):
    B = ec.case_B(case, n_cu)
    if B is None:
        pytest.fail("%s: no batch <= 1024 reaches (rg, ncs) = %s on %d CUs" % (case["id"], case["target"], n_cu))
    N1, N2, k1, k2 = case["N1"], case["N2"], case["k1"], case["k2"]
    seed = 1000 + ec.CASE_IDS.index(case["id"])
    ops = ec.make_case(seed, B, N1, N2, k1, k2, case["D"], case["n_ops"])
    pairs = ec.sample_pairs(B, seed)
    for w in case["sets"]:
        tag = (case["id"], B, tuple(sorted(w)))
        plan = eng.energy_plan(B, N1, N2, k1, k2, w, case["n_ops"])
        assert plan == ec.plan(n_cu, B, N1, N2, k1, k2, w, case["n_ops"]), (tag, plan)
        if case["target"] and plan["m_terms"]:
            assert (plan["rg"], plan["ncs"]) == case["target"], (tag, plan)
        for name, v in case["expect"].items():
            if name in ("m_terms", "cp_inline", "nsplit_d") or plan["m_terms"]:
                assert plan[name] == v, (tag, name, plan)
        E, G, rep = evaluate(eng, ops, w)
        check_launches(plan, rep, tag)
        worst = worst_ratio(E, G, ops, w, pairs, tag)
        print("%s B=%d %s plan=%s pairs=%s worst ratio to the 1e-11 bound: %.3g" % (case["id"], B, "+".join(sorted(w)), plan, pairs, worst))


def test_sweep_reaches_every_row_group_on_this_device(eng, n_cu):
    """the five (rg, ncs) of the sweep are five different plans here, with the batches the table promises on 256 CUs"""
    s = ec.SWEEP_SHAPE
    got = {}
    for t in ec.SWEEP_TARGETS:
        B = ec.pick_B(t[0], t[1], s["N1"], s["N2"], n_cu)
        assert B is not None, (t, n_cu)
        p = eng.energy_plan(B, s["N1"], s["N2"], s["k1"], s["k2"], ec.W_STO)
        assert (p["rg"], p["ncs"]) == t, (t, B, p)
        got[t] = B
    print("row-group sweep on %d CUs: first B per (rg, ncs) = %s" % (n_cu, got))
    if n_cu == 256:
        assert got == ec.SWEEP_FIRST_B_256CU


def test_refusals(eng):
    """k1 = 257 with an indicator term, and more than 65535 (pair, operator) slots: refused by the plan and by the evaluation alike"""
    ops = ec.make_case(7, 1, 70, 65, 257, 8, 8)
    with pytest.raises(ValueError):
        eng.energy_plan(1, 70, 65, 257, 8, ec.W_ENT)
    with pytest.raises(ValueError):
        eng.energy_grad(ops["C"], ops["A"], ops["Bm"], ops["lam1"], ops["lam2"], ec.W_ENT, ops["e1"], ops["e2"], ops["a1"])
    E, G, _ = evaluate(eng, ops, ec.W_QUAD)                        # the quadratic terms take any k1
    assert worst_ratio(E, G, ops, ec.W_QUAD, [0], "k1=257 quadratic") <= 1.0
    ops = ec.make_case(8, 1, 4, 4, 2, 2, 2, n_ops=65536)
    with pytest.raises(ValueError):
        eng.energy_plan(1, 4, 4, 2, 2, ec.W_DCOMM, 65536)
    with pytest.raises(ValueError):
        eng.energy_grad(ops["C"], ops["A"], ops["Bm"], ops["lam1"], ops["lam2"], ec.W_DCOMM, ops["e1"], ops["e2"], ops["a1"], ops["ops1"], ops["ops2"])


def test_same_plan_same_bits(eng, n_cu):
    """A pair's energy and gradient are bit-identical whenever the plan is the same: B = 1, 2, 3 (all (rg, ncs) = (64, 4) at these
    sizes on 256 CUs) and repeated calls.  Inside a batch whose plan differs (the first B with ncs = 1) the pair still meets the oracle
    bound; whether its bits equal the B = 1 result is printed (DESIGN.md records it: the summation orders of the column sums, the row
    sums, Y and the energy shares follow rg and ncs)."""
    s = ec.SAME_PLAN_SHAPE
    N1, N2, k1, k2 = s["N1"], s["N2"], s["k1"], s["k2"]
    w = ec.W_FULL
    Bbig = next((B for B in range(1, 1025) if ec.plan(n_cu, B, N1, N2, k1, k2, w)["ncs"] == 1), None)
    assert Bbig is not None
    ops = ec.make_case(4242, Bbig, N1, N2, k1, k2, s["D"])
    plans = [eng.energy_plan(B, N1, N2, k1, k2, w) for B in (1, 2, 3)]
    if n_cu == 256:
        assert all((p["rg"], p["ncs"], p["cchunk"]) == (64, 4, 128) for p in plans), plans
    assert plans[0] == plans[1] == plans[2], plans                 # (nothing but B differs, and no field depends on it here)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    ref = None
    for B in (1, 2, 3, 1, 3):
        E, G, _ = evaluate(eng, ops, w, B)
        if ref is None:
            ref = (bits(E[:1]).copy(), bits(G[0]).copy())
            assert worst_ratio(E, G, ops, w, [0], "same plan B=1") <= 1.0
        assert np.array_equal(bits(E[:1]), ref[0]) and np.array_equal(bits(G[0]), ref[1]), B
    pbig = eng.energy_plan(Bbig, N1, N2, k1, k2, w)
    assert pbig["ncs"] == 1 and (pbig["rg"], pbig["ncs"]) != (plans[0]["rg"], plans[0]["ncs"])
    E, G, _ = evaluate(eng, ops, w, Bbig)
    worst = worst_ratio(E, G, ops, w, ec.sample_pairs(Bbig, 4242), "other plan")
    same = bool(np.array_equal(bits(E[:1]), ref[0]) and np.array_equal(bits(G[0]), ref[1]))
    print("same plan, same bits: B = 1, 2, 3 under %s; pair 0 inside B = %d under (rg, ncs) = (%d, %d): worst ratio %.3g, bits equal to "
          "the B = 1 result: %s (largest difference %.3g of max |G|)"
          % (plans[0], Bbig, pbig["rg"], pbig["ncs"], worst, same, np.abs(G[0] - ref[1].view(np.float64)).max() / np.abs(G[0]).max()))

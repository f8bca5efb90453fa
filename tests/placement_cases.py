"""
The cases of the placement tests (tests/test_gpu_placement.py, tests/test_placement_cpu.py): per entry point of the library
    configs()           the parametrisation (dicts of plain values; their str() is the pytest id)
    build(cfg)          the LOGICAL operands, name -> numpy array, in the order of the call
    ld_of               the operands that take a row stride ld > width (the eigenvector arrays)
    rows_of             the operands whose rows behind the logical count are padding as well (the square padded maps of dm_fmn_*,
                        the distance matrices of padded batches)
    rows_only           the operands of a padded batch whose rows behind n_verts are padding (vertex and eigenvector arrays)
    oracle(ops, cfg)    the float64 oracle (oracle/dm_oracle.py) of the operation on the logical operands, name -> numpy array
    call(eng, T, cfg)   the engine call on torch operands T (same names; eigenvector arrays possibly wider than k) -> name -> tensor
    lib(cfg)            the C entry the call ends in (its pointer arguments are recorded)
    check(got, ref, cfg) -> None or a message: the tolerance of the entry's EXISTING test, cited where it is applied
    loose(cfg, moved)   True where the placed call may differ from the aligned control in the last bits (module docstring of
                        tests/test_gpu_placement.py lists every such case with its reason)

Sizes: the smallest that still reach every branch -- N1 = 333, N2 = 517 (odd, more than one tile, N * ld = 1 .. 3 mod 4 floats per
pair), (k1, k2) in {(15, 17), (16, 16)}, three pairs.
"""
import zlib

import numpy as np

from oracle import dm_oracle as orc

B, N1, N2 = 3, 333, 517
KPAIRS = ((15, 17), (16, 16))
DTS = ("f32", "f64")
NPDT = {"f32": np.float32, "f64": np.float64}
LD_EXTRA = (1, 5)          # row strides k + 1 (odd / even flips with k) and k + 5


def _rng(*key):
    """a generator seeded by the case's own key: the CPU and the GPU test build the same operands"""
    return np.random.default_rng(zlib.crc32("/".join(str(x) for x in key).encode()))


def _basis(rng, N, k, dt):
    return (rng.standard_normal((B, N, k)) * 0.05).astype(NPDT[dt])


def _smooth_basis(rng, N, k, dt):
    """low-frequency-looking columns (tests/test_gpu_parity.py: _smooth_basis), another phase per pair"""
    x = np.linspace(0.0, 1.0, N)[None, :, None]
    f = np.arange(1, k + 1)[None, None, :]
    return (np.cos(np.pi * f * x + rng.uniform(0, 6.28, (B, 1, k))) * np.sqrt(2.0 / N)).astype(NPDT[dt])


def _mass(rng, N, dt):
    return (rng.uniform(0.5, 1.5, (B, N)) / N).astype(NPDT[dt])


def _lam(rng, k):
    lam = np.sort(rng.uniform(0.5, 60.0, (B, k)), axis=1)
    lam[:, 0] = 0.0
    return lam


def _per_pair(fn):
    return np.stack([np.asarray(fn(b)) for b in range(B)])


def _maxerr(got, ref, scale=1.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - ref).max() / scale)


class Entry:
    ld_of = ()          # operands that take a row stride above their width
    rows_of = ()        # operands that also take a row count above their own (square padded maps: rows = ld)
    rows_only = ()      # operands of a padded batch: rows behind n_verts are padding, whatever the row stride
    batched = True      # the leading axis of every operand of two or more dimensions is the batch (a slice of it is an operand)

    def configs(self):
        raise NotImplementedError

    def loose(self, cfg, moved):
        return False


# ------------------------------------------------------------------------------------------------ projection
def _odd_f16(moved, names):
    """an fp16 operand of `names` that starts at an odd element: not on a dword boundary"""
    return any(kw.get("offset_elems", 0) % 2 == 1 for n, kw in moved.items() if n in names)


class Project(Entry):
    name, ld_of = "project", ("Phi",)

    def configs(self):
        return [dict(dt=dt, k=k, fdt=fdt, D=D, exact=ex, onepass=op) for dt in DTS for k in (15, 16)
                for fdt, D, ex, op in (("f16", 24, 0, 1), ("f16", 40, 0, 1), ("f16", 24, 0, 0), ("f16", 40, 0, 0), ("f16", 24, 1, 1), ("f16", 24, 1, 0),
                                    ("f32", 22, 0, 1), ("f32", 22, 0, 0))]

    def build(self, c):
        rng = _rng("project", c["dt"], c["k"], c["D"])
        F = rng.standard_normal((B, N1, c["D"])).astype(np.float16 if c["fdt"] == "f16" else np.float32)
        return dict(Phi=_basis(rng, N1, c["k"], c["dt"]), mass=_mass(rng, N1, c["dt"]), F=F)

    def oracle(self, o, c):
        # (tests/test_gpu_project.py: _ref) the float64 product of the fp32-rounded operands and the sum of its absolute terms
        X = o["Phi"].astype(np.float32).astype(np.float64) * o["mass"].astype(np.float32).astype(np.float64)[:, :, None]
        Fd = o["F"].astype(np.float64)
        return dict(R=np.einsum("bnk,bnd->bkd", X, Fd), S=np.einsum("bnk,bnd->bkd", np.abs(X), np.abs(Fd)),
                    A64=_per_pair(lambda b: orc.project(o["Phi"][b], o["mass"][b], o["F"][b])))

    def lib(self, c):
        return "dm_project" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        eng.set_option("proj_onepass", c["onepass"])
        return dict(A=eng.project(T["Phi"], T["mass"], T["F"], c["k"], exact=bool(c["exact"])))

    def check(self, got, ref, c):
        A = got["A"].astype(np.float64)
        if not np.isfinite(A).all():
            return "non-finite projection"
        if c["fdt"] == "f16" and not c["exact"]:
            e = float((np.abs(A - ref["R"]) / np.maximum(ref["S"], 1e-300)).max())
            return None if e <= 2e-6 else f"|A - R| / S = {e:.3e} > 2e-6"           # tests/test_gpu_project.py:62
        e, lim = np.abs(A - ref["A64"]).max(), 2e-7 * np.abs(ref["A64"]).max() + 1e-12      # tests/test_gpu_parity.py:48
        return None if e <= lim else f"|A - A64| = {e:.3e} > {lim:.3e}"

    def loose(self, c, moved):
        return c["fdt"] == "f16" and not c["exact"] and c["onepass"] == 1 and _odd_f16(moved, ("F",))


class C00(Entry):
    name, ld_of = "c00", ("Phi1", "Phi2")

    def configs(self):
        return [dict(dt=dt, k=15) for dt in DTS]

    def build(self, c):
        rng = _rng("c00", c["dt"])
        return dict(Phi1=_basis(rng, N1, c["k"], c["dt"]), Phi2=_basis(rng, N2, c["k"], c["dt"]), a1=_mass(rng, N1, c["dt"]),
                    a2=_mass(rng, N2, c["dt"]))

    def oracle(self, o, c):
        return dict(c00=_per_pair(lambda b: orc.get_x0(1, 1, float(o["Phi1"][b, 0, 0]), float(o["Phi2"][b, 0, 0]),
                                                       float(o["a1"][b].astype(np.float64).sum()), float(o["a2"][b].astype(np.float64).sum()))[0, 0]))

    def lib(self, c):
        return "dm_fmap_c00" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        return dict(c00=eng.c00(T["Phi1"], T["Phi2"], T["a1"], T["a2"]))

    def check(self, got, ref, c):
        e = _maxerr(got["c00"] / ref["c00"], 1.0)
        return None if e <= 1e-14 else f"relative error {e:.3e} > 1e-14"           # tests/test_gpu_parity.py:61


W_DESCR, W_LAP = 1e4, 1e3      # the fit's weights everywhere in the suite (tests/test_gpu_parity.py, __graft_entry__.smoke)


class FmapFit(Entry):
    name, ld_of = "fmap_fit", ("Phi1", "Phi2")

    def configs(self):
        return [dict(dt=dt, k1=k1, k2=k2, D=D, onepass=op) for dt in DTS for k1, k2 in KPAIRS for D in (24, 40) for op in (1, 0)]

    def build(self, c):
        rng = _rng("fit", c["dt"], c["k1"], c["k2"], c["D"])
        return dict(Phi1=_basis(rng, N1, c["k1"], c["dt"]), Phi2=_basis(rng, N2, c["k2"], c["dt"]), a1=_mass(rng, N1, c["dt"]),
                    a2=_mass(rng, N2, c["dt"]), F1=rng.standard_normal((B, N1, c["D"])).astype(np.float16),
                    F2=rng.standard_normal((B, N2, c["D"])).astype(np.float16), lam1=_lam(rng, c["k1"]), lam2=_lam(rng, c["k2"]))

    def oracle(self, o, c):
        return dict(C=_per_pair(lambda b: orc.fit(o["Phi1"][b], o["Phi2"][b], o["lam1"][b], o["lam2"][b], o["a1"][b], o["a2"][b],
                                                  o["F1"][b], o["F2"][b], W_DESCR, W_LAP)))

    def lib(self, c):
        return "dm_fmap_fit" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        eng.set_option("proj_onepass", c["onepass"])
        return dict(C=eng.fmap_fit(T["Phi1"], T["Phi2"], T["a1"], T["a2"], T["F1"], T["F2"], T["lam1"], T["lam2"], W_DESCR, W_LAP,
                                   c["k1"], c["k2"]))

    def check(self, got, ref, c):
        e = _maxerr(got["C"], ref["C"])
        return None if e <= 1e-4 else f"|C - C_oracle| = {e:.3e} > 1e-4"           # tests/test_gpu_parity.py:13,66 (C_TOL)

    def loose(self, c, moved):
        return c["onepass"] == 1 and _odd_f16(moved, ("F1", "F2"))


class FmapSolve(Entry):
    name = "fmap_solve"

    def configs(self):
        return [dict(k1=k1, k2=k2, D=D) for k1, k2 in KPAIRS for D in (24, 22)]

    def build(self, c):
        rng = _rng("solve", c["k1"], c["k2"], c["D"])
        A = np.stack([orc.project(_basis(rng, N1, c["k1"], "f32")[0], _mass(rng, N1, "f32")[0], rng.standard_normal((N1, c["D"]))) for _ in range(B)])
        Bm = np.stack([orc.project(_basis(rng, N2, c["k2"], "f32")[0], _mass(rng, N2, "f32")[0], rng.standard_normal((N2, c["D"]))) for _ in range(B)])
        return dict(A=A.astype(np.float32), Bm=Bm.astype(np.float32), lam1=_lam(rng, c["k1"]), lam2=_lam(rng, c["k2"]),
                    c00=rng.uniform(0.8, 1.2, B) * np.array([1.0, -1.0, 1.0]))

    def oracle(self, o, c):
        def one(b):
            x0 = np.zeros((c["k2"], c["k1"]))
            x0[0, 0] = o["c00"][b]
            return orc.fmap_solve(o["A"][b], o["Bm"][b], o["lam1"][b], o["lam2"][b], x0, W_DESCR, W_LAP)
        return dict(C=_per_pair(one))

    def lib(self, c):
        return "dm_fmap_solve"

    def call(self, eng, T, c):
        Cm, info = eng.fmap_solve(T["A"], T["Bm"], T["lam1"], T["lam2"], T["c00"], W_DESCR, W_LAP, return_info=True)
        return dict(C=Cm, info=info)

    def check(self, got, ref, c):
        if got["info"].any():
            return f"info = {got['info']}"
        e = _maxerr(got["C"], ref["C"])
        return None if e <= 1e-9 else f"|C - C_oracle| = {e:.3e} > 1e-9"           # tests/test_gpu_parity.py:73


class DescrOps(Entry):
    name, ld_of = "descr_ops", ("Phi",)

    def configs(self):
        return [dict(k=k, fdt=fdt, D=D) for k in (15, 16) for fdt, D in (("f16", 24), ("f32", 22))]

    def build(self, c):
        rng = _rng("descr_ops", c["k"], c["D"])
        return dict(Phi=_basis(rng, N1, c["k"], "f32"), mass=_mass(rng, N1, "f32"),
                    F=rng.standard_normal((B, N1, c["D"])).astype(np.float16 if c["fdt"] == "f16" else np.float32))

    def oracle(self, o, c):
        return dict(ops=_per_pair(lambda b: orc.descr_ops(o["Phi"][b], o["mass"][b], o["F"][b])))

    def lib(self, c):
        return "dm_fmap_descr_ops"

    def call(self, eng, T, c):
        return dict(ops=eng.descr_ops(T["Phi"], T["mass"], T["F"], c["k"]))

    def check(self, got, ref, c):
        e = _maxerr(got["ops"], ref["ops"], np.abs(ref["ops"]).max())
        return None if e <= 1e-13 else f"relative error {e:.3e} > 1e-13"           # tests/test_gpu_api.py:262


# ------------------------------------------------------------------------------------------------ energy terms
# (tests/test_gpu_api.py: MIX -- every term of dm_fmap_energy_grad at once)
MIX = dict(w_descr=1e4, w_lap=1e3, w_dcomm=0.5, w_p2p=0.05, w_stochastic=0.02, w_ent=0.1, w_range01=1.0, w_sumto1=2.0)
# (tests/test_gpu_fitfuse.py:40 -- every term dm_fmap_fit_fused takes)
FUSED_W = {"w_p2p": 0.5, "w_ent": 0.3, "w_range01": 1.5, "w_sumto1": 2.0, "w_descr": 1.0, "w_lap": 0.1}
N_OPS = 3


def _energy_ops(tag, c, with_ops):
    """(tests/test_gpu_fitfuse.py: _random_problem) the second pair's map scaled up: indicator entries on both sides of the clamp"""
    rng = _rng(tag, c["k1"], c["k2"], c["D"])
    k1, k2 = c["k1"], c["k2"]
    Cm = rng.standard_normal((B, k2, k1)) * 3.0
    Cm[1] *= 40.0
    o = dict(C=Cm, A=rng.standard_normal((B, k1, c["D"])).astype(np.float32), Bm=rng.standard_normal((B, k2, c["D"])).astype(np.float32),
             lam1=np.sort(rng.uniform(0, 50, (B, k1)), axis=1), lam2=np.sort(rng.uniform(0, 50, (B, k2)), axis=1),
             Phi1=(rng.standard_normal((B, N1, k1)) / np.sqrt(N1)).astype(np.float32),
             Phi2=(rng.standard_normal((B, N2, k2)) / np.sqrt(N2)).astype(np.float32), a1=_mass(rng, N1, "f32"))
    if with_ops:
        o["ops1"] = rng.standard_normal((B, N_OPS, k1, k1)) * 0.1
        o["ops2"] = rng.standard_normal((B, N_OPS, k2, k2)) * 0.1
    return o


def _energy_oracle(o, w):
    per = [orc.energy_grad_general(o["C"][b], o["A"][b].astype(np.float64), o["Bm"][b].astype(np.float64), orc.ev_sqdiff(o["lam1"][b], o["lam2"][b]),
                                   o["Phi1"][b], o["Phi2"][b], o["a1"][b], w, *((o["ops1"][b], o["ops2"][b]) if "ops1" in o else ()))
           for b in range(B)]
    return dict(E=np.array([p[0] for p in per]), G=np.stack([p[1] for p in per]))


def _energy_check(got, ref, tol, cite):
    for b in range(B):
        if not (np.isfinite(got["E"][b]) and np.isfinite(got["G"][b]).all()):
            return f"pair {b}: non-finite energy / gradient"
        e = abs(got["E"][b] - ref["E"][b]) / abs(ref["E"][b])
        g = np.abs(got["G"][b] - ref["G"][b]).max() / max(np.abs(ref["G"][b]).max(), 1e-300)
        if e > tol or g > tol:
            return f"pair {b}: energy {e:.3e}, gradient {g:.3e} > {tol:g} ({cite})"
    return None


class EnergyGrad(Entry):
    name, ld_of = "energy_grad", ("Phi1", "Phi2")

    def configs(self):
        return [dict(k1=k1, k2=k2, D=D) for k1, k2 in KPAIRS for D in (24, 22)]

    def build(self, c):
        return _energy_ops("energy_grad", c, True)

    def oracle(self, o, c):
        return _energy_oracle(o, MIX)

    def lib(self, c):
        return "dm_fmap_energy_grad"

    def call(self, eng, T, c):
        E, G = eng.energy_grad(T["C"], T["A"], T["Bm"], T["lam1"], T["lam2"], MIX, T["Phi1"], T["Phi2"], T["a1"], T["ops1"], T["ops2"])
        return dict(E=E, G=G)

    def check(self, got, ref, c):
        return _energy_check(got, ref, 1e-11, "tests/test_gpu_api.py:269-270")


class EnergyGradFused(Entry):
    name, ld_of = "energy_grad_fused", ("Phi1", "Phi2")

    def configs(self):
        return [dict(k1=k1, k2=k2, D=D) for k1, k2 in KPAIRS for D in (24, 22)]

    def build(self, c):
        return _energy_ops("energy_grad_fused", c, False)

    def oracle(self, o, c):
        return _energy_oracle(o, FUSED_W)

    def lib(self, c):
        return "dm_fmap_fit_fused"

    def call(self, eng, T, c):
        E, G = eng.energy_grad_fused(T["C"], T["A"], T["Bm"], T["lam1"], T["lam2"], FUSED_W, T["Phi1"], T["Phi2"], T["a1"])
        return dict(E=E, G=G)

    def check(self, got, ref, c):
        return _energy_check(got, ref, 1e-10, "tests/test_gpu_fitfuse.py:46-47")


# ------------------------------------------------------------------------------------------------ vertex maps
def _map_ops(tag, c):
    rng = _rng(tag, c["dt"], c["k1"], c["k2"])
    return dict(Phi1=_basis(rng, N1, c["k1"], c["dt"]), Phi2=_basis(rng, N2, c["k2"], c["dt"]), a1=_mass(rng, N1, c["dt"]),
                C=rng.standard_normal((B, c["k2"], c["k1"])))


class FmToP2p(Entry):
    name, ld_of = "fm_to_p2p", ("Phi1", "Phi2")
    MAPS = ("knn21", "knn12", "ind21", "ind12")

    def configs(self):
        return [dict(dt=dt, k1=k1, k2=k2, p2p_split=ps, knn_split=ks) for dt in DTS for k1, k2 in KPAIRS for ps in (2, 0) for ks in (1, 0)]

    def build(self, c):
        return _map_ops("fm_to_p2p", c)

    def oracle(self, o, c):
        per = [orc.fm_to_p2p_all(o["C"][b], o["Phi1"][b], o["Phi2"][b], o["a1"][b]) for b in range(B)]
        return {n: np.stack([np.asarray(p[i]) for p in per]) for i, n in enumerate(self.MAPS)}

    def lib(self, c):
        return "dm_fm_to_p2p" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        eng.set_option("p2p_split", c["p2p_split"])
        eng.set_option("knn_split", c["knn_split"])
        return eng.fm_to_p2p(T["Phi1"], T["Phi2"], T["a1"], T["C"])

    def check(self, got, ref, c):
        bad = [f"{n}: {(got[n] != ref[n]).sum()} mismatches" for n in self.MAPS if not np.array_equal(got[n], ref[n])]
        return "; ".join(bad) or None                                             # tests/test_gpu_parity.py:106 (bit-exact maps)


class MappedIndicator(Entry):
    name, ld_of = "mapped_indicator", ("Phi1", "Phi2")

    def configs(self):
        return [dict(dt=dt, k1=k1, k2=k2) for dt in DTS for k1, k2 in KPAIRS]

    def build(self, c):
        return _map_ops("mapped_indicator", c)

    def oracle(self, o, c):
        return dict(M=_per_pair(lambda b: orc.mapped_indicator(o["C"][b], o["Phi1"][b], o["Phi2"][b], o["a1"][b])))

    def lib(self, c):
        return "dm_mapped_indicator" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        return dict(M=eng.mapped_indicator(T["Phi1"], T["Phi2"], T["a1"], T["C"]))

    def check(self, got, ref, c):
        e = _maxerr(got["M"], ref["M"], max(1.0, np.abs(ref["M"]).max()))
        return None if e <= 1e-12 else f"error {e:.3e} > 1e-12"                    # tests/test_gpu_f64_basis.py:89


class P2pToFm(Entry):
    name, ld_of = "p2p_to_fm", ("Phi1", "Phi2")

    def configs(self):
        return [dict(dt=dt, k1=k1, k2=k2, direct=d) for dt in DTS for k1, k2 in KPAIRS for d in (1, 0)]

    def build(self, c):
        rng = _rng("p2p_to_fm", c["dt"], c["k1"], c["k2"])
        return dict(p21=rng.integers(0, N1, (B, N2)).astype(np.int32), Phi1=_basis(rng, N1, c["k1"], c["dt"]),
                    Phi2=_basis(rng, N2, c["k2"], c["dt"]), a2=_mass(rng, N2, c["dt"]))

    def oracle(self, o, c):
        return dict(C=_per_pair(lambda b: orc.p2p_to_fm(o["p21"][b], o["Phi1"][b], o["Phi2"][b], o["a2"][b])))

    def lib(self, c):
        return "dm_p2p_to_fm" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        eng.set_option("p2pfm_direct", c["direct"])
        return dict(C=eng.p2p_to_fm(T["p21"], T["Phi1"], T["Phi2"], T["a2"], c["k1"], c["k2"]))

    def check(self, got, ref, c):
        e = _maxerr(got["C"], ref["C"], max(1.0, np.abs(ref["C"]).max()))
        return None if e <= 1e-13 else f"error {e:.3e} > 1e-13"                    # tests/test_gpu_parity.py:209


class P2pToFmLstsq(Entry):
    name, ld_of = "p2p_to_fm_lstsq", ("Phi1", "Phi2")

    def configs(self):
        return [dict(dt=dt, k1=k1, k2=k2) for dt in DTS for k1, k2 in KPAIRS]

    def build(self, c):
        rng = _rng("p2p_to_fm_lstsq", c["dt"], c["k1"], c["k2"])
        return dict(p21=rng.integers(0, N1, (B, N2)).astype(np.int32), Phi1=_smooth_basis(rng, N1, c["k1"], c["dt"]),
                    Phi2=_smooth_basis(rng, N2, c["k2"], c["dt"]))

    def oracle(self, o, c):
        return dict(C=_per_pair(lambda b: orc.p2p_to_fm(o["p21"][b], o["Phi1"][b], o["Phi2"][b], None)))

    def lib(self, c):
        return "dm_p2p_to_fm_lstsq" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        return dict(C=eng.p2p_to_fm_lstsq(T["p21"], T["Phi1"], T["Phi2"], c["k1"], c["k2"]))

    def check(self, got, ref, c):
        e = _maxerr(got["C"], ref["C"])
        return None if e <= 1e-9 else f"|C - C_oracle| = {e:.3e} > 1e-9"           # tests/test_gpu_f64_basis.py:69


# ------------------------------------------------------------------------------------------------ refinement
K0, NIT = 5, 3


class ZoomOut(Entry):
    name, ld_of = "zoomout", ("Phi1", "Phi2")

    def configs(self):
        return [dict(dt=dt, step=s, fused=f) for dt in DTS for s in (1, 2) for f in (1, 0)]

    def build(self, c):
        rng = _rng("zoomout", c["dt"], c["step"])
        kf = K0 + NIT * c["step"]
        return dict(Phi1=_smooth_basis(rng, N1, kf, c["dt"]), Phi2=_smooth_basis(rng, N2, kf, c["dt"]), a2=_mass(rng, N2, c["dt"]),
                    C0=np.eye(K0)[None] + 0.05 * rng.standard_normal((B, K0, K0)))

    def oracle(self, o, c):
        per = [orc.zoomout_refine(o["C0"][b], o["Phi1"][b], o["Phi2"][b], nit=NIT, step=c["step"], a2=o["a2"][b], return_p2p=True)
               for b in range(B)]
        return dict(C=np.stack([p[0] for p in per]), p21=np.stack([p[1] for p in per]))

    def lib(self, c):
        return "dm_zoomout" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        eng.set_option("zoomout_fused", c["fused"])
        Cm, p = eng.zoomout(T["Phi1"], T["Phi2"], T["a2"], T["C0"], nit=NIT, step=c["step"], return_p2p=True)
        return dict(C=Cm, p21=p)

    def check(self, got, ref, c):
        if not np.array_equal(got["p21"], ref["p21"]):
            return f"p21: {(got['p21'] != ref['p21']).sum()} mismatches"          # tests/test_gpu_parity.py:203
        e = _maxerr(got["C"], ref["C"])
        return None if e <= 1e-11 else f"|C - C_oracle| = {e:.3e} > 1e-11"         # tests/test_gpu_parity.py:204


class ZoomOutSub(Entry):
    """the subsampled form: the iterations on Phi1[sub1], Phi2[sub2] with the least-squares map, the returned vertex map on all vertices"""
    name, ld_of = "zoomout_sub", ("Phi1", "Phi2")
    NS = 96

    def configs(self):
        return [dict(dt=dt, step=s, fused=f) for dt in DTS for s in (1, 2) for f in (1, 0)]

    def build(self, c):
        rng = _rng("zoomout_sub", c["dt"], c["step"])
        kf = K0 + NIT * c["step"]
        return dict(Phi1=_smooth_basis(rng, N1, kf, c["dt"]), Phi2=_smooth_basis(rng, N2, kf, c["dt"]),
                    C0=np.eye(K0)[None] + 0.05 * rng.standard_normal((B, K0, K0)),
                    sub1=np.stack([np.sort(rng.choice(N1, self.NS, replace=False)) for _ in range(B)]).astype(np.int32),
                    sub2=np.stack([np.sort(rng.choice(N2, self.NS + 32, replace=False)) for _ in range(B)]).astype(np.int32))

    def oracle(self, o, c):
        per = [orc.zoomout_refine(o["C0"][b], o["Phi1"][b], o["Phi2"][b], nit=NIT, step=c["step"], subsample=(o["sub1"][b], o["sub2"][b]),
                                  return_p2p=True) for b in range(B)]
        return dict(C=np.stack([p[0] for p in per]), p21=np.stack([p[1] for p in per]))

    def lib(self, c):
        return "dm_zoomout_sub" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        eng.set_option("zoomout_sub_fused", c["fused"])
        Cm, p = eng.zoomout(T["Phi1"], T["Phi2"], None, T["C0"], nit=NIT, step=c["step"], return_p2p=True, subsample=(T["sub1"], T["sub2"]))
        return dict(C=Cm, p21=p)

    def check(self, got, ref, c):
        if not np.array_equal(got["p21"], ref["p21"]):
            return f"p21: {(got['p21'] != ref['p21']).sum()} mismatches"          # tests/test_gpu_zoomout_sub.py:65
        e = _maxerr(got["C"], ref["C"])
        return None if e <= 1e-9 else f"|C - C_oracle| = {e:.3e} > 1e-9"           # tests/test_gpu_zoomout_sub.py:66


class Icp(Entry):
    name, ld_of = "icp", ("Phi1", "Phi2")

    def configs(self):
        return [dict(dt=dt, k1=k1, k2=k2) for dt in DTS for k1, k2 in KPAIRS]

    def build(self, c):
        rng = _rng("icp", c["dt"], c["k1"], c["k2"])
        return dict(Phi1=_smooth_basis(rng, N1, c["k1"], c["dt"]), Phi2=_smooth_basis(rng, N2, c["k2"], c["dt"]),
                    C0=np.eye(c["k2"], c["k1"])[None] + 0.05 * rng.standard_normal((B, c["k2"], c["k1"])))

    def oracle(self, o, c):
        return dict(C=_per_pair(lambda b: orc.icp_refine(o["C0"][b], o["Phi1"][b], o["Phi2"][b], nit=3)))

    def lib(self, c):
        return "dm_icp" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        # (engine.icp takes k from C0 and the row strides from the arrays)
        return dict(C=eng.icp(T["Phi1"], T["Phi2"], T["C0"], nit=3))

    def check(self, got, ref, c):
        e = _maxerr(got["C"], ref["C"])
        return None if e <= 1e-9 else f"|C - C_oracle| = {e:.3e} > 1e-9"           # tests/test_gpu_parity.py:213


# ------------------------------------------------------------------------------------------------ assignment
class Lsa(Entry):
    name = "linear_sum_assignment"

    def configs(self):
        return [dict(nr=nr, nc=nc, lsa_reg=m, maximize=mx) for nr, nc in ((33, 45), (45, 33), (65, 65)) for m in (2, 1, 0) for mx in (0, 1)]

    def build(self, c):
        rng = _rng("lsa", c["nr"], c["nc"])
        cost = rng.standard_normal((B, c["nr"], c["nc"]))
        cost[1] = np.round(3 * cost[1])                        # (tests/test_gpu_parity.py:738) integer costs with many ties
        return dict(cost=cost)

    def oracle(self, o, c):
        import scipy.optimize
        out = np.full((B, c["nr"]), -1, np.int64)
        for b in range(B):
            r0, c0 = scipy.optimize.linear_sum_assignment(o["cost"][b], maximize=bool(c["maximize"]))
            out[b, r0] = c0
        return dict(col=out)

    def lib(self, c):
        return "dm_linear_sum_assignment"

    def call(self, eng, T, c):
        eng.set_option("lsa_reg", c["lsa_reg"])
        return dict(col=eng.linear_sum_assignment(T["cost"], maximize=bool(c["maximize"])))

    def check(self, got, ref, c):
        return None if np.array_equal(got["col"], ref["col"]) else f"{(got['col'] != ref['col']).sum()} rows differ from SciPy"   # tests/test_gpu_parity.py:757


# ------------------------------------------------------------------------------------------------ functional map networks
FMN_N, FMN_PAD = 5, 3
FMN_EDGES = [(i, j) for i in range(FMN_N) for j in range(FMN_N) if i != j and (i + 2 * j) % 7 != 3]
U2 = 2.0 ** -53


def _fmn_maps(M, seed):
    rng = _rng("fmn", M, seed)
    E = len(FMN_EDGES)
    return np.stack([np.linalg.qr(rng.standard_normal((M, M)))[0] for _ in range(E)]) + 0.02 * rng.standard_normal((E, M, M))


class _FmnEntry(Entry):
    """maps are (E, ldm, ldm) with the leading M x M block used: rows AND columns behind M are padding"""
    ld_of, rows_of = ("maps",), ("maps",)

    def configs(self):
        return [dict(M=M) for M in (15, 16)]


class FmnOrthDefect(_FmnEntry):
    name = "fmn_orth_defect"

    def build(self, c):
        return dict(maps=_fmn_maps(c["M"], 0))

    def oracle(self, o, c):
        Cm, M = o["maps"], c["M"]
        return dict(d=np.asarray([np.linalg.norm(Cm[q].T @ Cm[q] - np.eye(M)) for q in range(len(Cm))]),
                    bound=np.asarray([M * U2 * np.linalg.norm(np.abs(Cm[q]).T @ np.abs(Cm[q])) for q in range(len(Cm))]))

    def lib(self, c):
        return "dm_fmn_orth_defect"

    def call(self, eng, T, c):
        return dict(d=eng.fmn_orth_defect(T["maps"], c["M"]))

    def check(self, got, ref, c):
        ok = np.isfinite(got["d"]).all() and np.all(np.abs(got["d"] - ref["d"]) <= ref["bound"])           # tests/test_gpu_fmn.py:110-112
        return None if ok else f"defect off by {np.abs(got['d'] - ref['d']).max():.3e}"


def _fmn_cycles():
    idx = {e: q for q, e in enumerate(FMN_EDGES)}
    return np.asarray([(idx[(i, j)], idx[(j, k)], idx[(k, i)]) for i in range(FMN_N) for j in range(FMN_N) for k in range(FMN_N)
                       if i < j and i < k and j != k and (i, j) in idx and (j, k) in idx and (k, i) in idx], np.int32)


class FmnCycleCosts(_FmnEntry):
    name = "fmn_cycle_costs"

    def build(self, c):
        return dict(maps=_fmn_maps(c["M"], 1), cyc=_fmn_cycles())

    def oracle(self, o, c):
        Cm, M, eye = o["maps"], c["M"], np.eye(c["M"])
        cost, bnd = [], []
        for a, b, cc in o["cyc"]:
            rots = [(a, b, cc), (b, cc, a), (cc, a, b)]
            cost.append(max(np.linalg.norm(Cm[x] @ Cm[y] @ Cm[z] - eye) for x, y, z in rots))
            bnd.append(max(2 * M * U2 * np.linalg.norm(np.abs(Cm[x]) @ np.abs(Cm[y]) @ np.abs(Cm[z])) for x, y, z in rots))
        return dict(cost=np.asarray(cost), bound=np.asarray(bnd))

    def lib(self, c):
        return "dm_fmn_cycle_costs"

    def call(self, eng, T, c):
        return dict(cost=eng.fmn_cycle_costs(T["maps"], c["M"], T["cyc"]))

    def check(self, got, ref, c):
        ok = np.isfinite(got["cost"]).all() and np.all(np.abs(got["cost"] - ref["cost"]) <= ref["bound"])   # tests/test_gpu_fmn.py:120-121
        return None if ok else f"cycle cost off by {np.abs(got['cost'] - ref['cost']).max():.3e}"


class FmnQuadForm(_FmnEntry):
    name = "fmn_quad_form"

    def build(self, c):
        rng = _rng("fmn_w", c["M"])
        w = rng.uniform(0.2, 1.7, len(FMN_EDGES))
        w[0], w[1] = 0.0, 1.0
        return dict(maps=_fmn_maps(c["M"], 2), edges=np.asarray(FMN_EDGES, np.int32), w=w)

    def oracle(self, o, c):
        from scipy import sparse
        from densematcher_amd.pyFM import CLB_quad_form
        M = c["M"]
        I, J = o["edges"][:, 0], o["edges"][:, 1]
        wm = sparse.csr_matrix((o["w"], (I, J)), shape=(FMN_N, FMN_N))
        W = CLB_quad_form({tuple(e): o["maps"][q] for q, e in enumerate(FMN_EDGES)}, wm, M=M).toarray()
        Wabs = CLB_quad_form({tuple(e): np.abs(o["maps"][q]) for q, e in enumerate(FMN_EDGES)}, wm, M=M).toarray()
        return dict(W=W, Wabs=np.abs(Wabs))

    def lib(self, c):
        return "dm_fmn_quad_form"

    def call(self, eng, T, c):
        return dict(W=eng.fmn_quad_form(FMN_N, c["M"], T["maps"], T["edges"], T["w"]))

    def check(self, got, ref, c):
        M, W = c["M"], got["W"]
        if not np.isfinite(W).all():
            return "non-finite quadratic form"
        deg = np.bincount(np.asarray(FMN_EDGES).ravel(), minlength=FMN_N)
        for bi in range(FMN_N):
            for bj in range(FMN_N):
                sl = (slice(bi * M, (bi + 1) * M), slice(bj * M, (bj + 1) * M))
                if bi != bj and not np.array_equal(W[sl], ref["W"][sl]):                                # tests/test_gpu_fmn.py:86
                    return f"block {bi},{bj} differs from the host's bits"
                if bi == bj and not np.all(np.abs(W[sl] - ref["W"][sl]) <= (M + deg[bi]) * U2 * ref["Wabs"][sl]):   # tests/test_gpu_fmn.py:88-91
                    return f"diagonal block {bi} outside the summation bound"
        return None


# ------------------------------------------------------------------------------------------------ padded batches
# Meshes of NV vertices in arrays of N >= NV rows (and, for the distance matrices, columns): what lies behind n_verts is padding.
# The index lists of these entries are ragged host lists that the engine checks against n_verts before anything is launched: there
# is no index padding to fill.
NV = 97


def _dist(rng):
    """a symmetric 'distance' matrix per mesh: positive off the diagonal, zero on it"""
    D = rng.uniform(0.1, 1.0, (B, NV, NV))
    D = 0.5 * (D + D.transpose(0, 2, 1))
    D[:, np.arange(NV), np.arange(NV)] = 0.0
    return D


def _lists(rng, sizes):
    return [rng.integers(0, NV, n) for n in sizes]


def _scipy_problem(block, maximize=False):
    from scipy.optimize import linear_sum_assignment
    r, c = linear_sum_assignment(block, maximize=maximize)
    col = np.full(block.shape[0], -1, np.int32)
    col[r] = c
    return col, block[r, c].mean()


class Fps(Entry):
    name, rows_only = "fps", ("verts",)
    SIZE = 40

    def configs(self):
        return [dict(start=s) for s in (0, 11)]

    def build(self, c):
        return dict(verts=_rng("fps").standard_normal((B, NV, 3)))

    def oracle(self, o, c):
        def greedy(V):                                      # (tests/test_gpu_fps.py: euclid_greedy)
            inds = [c["start"]]
            d = np.linalg.norm(V - V[inds[0]], axis=1)
            for _ in range(self.SIZE - 1):
                inds.append(int(np.argmax(d)))
                d = np.minimum(d, np.linalg.norm(V - V[inds[-1]], axis=1))
            return np.asarray(inds)
        return dict(idx=_per_pair(lambda b: greedy(o["verts"][b])))

    def lib(self, c):
        return "dm_fps_euclid"

    def call(self, eng, T, c):
        return dict(idx=eng.fps(T["verts"], self.SIZE, c["start"], n_verts=[NV] * B))

    def check(self, got, ref, c):
        return None if np.array_equal(got["idx"], ref["idx"]) else f"{(got['idx'] != ref['idx']).sum()} samples differ"   # tests/test_gpu_fps.py:70-72


class LsaGather(Entry):
    name, ld_of, rows_of = "lsa_gather", ("D",), ("D",)

    def configs(self):
        return [dict(maximize=m) for m in (0, 1)]

    def _problems(self):
        rng = _rng("lsa_gather_lists")
        sizes_r, sizes_c = (1, 7, 33, 64, 20, 97), (5, 7, 20, 64, 45, 97)
        return _lists(rng, sizes_r), _lists(rng, sizes_c), np.asarray([0, 1, 2, 0, 1, 2])

    def build(self, c):
        return dict(D=_dist(_rng("lsa_gather")))

    def oracle(self, o, c):
        rows, cols, mesh = self._problems()
        per = [_scipy_problem(o["D"][m][np.ix_(r, cc)], bool(c["maximize"])) for r, cc, m in zip(rows, cols, mesh)]
        return dict(assign=np.concatenate([p[0] for p in per]), mean=np.asarray([p[1] for p in per]),
                    n=np.asarray([min(len(r), len(cc)) for r, cc in zip(rows, cols)]))

    def lib(self, c):
        return "dm_lsa_gather"

    def call(self, eng, T, c):
        rows, cols, mesh = self._problems()
        means, assign = eng.lsa_gather(T["D"], rows, cols, mesh=mesh, maximize=bool(c["maximize"]), return_assignment=True, n_verts=[NV] * B)
        return dict(mean=means, assign=np.concatenate(assign))

    def check(self, got, ref, c):
        if not np.array_equal(got["assign"], ref["assign"]):
            return "an assignment differs from SciPy's"                           # tests/test_gpu_groups.py:70
        ok = np.isfinite(got["mean"]).all() and np.all(np.abs(got["mean"] - ref["mean"]) <= ref["n"] * 2.0 ** -52 * np.abs(ref["mean"]))
        return None if ok else "a mean outside n 2^-52 |ref|"                       # tests/test_gpu_groups.py:71-73


class GroupsDmtx(Entry):
    name, ld_of, rows_of = "groups_dmtx", ("D",), ("D",)

    def configs(self):
        return [dict()]

    def _groups(self):
        rng = _rng("groups")
        return [_lists(rng, sz) for sz in ((3, 17, 40), (9, 9, 31, 2), (64, 33))]

    def build(self, c):
        return dict(D=_dist(_rng("groups_dmtx")))

    def oracle(self, o, c):
        out, bnd = [], []
        for b, gs in enumerate(self._groups()):
            for i in range(len(gs)):
                for j in range(i + 1, len(gs)):
                    out.append(_scipy_problem(o["D"][b][np.ix_(gs[i], gs[j])])[1])
                    bnd.append(min(len(gs[i]), len(gs[j])))
        return dict(m=np.asarray(out), n=np.asarray(bnd))

    def lib(self, c):
        return "dm_lsa_gather"

    def call(self, eng, T, c):
        mats = eng.groups_dmtx(T["D"], self._groups(), n_verts=[NV] * B)
        flat = []
        for M in mats:
            assert np.array_equal(M, M.T) and np.all(np.diag(M) == 0)
            flat.append(M[np.triu_indices(len(M), 1)])
        return dict(m=np.concatenate(flat))

    def check(self, got, ref, c):
        ok = np.isfinite(got["m"]).all() and np.all(np.abs(got["m"] - ref["m"]) <= ref["n"] * 2.0 ** -52 * np.abs(ref["m"]))
        return None if ok else "a group distance outside n 2^-52 |ref|"             # tests/groups_restate.py: mean_bound, tests/test_gpu_groups.py:208


LENGTHS = (1, 63, 64, 65, 97, 300)


class MapAccuracy(Entry):
    name, ld_of, rows_of = "map_accuracy", ("D",), ("D",)

    def configs(self):
        return [dict(scale=sc) for sc in ("none", "diameter")]

    def _maps(self):
        rng = _rng("accuracy_lists")
        return _lists(rng, LENGTHS), _lists(rng, LENGTHS), np.arange(len(LENGTHS)) % B

    def build(self, c):
        return dict(D=_dist(_rng("map_accuracy")))

    def oracle(self, o, c):
        p2p, gt, mesh = self._maps()
        d = [o["D"][m][(a, g)] / (o["D"][m].max() if c["scale"] == "diameter" else 1.0) for a, g, m in zip(p2p, gt, mesh)]
        return dict(d=np.concatenate(d), mean=np.asarray([x.mean() for x in d]))

    def lib(self, c):
        return "dm_map_metrics"

    def call(self, eng, T, c):
        p2p, gt, mesh = self._maps()
        means, dists = eng.map_accuracy(T["D"], p2p, gt, mesh=mesh, scale=None if c["scale"] == "none" else "diameter", return_all=True,
                                        n_verts=[NV] * B)
        return dict(mean=means, d=np.concatenate(dists))

    def check(self, got, ref, c):
        if not np.array_equal(got["d"], ref["d"]):
            return "a distance differs from the host's"                            # tests/test_gpu_eval.py:109
        ok = np.all(np.abs(got["mean"] - ref["mean"]) <= np.asarray(LENGTHS) * 2.0 ** -52 * np.abs(ref["mean"]))
        return None if ok else "a mean outside n 2^-52 |ref|"                       # tests/test_gpu_eval.py:79-81


class MapContinuity(Entry):
    name, ld_of, rows_of = "map_continuity", ("D1", "D2"), ("D1", "D2")
    NE = (1, 70, 300)

    def configs(self):
        return [dict()]

    def _maps(self):
        rng = _rng("continuity_lists")
        edges = []
        for n in self.NE:
            e = rng.integers(0, NV, (n, 2))
            e[:, 1] = np.where(e[:, 1] == e[:, 0], (e[:, 0] + 1) % NV, e[:, 1])     # (no edge of length zero)
            edges.append(e)
        return [rng.integers(0, NV, NV) for _ in self.NE], edges, np.arange(len(self.NE)) % B

    def build(self, c):
        return dict(D1=_dist(_rng("map_continuity", 1)), D2=_dist(_rng("map_continuity", 2)))

    def oracle(self, o, c):
        p2p, edges, mesh = self._maps()
        return dict(v=np.asarray([np.mean(o["D1"][m][(p[e[:, 0]], p[e[:, 1]])] / o["D2"][m][(e[:, 0], e[:, 1])]) for p, e, m in zip(p2p, edges, mesh)]))

    def lib(self, c):
        return "dm_map_metrics"

    def call(self, eng, T, c):
        p2p, edges, mesh = self._maps()
        return dict(v=eng.map_continuity(T["D1"], T["D2"], p2p, edges, mesh1=mesh, mesh2=mesh, n_verts1=[NV] * B, n_verts2=[NV] * B))

    def check(self, got, ref, c):
        ok = np.all(np.abs(got["v"] - ref["v"]) <= np.asarray(self.NE) * 2.0 ** -52 * np.abs(ref["v"]))
        return None if ok else "a continuity outside n 2^-52 |ref|"                 # tests/test_gpu_eval.py:79-81, 135


class MapCoverage(Entry):
    name, ld_of = "map_coverage", ("area",)

    def configs(self):
        return [dict()]

    def _maps(self):
        rng = _rng("coverage_lists")
        return _lists(rng, (1, 50, 97, 400)), np.arange(4) % B

    def build(self, c):
        return dict(area=_rng("map_coverage").uniform(0.5, 1.5, (B, NV)))

    def oracle(self, o, c):
        p2p, mesh = self._maps()
        return dict(v=np.asarray([o["area"][m][np.unique(p)].sum() / o["area"][m].sum() for p, m in zip(p2p, mesh)]),
                    n=np.asarray([len(np.unique(p)) + NV for p in p2p]))

    def lib(self, c):
        return "dm_map_metrics"

    def call(self, eng, T, c):
        p2p, mesh = self._maps()
        return dict(v=eng.map_coverage(T["area"], p2p, mesh=mesh, n_verts=[NV] * B))

    def check(self, got, ref, c):
        ok = np.all(np.abs(got["v"] - ref["v"]) <= ref["n"] * 2.0 ** -52 * np.abs(ref["v"]))
        return None if ok else "a coverage outside n 2^-52 |ref|"                   # tests/test_gpu_eval.py:79-81, 168


class Signatures(Entry):
    """plain heat / wave kernel signatures of meshes padded to N rows: rows past n_verts are exactly 0"""
    name, ld_of, rows_only = "signatures", ("Phi",), ("Phi",)
    K, NUM = 15, 6

    def configs(self):
        return [dict(dt=dt, kind=kind) for dt in DTS for kind in ("HKS", "WKS")]

    def build(self, c):
        rng = _rng("signatures", c["dt"])
        return dict(Phi=(rng.standard_normal((B, NV, self.K)) / np.sqrt(NV)).astype(NPDT[c["dt"]]))

    def _lam(self):
        lam = np.sort(_rng("signatures_lam").uniform(0.5, 60.0, (B, self.K)), axis=1)
        lam[:, 0] = 1e-9
        return lam

    def oracle(self, o, c):
        from densematcher_amd.pyFM import signatures as sg
        S, b, kept = [], [], []
        for q in range(B):                                   # (tests/test_gpu_signatures.py: _mirror, plain block)
            lam, ev = self._lam()[q], o["Phi"][q].astype(np.float64)
            t, mu, denom, k0 = sg.signature_tables(lam, c["kind"], self.NUM, False)
            w = np.exp(-(t[:, None] * mu[None, :])) if c["kind"] == "HKS" else np.exp(-np.square(t[:, None] - mu[None, k0:]) / denom)
            E = ev[:, k0:]
            S.append((sg.auto_HKS if c["kind"] == "HKS" else sg.auto_WKS)(lam, ev, self.NUM))
            b.append(((E * E) @ w.T) * (1.0 / w.sum(axis=1))[None, :])
            kept.append(E.shape[1])
        return dict(S=np.stack(S), b=np.stack(b), kept=np.asarray(kept, np.float64))

    def lib(self, c):
        return "dm_spectral_signatures" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        out = eng.signatures(T["Phi"], self._lam(), c["kind"], self.NUM, n_verts=[NV] * B)
        assert bool((out[:, NV:] == 0).all()), "rows past n_verts are not exactly 0"
        return dict(S=out[:, :NV])

    def check(self, got, ref, c):
        tol = 4.0 * (ref["kept"][:, None, None] + 8.0) * 2.0 ** -53 * ref["b"]      # tests/test_gpu_signatures.py:73
        ok = np.isfinite(got["S"]).all() and np.all(np.abs(got["S"] - ref["S"]) <= tol)
        return None if ok else "a signature outside 4 (kept + 8) u b"


class EighSmallest(Entry):
    """the k smallest eigenpairs of dense symmetric matrices; the engine hands the matrix over with lda = n (no row padding to fill)"""
    name = "eigh_smallest"
    N, K = 65, 6

    def configs(self):
        return [dict(route=r) for r in (1, 2)]

    def build(self, c):
        rng = _rng("eigh")
        Q = np.stack([np.linalg.qr(rng.standard_normal((self.N, self.N)))[0] for _ in range(B)])
        lam = np.sort(rng.uniform(0.0, 1.0, (B, self.N)), axis=1) + 0.05 * np.arange(self.N)[None, :]       # (gaps of at least 0.05)
        A = np.einsum("bik,bk,bjk->bij", Q, lam, Q)
        return dict(A=0.5 * (A + A.transpose(0, 2, 1)))

    def oracle(self, o, c):
        per = [np.linalg.eigh(o["A"][b]) for b in range(B)]
        return dict(lam=np.stack([p[0] for p in per]), V=np.stack([p[1] for p in per]), diag=np.stack([np.abs(np.diag(o["A"][b])).max() for b in range(B)]))

    def lib(self, c):
        return "dm_eigh_smallest"

    def call(self, eng, T, c):
        eng.set_option("fmn_eig_route", c["route"])
        lam, V, resid, _ = eng.eigh_smallest(T["A"], self.K)
        return dict(lam=lam, V=V, resid=resid)

    def check(self, got, ref, c):
        n, k = self.N, self.K
        for b in range(B):                                   # tests/test_gpu_fmn.py:176-182
            lam, V, resid, full = got["lam"][b], got["V"][b], float(got["resid"][b]), ref["lam"][b]
            lmax = np.abs(full).max()
            if not (np.isfinite(V).all() and resid <= 1e-9 * ref["diag"][b]):
                return f"matrix {b}: residual {resid:.3e}"
            if not np.all(np.abs(lam - full[:k]) <= np.sqrt(n) * resid + n * U2 * lmax):
                return f"matrix {b}: eigenvalues off by {np.abs(lam - full[:k]).max():.3e}"
            if np.abs(V.T @ V - np.eye(k)).max() > 1e-12:
                return f"matrix {b}: columns not orthonormal"
            Vr = ref["V"][b][:, :k]
            if np.linalg.norm(V @ V.T - Vr @ Vr.T, 2) > 2 * np.sqrt(n * k) * resid / (full[k] - full[k - 1]):
                return f"matrix {b}: invariant subspace off"
            if not np.all(V[np.abs(V).argmax(axis=0), np.arange(k)] > 0):
                return f"matrix {b}: sign rule"
        return None


class PreciseMap(Entry):
    """barycentric projection of mesh 2's vertices onto mesh 1's faces in the spectral embedding (emb1 = Phi1[:, :k1], emb2 = Phi2 C)"""
    name, ld_of = "precise_map", ("Phi1", "Phi2")
    NA, NB, NF = 60, 45, 70          # (the oracle walks every point-face pair in Python)

    def configs(self):
        return [dict(dt=dt, k1=k1, k2=k2) for dt in DTS for k1, k2 in KPAIRS]

    def build(self, c):
        rng = _rng("precise", c["dt"], c["k1"], c["k2"])
        faces = np.stack([np.stack([rng.choice(self.NA, 3, replace=False) for _ in range(self.NF)]) for _ in range(B)]).astype(np.int32)
        return dict(Phi1=(rng.standard_normal((B, self.NA, c["k1"])) * 0.3).astype(NPDT[c["dt"]]),
                    Phi2=(rng.standard_normal((B, self.NB, c["k2"])) * 0.3).astype(NPDT[c["dt"]]),
                    C=rng.standard_normal((B, c["k2"], c["k1"])) / np.sqrt(c["k2"]), faces=faces)

    @staticmethod
    def _dist(o, b, fm, bary):
        V, P = o["Phi1"][b].astype(np.float64), o["Phi2"][b].astype(np.float64) @ o["C"][b]
        proj = (np.asarray(bary)[:, :, None] * V[o["faces"][b][np.asarray(fm)]]).sum(1)        # (tests/precise_restate.py: projected)
        return np.linalg.norm(proj - P, axis=1)

    def oracle(self, o, c):
        per = [orc.precise_map_dense(o["C"][b], o["Phi1"][b], o["Phi2"][b], o["faces"][b]) for b in range(B)]
        return dict(d=np.stack([self._dist(o, b, per[b][1], per[b][2]) for b in range(B)]), Phi1=o["Phi1"], Phi2=o["Phi2"], C=o["C"], faces=o["faces"])

    def lib(self, c):
        return "dm_precise_map" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        fm, bary = eng.precise_map(T["Phi1"], T["Phi2"], T["C"], T["faces"])
        return dict(fm=fm, bary=bary)

    def check(self, got, ref, c):
        o = ref                                             # (the logical operands ride along: the distances are formed here)
        if got["fm"].min() < 0 or got["fm"].max() >= self.NF or not np.isfinite(got["bary"]).all():
            return "a face index outside the mesh or non-finite weights"
        if np.abs(got["bary"].sum(-1) - 1.0).max() > 1e-12:                                         # tests/test_gpu_precise.py:74
            return "weights do not sum to 1"
        for b in range(B):
            e = np.abs(self._dist(o, b, got["fm"][b], got["bary"][b]) - ref["d"][b]).max()
            if e > 1e-9 * max(1.0, ref["d"][b].max()):                                              # tests/test_gpu_precise.py:267
                return f"pair {b}: projected distance off by {e:.3e}"
        return None


class OrientationOps(Entry):
    """The faces go through the host (the engine checks them there and uploads its own copy), so only their PADDING is hostile here:
    five rows behind n_faces hold an index outside every mesh, which the entry documents it does not read."""
    name, ld_of = "orientation_ops", ("Phi",)
    D = 6

    def configs(self):
        return [dict(dt=dt, k=k, fdt=fdt) for dt in DTS for k in (15, 16) for fdt in ("f16", "f32")]

    def _mesh(self):
        from densematcher_amd import synth
        meshes = [synth.torus_mesh(12, 10, perturb=0.05 * (q + 1), seed=q) for q in range(B)]      # (tests/test_gpu_orient_ops.py:145)
        return np.stack([np.asarray(v, np.float64) for v, _ in meshes]), np.stack([np.asarray(f, np.int32) for _, f in meshes])

    def build(self, c):
        rng = _rng("orient", c["dt"], c["k"], c["fdt"])
        verts, _ = self._mesh()
        n = verts.shape[1]
        return dict(verts=verts, Phi=(rng.standard_normal((B, n, c["k"])) / np.sqrt(n)).astype(NPDT[c["dt"]]),
                    F=rng.standard_normal((B, n, self.D)).astype(np.float16 if c["fdt"] == "f16" else np.float32))

    def oracle(self, o, c):
        _, faces = self._mesh()
        n = o["verts"].shape[1]
        return dict(ops=_per_pair(lambda b: orc.orientation_ops(o["Phi"][b].astype(np.float64), np.ones(n), o["verts"][b], faces[b],
                                                                o["F"][b].astype(np.float64))))

    def lib(self, c):
        return "dm_fmap_orient_ops" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        _, faces = self._mesh()
        m = faces.shape[1]
        padded = np.concatenate([faces, np.full((B, 5, 3), 2 ** 30, np.int32)], axis=1)
        return dict(ops=eng.orientation_ops(T["verts"], padded, T["Phi"], T["F"], k=c["k"], n_faces=[m] * B))

    def check(self, got, ref, c):
        e = _maxerr(got["ops"], ref["ops"], np.abs(ref["ops"]).max())
        return None if e <= 1e-11 else f"relative error {e:.3e} > 1e-11"           # tests/test_gpu_orient_ops.py:17, 66


class LsaIndicator(Entry):
    name, ld_of = "lsa_indicator", ("Phi1", "Phi2")

    def configs(self):
        return [dict(dt=dt, k1=k1, k2=k2) for dt in DTS for k1, k2 in KPAIRS]

    def build(self, c):
        # (dm_lsa_indicator takes N2 <= N1: the larger mesh is the source here)
        rng = _rng("lsa_indicator", c["dt"], c["k1"], c["k2"])
        return dict(Phi1=_basis(rng, N2, c["k1"], c["dt"]), Phi2=_basis(rng, N1, c["k2"], c["dt"]), a1=_mass(rng, N2, c["dt"]),
                    C=rng.standard_normal((B, c["k2"], c["k1"])))

    def oracle(self, o, c):
        return dict(col=_per_pair(lambda b: _scipy_problem(orc.mapped_indicator(o["C"][b], o["Phi1"][b], o["Phi2"][b], o["a1"][b]), True)[0]))

    def lib(self, c):
        return "dm_lsa_indicator" + ("_f64" if c["dt"] == "f64" else "")

    def call(self, eng, T, c):
        return dict(col=eng.lsa_indicator(T["Phi1"], T["Phi2"], T["a1"], T["C"]))

    def check(self, got, ref, c):
        return None if np.array_equal(got["col"], ref["col"]) else f"{(got['col'] != ref['col']).sum()} rows differ from SciPy"   # tests/test_gpu_api.py:903


# ------------------------------------------------------------------------------------------------ nearest neighbours
class KnnQuery(Entry):
    name = "knn_query"

    def configs(self):
        return [dict(p=p, knn_split=ks) for p in (15, 16) for ks in (1, 0)]

    def build(self, c):
        rng = _rng("knn", c["p"])
        return dict(X=rng.standard_normal((B, N1, c["p"])), Y=rng.standard_normal((B, N2, c["p"])))

    def oracle(self, o, c):
        return dict(nn=_per_pair(lambda b: orc.knn_query(o["X"][b], o["Y"][b])))

    def lib(self, c):
        return "dm_knn_query_f64"

    def call(self, eng, T, c):
        eng.set_option("knn_split", c["knn_split"])
        return dict(nn=eng.knn_query(T["X"], T["Y"]))

    def check(self, got, ref, c):
        return None if np.array_equal(got["nn"], ref["nn"]) else f"{(got['nn'] != ref['nn']).sum()} mismatches"   # tests/test_gpu_parity.py:470-488


class KnnTopk(Entry):
    name = "knn_query_topk"

    def configs(self):
        return [dict(p=p, k=6) for p in (15, 16)]

    def build(self, c):
        rng = _rng("knntopk", c["p"])
        return dict(X=rng.standard_normal((B, N1, c["p"])), Y=rng.standard_normal((B, N2, c["p"])))

    def oracle(self, o, c):
        per = [orc.knn_query_topk(o["X"][b], o["Y"][b], c["k"]) for b in range(B)]
        return dict(dist=np.stack([p[0] for p in per]), idx=np.stack([p[1] for p in per]))

    def lib(self, c):
        return "dm_knn_query_topk_f64"

    def call(self, eng, T, c):
        idx, dist = eng.knn_query_topk(T["X"], T["Y"], c["k"])
        return dict(idx=idx, dist=dist)

    def check(self, got, ref, c):
        if not np.array_equal(got["idx"], ref["idx"]):
            return f"idx: {(got['idx'] != ref['idx']).sum()} mismatches"          # tests/test_gpu_api.py:579
        e = _maxerr(got["dist"], ref["dist"], max(1.0, ref["dist"].max()))
        return None if e <= 1e-12 else f"distance error {e:.3e} > 1e-12"           # tests/test_gpu_api.py:563


ENTRIES = [Project(), C00(), FmapFit(), FmapSolve(), DescrOps(), EnergyGrad(), EnergyGradFused(), FmToP2p(), MappedIndicator(), P2pToFm(), P2pToFmLstsq(), ZoomOut(), ZoomOutSub(), Icp(),
           KnnQuery(), KnnTopk(), Lsa(), FmnOrthDefect(), FmnCycleCosts(), FmnQuadForm(),
           EighSmallest(), PreciseMap(), OrientationOps(), LsaIndicator(), Fps(), LsaGather(), GroupsDmtx(), MapAccuracy(), MapContinuity(), MapCoverage(), Signatures()]


def all_cases():
    return [(e, c) for e in ENTRIES for c in e.configs()]


def case_id(ec):
    e, c = ec
    return e.name + "[" + ",".join(f"{k}={v}" for k, v in c.items()) + "]"

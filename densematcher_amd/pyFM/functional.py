"""
FunctionalMapping with the reference's interface (densematcher/pyFM/functional.py:19), restricted to what the
matching hot path uses.  Arithmetic: libdensematch (HIP) through densematcher_amd.engine.
"""
import copy

import numpy as np
from scipy import sparse

from . import refine, signatures as sg, spectral

_OPTIMIZERS = ("L-BFGS-B", "fmin_l_bfgs_b", "l-bfgs-b")
# L-BFGS stopping rule of the iterative fit.  The reference passes only maxiter (SciPy defaults ftol = 2.2e-9, gtol = 1e-5,
# maxcor = 10) and evaluates in float32, which stops 1e-4 .. 1e-3 short of the minimiser.  The float64
# evaluation here makes a tight rule meaningful: fit(..., stopping="tight") runs the options below (the 1e-4 parity bar on C against
# the float64 minimiser is tested with it); the DEFAULT is stopping="reference", SciPy's default rule, because a drop-in should end
# where the code it replaces ends: against the reference's own 14-tuple the ICP slots agree 0.97 / 0.98 with it, 0.92 / 0.90 tight.
# ftol = 1e-12: the energy is flat around its minimiser, and WHEN a relative decrease of a few machine epsilons is first seen
# is decided by rounding noise -- on the notebook's fit the same rule took 289, 322, 351, 440 or 448 evaluations at 1e-13 (740
# or 1690 at 1e-15) as summation orders inside the evaluation changed, for maps that agree to 2e-5.  Measured on that fit
# (tools/fit_profile.py <ftol>; distance of C from the 1e-15 result): 1e-14 464 evaluations 8e-7, 1e-13 448 1e-6,
# 1e-12 332 9e-6, 1e-11 261 4e-5, 1e-10 224 1.3e-4.  1e-12 keeps a factor ten under the 1e-4 bar on C.
CLOSED_FORM_MAX_K1 = 200          # dm_fmap_solve / dm_fmap_fit: the in-LDS solvers take systems of order <= 199
LBFGS_OPTIONS = {"ftol": 1e-12, "gtol": 1e-9, "maxcor": 30, "maxfun": 15000}
# maps wider than the closed form takes (quadratic energy, k^2 > 40 000 unknowns): run until the gradient test or the line search's noise floor
LBFGS_WIDE = {"ftol": 1e-15, "gtol": 1e-11, "maxcor": 30, "maxfun": 50000}


# FunctionalMapping.fit's parameters and their defaults (functional.py:352-360, and what is not in the reference: stopping, driver,
# orient_route).  compute_surface_map_batch's fit_params are the same names.  (fit keeps its explicit signature, like the reference's;
# tests/test_fit_stage_cpu.py holds the two lists together.)
FIT_DEFAULTS = dict(w_descr=1e-1, w_lap=1e-3, w_dcomm=1, w_orient=0, w_area=0, w_conformal=0, w_p2p=0, w_stochastic=0, w_ent=0, w_range01=0,
                    w_sumto1=0, w_area_difference=0, w_mumford_shah=0, mumford_shah_var=0.1, w_eta_entropy=0, orient_reversing=False,
                    optinit='zeros', verbose=False, maxiter=1000000, device=None, stopping="reference", driver="device", orient_route="host")
_OFF_PATH_TERMS = ("w_area_difference", "w_mumford_shah", "w_eta_entropy")
_ITERATIVE_TERMS = ("w_dcomm", "w_p2p", "w_stochastic", "w_ent", "w_range01", "w_sumto1", "w_orient", "w_area", "w_conformal")


def fit_parameters(given):
    """FIT_DEFAULTS with the caller's values, checked -- host code only, nothing here needs a device"""
    unknown = set(given) - set(FIT_DEFAULTS)
    if unknown:
        raise TypeError(f"fit() got unexpected keyword arguments {sorted(unknown)}")
    p = dict(FIT_DEFAULTS, **given)
    if p["orient_route"] not in ("host", "device"):
        raise ValueError(f'orient_route must be "host" or "device", not {p["orient_route"]!r}')
    if p["optinit"] not in ('random', 'identity', 'zeros'):
        raise ValueError(f"optinit arg should be 'random', 'identity' or 'zeros', not {p['optinit']}")
    if p["stopping"] not in ("tight", "reference"):
        raise ValueError("stopping must be 'tight' or 'reference'")
    live = [n for n in _OFF_PATH_TERMS if p[n] > 0]
    if live:
        raise NotImplementedError(f"energy terms {live} are not on the accelerated path; pass 0")
    if not any(p[n] > 0 for n in ("w_descr", "w_lap") + _ITERATIVE_TERMS):
        raise ValueError("every energy weight is 0")                           # base_functions.py:534,639 would fail too
    return p


def fit_plan(p, k1):
    """(route, L-BFGS options) of a fit with the parameters p (fit_parameters) of maps with k1 columns.
    "closed": only w_descr / w_lap and at most CLOSED_FORM_MAX_K1 columns -- the closed form solves k2 systems of order k1 - 1 in
    on-chip memory.  Wider quadratic fits (the reference has no cap, functional.py:352) take the reference's own scheme -- L-BFGS on
    the two quadratic terms, on the device, float64 -- run to LBFGS_WIDE whatever `stopping` says: they replace a closed form.
    Any other term: "iterative" with the rule `stopping` names at every width, LBFGS_OPTIONS ("tight") or SciPy's defaults (None)."""
    if any(p[n] > 0 for n in _ITERATIVE_TERMS):
        return "iterative", (LBFGS_OPTIONS if p["stopping"] == "tight" else None)
    if k1 > CLOSED_FORM_MAX_K1:
        return "iterative", LBFGS_WIDE
    return "closed", None


def _orient_row_scale(mesh):
    """mass / vertex_areas, the row scale that turns Phi into the left factor of compute_orientation_op's operators (pinv = Phi^T A, rows
    divided by vertex_areas); None where it is 1 everywhere (TriMesh: the row sums of a lumped A are its diagonal), i.e. the "mass" form"""
    mass = np.asarray(mesh.A.diagonal(), dtype=np.float64)
    if (mesh.A - sparse.diags(mesh.A.diagonal())).count_nonzero() != 0:
        raise NotImplementedError("the device route of the orientation operators takes a lumped (diagonal) mass matrix; use the host route")
    va = np.asarray(mesh.vertex_areas, dtype=np.float64)
    return None if np.array_equal(mass, va) else mass / va


def _orientation_ops_device(eng, models, Phis, Fs, area):
    """the orientation operators of a group of models of one size, both meshes, as device tensors (nb, D, k1, k1), (nb, D, k2, k2), never
    reversed (MatchEngine.orientation_ops on the stacked meshes; face counts may differ inside a group: padded, n_faces), and whether
    `area` made a difference.  Phis: the stacked bases in the meshes' own precision, Fs: the stacked descriptors as the fit stages them
    (fp16 when both sets are fp16, else fp32).  area "vertex": rows divided by vertex_areas, "mass": by diag(A) -- lumped masses ARE the
    vertex areas, the two forms are then the same operators."""
    if area not in ("vertex", "mass"):
        raise ValueError(f'area must be "vertex" or "mass", not {area!r}')
    out, scaled = [], False
    for side, (Phi, F) in enumerate(zip(Phis, Fs)):
        meshes = [(m.mesh1, m.mesh2)[side] for m in models]
        k = (models[0].k1, models[0].k2)[side]
        verts = np.stack([np.asarray(m.vertlist, dtype=np.float64) for m in meshes])
        nf = np.array([m.facelist.shape[0] for m in meshes], dtype=np.int32)
        faces = np.zeros((len(meshes), int(nf.max()), 3), dtype=np.int32)
        for q, m in enumerate(meshes):
            faces[q, :nf[q]] = m.facelist
        rs = [_orient_row_scale(m) for m in meshes]
        scale = None
        if any(r is not None for r in rs):
            scaled = True
            if area == "vertex":
                scale = np.stack([np.ones(m.n_vertices) if r is None else r for m, r in zip(meshes, rs)])
        out.append(eng.orientation_ops(verts, faces, Phi, F, k=k, row_scale=scale, n_faces=nf))
    return tuple(out), scaled


def _orientation_ops(eng, models, p, own, dev):
    """both operator sets of functional.py:432-456 for a group, each a pair (nb, D, k, k): the rescaling operators (rows divided by
    vertex_areas, the second reversed on request: compute_orientation_op) and those the optimisation runs with (energy_func_std rebuilds
    them itself, base_functions.py:567-597: rows divided by diag(A), never reversed) -- both restated as they are."""
    if p["orient_route"] == "host":
        st = lambda ops, side: np.stack([np.stack([o[side] for o in ops_q]) for ops_q in ops])
        resc = [m.compute_orientation_op(reversing=p["orient_reversing"]) for m in models]
        fit = [m.compute_orientation_op(reversing=False, area="mass") for m in models]
        return (st(resc, 0), st(resc, 1)), (st(fit, 0), st(fit, 1))
    Fs = (dev["F1"], dev["F2"])
    (r1, r2), scaled = _orientation_ops_device(eng, models, own[:2], Fs, "vertex")
    fit = _orientation_ops_device(eng, models, own[:2], Fs, "mass")[0] if scaled else (r1, r2)
    return (r1, -r2 if p["orient_reversing"] else r2), fit


def fit_models(eng, models, p, dev, own, report=None):
    """The fit of a group of models of one size (FunctionalMapping.fit passes [self], compute_surface_map_batch its size groups): from the
    staged inputs to C (nb, k2, k1) float64, stored on the models with fit_result, eta and w_orient_rescaled.
    p: fit_parameters(...); dev: the fit's device inputs, stacked (Phi1, Phi2, a1, a2 fp32 like the reference's fit, functional.py:412-413;
    lam1, lam2 float64; F1, F2 fp16 | fp32); own = (Phi1, Phi2, a1, a2): stacked bases and masses in the meshes' own precision (the
    pinned entry of the closed form, the device route of the orientation operators); report(eng, dev, weights, x, orient_ops, where):
    called at the start point and at the solution of an iterative fit."""
    import types
    nb = len(models)
    route, lbfgs_options = fit_plan(p, dev["Phi1"].shape[2])
    res = None
    if route == "closed":
        A = eng.project(dev["Phi1"], dev["a1"], dev["F1"])
        B = eng.project(dev["Phi2"], dev["a2"], dev["F2"])
        # pinned entry from the float64 spectrum and masses (get_x0 is float64 host code in the reference, :654-658)
        c00 = eng.c00(*own)
        C = eng.fmap_solve(A, B, dev["lam1"], dev["lam2"], c00, p["w_descr"], p["w_lap"], check=True).cpu().numpy()
    else:
        weights = {n: p[n] for n in ("w_descr", "w_lap") + _ITERATIVE_TERMS}
        x0 = np.stack([m.get_x0(optinit=p["optinit"]) for m in models])
        orient_ops = None
        if p["w_orient"] > 0:
            # functional.py:432-456: every pair's weight rescaled by (energy of the other terms at x0) / (orientation energy at x0)
            resc_ops, orient_ops = _orientation_ops(eng, models, p, own, dev)
            e_native = eng.fit_energy(dev, dict(weights, w_orient=0.0), x0)
            e_orient = eng.fit_energy(dev, dict(w_orient=1.0), x0, orient_ops=resc_ops)
            w_orient = [p["w_orient"] * float(e_native[q]) / float(e_orient[q]) for q in range(nb)]
            for q, m in enumerate(models):
                m.w_orient_rescaled = w_orient[q]
            weights["w_orient"] = np.asarray(w_orient, dtype=np.float64)
        if report is not None:
            report(eng, dev, weights, x0, orient_ops, "x0")
        C, res = eng.fit_general(dev, weights, x0, maxiter=p["maxiter"], lbfgs_options=lbfgs_options, driver=p["driver"], orient_ops=orient_ops)
        C = np.asarray(C, dtype=np.float64)
        if report is not None:
            report(eng, dev, weights, C, orient_ops, "solution")
    for q, m in enumerate(models):
        m.FM = C[q]
        m.eta = np.ones(m.mesh2.eigenvectors.shape[0])                         # functional.py:483
        if res is not None:
            # (a group's result holds one entry per pair: every model keeps its own slice.  A group of one keeps the result as it is:
            #  with driver="scipy" -- one pair per call -- it is SciPy's OptimizeResult, which has no per-pair axis to slice)
            m.fit_result = res if nb == 1 else types.SimpleNamespace(nit=res.nit[q:q + 1], nfev=res.nfev[q:q + 1], fun=res.fun[q:q + 1],
                                                                     status=res.status[q:q + 1], message=res.message[q:q + 1])
    return C, res


class FunctionalMapping:
    def __init__(self, mesh1, mesh2, partial=False, optimizer="fmin_l_bfgs_b"):
        self.mesh1 = copy.deepcopy(mesh1)          # functional.py:58-59
        self.mesh2 = copy.deepcopy(mesh2)
        self.descr1 = None
        self.descr2 = None
        self._FM_type = 'classic'
        self._FM_base = None
        self._FM_icp = None
        self._FM_zo = None
        self.SD_a = None                           # functional.py:72-73 (compute_SD itself sets D_a / D_c: the reference's names, both kept)
        self.SD_c = None
        self._k1, self._k2 = None, None
        self.optimizer = optimizer
        self.partial = partial
        self.eta = None
        self.mapped_indicator = None

    # ---------------------------------------------------------------- dimensions / state (functional.py:79-199)
    @property
    def k1(self):
        if self._k1 is None and not self.preprocessed and not self.fitted:
            raise ValueError('No information known about dimensions')
        return self.FM.shape[1] if self.fitted else self._k1

    @k1.setter
    def k1(self, k1):
        self._k1 = k1

    @property
    def k2(self):
        if self._k2 is None and not self.preprocessed and not self.fitted:
            raise ValueError('No information known about dimensions')
        return self.FM.shape[0] if self.fitted else self._k2

    @k2.setter
    def k2(self, k2):
        self._k2 = k2

    @property
    def FM_type(self):
        return self._FM_type

    @FM_type.setter
    def FM_type(self, FM_type):
        if FM_type.lower() not in ['classic', 'icp', 'zoomout']:
            raise ValueError(f'FM_type can only be set to "classic", "icp" or "zoomout", not {FM_type}')
        self._FM_type = FM_type

    def change_FM_type(self, FM_type):
        self.FM_type = FM_type

    @property
    def FM(self):
        return {'classic': self._FM_base, 'icp': self._FM_icp, 'zoomout': self._FM_zo}[self.FM_type.lower()]

    @FM.setter
    def FM(self, FM):
        self._FM_base = FM

    @property
    def preprocessed(self):
        test_descr = (self.descr1 is not None) and (self.descr2 is not None)
        test_evals = (self.mesh1.eigenvalues is not None) and (self.mesh2.eigenvalues is not None)
        test_evects = (self.mesh1.eigenvectors is not None) and (self.mesh2.eigenvectors is not None)
        return test_descr and test_evals and test_evects

    @property
    def fitted(self):
        return self.FM is not None

    def _get_lmks(self, landmarks, verbose=False):
        # (p,) / (p,1): the same vertex indices on both meshes; (p,2): one column per mesh      functional.py:253-262
        lm = np.asarray(landmarks)
        if lm.squeeze().ndim == 1:
            return lm.squeeze(), lm.squeeze().copy()
        return lm[:, 0], lm[:, 1]

    # ---------------------------------------------------------------- preprocess (functional.py:264-350)
    def preprocess(self, n_ev=(50, 50), n_descr=100, descr_type='WKS', landmarks=None, subsample_step=1, k_process=None,
                   verbose=False, descr1=None, descr2=None, signature_route="host", robust_backend=None):
        """signature_route (not in the reference): where descr_type 'HKS' / 'WKS' is evaluated.  "host" (default): the NumPy mirror
        of the reference, pyFM/signatures.py; "device": MatchEngine.signatures, the [plain | landmark] blocks of both meshes in one
        call, downloaded as NumPy float64 (equal to the host's up to the summation order and the device's exp).
        robust_backend (not in the reference): 'wheel' | 'restated' for the Laplacians of this call (TriMesh.process), None: the
        process default; meshes that bring their own `process` receive it only when the call names one."""
        if signature_route not in ("host", "device"):
            raise ValueError(f'signature_route must be "host" or "device", not {signature_route!r}')
        self.k1, self.k2 = n_ev
        if k_process is None:
            k_process = 1
        use_lm = landmarks is not None and len(landmarks) > 0
        # (functional.py:300-301: mesh1.process, mesh2.process; here the two eigensolves share one batched call)
        ks = [max(self.k1, k_process), max(self.k2, k_process)]
        if all(hasattr(m, "_assemble_laplacian") for m in (self.mesh1, self.mesh2)):
            type(self.mesh1).process_many([self.mesh1, self.mesh2], ks, robust=True, verbose=verbose, robust_backend=robust_backend)
        else:                                                                    # (duck-typed meshes bring their own process)
            own = {} if robust_backend is None else {"robust_backend": robust_backend}
            self.mesh1.process(ks[0], verbose=verbose, robust=True, intrinsic=False, **own)
            self.mesh2.process(ks[1], verbose=verbose, robust=True, intrinsic=False, **own)
        if use_lm:
            lmks1, lmks2 = self._get_lmks(landmarks)
        if descr1 is not None and descr2 is not None:
            self.descr1, self.descr2 = descr1, descr2
        elif descr_type in ('HKS', 'WKS') and signature_route == "device":
            self.descr1, self.descr2 = self._signatures_device(descr_type, n_descr, (lmks1, lmks2) if use_lm else None)
        elif descr_type in ('HKS', 'WKS'):                                       # functional.py:308-329
            sig = sg.mesh_HKS if descr_type == 'HKS' else sg.mesh_WKS
            self.descr1 = sig(self.mesh1, n_descr, k=self.k1)                    # (N1, n_descr)
            self.descr2 = sig(self.mesh2, n_descr, k=self.k2)
            if use_lm:
                self.descr1 = np.hstack([self.descr1, sig(self.mesh1, n_descr, landmarks=lmks1, k=self.k1)])
                self.descr2 = np.hstack([self.descr2, sig(self.mesh2, n_descr, landmarks=lmks2, k=self.k2)])
        else:
            raise ValueError(f'Descriptor type "{descr_type}" not implemented')
        if subsample_step != 1:                                                  # (step 1 selects every column: the arrays as they are)
            self.descr1 = self.descr1[:, np.arange(0, self.descr1.shape[1], subsample_step)]      # functional.py:333-334
            self.descr2 = self.descr2[:, np.arange(0, self.descr2.shape[1], subsample_step)]
        return self                                                                          # no normalisation (:336-344)

    def _signatures_device(self, descr_type, n_descr, lmks):
        """[plain | landmark blocks] of both meshes (functional.py:308-329) from one device call when the two use the same number of
        eigenpairs (the smaller mesh padded with rows that are not read), else one call per mesh"""
        from ..engine import default_engine
        eng = default_engine()
        sides = []
        for mesh, kk in ((self.mesh1, self.k1), (self.mesh2, self.k2)):
            assert mesh.eigenvalues is not None, "Eigenvalues should be processed"
            kk = min(kk, len(mesh.eigenvalues))
            sides.append((np.asarray(mesh.eigenvectors)[:, :kk], np.asarray(mesh.eigenvalues, dtype=np.float64)[:kk]))
        lm = None if lmks is None else [np.asarray(l).reshape(-1) for l in lmks]
        if sides[0][0].shape[1] == sides[1][0].shape[1] and sides[0][0].dtype == sides[1][0].dtype:
            n = [s_[0].shape[0] for s_ in sides]
            Phi = np.zeros((2, max(n), sides[0][0].shape[1]), dtype=sides[0][0].dtype)
            for q in range(2):
                Phi[q, :n[q]] = sides[q][0]
            S = eng.signatures(Phi, np.stack([s_[1] for s_ in sides]), descr_type, n_descr, landmarks=None if lm is None else np.stack(lm),
                               plain=True, n_verts=n).cpu().numpy()
            return S[0, :n[0]], S[1, :n[1]]
        return tuple(eng.signatures(sides[q][0][None], sides[q][1][None], descr_type, n_descr, landmarks=None if lm is None else lm[q][None],
                                    plain=True)[0].cpu().numpy() for q in range(2))

    # ---------------------------------------------------------------- fit (functional.py:352-487)
    def fit(self, w_descr=1e-1, w_lap=1e-3, w_dcomm=1, w_orient=0, w_area=0, w_conformal=0, w_p2p=0, w_stochastic=0, w_ent=0,
            w_range01=0, w_sumto1=0, w_area_difference=0, w_mumford_shah=0, mumford_shah_var=0.1, w_eta_entropy=0,
            orient_reversing=False, optinit='zeros', verbose=False, maxiter=1000000, device=None, stopping="reference", driver="device",
            orient_route="host"):
        """reference functional.py:352-487.  With only w_descr / w_lap > 0 the minimiser (what the reference's L-BFGS-B
        converges to, first column pinned) is obtained in closed form on the GPU for maps up to
        CLOSED_FORM_MAX_K1 columns; wider maps run L-BFGS on the two terms to LBFGS_WIDE, whatever `stopping` says.  With any of
        w_dcomm, w_orient, w_area, w_conformal, w_p2p, w_stochastic, w_ent, w_range01, w_sumto1 > 0 the reference's own scheme
        runs: limited-memory BFGS with L-BFGS-B's line search and stopping tests (scipy.optimize.minimize, :477) from
        get_x0(optinit), on the device, energy and gradient in float64 (maps up to 32 x 32 with the notebook's kind of terms:
        dm_fmap_fit_fused, one launch per evaluation; everything else: dm_fmap_fit_steps -> dm_fmap_energy_grad + dm_lbfgs_advance).
        Only the area-difference, Mumford-Shah and eta-entropy terms are not on the path (NotImplementedError).
        stopping = "reference" (default): SciPy's default rule, i.e. what the reference's call runs with (ftol 2.2e-9, gtol 1e-5):
        the fit ends where the reference's ends, a few 1e-4 short of the minimiser, and the drop-in agrees best with the
        reference's own outputs (INTEGRATION.md has the per-slot table); "tight": ftol 1e-12, the float64 minimiser to 1e-5.  The
        rule holds at every width of the map (fit_plan).  The parameters are checked by fit_parameters, the fit itself is
        fit_models -- both shared with compute_surface_map_batch.
        orient_route (not in the reference; read when w_orient > 0): "host" (default) builds the orientation operators with
        compute_orientation_op's sparse products per descriptor, as the reference does; "device" builds both operator sets
        (rescaling and optimisation) with MatchEngine.orientation_ops and keeps them on the device until the fit has read them.
        The device route reads the descriptors the fit itself reads (fp16 / fp32): for float64 descriptors that are not fp32
        numbers its operators differ from the host route's at 1e-7 relative."""
        p = fit_parameters(dict(
            w_descr=w_descr, w_lap=w_lap, w_dcomm=w_dcomm, w_orient=w_orient, w_area=w_area, w_conformal=w_conformal, w_p2p=w_p2p,
            w_stochastic=w_stochastic, w_ent=w_ent, w_range01=w_range01, w_sumto1=w_sumto1, w_area_difference=w_area_difference,
            w_mumford_shah=w_mumford_shah, mumford_shah_var=mumford_shah_var, w_eta_entropy=w_eta_entropy, orient_reversing=orient_reversing,
            optinit=optinit, verbose=verbose, maxiter=maxiter, device=device, stopping=stopping, driver=driver, orient_route=orient_route))
        from ..engine import default_engine
        from .spectral.convert import _real_dtype
        import torch
        if self.optimizer not in _OPTIMIZERS:
            raise ValueError(f"Unknown solver {self.optimizer}")
        if self.partial:
            raise NotImplementedError()                                        # functional.py:480
        if not self.preprocessed:
            self.preprocess()
        eng = default_engine()
        m1, m2 = self.mesh1, self.mesh2
        # like the reference (functional.py:412-413) fit uses every stored eigenvector column
        d1, d2 = np.asarray(self.descr1), np.asarray(self.descr2)
        fdt = np.float16 if (d1.dtype == np.float16 and d2.dtype == np.float16) else np.float32
        one = lambda x, dt: np.ascontiguousarray(x, dtype=dt)[None]
        a1, a2 = m1.A.diagonal(), m2.A.diagonal()
        batch = {"Phi1": one(m1.eigenvectors, np.float32), "Phi2": one(m2.eigenvectors, np.float32), "a1": one(a1, np.float32), "a2": one(a2, np.float32),
                 "lam1": one(m1.eigenvalues, np.float64), "lam2": one(m2.eigenvalues, np.float64), "F1": one(d1, fdt), "F2": one(d2, fdt)}
        tdt = {np.float16: torch.float16, np.float32: torch.float32, np.float64: torch.float64}
        dev = {n: eng._dev(v, tdt[v.dtype.type], n) for n, v in batch.items()}
        rdt = _real_dtype(m1.eigenvectors, m2.eigenvectors)
        own = (one(m1.eigenvectors, rdt), one(m2.eigenvectors, rdt), one(a1, None), one(a2, None))
        _, res = fit_models(eng, [self], p, dev, own, report=self._verbose_terms)
        if verbose and res is not None:
            print(f"\tTask funcall : {res.nfev}, nit : {res.nit}, warnflag : {res.message}")
        self._dev = dev

    # the reference's per-term printout (base_functions.py:27-29, 538-636: `VERBOSE` in the environment prints every live term's
    # weighted loss at every energy evaluation).  The optimiser runs on the device here, so the same lines are printed where the
    # host sees the map: at the start point and at the solution.
    _VERBOSE_LABELS = (("w_descr", "descr loss:"), ("w_lap", "lap loss:"), ("w_dcomm", "descr comm loss:"), ("w_orient", "orient loss:"),
                       ("w_area", "area loss:"), ("w_conformal", "conformal loss:"), ("w_p2p", "p2p loss:"),
                       ("w_stochastic", "stochastic loss:"), ("w_ent", "entropy loss:"), ("w_range01", "range01 loss:"),
                       ("w_sumto1", "sumto1 loss:"))

    def _verbose_terms(self, eng, dev, weights, x, orient_ops, where):
        """x (1, k2, k1); weights as fit_general takes them (w_orient: one weight per pair)"""
        import os
        if not os.environ.get("VERBOSE", False):
            return
        print(f"energy terms at the {where}:")
        for name, label in self._VERBOSE_LABELS:
            w = weights.get(name, 0)
            if np.any(np.asarray(w) > 0):
                e = eng.fit_energy(dev, {name: w}, x, orient_ops=orient_ops if name == "w_orient" else None)
                print(label, float(e[0]))

    def compute_orientation_op(self, reversing=False, normalize=False, area="vertex", route="host"):
        """functional.py:686-728: per descriptor the pair (pinv1 O1 Phi1, +-pinv2 O2 Phi2) of orientation operators in the reduced
        bases, O = TriMesh.orientation_op(gradient of the descriptor).  area = "vertex": rows divided by the mesh's vertex_areas (the
        reference's method); "mass": by diag(A) (what energy_func_std builds, base_functions.py:573).
        route (not in the reference) = "host" (default): sparse products per descriptor, as in the reference; "device": all descriptors
        of a mesh in one float64 matrix-core product (MatchEngine.orientation_ops), the same list downloaded.  The device route reads
        the descriptors as the fit stages them (fp16 when both sets are fp16, else fp32): float64 descriptors that are not fp32 numbers
        give operators that differ from the host route's at 1e-7 relative.  normalize=True is host-only."""
        if route not in ("host", "device"):
            raise ValueError(f'route must be "host" or "device", not {route!r}')
        if route == "device":
            if normalize:
                raise NotImplementedError('compute_orientation_op(normalize=True) is not on the device route; use route="host"')
            from ..engine import default_engine
            from .spectral.convert import _real_dtype
            d1, d2 = np.asarray(self.descr1), np.asarray(self.descr2)
            fdt = np.float16 if (d1.dtype == np.float16 and d2.dtype == np.float16) else np.float32      # (the dtype fit() stages)
            rdt = _real_dtype(self.mesh1.eigenvectors, self.mesh2.eigenvectors)
            one = lambda x, dt: np.ascontiguousarray(x, dtype=dt)[None]
            ops, _ = _orientation_ops_device(default_engine(), [self], (one(self.mesh1.eigenvectors, rdt), one(self.mesh2.eigenvectors, rdt)),
                                             (one(d1, fdt), one(d2, fdt)), area)
            o1, o2 = (o[0].cpu().numpy() for o in ops)
            return [(a, -b if reversing else b) for a, b in zip(o1, o2)]
        out = []
        sides = []
        for mesh, descr, k in ((self.mesh1, self.descr1, self.k1), (self.mesh2, self.descr2, self.k2)):
            ev = np.asarray(mesh.eigenvectors[:, :k], dtype=np.float64)
            pinv = ev.T @ mesh.A
            pva = None if area == "vertex" else np.asarray(mesh.A.diagonal())
            d = np.asarray(descr, dtype=np.float64)
            sides.append([np.asarray(pinv @ (mesh.orientation_op(mesh.gradient(d[:, i], normalize=normalize), per_vert_area=pva) @ ev))
                          for i in range(d.shape[1])])
        for a, b in zip(*sides):
            out.append((a, -b if reversing else b))
        return out

    def get_x0(self, optinit="zeros"):
        """functional.py:629-660"""
        if optinit == 'random':
            x0 = np.random.random((self.k2, self.k1))
            x0 = x0 / x0.sum()
        elif optinit == 'identity':
            x0 = np.eye(self.k2, self.k1)
        else:
            x0 = np.zeros((self.k2, self.k1))
        ev_sign = np.sign(self.mesh1.eigenvectors[0, 0] * self.mesh2.eigenvectors[0, 0])
        area_ratio = np.sqrt(self.mesh2.area / self.mesh1.area)
        x0[:, 0] = np.zeros(self.k2)
        x0[0, 0] = ev_sign * area_ratio
        return x0

    # ---------------------------------------------------------------- maps and refinement
    def get_p2p(self, use_adj=False, n_jobs=1):
        """functional.py:201-219: returns the kd-tree maps (p2p_21, p2p_12) and sets self.mapped_indicator"""
        p2p_21, p2p_12, self.mapped_indicator = spectral.mesh_FM_to_p2p(self.FM, self.mesh1, self.mesh2, use_adj=use_adj,
                                                                       n_jobs=n_jobs)
        return p2p_21, p2p_12

    def get_precise_map(self, precompute_dmin=True, use_adj=True, batch_size=None, n_jobs=1, verbose=False):
        """functional.py:221-251: (n2, n1) sparse precise map from mesh2 to mesh1"""
        if not self.fitted:
            raise ValueError('Model should be fit and fit to obtain p2p map')
        return spectral.mesh_FM_to_p2p_precise(self.FM, self.mesh1, self.mesh2, precompute_dmin=precompute_dmin, use_adj=use_adj,
                                               batch_size=batch_size, n_jobs=n_jobs, verbose=verbose)

    def _precise_map_device(self):
        """get_precise_map().toarray() kept on the GPU (compute_surface_map feeds it to the assignment kernel)"""
        from ..engine import default_engine
        k2, k1 = self.FM.shape
        from .spectral.convert import _basis, _real_dtype
        dt = _real_dtype(self.mesh1.eigenvectors, self.mesh2.eigenvectors)
        return default_engine().precise_map(_basis(self.mesh1.eigenvectors, k1, dt), _basis(self.mesh2.eigenvectors, k2, dt),
                                            np.asarray(self.FM, dtype=np.float64)[None],
                                            np.ascontiguousarray(self.mesh1.facelist, dtype=np.int32)[None], dense=True)[2][0]

    def icp_refine(self, nit=10, tol=None, use_adj=False, overwrite=True, verbose=False, n_jobs=1):
        """functional.py:564-586"""
        if not self.fitted:
            raise ValueError("The Functional map must be fit before refining it")
        self._FM_icp = refine.mesh_icp_refine(self.FM, self.mesh1, self.mesh2, nit=nit, tol=tol, return_p2p=False,
                                              use_adj=use_adj, n_jobs=n_jobs, verbose=verbose)
        if overwrite:
            self.FM_type = 'icp'

    def zoomout_refine(self, nit=10, step=1, subsample=None, overwrite=True, verbose=False):
        """functional.py:588-617"""
        if not self.fitted:
            raise ValueError("The Functional map must be fit before refining it")
        if subsample is None or (np.issubdtype(type(subsample), np.integer) and subsample == 0):   # functional.py:607-610
            sub = None
        else:
            sub = subsample                                                     # int: farthest point sampling of that size; or (sub1, sub2)
        self._FM_zo = refine.mesh_zoomout_refine(self.FM, self.mesh1, self.mesh2, nit, step=step, subsample=sub, verbose=verbose)
        if overwrite:
            self.FM_type = 'zoomout'

    def compute_SD(self):
        """functional.py:619-627: the area and conformal shape difference operators of the fitted map, as D_a / D_c.  A NumPy map
        takes the host products (the reference's bits), a map held as a GPU tensor dm_shape_diff_f64."""
        if not self.fitted:
            raise ValueError("The Functional map must be fit before computing the shape difference")
        self.D_a = spectral.area_SD(self.FM)
        self.D_c = spectral.conformal_SD(self.FM, self.mesh1.eigenvalues, self.mesh2.eigenvalues)

    # ---------------------------------------------------------------- small helpers (functional.py:730-831)
    def project(self, func, k=None, mesh_ind=1):
        if mesh_ind == 1:
            return self.mesh1.project(func, k=self.k1 if k is None else k)
        elif mesh_ind == 2:
            return self.mesh2.project(func, k=self.k2 if k is None else k)
        raise ValueError(f'Only indices 1 or 2 are accepted, not {mesh_ind}')

    def decode(self, encoded_func, mesh_ind=2):
        if mesh_ind == 1:
            return self.mesh1.decode(encoded_func)
        elif mesh_ind == 2:
            return self.mesh2.decode(encoded_func)
        raise ValueError(f'Only indices 1 or 2 are accepted, not {mesh_ind}')

    def transport(self, encoded_func, reverse=False):
        if not self.preprocessed:
            raise ValueError("The Functional map must be fit before transporting a function")
        return np.linalg.pinv(self.FM) @ encoded_func if reverse else self.FM @ encoded_func

    def transfer(self, func, reverse=False):
        if not reverse:
            return self.decode(self.transport(self.project(func)))
        return self.decode(self.transport(self.project(func, mesh_ind=2), reverse=True), mesh_ind=1)

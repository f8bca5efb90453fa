"""CPU: the fit stage that FunctionalMapping.fit and compute_surface_map_batch share -- its plan as a table, the parameter checks through
both entries, and robust_backend= as an argument of the call instead of a process-wide setting."""
import pytest

from test_orient_route_cpu import _model


# ---- the plan: (parameters, k1) -> (route, L-BFGS options)
QUADRATIC = dict(w_descr=1e-1, w_lap=1e-3, w_dcomm=0)


@pytest.mark.parametrize("given, k1, route, options", [
    (dict(QUADRATIC), 200, "closed", None),
    (dict(QUADRATIC, stopping="reference"), 201, "iterative", "LBFGS_WIDE"),
    (dict(QUADRATIC, stopping="tight"), 201, "iterative", "LBFGS_WIDE"),
    (dict(QUADRATIC, w_ent=1e-3, stopping="reference"), 201, "iterative", None),
    (dict(QUADRATIC, w_ent=1e-3, stopping="tight"), 201, "iterative", "LBFGS_OPTIONS"),
])
def test_fit_plan(given, k1, route, options):
    from densematcher_amd.pyFM import functional
    assert functional.CLOSED_FORM_MAX_K1 == 200
    want = None if options is None else getattr(functional, options)
    got_route, got_options = functional.fit_plan(functional.fit_parameters(given), k1)
    assert got_route == route and got_options == want


# ---- the same invalid input: the same exception type through both entries, before a device is needed
ALL_ZERO = dict(w_descr=0, w_lap=0, w_dcomm=0, w_orient=0, w_area=0, w_conformal=0, w_p2p=0, w_stochastic=0, w_ent=0, w_range01=0, w_sumto1=0)


@pytest.mark.parametrize("bad, error", [
    (dict(w_nonsense=1), TypeError),
    (dict(w_mumford_shah=1), NotImplementedError),
    (dict(optinit="x"), ValueError),
    (dict(stopping="x"), ValueError),
    (dict(orient_route="x"), ValueError),
    (ALL_ZERO, ValueError),
])
def test_invalid_fit_parameters_through_both_entries(fx_cfg1, bad, error, monkeypatch):
    from densematcher_amd import engine
    from densematcher_amd.functional_map import compute_surface_map_batch

    def no_device(*a, **kw):
        raise AssertionError("the parameters are checked before the device is asked for")
    monkeypatch.setattr(engine, "default_engine", no_device)
    with pytest.raises(error):
        _model(fx_cfg1).fit(**bad)
    with pytest.raises(error):
        compute_surface_map_batch([], [], [], [], fit_params=bad)


# ---- robust_backend does not travel through the process-wide setting
class _Sentinel(Exception):
    pass


class _Duck:
    def __init__(self, verts, faces):
        self.v, self.f = verts, faces

    def verts_list(self):
        return [self.v]

    def faces_list(self):
        return [self.f]


def _wheel_missing():
    try:
        import robust_laplacian  # noqa: F401
    except ImportError:
        return True
    return False


class _NestedCallEngine:
    """what default_engine returns in these tests.  TriMesh._assemble_many asks it for the tufted covers only AFTER it has decided which
    backend the call runs (the wheel is missing: ImportError unless that is "restated"), so reaching tufted_covers proves that the outer
    call's robust_backend="restated" arrived there.  The first tufted_covers, from inside the outer call, makes a call of its own on a
    second pair that names no backend, records what that call raised, and raises the sentinel."""
    def __init__(self, fx, seen):
        self.fx, self.seen = fx, seen

    def tufted_covers(self, meshes, **kw):
        from densematcher_amd.functional_map import compute_surface_map
        from densematcher_amd.pyFM.mesh import laplacian
        fx, seen = self.fx, self.seen
        assert "nested" not in seen, "the nested call must not get as far as the covers"
        seen["default_inside"] = laplacian.robust_backend()
        try:
            compute_surface_map(_Duck(fx["verts2"], fx["faces2"]), _Duck(fx["verts1"], fx["faces1"]), fx["F2"][:, :4], fx["F1"][:, :4], n_ev=10)
            seen["nested"] = None
        except BaseException as e:
            seen["nested"] = e
        raise _Sentinel()


def _no_device_streams(monkeypatch):
    """compute_surface_map_batch asks torch for the device and its streams before it processes the meshes: stand-ins, so that the call
    gets as far as the Laplacians on a machine without a GPU (with spectral signatures it stages no descriptors: no upload either)"""
    import types
    import torch
    from densematcher_amd import functional_map
    stream = types.SimpleNamespace(cuda_stream=0, device=types.SimpleNamespace(index=0))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **kw: stream)
    monkeypatch.setattr(functional_map, "_side_streams", lambda dev_index, n, caller=None: [stream] * n)
    monkeypatch.setattr(functional_map, "_upload_stream", lambda main_stream: stream)


@pytest.mark.parametrize("entry", ["compute_surface_map", "compute_surface_map_batch", "TriMesh.process"])
def test_robust_backend_is_an_argument_of_the_call(fx_cfg1, entry, monkeypatch):
    if not _wheel_missing():
        pytest.skip("the robust_laplacian wheel is installed: no backend is chosen")
    from densematcher_amd import engine, functional_map
    from densematcher_amd.pyFM.mesh import TriMesh, laplacian
    fx = fx_cfg1
    seen = {}
    fake = _NestedCallEngine(fx, seen)
    monkeypatch.setattr(engine, "default_engine", lambda *a, **kw: fake)
    m1, m2 = _Duck(fx["verts1"], fx["faces1"]), _Duck(fx["verts2"], fx["faces2"])
    old = laplacian.robust_backend()
    laplacian.set_robust_backend("wheel")
    try:
        # (a call that lost the argument on its way down ends in ImportError here, not in the sentinel)
        with pytest.raises(_Sentinel), pytest.warns(UserWarning, match="robust_laplacian"):
            if entry == "compute_surface_map":
                functional_map.compute_surface_map(m1, m2, fx["F1"][:, :4], fx["F2"][:, :4], n_ev=10, robust_backend="restated")
            elif entry == "compute_surface_map_batch":
                _no_device_streams(monkeypatch)
                functional_map.compute_surface_map_batch([m1], [m2], None, None, n_ev=10, descr_type="HKS", robust_backend="restated")
            else:
                TriMesh(fx["verts1"], fx["faces1"]).process(10, robust=True, robust_backend="restated")
        assert isinstance(seen["nested"], ImportError), seen["nested"]        # the nested call ran on the process default
        assert seen["default_inside"] == "wheel" and laplacian.robust_backend() == "wheel"
        for call in (lambda: TriMesh(fx["verts1"], fx["faces1"]).process(10, robust=True, robust_backend="x"),
                     lambda: functional_map.compute_surface_map(m1, m2, fx["F1"], fx["F2"], robust_backend="x"),
                     lambda: functional_map.compute_surface_map_batch([], [], [], [], robust_backend="x")):
            with pytest.raises(ValueError, match="robust backend"):
                call()
    finally:
        laplacian.set_robust_backend(old)


def test_fit_signature_is_the_parameter_table():
    """FunctionalMapping.fit keeps the reference's explicit signature; the shared table must list the same names with the same defaults"""
    import inspect
    from densematcher_amd.pyFM.functional import FIT_DEFAULTS, FunctionalMapping
    sig = {n: q.default for n, q in inspect.signature(FunctionalMapping.fit).parameters.items() if n != "self"}
    assert sig == FIT_DEFAULTS

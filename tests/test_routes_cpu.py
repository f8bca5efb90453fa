"""CPU: the one route picker (densematcher_amd/_routes.py) and _operands.image_frame.  Every row of the decision table at the seam, with
and without a GPU: "a GPU is present" is _routes.engine_or_none returning a sentinel object, so nothing touches a device.  The
auto -> device rows of the torch vocabulary need CUDA tensors and stay with the GPU suites (last_route == "device")."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from densematcher_amd import _routes
from densematcher_amd._operands import image_frame

ENGINE = object()
NO_GPU = "route='device' needs a ROCm GPU \\(gfx950\\)"


@pytest.fixture(params=[False, True], ids=["no-gpu", "gpu"])
def gpu(request, monkeypatch):
    monkeypatch.setattr(_routes, "engine_or_none", lambda: ENGINE if request.param else None)
    return request.param


def _never():
    raise AssertionError("not asked on this row")


# ---- names
def test_invalid_names(gpu):
    host, torch_ = "route must be 'auto', 'host' or 'device', not 'torch'", "route must be 'auto', 'torch' or 'device', not 'host'"
    for call, text in ((lambda: _routes.check("torch", _routes.HOST), host), (lambda: _routes.pick_host("torch"), host),
                       (lambda: _routes.check("host", _routes.TORCH), torch_), (lambda: _routes.pick_torch("host", "X", _never, True, _never), torch_)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    for name in _routes.HOST:
        _routes.check(name, _routes.HOST)
    for name in _routes.TORCH:
        _routes.check(name, _routes.TORCH)
    assert [_routes.torch_route(r) for r in ("auto", "host", "device", "torch")] == ["auto", "torch", "device", "torch"]


# ---- the host vocabulary
@pytest.mark.parametrize("auto", [True, False])
def test_pick_host(gpu, auto):
    assert _routes.pick_host("host", auto) == "host"
    assert _routes.pick_host("auto", auto) == ("device" if gpu and auto else "auto")     # left "auto": lifting's third outcome
    if gpu:
        assert _routes.pick_host("device", auto) == "device"
    else:
        with pytest.raises(RuntimeError, match=NO_GPU):
            _routes.pick_host("device", auto)
    assert _routes.pick_host("auto") == ("device" if gpu else "auto")                    # no table: whenever a GPU is present


def test_host_asks_for_no_engine(monkeypatch):
    monkeypatch.setattr(_routes, "engine_or_none", _never)
    assert _routes.pick_host("host") == "host" and _routes.pick_host("auto", False) == "auto"
    assert _routes.pick_torch("torch", "X", _never, True, _never) == "torch"
    assert _routes.pick_torch("auto", "X", lambda: None, False, _never) == "torch"
    assert _routes.pick_torch("auto", "X", lambda: "why", True, _never) == "torch"
    assert _routes.pick_torch("auto", "X", lambda: None, True, lambda: False) == "torch"
    assert _routes.pick_torch("device", "X", lambda: None, True) == "device"               # on_gpu=None: the obstacle covers the GPU
    assert _routes.pick_torch("auto", "X", lambda: None, True) == "device"


# ---- the torch vocabulary
@pytest.mark.parametrize("why", [None, "it is Tuesday"])
@pytest.mark.parametrize("on_gpu", [True, False])
@pytest.mark.parametrize("auto", [True, False])
def test_pick_torch(gpu, why, on_gpu, auto):
    pick = lambda route, **kw: _routes.pick_torch(route, "Thing", lambda: why, auto, lambda: on_gpu, **kw)
    assert pick("torch") == "torch"
    assert pick("auto") == ("device" if why is None and on_gpu and auto and gpu else "torch")
    if why is not None:                                  # the refusal comes first: also on a machine without a GPU
        for kind in (ValueError, RuntimeError):
            with pytest.raises(kind) as e:
                pick("device", refusal=kind)
            assert type(e.value) is kind and str(e.value) == "Thing route='device': it is Tuesday"
    elif not gpu:
        with pytest.raises(RuntimeError, match=NO_GPU):
            pick("device")
    else:
        assert pick("device") == "device"                # placement and the table are not asked: the engine checks its operands


def test_grad_obstacle():
    a, b = torch.zeros(2), torch.zeros(2, requires_grad=True)
    assert _routes.grad_obstacle([a]) is None and _routes.grad_obstacle([]) is None
    assert _routes.grad_obstacle([a, b]) == "a tensor requires grad (the device route records no autograd graph: call under torch.no_grad())"
    with torch.no_grad():
        assert _routes.grad_obstacle([a, b]) is None


# ---- the call sites whose refusals differ: ValueError before RuntimeError (JBU, AggreNet), RuntimeError (DiffusionNet)
def test_jbu_refuses_before_it_looks_for_a_gpu(gpu):
    from densematcher_amd.featup.upsamplers import JBULearnedRange, JBUStack
    up, stack = JBULearnedRange(3, 4, 32), JBUStack(4)
    src, img = torch.zeros(1, 4, 4, 4), torch.zeros(1, 3, 8, 8)
    with torch.no_grad():
        for module, name in ((up, "JBULearnedRange"), (stack, "JBUStack")):
            module.train()
            with pytest.raises(ValueError, match=f"^{name} route='device': the module is in training mode"):
                module(src, img, route="device")
            module.eval()
            if not gpu:
                with pytest.raises(RuntimeError, match=NO_GPU):
                    module(src, img, route="device")
        with pytest.raises(ValueError, match="^JBULearnedRange route='device': the guidance \\(7, 8\\) is not exactly twice"):
            up(src, img[:, :, :7], route="device")                    # the shape obstacle comes before the others
        assert up(src, img, route="auto").shape == (1, 4, 8, 8)       # operands on the CPU: torch, with or without a GPU
    with pytest.raises(ValueError, match="^JBUStack route='device': a tensor requires grad"):
        stack(src, img, route="device")


def test_aggre_refuses_before_it_looks_for_a_gpu(gpu):
    from densematcher_amd.featurizers.modules import projection_network as pn
    net = pn.AggregationNetwork(feature_dims=[8, 6], projection_dim=8, num_norm_groups=2)
    x = torch.zeros(1, 14, 2, 2)
    with torch.no_grad():
        with pytest.raises(ValueError, match="^AggregationNetwork route='device': the module is in training mode"):
            pn.route_of(net, "device", (x,))
        net.eval()
        if not gpu:
            with pytest.raises(RuntimeError, match=NO_GPU):
                pn.route_of(net, "device", (x,))
        else:
            assert pn.route_of(net, "device", (x,)) == "device"
        assert pn.route_of(net, "auto", (x,)) == "torch" and pn.route_of(net, "torch", (x,)) == "torch"
    with pytest.raises(ValueError, match="^AggregationNetwork route='device': a tensor requires grad"):
        pn.route_of(net, "device", (x,))


def test_dnet_refuses_with_runtime_error(gpu):
    from densematcher_amd.diffusion_net import layers
    net = layers.DiffusionNet(C_in=3, C_out=2, C_width=4, N_block=1, dropout=False).eval()
    x = torch.zeros(5, 3)                                             # on the CPU: an obstacle wherever this runs
    with torch.no_grad(), pytest.raises(RuntimeError, match="^DiffusionNet route='device': ") as e:
        net(x, route="device")
    assert type(e.value) is RuntimeError and str(e.value) == "DiffusionNet route='device': " + net._device_obstacle([x])
    with pytest.raises(ValueError, match="route must be 'auto', 'torch' or 'device', not 'host'"):
        net(x, route="host")
    mass, evals, evecs = torch.ones(5), torch.zeros(2), torch.zeros(5, 2)
    sp = torch.zeros(5, 5).to_sparse()
    with torch.no_grad():
        net(x, mass, None, evals, evecs, sp, sp, route="auto")
    assert net.last_route == "torch"


# ---- lifting keeps three outcomes
def test_lifting_auto_without_the_table_is_the_torch_lift(monkeypatch):
    """a GPU is present and the table says no: "auto" is neither the device route (the sentinel has no lift_features) nor "host" by
    name -- it runs the torch lift where the maps lie"""
    from densematcher_amd import projection as pj
    monkeypatch.setattr(_routes, "engine_or_none", lambda: ENGINE)
    monkeypatch.setattr(pj, "AUTO_DEVICE", {"nchw": False, "channels_last": False})
    verts = np.array([[0.5, 0.5, 0.5], [0.5, -0.5, -0.5], [-0.5, 0.5, -0.5], [-0.5, -0.5, 0.5]])
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    turn = lambda a: np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    cams = (np.stack([turn(a) for a in (0.0, 2.0, 4.0)]), np.tile([0.0, 0.0, 3.0], (3, 1)))
    fts = torch.arange(3 * 4 * 8 * 8, dtype=torch.float32).reshape(3, 4, 8, 8)
    seen = []
    real = pj._torch_lift
    monkeypatch.setattr(pj, "_torch_lift", lambda *a: seen.append(a[-1]) or real(*a))
    auto = pj.lift_features_many([fts], [(verts, faces)], [cams], route="auto")[0]
    host = pj.lift_features_many([fts], [(verts, faces)], [cams], route="host")[0]
    assert seen == [fts.device, torch.device("cpu")]
    assert auto.shape == (4, 4) and auto.device == fts.device and auto.abs().sum() > 0 and torch.equal(auto, host)
    with pytest.raises(AttributeError, match="lift_features"):                       # with the table, "auto" is the device route
        monkeypatch.setattr(pj, "AUTO_DEVICE", {"nchw": True, "channels_last": True})
        pj.lift_features_many([fts], [(verts, faces)], [cams], route="auto")


# ---- the engine lookups
def test_engine_or_none_reads_default_engine_at_call_time(monkeypatch):
    from densematcher_amd import engine
    monkeypatch.setattr(engine, "default_engine", lambda *a, **kw: ENGINE)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert _routes.engine_or_none() is ENGINE
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert _routes.engine_or_none() is None


def test_importing_routes_imports_neither_the_engine_nor_torch():
    code = "import sys; import densematcher_amd._routes; assert 'densematcher_amd.engine' not in sys.modules and 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], cwd=REPO, check=True)


def test_engine_for(gpu, monkeypatch):
    from densematcher_amd import engine

    def no_device(*a, **kw):
        raise RuntimeError("densematcher_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
    monkeypatch.setattr(engine, "default_engine", (lambda *a, **kw: ENGINE) if gpu else no_device)
    assert _routes.engine_for(None, True) is (ENGINE if gpu else None)
    assert _routes.engine_for(None, False) is None
    for default in (True, False):
        assert _routes.engine_for(False, default) is None and _routes.engine_for(0, default) is None
        if gpu:
            assert _routes.engine_for(True, default) is ENGINE
        else:
            with pytest.raises(RuntimeError, match="there is no CPU fallback"):      # what default_engine() raises: no silent fall-back
                _routes.engine_for(True, default)


def test_engine_for_raises_what_default_engine_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from densematcher_amd import engine, utils
    with pytest.raises(RuntimeError) as theirs:
        engine.default_engine()
    with pytest.raises(RuntimeError) as mine:
        _routes.engine_for(True, True)
    assert str(mine.value) == str(theirs.value)
    D = np.array([[0.0, 1.0], [1.0, 0.0]])
    assert utils.get_distance_between_groups(D, [0], [1]) == 1.0                     # device=None without a GPU: the host route
    with pytest.raises(RuntimeError):
        utils.get_distance_between_groups(D, [0], [1], device=True)


# ---- image_frame
def test_image_frame():
    assert image_frame(8, 8, 1.0, "w") == (8, 8) and image_frame(8, 8, None, "w") == (8, 8)
    got = image_frame(torch.zeros(1, 1, 6, 6).shape[2], np.int64(6), 2, "w")
    assert got == (6, 6) and all(type(v) is int for v in got)
    with pytest.raises(ValueError) as e:
        image_frame(8, 9, float("nan"), "w")                                          # square first
    assert str(e.value) == "w: square images only (H = 8, W = 9)"
    with pytest.raises(ValueError) as e:
        image_frame(0, 0, -1.0, "w")                                                  # then positive
    assert str(e.value) == "w: H and W must be positive"
    for f in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError) as e:
            image_frame(8, 8, f, "w")                                                 # then the focal length
        assert str(e.value) == "w: the focal length must be positive and finite"
    assert image_frame(8, 8, None, "w") == (8, 8)                                     # a caller without a focal length checks none

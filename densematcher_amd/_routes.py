"""
Which route a call takes, once ('Routes').  Two vocabularies: HOST ('auto' | 'host' | 'device') where the other route is
NumPy / SciPy or torch on the CPU, TORCH ('auto' | 'torch' | 'device') where it is the reference's expressions on PyTorch, on any
device and with autograd.  'device' is the HIP path or an error, never a fall-back; 'auto' takes it where it can run and the
measurement recorded in the calling module (its AUTO_DEVICE / DEVICE_DEFAULT, read by the caller at call time) found it not slower.
Plain functions, no state.  torch and the engine are imported when a function needs them: pyFM's host routes import neither.
"""
HOST = ("auto", "host", "device")
TORCH = ("auto", "torch", "device")

NO_GPU = "route='device' needs a ROCm GPU (gfx950)"


def engine_or_none():
    """the default engine, or None in a process without a GPU"""
    import torch
    if not torch.cuda.is_available():
        return None
    from .engine import default_engine
    return default_engine()


def engine_for(device, default):
    """device=None | True | False of utils and pyFM.FMN: None takes the engine when `default` holds and a GPU is present, a truthy
    value takes it or fails as default_engine() does without a GPU, a falsy one gives None (the host route)"""
    if device is None:
        return engine_or_none() if default else None
    if not device:
        return None
    from .engine import default_engine
    return default_engine()


def check(route, names):
    if route not in names:
        raise ValueError(f"route must be 'auto', '{names[1]}' or 'device', not {route!r}")


def torch_route(route):
    """a HOST route as the TORCH callees of the same call take it"""
    return "torch" if route == "host" else route


def grad_obstacle(tensors):
    """why the device route cannot take these tensors as far as autograd goes, or None"""
    import torch
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return "a tensor requires grad (the device route records no autograd graph: call under torch.no_grad())"
    return None


def pick_host(route, auto=True):
    """HOST vocabulary: 'device', or `route` as it came.  'device' without a GPU is a RuntimeError; 'auto' takes the device when `auto`
    (the caller's measurement) holds and a GPU is present, and otherwise stays 'auto': a caller for which that differs from 'host'
    (lifting runs torch on the maps' own device) sees which it was."""
    check(route, HOST)
    if route == "device" and engine_or_none() is None:
        raise RuntimeError(NO_GPU)
    return "device" if route == "device" or (route == "auto" and auto and engine_or_none() is not None) else route


def pick_torch(route, who, obstacle, auto, on_gpu=None, refusal=ValueError):
    """TORCH vocabulary: 'torch' or 'device'.  obstacle() gives why the device route cannot run this call, or None; it is not asked
    when route is 'torch'.  'device' with an obstacle raises refusal(f"{who} route='device': {why}"), and only then RuntimeError
    without a GPU.  'auto' takes the device when there is no obstacle, `auto` (the caller's measurement) holds, on_gpu() says the
    operands are on the GPU and an engine exists.  on_gpu=None: the obstacle covers the GPU and the placement itself, no engine is
    asked for."""
    check(route, TORCH)
    if route == "torch":
        return "torch"
    why = obstacle()
    if route == "device":
        if why is not None:
            raise refusal(f"{who} route='device': {why}")
        if on_gpu is not None and engine_or_none() is None:
            raise RuntimeError(NO_GPU)
        return "device"
    return "device" if why is None and auto and (on_gpu is None or (on_gpu() and engine_or_none() is not None)) else "torch"

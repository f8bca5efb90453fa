"""CPU: the backward of the JBU apply.  The float64 restatement of the adjoint (tests/jbu_bwd_checks.py: explicit axis matrices, so the
border folds are pinned independently of torch's own backward) against float64 autograd on every shape of the GPU tests, and the new
surface as far as it exists without a GPU: the differentiable= flag of JBULearnedRange / JBUStack / upsample_features, which the torch
and auto routes ignore and the device route answers as it does today, and the two entry points in the header, in _lib.SIGNATURES and
in the built library."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import jbu_bwd_checks as bc
import jbu_checks as jc
from densematcher_amd import extractor
from densematcher_amd.featup.upsamplers import JBULearnedRange, JBUStack

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dm_jbu_apply_bwd_filters_f32": 17, "dm_jbu_apply_bwd_source_f32": 12}


@pytest.mark.parametrize("shape", bc.SHAPES)
@pytest.mark.parametrize("kind", ["normal", "ones"])
def test_restatement_agrees_with_float64_autograd(shape, kind):
    o = bc.oracle(shape, kind)
    gsrc, gfilt = bc.restate(o["src"], o["filt"], o["gout"])
    for name, got, ref in (("gsrc", gsrc, o["gsrc64"]), ("gfilt", gfilt, o["gfilt64"])):
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"{shape} {kind} {name}: {err:.2e} relative; floors {o['floor_gsrc']:.2e} (gsrc), {o['floor_gfilt']:.2e} (gfilt)")
        assert got.shape == ref.shape and err <= 1e-12, (name, err)


def test_axis_matrix_rows():
    """every row holds the whole weight of its upsampled index; at 2 texels reflection and clamping cover the whole axis"""
    for n in (2, 3, 5, 11, 13):
        A = bc.axis_matrix(n)
        assert A.shape == (2 * n + 6, n) and np.allclose(A.sum(1), 1.0, atol=1e-15) and ((A != 0).sum(1) <= 4).all()
        assert np.array_equal(A[:3], A[4:7][::-1]) and np.array_equal(A[-3:], A[-7:-4][::-1])        # the reflection by 3


def test_forward_signatures_take_the_flag():
    for fn in (JBULearnedRange.forward, JBUStack.forward, JBUStack.upsample, extractor.upsample_features):
        assert inspect.signature(fn).parameters["differentiable"].default is False, fn


@pytest.mark.parametrize("route", ["torch", "auto"])
def test_torch_and_auto_ignore_the_flag(route):
    d, m = jc.case("b"), jc.model("b")                      # on the CPU: auto is the torch route with or without a GPU
    src, img = torch.from_numpy(d["src"]), torch.from_numpy(d["img"])
    with torch.no_grad():
        assert torch.equal(m(src, img, route=route, differentiable=True), m(src, img, route=route))
        g = img[:, :, :2 * src.shape[2], :2 * src.shape[3]]
        assert torch.equal(m.up1(src, g, route=route, differentiable=True), m.up1(src, g, route=route))
        assert torch.equal(extractor.upsample_features(m, src, img, route=route, differentiable=True), m(src, img, route=route))
    # and with a graph: the same gradients
    grads = []
    for flag in (False, True):
        s = src.clone().requires_grad_(True)
        m.zero_grad()
        m(s, img, route=route, differentiable=flag).square().sum().backward()
        grads.append([s.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    m.zero_grad()
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_differentiable_device_route_without_a_gpu():
    if torch.cuda.is_available():
        return                                              # what a process without a GPU answers
    d, m = jc.case("a"), jc.model("a")
    src, img = torch.from_numpy(d["src"]), torch.from_numpy(d["img"])
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU") as plain:
            m(src, img, route="device")
    for module, g in ((m, img), (m.up1, img[:, :, :6, :6])):
        for train in (False, True):
            module.train(train)
            with pytest.raises(RuntimeError, match="GPU") as flagged:                 # a gradient and training mode are no obstacles
                module(src.clone().requires_grad_(True), g, route="device", differentiable=True)
            assert str(flagged.value) == str(plain.value)
    m.eval()


def test_differentiable_device_route_refuses_by_name():
    d, m = jc.case("a"), jc.model("a")
    src, img = torch.from_numpy(d["src"]), torch.from_numpy(d["img"])
    with pytest.raises(ValueError, match="twice"):
        m.up1(src, img[:, :, :7, :6], route="device", differentiable=True)
    with pytest.raises(ValueError, match="2 x 2"):
        m(src[:, :, :1], img, route="device", differentiable=True)
    with pytest.raises(ValueError, match="float16 or float32"):
        m(src.double(), img, route="device", differentiable=True)
    with pytest.raises(ValueError, match="float32"):
        m(src, img.double(), route="device", differentiable=True)
    with pytest.raises(ValueError, match="route"):
        m(src, img, route="gpu", differentiable=True)
    with pytest.raises(ValueError, match="grad"):                                      # without the flag: as before
        m(src, img, route="device")


def test_adaptive_conv_names_the_differentiable_route():
    import sys
    from densematcher_amd.featup import adaptive_conv
    with pytest.raises(ValueError, match="differentiable=True"):
        adaptive_conv(torch.zeros(1, 1, 10, 10), torch.zeros(1, 4, 4, 7, 7), route="device")
    assert "differentiable=True" in sys.modules["densematcher_amd.featup.adaptive_conv"].__doc__


@pytest.fixture(scope="module")
def lib():
    from densematcher_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_entry_points_declared_bound_and_exported(lib):
    from densematcher_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "densematch.h")).read(), flags=re.S)
    for name, n_args in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert decl, f"{name} is not declared in densematch.h"
        assert len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} is not exported"


def test_null_context_is_refused(lib):
    assert lib.dm_jbu_apply_bwd_filters_f32(None, 1, 1, 2, 2, 2, None, 0, 0, 0, 0, None, 0, 0, 0, 0, None) != 0
    assert lib.dm_jbu_apply_bwd_source_f32(None, 1, 1, 2, 2, None, 0, 0, 0, 0, None, None) != 0

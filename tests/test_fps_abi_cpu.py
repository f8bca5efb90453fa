"""CPU: the entry points of farthest-point sampling and of the subsampled ZoomOut loop are declared in include/densematch.h, bound in
_lib.SIGNATURES and exported by the built library; the options that go with them exist."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dm_fps_euclid", "dm_fps_heat", "dm_zoomout_sub", "dm_zoomout_sub_f64")


@pytest.fixture(scope="module")
def lib():
    from densematcher_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_new_symbols_declared_bound_and_exported(lib):
    from densematcher_amd import _lib
    hdr = open(os.path.join(REPO, "include", "densematch.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert name in declared, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["dm_zoomout_sub"][1]) == 19 and _lib.SIGNATURES["dm_zoomout_sub_f64"] == _lib.SIGNATURES["dm_zoomout_sub"]
    assert len(_lib.SIGNATURES["dm_fps_euclid"][1]) == 8 and len(_lib.SIGNATURES["dm_fps_heat"][1]) == 9


def test_options_exist():
    from densematcher_amd.engine import MatchEngine
    assert MatchEngine.OPTION_DEFAULTS["zoomout_sub_fused"] == 1
    assert MatchEngine.OPTION_DEFAULTS["fps_heat_route"] == 0
    hdr = open(os.path.join(REPO, "include", "densematch.h")).read()
    assert '"zoomout_sub_fused"' in hdr and '"fps_heat_route"' in hdr
    assert "zoomout_sub_fused" in MatchEngine.set_option.__doc__


def test_null_context_is_refused(lib):
    assert lib.dm_fps_euclid(None, 1, 4, None, None, 2, None, None) != 0
    assert lib.dm_fps_heat(None, 1, 4, 2, None, 2, None, None, None) != 0
    assert lib.dm_zoomout_sub(None, 1, 4, 4, 2, 2, None, None, 1, 1, 1, None, 4, None, 4, None, None, None, None) != 0

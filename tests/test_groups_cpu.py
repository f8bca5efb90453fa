"""CPU: the semantic group distances (densematcher/utils.py:115-143).  The reference's own results (tests/golden/fx_groups.npz,
tools/make_golden_groups.py) against the restatement of tests/groups_restate.py and against densematcher_amd.utils on its host
route, exactly; empty groups and the VERBOSE warning; the ABI entry; the module's imports."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import groups_restate as gr
from conftest import REPO, load_golden


@pytest.fixture(scope="module")
def fx():
    g = load_golden("fx_groups.npz")
    return {"a": (load_golden("fx_geod.npz")["small_D"], gr.unpack_groups(g["a_flat"], g["a_off"]), g["a_dmtx"]),
            "b": (g["b_D"], gr.unpack_groups(g["b_flat"], g["b_off"]), g["b_dmtx"])}


def test_fixture_is_what_the_issue_describes(fx):
    D, groups, ref = fx["a"]
    assert D.shape == (160, 160) and not np.array_equal(D, D.T)
    assert len(groups) == 6 and [len(g) for g in groups].count(0) == 1 and ref.shape == (6, 6)
    D, groups, ref = fx["b"]
    assert D.shape == (96, 96) and np.array_equal(D, np.round(D)) and ref.shape == (len(groups), len(groups))
    assert any(len(set(g)) < len(g) for g in groups)                             # repeated indices
    assert set(groups[0]) & set(groups[1]) and len(set(i for g in groups for i in g)) < 96


@pytest.mark.parametrize("which", ["a", "b"])
def test_restatement_equals_reference(fx, which):
    D, groups, ref = fx[which]
    np.testing.assert_array_equal(gr.groups_dmtx(D, groups), ref)


@pytest.mark.parametrize("which", ["a", "b"])
def test_host_route_equals_reference(fx, which):
    from densematcher_amd import utils
    D, groups, ref = fx[which]
    got = utils.get_groups_dmtx(D, groups, device=False)
    assert got.dtype == np.float64 and got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(np.diag(got), 0.0)
    many = utils.get_groups_dmtx_many([D, D], [groups, groups[:3]], device=False)
    np.testing.assert_array_equal(many[0], ref)
    np.testing.assert_array_equal(many[1], ref[:3, :3])
    i, j = (0, 1)
    assert utils.get_distance_between_groups(D, groups[i], groups[j], device=False) == ref[i, j]


def test_orientation_rows_first_group(fx):
    from densematcher_amd import utils
    D, groups, ref = fx["a"]
    full = [g for g in groups if len(g)]
    d01 = utils.get_distance_between_groups(D, full[0], full[1], device=False)
    d10 = utils.get_distance_between_groups(D, full[1], full[0], device=False)
    assert d01 == gr.pair_distance(D, full[0], full[1]) and d10 == gr.pair_distance(D, full[1], full[0])
    got = utils.get_groups_dmtx(D, full[:2], device=False)
    assert got[0, 1] == d01 and got[1, 0] == d01                                 # the mirror is a copy, not the other orientation


def test_empty_groups_and_verbose(fx, capsys, monkeypatch):
    from densematcher_amd import utils
    D, groups, _ = fx["a"]
    warning = "Warning: empty group when computing distance between groups"
    monkeypatch.delenv("VERBOSE", raising=False)
    r = utils.get_distance_between_groups(D, [], groups[0], device=False)
    assert r == 0 and isinstance(r, int)
    assert utils.get_distance_between_groups(D, groups[0], [], device=False) == 0
    assert capsys.readouterr().out == ""
    monkeypatch.setenv("VERBOSE", "1")
    assert utils.get_distance_between_groups(D, [], groups[0], device=False) == 0
    assert capsys.readouterr().out.strip() == warning
    got = utils.get_groups_dmtx(D, [groups[0], [], groups[1]], device=False)
    assert capsys.readouterr().out.strip().splitlines() == [warning, warning]    # the pairs (0, 1) and (1, 2)
    assert got[0, 1] == 0 and got[1, 2] == 0 and got[1, 0] == 0 and got[0, 2] == gr.pair_distance(D, groups[0], groups[1])
    np.testing.assert_array_equal(utils.get_groups_dmtx(D, [groups[0]], device=False), [[0.0]])
    np.testing.assert_array_equal(utils.get_groups_dmtx(D, [groups[0], []], device=False), np.zeros((2, 2)))
    assert utils.get_groups_dmtx(D, [], device=False).shape == (0, 0)


def test_device_route_fails_closed_without_gpu(fx):
    import torch
    from densematcher_amd import utils
    D, groups, ref = fx["a"]
    if torch.cuda.is_available():
        return                                                                   # (tests/test_gpu_groups.py covers the device route)
    with pytest.raises(RuntimeError):
        utils.get_groups_dmtx(D, groups, device=True)
    np.testing.assert_array_equal(utils.get_groups_dmtx(D, groups), ref)         # device=None: the host route here


def test_abi_entry():
    from densematcher_amd import _build, _lib
    assert "dm_lsa_gather" in _lib.SIGNATURES and "dm_lsa_gather.hip" in _build.SOURCES
    header = open(os.path.join(REPO, "include", "densematch.h")).read()
    assert re.search(r"\bint dm_lsa_gather\(dm_ctx\* ctx,", header) and "densematcher/utils.py:115-143" in header
    lib = _lib.load()
    assert lib.dm_lsa_gather.argtypes == _lib.SIGNATURES["dm_lsa_gather"][1]
    assert len(_lib.SIGNATURES["dm_lsa_gather"][1]) == 13


def test_module_imports_without_rendering_packages():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('pytorch3d', 'meshplot', 'matplotlib', 'trimesh', 'cv2'):\n"
            "            raise ImportError('blocked: ' + name)\n"
            "sys.meta_path.insert(0, Block())\n"
            "import densematcher_amd.utils as u\n"
            "assert callable(u.get_distance_between_groups) and callable(u.get_groups_dmtx) and callable(u.get_groups_dmtx_many)\n"
            "assert not any(m.split('.')[0] in ('pytorch3d', 'meshplot') for m in sys.modules)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

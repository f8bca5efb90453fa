"""CPU: the host route of pyFM.spectral.shape_difference against the reference's own arrays (tests/golden/fx_sd.npz, written by
tools/make_golden_sd.py from a run of the reference) -- the same NumPy arithmetic, so every array must be BIT-identical, the noise
row 0 of the conformal operator at k1 = 5 (lambda_0 ~ -6e-15 survives np.linalg.pinv's cut-off there) and the exact-zero row 0 at
k1 = 12 included; the reference's assert and error; TriMesh.h1_inner; and the new entry points declared, bound and exported."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sparse

from conftest import load_golden
from densematcher_amd.pyFM import spectral
from densematcher_amd.pyFM.spectral import shape_difference as sd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [(5, None), (12, None), (17, 8), (40, 40)]
NEW = ("dm_shape_diff_f64", "dm_pullback_forms_f64")


class Mesh:
    """what compute_SD reads of a mesh"""
    def __init__(self, fx, q):
        n = fx[f"verts_{q}"].shape[0]
        self.vertlist, self.facelist = fx[f"verts_{q}"], fx[f"faces_{q}"]
        self.eigenvalues, self.eigenvectors = fx[f"lam_{q}"], fx[f"Phi_{q}"]
        self.A = sparse.diags(fx[f"mass_{q}"]).tocsr()
        self.W = sparse.coo_matrix((fx[f"W_val_{q}"], (fx[f"W_row_{q}"], fx[f"W_col_{q}"])), shape=(n, n)).tocsr()
        self.n_vertices = n


@pytest.fixture(scope="module")
def fx():
    return load_golden("fx_sd.npz")


@pytest.fixture(scope="module")
def pairs(fx):
    m = [Mesh(fx, q) for q in range(3)]
    return {"m": (m[0], m[1], fx["p2p"].astype(np.int64)), "i": (m[0], m[2], None)}


def tag(k1, k2):
    return f"{k1}_{'N' if k2 is None else k2}"


def same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} entries differ, max {np.abs(got - ref).max():.3e}"


def test_names_exported():
    for name in ("area_SD", "conformal_SD", "compute_SD", "compute_SD_many"):
        assert getattr(spectral, name) is getattr(sd, name)
    assert spectral.shape_difference is sd


@pytest.mark.parametrize("pn", ["m", "i"])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: tag(*d))
def test_area_and_conformal_of_stored_maps(fx, pairs, pn, dims):
    m1, m2, _ = pairs[pn]
    FM = fx[f"{pn}_FM_{tag(*dims)}"]
    same_bits(sd.area_SD(FM), fx[f"{pn}_FM_{tag(*dims)}_a"], "area_SD")
    same_bits(sd.conformal_SD(FM, m1.eigenvalues, m2.eigenvalues), fx[f"{pn}_FM_{tag(*dims)}_c"], "conformal_SD")


@pytest.mark.parametrize("pn", ["m", "i"])
@pytest.mark.parametrize("SD_type", ["spectral", "semican"])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: tag(*d))
def test_compute_SD_host_route_is_the_reference(fx, pairs, pn, SD_type, dims):
    m1, m2, p2p = pairs[pn]
    a, c = sd.compute_SD(m1, m2, k1=dims[0], k2=dims[1], p2p=p2p, SD_type=SD_type)
    assert isinstance(a, np.ndarray) and isinstance(c, np.ndarray)
    same_bits(a, fx[f"{pn}_{SD_type}_{tag(*dims)}_a"], "SD_a")
    same_bits(c, fx[f"{pn}_{SD_type}_{tag(*dims)}_c"], "SD_c")
    if dims[0] == 5:                 # lambda_0 is kept: row 0 is noise / lambda_0, and still the reference's bits
        assert np.any(c[0] != 0.0)
    if dims[0] == 12:                # lambda_0 is cut: exact zeros
        assert not np.any(c[0] != 0.0) and np.any(c[1] != 0.0)


def test_defaults_and_silent_clipping(fx, pairs):
    """k1 = all of mesh1's eigenpairs, k2 = 3 k1 clipped silently to the 40 that mesh2 holds: the (40, 40) arrays"""
    m1, m2, p2p = pairs["m"]
    for SD_type in ("spectral", "semican"):
        a, c = sd.compute_SD(m1, m2, p2p=p2p, SD_type=SD_type)
        same_bits(a, fx[f"m_{SD_type}_40_40_a"], "SD_a")
        same_bits(c, fx[f"m_{SD_type}_40_40_c"], "SD_c")
    la, lc = sd.compute_SD_many(m1, [m2, pairs["i"][1]], k1=12, p2ps=[p2p, None], SD_type="semican", device=False)
    same_bits(la[0], fx["m_semican_12_N_a"], "many[0]")
    same_bits(lc[1], fx["i_semican_12_N_c"], "many[1]")


def test_unknown_type_asserts(pairs):
    m1, m2, p2p = pairs["m"]
    with pytest.raises(AssertionError, match="Problem with type of SD type : other"):
        sd.compute_SD(m1, m2, k1=5, p2p=p2p, SD_type="other")
    with pytest.raises(AssertionError):
        sd.compute_SD_many([m1], [m2], k1=5, p2ps=[p2p], SD_type="other", device=False)


def test_functional_mapping_before_fit(fx):
    from densematcher_amd.pyFM.functional import FunctionalMapping
    from densematcher_amd.pyFM.mesh import TriMesh
    model = FunctionalMapping(TriMesh(fx["verts_0"], fx["faces_0"]), TriMesh(fx["verts_2"], fx["faces_2"]))
    assert model.SD_a is None and model.SD_c is None
    with pytest.raises(ValueError, match="The Functional map must be fit before computing the shape difference"):
        model.compute_SD()
    # a map set by hand: the host functions, under the reference's names D_a / D_c
    model.mesh1.eigenvalues, model.mesh2.eigenvalues = fx["lam_0"], fx["lam_2"]
    model.FM = fx["i_FM_17_8"]
    model.compute_SD()
    same_bits(model.D_a, fx["i_FM_17_8_a"], "D_a")
    same_bits(model.D_c, fx["i_FM_17_8_c"], "D_c")


def test_h1_inner_is_the_quadratic_form_of_W(fx, pairs):
    from densematcher_amd.pyFM.mesh import TriMesh
    mesh = TriMesh(fx["verts_1"], fx["faces_1"])
    mesh.W = pairs["m"][1].W
    rng = np.random.default_rng(5)
    f, g = rng.standard_normal((2, mesh.n_vertices))
    assert mesh.h1_inner(f, g) == f.T @ mesh.W @ g
    assert mesh.h1_sqnorm(f) == f.T @ mesh.W @ f
    F, G = rng.standard_normal((2, mesh.n_vertices, 3))
    got = mesh.h1_inner(F, G)
    assert got.shape == (3,)
    assert np.array_equal(got, np.einsum('np,np->p', F, mesh.W @ G))
    assert np.array_equal(mesh.h1_sqnorm(F), mesh.h1_inner(F, F))
    with pytest.raises(AssertionError):
        mesh.h1_inner(f, F)


# ---- ABI
@pytest.fixture(scope="module")
def lib():
    from densematcher_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_new_symbols_declared_bound_and_exported(lib):
    from densematcher_amd import _build, _lib
    hdr = open(os.path.join(REPO, "include", "densematch.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert name in declared, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["dm_shape_diff_f64"][1]) == 12 and len(_lib.SIGNATURES["dm_pullback_forms_f64"][1]) == 18
    assert "dm_shapediff.hip" in _build.SOURCES


def test_null_context_is_refused(lib):
    assert lib.dm_shape_diff_f64(None, 1, 4, 4, None, 4, None, 4, None, 4, None, None) != 0
    assert lib.dm_pullback_forms_f64(None, 1, 4, 4, 2, None, None, 2, None, None, 1, None, None, None, None, 0, None, None) != 0


def test_engine_methods_exist():
    from densematcher_amd.engine import MatchEngine
    assert callable(MatchEngine.shape_difference) and callable(MatchEngine.pullback_forms) and callable(MatchEngine._stiffness_rows)
    assert (MatchEngine.SD_MAX_K1, MatchEngine.SD_MAX_K2) == (256, 768)

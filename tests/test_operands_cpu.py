"""The operand layer of MatchEngine (densematcher_amd/_operands.py) on CPU tensors and NumPy arrays: the stride rule of the ABI,
CSR -> ELL rows, the count / index tables of padded batches and their range checks, info words -> errors.  Expected values are
written out; none is computed from a second copy of the helper."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from densematcher_amd import _operands as ops

BASE = torch.zeros(4, 6, 10)
VIEWS = [
    ("base", BASE, 10),
    ("columns cut", BASE[:, :, :7], 10),
    ("columns from an offset", BASE[:, :, 2:9], 10),
    ("meshes from an offset", BASE[1:], 10),
    ("every second row", BASE[:, ::2, :], 20),
    ("one mesh, rows and columns cut", BASE[:1, :5, :7], 10),
    ("one column", BASE[:, :, 3:4], 10),
    ("one row per mesh: the batch stride", BASE[:, :1, :7], 60),
    ("one row of one mesh", BASE[2:3, 1:2, :7], 7),
    ("rows cut: meshes not N ld apart", BASE[:, :5, :], None),
    ("every second column", BASE[:, :, ::2], None),
    ("transposed", BASE.transpose(1, 2), None),
    ("expanded", torch.zeros(1, 6, 10).expand(4, 6, 10), None),
    ("a corner of square matrices", torch.zeros(3, 8, 8)[:, :5, :5], None),
    ("2-D", BASE[0], 10),
    ("2-D, columns cut", BASE[0][:, :7], 10),
    ("2-D, transposed", BASE[0].t(), None),
    ("2-D, one row", BASE[0][:1, :7], 7),
]


@pytest.mark.parametrize("name,view,ld", VIEWS, ids=[v[0] for v in VIEWS])
def test_fits_abi(name, view, ld):
    assert ops.fits_abi(view) == ld


def test_fits_abi_row_stride_must_fit_an_int():
    assert ops.fits_strides((2, 3, 5), (3 * 2 ** 31, 2 ** 31, 1)) is None
    assert ops.fits_strides((2, 3, 5), (3 * (2 ** 31 - 1), 2 ** 31 - 1, 1)) == 2 ** 31 - 1
    assert ops.fits_strides((2, 3, 5), (24, 8, 1), min_ld=8) == 8
    assert ops.fits_strides((2, 3, 5), (24, 8, 1), min_ld=9) is None


# row 0: two entries; row 1: empty; row 2: three entries, columns unsorted; row 3: one explicit zero; row 4: two entries
INDPTR = np.array([0, 2, 2, 5, 6, 8])
INDICES = np.array([1, 3, 4, 0, 2, 3, 0, 4])
DATA = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 6.0, 7.0])
ELL_COLS = [[1, 3, -1], [-1, -1, -1], [4, 0, 2], [3, -1, -1], [0, 4, -1]]
ELL_VALS = [[1.0, 2.0, 0.0], [0.0, 0.0, 0.0], [3.0, 4.0, 5.0], [0.0, 0.0, 0.0], [6.0, 7.0, 0.0]]


def test_csr_to_ell_keeps_order_zeros_and_pads():
    M = sp.csr_matrix((DATA, INDICES, INDPTR), shape=(5, 5))
    cols, vals = ops.csr_to_ell(M.indptr, M.indices, M.data, 5)
    assert cols.dtype == np.int32 and vals.dtype == np.float64 and cols.shape == (5, 3)
    assert cols.tolist() == ELL_COLS and vals.tolist() == ELL_VALS
    assert cols[3, 0] == 3 and vals[3, 0] == 0.0                    # the explicit zero is an entry, not padding
    dense = np.zeros((5, 5))
    r, q = np.nonzero(cols >= 0)
    dense[r, cols[r, q]] = vals[r, q]
    assert np.array_equal(dense, M.toarray())


def test_csr_to_ell_on_csc_gives_the_vertex_minor_layout():
    G = sp.csc_matrix((DATA, INDICES, INDPTR), shape=(5, 5))        # column v holds the edges into v
    cols, w = ops.csr_to_ell(G.indptr, G.indices, G.data, 5)
    assert cols.T.tolist() == [[1, -1, 4, 3, 0], [3, -1, 0, -1, 4], [-1, -1, 2, -1, -1]]
    dense = np.zeros((5, 5))
    q, v = np.nonzero(cols.T >= 0)
    dense[cols.T[q, v], v] = w.T[q, v]
    assert np.array_equal(dense, G.toarray())


def test_csr_to_ell_width_and_padding_column():
    E = sp.csr_matrix((5, 5))
    cols, vals = ops.csr_to_ell(E.indptr, E.indices, E.data, 5)
    assert cols.tolist() == [[-1]] * 5 and vals.tolist() == [[0.0]] * 5
    cols, vals = ops.csr_to_ell(INDPTR, INDICES, DATA, 5, 4, np.arange(5)[:, None])
    assert cols.tolist() == [[1, 3, 0, 0], [1, 1, 1, 1], [4, 0, 2, 2], [3, 3, 3, 3], [0, 4, 4, 4]]
    assert vals[:, 3].tolist() == [0.0] * 5


def test_stack_ell():
    rows = [(torch.tensor([[1], [0]]), torch.tensor([[2.0], [3.0]])), (torch.tensor([[1, 2], [0, -1], [0, -1]]), torch.ones(3, 2))]
    cols, w = ops.stack_ell(rows, 3, "cpu")
    assert cols.dtype == torch.int32 and w.dtype == torch.float64
    assert cols.tolist() == [[[1, -1], [0, -1], [-1, -1]], [[1, 2], [0, -1], [0, -1]]]
    assert w.tolist() == [[[2.0, 0.0], [3.0, 0.0], [0.0, 0.0]], [[1.0, 1.0]] * 3]


def test_counts():
    for given, want in ((None, [5, 5]), (3, [3, 3]), ([5, 3], [5, 3]), (np.array([[1], [5]]), [1, 5])):
        nv = ops.counts(given, 2, 5, 1, "who")
        assert nv.dtype == np.int32 and nv.flags.c_contiguous and nv.tolist() == want
    assert ops.counts([5, 0], 2, 5, 0, "who").tolist() == [5, 0]
    for given, lo in (([5, 0], 1), ([6, 3], 1), ([-1, 3], 0), ([5, 6], 0)):
        with pytest.raises(ValueError, match=r"who: n_verts must lie in \[%d, N\]" % lo):
            ops.counts(given, 2, 5, lo, "who")
    with pytest.raises(ValueError, match=r"who: n_verts2 must lie in \[1, 5\]"):
        ops.counts([5, 6], 2, 5, 1, "who", "n_verts2", 5)


def test_problem_meshes():
    for given, want in ((None, [0, 0, 0]), (1, [1, 1, 1]), ([0, 1, 1], [0, 1, 1])):
        mesh = ops.problem_meshes(given, 3, 2, "who")
        assert mesh.dtype == np.int64 and mesh.tolist() == want
    assert ops.problem_meshes(None, 0, 2, "who").shape == (0,)
    for given in (2, [0, 1, -1]):
        with pytest.raises(ValueError, match=r"who: mesh indices must lie in \[0, 2\)"):
            ops.problem_meshes(given, 3, 2, "who")


def test_source_table():
    for given, want in ((None, [[0, 1, 2, 3, 4], [0, 1, 2, -1, -1]]), ([0, 2], [[0, 2], [0, 2]]), ([[4, -1], [2, 0]], [[4, -1], [2, 0]])):
        src = ops.source_table(given, [5, 3], 5, "who")
        assert src.dtype == np.int32 and src.flags.c_contiguous and src.tolist() == want
    for given, mesh, n in (([0, 3], 1, 3), ([[5, 0], [0, 0]], 0, 5), ([[0, 0], [0, -2]], 1, 3)):
        with pytest.raises(ValueError, match=r"who: mesh %d: source indices must lie in \[0, %d\)" % (mesh, n)):
            ops.source_table(given, [5, 3], 5, "who")
    for given in (np.zeros((2, 0), np.int64), np.zeros((3, 2), np.int64), np.zeros((1, 2, 2), np.int64)):
        with pytest.raises(ValueError, match=r"who: sources must be \(ns,\) or \(2, ns\)"):
            ops.source_table(given, [5, 3], 5, "who")


def test_start_vertices():
    for given, want in ((2, [2, 2]), ([4, 2], [4, 2]), (0, [0, 0])):
        st = ops.start_vertices(given, [5, 3], "who")
        assert st.dtype == np.int32 and st.flags.c_contiguous and st.tolist() == want
    for given, mesh, n in ((3, 1, 3), ([5, 0], 0, 5), ([0, -1], 1, 3)):
        with pytest.raises(ValueError, match=r"who: mesh %d: the start vertex must lie in \[0, %d\)" % (mesh, n)):
            ops.start_vertices(given, [5, 3], "who")


def test_index_list_is_strict():
    a = ops.index_list([0, 4, 4], 5, "who")
    assert a.dtype == np.int32 and a.tolist() == [0, 4, 4]
    assert ops.index_list([], 5, "who").size == 0
    for given in ([0, 5], [-1, 2]):
        with pytest.raises(ValueError, match=r"who: vertex indices must lie in \[0, 5\)"):
            ops.index_list(given, 5, "who")
    with pytest.raises(ValueError, match="must hold integers"):
        ops.index_list([0.0, 1.0], 5, "who")
    with pytest.raises(ValueError, match="one-dimensional"):
        ops.index_list([[0, 1]], 5, "who")


def test_numpy_index_follows_numpy():
    a = ops.numpy_index([-5, -1, 0, 4], 5, "who")
    assert a.dtype == np.int32 and a.tolist() == [0, 4, 0, 4]
    assert ops.numpy_index(torch.tensor([-2, 1]), 5, "who").tolist() == [3, 1]
    assert ops.numpy_index([], 5, "who").size == 0
    for given, shown in (([0, 5], 5), ([-6, 0], -6)):
        with pytest.raises(IndexError, match=f"who: index {shown} is out of bounds for axis 0 with size 5"):
            ops.numpy_index(given, 5, "who")
    with pytest.raises(IndexError, match="arrays used as indices must be of integer type"):
        ops.numpy_index([0.0], 5, "who")


def test_raise_info_names_the_mesh_and_joins_the_bits():
    from densematcher_amd.engine import MatchEngine
    ops.raise_info(np.zeros(2, np.int32), MatchEngine._GEOD_INFO, "who")
    with pytest.raises(ValueError) as e:
        ops.raise_info(np.array([0, 5], np.int32), MatchEngine._GEOD_INFO, "who")
    assert str(e.value) == "who: mesh 1: A + tW is not positive definite; the mesh has a face of zero area"
    with pytest.raises(ValueError, match="^who: pair 0: a source lies outside$"):
        ops.raise_info(np.array([2, 1], np.int32), ((~0, "a source lies outside"),), "who", what="pair")

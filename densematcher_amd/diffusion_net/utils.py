"""The helpers of the reference's diffusion_net/utils.py that geometry.py uses (array conversions, the cache's hash)."""
import hashlib
import os

import numpy as np
import scipy.sparse
import torch


def toNP(x):
    return x.detach().to(torch.device("cpu")).numpy()


def sparse_np_to_torch(A, dtype=torch.float32):
    """SciPy sparse -> coalesced torch COO (the reference builds float32 values here; `dtype` keeps float64 where the caller rounds once)"""
    Acoo = A.tocoo()
    indices = torch.from_numpy(np.vstack((Acoo.row, Acoo.col)).astype(np.int64))
    return torch.sparse_coo_tensor(indices, torch.from_numpy(np.asarray(Acoo.data)).to(dtype), torch.Size(Acoo.shape)).coalesce()


def sparse_torch_to_np(A):
    """torch sparse COO matrix -> SciPy CSC"""
    if A.dim() != 2:
        raise RuntimeError(f"sparse_torch_to_np takes a matrix, not a tensor of shape {tuple(A.shape)}")
    A = A.coalesce()
    row, col = toNP(A.indices())
    return scipy.sparse.csc_matrix((toNP(A.values()), (row, col)), shape=tuple(A.shape))


def hash_arrays(arrs):
    """hex SHA-1 of the arrays' bytes, one after the other (the name of a mesh's file in the operator cache)"""
    h = hashlib.sha1()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def ensure_dir_exists(d):
    os.makedirs(d, exist_ok=True)

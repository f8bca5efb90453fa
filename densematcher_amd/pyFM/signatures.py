"""
Spectral point signatures with the reference's interface and parameter choices
(densematcher/pyFM/signatures/{HKS_functions,WKS_functions}.py): an alternative descriptor source of
FunctionalMapping.preprocess (functional.py:308-329) besides the neural features.  Host NumPy float64 like the
reference -- one (N x k) by (k x n_descr) product per mesh; mesh_HKS_many / mesh_WKS_many below run the same products on the device.

Both signatures are   S[n, t] = sum_k w[t, k] Phi[n, k]^2 / sum_k w[t, k]     (scaled=True everywhere in the reference)
and their landmark versions   S_p[n, t] = sum_k w[t, k] Phi[p, k] Phi[n, k] / sum_k w[t, k]   for each landmark p:
  HKS:  w[t, k] = exp(-t lambda_k),  t log-spaced in [4 ln10 / lambda_max, 4 ln10 / lambda_1]        HKS_functions.py:97-98
  WKS:  w[e, k] = exp(-(e - ln lambda_k)^2 / (2 sigma^2)),  sigma = 7 (ln lambda_max - ln lambda_1) / n,
        e linearly spaced in [ln lambda_1 + 2 sigma, ln lambda_max - 2 sigma], eigenvalues <= 1e-5 (landmark version:
        <= 1e-2) left out                                                                             WKS_functions.py:29,71,118-126
"""
import numpy as np


def _weighted(weights, evects, landmarks):
    """weights (T, K), evects (N, K) -> (N, T), or (N, p*T) with the landmark-major column order of the reference
    (HKS_functions.py:73: reshape of a (p, T, N) array)."""
    scale = 1.0 / weights.sum(axis=1)                                        # (T,)
    if landmarks is None:
        return (np.square(evects) @ weights.T) * scale[None, :]
    lm = np.asarray(landmarks).reshape(-1)
    cols = [(evects * evects[p][None, :]) @ weights.T * scale[None, :] for p in lm]      # each (N, T)
    return np.concatenate(cols, axis=1)


def auto_HKS(evals, evects, num_T, landmarks=None, scaled=True):
    if not scaled:
        raise NotImplementedError("the reference only ever calls the scaled signature")
    lam = np.sort(np.abs(np.asarray(evals, dtype=np.float64).reshape(-1)))
    times = np.geomspace(4 * np.log(10) / lam[-1], 4 * np.log(10) / lam[1], num_T)
    weights = np.exp(-np.outer(times, lam))
    return _weighted(weights, np.asarray(evects, dtype=np.float64), landmarks)


def auto_WKS(evals, evects, num_E, landmarks=None, scaled=True):
    if not scaled:
        raise NotImplementedError("the reference only ever calls the scaled signature")
    lam = np.sort(np.abs(np.asarray(evals, dtype=np.float64).reshape(-1)))
    e_min, e_max = np.log(lam[1]), np.log(lam[-1])
    sigma = 7 * (e_max - e_min) / num_E
    assert sigma > 0, f"Sigma should be positive ! Given value : {sigma}"
    energies = np.linspace(e_min + 2 * sigma, e_max - 2 * sigma, num_E)
    keep = lam > (1e-5 if landmarks is None else 1e-2)
    weights = np.exp(-np.square(energies[:, None] - np.log(lam[keep])[None, :]) / (2 * sigma ** 2))
    return _weighted(weights, np.asarray(evects, dtype=np.float64)[:, keep], landmarks)


def _mesh_signature(fn, mesh, num, landmarks, k):
    assert mesh.eigenvalues is not None, "Eigenvalues should be processed"
    if k is None:
        k = len(mesh.eigenvalues)
    return fn(mesh.eigenvalues[:k], mesh.eigenvectors[:, :k], num, landmarks=landmarks, scaled=True)


def mesh_HKS(mesh, num_T, landmarks=None, k=None):
    """Heat kernel signature of a processed mesh, (N, num_T) or (N, p*num_T)  -- HKS_functions.py:106-135"""
    return _mesh_signature(auto_HKS, mesh, num_T, landmarks, k)


def mesh_WKS(mesh, num_E, landmarks=None, k=None):
    """Wave kernel signature of a processed mesh, (N, num_E) or (N, p*num_E)  -- WKS_functions.py:127-152"""
    return _mesh_signature(auto_WKS, mesh, num_E, landmarks, k)


# ---------------------------------------------------------------------------------------------------------------------
# The same signatures on the device (csrc/dm_signatures.hip).  The parameter table -- times or energies, the sorted spectrum
# (or its logarithm), 2 sigma^2, the first eigen-column kept -- is built here with the very NumPy calls of auto_HKS /
# auto_WKS above, so that exp sees the same arguments on both routes; the device forms the weights, their sums and the products.
def signature_tables(evals, kind, num, landmark_version=False):
    """(t (num,), mu (K,), denom, k0) of one mesh such that the weights of auto_HKS / auto_WKS are exactly
        HKS:  exp(-(t[:, None] * mu[None, :]))                                   k0 = 0
        WKS:  exp(-np.square(t[:, None] - mu[None, k0:]) / denom)                on the eigen-columns k0 .. K-1
    landmark_version: WKS keeps lambda > 1e-2 instead of > 1e-5 (WKS_functions.py:71,118).  The sorted |lambda| is ascending, so
    what is kept is a suffix.  t, mu and denom do not depend on landmark_version."""
    lam = np.sort(np.abs(np.asarray(evals, dtype=np.float64).reshape(-1)))
    if kind == "HKS":
        times = np.geomspace(4 * np.log(10) / lam[-1], 4 * np.log(10) / lam[1], num)
        return times, lam, 1.0, 0
    if kind != "WKS":
        raise ValueError(f'signature kind must be "HKS" or "WKS", not {kind!r}')
    e_min, e_max = np.log(lam[1]), np.log(lam[-1])
    sigma = 7 * (e_max - e_min) / num
    assert sigma > 0, f"Sigma should be positive ! Given value : {sigma}"
    energies = np.linspace(e_min + 2 * sigma, e_max - 2 * sigma, num)
    keep = lam > (1e-2 if landmark_version else 1e-5)
    k0 = int(len(lam) - np.count_nonzero(keep))
    with np.errstate(divide="ignore"):
        mu = np.log(lam)                                   # (-inf where lambda = 0: a dropped column, never read)
    return energies, mu, float(2 * sigma ** 2), k0


def _signatures_many(kind, meshes, num, landmarks_list, k, device):
    from ..engine import default_engine
    eng = default_engine(device)
    meshes = list(meshes)
    if landmarks_list is None:
        landmarks_list = [None] * len(meshes)
    assert len(landmarks_list) == len(meshes)
    lms = [None if lm is None else np.asarray(lm).reshape(-1) for lm in landmarks_list]
    groups = {}
    for i, m in enumerate(meshes):
        assert m.eigenvalues is not None, "Eigenvalues should be processed"
        kk = len(m.eigenvalues) if k is None else min(k, len(m.eigenvalues))
        ev = np.asarray(m.eigenvectors)
        groups.setdefault((ev.shape[0], kk, str(ev.dtype), None if lms[i] is None else len(lms[i])), []).append(i)
    out = [None] * len(meshes)
    for (n, kk, _, p), idx in groups.items():                                    # one launch per group of equal N
        Phi = np.stack([np.asarray(meshes[i].eigenvectors)[:, :kk] for i in idx])
        lam = np.stack([np.asarray(meshes[i].eigenvalues, dtype=np.float64)[:kk] for i in idx])
        lm = None if p is None else np.stack([lms[i] for i in idx])
        S = eng.signatures(Phi, lam, kind, num, landmarks=lm, plain=p is None).cpu().numpy()
        for q, i in enumerate(idx):
            out[i] = S[q]
    return out


def mesh_HKS_many(meshes, num, landmarks_list=None, k=None, device=None):
    """mesh_HKS of every mesh (landmarks_list: None, or per mesh None | indices) on the GPU: list of NumPy float64 arrays"""
    return _signatures_many("HKS", meshes, num, landmarks_list, k, device)


def mesh_WKS_many(meshes, num, landmarks_list=None, k=None, device=None):
    """mesh_WKS of every mesh on the GPU: list of NumPy float64 arrays"""
    return _signatures_many("WKS", meshes, num, landmarks_list, k, device)


class LazySignature:
    """descr1 / descr2 of the models compute_surface_map_batch(descr_type="HKS" | "WKS") returns: the (N, num) plain signature of
    `mesh`, kept implicit.  The batched call computes the values on the device and feeds them to the fit without ever bringing them
    to the host; converting this object to an array (np.asarray, indexing, arithmetic) evaluates the host mirror above on demand.
    It makes no download and holds no device memory."""
    ndim = 2
    dtype = np.dtype(np.float64)

    def __init__(self, mesh, kind, num, k):
        assert kind in ("HKS", "WKS")
        self._mesh, self.kind, self.num, self.k = mesh, kind, int(num), k

    @property
    def shape(self):
        return (self._mesh.n_vertices, self.num)

    def __len__(self):
        return self.shape[0]

    def __array__(self, dtype=None, copy=None):
        a = (mesh_HKS if self.kind == "HKS" else mesh_WKS)(self._mesh, self.num, k=self.k)
        return a if dtype is None else a.astype(dtype, copy=False)

    def __getitem__(self, item):
        return np.asarray(self)[item]

    def astype(self, dtype, **kw):
        return np.asarray(self).astype(dtype, **kw)

"""The precise map's reference side, restated independently: a closest-point-on-triangle solver in np.longdouble that knows nothing of
Eberly's regions, a classifier that names the return statement _point_triangle / point_triangle leaves through, and the designed inputs
(four planar triangles, the open obtuse corner, lattice and sliver meshes) that tests/test_precise_cpu.py, tests/test_gpu_precise.py and
tools/make_golden_precise.py share.  A helper module, not a test file."""
import hashlib

import numpy as np

LD = np.longdouble

LABELS = ("0", "1a", "1b", "1c", "2a", "2b", "2c", "2d", "2e", "3a", "3b", "3c", "4a", "4b", "4c", "4d", "4e",
          "5a", "5b", "5c", "6a", "6b", "6c", "6d", "6e")

# (x, y) of the three corners; the obtuse ones are what regions 2, 4 and 6 need to reach their far branches
SHAPES = {
    "acute": ((0.0, 0.0), (1.0, 0.0), (0.4, 0.9)),
    "obtuse0": ((0.0, 0.0), (1.0, 0.0), (-0.6, 0.5)),
    "obtuse1": ((0.0, 0.0), (1.0, 0.0), (1.6, 0.5)),
    "obtuse2": ((0.0, 0.0), (1.0, 0.0), (0.5, 0.15)),
}
# the open obtuse corner and a large triangle far below it: in the cone behind vertex 0 the vectorised reference's region-4
# distances (formed with the unclamped s / t) overstate the corner's distance, and near the bisector the far triangle wins
CORNER_V3 = np.array([(0, 0, 0), (1, 0, 0), (-.6, .5, 0), (-3, -6, 0), (5, -6, 0), (1, -6, 4)], dtype=np.float64)
CORNER_FACES = {"corner": np.array([[0, 1, 2], [3, 4, 5]]), "twin": np.array([[0, 2, 1], [3, 4, 5]])}


# --------------------------------------------------------------------------- #
# the independent solver
def _dot(x, y):
    return (x * y).sum(-1)


def closest_point(tris, pts):
    """Closest point of triangle tris[i] (.., 3, k) to pts[i] (.., k), pairwise with broadcasting, in np.longdouble: the foot of the
    perpendicular on the triangle's plane if it lies inside, else the nearest of the three clamped segment projections.
    Returns (point (m,k), bary (m,3), distance (m,)) as longdouble."""
    T, P = np.asarray(tris, dtype=LD), np.asarray(pts, dtype=LD)
    T = T[None] if T.ndim == 2 else T
    P = P[None] if P.ndim == 1 else P
    m = max(T.shape[0], P.shape[0])
    T, P = np.broadcast_to(T, (m,) + T.shape[1:]), np.broadcast_to(P, (m, P.shape[1]))
    best_d2 = np.full(m, np.inf, dtype=LD)
    best_q = np.zeros(P.shape, dtype=LD)
    best_b = np.zeros((m, 3), dtype=LD)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        a, e = T[:, i], T[:, j] - T[:, i]
        L = _dot(e, e)
        lam = np.clip(np.where(L > 0, _dot(P - a, e) / np.where(L > 0, L, 1), 0), 0, 1)
        q = a + lam[:, None] * e
        d2 = _dot(P - q, P - q)
        upd = d2 < best_d2
        bb = np.zeros((m, 3), dtype=LD)
        bb[:, i], bb[:, j] = 1 - lam, lam
        best_d2, best_q, best_b = np.where(upd, d2, best_d2), np.where(upd[:, None], q, best_q), np.where(upd[:, None], bb, best_b)
    v0, u, w = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    r = P - v0
    uu, uw, ww, ru, rw = _dot(u, u), _dot(u, w), _dot(w, w), _dot(r, u), _dot(r, w)
    det = uu * ww - uw * uw
    ok = det > 0
    sd = np.where(ok, det, 1)
    s, t = (ww * ru - uw * rw) / sd, (uu * rw - uw * ru) / sd
    inside = ok & (s >= 0) & (t >= 0) & (s + t <= 1)
    q = v0 + s[:, None] * u + t[:, None] * w
    bb = np.stack([1 - s - t, s, t], 1)
    best_q, best_b = np.where(inside[:, None], q, best_q), np.where(inside[:, None], bb, best_b)
    best_d2 = np.where(inside, _dot(P - q, P - q), best_d2)
    return best_q, best_b, np.sqrt(best_d2)


def nearest_distance(V, faces, P, slack=1e-9):
    """min over ALL faces of the distance of every point to the face, by closest_point.  A face whose nearest corner is farther than
    the point's nearest vertex plus the face's longest edge cannot hold the minimum (every point of a face lies within one edge
    length of each corner, and the nearest vertex itself is a point of the surface), so it is left out -- with `slack` to spare,
    the bound being evaluated in float64.  Returns (distance (n,) longdouble, face (n,))."""
    V, P, faces = np.asarray(V, np.float64), np.asarray(P, np.float64), np.asarray(faces)
    tri = V[faces]
    lmax = np.max([np.linalg.norm(tri[:, a] - tri[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))], axis=0)
    out_d, out_f = np.zeros(len(P), dtype=LD), np.zeros(len(P), dtype=np.int64)
    for i, p in enumerate(P):
        dv = np.linalg.norm(V - p, axis=1)
        keep = np.where(dv[faces].min(1) - lmax <= dv.min() + slack)[0]
        d = closest_point(tri[keep], p)[2]
        j = int(np.argmin(d))
        out_d[i], out_f[i] = d[j], keep[j]
    return out_d, out_f


# --------------------------------------------------------------------------- #
# which return statement?
def branch(a, b, c, d, e, f):
    """The label of the return statement that _point_triangle (oracle) / point_triangle (dm_precise.hip) leaves through for these
    arguments: the region's number and the statement's letter, in the order the statements stand in the code."""
    det = a * c - b * b
    s = b * e - c * d
    t = b * d - a * e
    if s + t <= det:
        if s < 0:
            if t < 0:
                if d < 0:
                    return "4a" if -d >= a else "4b"
                if e >= 0:
                    return "4c"
                return "4d" if -e >= c else "4e"
            if e >= 0:
                return "3a"
            return "3b" if -e >= c else "3c"
        if t < 0:
            if d >= 0:
                return "5a"
            return "5b" if -d >= a else "5c"
        return "0"
    if s < 0:
        tmp0, tmp1 = b + d, c + e
        if tmp1 > tmp0:
            return "2a" if tmp1 - tmp0 >= a - 2.0 * b + c else "2b"
        if tmp1 <= 0:
            return "2c"
        return "2d" if e >= 0 else "2e"
    if t < 0:
        tmp0, tmp1 = b + e, a + d
        if tmp1 > tmp0:
            return "6a" if tmp1 - tmp0 >= a - 2.0 * b + c else "6b"
        if tmp1 <= 0:
            return "6c"
        return "6d" if d >= 0 else "6e"
    numer = c + e - b - d
    if numer <= 0:
        return "1a"
    return "1b" if numer >= a - 2.0 * b + c else "1c"


def abcdef(tri, P):
    """the six arguments of _point_triangle for one triangle (3,k) and the points (n,k), formed as the oracle forms them -> (n,6)"""
    tri, P = np.asarray(tri, np.float64), np.asarray(P, np.float64)
    ax1, ax2 = tri[1] - tri[0], tri[2] - tri[0]
    diff = tri[0] - P
    n = len(P)
    return np.stack([np.full(n, ax1 @ ax1), np.full(n, ax1 @ ax2), np.full(n, ax2 @ ax2), diff @ ax1, diff @ ax2,
                     np.einsum("ij,ij->i", diff, diff)], 1)


def branches(tri, P):
    return np.array([branch(*row) for row in abcdef(tri, P)])


# --------------------------------------------------------------------------- #
# designed inputs
def rotation(k, seed):
    """a seeded random orthogonal k x k matrix"""
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((k, k)))
    return q * np.sign(np.diag(r))


def embed(X3, k, seed, f32=True):
    """rows (x, y, z) -> k dimensions: padded with zeros (k = 2: z dropped) and turned by rotation(k, seed); f32: rounded to float32
    values (what the float32 entry point is handed), returned as float64"""
    X3 = np.asarray(X3, np.float64)
    X = np.zeros((X3.shape[0], k))
    X[:, :min(k, 3)] = X3[:, :min(k, 3)]
    X = X @ rotation(k, seed).T
    return X.astype(np.float32).astype(np.float64) if f32 else X


def plane_grid(k):
    """linspace(-2, 3, 41)^2 at heights 0 and 0.3 (k = 2 has no room for a height: the plane once)"""
    g = np.linspace(-2.0, 3.0, 41)
    x, y = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    return np.concatenate([np.stack([x, y, np.full_like(x, h)], 1) for h in ((0.0,) if k == 2 else (0.0, 0.3))])


def designed_case(shape, k, seed=0, f32=True):
    """one of SHAPES and the grid around it in k dimensions -> (V (3,k), P (n,k)), turned by the same rotation"""
    tri = np.array([(x, y, 0.0) for x, y in SHAPES[shape]])
    both = embed(np.concatenate([tri, plane_grid(k)]), k, 1000 * seed + k, f32)
    return both[:3], both[3:]


def corner_points():
    """the points of the open-corner fixture (3-d): a coarse 31 x 41 x 2 grid over the cone behind vertex 0, refined around the two
    zones where the corner and the far triangle are about equally far -- below the edge 0-1, and beside the edge 0-2"""
    def lift(x, y):
        return np.concatenate([np.stack([x.ravel(), y.ravel(), np.full(x.size, h)], 1) for h in (0.0, 0.3)])
    x, y = np.meshgrid(np.linspace(-4.0, 4.0, 31), np.linspace(-5.0, 1.0, 41), indexing="ij")
    coarse = lift(x, y)
    x, dy = np.meshgrid(np.linspace(0.05, 0.95, 19), np.linspace(-0.15, 0.15, 31), indexing="ij")
    below = lift(x, -3.0 + dy)
    x, dy = np.meshgrid(np.linspace(-2.9, -2.0, 19), np.linspace(-0.15, 0.15, 31), indexing="ij")
    beside = lift(x, (-0.5 * x - 6.0 * np.sqrt(0.61)) / (np.sqrt(0.61) + 0.6) + dy)
    return np.concatenate([coarse, below, beside])


def corner_case(which, k, seed=0, f32=True):
    """CORNER_V3 and corner_points() in k >= 3 dimensions -> (V (6,k), faces (2,3), P (n,k)).  The 3-d coordinates are float32
    values (what the reference was run on, k = 3); for k > 3 they are turned by a rotation, and with f32=False not rounded again,
    so that the turned figure is the same figure to float64 rounding."""
    base = np.concatenate([CORNER_V3, corner_points()]).astype(np.float32).astype(np.float64)
    both = embed(base, k, 2000 * seed + k, f32) if k > 3 else base
    return both[:6], CORNER_FACES[which], both[6:]


def sha256_of(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def fixture_inputs():
    """every input of tests/golden/fx_precise_regions.npz, regenerated: name -> (V, faces, P).
    (a) the four shapes, the triangle twice, at k = 3 and k = 17;  (b) the open corner and its twin at k = 3."""
    out = {}
    for shape in SHAPES:
        for k in (3, 17):
            V, P = designed_case(shape, k)
            out[f"a_{shape}_k{k}"] = (V, np.array([[0, 1, 2], [0, 1, 2]]), P)
    for which in CORNER_FACES:
        out[f"b_{which}"] = corner_case(which, 3)
    return out


def fixture_hash(inputs):
    return sha256_of(*[x for name in sorted(inputs) for x in inputs[name]])


def face_distance(V, faces, P, fm):
    """true distance (closest_point) of every point to the face named for it"""
    return closest_point(np.asarray(V)[np.asarray(faces)[np.asarray(fm)]], P)[2]


def projected(V, faces, fm, bary):
    """the point that (face, barycentric weights) names, float64"""
    return (np.asarray(bary)[:, :, None] * np.asarray(V, np.float64)[np.asarray(faces)[np.asarray(fm)]]).sum(1)

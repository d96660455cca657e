"""The named clouds of the kNN tests: one table for tests/test_gpu_knn.py (HIP kernels against the brute-force oracle, bit for bit),
tests/test_knn_host.py (the oracle's own semantics, and numpy mutants that every wrong search must fail on) and tools/time_knn.py.

Every cloud is seeded, float32, (n, 3), and returned read-only: the tests share one instance and one oracle result per case.
`why` says which path of csrc/knn.hip the case is there for (boxes are runs of 512 curve-consecutive points, one wave tests 64 boxes
per pass of its box-group loop, one wave holds 64 queries, the first bound looks K points to either side along the curve).
"""
import functools

import numpy as np

BOX, WAVE = 512, 64


def lidar_cloud(n, seed, clustered=True):
    """LiDAR-like: an anisotropic background, and (clustered) a third of the points in dense blobs plus up to 50 exact duplicates."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 3)).astype(np.float32) * np.array([30, 5, 30], np.float32)
    if clustered:
        k = n // 3
        pts[:k] = rng.normal(size=(k, 3)).astype(np.float32) * 0.05 + rng.integers(-3, 4, size=(k, 3)).astype(np.float32)
        m = min(50, k)
        pts[k:k + m] = pts[:m]
    return pts


def _frozen(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
# self mode: fewer than K others (1..4, 10, 11), one wave +-1 (63..65), one block of 4 waves +-1 (255..257), one box +-1 (511..513),
# two boxes +-1, 64 boxes +-1 (32768, 32769: the second pass of the box-group loop starts at 32769), two full passes + 1 (65537)
SELF_SIZES = (1, 2, 3, 4, 10, 11, 12, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1025, 32768, 32769, 65537)
# reference mode (nq, nr): one query / many boxes; nr < K; one wave against one box + 1; nr < 10; a second box-group pass;
# nq > nr (the sort's temporary is sized by the larger); nq < 64 with nr = 64; nq and nr on either side of 512
REF_SIZES = ((1, 40000), (65, 2), (64, 513), (5000, 9), (4000, 32769), (33000, 700), (63, 64), (513, 512))


@functools.lru_cache(maxsize=None)
def self_cloud(n):
    return _frozen(lidar_cloud(n, 1000 + n))


@functools.lru_cache(maxsize=None)
def ref_clouds(nq, nr):
    """(query, reference); the first min(nq, nr, 20) queries sit exactly on reference points (distance 0 counts in reference mode)."""
    ref = lidar_cloud(nr, 2000 + nr)
    qry = lidar_cloud(nq, 3000 + nq)
    m = min(nq, nr, 20)
    qry[:m] = ref[:m]
    return _frozen(qry), _frozen(ref)


# ---- cloud shapes --------------------------------------------------------------------------------------------------------------
def _identical_box():
    rng = np.random.default_rng(11)
    p = np.array([1.5, -2.25, 0.75], np.float32)
    # the repeated point is the cloud's minimum corner: Morton code 0, so the 600 copies lead the curve and box 0 is 512 copies of it
    return np.concatenate([np.tile(p, (600, 1)), p + rng.uniform(0.5, 2.0, size=(20, 3)).astype(np.float32)])


def _three_points():
    rng = np.random.default_rng(12)
    pts = np.repeat(np.array([[0.25, 1.0, -3.0], [0.5, 1.0, -3.0], [7.0, -2.0, 4.0]], np.float32), 2000, axis=0)
    return pts[rng.permutation(len(pts))]


def _lattice():
    rng = np.random.default_rng(13)
    g = np.arange(17, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return pts[rng.permutation(len(pts))]


def _line():
    rng = np.random.default_rng(14)
    pts = np.empty((3000, 3), np.float32)
    pts[:, 0] = rng.normal(size=3000) * 20
    pts[:, 1], pts[:, 2] = 2.5, -7.0
    return pts


def _plane():
    rng = np.random.default_rng(15)
    pts = (rng.normal(size=(4000, 3)) * [30, 5, 1]).astype(np.float32)
    pts[:, 2] = 4.0
    return pts


def _far_outlier():
    rng = np.random.default_rng(16)
    pts = rng.normal(size=(3001, 3)).astype(np.float32)
    pts[1700] = 1e6
    return pts


def _offset_blob():
    rng = np.random.default_rng(17)
    return rng.normal(size=(3000, 3)).astype(np.float32) + np.array([1e5, -2e5, 3e4], np.float32)


def _denormal_blob():
    rng = np.random.default_rng(18)
    return (rng.normal(size=(2000, 3)) * 1e-21).astype(np.float32)


def _sub_floor_blob():
    rng = np.random.default_rng(19)
    return (rng.normal(size=(1500, 3)) * 1e-32).astype(np.float32)


SHAPES = {
    "identical_box": ("600 copies of one point + 20 others: box 0 has a zero-size AABB and every distance inside it ties at 0", _identical_box),
    "three_points_x2000": ("2000 copies each of 3 points: ties span whole boxes, the K nearest are all at distance 0", _three_points),
    "lattice_17": ("17^3 integer lattice: many exactly equal distances at the K-th place", _lattice),
    "line": ("points on an axis-parallel line: two degenerate axes in the Morton grid and in every AABB", _line),
    "plane": ("points in an axis-aligned plane: one degenerate axis", _plane),
    "far_outlier": ("unit blob + one point at 1e6: the Morton grid collapses to one cell, the box pruning alone keeps the search exact", _far_outlier),
    "offset_blob": ("unit blob at (1e5, -2e5, 3e4): coordinates quantised to 2^-7 .. 2^-6, differences exact, many ties", _offset_blob),
    "denormal_blob": ("spread 1e-21: every squared distance is a float32 denormal or 0 (a flush to zero on either side shows)", _denormal_blob),
    "sub_floor_blob": ("spread 1e-32: the extent is under knn_morton_kernel's 1e-30 floor and every squared distance underflows to 0", _sub_floor_blob),
    "lidar": ("the LiDAR-like cloud (blobs, sparse background, exact duplicates) at 5000 points", lambda: lidar_cloud(5000, 20)),
}


@functools.lru_cache(maxsize=None)
def shape_cloud(name):
    return _frozen(SHAPES[name][1]())


# ---- non-finite points ---------------------------------------------------------------------------------------------------------
# name -> (why, [(row, column or None for the whole row, value)]); rows are given for a cloud of NONFINITE_N points.  n <= 4096: an inf
# in the bounds makes every wave scan every box.
NONFINITE_N = 3000
_ROWS = (0, 1300, NONFINITE_N - 1)     # first, inside, last position of the input
NONFINITE = {
    "nan_points": ("3 all-NaN points (Morton code 0: they lead the curve, where every K-list is still empty, so even a NaN-duplicating insertion gets by; nan_y is the case that sits among real neighbours)",
                   [(r, None, np.nan) for r in _ROWS]),
    "inf_coords": ("one +inf and one -inf coordinate: infinite bounds, the Morton grid collapses on two axes, boxes with infinite AABBs",
                   [(7, 0, np.inf), (2000, 2, -np.inf)]),
    "nan_y": ("NaN only in y: the points keep their x/z place on the curve, so they sit in the middle of boxes among real neighbours",
              [(r, 1, np.nan) for r in _ROWS]),
}


def _poison(base, edits):
    pts = base.copy()
    for row, col, value in edits:
        if col is None:
            pts[row] = value
        else:
            pts[row, col] = value
    return pts, np.array(sorted({row for row, _, _ in edits}))


@functools.lru_cache(maxsize=None)
def nonfinite_self(name):
    """(cloud, rows of the non-finite points)"""
    pts, bad = _poison(lidar_cloud(NONFINITE_N, 30), NONFINITE[name][1])
    return _frozen(pts), bad


NONFINITE_NQ = 1000


@functools.lru_cache(maxsize=None)
def nonfinite_ref(name, side):
    """(query, reference, rows of the non-finite points of cloud `side`): side is "query" or "reference"."""
    ref = lidar_cloud(NONFINITE_N, 31)
    qry = lidar_cloud(NONFINITE_NQ, 32)
    qry[:20] = ref[:20]
    edits = NONFINITE[name][1]
    if side == "reference":
        ref, bad = _poison(ref, edits)
    else:
        qry, bad = _poison(qry, [(r * (NONFINITE_NQ - 1) // (NONFINITE_N - 1), c, v) for r, c, v in edits])   # first and last stay so
    return _frozen(qry), _frozen(ref), bad


# ---- references ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(kind, key, K, take_sqrt=False):
    """The brute-force oracle's result for a named case, computed once: kind in self / ref / shape / nonfinite_self / nonfinite_ref."""
    from oracle.knn_oracle import knn_mean_dist2
    if kind == "self":
        out = knn_mean_dist2(self_cloud(key), K, take_sqrt=take_sqrt)
    elif kind == "ref":
        q, r = ref_clouds(*key)
        out = knn_mean_dist2(q, K, reference=r, take_sqrt=take_sqrt)
    elif kind == "shape":
        out = knn_mean_dist2(shape_cloud(key), K, take_sqrt=take_sqrt)
    elif kind == "nonfinite_self":
        out = knn_mean_dist2(nonfinite_self(key)[0], K, take_sqrt=take_sqrt)
    else:
        q, r, _ = nonfinite_ref(*key)
        out = knn_mean_dist2(q, K, reference=r, take_sqrt=take_sqrt)
    out.setflags(write=False)
    return out


def dist2_f32(q, r):
    """[nq, nr] float32 squared distances with the kernels' and the oracle's operation order: (dx*dx + dy*dy) + dz*dz."""
    q, r = np.asarray(q, np.float32), np.asarray(r, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dx, dy, dz = (q[:, None, c] - r[None, :, c] for c in range(3))
        return (dx * dx + dy * dy) + dz * dz


def mean_of_k_smallest(d, K):
    """Rows of float32 candidates -> the oracle's reduction: candidates that are not < FLT_MAX (NaN, inf) do not count, missing ones are
    FLT_MAX, the K smallest are summed in ascending order in float32 and divided by K."""
    big = np.float32(np.finfo(np.float32).max)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = np.where(d < big, d, big).astype(np.float32)
        if d.shape[1] < K:
            d = np.concatenate([d, np.full((d.shape[0], K - d.shape[1]), big, np.float32)], axis=1)
        best = np.sort(d, axis=1)[:, :K]
        s = best[:, 0].copy()
        for k in range(1, K):
            s = s + best[:, k]
        return s / np.float32(K)


def kdtree_exact_mean_dist2(pts, K, c, idx=None):
    """Exact float32 self-mode result from a float64 KD-tree: the c nearest others of every point are re-measured in float32 with the
    kernels' operation order and the K smallest of those are averaged.  It equals the brute-force oracle wherever the float32 K nearest are
    among the float64 c nearest (c > K leaves room for float32 ties and reorderings at the K-th place)."""
    if idx is None:      # else: the [n, c + 1] neighbour indices of such a query, made by the caller
        from scipy.spatial import cKDTree
        p64 = pts.astype(np.float64)
        _, idx = cKDTree(p64).query(p64, k=c + 1, workers=-1)
    own = idx == np.arange(len(pts))[:, None]
    own[~own.any(axis=1), -1] = True      # a duplicate may have pushed the point itself out of its own list: drop the farthest then
    first = own.argmax(axis=1)
    keep = np.ones_like(own)
    keep[np.arange(len(pts)), first] = False
    nbr = idx[keep].reshape(len(pts), c)
    d = np.empty((len(pts), c), np.float32)
    for j in range(c):
        diff = pts - pts[nbr[:, j]]
        d[:, j] = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
    return mean_of_k_smallest(d, K)

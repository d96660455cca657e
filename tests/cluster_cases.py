"""The oracle and the named cases of the radius-clustering tests: one table for tests/test_gpu_cluster.py (the HIP kernels against the
oracle, label for label) and tests/test_cluster_host.py (the oracle's own semantics, and numpy mutants that every wrong clustering must
fail on).

The op (csrc/cluster.hip, streetunveiler_amd/cluster.py) returns, for every point that takes part, the smallest index of the points it is
connected to through steps with  sqrt((dx*dx + dy*dy) + dz*dz) < float32(threshold)  in float32 -- the comparison is strict -- ; -1 for a
masked-out point; its own index for an active point with a NaN / inf coordinate, which is within range of nobody, itself included.

Every case is seeded, has a few thousand points at most, and is returned read-only: the tests share one instance and one oracle result
per case.  `why` says what the case is there for (boxes are runs of 512 curve-consecutive points, one wave holds 64 queries).
"""
import functools

import numpy as np

F = np.float32
BOX, WAVE = 512, 64


# ---- oracle ----------------------------------------------------------------------------------------------------------------------
def takes_part(xyz, mask=None):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    part = np.isfinite(xyz).all(axis=1)
    return part if mask is None else part & np.asarray(mask, bool)


def adjacency(xyz, threshold, mask=None, below=None):
    """[n, n] bool: the full float32 distance matrix against float32(threshold), rows and columns of points that take no part cleared.
    `below(d2, r)` replaces the predicate (the mutants of tests/test_cluster_host.py)."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dx, dy, dz = (xyz[:, None, c] - xyz[None, :, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        adj = np.sqrt(d2) < F(threshold) if below is None else below(d2, F(threshold))
    part = takes_part(xyz, mask)
    return adj & part[:, None] & part[None, :]


def name_by_smallest_index(comp):
    """Component numbers -> the smallest index of each component."""
    comp = np.asarray(comp)
    smallest = np.full(comp.max() + 1 if len(comp) else 0, len(comp), np.int64)
    np.minimum.at(smallest, comp, np.arange(len(comp)))
    return smallest[comp]


def labels_from_adjacency(adj, xyz, mask=None):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(adj)
    labels = np.arange(n, dtype=np.int64)       # a point without a neighbour, a non-finite one among them, keeps its own index
    if n:
        labels = name_by_smallest_index(connected_components(csr_matrix(adj), directed=False)[1])
    if mask is not None:
        labels[~np.asarray(mask, bool)] = -1
    return labels


def oracle_labels(xyz, threshold, mask=None):
    return labels_from_adjacency(adjacency(xyz, threshold, mask), xyz, mask)


def partition(labels):
    """The clustering as a set of frozensets of point indices (masked-out points, label -1, left out)."""
    groups = {}
    for i, l in enumerate(np.asarray(labels).tolist()):
        if l >= 0:
            groups.setdefault(l, []).append(i)
    return {frozenset(g) for g in groups.values()}


# ---- clouds ----------------------------------------------------------------------------------------------------------------------
def _frozen(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


def uniform_cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=F)


def critical_radius(n, rng):
    """A radius around the one at which a uniform cloud of n points in the unit cube grows its giant component (0.86 n^(-1/3): at 4000
    points that is 0.0544, the middle of the three radii below), so that singletons, mid-size and large components occur together."""
    return float(F(rng.uniform(0.6, 1.1) * max(n, 1) ** (-1.0 / 3.0)))


SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 1025)


def _size_case(n):
    rng = np.random.default_rng(100 + n)
    return uniform_cloud(n, 200 + n), critical_radius(n, rng), None


def _pair(touching):
    r = 0.07
    return np.array([[0.25, 0.5, 0.75], [0.25 + (0.06 if touching else 0.08), 0.5, 0.75]], F), r, None


def _identical():
    return np.tile(np.array([1.5, -2.25, 0.75], F), (600, 1)), 0.1, None


def _chain(gap_at=None):
    r, n = 0.01, 1500
    step = np.full(n, 0.9 * r)
    step[0] = 0.0
    if gap_at is not None:
        step[gap_at] = 1.1 * r
    t = np.cumsum(step) / np.sqrt(3.0)
    pts = np.stack([t, t, t], -1).astype(F)
    return pts[np.random.default_rng(31).permutation(n)], r, None


def _lattice(threshold):
    g = np.arange(9, dtype=F) * F(0.0625)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return pts[np.random.default_rng(32).permutation(len(pts))], float(threshold), None


def _parallel_lines():
    """Two lines along x, 1.5 r apart in y, points 0.5 r apart; two lone points 250 r below and 261 r above stretch the Morton grid's y
    axis to two steps per r, so the lines fall into y cells 500 and 503: they differ in the two low y bits only and alternate along the curve."""
    r, m = 0.01, 700
    x = np.arange(m) * 0.5 * r
    a = np.stack([x, np.zeros(m), np.zeros(m)], -1)
    b = np.stack([x, np.full(m, 1.5 * r), np.zeros(m)], -1)
    ends = np.array([[0.0, -250 * r, 0.0], [0.0, 261 * r, 0.0]])
    pts = np.concatenate([a, b, ends]).astype(F)
    return pts[np.random.default_rng(33).permutation(len(pts))], r, None


UNIFORM_N = 4000
UNIFORM_RADII = (0.05, 0.0544, 0.06)


def _uniform(r, masked):
    pts = uniform_cloud(UNIFORM_N, 40)
    return pts, r, (np.random.default_rng(41).random(UNIFORM_N) < 0.5 if masked else None)


def _masked_bridge():
    """Two groups of 300 points, each in a cube of side 0.1, 1.5 r between their nearest members; the one point that is within r of both
    is masked out."""
    r, side = 0.05, 0.1
    rng = np.random.default_rng(42)
    left = rng.random((300, 3)) * side
    right = rng.random((300, 3)) * side + [side + 1.5 * r, 0, 0]
    left[0], right[0] = [side, side / 2, side / 2], [side + 1.5 * r, side / 2, side / 2]
    bridge = np.array([[side + 0.75 * r, side / 2, side / 2]])
    pts = np.concatenate([left, bridge, right]).astype(F)
    mask = np.ones(len(pts), bool)
    mask[300] = False
    perm = rng.permutation(len(pts))
    return pts[perm], r, mask[perm]


NONFINITE_ROWS = {0: (None, np.nan), 7: (0, np.inf), 700: (1, np.nan), 1301: (2, -np.inf), 2100: (None, np.inf), 2999: (None, np.nan)}


def _nonfinite(masked):
    pts = uniform_cloud(3000, 43)
    for row, (col, value) in NONFINITE_ROWS.items():
        if col is None:
            pts[row] = value
        else:
            pts[row, col] = value
    mask = np.random.default_rng(44).random(3000) < 0.6 if masked else None
    if masked:
        mask[[0, 700, 2999]] = True       # non-finite points on either side of the mask
        mask[[7, 1301]] = False
    return pts, 0.06, mask


def _far_outlier():
    pts = uniform_cloud(2001, 45)
    pts[1234] = 1e6
    return pts, 0.07, None


def _flat():
    pts = uniform_cloud(2500, 46)
    pts[:, 1] = 0.375
    return pts, 0.025, None


# sqrt(d2) < r against a pair whose squared distance is EXACTLY the smallest float32 whose root reaches r = float32(0.07): the root
# equals r, so the pair is apart -- but d2 < float32(r * r) holds, r * r being one step above.  And the pair one step nearer, which is joined.
ROOT_R = F(0.07)
ROOT_D2 = F(0.0048999996)


def _on_the_root_boundary(steps_inside):
    want = np.int32(ROOT_D2.view(np.int32) - steps_inside)      # the bits of the squared distance to hit: x fixed, y searched
    x = F(0.06)
    y0 = np.sqrt(want.view(F) - x * x)
    ys = (y0.view(np.int32) + np.arange(-64, 65)).astype(np.int32).view(F)
    d2 = (x * x + ys * ys) + F(0) * F(0)
    y = ys[np.flatnonzero(d2.view(np.int32) == want)[0]]
    return np.array([[0, 0, 0], [x, y, 0]], F), float(ROOT_R), None


CASES = {}
for _n in SIZES:
    CASES[f"size_{_n}"] = (f"{_n} uniform points at a radius around the critical one: empty / one lane / a wave, a box, two boxes, each +-1", functools.partial(_size_case, _n))
CASES.update({
    "pair_touching": ("two points 0.06 apart at radius 0.07: one component", functools.partial(_pair, True)),
    "pair_apart": ("two points 0.08 apart at radius 0.07: two components", functools.partial(_pair, False)),
    "identical_600": ("600 copies of one point: more than a box of zero-size AABBs, every pair an edge, one component", _identical),
    "chain": ("1500 points 0.9 r apart on a space diagonal, indices shuffled: one component across boxes and waves, a tree that is deep before it is flat", _chain),
    "chain_gap": ("the same chain with one step of 1.1 r: two components", functools.partial(_chain, 777)),
    "lattice_at_spacing": ("9^3 lattice of spacing 0.0625 at threshold 0.0625: the comparison is strict, 729 singletons", functools.partial(_lattice, F(0.0625))),
    "lattice_above_spacing": ("the lattice at the next float32 above 0.0625: one component", functools.partial(_lattice, np.nextafter(F(0.0625), F(1)))),
    "parallel_lines": ("two lines 1.5 r apart that alternate along the Morton curve: two components (and two lone points)", _parallel_lines),
    "masked_bridge": ("two groups whose only bridge is a masked-out point: they stay apart", _masked_bridge),
    "nonfinite": ("NaN / inf coordinates in 6 of 3000 active points: each keeps its own index, every other label is that of the cloud without them", functools.partial(_nonfinite, False)),
    "nonfinite_masked": ("the same under a mask, non-finite points on either side of it", functools.partial(_nonfinite, True)),
    "far_outlier": ("unit cloud + one point at 1e6: the Morton grid puts the whole cloud into one cell, the boxes alone keep the search exact", _far_outlier),
    "flat": ("all y equal: a degenerate axis in the Morton grid and in every AABB", _flat),
    "root_boundary_apart": ("two points whose squared distance is the smallest float32 whose root is 0.07f: apart, though d2 < float32(r * r)", functools.partial(_on_the_root_boundary, 0)),
    "root_boundary_joined": ("two points one float32 step of squared distance nearer: joined", functools.partial(_on_the_root_boundary, 1)),
})
for _r in UNIFORM_RADII:
    CASES[f"uniform_{_r}"] = (f"4000 uniform points at radius {_r}: singletons, mid-size components and (from 0.0544 up) a giant one, where hooks collide", functools.partial(_uniform, _r, False))
    CASES[f"uniform_{_r}_half_masked"] = (f"the same cloud at radius {_r} with a random half masked out", functools.partial(_uniform, _r, True))
# the cases drawn at random (tests/test_cluster_host.py evaluates the reference's torch expression on them)
RANDOM_CASES = tuple(k for k in CASES if k.startswith(("size_", "uniform_", "nonfinite", "far_outlier", "flat", "masked_bridge")))


@functools.lru_cache(maxsize=None)
def case(name):
    """(xyz float32 [n, 3], threshold, mask bool [n] or None), read-only."""
    xyz, threshold, mask = CASES[name][1]()
    return _frozen(np.asarray(xyz, F).reshape(-1, 3), F), float(threshold), None if mask is None else _frozen(mask, bool)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle's labels of a named case, computed once."""
    out = oracle_labels(*case(name))
    out.setflags(write=False)
    return out

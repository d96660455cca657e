"""The cases and the bars of the LiDAR colouring and labelling (streetunveiler_amd/lidar_label.py), shared by tests/test_lidar_label_host.py
(CPU) and tests/test_gpu_lidar_label.py.  Small: the kernels can go wrong at edges, not at size.

Shapes: N in {0, 1, 63, 64, 65, 4097}; S in {1, 3} with the middle sweep empty; C in {1, 3, 32}; V in {1, 3, 70} for the vote; views of
1x1, 1x17, 17x1, 21x21 and 48x64 in one call; r in {1, 3, 10} and r = 100, larger than every picture (no corner valid, everything certain);
maps constant, in stripes two columns wide (so that the wrapped fourth column differs from l0), in 8x8 blocks and random; a non-identity
label_lut over raw bytes 0..255; float32 and float64 points; NaN and inf rows; a cloud no view sees; points seen by 0, 1 and all cameras
of a sweep whose maps disagree; vote ties and a label >= n_classes; a world offset of 2^20 m (1.05e6).

PLANTED ROWS.  Cameras A and B have an axis permutation as rotation, a dyadic translation, focal length 16 and the principal point at the
picture's centre (B's K has the projective last row (4, 0, 1), so that a point with cam.z == 0 has a finite pix and z > 0 alone decides it).
Planted points lie at cam.z == 2 with dyadic coordinates of few bits, so every float64 operation on them is exact in any order, fused or
not, in every A or B view (all of them share the pose): pix == 0, == w, == h, z == 0, integer pixels and fractions of .75, every
combination of u and v in {0, r-1, r, r+1, w-1-r, w-r, w-1} (u-r == 0 and == 1, u+r == w-1 and == w, the wrapping fourth corner u < r
with v+r < h, u+r < w) and, where N allows, a point in every pixel of the 48x64 and the 21x21 picture.

RANDOM ROWS.  A decision is robust when the float64 checker decides the same with every intermediate moved by its forward-error bound,
the bound of tests/unveil_cases.py with u = 2^-53 (Higham, section 3.1: gamma_n = n u / (1 - n u); cam: gamma_4, p: gamma_3 on the perturbed
cam, pix: one more rounding; trunc(pix) must not change within the bound).  The trunc of a random pixel is unstable within that bound with
probability about 1e-9, so a case must have NO non-robust (point, view) pair outside the planted ones: tests/test_lidar_label_host.py asserts
it.  Everything is then compared exactly: xyz and rgb bit for bit, labels, index, order, rows_per_sweep, valid_mask and tag."""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np
import torch

from streetunveiler_amd import lidar_label as LL

U64 = 2.0 ** -53
R_PERM = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])      # cam = (y, z, x) + t
T_DYADIC = np.array([0.5, -0.25, 1.0])
FOCAL = 16.0
OFFSET = np.array([2.0 ** 20, -(2.0 ** 20), 2.0 ** 19])
SIZES = ((48, 64), (21, 21), (1, 1), (1, 17), (17, 1))                      # (h, w)
MAP_KINDS = ("constant", "stripes", "blocks", "random")
N_CLASSES = 6


def _gamma(n):
    return n * U64 / (1 - n * U64)


# ---- views --------------------------------------------------------------------------------------------------------------------------------
def _K(kind, h, w, rng):
    if kind == "G":
        return np.array([[0.83 * w + rng.random(), 0.0, 0.5 * w + rng.normal()], [0.0, 0.79 * w + rng.random(), 0.5 * h + rng.normal()], [0.0, 0.0, 1.0]])
    return np.array([[FOCAL, 0.0, w / 2], [0.0, FOCAL, h / 2], [4.0 if kind == "B" else 0.0, 0.0, 1.0]])


def _nearby_rotation(rng):
    """a general rotation a few degrees off A's and B's, so that the three frusta overlap and a point can be seen by all cameras of a sweep"""
    q = np.concatenate([[1.0], rng.normal(size=3) * 0.03])
    r, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]]) @ R_PERM


def _w2c(R, t, offset):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t - R @ offset       # cam = R (x - offset) + t; exact for the permutation and the dyadic offset
    return m


def label_map(kind, h, w, rng, raw=False):
    """uint8 [h,w]: labels 0..5, or -- raw -- bytes 0..255 for a lut to fold"""
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if kind == "constant":
        m = np.full((h, w), int(rng.integers(N_CLASSES)))
    elif kind == "stripes":
        m = (cols // 2 + int(rng.integers(N_CLASSES))) % N_CLASSES
    elif kind == "blocks":
        m = (rows // 8 * 3 + cols // 8 + int(rng.integers(N_CLASSES))) % N_CLASSES
    else:
        m = rng.integers(0, N_CLASSES, size=(h, w))
    if raw:
        m = m + N_CLASSES * rng.integers(0, 42, size=(h, w))      # 0..251; lut: byte % 6
    return m.astype(np.uint8)


LUT = (np.arange(256) % N_CLASSES).astype(np.uint8)


def to_world(cam_points, R, t, offset):
    return (np.asarray(cam_points, np.float64) - t) @ R + offset      # R^T (cam - t) + offset, row-wise


def _edge_values(size, r):
    return sorted({x for x in (0, r - 1, r, r + 1, size - 1 - r, size - r, size - 1) if 0 <= x < size})


def planted_pixels(h, w, r, every_pixel):
    """the (pix.x, pix.y) targets in an A view of (h, w): one inside first, the borders, the corner-validity edges, then every pixel"""
    t = [(w // 2, h // 2), (0.0, h / 2), (float(w), h / 2), (w / 2, 0.0), (w / 2, float(h)), (w // 2 + 0.75, h // 2 + 0.75)]
    t += [(u + 0.75, v + 0.25) for v in _edge_values(h, r) for u in _edge_values(w, r)]
    if every_pixel:
        t += [(u + 0.25, v + 0.75) for v in range(h) for u in range(w)]
    return t


def _cam_of_pixel(pu, pv, h, w, z=2.0):
    return [(pu - w / 2) * z / FOCAL, (pv - h / 2) * z / FOCAL, z]


PLANTED_B = [[0.25, 0.25, 0.0],                 # z == 0 with p = (4 + w/2 . 0, ..): pix finite and inside, out by z > 0 alone
             [0.25, 0.25, 2.0 ** -10],          # one step in front: in
             [0.125, 0.25, 0.5]]
SPECIAL = [[np.nan, 0.0, 1.0], [0.5, np.inf, 0.25], [-np.inf, 0.0, 0.0], [np.inf, np.inf, np.inf]]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    op: str                       # "merge", "per_view" or "vote"
    points: np.ndarray            # [N,3] float32 or float64, read-only
    sweep_offsets: np.ndarray     # [S+1] int64 (vote: [0, N])
    views: LL.LabelViews          # CPU pictures
    cameras: int                  # C (vote: V)
    check_range: int
    fourth_corner: str
    exact_rows: np.ndarray        # [N] bool: planted (exact in every A and B view) or NaN / inf
    view_kinds: tuple             # per view "A", "B" or "G"
    raises: bool                  # vote: a label >= n_classes


def _spec(op, N, S=1, views=(("A", 48, 64, "constant"),), r=10, dtype="f64", offset=False, lut=False, fourth="reference", unseen=False, bad_label=False):
    return dict(op=op, N=N, S=S, views=tuple(views), r=r, dtype=dtype, offset=offset, lut=lut, fourth=fourth, unseen=unseen, bad_label=bad_label)


_THREE = (("A", 48, 64, "blocks"), ("B", 21, 21, "constant"), ("G", 48, 64, "blocks"))
_MANY = tuple((("A", "B", "G", "A")[k % 4], *SIZES[k % 5], MAP_KINDS[k % 4]) for k in range(32))
_SEVENTY = tuple((("A", "G", "B", "A", "G")[k % 5], *SIZES[(k * 3) % 5], MAP_KINDS[(k + k // 4) % 4]) for k in range(70))
SPECS = {
    **{f"merge_N{N}_S1_C1_r10": _spec("merge", N, views=(("A", 48, 64, "constant" if N != 4097 else "stripes"),)) for N in (0, 1, 63, 64, 65, 4097)},
    "merge_N65_S1_C1_B_r3": _spec("merge", 65, views=(("B", 21, 21, "constant"),), r=3),
    "merge_N65_S3_C3_r3": _spec("merge", 65, S=3, views=_THREE, r=3),
    "merge_N4097_S3_C3_r1_f32": _spec("merge", 4097, S=3, views=_THREE, r=1, dtype="f32"),
    "merge_N4097_S3_C3_r3_offset": _spec("merge", 4097, S=3, views=_THREE, r=3, offset=True),
    "merge_N4097_S1_C32_r3": _spec("merge", 4097, views=_MANY, r=3),
    "merge_N4097_S1_C3_r100": _spec("merge", 4097, views=_THREE, r=100),
    "merge_N4097_S1_C3_r3_lut": _spec("merge", 4097, views=_THREE, r=3, lut=True),
    "merge_N4097_S1_C1_r10_mirrored": _spec("merge", 4097, views=(("A", 48, 64, "stripes"),), fourth="mirrored"),
    "merge_N65_S3_C3_unseen": _spec("merge", 65, S=3, views=_THREE, r=3, unseen=True),
    "per_view_N0_S1_C3": _spec("per_view", 0, views=_THREE, r=3),
    "per_view_N65_S1_C1_r1": _spec("per_view", 65, views=(("A", 21, 21, "blocks"),), r=1),
    "per_view_N4097_S3_C3_r3": _spec("per_view", 4097, S=3, views=_THREE, r=3),
    "per_view_N64_S3_C32_r10_f32": _spec("per_view", 64, S=3, views=_MANY, r=10, dtype="f32"),
    "vote_N0_V1": _spec("vote", 0),
    "vote_N1_V1": _spec("vote", 1),
    "vote_N63_V3": _spec("vote", 63, views=_THREE),
    "vote_N64_V3_f32": _spec("vote", 64, views=_THREE, dtype="f32"),
    "vote_N65_V70": _spec("vote", 65, views=_SEVENTY),
    "vote_N4097_V3_offset_lut": _spec("vote", 4097, views=_THREE, offset=True, lut=True),
    "vote_N4097_V70": _spec("vote", 4097, views=_SEVENTY),
    "vote_N4097_V2_ties": _spec("vote", 4097, views=(("A", 48, 64, "constant"), ("A", 48, 64, "constant"))),
    "vote_N65_V3_unseen": _spec("vote", 65, views=_THREE, unseen=True),
    "vote_N65_V3_bad_label": _spec("vote", 65, views=_THREE, bad_label=True),
}
NAMES = tuple(SPECS)
SWEEP_NAMES = tuple(n for n in NAMES if SPECS[n]["op"] != "vote")
VOTE_NAMES = tuple(n for n in NAMES if SPECS[n]["op"] == "vote")


@functools.lru_cache(maxsize=None)
def case(name):
    sp = SPECS[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    vote = sp["op"] == "vote"
    N, S, C, r = sp["N"], sp["S"], len(sp["views"]), sp["r"]
    offset = OFFSET if sp["offset"] else np.zeros(3)
    n_groups = 1 if vote else S                    # a group: the views one point goes through
    cams, images, maps, kinds = [], [], [], []
    for s in range(n_groups):
        for k, (kind, h, w, map_kind) in enumerate(sp["views"]):
            R, t = (_nearby_rotation(rng), T_DYADIC + rng.normal(size=3) * 0.05) if kind == "G" else (R_PERM, T_DYADIC)
            cams.append((R, t, _K(kind, h, w, rng), h, w))
            kinds.append(kind)
            images.append(rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8))
            m = label_map(map_kind, h, w, rng, raw=sp["lut"])
            if name.endswith("_ties"):             # two equal views, constant 4 then constant 2: every seen point ties, class 2 wins
                m[:] = (4, 2)[k]
            if sp["bad_label"] and k == 0:
                m[h // 4:, :] = N_CLASSES
            maps.append(m)
    views = LL.LabelViews(np.stack([_w2c(R, t, offset) for R, t, _, _, _ in cams]), np.stack([c[2] for c in cams]), [(c[3], c[4]) for c in cams],
                          None if vote else images, maps, LUT if sp["lut"] else None)
    # the sweeps: the middle one of three is empty
    if vote or S == 1:
        offsets = np.array([0, N], dtype=np.int64)
    else:
        offsets = np.array([0, N // 2, N // 2, N], dtype=np.int64)
    rows, exact = [], []
    for s in range(n_groups):
        n_s = int(offsets[s + 1] - offsets[s])
        group = cams[s * C:(s + 1) * C]
        block, block_exact = [], []
        if not sp["unseen"]:
            for k, (kind, h, w, _) in enumerate(sp["views"][:2]):      # plant for the first A and the first B view among the first two
                if kind == "A":
                    cam_rows = [_cam_of_pixel(pu, pv, h, w) for pu, pv in planted_pixels(h, w, r, every_pixel=n_s >= 3500)]
                elif kind == "B":
                    cam_rows = PLANTED_B
                else:
                    continue
                block += list(to_world(cam_rows, R_PERM, T_DYADIC, offset))
                block_exact += [True] * len(cam_rows)
        if n_s > 8:
            block, block_exact = block[:n_s - 4] + [list(x) for x in SPECIAL], block_exact[:n_s - 4] + [True] * 4
        block, block_exact = block[:n_s], block_exact[:n_s]

        def random_row():
            R, t, K, h, w = group[rng.integers(len(group))]
            z = -rng.uniform(0.5, 5.0) if sp["unseen"] else rng.uniform(-2.0, 12.0)
            pixel = np.array([rng.uniform(-0.2 * w, 1.2 * w), rng.uniform(-0.2 * h, 1.2 * h), 1.0])
            return to_world((np.linalg.solve(K, pixel) * z)[None], R, t, offset)[0]

        def seen(row):                             # by a view of the group, in the dtype the case stores
            p = np.asarray(row, np.float64)[None].astype(np.float32 if sp["dtype"] == "f32" else np.float64)
            return any(LL.in_frame_numpy(h, w, p, _w2c(R, t, offset), K)[0][0] for R, t, K, h, w in group)

        while len(block) < n_s:
            row = random_row()
            while sp["unseen"] and seen(row):      # behind one camera is not yet outside the others
                row = random_row()
            block.append(row)
            block_exact.append(False)
        rows += block
        exact += block_exact
    points = np.asarray(rows, dtype=np.float64).reshape(N, 3).astype(np.float32 if sp["dtype"] == "f32" else np.float64)
    exact = np.asarray(exact, dtype=bool).reshape(N)
    points.setflags(write=False)
    return Case(name, sp["op"], points, offsets, views, C, r, sp["fourth"], exact, tuple(kinds), sp["bad_label"])


def groups(c):
    """[(first point, last point + 1, first view, last view + 1)]: the views each run of points goes through"""
    if c.op == "vote":
        return [(0, len(c.points), 0, len(c.views))]
    return [(int(c.sweep_offsets[s]), int(c.sweep_offsets[s + 1]), s * c.cameras, (s + 1) * c.cameras) for s in range(len(c.sweep_offsets) - 1)]


def robustness(xyz, w2c, K, h, w):
    """[n] bool: the decisions on every point in this view survive the forward-error bound of the module's docstring"""
    x = np.asarray(xyz, np.float64)
    R, t = w2c[:3, :3], w2c[:3, 3]
    with np.errstate(all="ignore"):
        cam = x @ R.T + t
        dc = _gamma(4) * (np.abs(x) @ np.abs(R).T + np.abs(t))
        p = cam @ K.T
        dp = dc @ np.abs(K).T + _gamma(3) * ((np.abs(cam) + dc) @ np.abs(K).T)
        pix = p[:, :2] / p[:, 2:3]
        B = (dp[:, :2] + np.abs(pix) * dp[:, 2:3]) / (np.abs(p[:, 2:3]) - dp[:, 2:3]) + 2 * U64 * np.abs(pix)
        B = np.where(np.abs(p[:, 2:3]) > dp[:, 2:3], B, np.inf)
        far = lambda v, edge, bound: np.abs(v - edge) > bound
        ok = far(pix[:, 0], 0, B[:, 0]) & far(pix[:, 0], w, B[:, 0]) & far(pix[:, 1], 0, B[:, 1]) & far(pix[:, 1], h, B[:, 1]) & far(cam[:, 2], 0, dc[:, 2])
        admitted = (pix[:, 0] > 0) & (pix[:, 0] < w) & (pix[:, 1] > 0) & (pix[:, 1] < h) & (cam[:, 2] > 0)
        ok &= ~admitted | (np.floor(pix - B) == np.floor(pix + B)).all(axis=1)
        ok &= np.isfinite(B).all(axis=1)
    return np.where(np.isfinite(x).all(axis=1), ok, True)      # a NaN or infinite row is in no view for everyone


def non_robust_pairs(c):
    """the number of (point, view) pairs of the case whose decision is neither exact by construction nor robust by the bound"""
    bad = 0
    for a, b, f0, f1 in groups(c):
        for f in range(f0, f1):
            ok = robustness(c.points[a:b], c.views.w2c[f], c.views.K[f], int(c.views.hw[f, 0]), int(c.views.hw[f, 1]))
            if c.view_kinds[f] != "G":
                ok |= c.exact_rows[a:b]
            bad += int((~ok).sum())
    return bad


# ---- the expectation and the bar ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(name):
    """the checkers of the library on the case -> dict of read-only numpy arrays (vote with a bad label: {})"""
    c = case(name)
    if c.op == "vote":
        if c.raises:
            return {}
        xyz, tag, valid = LL.vote_semantics_numpy(c.points, c.views, N_CLASSES)
        out = {"xyz": xyz, "tag": tag, "valid_mask": valid}
    else:
        out = LL.label_sweeps_numpy(c.points, c.sweep_offsets, c.views, c.cameras, c.op, c.check_range, c.fourth_corner)
    for a in out.values():
        a.setflags(write=False)
    return out


DTYPES = {"rgb": np.float64, "semantics": np.int32, "index": np.int64, "rows_per_sweep": np.int32, "tag": np.int32, "valid_mask": np.bool_}


def compare(name, got, label):
    """`got`: dict of arrays under the expectation's keys.  Everything exactly: shapes, dtypes, xyz and rgb bit for bit, the order."""
    want = expected(name)
    assert sorted(got) == sorted(want), (label, name, sorted(got))
    for key, w in want.items():
        g = np.asarray(got[key])
        assert g.dtype == (DTYPES.get(key) or case(name).points.dtype) and g.shape == w.shape, (label, name, key, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), f"{label} {name}: {key} differs" + (f" in {int((g != w).sum())} entries" if g.dtype.kind in "iub" else "")


def device_views(c, device):
    """the case's views with the pictures resident on `device`"""
    v = c.views
    up = lambda pictures: None if pictures is None else [p.to(device) for p in pictures]
    return LL.LabelViews(v.w2c, v.K, v.hw, up(v.images), up(v.maps), v.label_lut)


def points_tensor(c, device="cpu"):
    return torch.from_numpy(c.points.copy()).to(device)


# ---- a second statement of the three operations, with one flaw switched on: what the bars must reject ---------------------------------
FLAWS = ("le_w", "ge_x0", "le_h", "ge_y0", "ge_z0", "round", "corner_ge0", "mirrored", "clamped", "first_camera", "uncertain_means", "last_max",
         "point_major", "float32")


def _hits(c, f, xyz, flaw):
    """-> (rows inside [m], u [m], v [m], certain [m]) of view f"""
    h, w = int(c.views.hw[f, 0]), int(c.views.hw[f, 1])
    if flaw == "float32":
        x32, R, K = xyz.astype(np.float32), c.views.w2c[f].astype(np.float32), c.views.K[f].astype(np.float32)
        with np.errstate(all="ignore"):            # the inputs rounded to float32 and float32 operations
            cam = [((R[i, 0] * x32[:, 0] + R[i, 1] * x32[:, 1]) + R[i, 2] * x32[:, 2]) + R[i, 3] for i in range(3)]
            q = [(K[i, 0] * cam[0] + K[i, 1] * cam[1]) + K[i, 2] * cam[2] for i in range(3)]
            pix, z = np.stack([q[0] / q[2], q[1] / q[2]], axis=1).astype(np.float64), cam[2].astype(np.float64)
    else:
        pix, z = LL.project_numpy(xyz, c.views.w2c[f], c.views.K[f])
    lt = lambda a, b, loose: (a <= b) if loose else (a < b)
    with np.errstate(invalid="ignore"):
        mask = lt(pix[:, 0], w, flaw == "le_w") & lt(0, pix[:, 0], flaw == "ge_x0") & lt(pix[:, 1], h, flaw == "le_h") & lt(0, pix[:, 1], flaw == "ge_y0") & \
            lt(0, z, flaw == "ge_z0") & np.isfinite(pix).all(axis=1)
    whole = np.round(pix[mask]) if flaw == "round" else np.trunc(pix[mask])
    u, v = np.clip(whole[:, 0], 0, w - 1).astype(np.int64), np.clip(whole[:, 1], 0, h - 1).astype(np.int64)      # (a flawed index is kept inside the picture)
    m = c.views.map_numpy(f)
    r = c.check_range
    top, bottom, left, right = v - r, v + r, u - r, u + r
    low = (lambda a: a >= 0) if flaw == "corner_ge0" else (lambda a: a > 0)
    fourth = right if (c.fourth_corner == "mirrored") != (flaw == "mirrored") else left
    if flaw == "clamped":
        fourth = np.maximum(left, 0)
    certain = np.ones(len(u), dtype=bool)
    for rows, row_ok, cols, col_ok in ((top, low(top), left, low(left)), (top, low(top), right, right < w), (bottom, bottom < h, left, low(left)),
                                       (bottom, bottom < h, fourth, right < w)):
        ok = row_ok & col_ok
        certain[ok] &= m[rows[ok], cols[ok]] == m[v[ok], u[ok]]
    return np.flatnonzero(mask), u, v, certain


def restated(name, flaw=None):
    """the case through this module's own statement of its operation (flaw=None must equal the library's checker: the host test asserts it)"""
    c = case(name)
    pts = c.points
    if c.op == "vote":
        hits, seen = np.zeros((len(pts), N_CLASSES), dtype=np.int64), np.zeros(len(pts), dtype=bool)
        for f in range(len(c.views)):
            rows, u, v, _ = _hits(c, f, pts, flaw)
            np.add.at(hits, (rows, c.views.map_numpy(f)[v, u].astype(np.int64)), 1)
            seen[rows] = True
        tag = (N_CLASSES - 1 - np.argmax(hits[seen][:, ::-1], axis=1)) if flaw == "last_max" else np.argmax(hits[seen], axis=1)
        return {"xyz": pts[seen], "tag": tag.astype(np.int32), "valid_mask": seen}
    out = []                                       # (sweep, camera, point index, r, g, b, count, label) rows
    rows_per_sweep = []
    for s, (a, b, f0, f1) in enumerate(groups(c)):
        sums, count, label = np.zeros((b - a, 3)), np.zeros(b - a), np.full(b - a, -1, dtype=np.int64)
        certain_count = np.zeros(b - a)
        before = len(out)
        for f in range(f0, f1):
            rows, u, v, certain = _hits(c, f, pts[a:b], flaw)
            colour, lab = c.views.images[f].numpy()[v, u].astype(np.float64), c.views.map_numpy(f)[v, u].astype(np.int64)
            if c.op == "per_view":
                out += [(s, f - f0, a + i, *colour[k], 1.0, lab[k]) for k, i in enumerate(rows) if certain[k]]
                continue
            add = np.ones(len(rows), dtype=bool) if flaw == "uncertain_means" else certain
            sums[rows[add]] += colour[add]
            count[rows[add]] += 1
            certain_count[rows[certain]] += 1
            write = certain & (label[rows] < 0) if flaw == "first_camera" else certain
            label[rows[write]] = lab[write]
        if c.op == "merge":
            out += [(s, 0, a + i, *sums[i], count[i], label[i]) for i in np.flatnonzero(certain_count > 0)]
        rows_per_sweep.append(len(out) - before)
    if flaw == "point_major":
        out.sort(key=lambda row: (row[0], row[2], row[1]))
    table = np.asarray(out, dtype=np.float64).reshape(-1, 8)
    index = table[:, 2].astype(np.int64)
    return {"xyz": pts[index], "rgb": table[:, 3:6] / table[:, 6:7], "semantics": table[:, 7].astype(np.int32), "index": index,
            "rows_per_sweep": np.asarray(rows_per_sweep, dtype=np.int32)}

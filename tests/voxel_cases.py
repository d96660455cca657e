"""The cases and the bars of the LiDAR voxel downsample (streetunveiler_amd/voxel.py), shared by tests/test_voxel_host.py (the bars
reject wrong implementations; the checker against the reference's class) and tests/test_gpu_voxel.py (csrc/voxel.hip under the bars).

The bars (compare):
  exact      the voxel index of every output row, the row order, the member counts, the labels, the keep decisions and m, integer for
             integer against voxel_down_sample_torch run on the CPU in the input's dtype.  The predicate is the same IEEE expression on both
             sides (one subtraction, one division, a truncation), so no point is left out.
  means      every component within ONE float32 ulp of the largest |value| of that component among the voxel's members, against the means
             of the float64 checker (not rounded to float32).  Derivation: rounding the mean once to float32 costs at most half an ulp of
             the mean, |mean| <= the largest |member|; a float64 sum of n members is off by at most n 2^-53 of the sum of |members|, and its
             quotient by one more 2^-53 -- for the 5 000 members of the heaviest voxel here 2^-40 of the largest member, against 2^-24 for
             the half ulp.  The factor of two is the margin.
The block sizes the cases straddle are the code's: radix_sort.hip kRsTile = 2048 items a sort block, launch.h kScanInPlaceChunk = 4096 words a
scan chunk, kVoxelHeavy = 128 members from which a voxel gets a wave, voxel.hip kVoxelBoundChunk = 2048 points a bounds block."""
import functools

import numpy as np
import torch

from streetunveiler_amd import voxel as V

SORT_BLOCK, SCAN_CHUNK, HEAVY = 2048, 4096, 128


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def _case(name, points, voxel_size, colors=None, normals=None, semantics=None):
    return {"name": name, "points": points, "voxel_size": voxel_size, "colors": colors, "normals": normals, "semantics": semantics}


def _attrs(r, n, dtype=np.float32):
    normals = r.normal(size=(n, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return r.random((n, 3)).astype(dtype), normals.astype(dtype)


def _own_voxels(n, dtype=np.float32):
    """n points, each in a voxel of its own: the centres of a 3-D lattice of 0.5 m cells, shuffled."""
    side = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    pts = ((g + 0.5) * 0.5).astype(dtype)
    return pts[_rng(n).permutation(n)]


def _face_points():
    """Points exactly on voxel faces: voxel_size 0.25 and coordinates min + (j + 0.5) 0.25, so (p - lo) / v = j + 1 exactly."""
    r = _rng(11)
    j = r.integers(0, 12, size=(600, 3))
    pts = (np.float32(-1.5) + (j + 0.5).astype(np.float32) * np.float32(0.25)).astype(np.float32)
    pts[0] = np.float32(-1.5)                            # the minimum itself
    return pts


def _reciprocal_trap():
    """float32 points at voxel_size 0.1 for which trunc((p - lo) / v) and trunc((p - lo) * (1 / v)) differ: what stock torch computes on
    a GPU for `tensor / python_scalar` is not the contract."""
    v = np.float32(0.1)
    lo = np.float32(0.0) - np.float32(0.1 * 0.5)
    r = _rng(5)
    k = r.integers(1, 4000, size=400000).astype(np.float32)
    cand = (k * v + lo).astype(np.float32)               # near a face
    cand = np.concatenate([cand, np.nextafter(cand, np.float32(np.inf)), np.nextafter(cand, np.float32(-np.inf))])
    d = (cand - lo).astype(np.float32)
    differ = np.trunc(d / v) != np.trunc(d * (np.float32(1.0) / v))
    x = np.unique(cand[differ])[:300]
    assert x.size >= 50, "no float32 value separates the division from the reciprocal product"
    pts = np.zeros((x.size + 1, 3), np.float32)          # the first point is the minimum of every axis: lo is as assumed
    pts[1:, 0] = x
    pts[1:, 1] = r.random(x.size).astype(np.float32) * 3
    pts[1:, 2] = r.random(x.size).astype(np.float32) * 3
    assert (pts[1:] >= 0).all()
    return pts


def _label_shares():
    """One voxel per rule: 4/5 and 8/10 kept, 3/4 and 7/9 dropped, a 1/1 tie of two dropped, a single label kept; labels 0 and 255."""
    groups = [([255] * 4 + [0], True), ([0] * 8 + [255, 7], True), ([3] * 3 + [4], False), ([9] * 7 + [1, 2], False), ([5, 6], False), ([255], True),
              ([0], True), ([2, 2, 2], True)]
    r = _rng(3)
    pts, sem = [], []
    for g, (labels, _) in enumerate(groups):
        centre = np.array([g * 1.0 + 0.5, 0.5, 0.5])
        pts.append(centre + (r.random((len(labels), 3)) - 0.5) * 0.3)
        sem.append(r.permutation(np.array(labels)))
    return np.concatenate(pts).astype(np.float32), np.concatenate(sem).astype(np.int32), [k for _, k in groups]


def _heavy_threshold():
    """Voxels of HEAVY - 1, HEAVY, HEAVY + 1 and HEAVY + 2 members at a share of just 4/5 (kept), two more one member short of it
    (dropped).  A point at the origin anchors the lattice: lo = -0.5, so the voxel of integer coordinates k covers [k - 0.5, k + 0.5)."""
    r = _rng(17)
    pts, sem = [np.zeros((1, 3))], [np.array([0])]
    for g, n in enumerate([HEAVY - 1, HEAVY, HEAVY + 1, HEAVY + 2, HEAVY + 1, HEAVY + 2]):
        centre = np.array([2.0, 2.0 * g + 2.0, 2.0])
        pts.append(centre + (r.random((n, 3)) - 0.5) * 0.8)
        major = -(-4 * n // 5) if g < 4 else -(-4 * n // 5) - 1      # ceil(4 n / 5): kept; one fewer: dropped
        sem.append(r.permutation(np.array([g] * major + [200 + g] * (n - major))))
    return np.concatenate(pts).astype(np.float32), np.concatenate(sem).astype(np.int32)


def _mix(n=20000):
    """A uniform part and a tightly clustered part (voxels of hundreds of members), 4 labels by region with a noisy border."""
    r = _rng(23)
    uni = r.random((n // 2, 3)) * np.array([12.0, 12.0, 3.0])
    clu = np.array([6.0, 6.0, 1.5]) + r.normal(size=(n - n // 2, 3)) * 0.08
    pts = np.concatenate([uni, clu])
    sem = (pts[:, 0] > 6).astype(np.int64) * 2 + (pts[:, 1] > 6).astype(np.int64)
    noisy = r.random(n) < 0.1
    sem[noisy] = r.integers(0, 4, size=int(noisy.sum()))
    order = r.permutation(n)
    return pts[order], sem[order]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    r = _rng(1)
    out.append(_case("n0", np.zeros((0, 3), np.float32), 0.1, np.zeros((0, 3), np.float32), None, np.zeros((0,), np.int32)))
    c, nrm = _attrs(r, 1)
    out.append(_case("n1", np.array([[1.5, -2.0, 3.0]], np.float32), 0.1, c, nrm, np.array([7], np.int32)))
    c, nrm = _attrs(r, 300)
    out.append(_case("identical", np.tile(np.array([[3.25, -1.0, 0.125]], np.float32), (300, 1)), 0.2, c, nrm, np.full((300,), 4, np.int32)))
    c, nrm = _attrs(r, 5000)
    sem = np.where(np.arange(5000) < 4100, 3, 8).astype(np.int32)[r.permutation(5000)]
    out.append(_case("one_voxel_5000", (np.array([37.0, -12.0, 2.0]) + r.random((5000, 3)) * 0.04).astype(np.float32), 0.1, c, nrm, sem))
    for n in (SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1):
        c, _ = _attrs(r, n)
        out.append(_case(f"own_voxel_{n}", _own_voxels(n), 0.5, c, None, (np.arange(n) % 5).astype(np.int32)))
    out.append(_case("faces", _face_points(), 0.25, None, None, None))
    out.append(_case("reciprocal_trap", _reciprocal_trap(), 0.1, None, None, None))
    c, nrm = _attrs(r, 1500)
    out.append(_case("negative", (r.random((1500, 3)) * 8 - 9).astype(np.float32), 0.3, c, nrm, r.integers(0, 3, 1500).astype(np.int32)))
    far = np.array([10000.0, -10000.0, 50.0]) + (r.random((3000, 3)) - 0.5) * np.array([40.0, 40.0, 6.0])
    for dtype in (np.float32, np.float64):
        c, _ = _attrs(r, 3000, dtype)
        out.append(_case(f"far_10km_{np.dtype(dtype).name}", far.astype(dtype), 0.1, c, None, (far[:, 0] > 10000).astype(np.int32)))
    two = np.concatenate([r.random((1000, 3)) * 2.0, 300.0 + r.random((1000, 3)) * 2.0])
    out.append(_case("two_clusters_300m", two.astype(np.float32), 0.1, None, None, r.integers(0, 2, 2000).astype(np.int32)))
    pts, sem, _ = _label_shares()
    out.append(_case("label_shares", pts, 1.0, None, None, sem))
    pts, sem = _heavy_threshold()
    c, nrm = _attrs(r, pts.shape[0], np.float64)
    out.append(_case("heavy_threshold", pts, 1.0, c, nrm, sem))
    base = (r.random((500, 3)) * 3).astype(np.float32)
    c, nrm = _attrs(r, 500)
    sem = r.integers(0, 2, 500)
    for k in range(8):
        out.append(_case(f"absent_{k}", base, 0.4, c if k & 1 else None, nrm if k & 2 else None,
                         sem.astype([np.int32, np.int64, np.uint8, np.int16][k - 4]) if k & 4 else None))
    pts, sem = _mix()
    c, nrm = _attrs(r, pts.shape[0])
    out.append(_case("mix_20000_f32", pts.astype(np.float32), 0.1, c, nrm, sem))
    out.append(_case("mix_20000_f64", pts.astype(np.float64), 0.1, c.astype(np.float64), nrm, sem.astype(np.int32)))
    return out


def case(name):
    return next(c for c in cases() if c["name"] == name)


NAMES = [c["name"] for c in cases()]
LABEL_SHARES_KEPT = _label_shares()[2]


def refusals():
    """(name, kwargs of voxel_down_sample as numpy arrays, exception fragment)."""
    r = _rng(2)
    pts = (r.random((50, 3)) * 2).astype(np.float32)
    sem = r.integers(0, 3, 50).astype(np.int32)

    def with_point(i, value):
        p = pts.copy()
        p[i, 1] = value
        return p

    def with_label(value, dtype=np.int32):
        s = sem.astype(dtype)
        s[7] = value
        return s
    wide = pts.copy()
    wide[0, 0] = 3.0e5                                    # 300 km at 0.1 m: offset about 3 000 000 >= 2^21
    return [("label_256", dict(points=pts, voxel_size=0.1, semantics=with_label(256)), "outside 0..255"),
            ("label_minus_1", dict(points=pts, voxel_size=0.1, semantics=with_label(-1)), "outside 0..255"),
            ("label_2_pow_32", dict(points=pts, voxel_size=0.1, semantics=with_label(1 << 32, np.int64)), "outside 0..255"),
            ("nan", dict(points=with_point(3, np.nan), voxel_size=0.1), "NaN or infinite"),
            ("inf", dict(points=with_point(49, np.inf), voxel_size=0.1), "NaN or infinite"),
            ("minus_inf", dict(points=with_point(0, -np.inf), voxel_size=0.1), "NaN or infinite"),
            ("offset", dict(points=wide, voxel_size=0.1), "2\\*\\*21"),
            ("voxel_size_0", dict(points=pts, voxel_size=0.0), "positive and finite"),
            ("voxel_size_negative", dict(points=pts, voxel_size=-0.1), "positive and finite"),
            ("voxel_size_nan", dict(points=pts, voxel_size=float("nan")), "positive and finite"),
            ("rows_colors", dict(points=pts, voxel_size=0.1, colors=pts[:49]), "rows"),
            ("rows_normals", dict(points=pts, voxel_size=0.1, normals=pts[:10]), "rows"),
            ("rows_semantics", dict(points=pts, voxel_size=0.1, semantics=sem[:49]), "rows")]


# ---- the expectation, computed once per case ------------------------------------------------------------------------------------------------
def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def expected(name):
    """{index, counts, semantics (None without), truth_points / truth_colors / truth_normals (float64, None without), tol_*: the bar per
    component}: the checker on the CPU in the input's dtype, its float64 means, and the largest |member| per voxel and component."""
    c = case(name)
    pts, col, nrm, sem = _t(c["points"]), _t(c["colors"]), _t(c["normals"]), _t(c["semantics"])
    p, cc, nn, s, counts, index = V.voxel_down_sample_torch(pts, c["voxel_size"], col, nrm, sem, mean_dtype=torch.float64, return_counts=True,
                                                           return_index=True, round_means=False)
    out = {"index": index.numpy(), "counts": counts.numpy(), "semantics": None if s is None else s.numpy(),
           "truth_points": p.numpy(), "truth_colors": None if cc is None else cc.numpy(), "truth_normals": None if nn is None else nn.numpy()}
    if pts.shape[0] == 0:
        for key in ("points", "colors", "normals"):
            out["tol_" + key] = np.zeros((0, 3), np.float32)
        return out
    all_index = V.voxel_index_torch(pts, c["voxel_size"])[0].numpy()
    rows = np.searchsorted(out["index"], all_index)                       # the row of every point whose voxel was kept
    rows_ok = (rows < out["index"].size)
    rows_ok[rows_ok] = out["index"][rows[rows_ok]] == all_index[rows_ok]
    for key, arr in (("points", c["points"]), ("colors", c["colors"]), ("normals", c["normals"])):
        if arr is None:
            out["tol_" + key] = None
            continue
        largest = np.zeros((out["index"].size, 3), np.float64)
        np.maximum.at(largest, rows[rows_ok], np.abs(arr[rows_ok].astype(np.float64)))
        out["tol_" + key] = np.spacing(largest.astype(np.float32)).astype(np.float64)      # one float32 ulp of the largest |member|
    return out


def compare(name, got, what=""):
    """`got`: {points, colors, normals, semantics, counts, index} as numpy arrays (None where the case has no such attribute)."""
    c, want = case(name), expected(name)
    tag = f"{what} {name}"
    assert got["index"].dtype == np.int64 and got["counts"].dtype == np.int32, tag
    assert got["index"].shape == want["index"].shape, f"{tag}: m = {got['index'].shape[0]}, expected {want['index'].shape[0]}"
    assert np.array_equal(got["index"], want["index"]), f"{tag}: voxel indices / row order / keep decisions"
    assert np.array_equal(got["counts"], want["counts"]), f"{tag}: member counts"
    if c["semantics"] is None:
        assert got["semantics"] is None, tag
    else:
        assert got["semantics"].dtype == np.int32 and np.array_equal(got["semantics"], want["semantics"]), f"{tag}: labels"
    m = want["index"].shape[0]
    for key in ("points", "colors", "normals"):
        if c[key] is None:
            assert got[key] is None, f"{tag}: {key} given back without an input"
            continue
        g = got[key]
        assert g.dtype == np.float32 and g.shape == (m, 3), f"{tag}: {key} is {g.dtype} {g.shape}"
        err = np.abs(g.astype(np.float64) - want["truth_" + key])
        bad = ~(err <= want["tol_" + key])                 # (a NaN is bad)
        assert not bad.any(), f"{tag}: {key}: {int(bad.sum())} components beyond one ulp of the largest member, worst {np.nanmax(err / want['tol_' + key]):.3g} ulp"


# ---- an independent statement of the routine, with the mistakes the bars must catch ---------------------------------------------------------
VARIANTS = ("reciprocal", "round", "lo_without_half", "offset_per_axis", "strict_share", "float32_sum", "wrong_divisor", "descending")


def numpy_down_sample(c, variant=None):
    """The routine in numpy, a loop over the voxels; `variant` plants one mistake."""
    assert variant is None or variant in VARIANTS
    pts, v = c["points"], c["voxel_size"]
    T = pts.dtype.type
    n = pts.shape[0]
    none = lambda a: None if a is None else np.zeros((0, 3), np.float32)
    if n == 0:
        return {"points": none(pts), "colors": none(c["colors"]), "normals": none(c["normals"]),
                "semantics": None if c["semantics"] is None else np.zeros((0,), np.int32), "counts": np.zeros((0,), np.int32), "index": np.zeros((0,), np.int64)}
    half = T(0.0) if variant == "lo_without_half" else T(v * 0.5)
    lo, hi = (pts.min(0) - half).astype(T), (pts.max(0) + half).astype(T)
    offset = int((float(hi.max()) - float(lo.min()) + 2 * v) / v)
    d = (pts - lo).astype(T)
    q = (d * (T(1.0) / T(v))).astype(T) if variant == "reciprocal" else (d / T(v)).astype(T)
    cidx = (np.rint(q) if variant == "round" else np.trunc(q)).astype(np.int64)
    if variant == "offset_per_axis":
        ox, oy = [int((float(hi[k]) - float(lo[k]) + 2 * v) / v) for k in (0, 1)]
        index = cidx[:, 0] + ox * cidx[:, 1] + ox * oy * cidx[:, 2]
    else:
        index = cidx[:, 0] + offset * cidx[:, 1] + offset * offset * cidx[:, 2]
    order = np.argsort(index, kind="stable")
    voxels, starts, counts = np.unique(index[order], return_index=True, return_counts=True)
    acc = np.float32 if variant == "float32_sum" else np.float64
    rows = {"points": [], "colors": [], "normals": [], "semantics": [], "counts": [], "index": []}
    for vox, b, k in zip(voxels, starts, counts):
        members = order[b:b + k]
        label = None
        if c["semantics"] is not None:
            labels, freq = np.unique(c["semantics"][members].astype(np.int64), return_counts=True)
            most = int(freq.max())
            if (5 * most > 4 * k) if variant == "strict_share" else (5 * most >= 4 * k):
                label = int(labels[np.argmax(freq)])
            else:
                continue
        for key in ("points", "colors", "normals"):
            if c[key] is not None:
                s = np.zeros(3, acc)
                for row in c[key][members].astype(acc):      # one member at a time, in the accumulator's precision
                    s = (s + row).astype(acc)
                rows[key].append((s / acc(k + 1 if variant == "wrong_divisor" else k)).astype(np.float32))
        rows["semantics"].append(label)
        rows["counts"].append(k)
        rows["index"].append(vox)
    pick = slice(None, None, -1) if variant == "descending" else slice(None)
    out = {key: (np.array(rows[key], np.float32).reshape(-1, 3)[pick] if c[key] is not None else None) for key in ("points", "colors", "normals")}
    out["semantics"] = None if c["semantics"] is None else np.array(rows["semantics"], np.int32)[pick]
    out["counts"] = np.array(rows["counts"], np.int32)[pick]
    out["index"] = np.array(rows["index"], np.int64)[pick]
    return out

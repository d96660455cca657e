"""Colouring and labelling the LiDAR returns from the camera frames on the GPU (csrc/lidar_label.hip; include/surfel_raster.h states the
semantics once more): the step every dataset reader of the reference takes between a sweep and `SemanticPointCloud.voxel_down_sample`
[REF scene/dataset_readers/projection_utils.py:17-104, waymo.py:79-192, kitti.py:117-163, pandaset.py:53-106].

    LabelViews              the cameras and their pictures: w2c [V,4,4], K [V,3,3], hw [V,2], the resident uint8 images [h,w,3] (None for the
                            vote) and label maps [h,w], an optional label_lut (uint8 [256], applied to every map byte as it is read: the
                            segmenter's Cityscapes ids can stay resident); the device table of V records is built once
    label_sweeps            mode="merge": getWaymoPointCloudSemanticFromImageAtCertainFrame for S sweeps at once -- sweep s through the views
                            s C .. s C + C - 1; per point the colours of the cameras that see it with a certain label are averaged, the last
                            camera's label wins, the points no camera took are dropped.  mode="per_view": KITTI's and Pandaset's shape -- one row
                            per (point, camera) that is inside and certain, in the order (sweep, camera, point).  One read-back (the row count)
    vote_semantics          getWaymoPointCloudSemanticFromImage: every point through every view, no certainty test, the class seen most often
                            (the first of equals, as argmax); one read-back
    in_frame_numpy, certain_mask_numpy, label_sweeps_numpy, vote_semantics_numpy
                            the checkers: the reference's lines in float64 numpy
    label_sweeps_torch, vote_semantics_torch
                            the same in stock torch float64 on the tensors' device: the timing baseline on the GPU

The predicate, in float64 in a fixed order (the kernel is built without contraction, numpy and torch have none between two operations):
    cam_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i,   p_i = (K_i0 cam_0 + K_i1 cam_1) + K_i2 cam_2,   pix = p_xy / p_z   (IEEE divisions)
    inside = pix.x < w && pix.x > 0 && pix.y < h && pix.y > 0 && cam_z > 0     all strict, false for a NaN; a non-finite coordinate is in no view
    (u, v) = trunc(pix)
The certainty test with r = check_range and l0 = map[v,u]: the corners (v-r, u-r), (v-r, u+r), (v+r, u-r) and the fourth are compared with
l0 where they are valid (v-r > 0 resp. v+r < h, u-r > 0 resp. u+r < w: row 0 and column 0 never are); a point is certain when no valid
corner differs.  fourth_corner="reference" (the default): the fourth corner, valid when v+r < h && u+r < w, reads column u-r as the reference's
line 94 does, which wraps to w + u - r where it is negative (numpy's indexing); "mirrored" reads (v+r, u+r).

Deliberate differences from the reference: the reference multiplies matrices through BLAS, whose summation order is not stated -- the order
above is this library's contract and the decisions agree wherever they do not hang on the last bit; a picture that is not exactly (h, w)
raises ValueError (the reference raises IndexError at the first point outside it); a projective w2c is refused (the reference divides by a w
that is 1); in the vote a label >= n_classes is counted and raises ValueError after the call's read-back (the reference's index raises at
once); `tag` is int32 (argmax gives int64).  Limits: V <= 65535, 32 views a sweep, n < 2**31, n * C < 2**31 in the per-view mode, n_classes <= 8.
CPU tensors raise SurfelRasterError: there is no CPU path."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from ._call import buf, call, ptr, workspace

MAX_VIEWS, MAX_CAMERAS, MAX_CLASSES = 65535, 32, 8
FOURTH_CORNER = {"reference": 0, "mirrored": 1}
# struct SrLabelView of include/surfel_raster.h (tests/test_lidar_label_host.py holds this to the header's text)
VIEW_DTYPE = np.dtype([("w2c", np.float64, (12,)), ("K", np.float64, (9,)), ("h", np.int32), ("w", np.int32), ("image", np.uint64), ("map", np.uint64)],
                      align=True)
_REAL = (torch.float32, torch.float64)


class LabelledSweeps(NamedTuple):
    xyz: torch.Tensor             # [M,3] in the points' dtype, the kept rows bit for bit
    rgb: torch.Tensor             # [M,3] float64 on the 0..255 scale
    semantics: torch.Tensor       # [M] int32
    index: torch.Tensor           # [M] int64: the row's point
    rows_per_sweep: torch.Tensor  # [S] int32


def _host(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


class LabelViews:
    """The cameras and their pictures.  w2c, K (float64) and hw (integers) may be arrays, host or device tensors: they are read once.
    `images` (None: labels only) and `maps` are lists of V uint8 pictures of exactly (h, w); for the GPU calls they are resident tensors,
    taken as they are (made contiguous where they are not) and kept alive here; the checkers take arrays or CPU tensors."""

    def __init__(self, w2c, K, hw, images, maps, label_lut=None):
        self.w2c, self.K, self.hw = _host(w2c, np.float64), _host(K, np.float64), _host(hw, np.int64)
        V = self.w2c.shape[0]
        if self.w2c.shape != (V, 4, 4) or self.K.shape != (V, 3, 3) or self.hw.shape != (V, 2):
            raise ValueError(f"w2c [V,4,4], K [V,3,3], hw [V,2]; got {self.w2c.shape}, {self.K.shape}, {self.hw.shape}")
        if V > MAX_VIEWS:
            raise ValueError(f"{V} views: at most {MAX_VIEWS}")
        if not np.array_equal(self.w2c[:, 3, :], np.tile([0.0, 0.0, 0.0, 1.0], (V, 1))):
            bad = int(np.flatnonzero((self.w2c[:, 3, :] != [0.0, 0.0, 0.0, 1.0]).any(axis=1))[0])
            raise ValueError(f"w2c[{bad}] is projective: its last row is {self.w2c[bad, 3].tolist()}, not (0, 0, 0, 1)")
        if V and (self.hw.min() < 1 or self.hw.max() >= 1 << 31):
            raise ValueError("hw: every picture has at least one pixel a side and fewer than 2**31")
        self.images = None if images is None else self._pictures("images", images, 3)
        self.maps = self._pictures("maps", maps, None)
        self.label_lut = None
        if label_lut is not None:
            lut = torch.as_tensor(label_lut)
            if lut.dtype != torch.uint8 or tuple(lut.shape) != (256,):
                raise ValueError(f"label_lut must be uint8 [256]; got {lut.dtype} {list(lut.shape)}")
            self.label_lut = lut.contiguous()
        self._tables = {}

    def __len__(self):
        return int(self.w2c.shape[0])

    def _pictures(self, name, pictures, channels):
        pictures = [torch.as_tensor(p) for p in pictures]
        if len(pictures) != len(self):
            raise ValueError(f"{len(pictures)} {name} for {len(self)} views")
        out = []
        for f, p in enumerate(pictures):
            h, w = (int(x) for x in self.hw[f])
            want = (h, w) if channels is None else (h, w, channels)
            if p.dtype != torch.uint8 or tuple(p.shape) != want:
                raise ValueError(f"{name}[{f}] must be uint8 {list(want)} (the view's h, w exactly); got {p.dtype} {list(p.shape)}")
            out.append(p.detach().contiguous())
        return out

    def lut_numpy(self):
        return np.arange(256, dtype=np.uint8) if self.label_lut is None else self.label_lut.cpu().numpy()

    def map_numpy(self, f):
        """the label map of view f with the lut applied, uint8 [h,w]"""
        return self.lut_numpy()[self.maps[f].cpu().numpy()]

    def table(self, dev):
        """-> (the device table uint8 [V * 192], the lut on the device or None); built once per device"""
        dev = torch.device(dev)
        if dev not in self._tables:
            for name, pictures in (("images", self.images), ("maps", self.maps)):
                for f, p in enumerate(pictures or []):
                    if not p.is_cuda:
                        raise L.SurfelRasterError(f"{name}[{f}] is on {p.device}: the pictures must be resident CUDA (ROCm) tensors; there is no CPU path")
                    if p.device != dev:
                        raise L.SurfelRasterError(f"{name}[{f}] is on {p.device}, the points on {dev}")
            rec = np.zeros((len(self),), dtype=VIEW_DTYPE)
            rec["w2c"] = self.w2c[:, :3, :].reshape(len(self), 12)
            rec["K"] = self.K.reshape(len(self), 9)
            rec["h"], rec["w"] = self.hw[:, 0], self.hw[:, 1]
            rec["image"] = 0 if self.images is None else [p.data_ptr() for p in self.images]
            rec["map"] = [p.data_ptr() for p in self.maps]
            table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
            lut = None if self.label_lut is None else self.label_lut.to(dev)
            self._tables[dev] = (table, lut)
        return self._tables[dev]


# ---- argument checks ----------------------------------------------------------------------------------------------------------------------
def _check_points(points):
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype not in _REAL:
        raise ValueError(f"points must be a float32 or float64 tensor [n,3]; got {getattr(points, 'dtype', type(points).__name__)} "
                         f"{list(getattr(points, 'shape', []))}")
    if points.shape[0] >= 1 << 31:
        raise ValueError(f"{points.shape[0]} points: fewer than 2**31")
    return int(points.shape[0])


def _check_sweeps(n, sweep_offsets, views, cameras_per_sweep, mode, check_range, fourth_corner):
    offsets = _host(sweep_offsets, np.int64).reshape(-1)
    if offsets.size < 2 or offsets[0] != 0 or offsets[-1] != n or (np.diff(offsets) < 0).any():
        raise ValueError(f"sweep_offsets must ascend from 0 to n = {n} in S + 1 >= 2 entries; got {offsets.tolist()[:8]}{'...' if offsets.size > 8 else ''}")
    S, C = offsets.size - 1, int(cameras_per_sweep)
    if not 1 <= C <= MAX_CAMERAS:
        raise ValueError(f"cameras_per_sweep = {cameras_per_sweep}: 1..{MAX_CAMERAS}")
    if S * C != len(views):
        raise ValueError(f"{S} sweeps x {C} cameras need {S * C} views; got {len(views)}")
    if mode not in ("merge", "per_view"):
        raise ValueError(f"mode = {mode!r}: 'merge' or 'per_view'")
    if mode == "per_view" and n * C >= 1 << 31:
        raise ValueError(f"{n} points x {C} cameras: fewer than 2**31 rows a call (fewer sweeps a call)")
    if int(check_range) != check_range or not 0 <= check_range < 1 << 31:
        raise ValueError(f"check_range = {check_range}: a non-negative integer")
    if fourth_corner not in FOURTH_CORNER:
        raise ValueError(f"fourth_corner = {fourth_corner!r}: 'reference' or 'mirrored'")
    if views.images is None:
        raise ValueError("label_sweeps needs views with images")
    return offsets, S, C


def _need_cuda(points, what):
    if not points.is_cuda:
        raise L.SurfelRasterError(f"points is on {points.device}: {what} needs CUDA (ROCm) tensors; there is no CPU path ({what}_numpy is the checker)")


# ---- the fused ops ------------------------------------------------------------------------------------------------------------------------
def _emit(dev, n, points, offsets_dev, S, max_sweep, rows_per_point, ws, m, want_rgb, want_rows):
    xyz = torch.empty((m, 3), dtype=points.dtype, device=dev)
    rgb = torch.empty((m, 3), dtype=torch.float64, device=dev) if want_rgb else None
    sem = torch.empty((m,), dtype=torch.int32, device=dev)
    index = torch.empty((m,), dtype=torch.int64, device=dev)
    rows = torch.empty((S,), dtype=torch.int32, device=dev) if want_rows else None
    call("sr_lidar_label_emit", dev, n, ptr(points), int(points.dtype == torch.float64), ptr(offsets_dev), S, max_sweep, rows_per_point, *buf(ws), m,
         ptr(xyz), ptr(rgb), ptr(sem), ptr(index), ptr(rows))
    return xyz, rgb, sem, index, rows


def label_sweeps(points, sweep_offsets, views, cameras_per_sweep, mode="merge", check_range=10, fourth_corner="reference"):
    """-> LabelledSweeps on the points' device; runs on the current stream: decide, scan, one read-back of the row count, emit.  See the
    module docstring for the semantics and the refusals."""
    n = _check_points(points)
    offsets, S, C = _check_sweeps(n, sweep_offsets, views, cameras_per_sweep, mode, check_range, fourth_corner)
    _need_cuda(points, "label_sweeps")
    dev = points.device
    table, lut = views.table(dev)
    if n == 0:
        z = lambda *shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        return LabelledSweeps(z(0, 3, dtype=points.dtype), z(0, 3, dtype=torch.float64), z(0, dtype=torch.int32), z(0, dtype=torch.int64), z(S, dtype=torch.int32))
    points = points.detach().contiguous()
    offsets_dev = torch.from_numpy(offsets.astype(np.int32)).to(dev)
    max_sweep = int(np.diff(offsets).max())
    rows_per_point = C if mode == "per_view" else 1
    ws = workspace("sr_lidar_label_workspace_bytes", dev, n, rows_per_point)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    call("sr_lidar_label_decide", dev, n, ptr(points), int(points.dtype == torch.float64), ptr(offsets_dev), S, max_sweep, ptr(table), len(views), C,
         int(check_range), FOURTH_CORNER[fourth_corner], ptr(lut), int(mode == "per_view"), *buf(ws), ptr(counts))
    m = int(counts.cpu()[0])                                # the one read-back
    return LabelledSweeps(*_emit(dev, n, points, offsets_dev, S, max_sweep, rows_per_point, ws, m, True, True))


def vote_semantics(points, views, n_classes=6):
    """-> (xyz[valid] in the points' dtype, tag int32 [M], valid_mask bool [n]) on the points' device; one read-back."""
    n = _check_points(points)
    if not 1 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError(f"n_classes = {n_classes}: 1..{MAX_CLASSES}")
    if len(views) < 1:
        raise ValueError("vote_semantics needs at least one view")
    _need_cuda(points, "vote_semantics")
    dev = points.device
    table, lut = views.table(dev)
    if n == 0:
        return torch.zeros((0, 3), dtype=points.dtype, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.bool, device=dev)
    points = points.detach().contiguous()
    ws = workspace("sr_lidar_label_workspace_bytes", dev, n, 1)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    valid = torch.empty((n,), dtype=torch.uint8, device=dev)
    call("sr_lidar_vote", dev, n, ptr(points), int(points.dtype == torch.float64), ptr(table), len(views), int(n_classes), ptr(lut), *buf(ws), ptr(valid),
         ptr(counts))
    m, bad = (int(x) for x in counts.cpu())                 # the one read-back
    if bad:
        raise ValueError(f"{bad} (point, view) hits read a label >= n_classes = {n_classes}: refused (the reference's index raises)")
    xyz, _, tag, _, _ = _emit(dev, n, points, None, 1, n, 1, ws, m, False, False)
    return xyz, tag, valid.view(torch.bool)


# ---- the checkers: float64 numpy ----------------------------------------------------------------------------------------------------------
def project_numpy(xyz, w2c, K):
    """-> (pix [n,2], cam_z [n]) in float64, the operations of the module docstring in their order"""
    p = np.asarray(xyz).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    R, K = np.asarray(w2c, np.float64), np.asarray(K, np.float64)
    with np.errstate(all="ignore"):
        cam = [((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + R[i, 3] for i in range(3)]
        q = [(K[i, 0] * cam[0] + K[i, 1] * cam[1]) + K[i, 2] * cam[2] for i in range(3)]
        pix = np.stack([q[0] / q[2], q[1] / q[2]], axis=1)
    return pix, cam[2]


def in_frame_numpy(h, w, xyz, w2c, K):
    """getCullMaskPointCloudInFrame: -> (mask bool [n], valid_pix int32 [m,2] = trunc(pix) of the points inside, as (u, v))"""
    pix, z = project_numpy(xyz, w2c, K)
    with np.errstate(invalid="ignore"):
        mask = (pix[:, 0] < w) & (pix[:, 0] > 0) & (pix[:, 1] < h) & (pix[:, 1] > 0) & (z > 0) & np.isfinite(np.asarray(xyz, np.float64)).all(axis=1)
    return mask, pix[mask].astype(np.int32)


def certain_mask_numpy(semantic_map, pix, check_range=10, fourth_corner="reference"):
    """getCertainSemanticMask: -> bool [m]; pix int [m,2] as (u, v), inside the map"""
    m = np.asarray(semantic_map)
    h, w = m.shape[:2]
    u, v = np.asarray(pix)[:, 0].astype(np.int64), np.asarray(pix)[:, 1].astype(np.int64)
    r = int(check_range)
    top, bottom, left, right = v - r, v + r, u - r, u + r
    l0 = m[v, u]
    certain = np.ones(u.shape, dtype=bool)
    fourth = left if fourth_corner == "reference" else right      # a negative column wraps: numpy's own indexing, as in the reference
    for rows, row_ok, cols, col_ok in ((top, top > 0, left, left > 0), (top, top > 0, right, right < w), (bottom, bottom < h, left, left > 0),
                                       (bottom, bottom < h, fourth, right < w)):
        ok = row_ok & col_ok
        certain[ok] &= m[rows[ok], cols[ok]] == l0[ok]
    return certain


def label_sweeps_numpy(points, sweep_offsets, views, cameras_per_sweep, mode="merge", check_range=10, fourth_corner="reference"):
    """-> dict of numpy arrays under LabelledSweeps' names: the reference's loops, sweep by sweep and camera by camera"""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    offsets, S, C = _check_sweeps(len(pts), sweep_offsets, views, cameras_per_sweep, mode, check_range, fourth_corner)
    out = {"xyz": [], "rgb": [], "semantics": [], "index": []}
    rows_per_sweep = np.zeros(S, dtype=np.int32)
    for s in range(S):
        a, b = int(offsets[s]), int(offsets[s + 1])
        xyz = pts[a:b]
        sums, count, label = np.zeros((b - a, 3)), np.zeros(b - a), np.full(b - a, -1, dtype=np.int32)
        for c in range(C):
            f = s * C + c
            h, w = (int(x) for x in views.hw[f])
            semantic_map, image = views.map_numpy(f), views.images[f].cpu().numpy()
            mask, pix = in_frame_numpy(h, w, xyz, views.w2c[f], views.K[f])
            certain = certain_mask_numpy(semantic_map, pix, check_range, fourth_corner)
            took = np.flatnonzero(mask)[certain]
            pix = pix[certain]
            colour, lab = image[pix[:, 1], pix[:, 0]].astype(np.float64), semantic_map[pix[:, 1], pix[:, 0]].astype(np.int32)
            if mode == "per_view":
                out["xyz"].append(xyz[took]); out["rgb"].append(colour); out["semantics"].append(lab); out["index"].append(took + a)
                rows_per_sweep[s] += len(took)
            else:
                sums[took] += colour
                count[took] += 1
                label[took] = lab                           # the later camera overwrites
        if mode == "merge":
            keep = count > 0
            out["xyz"].append(xyz[keep]); out["rgb"].append(sums[keep] / count[keep, None]); out["semantics"].append(label[keep])
            out["index"].append(np.flatnonzero(keep) + a)
            rows_per_sweep[s] = int(keep.sum())
    cat = lambda parts, dtype, tail: np.concatenate(parts).astype(dtype) if parts else np.zeros((0,) + tail, dtype=dtype)
    return {"xyz": cat(out["xyz"], pts.dtype, (3,)).reshape(-1, 3), "rgb": cat(out["rgb"], np.float64, (3,)).reshape(-1, 3),
            "semantics": cat(out["semantics"], np.int32, ()), "index": cat(out["index"], np.int64, ()), "rows_per_sweep": rows_per_sweep}


def vote_semantics_numpy(points, views, n_classes=6):
    """-> (xyz[valid], tag int32 [M], valid_mask bool [n]); a label >= n_classes raises ValueError"""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    hits, seen = np.zeros((len(pts), int(n_classes)), dtype=np.int64), np.zeros(len(pts), dtype=np.int64)
    for f in range(len(views)):
        h, w = (int(x) for x in views.hw[f])
        mask, pix = in_frame_numpy(h, w, pts, views.w2c[f], views.K[f])
        lab = views.map_numpy(f)[pix[:, 1], pix[:, 0]].astype(np.int64)
        if (lab >= n_classes).any():
            raise ValueError(f"{int((lab >= n_classes).sum())} hits of view {f} read a label >= n_classes = {n_classes}")
        hits[np.flatnonzero(mask), lab] += 1
        seen[mask] += 1
    valid = seen > 0
    return pts[valid], np.argmax(hits[valid], axis=1).astype(np.int32), valid


# ---- the twins: stock torch float64 on the tensors' device --------------------------------------------------------------------------------
def _project_torch(p, w2c, K):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    cam = [((w2c[i, 0] * x + w2c[i, 1] * y) + w2c[i, 2] * z) + w2c[i, 3] for i in range(3)]
    q = [(K[i, 0] * cam[0] + K[i, 1] * cam[1]) + K[i, 2] * cam[2] for i in range(3)]
    return q[0] / q[2], q[1] / q[2], cam[2]


def _in_frame_torch(p, w2c, K, h, w):
    pu, pv, z = _project_torch(p, w2c, K)
    mask = (pu < w) & (pu > 0) & (pv < h) & (pv > 0) & (z > 0) & torch.isfinite(p).all(dim=1)
    return mask, pu[mask].to(torch.int64), pv[mask].to(torch.int64)


def _certain_torch(m, u, v, r, fourth_corner):
    h, w = m.shape
    top, bottom, left, right = v - r, v + r, u - r, u + r
    l0 = m[v, u]
    certain = torch.ones_like(u, dtype=torch.bool)
    fourth = torch.where(left < 0, left + w, left) if fourth_corner == "reference" else right
    for rows, row_ok, cols, col_ok in ((top, top > 0, left, left > 0), (top, top > 0, right, right < w), (bottom, bottom < h, left, left > 0),
                                       (bottom, bottom < h, fourth, right < w)):
        ok = row_ok & col_ok
        certain &= ~ok | (m[rows.clamp(0, h - 1), cols.clamp(0, w - 1)] == l0)
    return certain


def _views_torch(views, dev):
    lut = torch.from_numpy(views.lut_numpy()).to(dev)
    return torch.from_numpy(views.w2c).to(dev), torch.from_numpy(views.K).to(dev), lut


def label_sweeps_torch(points, sweep_offsets, views, cameras_per_sweep, mode="merge", check_range=10, fourth_corner="reference"):
    """label_sweeps_numpy in stock torch on the points' device -> LabelledSweeps"""
    n = _check_points(points)
    offsets, S, C = _check_sweeps(n, sweep_offsets, views, cameras_per_sweep, mode, check_range, fourth_corner)
    dev = points.device
    w2c, K, lut = _views_torch(views, dev)
    p64 = points.to(torch.float64)
    parts = {"xyz": [], "rgb": [], "semantics": [], "index": []}
    rows_per_sweep = []
    for s in range(S):
        a, b = int(offsets[s]), int(offsets[s + 1])
        xyz = p64[a:b]
        sums = torch.zeros((b - a, 3), dtype=torch.float64, device=dev)
        count = torch.zeros((b - a,), dtype=torch.float64, device=dev)
        label = torch.full((b - a,), -1, dtype=torch.int32, device=dev)
        rows = 0
        for c in range(C):
            f = s * C + c
            h, w = (int(x) for x in views.hw[f])
            m = lut[views.maps[f].to(dev).long()]
            mask, u, v = _in_frame_torch(xyz, w2c[f], K[f], h, w)
            certain = _certain_torch(m, u, v, int(check_range), fourth_corner)
            took = torch.nonzero(mask)[:, 0][certain]
            u, v = u[certain], v[certain]
            colour, lab = views.images[f].to(dev)[v, u].to(torch.float64), m[v, u].to(torch.int32)
            if mode == "per_view":
                parts["xyz"].append(points[a:b][took]); parts["rgb"].append(colour); parts["semantics"].append(lab); parts["index"].append(took + a)
                rows = rows + took.shape[0]
            else:
                sums[took] += colour
                count[took] += 1
                label[took] = lab
        if mode == "merge":
            keep = count > 0
            parts["xyz"].append(points[a:b][keep]); parts["rgb"].append(sums[keep] / count[keep, None]); parts["semantics"].append(label[keep])
            parts["index"].append(torch.nonzero(keep)[:, 0] + a)
            rows = parts["index"][-1].shape[0]
        rows_per_sweep.append(rows)
    cat = lambda key, dtype, tail: torch.cat(parts[key]).to(dtype) if parts[key] else torch.zeros((0,) + tail, dtype=dtype, device=dev)
    return LabelledSweeps(cat("xyz", points.dtype, (3,)), cat("rgb", torch.float64, (3,)), cat("semantics", torch.int32, ()), cat("index", torch.int64, ()),
                          torch.tensor(rows_per_sweep, dtype=torch.int32, device=dev))


def vote_semantics_torch(points, views, n_classes=6):
    """vote_semantics_numpy in stock torch on the points' device; the check of the labels is one read-back at the end"""
    n = _check_points(points)
    dev = points.device
    w2c, K, lut = _views_torch(views, dev)
    p64 = points.to(torch.float64)
    hits = torch.zeros((n, int(n_classes) + 1), dtype=torch.int64, device=dev)      # the last column: labels >= n_classes
    seen = torch.zeros((n,), dtype=torch.int64, device=dev)
    for f in range(len(views)):
        h, w = (int(x) for x in views.hw[f])
        mask, u, v = _in_frame_torch(p64, w2c[f], K[f], h, w)
        lab = lut[views.maps[f].to(dev)[v, u].long()].long().clamp(max=int(n_classes))
        hits[torch.nonzero(mask)[:, 0], lab] += 1
        seen += mask
    valid = seen > 0
    bad = int(hits[:, -1].sum())
    if bad:
        raise ValueError(f"{bad} (point, view) hits read a label >= n_classes = {n_classes}")
    return points[valid], torch.argmax(hits[valid][:, :-1], dim=1).to(torch.int32), valid

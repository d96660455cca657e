"""The cases and the bars of the unveiling stage's frame masks (streetunveiler_amd/unveil.py), shared by tests/test_unveil_host.py (CPU)
and tests/test_gpu_unveil.py.  Small: the kernels can go wrong at edges, not at size.

Images: sizes 1x1, 1x17, 17x1, 4x4 (smaller than every k > 4), 63, 64 and 65 wide (one tile, exactly one, one column into the next),
37x53 (two tile rows) and 40x130 (three tile columns: a tile with real pixels on both sides); k in {1, 2, 5, 10, 15, 31}; masks: empty,
full, one pixel in each corner and in the middle, a checkerboard, random at 1 % and 50 %; uint8 masks with values other than 0 and 1;
non-contiguous inputs.

Points: P in {0, 1, 63, 64, 65, 4097}, F in {1, 3} with frames of different (h, w), max_z given and None, reso_scale None, 1.0 and 2.0,
rows with NaN and inf, points behind the camera, a cloud no frame sees.

PLANTED ROWS.  Cameras A and B have an axis permutation as rotation, a dyadic translation, and focal lengths and principal point that are
powers of two (B's K has a projective last row (4, 0, 1), so that a point with cam.z == 0 has a finite pix and the test z > 0 alone decides
it); the planted coordinates are dyadic with few bits.  Every float32 operation on them is then exact in any order, fused or not, and the
rows land exactly on pix.x == 0, == w, pix.y == 0, == h, z == 0, z == max_z, on integer pixel coordinates, one step inside each border and
on a pixel coordinate with fraction 0.75: every implementation must decide them alike, so they count as robust whatever the bound says.

RANDOM ROWS.  A decision is robust when the float64 checker decides the same with every intermediate moved by its float32 forward-error
bound.  With u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a dot product of
n terms, in any order, with or without fused multiply-adds, errs by at most gamma_n sum |a_i b_i|):
    cam_i = sum_j R_ij x_j + t_i, three products and three additions:  |d cam_i| <= gamma_4 (sum_j |R_ij x_j| + |t_i|) =: dc_i
    p_i = sum_j K_ij cam_j on the perturbed cam:  |d p_i| <= sum_j |K_ij| dc_j + gamma_3 sum_j |K_ij| (|cam_j| + dc_j) =: dp_i
    pix = p_xy / p_z, one more rounding:  |d pix| <= (dp_xy + |pix| dp_z) / (|p_z| - dp_z) + 2 u |pix| =: B   (infinite where |p_z| <= dp_z)
A point is robust in a frame when pix.x and pix.x - w, pix.y and pix.y - h are farther than B from 0, cam.z and cam.z - max_z farther than
dc_z, and -- where the point is admitted, max_z aside -- floor(pix - B) == floor(pix + B) in both axes: trunc(pix) does not change within the bound.
The reso_scale values used (1.0 and 2.0) divide exactly.  The float64 checker's own rounding (2^-53) is nothing against these.
Masks and lists are compared on robust points only; frame_visibility, pick_view and the compacted lists run on clouds filtered to the
points robust in every frame, where counts, order and pix must be equal exactly.  At most 1 % of a random case's points are non-robust
(asserted by the host test).  Depths and depth sums: within twice the float32 twin's own deviation from float64, floor half an ulp.

THRESHOLDS.  Planted values sit exactly on float32(threshold) and one float32 step on either side; random pixels are compared where the
float64 quantity is farther than 4 ulp of the threshold from it; at most 0.1 % of a case's pixels may be excluded.

BYTES.  Every byte within 1 of the float64 checker's, and equal wherever the float64 value of 255 x + 0.5 is farther than 1e-3 from an
integer: the float32 composite and the scaling err by under 2e-4 there (a few ulp of 2, times 255, plus a few ulp of 256), which leaves
5 x slack.  The band is taken only round the integers 1 .. 255, where trunc(clamp(., 0, 255)) steps: elsewhere equality is demanded too.
At most 1 % of a case's bytes may lie in the excluded band (none in a case of fewer than 100 pixels, where one byte is more than that).  Planted pixels: x in {0, 1, < 0, > 1, NaN}, depth in {0, inf,
negative, 0.5}, alpha in {0, 1}."""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np
import torch

from streetunveiler_amd import unveil as U

U32 = 2.0 ** -24
KS = (1, 2, 5, 10, 15, 31)
IMAGE_SIZES = ((1, 1), (1, 17), (17, 1), (4, 4), (5, 63), (5, 64), (5, 65), (37, 53), (40, 130))
MASK_KINDS = ("empty", "full", "corner_tl", "corner_tr", "corner_bl", "corner_br", "middle", "checkerboard", "random_1", "random_50", "uint8_values")


def _gamma(n):
    return n * U32 / (1 - n * U32)


# ---- images -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_case(kind, H, W):
    """-> read-only uint8 [H,W] (values other than 0 and 1 in "uint8_values")"""
    rng = np.random.default_rng(zlib.crc32(f"{kind} {H} {W}".encode()))
    m = np.zeros((H, W), dtype=np.uint8)
    if kind == "full":
        m[:] = 1
    elif kind.startswith("corner_"):
        m[0 if kind[7] == "t" else H - 1, 0 if kind[8] == "l" else W - 1] = 1
    elif kind == "middle":
        m[H // 2, W // 2] = 1
    elif kind == "checkerboard":
        m[(np.add.outer(np.arange(H), np.arange(W)) % 2) == 0] = 1
    elif kind == "random_1":
        m[rng.random((H, W)) < 0.01] = 1
        m[rng.integers(H), rng.integers(W)] = 1
    elif kind == "random_50":
        m[rng.random((H, W)) < 0.5] = 1
    elif kind == "uint8_values":
        m[rng.random((H, W)) < 0.05] = 1
        m = (m * rng.integers(1, 256, size=(H, W))).astype(np.uint8)      # 2, 128, 255, ...: set is "not 0"
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def dilated(kind, H, W, k):
    out = U.dilate_mask_numpy(mask_case(kind, H, W), k)
    out.setflags(write=False)
    return out


def dilate_cases():
    return [(kind, H, W, k) for H, W in IMAGE_SIZES for k in KS for kind in MASK_KINDS]


def compare_dilation(run, label="dilate_mask"):
    """`run(mask uint8 [H,W] numpy, k)` -> bool [H,W] (anything np.asarray takes) on every case: exact."""
    for kind, H, W, k in dilate_cases():
        got = np.asarray(run(mask_case(kind, H, W), k))
        assert got.dtype == np.bool_ and got.shape == (H, W), (label, kind, H, W, k, got.dtype, got.shape)
        assert np.array_equal(got, dilated(kind, H, W, k)), f"{label}: {kind} {H}x{W} k={k}: {int((got != dilated(kind, H, W, k)).sum())} pixels differ"


class ThresholdCase(NamedTuple):
    a: np.ndarray            # [C,H,W] float32 (C = 1: the alphas)
    b: np.ndarray
    mask: np.ndarray         # [H,W] uint8 (refill only)
    compare: np.ndarray      # [H,W] bool: the undilated float64 decision is farther than 4 ulp of the threshold from it (or planted)


def _steps(value):
    t = np.float32(value)
    return np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))


@functools.lru_cache(maxsize=None)
def threshold_case(op, H, W):
    """op = "instance" (|a - b| > float32(0.01), C = 1) or "refill" (~(sum_c |a - b| < float32(0.02)) & mask, C = 3).  Random pixels + planted
    ones: exactly below, on and above the threshold, and a NaN (row 0, where the image is wide enough)."""
    rng = np.random.default_rng(11 + H * 1000 + W + (op == "refill"))
    C, thr = (1, 0.01) if op == "instance" else (3, 0.02)
    a = rng.random((C, H, W), dtype=np.float32)
    b = a + (rng.random((C, H, W), dtype=np.float32) < 0.5) * rng.normal(0, thr, (C, H, W)).astype(np.float32)      # half the pixels near the threshold
    b = b.astype(np.float32)
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=(H, W)).astype(np.uint8)
    planted = np.zeros((H, W), dtype=bool)
    values = list(_steps(thr)) + [np.float32("nan")]
    for x, v in enumerate(values[:W]):
        b[:, 0, x] = 0.0
        a[:, 0, x] = 0.0
        a[0, 0, x] = v           # the difference (and the sum over the channels) IS v: exact
        mask[0, x] = 1
        planted[0, x] = True
    quantity = np.abs(a.astype(np.float64) - b.astype(np.float64)).sum(0)
    t32 = np.float64(np.float32(thr))
    compare = planted | (np.abs(quantity - t32) > 4 * np.spacing(np.float32(thr))) | np.isnan(quantity)
    for arr in (a, b, mask, compare):
        arr.setflags(write=False)
    return ThresholdCase(a, b, mask, compare)


THRESHOLD_SIZES = IMAGE_SIZES
THRESHOLD_EXCLUDED_SHARE = 1e-3


def threshold_expected(op, H, W, k):
    """-> (undilated float64 decision [H,W], its dilation) -- the dilation of a decision that is only compared where `compare` holds would
    spread the doubt, so the cases are built to have NO excluded pixel a dilation could spread (asserted by the host test for these sizes)
    or the comparison is made on the undilated k = 1 result."""
    c = threshold_case(op, H, W)
    t = lambda x: torch.from_numpy(np.array(x))
    if op == "instance":
        raw = U.instance_pixel_mask_torch(t(c.a), t(c.b), 0.01, 1, torch.float64, undilated=True).numpy()
    else:
        raw = U.refill_mask_torch(t(c.a), t(c.b), t(c.mask), 2e-2, 1, torch.float64, undilated=True).numpy()
    return raw, U.dilate_mask_numpy(raw, k)


def compare_threshold(op, run, label):
    """`run(a, b, mask, k)` -> bool [H,W]: k = 1 gives the undilated decision, compared where the case allows; for every other k of KS the
    result must be the dilation of a decision that agrees with the float64 one wherever it is compared -- i.e. of run(..., 1) itself."""
    for H, W in THRESHOLD_SIZES:
        c = threshold_case(op, H, W)
        raw_want, _ = threshold_expected(op, H, W, 1)
        raw = np.asarray(run(c.a, c.b, c.mask, 1))
        assert raw.shape == (H, W) and raw.dtype == np.bool_
        assert np.array_equal(raw[c.compare], raw_want[c.compare]), f"{label} {op} {H}x{W}: {int((raw != raw_want)[c.compare].sum())} compared pixels differ"
        for k in KS[1:]:
            assert np.array_equal(np.asarray(run(c.a, c.b, c.mask, k)), U.dilate_mask_numpy(raw, k)), f"{label} {op} {H}x{W} k={k}: not the dilation of its own k = 1 result"


CONDITION_SIZES = IMAGE_SIZES      # below 100 pixels one byte is more than the share: those cases hold NO byte in the band (asserted by the host test)
BYTE_BAND = 1e-3
BYTE_EXCLUDED_SHARE = 1e-2


@functools.lru_cache(maxsize=None)
def condition_case(H, W):
    """-> (full, background, sky): dicts of read-only float32 numpy arrays under the render dicts' keys, random + the planted pixels"""
    rng = np.random.default_rng(5 + 131 * H + W)
    r = lambda *s: rng.random(s, dtype=np.float32)
    full = {"render": r(3, H, W) * 1.2 - 0.1, "rend_alpha": r(1, H, W)}
    bg = {"render": r(3, H, W) * 1.2 - 0.1, "rend_alpha": r(1, H, W), "surf_depth": r(1, H, W) * 5 + 0.3, "rend_normal": r(3, H, W) * 2.4 - 1.2}
    sky = r(3, H, W)
    flat = lambda a: a.reshape(a.shape[0], -1)
    n = H * W
    nan, inf = np.float32("nan"), np.float32("inf")
    for i, x in enumerate([0.0, 1.0, -0.25, 1.5, nan][:n]):                  # x itself: sky 0 -> original_rgb = inpainted_rgb = render
        flat(full["render"])[:, i] = x
        flat(bg["render"])[:, i] = x
        flat(sky)[:, i] = 0.0
        flat(bg["rend_normal"])[:, i] = 2 * x - 1                            # 0.5 n + 0.5 = x (exact for these)
    for i, d in enumerate([0.0, inf, -2.0, 0.5, -0.0, nan][:n]):
        flat(bg["surf_depth"])[0, i] = d
    for i, al in enumerate([0.0, 1.0, 1.0, 0.0][:n]):
        flat(full["rend_alpha"])[0, i] = al
        flat(bg["rend_alpha"])[0, i] = [0.0, 0.0, 1.0, 1.0][i]
    for d in (full, bg):
        for v in d.values():
            v.setflags(write=False)
    sky.setflags(write=False)
    return full, bg, sky


def condition_tensors(H, W, device="cpu"):
    full, bg, sky = condition_case(H, W)
    up = lambda a: torch.from_numpy(a.copy()).to(device)
    return {k: up(v) for k, v in full.items()}, {k: up(v) for k, v in bg.items()}, up(sky)


@functools.lru_cache(maxsize=None)
def condition_expected(H, W):
    out = U.inpaint_conditions_torch(*condition_tensors(H, W), 0.01, 5, torch.float64, values=True)
    return {k: v.numpy() for k, v in out.items()}


def byte_band(value):
    """[...] bool: the float64 value of 255 x + 0.5 is within BYTE_BAND of an integer at which trunc(clamp(., 0, 255)) steps, 1 .. 255 (a
    NaN is not: its byte is 0 for everyone; below 1 - BYTE_BAND and above 255 + BYTE_BAND every implementation clamps alike, so equality
    is demanded there too: no less than "farther than 1e-3 from an integer" asks)"""
    with np.errstate(invalid="ignore"):
        return (np.abs(value - np.round(value)) <= BYTE_BAND) & (value >= 1 - BYTE_BAND) & (value <= 255 + BYTE_BAND)


def compare_conditions(got, H, W, label):
    """`got`: the dict of inpaint_conditions (numpy arrays) against the float64 checker under the byte bars; the mask exactly (the alphas'
    differences of these cases keep away from the threshold: asserted by the host test)."""
    want = condition_expected(H, W)
    assert np.array_equal(np.asarray(got["mask"]), want["mask"]), f"{label} {H}x{W}: mask"
    for name, channels in U.CONDITION_IMAGES:
        g, w, v = np.asarray(got[name]), want[name], want[name + "_value"]
        assert g.dtype == np.uint8 and g.shape == (H, W, channels), (label, name, g.dtype, g.shape)
        diff = np.abs(g.astype(np.int32) - w.astype(np.int32))
        assert diff.max(initial=0) <= 1, f"{label} {H}x{W} {name}: a byte is off by {diff.max()}"
        strict = ~byte_band(v)
        assert not diff[strict].any(), f"{label} {H}x{W} {name}: {int((diff[strict] > 0).sum())} bytes differ where 255 x + 0.5 is farther than {BYTE_BAND} from an integer"


# ---- points -----------------------------------------------------------------------------------------------------------------------------
FRAME_SIZES = ((32, 64), (48, 40), (60, 100))      # (h, w) of frames 0, 1, 2
R_PERM = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])      # cam = (y, z, x) + t
T_DYADIC = np.array([0.5, -0.25, 1.0])
K_A = np.array([[64.0, 0.0, 32.0], [0.0, 32.0, 16.0], [0.0, 0.0, 1.0]])
K_B = np.array([[64.0, 0.0, 32.0], [0.0, 32.0, 16.0], [4.0, 0.0, 1.0]])
PLANTED_MAX_Z = 8.0
# camera-space rows for camera A (h, w) = (32, 64): pix = (64 cx / cz + 32, 32 cy / cz + 16)
PLANTED_A = np.array([
    [-0.5, 0.0, 2.0],                  # pix (16, 16): in, integer coordinates
    [-1.0, 0.0, 2.0],                  # pix.x == 0: out
    [1.0, 0.0, 2.0],                   # pix.x == w: out
    [0.0, -1.0, 2.0],                  # pix.y == 0: out
    [0.0, 1.0, 2.0],                   # pix.y == h: out
    [0.0, 0.0, PLANTED_MAX_Z],         # z == max_z: out where max_z is given, in (32, 16) where it is None
    [-1.0 + 2.0 ** -15, 0.0, 2.0],     # pix.x = 2^-10: in, trunc 0
    [1.0 - 2.0 ** -15, 0.0, 2.0],      # pix.x = 64 - 2^-10: in, trunc 63
    [0.0, -1.0 + 2.0 ** -14, 2.0],     # pix.y = 2^-10: in, trunc 0
    [0.0, 1.0 - 2.0 ** -14, 2.0],      # pix.y = 32 - 2^-10: in, trunc 31
    [-0.4765625, 0.171875, 2.0],       # pix (16.75, 18.75): in, trunc (16, 18) -- rounding gives (17, 19)
    [0.0, 0.0, 0.0],                   # z == 0 at the principal ray: 0 / 0
    [0.5, 0.25, -2.0],                 # behind the camera (pix would be in the frame)
])
# camera-space rows for camera B (projective last row of K): p_z = 4 cx + cz
PLANTED_B = np.array([
    [0.25, 0.25, 0.0],                 # z == 0 with p = (16, 8, 1): pix (16, 8) inside the frame, out by z > 0 alone
    [0.25, 0.25, 2.0 ** -10],          # one step in front: in, pix about (16.016, 8.008)
    [0.125, 0.25, 0.5],                # p = (24, 16, 1): pix (24, 16), in
])


def _to_world(cam_points, R, t):
    return (np.asarray(cam_points, np.float64) - t) @ R      # R^T (cam - t), row-wise


def _w2c(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m


def _random_rotation(rng):
    q = rng.normal(size=4)
    r, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def _general_camera(rng, h, w):
    K = np.array([[0.83 * w + rng.random(), 0.0, 0.5 * w + rng.normal()], [0.0, 0.79 * w + rng.random(), 0.5 * h + rng.normal()], [0.0, 0.0, 1.0]])
    return _random_rotation(rng), rng.normal(size=3) * 0.7, K


class PointCase(NamedTuple):
    name: str
    xyz: np.ndarray               # [P,3] float32, read-only
    cameras: U.FrameCameras       # CPU tensors
    robust: np.ndarray            # [F,P] bool
    random_rows: np.ndarray       # [P] bool: not planted (the 1 % condition is on these)
    kinds: tuple                  # per frame "A", "B" or "general"


def robustness(xyz, camera):
    """[P] bool: the decisions on every point of `xyz` (float32 numpy) in `camera` are robust by the bound of the module's docstring."""
    x = np.asarray(xyz, np.float64)
    M, K = camera.w2c.numpy().astype(np.float64), camera.K.numpy().astype(np.float64)
    R, t = M[:3, :3], M[:3, 3]
    with np.errstate(all="ignore"):
        cam = x @ R.T + t
        dc = _gamma(4) * (np.abs(x) @ np.abs(R).T + np.abs(t))
        p = cam @ K.T
        dp = dc @ np.abs(K).T + _gamma(3) * ((np.abs(cam) + dc) @ np.abs(K).T)
        pix = p[:, :2] / p[:, 2:3]
        B = (dp[:, :2] + np.abs(pix) * dp[:, 2:3]) / (np.abs(p[:, 2:3]) - dp[:, 2:3]) + 2 * U32 * np.abs(pix)
        B = np.where(np.abs(p[:, 2:3]) > dp[:, 2:3], B, np.inf)
        far = lambda v, edge, bound: np.abs(v - edge) > bound
        ok = far(pix[:, 0], 0, B[:, 0]) & far(pix[:, 0], camera.w, B[:, 0]) & far(pix[:, 1], 0, B[:, 1]) & far(pix[:, 1], camera.h, B[:, 1])
        ok &= far(cam[:, 2], 0, dc[:, 2])
        if camera.max_z is not None:
            ok &= far(cam[:, 2], camera.max_z, dc[:, 2])
        admitted = (pix[:, 0] > 0) & (pix[:, 0] < camera.w) & (pix[:, 1] > 0) & (pix[:, 1] < camera.h) & (cam[:, 2] > 0)
        # (max_z is not applied here: semantic_mask_of_points drops it, and its pixel index must be as stable as the lists')
        same_pixel = (np.floor(pix - B) == np.floor(pix + B)).all(axis=1)
        ok &= ~admitted | same_pixel
    finite = np.isfinite(x).all(axis=1)
    return np.where(finite, ok & np.isfinite(B).all(axis=1), True)      # a NaN or infinite row is in no frame for everyone


@functools.lru_cache(maxsize=None)
def point_case(name):
    """name = "<layout>_P<P>_F<F>_v<variant>": layout "mixed" (planted + special + random rows), "general" (a general camera alone) or "unseen"
    (every point behind every camera); the variant picks max_z and reso_scale."""
    layout, P, F, variant = name.split("_")
    P, F, variant = int(P[1:]), int(F[1:]), int(variant[1:])
    rng = np.random.default_rng(1000 * P + 10 * F + variant + (layout == "general"))
    kinds = {("mixed", 1): ("A", "B")[variant % 2:][:1], ("mixed", 3): ("A", "general", "B"), ("general", 1): ("general",), ("general", 3): ("general",) * 3,
             ("unseen", 1): ("A",), ("unseen", 3): ("A", "general", "B")}[(layout, F)]
    cams = []
    for f, kind in enumerate(kinds):
        h, w = FRAME_SIZES[f] if kind == "general" else FRAME_SIZES[0]
        if kind == "general":
            R, t, K = _general_camera(rng, h, w)
        else:
            R, t, K = R_PERM, T_DYADIC, (K_A if kind == "A" else K_B)
        max_z = (PLANTED_MAX_Z if kind != "general" else 9.5) if (variant + f) % 2 == 0 else None
        reso = (None, 1.0, 2.0)[(variant + f) % 3]
        cams.append((R, t, K, h, w, max_z, reso))
    rows, planted_for = [], []
    if layout == "mixed":
        for f, kind in enumerate(kinds):
            if kind != "general":
                block = _to_world(PLANTED_A if kind == "A" else PLANTED_B, cams[f][0], cams[f][1])
                rows += list(block)
                planted_for += [f] * len(block)
        if P == 1:
            rows, planted_for = rows[:1], planted_for[:1]
        rows, planted_for = rows[:P], planted_for[:P]
        special = [[np.nan, 0.0, 1.0], [0.5, np.inf, 0.25], [-np.inf, 0.0, 0.0], [np.inf, np.inf, np.inf]]
        for s in special[:max(0, P - len(rows))]:
            rows.append(s)
            planted_for.append(-1)
    n_random = P - len(rows)
    if n_random > 0:
        def random_row():
            R, t, K, h, w, _, _ = cams[rng.integers(len(cams))]
            z = -rng.uniform(0.5, 5.0) if layout == "unseen" else rng.uniform(-2.0, 12.0)
            pixel = np.array([rng.uniform(-0.2 * w, 1.2 * w), rng.uniform(-0.2 * h, 1.2 * h), 1.0])
            return _to_world((np.linalg.solve(K, pixel) * z)[None], R, t)[0]

        pts = np.stack([random_row() for _ in range(n_random)])
        if n_random < 200:      # one non-robust row of fewer than a hundred is more than the 1 % a case may hold: such a row is drawn again
            views = [U.FrameCamera(torch.tensor(_w2c(c[0], c[1]), dtype=torch.float32), torch.tensor(c[2], dtype=torch.float32), *c[3:]) for c in cams]
            for i in range(n_random):
                while not all(robustness(pts[i:i + 1].astype(np.float32), v)[0] for v in views):
                    pts[i] = random_row()
        rows += list(pts)
        planted_for += [-1] * n_random
    xyz = np.asarray(rows, dtype=np.float64).reshape(P, 3).astype(np.float32)
    cameras = U.FrameCameras(torch.tensor(np.stack([_w2c(c[0], c[1]) for c in cams]), dtype=torch.float32),
                             torch.tensor(np.stack([c[2] for c in cams]), dtype=torch.float32), [(c[3], c[4]) for c in cams],
                             [c[5] for c in cams], [c[6] for c in cams])
    planted_for = np.asarray(planted_for, dtype=np.int64).reshape(P)
    if layout == "unseen":          # drop to the points no frame admits (float64), then pad back to P by repeating them
        seen = np.zeros(P, dtype=bool)
        for f in range(F):
            seen |= U.points_in_frame_torch(torch.from_numpy(xyz), cameras.frame(f)).numpy()
        keep = xyz[~seen]
        xyz = keep[np.arange(P) % max(1, len(keep))] if len(keep) else xyz
    robust = np.stack([robustness(xyz, cameras.frame(f)) | (planted_for == f) for f in range(F)]) if F else np.zeros((0, P), bool)
    xyz.setflags(write=False)
    robust.setflags(write=False)
    return PointCase(name, xyz, cameras, robust, planted_for < 0, tuple(kinds))


POINT_CASES = tuple(f"mixed_P{P}_F{F}_v{v}" for P in (0, 1, 63, 64, 65, 4097) for F, v in ((1, 0), (1, 1), (3, 0), (3, 1))) + \
    ("general_P65_F1_v0", "general_P4097_F3_v1", "unseen_P65_F1_v0", "unseen_P65_F3_v1")
NONROBUST_SHARE = 1e-2


def xyz_tensor(case, device="cpu"):
    return torch.from_numpy(case.xyz.copy()).to(device)


@functools.lru_cache(maxsize=None)
def expected_in_frame(name, f):
    """the float64 checker on frame f -> (mask [P], pix [n,2] int64, depth [n] float64)"""
    c = point_case(name)
    mask, pix, depth = U.points_in_frame_torch(xyz_tensor(c), c.cameras.frame(f), True, torch.float64)
    return mask.numpy(), pix.numpy(), depth.numpy()


def robust_cloud(name):
    """-> float32 [n,3]: the rows of the case that are robust in every frame (what frame_visibility, pick_view and the lists run on)"""
    c = point_case(name)
    return np.ascontiguousarray(c.xyz[c.robust.all(axis=0)] if c.robust.shape[0] else c.xyz)


def depth_bar(truth, twin):
    """Per element: twice the float32 twin's own deviation from float64, floor half an ulp (of the float32 value)."""
    truth = np.asarray(truth, np.float64)
    return np.maximum(2 * np.abs(np.asarray(twin, np.float64) - truth), 0.5 * np.spacing(np.abs(truth).astype(np.float32)).astype(np.float64))


def compare_in_frame(name, f, mask, label):
    c = point_case(name)
    want = expected_in_frame(name, f)[0]
    mask = np.asarray(mask)
    assert mask.dtype == np.bool_ and mask.shape == want.shape, (label, name, f, mask.dtype, mask.shape)
    r = c.robust[f]
    assert np.array_equal(mask[r], want[r]), f"{label} {name} frame {f}: {int((mask != want)[r].sum())} robust points decided differently"


def compare_lists(xyz, camera, mask, pix, depth, label):
    """On an all-robust cloud: mask, order and pix exactly the float64 checker's; depth within the bar of the float32 twin (CPU)."""
    t = torch.from_numpy(np.array(xyz))
    want_mask, want_pix, want_depth = U.points_in_frame_torch(t, camera, True, torch.float64)
    _, _, twin_depth = U.points_in_frame_torch(t, camera, True, torch.float32)
    assert np.array_equal(np.asarray(mask), want_mask.numpy()), f"{label}: mask"
    pix, depth = np.asarray(pix), np.asarray(depth)
    assert pix.dtype == np.int64 and pix.shape == tuple(want_pix.shape), (label, pix.dtype, pix.shape, tuple(want_pix.shape))
    assert np.array_equal(pix, want_pix.numpy()), f"{label}: pix (or the order of the rows)"
    assert depth.shape == tuple(want_depth.shape)
    twin = twin_depth.numpy() if twin_depth.shape == want_depth.shape else want_depth.numpy()
    err = np.abs(depth.astype(np.float64) - want_depth.numpy())
    assert (err <= depth_bar(want_depth.numpy(), twin)).all(), f"{label}: depth off by {err.max():.3e}"


def compare_visibility(xyz, cameras, count, depth_sum, label, max_z="keep"):
    t = torch.from_numpy(np.array(xyz))
    want_count, want_sum = U.frame_visibility_torch(t, cameras, max_z, torch.float64)
    _, twin_sum = U.frame_visibility_torch(t, cameras, max_z, torch.float32)
    count, depth_sum = np.asarray(count), np.asarray(depth_sum)
    assert count.dtype == np.int64 and depth_sum.dtype == np.float64
    assert np.array_equal(count, want_count.numpy()), f"{label}: counts {count.tolist()} != {want_count.tolist()}"
    # the floor of a sum: half an ulp of every float32 depth it adds
    floor = np.zeros(len(want_count))
    for f, camera in enumerate(U._frames(cameras)):
        in_frame, _, depth = U.project_torch(t, camera if max_z == "keep" else camera._replace(max_z=max_z), torch.float64)
        floor[f] = 0.5 * np.spacing(depth[in_frame].numpy().astype(np.float32)).astype(np.float64).sum()
    bar = np.maximum(2 * np.abs(twin_sum.numpy() - want_sum.numpy()), floor)
    assert (np.abs(depth_sum - want_sum.numpy()) <= bar).all(), f"{label}: depth_sum {depth_sum.tolist()} vs {want_sum.tolist()}"


# pick_view: clouds in front of one chosen frame of three general cameras; the float64 rule is the expectation
@functools.lru_cache(maxsize=None)
def pick_case(name):
    """-> (xyz float32 [P,3] all-robust, cameras): "near_f1" (rule 1 picks frame 1), "far_f2" (mean depth >= 4: rule 2), "half" (60 % of
    the cloud in frame 1, too few for rule 1), "unseen" (-1), "empty" (P = 0)."""
    rng = np.random.default_rng(77)
    cams = [_general_camera(rng, *FRAME_SIZES[f]) for f in range(3)]
    cameras = U.FrameCameras(torch.tensor(np.stack([_w2c(R, t) for R, t, _ in cams]), dtype=torch.float32),
                             torch.tensor(np.stack([K for _, _, K in cams]), dtype=torch.float32), list(FRAME_SIZES), None, None)

    def cloud(f, n, z_lo, z_hi):
        R, t, K = cams[f]
        h, w = FRAME_SIZES[f]
        z = rng.uniform(z_lo, z_hi, n)
        pixel = np.stack([rng.uniform(0.3 * w, 0.7 * w, n), rng.uniform(0.3 * h, 0.7 * h, n), np.ones(n)], axis=1)
        return _to_world(np.linalg.solve(K, pixel.T).T * z[:, None], R, t)

    if name == "near_f1":
        pts = cloud(1, 300, 2.0, 3.5)
    elif name == "far_f2":
        pts = cloud(2, 300, 5.0, 8.0)
    elif name == "half":
        pts = np.concatenate([cloud(1, 180, 2.0, 3.5), cloud(1, 120, -6.0, -3.0)])
    elif name == "unseen":
        pts = np.concatenate([cloud(0, 100, -6.0, -3.0), cloud(1, 100, 30.0, 40.0)])      # behind one, beyond max_z of another
    else:
        pts = np.zeros((0, 3))
    xyz = pts.astype(np.float32).reshape(-1, 3)
    robust = np.ones(len(xyz), dtype=bool)
    for f in range(3):
        robust &= robustness(xyz, cameras.frame(f)._replace(max_z=10.0))
    xyz = np.ascontiguousarray(xyz[robust])
    xyz.setflags(write=False)
    return xyz, cameras


PICK_CASES = ("near_f1", "far_f2", "half", "unseen", "empty")


def pick_expected(name):
    xyz, cameras = pick_case(name)
    return U.pick_view_torch(torch.from_numpy(xyz.copy()), cameras, 10.0, torch.float64)


# semantic maps
REMAIN_BIT = 0x55555555 | (1 << 31)      # every other label of 0..30 remains (bit 31 is ignored)


@functools.lru_cache(maxsize=None)
def semantic_maps(name, undersized=False):
    """uint8 [F,Hm,Wm] labels in 0..40 (31 and more match nothing); sized for the largest frame, or -- undersized -- for a quarter of it"""
    c = point_case(name)
    F = len(c.cameras)
    Hm, Wm = max(h for h, _ in c.cameras.hw), max(w for _, w in c.cameras.hw)
    if undersized:
        Hm, Wm = Hm // 4, Wm // 4
    maps = np.random.default_rng(3).integers(0, 41, size=(F, Hm, Wm)).astype(np.uint8)
    maps.setflags(write=False)
    return maps


def semantic_expected(xyz, cameras, maps):
    mask, outside = U.semantic_mask_of_points_torch(torch.from_numpy(np.array(xyz)), cameras, torch.from_numpy(np.array(maps)), REMAIN_BIT, torch.float64)
    return mask.numpy(), int(outside)

"""The cases of the frame resize (streetunveiler_amd/frames.py, csrc/resize.hip), shared by tests/test_frames_host.py,
tests/test_gpu_frames.py and tools/make_frames_golden.py, and their stored answers: tests/golden/frames_golden.npz holds what Pillow's own
`Image.resize` gave for every case on the machine that made it (its version is in the file), so a machine without Pillow still checks
against Pillow.

A case is (frames, input size, output size, channels, filter, fill).  The fills: seeded random bytes; a 0 / 255 checkerboard of period 1
and one of period 3, on which the cubic overshoots and the clamp works at both ends; all 255 and all 0 -- the rounded coefficients need not
sum to 2^22, so a constant picture need not stay constant: whatever Pillow gives is right.

The sizes (H, W) -> (h, w): the degenerate ones (one pixel in, one pixel out), up- and downscales with odd sizes, each pass left out once
and both (a copy), the exact quarter, a table 401 wide in either axis, a batch of three frames, and two pairs whose OUTPUT crosses the
kernels' tile seams in both axes by one sample: a tile is 64 samples of a row x 4 rows, a row's samples its w C bytes (uint8 output) or its
w pixels (float output) -- 5 x 43 x 3 = 5 rows of 129 bytes, and 5 x 65 x 1 = 5 rows of 65 bytes and of 65 pixels."""
import functools
import os
import zlib
from typing import NamedTuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_golden.npz")


class Size(NamedTuple):
    frames: int          # 0: one picture without a batch dimension
    src: tuple           # (H, W)
    dst: tuple           # (h, w)

    @property
    def name(self):
        return (f"n{self.frames}-" if self.frames else "") + f"{self.src[0]}x{self.src[1]}-{self.dst[0]}x{self.dst[1]}"


SIZES = [Size(0, *p) for p in [((1, 1), (4, 4)), ((5, 7), (1, 1)), ((3, 2), (11, 9)), ((16, 16), (16, 4)), ((40, 60), (13, 60)),
                               ((33, 50), (33, 50)), ((37, 53), (9, 13)), ((64, 96), (16, 24)), ((20, 31), (47, 64)), ((200, 3), (2, 3)),
                               ((3, 200), (3, 2)), ((11, 90), (5, 43)), ((9, 131), (5, 65))]] + [Size(3, (37, 53), (9, 13))]
SIZE_NAMES = [s.name for s in SIZES]
# (channels, filter, fill) of every size: the four (channels, filter) pairs on random bytes, the checkerboards and the constants on two each
VARIANTS = [(3, "bicubic", "random"), (1, "bicubic", "random"), (3, "bilinear", "random"), (1, "bilinear", "random"),
            (3, "bicubic", "checker1"), (1, "bilinear", "checker1"), (1, "bicubic", "checker3"), (3, "bilinear", "checker3"),
            (3, "bicubic", "all255"), (1, "bilinear", "all255"), (3, "bicubic", "all0")]


class Case(NamedTuple):
    size: Size
    channels: int
    resample: str
    fill: str

    @property
    def name(self):
        return f"{self.size.name}-c{self.channels}-{self.resample}-{self.fill}"

    @property
    def wh(self):        # Pillow's (w, h)
        return (self.size.dst[1], self.size.dst[0])


CASES = [Case(s, *v) for s in SIZES for v in VARIANTS]
BY_NAME = {c.name: c for c in CASES}


def cases_of(size_name):
    return [c for c in CASES if c.size.name == size_name]


def image(case):
    """uint8 [H,W] (one channel), [H,W,3], or [N,H,W,C] for a batch; the same bytes on every machine."""
    (H, W), C, n = case.size.src, case.channels, max(case.size.frames, 1)
    if case.fill == "random":
        a = np.random.default_rng(zlib.crc32(case.name.encode())).integers(0, 256, (n, H, W, C), dtype=np.uint8)
    elif case.fill.startswith("checker"):
        p = int(case.fill[len("checker"):])
        f, y, x, c = np.indices((n, H, W, C))
        a = ((((y // p) + (x // p) + f + c) % 2) * 255).astype(np.uint8)      # every channel and frame its own phase
    else:
        a = np.full((n, H, W, C), 255 if case.fill == "all255" else 0, dtype=np.uint8)
    if case.size.frames:
        return np.ascontiguousarray(a)      # a batch keeps its channel dimension: [N,H,W,1] is not [H,W,3]
    return np.ascontiguousarray(a[0, :, :, 0] if C == 1 else a[0])


@functools.lru_cache(maxsize=1)
def golden():
    """{case name: Pillow's output} + "pillow_version"; read once."""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def expected(case):
    return golden()[case.name]


def float_chw(u8, case):
    """The reference's lines on a resized uint8 picture: torch.from_numpy(u8) / 255.0, permuted to [C,h,w] ([N,C,h,w]); float32, IEEE."""
    a = u8 if case.channels == 3 or case.size.frames else u8[..., None]
    a = np.moveaxis(a, -1, -3)
    return np.ascontiguousarray(a).astype(np.float32) / np.float32(255.0)


# ---- nearest label maps: the same size pairs, three dtypes, + one pair at which a float64 scale picks another source row ---------------
LABEL_DTYPES = ["uint8", "int32", "int64"]
LABEL_SIZES = SIZES + [Size(0, (3, 6), (123, 74))]


def label_map(size, dtype):
    """Labels whose value names their own position (so a wrong source index shows), of the given dtype; int32 / int64 also carry negative
    values and values beyond 2^31 (int64) -- the elements are copied as they are."""
    (H, W), n = size.src, max(size.frames, 1)
    f, y, x = np.indices((n, H, W))
    v = (y * W + x) * 7 + f
    if dtype == "uint8":
        a = (v % 251).astype(np.uint8)
    elif dtype == "int32":
        a = np.where(v % 3 == 0, -v, v * 1000003 % (1 << 31)).astype(np.int32)
    else:
        a = np.where(v % 3 == 0, -v, v * ((1 << 40) + 12345)).astype(np.int64)
    return np.ascontiguousarray(a if size.frames else a[0])

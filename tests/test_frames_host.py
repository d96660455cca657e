"""CPU: the checkers of the frame resize (streetunveiler_amd/frames.py) against Pillow -- the stored outputs of tests/golden/frames_golden.npz
on every case, a live Pillow where one is importable -- and against torch's nearest rule; the float epilogue against the reference's
division; and the bar itself: exact equality, shown rejecting wrong implementations, each on a named case.

The mutants are a second implementation (`_resize` below, dense coefficient matrices, every deviation behind a flag) that equals the checker
with no flag set.  One mutant of the issue's list is DROPPED: coefficients rounded half-to-even.  It differs from Pillow's rounding only
where w 2^22 lies exactly half-way between two integers, which no table of any case does (test_no_case_has_a_coefficient_tie shows it), so
no case can tell it apart; truncated coefficients are told apart and stay."""
import numpy as np
import pytest
import torch

from streetunveiler_amd import frames as F
from tests import frames_cases as fc


@pytest.mark.parametrize("size_name", fc.SIZE_NAMES)
def test_checker_equals_the_stored_pillow_outputs(size_name):
    for c in fc.cases_of(size_name):
        got = F.resize_u8_numpy(fc.image(c), c.wh, c.resample)
        want = fc.expected(c)
        assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), c.name


def test_golden_file_names_its_pillow_and_holds_every_case():
    g = fc.golden()
    assert str(g["pillow_version"]) and sorted(k for k in g if k != "pillow_version") == sorted(fc.BY_NAME)


def test_checker_equals_a_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    how = {"bicubic": Image.Resampling.BICUBIC, "bilinear": Image.Resampling.BILINEAR}
    for c in fc.CASES:
        if c.size.frames:
            continue
        a = fc.image(c)
        want = np.array(Image.fromarray(a).resize(c.wh, resample=how[c.resample]))
        assert F.resize_u8_numpy(a, c.wh, c.resample).tobytes() == want.tobytes(), c.name
    a = fc.image(fc.BY_NAME["37x53-9x13-c3-bicubic-random"])
    assert np.array_equal(F.resize_u8_numpy(a, (13, 9)), np.array(Image.fromarray(a).resize((13, 9))))      # no `resample`: bicubic


def test_tables_are_as_wide_as_the_ratio_asks():
    bounds, coeffs = F.resize_tables(200, 2, "bicubic")
    assert coeffs.shape == (2, 401) and bounds.dtype == np.int32 and coeffs.dtype == np.int32
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 200).all() and (bounds[:, 1] <= 401).all()
    bounds, coeffs = F.resize_tables(20, 47, "bilinear")
    assert coeffs.shape == (47, 3) and (bounds[:, 0] + bounds[:, 1] <= 20).all()


@pytest.mark.parametrize("dtype", fc.LABEL_DTYPES)
def test_label_checker_equals_torch_nearest(dtype):
    for size in fc.LABEL_SIZES:
        a = fc.label_map(size, dtype)
        got = F.resize_labels_numpy(a, (size.dst[1], size.dst[0]))
        assert got.dtype == a.dtype
        # torch's CPU kernel takes uint8 and floats, and computes the scale in the tensor's own float type: the int32 and int64 maps go
        # through the float32 map of their own positions (below 2^24: exact), which the rule then gathers
        src = a if dtype == "uint8" else np.arange(a.size, dtype=np.float32).reshape(a.shape)
        t = torch.from_numpy(src)
        t4 = t[None] if size.frames else t[None, None]
        want = torch.nn.functional.interpolate(t4, size=size.dst, mode="nearest")[0].numpy()
        want = want if size.frames else want[0]
        if dtype != "uint8":
            want = a.reshape(-1)[want.astype(np.int64)]
        assert np.array_equal(got, want.astype(a.dtype)), (size.name, dtype)


def test_float_epilogue_is_the_references_division():
    c = fc.BY_NAME["20x31-47x64-c3-bicubic-random"]
    u8 = fc.expected(c)
    want = (torch.from_numpy(u8) / 255.0).permute(2, 0, 1).contiguous().numpy()
    got = F.resize_u8_numpy(fc.image(c), c.wh, c.resample, out="f32_chw")
    assert got.dtype == np.float32 and got.shape == (3, 47, 64) and got.tobytes() == want.tobytes()
    assert fc.float_chw(u8, c).tobytes() == want.tobytes()
    one = fc.BY_NAME["20x31-47x64-c1-bicubic-random"]
    assert F.resize_u8_numpy(fc.image(one), one.wh, out="f32_chw").shape == (1, 47, 64)
    # over all 256 bytes a product with the float32 reciprocal of 255 misses the IEEE quotient on 126 of them, 3 the first
    v = np.arange(256, dtype=np.float32)
    wrong = np.nonzero(v * (np.float32(1.0) / np.float32(255.0)) != v / np.float32(255.0))[0]
    assert len(wrong) == 126 and wrong[0] == 3
    assert (torch.arange(256, dtype=torch.uint8) / 255.0).numpy().tobytes() == (v / np.float32(255.0)).tobytes()
    assert (u8 == 3).any()      # ... and the case above holds such a byte: the reciprocal product is a mutant it rejects
    assert (np.moveaxis(u8, -1, 0).astype(np.float32) * (np.float32(1.0) / np.float32(255.0))).tobytes() != want.tobytes()


def test_binarise_is_the_stages_mask_line():
    c = fc.BY_NAME["20x31-47x64-c1-bilinear-checker1"]
    want = fc.expected(c).copy()
    want[want > 0] = 255
    assert np.array_equal(F.resize_u8_numpy(fc.image(c), c.wh, "bilinear", binarise=True), want)


def test_refusals_of_the_checkers():
    a = np.zeros((4, 5, 3), dtype=np.uint8)
    for bad in (np.zeros((4, 5, 2), np.uint8), np.zeros((4, 5, 4), np.uint8), np.zeros((4, 5, 3), np.float32), np.zeros((1, 2, 4, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            F.resize_u8_numpy(bad, (3, 3))
    for size in ((0, 3), (3, -1)):
        with pytest.raises(ValueError):
            F.resize_u8_numpy(a, size)
        with pytest.raises(ValueError):
            F.resize_labels_numpy(a[..., 0], size)
    with pytest.raises(ValueError, match="binarise"):
        F.resize_u8_numpy(a, (3, 3), out="f32_chw", binarise=True)
    with pytest.raises(ValueError, match="Lanczos"):
        F.resize_u8_numpy(a, (3, 3), "lanczos")
    with pytest.raises(ValueError, match="GPU"):
        F.resize_u8(torch.zeros(4, 5, 3, dtype=torch.uint8), (3, 3))
    with pytest.raises(ValueError, match="GPU"):
        F.resize_labels(torch.zeros(4, 5, dtype=torch.uint8), (3, 3))


def test_argument_refusals_of_the_c_abi_without_a_gpu():
    """What the entry points refuse before they touch a device: sizes, channels, flags, NULL."""
    from streetunveiler_amd import _lib as L
    from streetunveiler_amd.build import build
    build()
    lib = L.load()
    p = lambda *a: lib.sr_resize_u8_pass(*a)
    ok = dict(N=1, H=4, W=4, C=3, src=None, bs=0, rs=12, axis=0, out_size=2, bounds=None, coeffs=None, ksize=5, flags=0, out=None, stream=None)
    for change, code, text in [({"C": 2}, -4, b"1 or 3"), ({"C": 4}, -4, b"premultiplied"), ({"out_size": 0}, -1, b"out_size"), ({"H": 0}, -1, b"at least 1"),
                               ({"axis": 2}, -1, b"axis"), ({"flags": 3}, -1, b"SR_RESIZE_BINARISE"), ({"flags": 8}, -1, b"unknown bits"),
                               ({"rs": 11}, -1, b"dense row"), ({"ksize": 0}, -1, b"ksize"), ({}, -1, b"in is NULL")]:
        assert p(*dict(ok, **change).values()) == code and text in lib.sr_last_error(), change
    n = lambda *a: lib.sr_resize_nearest(*a)
    assert n(1, 4, 4, 2, None, 0, 4, 2, 2, None, None) == -4 and b"elem_bytes" in lib.sr_last_error()
    assert n(1, 4, 4, 4, None, 0, 4, 0, 2, None, None) == -1 and b"at least 1" in lib.sr_last_error()
    assert n(1, 4, 4, 4, None, 0, 4, 2, 2, None, None) == -1 and b"in is NULL" in lib.sr_last_error()


# ---- the bar rejects wrong implementations ---------------------------------------------------------------------------------------------
def _matrices(in_size, out_size, resample, m):
    """Dense [out_size, in_size] matrices of one pass: the float64 weights and the integer coefficients, every deviation behind a flag of m."""
    sup = 2.0 if resample == "bicubic" else 1.0
    a = m.get("a", -0.5)

    def f(x):
        x = abs(x)
        if resample == "bilinear":
            return 1.0 - x if x < 1.0 else 0.0
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        return (((x - 5) * x + 8) * x - 4) * a if x < 2.0 else 0.0
    scale = in_size / out_size
    fs = 1.0 if m.get("no_antialias") else max(scale, 1.0)
    support, ss = sup * fs, 1.0 / fs
    wf, ki = np.zeros((out_size, in_size)), np.zeros((out_size, in_size), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + (0.0 if m.get("center_without_half") else 0.5)) * scale
        lo = center - support + 0.5
        xmin = max(int(round(lo)) if m.get("xmin_rounded") else int(lo), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            wf[xx, xmin + x] = v
            s = v * (1 << 22)
            ki[xx, xmin + x] = {"half_even": round(s), "truncated": int(s)}.get(m.get("coefficients"), int(0.5 + s) if v >= 0 else int(-0.5 + s))
    return wf, ki


def _finish(acc, m):
    """The 32-bit sum (already holding 2^21) -> the byte."""
    acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)              # two's complement, 32 bits
    v = (acc % (1 << 32)) >> 22 if m.get("logical_shift") else acc >> 22
    return (v % 256 if m.get("no_clamp") else np.clip(v, 0, 255)).astype(np.uint8)


def _resize(image, wh, resample, **m):
    """One picture [H,W] or [H,W,C] -> Pillow's resize, or a deliberately wrong one."""
    img = image.astype(np.int64)
    passes = [(1, wh[0]), (0, wh[1])]
    if m.get("vertical_first"):
        passes.reverse()
    passes = [(axis, n) for axis, n in passes if n != image.shape[axis]]
    if m.get("no_uint8_between") and len(passes) == 2:             # integer coefficients, the first pass's sum kept whole
        (a0, n0), (a1, n1) = passes
        k0, k1 = _matrices(image.shape[a0], n0, resample, m)[1], _matrices(image.shape[a1], n1, resample, m)[1]
        whole = np.moveaxis(np.tensordot(k1, np.moveaxis(np.moveaxis(np.tensordot(k0, np.moveaxis(img, a0, 0), 1), 0, a0), a1, 0), 1), 0, a1)
        return np.clip(((1 << 43) + whole) >> 44, 0, 255).astype(np.uint8)
    for axis, n in passes:
        wf, ki = _matrices(img.shape[axis], n, resample, m)
        moved = np.moveaxis(img, axis, 0)
        if m.get("float_accumulation"):
            out = np.clip(np.rint(np.tensordot(wf, moved.astype(np.float64), 1)), 0, 255).astype(np.uint8)
        else:
            out = _finish((1 << 21) + np.tensordot(ki, moved, 1), m)
        img = np.moveaxis(out, 0, axis).astype(np.int64)
    return img.astype(np.uint8)


def test_the_second_implementation_equals_the_checker():
    for c in fc.CASES:
        if not c.size.frames and c.fill in ("random", "checker1"):
            assert _resize(fc.image(c), c.wh, c.resample).tobytes() == fc.expected(c).tobytes(), c.name


def test_no_case_has_a_coefficient_tie():
    """Why `coefficients rounded half-to-even` is not in MUTANTS: it gives every case's tables bit for bit."""
    for c in fc.CASES:
        if not c.size.frames and c.fill == "random":
            for axis, n in ((1, c.wh[0]), (0, c.wh[1])):
                plain, even = (_matrices(c.size.src[axis], n, c.resample, m)[1] for m in ({}, {"coefficients": "half_even"}))
                assert np.array_equal(plain, even), c.name


MUTANTS = [
    ({"float_accumulation": True}, "3x2-11x9-c3-bicubic-random"),
    ({"no_uint8_between": True}, "37x53-9x13-c3-bicubic-random"),
    ({"vertical_first": True}, "37x53-9x13-c3-bicubic-random"),
    ({"a": -0.75}, "20x31-47x64-c3-bicubic-random"),
    ({"no_antialias": True}, "64x96-16x24-c3-bicubic-random"),
    ({"coefficients": "truncated"}, "37x53-9x13-c3-bilinear-random"),
    ({"center_without_half": True}, "64x96-16x24-c3-bicubic-random"),
    ({"xmin_rounded": True}, "37x53-9x13-c3-bicubic-random"),
    ({"logical_shift": True}, "20x31-47x64-c3-bicubic-checker1"),
    ({"no_clamp": True}, "20x31-47x64-c3-bicubic-checker1"),
]


@pytest.mark.parametrize("flags,case_name", MUTANTS, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in MUTANTS])
def test_exact_equality_rejects_the_mutant(flags, case_name):
    c = fc.BY_NAME[case_name]
    assert _resize(fc.image(c), c.wh, c.resample).tobytes() == fc.expected(c).tobytes()
    wrong = _resize(fc.image(c), c.wh, c.resample, **flags)
    assert wrong.shape == fc.expected(c).shape and wrong.tobytes() != fc.expected(c).tobytes(), (flags, case_name)


def test_exact_equality_rejects_the_nearest_mutants():
    """A float64 scale, and round() in place of floor(): each picks another source index on a named pair."""
    def index(in_size, out_size, dtype=np.float32, rule=np.floor):
        return np.minimum(rule(np.arange(out_size, dtype=dtype) * (dtype(in_size) / dtype(out_size))).astype(np.int64), in_size - 1)
    size = next(s for s in fc.LABEL_SIZES if s.name == "3x6-123x74")
    a = fc.label_map(size, "int32")
    want = F.resize_labels_numpy(a, (74, 123))
    assert np.array_equal(want, a[index(3, 123)[:, None], index(6, 74)[None, :]])
    assert not np.array_equal(want, a[index(3, 123, np.float64)[:, None], index(6, 74, np.float64)[None, :]])
    size = next(s for s in fc.LABEL_SIZES if s.name == "37x53-9x13")
    a = fc.label_map(size, "uint8")
    assert not np.array_equal(F.resize_labels_numpy(a, (13, 9)), a[index(37, 9, rule=np.rint)[:, None], index(53, 13, rule=np.rint)[None, :]])

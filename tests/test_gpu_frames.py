"""-m gpu: the frame resize (csrc/resize.hip) on every case of tests/frames_cases.py, everything exactly -- through resize_u8 /
resize_labels twice (equal inputs, equal bits) and through the raw C-ABI on caller-owned, sentinel-filled buffers one row larger than
needed, whose guard row must come back untouched --, non-contiguous and batched inputs, a non-default stream, pil_to_torch / frame_tensor
against the reference's three lines run on the checker's output, the 255 / 0 mask, and every refusal.  The answers are Pillow's own
(tests/golden/frames_golden.npz); the float outputs are held bit for bit to the IEEE division of those bytes."""
import numpy as np
import pytest
import torch

from streetunveiler_amd import _lib as L
from streetunveiler_amd import frames as F
from streetunveiler_amd._call import call, ptr
from tests import frames_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_U8, GUARD_F32 = 0xA5, -7.0


def _dev(a):
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("size_name", fc.SIZE_NAMES)
def test_every_case_through_the_function_twice(size_name):
    for c in fc.cases_of(size_name):
        img = _dev(fc.image(c))
        want = fc.expected(c)
        got = F.resize_u8(img, c.wh, c.resample)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape, c.name
        assert got.cpu().numpy().tobytes() == want.tobytes(), c.name
        flt = F.resize_u8(img, c.wh, c.resample, out="f32_chw")
        want_f = fc.float_chw(want, c)
        assert flt.dtype == torch.float32 and tuple(flt.shape) == want_f.shape, c.name
        assert flt.cpu().numpy().tobytes() == want_f.tobytes(), c.name
        assert F.resize_u8(img, c.wh, c.resample).cpu().numpy().tobytes() == want.tobytes(), c.name
        assert F.resize_u8(img, c.wh, c.resample, out="f32_chw").cpu().numpy().tobytes() == want_f.tobytes(), c.name


def _raw_resize(img, wh, resample, flags):
    """The C-ABI sequence a caller without the wrapper makes on a contiguous [N,H,W,C] device tensor; every output buffer has one row more
    than the pass writes, filled with a sentinel like the rest of it."""
    dev = img.device
    N, H, W, C = (int(v) for v in img.shape)
    w, h = wh
    passes = ([(0, w)] if w != W else []) + ([(1, h)] if h != H else []) or [(-1, 0)]
    bs, rs = H * W * C, W * C
    for i, (axis, out_size) in enumerate(passes):
        last = i == len(passes) - 1
        oh, ow = (out_size if axis == 1 else H), (out_size if axis == 0 else W)
        if last and flags & L.SR_RESIZE_F32_CHW:
            out, rows = torch.full((N * C * oh + 1, ow), GUARD_F32, dtype=torch.float32, device=dev), N * C * oh
        else:
            out, rows = torch.full((N * oh + 1, ow, C), GUARD_U8, dtype=torch.uint8, device=dev), N * oh
        bounds = coeffs = None
        ksize = 0
        if axis >= 0:
            b, k = F.resize_tables(W if axis == 0 else H, out_size, resample)
            bounds, coeffs, ksize = _dev(b), _dev(k), k.shape[1]
        call("sr_resize_u8_pass", dev, N, H, W, C, ptr(img), bs, rs, axis, out_size, ptr(bounds), ptr(coeffs), ksize, flags if last else 0, ptr(out))
        guard = out[rows].cpu().numpy()
        assert (guard == (GUARD_F32 if out.dtype == torch.float32 else GUARD_U8)).all(), "the guard row was written"
        img, H, W, bs, rs = out[:rows], oh, ow, oh * ow * C, ow * C
    return img.cpu().numpy()


@pytest.mark.parametrize("size_name", fc.SIZE_NAMES)
def test_every_case_through_the_raw_abi_with_a_guard_row(size_name):
    for c in fc.cases_of(size_name):
        a = fc.image(c)
        nhwc = a if c.size.frames else (a[None, :, :, None] if a.ndim == 2 else a[None])
        img = _dev(np.ascontiguousarray(nhwc))
        want = fc.expected(c)
        assert _raw_resize(img, c.wh, c.resample, 0).tobytes() == want.tobytes(), c.name
        assert _raw_resize(img, c.wh, c.resample, L.SR_RESIZE_F32_CHW).tobytes() == fc.float_chw(want, c).tobytes(), c.name
        mask = np.where(want > 0, 255, 0).astype(np.uint8)
        assert _raw_resize(img, c.wh, c.resample, L.SR_RESIZE_BINARISE).tobytes() == mask.tobytes(), c.name


@pytest.mark.parametrize("dtype", fc.LABEL_DTYPES)
def test_label_maps_through_the_function_twice_and_the_raw_abi(dtype):
    for size in fc.LABEL_SIZES:
        a = fc.label_map(size, dtype)
        (h, w), n = size.dst, max(size.frames, 1)
        want = F.resize_labels_numpy(a, (w, h))
        maps = _dev(a)
        got = F.resize_labels(maps, (w, h))
        assert got.is_cuda and got.dtype == maps.dtype and tuple(got.shape) == want.shape, (size.name, dtype)
        assert got.cpu().numpy().tobytes() == want.tobytes(), (size.name, dtype)
        assert F.resize_labels(maps, (w, h)).cpu().numpy().tobytes() == want.tobytes(), (size.name, dtype)
        H, W = size.src
        out = torch.full((n * h + 1, w), -91 if dtype != "uint8" else GUARD_U8, dtype=maps.dtype, device=DEV)
        call("sr_resize_nearest", maps.device, n, H, W, maps.element_size(), ptr(maps), H * W, W, h, w, ptr(out))
        assert out[:n * h].cpu().numpy().tobytes() == want.tobytes(), (size.name, dtype)
        assert (out[n * h] == (-91 if dtype != "uint8" else GUARD_U8)).all(), (size.name, dtype)


def test_non_contiguous_and_batched_inputs():
    c = fc.BY_NAME["n3-37x53-9x13-c3-bicubic-random"]
    a, want = fc.image(c), fc.expected(c)
    # rows and frames of a larger allocation: taken through their strides
    big = torch.zeros((3, 80, 53, 3), dtype=torch.uint8, device=DEV)
    big[:, ::2][:, :37] = _dev(a)
    view = big[:, ::2][:, :37]
    assert not view.is_contiguous() and view[0, 0].is_contiguous()
    assert F.resize_u8(view, c.wh).cpu().numpy().tobytes() == want.tobytes()
    assert F.resize_u8(view[1], c.wh).cpu().numpy().tobytes() == want[1].tobytes()
    assert F.resize_u8(_dev(a)[1:2].expand(3, -1, -1, -1), c.wh).cpu().numpy().tobytes() == np.stack([want[1]] * 3).tobytes()
    # pixels that are not dense (a [C,H,W] picture permuted, every other column): copied once
    chw = _dev(np.ascontiguousarray(np.moveaxis(a[0], -1, 0)))
    assert F.resize_u8(chw.permute(1, 2, 0), c.wh).cpu().numpy().tobytes() == want[0].tobytes()
    wide = torch.zeros((37, 106, 3), dtype=torch.uint8, device=DEV)
    wide[:, ::2] = _dev(a[2])
    assert F.resize_u8(wide[:, ::2], c.wh, out="f32_chw").cpu().numpy().tobytes() == fc.float_chw(want[2], c._replace(size=c.size._replace(frames=0))).tobytes()
    # label maps likewise
    m = fc.label_map(c.size, "int32")
    wide_m = torch.zeros((3, 37, 106), dtype=torch.int32, device=DEV)
    wide_m[:, :, :53] = _dev(m)
    assert F.resize_labels(wide_m[:, :, :53], c.wh).cpu().numpy().tobytes() == F.resize_labels_numpy(m, c.wh).tobytes()
    assert F.resize_labels(_dev(m).transpose(1, 2), (9, 13)).cpu().numpy().tobytes() == F.resize_labels_numpy(m.transpose(0, 2, 1), (9, 13)).tobytes()


def test_a_non_default_stream():
    c = fc.BY_NAME["64x96-16x24-c3-bicubic-random"]
    img, s = _dev(fc.image(c)), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    got = F.resize_u8(img, c.wh, stream=s)
    flt = F.resize_u8(img, c.wh, out="f32_chw", stream=s)
    lab = F.resize_labels(img[..., 0], c.wh, stream=s)
    s.synchronize()
    assert got.cpu().numpy().tobytes() == fc.expected(c).tobytes()
    assert flt.cpu().numpy().tobytes() == fc.float_chw(fc.expected(c), c).tobytes()
    assert lab.cpu().numpy().tobytes() == F.resize_labels_numpy(fc.image(c)[..., 0], c.wh).tobytes()


def test_pil_to_torch_and_frame_tensor_are_the_references_lines():
    c = fc.BY_NAME["37x53-9x13-c3-bicubic-random"]
    a = fc.image(c)
    resized = torch.from_numpy(F.resize_u8_numpy(a, c.wh)) / 255.0                      # [REF utils/general_utils.py:22-25]
    want = resized.permute(2, 0, 1).contiguous().numpy()
    for given in (a, torch.from_numpy(a), _dev(a)):
        got = F.pil_to_torch(given, c.wh)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 9, 13)
        assert got.cpu().numpy().tobytes() == want.tobytes()
    stage = torch.from_numpy(F.resize_u8_numpy(a, c.wh)).permute(2, 0, 1) / 255.       # [REF 3_reoptimization/1_optimization.py:175]
    assert F.frame_tensor(a, c.wh).cpu().numpy().tobytes() == stage.contiguous().numpy().tobytes()
    grey = fc.BY_NAME["37x53-9x13-c1-bicubic-random"]
    g = fc.image(grey)
    want_g = (torch.from_numpy(F.resize_u8_numpy(g, grey.wh)) / 255.0).unsqueeze(dim=-1).permute(2, 0, 1).contiguous().numpy()
    got_g = F.pil_to_torch(g, grey.wh)
    assert tuple(got_g.shape) == (1, 9, 13) and got_g.cpu().numpy().tobytes() == want_g.tobytes()
    try:
        from PIL import Image
    except ImportError:
        return
    assert F.pil_to_torch(Image.fromarray(a), c.wh).cpu().numpy().tobytes() == want.tobytes()
    assert F.pil_to_torch(Image.fromarray(g), grey.wh).cpu().numpy().tobytes() == want_g.tobytes()


def test_binarise_is_the_stages_mask_line():
    c = fc.BY_NAME["20x31-47x64-c1-bilinear-checker1"]
    want = fc.expected(c).copy()
    want[want > 0] = 255
    got = F.resize_u8(_dev(fc.image(c)), c.wh, "bilinear", binarise=True)
    assert got.cpu().numpy().tobytes() == want.tobytes() and set(np.unique(want)) == {0, 255}


def test_every_refusal():
    img = torch.zeros((4, 5, 3), dtype=torch.uint8, device=DEV)
    for bad in (torch.zeros((4, 5, 2), dtype=torch.uint8, device=DEV), torch.zeros((1, 4, 5, 4), dtype=torch.uint8, device=DEV),
                torch.zeros((4, 5, 3), dtype=torch.float32, device=DEV), torch.zeros((4, 5, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            F.resize_u8(bad, (3, 3))
    for size in ((0, 3), (3, -2)):
        with pytest.raises(ValueError):
            F.resize_u8(img, size)
        with pytest.raises(ValueError):
            F.resize_labels(img[..., 0], size)
    with pytest.raises(ValueError, match="binarise"):
        F.resize_u8(img, (3, 3), out="f32_chw", binarise=True)
    with pytest.raises(ValueError):
        F.resize_labels(torch.zeros((4, 5), dtype=torch.float32, device=DEV), (3, 3))
    with pytest.raises(ValueError):
        F.pil_to_torch(np.zeros((4, 5, 3), dtype=np.float32), (3, 3))
    with pytest.raises(ValueError):
        F.frame_tensor(np.zeros((4, 5), dtype=np.uint8), (3, 3))
    # the raw ABI: a status, the text in sr_last_error(), nothing launched
    lib = L.load()
    b, k = F.resize_tables(5, 3)
    bounds, coeffs, out = _dev(b), _dev(k), torch.full((4, 3, 3), GUARD_U8, dtype=torch.uint8, device=DEV)
    host = torch.zeros((4, 5, 3), dtype=torch.uint8)
    good = [1, 4, 5, 3, ptr(img), 60, 15, 0, 3, ptr(bounds), ptr(coeffs), k.shape[1], 0, ptr(out), None]
    for at, value, code, text in [(4, ptr(host), -1, b"in is not device memory"), (13, ptr(host), -1, b"out is not device memory"),
                                  (9, ptr(torch.from_numpy(b)), -1, b"bounds is not device memory"), (3, 2, -4, b"1 or 3"), (3, 4, -4, b"1 or 3"),
                                  (8, 0, -1, b"out_size"), (8, -3, -1, b"out_size"), (12, 3, -1, b"SR_RESIZE_BINARISE"), (13, ptr(img), -1, b"must not be the input")]:
        args = list(good)
        args[at] = value
        assert lib.sr_resize_u8_pass(*args) == code and text in lib.sr_last_error(), (at, lib.sr_last_error())
    lab, lab_out = torch.zeros((4, 5), dtype=torch.int32, device=DEV), torch.zeros((3, 3), dtype=torch.int32, device=DEV)
    assert lib.sr_resize_nearest(1, 4, 5, 4, ptr(host), 20, 5, 3, 3, ptr(lab_out), None) == -1 and b"in is not device memory" in lib.sr_last_error()
    assert lib.sr_resize_nearest(1, 4, 5, 4, ptr(lab), 20, 5, 3, 0, ptr(lab_out), None) == -1 and b"at least 1" in lib.sr_last_error()
    assert lib.sr_resize_nearest(1, 4, 5, 2, ptr(lab), 20, 5, 3, 3, ptr(lab_out), None) == -4 and b"elem_bytes" in lib.sr_last_error()
    torch.cuda.synchronize()
    assert (out == GUARD_U8).all()
    assert lib.sr_resize_u8_pass(*good) == 0      # ... and the same call with nothing wrong runs
    assert out.cpu().numpy().tobytes() == F.resize_u8_numpy(np.zeros((4, 5, 3), np.uint8), (3, 4)).tobytes()

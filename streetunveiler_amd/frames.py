"""Frames at the training resolution, on the GPU, with the reference's bits (csrc/resize.hip; include/surfel_raster.h states the semantics
once more): Pillow's 8-bit `Image.resize` -- antialiased bicubic or bilinear, integer arithmetic throughout -- and torch's nearest rule
for label maps.

    resize_u8        a uint8 frame [H,W], [H,W,3] or [N,H,W,C] on the device -> uint8 in the same layout, or float32 [C,h,w] / [N,C,h,w]
                     holding v / 255; `binarise` turns the uint8 result into 255 / 0 (the stage's mask[mask > 0] = 255)
    pil_to_torch     the drop-in for the reference's PILtoTorch [REF utils/general_utils.py:21-27]: PIL image, numpy array or uint8
                     tensor on host or device -> float32 [C,h,w] on the GPU
    frame_tensor     what the unveiling stage does to every inpainted frame [REF 3_reoptimization/1_optimization.py:140-199]: bicubic
                     resize, / 255., [3,h,w]
    resize_labels    transforms.Resize(NEAREST) of a label map [REF utils/camera_utils.py:64-65]: uint8, int32 or int64, copied as they are
The checkers, in numpy, written from the definition: resize_tables, resize_u8_numpy, resize_labels_numpy.

One PASS resamples one axis from inS to outS samples with filter f of support sup (bicubic: sup 2, a = -0.5; bilinear: sup 1).  In float64,
in this order: scale = inS / outS, fs = max(scale, 1), support = sup fs, ss = 1 / fs; for output xx: center = (xx + 0.5) scale, xmin =
max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), inS) - xmin, w[x] = f((x + xmin - center + 0.5) ss) for
x < xmax, divided by their sum in ascending x where that is not 0; the integer coefficient is int(w 2^22 + 0.5) (- 0.5 for w < 0),
truncating; the output sample clamp((2^21 + sum in[xmin + x] k[x]) >> 22, 0, 255) in 32-bit integers with an arithmetic shift.  A resize
to (w, h) is the horizontal pass, then the vertical pass on its uint8 result; a pass whose axis keeps its size is left out, and with
both unchanged the resize is a copy.  The tables are computed on the host in numpy float64, uploaded once and kept per (inS, outS,
filter, device); the kernels only read them.

Not here: image decoding and PNG writing, the Scene / Camera classes, the LeftRefill and ZITS pre-processing (make_batch_sd, cv2.resize),
the Lanczos, box and hamming filters, `reducing_gap` and `box=`.  Two or four channels are refused: Pillow resizes an alpha channel
through premultiplied alpha, which is not built (the reference's alpha branch is dead code).  There is no CPU path for the ops themselves."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._call import call, ptr

PRECISION_BITS = 22
_FILTERS = {"bicubic": 2.0, "bilinear": 1.0}      # name -> support


def _filter(name, x):
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _resample_name(resample):
    if isinstance(resample, str):
        name = resample.lower()
    else:      # PIL.Image.Resampling values: BILINEAR = 2, BICUBIC = 3
        name = {2: "bilinear", 3: "bicubic"}.get(int(resample))
    if name not in _FILTERS:
        raise ValueError(f"resample = {resample!r}: 'bicubic' or 'bilinear' (Lanczos, box and hamming are not built)")
    return name


def resize_tables(in_size, out_size, resample="bicubic"):
    """(bounds int32 [out_size,2] = (xmin, count), coeffs int32 [out_size,ksize]) of one pass, ksize = 2 ceil(support) + 1."""
    name = _resample_name(resample)
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"a pass from {in_size} to {out_size} samples: both must be at least 1")
    scale = np.float64(in_size) / np.float64(out_size)
    fs = max(scale, np.float64(1.0))
    support = _FILTERS[name] * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    count = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < count[:, None]
    w = np.where(live, _filter(name, ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for i in range(ksize):      # the sum in ascending x, one addition each (np.sum adds in pairs)
        ww = ww + w[:, i]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = np.where(w < 0, np.trunc(-0.5 + w * (1 << PRECISION_BITS)), np.trunc(0.5 + w * (1 << PRECISION_BITS)))
    return np.stack([xmin, count], 1).astype(np.int32), np.ascontiguousarray(np.where(live, k, 0.0).astype(np.int32))


def _pass_numpy(img, axis, out_size, name):
    """img uint8 [N,H,W,C]; axis 2 = the columns, 1 = the rows."""
    bounds, coeffs = resize_tables(img.shape[axis], out_size, name)
    src = np.moveaxis(img, axis, 1).astype(np.int32)                       # [N, inS, ...]
    acc = np.full((src.shape[0], out_size) + src.shape[2:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
    tail = (None,) * (src.ndim - 2)
    for i in range(coeffs.shape[1]):
        at = np.minimum(bounds[:, 0] + i, img.shape[axis] - 1)              # beyond count the coefficient is 0
        acc += src[:, at] * coeffs[:, i][(None, slice(None)) + tail]       # int32: wraps like the kernel's sum
    return np.moveaxis(np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8), 1, axis)


def _as_nhwc(image, what):
    """-> ([N,H,W,C] view, the function that gives a result its caller's layout back)."""
    if image.dtype != (torch.uint8 if torch.is_tensor(image) else np.uint8):
        raise ValueError(f"{what}: the image must be uint8; got {image.dtype}")
    if image.ndim == 2:
        return image[None, :, :, None], lambda r, chw: r[0] if chw else r[0, :, :, 0]
    if image.ndim == 3:
        return image[None], lambda r, chw: r[0]
    if image.ndim == 4:
        return image, lambda r, chw: r
    raise ValueError(f"{what}: the image must be [H,W], [H,W,C] or [N,H,W,C]; got {list(image.shape)}")


def _check_frame(shape, size, out, binarise, what):
    n, H, W, C = (int(v) for v in shape)
    if C not in (1, 3):
        raise ValueError(f"{what}: {C} channels: 1 or 3 (Pillow resizes an alpha channel through premultiplied alpha, which is not built)")
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: an empty image {list(shape)}")
    w, h = (int(v) for v in size)
    if w < 1 or h < 1:
        raise ValueError(f"{what}: size = {tuple(size)}: (w, h), both at least 1")
    if out not in ("u8", "f32_chw"):
        raise ValueError(f"{what}: out = {out!r}: 'u8' or 'f32_chw'")
    if binarise and out != "u8":
        raise ValueError(f"{what}: binarise gives a 255 / 0 uint8 mask: not with out = {out!r}")
    return w, h


def resize_u8_numpy(image, size, resample="bicubic", out="u8", binarise=False):
    """The checker of resize_u8 on a numpy uint8 array, written from the definition in the module's docstring."""
    image = np.asarray(image)
    img, back = _as_nhwc(image, "resize_u8_numpy")
    w, h = _check_frame(img.shape, size, out, binarise, "resize_u8_numpy")
    name = _resample_name(resample)
    if w != img.shape[2]:
        img = _pass_numpy(img, 2, w, name)
    if h != img.shape[1]:
        img = _pass_numpy(img, 1, h, name)
    if out == "f32_chw":
        return back(np.ascontiguousarray(np.transpose(img, (0, 3, 1, 2))).astype(np.float32) / np.float32(255.0), True)
    img = np.where(img > 0, 255, 0).astype(np.uint8) if binarise else img.copy()
    return back(img, False)


def _nearest_index(in_size, out_size):
    scale = np.float32(in_size) / np.float32(out_size)
    return np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1)


def resize_labels_numpy(label_map, size):
    """The checker of resize_labels: out[..., y, x] = in[..., min(floor(y sy), H - 1), min(floor(x sx), W - 1)], sy = float32(H) / float32(h)
    and the product in float32."""
    label_map = np.asarray(label_map)
    w, h = (int(v) for v in size)
    if label_map.ndim not in (2, 3) or w < 1 or h < 1:
        raise ValueError(f"resize_labels_numpy: a map [H,W] or [N,H,W] and a size (w, h) of at least 1; got {list(label_map.shape)}, {tuple(size)}")
    H, W = label_map.shape[-2:]
    return np.ascontiguousarray(label_map[..., _nearest_index(H, h)[:, None], _nearest_index(W, w)[None, :]])


# ---- the device side --------------------------------------------------------------------------------------------------------------------
_TABLES = {}      # (inS, outS, filter, device) -> (bounds, coeffs, ksize) on that device: computed and uploaded once


def _device_tables(in_size, out_size, name, dev):
    key = (in_size, out_size, name, dev)
    got = _TABLES.get(key)
    if got is None:
        bounds, coeffs = resize_tables(in_size, out_size, name)
        got = _TABLES[key] = (torch.from_numpy(bounds).to(dev), torch.from_numpy(coeffs).to(dev), int(coeffs.shape[1]))
    return got


def _device_frame(t, what, dtypes):
    """A tensor the kernels can walk: on the GPU, its rows' elements dense; the strides of the leading dimensions are handed over."""
    if not torch.is_tensor(t):
        raise ValueError(f"{what}: a torch tensor is needed; got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what}: the tensor is on {t.device}: it must be on the GPU (pil_to_torch uploads; *_numpy is the checker)")
    if t.dtype not in dtypes:
        raise ValueError(f"{what}: the tensor must be {' or '.join(str(d) for d in dtypes)}; got {t.dtype}")
    return t.detach()


def _leading_strides(t, row_elems):
    """t [N,H,...] with dense rows -> (t or one contiguous copy, batch stride, row stride)."""
    if not (t[0, 0].is_contiguous() and (t.shape[1] == 1 or t.stride(1) >= row_elems)):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else 0), (t.stride(1) if t.shape[1] > 1 else row_elems)


def resize_u8(image, size, resample="bicubic", out="u8", binarise=False, stream=None):
    """Pillow's `Image.resize(size, resample)` of a uint8 frame on the device, bit for bit.  image: [H,W], [H,W,3] or [N,H,W,C] (C = 1 or
    3), non-contiguous in the leading dimensions or not; size = (w, h) as in Pillow.  out = "u8": uint8 in the input's layout; "f32_chw":
    float32 [C,h,w] ([N,C,h,w] for a batch) = v / 255.  binarise (uint8 only): 255 where the resized byte is > 0, else 0.  Runs on
    `stream` (a torch.cuda.Stream; None: the current one)."""
    image = _device_frame(image, "resize_u8", (torch.uint8,))
    img, back = _as_nhwc(image, "resize_u8")
    w, h = _check_frame(img.shape, size, out, binarise, "resize_u8")
    name = _resample_name(resample)
    if stream is not None:
        with torch.cuda.stream(stream):
            return resize_u8(image, size, name, out, binarise)
    dev = img.device
    N, H, W, C = (int(v) for v in img.shape)
    img, bs, rs = _leading_strides(img, W * C)
    flags = L.SR_RESIZE_F32_CHW if out == "f32_chw" else (L.SR_RESIZE_BINARISE if binarise else 0)
    passes = [(0, w)] if w != W else []
    passes += [(1, h)] if h != H else []
    if not passes:
        passes = [(-1, 0)]
    for i, (axis, out_size) in enumerate(passes):
        last = i == len(passes) - 1
        oh, ow = (out_size if axis == 1 else H), (out_size if axis == 0 else W)
        if last and out == "f32_chw":
            result = torch.empty((N, C, oh, ow), dtype=torch.float32, device=dev)
        else:
            result = torch.empty((N, oh, ow, C), dtype=torch.uint8, device=dev)
        bounds, coeffs, ksize = _device_tables(W if axis == 0 else H, out_size, name, dev) if axis >= 0 else (None, None, 0)
        call("sr_resize_u8_pass", dev, N, H, W, C, ptr(img), bs, rs, axis, out_size, ptr(bounds), ptr(coeffs), ksize, flags if last else 0,
             ptr(result))
        img, H, W, bs, rs = result, oh, ow, oh * ow * C, ow * C
    return back(img, out == "f32_chw")


def _to_device_u8(image, what, device):
    """A PIL image, a numpy array or a uint8 tensor on host or device -> a uint8 tensor on the GPU, [H,W] or [H,W,C]."""
    if not torch.is_tensor(image):
        image = torch.from_numpy(np.array(image))      # a PIL image: its decoded bytes, [H,W] ("L") or [H,W,C]; a copy, as the reference makes
    if image.dtype != torch.uint8:
        raise ValueError(f"{what}: the image must be uint8; got {image.dtype}")
    if not image.is_cuda:
        image = image.to(torch.device("cuda" if device is None else device))
    return image


def pil_to_torch(image, resolution, device=None):
    """The reference's PILtoTorch(pil_image, resolution) with the resize on the GPU: a PIL image ("L" or "RGB"), a numpy array or a uint8
    tensor ([H,W] or [H,W,3], on host or device; a host image is uploaded at its own size, `device`: where, for a host image) -> float32
    [C,h,w] on the GPU, bit for bit what `torch.from_numpy(np.array(image.resize(resolution))) / 255.0`, permuted, holds.  A 2-D input
    gives [1,h,w]."""
    image = _to_device_u8(image, "pil_to_torch", device)
    if image.ndim not in (2, 3):
        raise ValueError(f"pil_to_torch: one image [H,W] or [H,W,C]; got {list(image.shape)}")
    return resize_u8(image, resolution, "bicubic", out="f32_chw")


def frame_tensor(image, size, device=None):
    """An inpainted frame as the unveiling stage holds it: `.resize(size, BICUBIC)`, then `/ 255.`, float32 [3,h,w] on the GPU."""
    image = _to_device_u8(image, "frame_tensor", device)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"frame_tensor: an RGB frame [H,W,3]; got {list(image.shape)}")
    return resize_u8(image, size, "bicubic", out="f32_chw")


def resize_labels(label_map, size, stream=None):
    """transforms.Resize((h, w), NEAREST) of a label map on the device: [H,W] or [N,H,W], uint8, int32 or int64, -> [h,w] or [N,h,w] of the
    same dtype, every element copied as it is.  size = (w, h)."""
    label_map = _device_frame(label_map, "resize_labels", (torch.uint8, torch.int32, torch.int64))
    if label_map.ndim not in (2, 3):
        raise ValueError(f"resize_labels: a map [H,W] or [N,H,W]; got {list(label_map.shape)}")
    w, h = (int(v) for v in size)
    if w < 1 or h < 1:
        raise ValueError(f"resize_labels: size = {tuple(size)}: (w, h), both at least 1")
    if label_map.numel() == 0:
        raise ValueError(f"resize_labels: an empty map {list(label_map.shape)}")
    if stream is not None:
        with torch.cuda.stream(stream):
            return resize_labels(label_map, size)
    maps = label_map if label_map.ndim == 3 else label_map[None]
    N, H, W = (int(v) for v in maps.shape)
    maps, bs, rs = _leading_strides(maps, W)
    out = torch.empty((N, h, w), dtype=maps.dtype, device=maps.device)
    call("sr_resize_nearest", maps.device, N, H, W, maps.element_size(), ptr(maps), bs, rs, h, w, ptr(out))
    return out if label_map.ndim == 3 else out[0]

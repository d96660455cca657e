"""The frame masks of the unveiling stage on the GPU (csrc/unveil.hip; include/surfel_raster.h states the semantics once more): what
connects the instance selection, the masked model and its losses in the reference's inpainting_pipeline/.

Per point [REF scene/__init__.py:217-312, inpainting_pipeline/1_selection/1_instance_visualization.py:85-100]:
    points_in_frame            getPcdInTrainFrame / getPcdPixelCoordsInTrainFrame[WithDepth]: bool[P], with coords=True also pix int64[n,2]
                               and depth float32[n] of the admitted points in ascending point index (one read-back: n)
    frame_visibility           count int64[F] and depth_sum float64[F] over points x frames, one launch and a fold
    pick_view                  the view 1_instance_visualization.py picks for a cluster
    semantic_mask_of_points    Scene.getSemanticMaskOfSplatting with the maps resident on the GPU -> (bool[P], out-of-range count)
Per pixel [REF inpainting_pipeline/utils.py:17-30, 2_generate_inpainted_mask.py:111-159, 3_reoptimization/1_optimization.py:115-187]:
    dilate_mask                cv2.dilate with a k x k kernel of ones, on the GPU, no host copy
    instance_pixel_mask        |alpha_a - alpha_b| > threshold, dilated, fused
    refill_mask                ~(|a - b|.sum(0) < eps) & mask, dilated, fused
    inpaint_conditions         the dilated mask and the five uint8 images a frame hands to the inpainting networks, two launches
The checkers: `*_torch` functions, the reference's lines in the reference's order -- in float64 the truth, in float32 on the same device
the twin and the timing baseline -- and dilate_mask_numpy, written from the definition.

A camera is FrameCamera(w2c [4,4], K [3,3], h, w, max_z=None, reso_scale=None), a batch FrameCameras with the stacked [F,...] tensors and
per-frame h, w (max_z and reso_scale: None, one value, or one per frame with None where a frame has none).  pack_cameras() turns either
into the two device arrays the kernels read; the ops accept the packed form as well, so a loop packs once.

The predicate is the reference's, in float32 with strict inequalities: cam = R x + t, z = cam.z > 0 (and z < max_z), pix = (K cam).xy /
(K cam).z, 0 < pix.x < w, 0 < pix.y < h.  Pixel coordinates are trunc(pix) as int64, then trunc(trunc(pix) / reso_scale) in float32 true
division where a scale is given.  A point with a NaN or infinite coordinate is in no frame.

The dilation: out(y, x) = OR of mask(y + dy, x + dx) over dy, dx in [-(k // 2), k - 1 - k // 2], nothing from outside the image -- cv2.dilate
with np.ones((k, k)), the default anchor (k // 2, k // 2) and the default border AS OPENCV DOCUMENTS THEM.  cv2 is not a dependency of this
project and was not available to check against: the identification is unverified.  For even k the window is not symmetric: one set pixel
grows by k // 2 - 1 up and left and by k // 2 down and right.

Deliberate differences from the reference: (1) a semantic label of 31 or more matches nothing (the reference shifts an int32 by it);
(2) a pixel index outside the semantic map -- reso_scale and the map size disagree -- is not read, matches nothing and is counted, for
every frame tested before the point was set (the reference raises); (3) pick_view takes the mean depth as depth_sum / count in float64,
where the reference takes a float32 mean; (4) a NaN in a condition image becomes byte 0 (the reference's cast of a NaN is undefined).
There is no CPU path for the ops themselves."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from ._call import buf, call, ptr, workspace

CAM_FLOATS = 24      # kUnveilCamFloats: w2c rows 0..2, K, max_z, reso_scale, one unused


class FrameCamera(NamedTuple):
    w2c: torch.Tensor                     # [4,4] world -> camera
    K: torch.Tensor                       # [3,3] (a larger intrinsic matrix is cut to its upper-left 3 x 3, as the reference does)
    h: int
    w: int
    max_z: Optional[float] = None
    reso_scale: Optional[float] = None


class FrameCameras(NamedTuple):
    w2c: torch.Tensor                     # [F,4,4]
    K: torch.Tensor                       # [F,3,3]
    hw: object                            # F pairs (h, w)
    max_z: object = None                  # None, one value, or F values (None where a frame has none)
    reso_scale: object = None

    def __len__(self):
        return int(self.w2c.shape[0])

    def frame(self, f):
        pick = lambda v: v[f] if isinstance(v, (list, tuple)) else v
        h, w = self.hw[f]
        return FrameCamera(self.w2c[f], self.K[f], int(h), int(w), pick(self.max_z), pick(self.reso_scale))


class PackedCameras(NamedTuple):
    cams: torch.Tensor                    # [F,24] float32 on the device
    hw: torch.Tensor                      # [F,2] int32 on the device

    def __len__(self):
        return int(self.cams.shape[0])


def _per_frame(value, F, name, none):
    values = list(value) if isinstance(value, (list, tuple)) else [value] * F
    if len(values) != F:
        raise ValueError(f"{len(values)} {name} values for {F} frames")
    out = []
    for v in values:
        if v is None:
            out.append(none)
            continue
        v = float(v)
        if name == "reso_scale" and not (v > 0 and np.isfinite(v)):
            raise ValueError(f"reso_scale = {v}: must be positive and finite (or None)")
        if v != v:
            raise ValueError(f"{name} is NaN")
        out.append(v)
    return out


def pack_cameras(cameras, device, max_z="keep"):
    """FrameCamera / FrameCameras (tensors on any device) -> PackedCameras on `device`.  `max_z` other than "keep" replaces the cameras' own.
    A PackedCameras is checked, not moved: one on another device than `device`, or of another dtype or shape, is refused."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if isinstance(cameras, PackedCameras):      # its addresses go to the kernels as they are: held to the device of the call and to the layout
        cams, hw = cameras.cams, cameras.hw
        if not (torch.is_tensor(cams) and torch.is_tensor(hw)):
            raise ValueError("PackedCameras must hold two tensors")
        if cams.device != device or hw.device != device:
            raise L.SurfelRasterError(f"the packed cameras are on {cams.device} / {hw.device}, the call is on {device}: pack them with "
                                      f"pack_cameras(cameras, {str(device)!r}); there is no CPU path")
        if cams.dtype != torch.float32 or cams.dim() != 2 or cams.shape[1] != CAM_FLOATS or not cams.is_contiguous():
            raise ValueError(f"PackedCameras.cams must be a contiguous float32 tensor [F,{CAM_FLOATS}]; got {cams.dtype} {list(cams.shape)}")
        if hw.dtype != torch.int32 or tuple(hw.shape) != (cams.shape[0], 2) or not hw.is_contiguous():
            raise ValueError(f"PackedCameras.hw must be a contiguous int32 tensor [{cams.shape[0]},2]; got {hw.dtype} {list(hw.shape)}")
        if max_z != "keep":
            cams = cameras.cams.clone()
            cams[:, 21] = float("inf") if max_z is None else float(max_z)
            return PackedCameras(cams, cameras.hw)
        return cameras
    if isinstance(cameras, FrameCamera):
        cameras = FrameCameras(cameras.w2c[None], cameras.K[None], [(cameras.h, cameras.w)], cameras.max_z, cameras.reso_scale)
    if not isinstance(cameras, FrameCameras):
        raise ValueError(f"cameras must be a FrameCamera, FrameCameras or PackedCameras; got {type(cameras).__name__}")
    w2c, K = cameras.w2c, cameras.K
    if not (torch.is_tensor(w2c) and torch.is_tensor(K)):
        raise ValueError("w2c and K must be tensors")
    if w2c.dim() != 3 or tuple(w2c.shape[1:]) != (4, 4) or K.dim() != 3 or K.shape[1] < 3 or K.shape[2] < 3 or K.shape[0] != w2c.shape[0]:
        raise ValueError(f"w2c must be [F,4,4] and K [F,3,3]; got {list(w2c.shape)} and {list(K.shape)}")
    if w2c.dtype != torch.float32 or K.dtype != torch.float32:
        raise ValueError(f"w2c and K must be float32; got {w2c.dtype} and {K.dtype}")
    F = int(w2c.shape[0])
    hw = [(int(h), int(w)) for h, w in cameras.hw]
    if len(hw) != F:
        raise ValueError(f"{len(hw)} (h, w) pairs for {F} frames")
    if any(h < 1 or w < 1 or h > 1 << 24 or w > 1 << 24 for h, w in hw):
        raise ValueError("every frame's h and w must be in 1..2^24")
    tail = torch.tensor([[z, r, 0.0] for z, r in zip(_per_frame(cameras.max_z if max_z == "keep" else max_z, F, "max_z", float("inf")),
                                                      _per_frame(cameras.reso_scale, F, "reso_scale", 0.0))], dtype=torch.float32).reshape(F, 3)
    cams = torch.cat([w2c.detach()[:, :3, :].reshape(F, 12).to(device), K.detach()[:, :3, :3].reshape(F, 9).to(device), tail.to(device)], dim=1)
    return PackedCameras(cams.contiguous(), torch.tensor(hw, dtype=torch.int32).reshape(F, 2).to(device))


def _device_points(xyz, what):
    if not torch.is_tensor(xyz):
        raise ValueError(f"xyz must be a tensor; got {type(xyz).__name__}")
    if not xyz.is_cuda:
        raise L.SurfelRasterError(f"xyz is on {xyz.device}: {what} needs CUDA (ROCm) tensors; there is no CPU path ({what}_torch is the checker)")
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must be a float32 tensor [P,3]; got {xyz.dtype} {list(xyz.shape)}")
    return xyz.detach().contiguous()


# ---- per point --------------------------------------------------------------------------------------------------------------------------
def points_in_frame(xyz, camera, coords=False):
    """`xyz` [P,3] float32 on the GPU, one camera -> bool[P]; with coords=True -> (bool[P], pix int64[n,2] = (x, y), depth float32[n]) of the
    admitted points in ascending point index -- the order of the reference's boolean indexing.  The compaction is a scan; n is the one
    read-back.  Runs on the current stream."""
    xyz = _device_points(xyz, "points_in_frame")
    dev, P = xyz.device, xyz.shape[0]
    cam = pack_cameras(camera, dev)
    if len(cam) != 1:
        raise ValueError(f"points_in_frame takes one camera; got {len(cam)} (frame_visibility takes a batch)")
    mask = torch.empty((P,), dtype=torch.bool, device=dev)
    if not coords:
        call("sr_points_in_frame", dev, P, ptr(xyz), ptr(cam.cams), ptr(cam.hw), ptr(mask), None, 0, None)
        return mask
    ws = workspace("sr_unveil_workspace_bytes", dev, P, 1)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    call("sr_points_in_frame", dev, P, ptr(xyz), ptr(cam.cams), ptr(cam.hw), ptr(mask), *buf(ws), ptr(count))
    n = int(count.item())      # the one synchronisation
    pix = torch.empty((n, 2), dtype=torch.int64, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    call("sr_points_in_frame_emit", dev, P, ptr(xyz), ptr(cam.cams), ptr(cam.hw), *buf(ws), n, ptr(pix), ptr(depth))
    return mask, pix, depth


def frame_visibility(xyz, cameras, max_z="keep"):
    """-> (count int64[F], depth_sum float64[F]) on the device: per frame the number of admitted points and the sum of their depths.
    Fixed-order sums, no floating atomics: equal inputs give equal bits.  Nothing is read back."""
    xyz = _device_points(xyz, "frame_visibility")
    dev, P = xyz.device, xyz.shape[0]
    cams = pack_cameras(cameras, dev, max_z)
    F = len(cams)
    count = torch.empty((F,), dtype=torch.int64, device=dev)
    depth_sum = torch.empty((F,), dtype=torch.float64, device=dev)
    ws = workspace("sr_unveil_workspace_bytes", dev, P, F)
    call("sr_frame_visibility", dev, P, F, ptr(xyz), ptr(cams.cams), ptr(cams.hw), *buf(ws), ptr(count), ptr(depth_sum))
    return count, depth_sum


def pick_view_from_counts(count, depth_sum, P):
    """The rule of 1_instance_visualization.py:85-100 on per-frame counts and depth sums (sequences): the first frame with count > 0.9 P and
    mean depth < 4, else the first with count > 0.5 P, else -1.  With count == 0 the mean is NaN and the first test is false."""
    count, depth_sum = [int(c) for c in count], [float(s) for s in depth_sum]
    for f, (c, s) in enumerate(zip(count, depth_sum)):
        mean = s / c if c > 0 else float("nan")
        if c > 0.9 * P and mean < 4.0:
            return f
    for f, c in enumerate(count):
        if c > 0.5 * P:
            return f
    return -1


def pick_view(xyz, cameras, max_z=10.0):
    """The view the reference renders a cluster in -> frame index or -1.  One launch over all frames and one read-back of 2 F numbers."""
    count, depth_sum = frame_visibility(xyz, cameras, max_z)
    return pick_view_from_counts(count.tolist(), depth_sum.tolist(), int(xyz.shape[0]))


def semantic_mask_of_points(xyz, cameras, semantic_maps, remain_bit):
    """Scene.getSemanticMaskOfSplatting: `semantic_maps` uint8[F,Hm,Wm] on the GPU, `remain_bit` the mask of the labels that remain ->
    (bool[P], n_out_of_range int64[1] on the device).  The cameras' max_z is not applied, as the reference passes None."""
    xyz = _device_points(xyz, "semantic_mask_of_points")
    dev, P = xyz.device, xyz.shape[0]
    cams = pack_cameras(cameras, dev, None)
    F = len(cams)
    if not torch.is_tensor(semantic_maps) or not semantic_maps.is_cuda:
        raise L.SurfelRasterError("semantic_maps must be a CUDA (ROCm) tensor: the maps stay resident on the GPU; there is no CPU path")
    if semantic_maps.device != dev:
        raise L.SurfelRasterError(f"semantic_maps is on {semantic_maps.device}, xyz on {dev}: the maps must be resident on the device of the call")
    if semantic_maps.dtype != torch.uint8 or semantic_maps.dim() != 3:
        raise ValueError(f"semantic_maps must be uint8 [F,Hm,Wm]; got {semantic_maps.dtype} {list(semantic_maps.shape)}")
    if semantic_maps.shape[0] != F:
        raise ValueError(f"{semantic_maps.shape[0]} semantic maps for {F} cameras")
    maps = semantic_maps.contiguous()
    mask = torch.empty((P,), dtype=torch.bool, device=dev)
    outside = torch.empty((1,), dtype=torch.int64, device=dev)
    call("sr_semantic_mask_of_points", dev, P, F, ptr(xyz), ptr(cams.cams), ptr(cams.hw), ptr(maps), maps.shape[1], maps.shape[2],
         int(remain_bit) & 0x7FFFFFFF, ptr(mask), ptr(outside))
    return mask, outside


# ---- per pixel --------------------------------------------------------------------------------------------------------------------------
def _check_k(k):
    k = int(k)
    if not 1 <= k <= 31:
        raise ValueError(f"k = {k}: must be in 1..31")
    return k


def _device_image(t, name, what, shape=None, dtypes=(torch.float32,)):
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a tensor; got {type(t).__name__}")
    if not t.is_cuda:
        raise L.SurfelRasterError(f"{name} is on {t.device}: {what} needs CUDA (ROCm) tensors; there is no CPU path ({what}_torch is the checker)")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}; got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}; got {list(t.shape)}")
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.view(torch.uint8) if t.is_contiguous() else t.contiguous().view(torch.uint8)
    return t.contiguous()


def _plane(t, name, what):
    """[H,W] or [1,H,W] float32 -> contiguous [H,W]"""
    if torch.is_tensor(t) and t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if torch.is_tensor(t) and t.dim() != 2:
        raise ValueError(f"{name} must be [H,W] or [1,H,W]; got {list(t.shape)}")
    t = _device_image(t, name, what)
    if t.numel() == 0:
        raise ValueError(f"{name} is empty")
    return t


def dilate_mask(mask, k):
    """`mask` [H,W] bool or uint8 (not 0 = set) on the GPU, 1 <= k <= 31 -> bool[H,W]; the module's docstring states the window."""
    k = _check_k(k)
    if torch.is_tensor(mask) and mask.dim() != 2:
        raise ValueError(f"mask must be [H,W]; got {list(mask.shape)}")
    m = _device_image(mask, "mask", "dilate_mask", dtypes=(torch.bool, torch.uint8))
    if m.numel() == 0:
        raise ValueError("mask is empty")
    out = torch.empty(m.shape, dtype=torch.bool, device=m.device)
    call("sr_dilate_mask", m.device, m.shape[0], m.shape[1], k, ptr(m), ptr(out))
    return out


def instance_pixel_mask(alpha_a, alpha_b, threshold=0.01, k=5):
    """|alpha_a - alpha_b| > threshold ([1,H,W] or [H,W] float32 each), dilated by k -> bool[H,W].  A NaN difference is not set."""
    k = _check_k(k)
    a = _plane(alpha_a, "alpha_a", "instance_pixel_mask")
    b = _plane(alpha_b, "alpha_b", "instance_pixel_mask")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"alpha_a {list(a.shape)} on {a.device} and alpha_b {list(b.shape)} on {b.device} must agree")
    out = torch.empty(a.shape, dtype=torch.bool, device=a.device)
    call("sr_instance_pixel_mask", a.device, a.shape[0], a.shape[1], ptr(a), ptr(b), float(threshold), k, ptr(out))
    return out


def refill_mask(render_a, render_b, mask, eps=2e-2, k=10):
    """~((render_a - render_b).abs().sum(0) < eps) & mask ([C,H,W] float32 renders, [H,W] bool or uint8 mask), dilated by k -> bool[H,W].
    A NaN sum is set, as in the reference's ~(... < eps)."""
    k = _check_k(k)
    if not torch.is_tensor(render_a) or render_a.dim() != 3:
        raise ValueError("render_a must be a tensor [C,H,W]")
    a = _device_image(render_a, "render_a", "refill_mask")
    b = _device_image(render_b, "render_b", "refill_mask", shape=a.shape)
    m = _device_image(mask, "mask", "refill_mask", shape=a.shape[1:], dtypes=(torch.bool, torch.uint8))
    if a.numel() == 0:
        raise ValueError("render_a is empty")
    if b.device != a.device or m.device != a.device:
        raise ValueError("render_a, render_b and mask must be on one device")
    out = torch.empty(a.shape[1:], dtype=torch.bool, device=a.device)
    call("sr_refill_mask", a.device, a.shape[1], a.shape[2], a.shape[0], ptr(a), ptr(b), ptr(m), float(eps), k, ptr(out))
    return out


CONDITION_IMAGES = (("original_rgb", 3), ("inpainted_rgb", 3), ("empty_opacity", 1), ("inpainted_depth", 1), ("inpainted_normal", 3))


def inpaint_conditions(full, background, sky, threshold=0.01, k=5):
    """The body of render_set in 2_generate_inpainted_mask.py for its RENDER_WO_INSTANCE setting: `full` and `background` are the dicts
    `render` and `render_with_mask` return (render [3,H,W], rend_alpha [1,H,W]; of background also surf_depth [1,H,W] and rend_normal
    [3,H,W]), `sky` [3,H,W] -> {"mask": bool[H,W], "original_rgb", "inpainted_rgb", "inpainted_normal": uint8[H,W,3], "empty_opacity",
    "inpainted_depth": uint8[H,W,1]}, ready for an image writer.  Two launches, no host round trip."""
    k = _check_k(k)
    what = "inpaint_conditions"
    alpha = _plane(full["rend_alpha"], "full['rend_alpha']", what)
    H, W = alpha.shape
    dev = alpha.device
    render = _device_image(full["render"], "full['render']", what, shape=(3, H, W))
    bg_render = _device_image(background["render"], "background['render']", what, shape=(3, H, W))
    bg_alpha = _plane(background["rend_alpha"], "background['rend_alpha']", what)
    bg_depth = _plane(background["surf_depth"], "background['surf_depth']", what)
    bg_normal = _device_image(background["rend_normal"], "background['rend_normal']", what, shape=(3, H, W))
    sky = _device_image(sky, "sky", what, shape=(3, H, W))
    for name, t in (("background['rend_alpha']", bg_alpha), ("background['surf_depth']", bg_depth)):
        if t.shape != alpha.shape:
            raise ValueError(f"{name} must be [1,{H},{W}]; got {list(t.shape)}")
    if any(t.device != dev for t in (render, bg_render, bg_alpha, bg_depth, bg_normal, sky)):
        raise ValueError("every image must be on one device")
    out = {"mask": torch.empty((H, W), dtype=torch.bool, device=dev)}
    for name, channels in CONDITION_IMAGES:
        out[name] = torch.empty((H, W, channels), dtype=torch.uint8, device=dev)
    call("sr_inpaint_conditions", dev, H, W, ptr(render), ptr(alpha), ptr(bg_render), ptr(bg_alpha), ptr(bg_depth), ptr(bg_normal), ptr(sky),
         float(threshold), k, ptr(out["mask"]), *(ptr(out[name]) for name, _ in CONDITION_IMAGES))
    return out


# ---- the checkers: the reference's lines in the reference's order ------------------------------------------------------------------------
def _as_camera(camera):
    if isinstance(camera, FrameCameras):
        if len(camera) != 1:
            raise ValueError("one camera expected")
        return camera.frame(0)
    return camera


def project_torch(xyz, camera, dtype=torch.float64):
    """-> (in_frame bool[P], pix [P,2], depth [P]) in `dtype` on xyz's device [REF getPcdPixelCoordsInTrainFrameWithDepth, up to the mask]."""
    camera = _as_camera(camera)
    lidar_pcd = xyz.to(dtype)
    w2c = camera.w2c.to(device=xyz.device, dtype=dtype)
    intr = camera.K.to(device=xyz.device, dtype=dtype)
    camera_point = (w2c[:3, :3] @ lidar_pcd.T).T + w2c[:3, 3]
    positive_z_mask = camera_point[..., 2] > 0
    if camera.max_z is None:
        small_z_mask = torch.ones_like(camera_point[..., 2], dtype=torch.bool)
    else:
        small_z_mask = camera_point[..., 2] < camera.max_z
    pixel_point = (intr[:3, :3] @ camera_point.T).T
    pix = pixel_point[..., :2] / pixel_point[..., 2][..., None]
    h, w = camera.h, camera.w
    in_frame_mask = (pix[..., 0] < w) * (pix[..., 0] > 0) * (pix[..., 1] < h) * (pix[..., 1] > 0) * positive_z_mask * small_z_mask
    in_frame_mask = in_frame_mask * torch.isfinite(xyz).all(dim=-1)      # stated, not left to 0 * inf: such a point is in no frame
    return in_frame_mask, pix, camera_point[..., 2]


def points_in_frame_torch(xyz, camera, coords=False, dtype=torch.float64):
    """The checker of points_in_frame: bool[P], with coords=True (bool[P], pix int64[n,2], depth [n] in `dtype`)."""
    camera = _as_camera(camera)
    in_frame_mask, pix, depth = project_torch(xyz, camera, dtype)
    if not coords:
        return in_frame_mask
    valid_pix = pix[in_frame_mask].to(torch.int64)
    if camera.reso_scale is not None:      # an int64 tensor over a Python float: float32 true division
        scale = torch.full((), float(camera.reso_scale), dtype=torch.float32, device=xyz.device)
        valid_pix = torch.div(valid_pix.to(torch.float32), scale).to(torch.int64)
    return in_frame_mask, valid_pix, depth[in_frame_mask]


def _frames(cameras):
    return [cameras] if isinstance(cameras, FrameCamera) else [cameras.frame(f) for f in range(len(cameras))]


def frame_visibility_torch(xyz, cameras, max_z="keep", dtype=torch.float64):
    """The checker of frame_visibility: the reference's loop over the frames -> (count int64[F], depth_sum float64[F]) on xyz's device."""
    counts, sums = [], []
    for camera in _frames(cameras):
        if max_z != "keep":
            camera = camera._replace(max_z=max_z)
        in_frame_mask, _, depth = project_torch(xyz, camera, dtype)
        valid_pcd_depth = depth[in_frame_mask]
        counts.append(valid_pcd_depth.shape[0])
        sums.append(valid_pcd_depth.to(torch.float64).sum())
    return (torch.tensor(counts, dtype=torch.int64, device=xyz.device),
            torch.stack(sums) if sums else torch.zeros((0,), dtype=torch.float64, device=xyz.device))


def pick_view_torch(xyz, cameras, max_z=10.0, dtype=torch.float64):
    count, depth_sum = frame_visibility_torch(xyz, cameras, max_z, dtype)
    return pick_view_from_counts(count.tolist(), depth_sum.tolist(), int(xyz.shape[0]))


def semantic_mask_of_points_torch(xyz, cameras, semantic_maps, remain_bit, dtype=torch.float64):
    """The checker of semantic_mask_of_points [REF getSemanticMaskOfSplatting], everything on xyz's device -> (bool[P], out-of-range count).
    The two deliberate differences are written out: labels of 31 or more, and indices outside the map (counted where the point is not yet set)."""
    P = xyz.shape[0]
    final_mask = torch.zeros((P,), dtype=torch.bool, device=xyz.device)
    index_tensor = torch.arange(P, device=xyz.device)
    outside = 0
    remain_bit = int(remain_bit) & 0x7FFFFFFF
    Hm, Wm = semantic_maps.shape[1:]
    for frame_id, camera in enumerate(_frames(cameras)):
        current_semantic_map = semantic_maps[frame_id]
        in_frame_mask, valid_pix, _ = points_in_frame_torch(xyz, camera._replace(max_z=None), True, dtype)
        in_frame_index = index_tensor[in_frame_mask]
        inside = (valid_pix[..., 0] >= 0) & (valid_pix[..., 0] < Wm) & (valid_pix[..., 1] >= 0) & (valid_pix[..., 1] < Hm)
        outside += int((~inside & ~final_mask[in_frame_index]).sum())
        valid_pix, in_frame_index = valid_pix[inside], in_frame_index[inside]
        valid_pix_semantic = current_semantic_map[valid_pix[..., 1], valid_pix[..., 0]].to(torch.int64)
        if_in_semantic_region = (((1 << valid_pix_semantic.clamp(max=31)) & remain_bit) > 0) & (valid_pix_semantic < 31)
        final_mask[in_frame_index[if_in_semantic_region]] = True
    return final_mask, outside


def dilate_mask_numpy(mask, k):
    """The checker of dilate_mask, from the definition: out(y, x) = OR of mask(y + dy, x + dx), dy, dx in [-(k // 2), k - 1 - k // 2], nothing
    from outside the image.  numpy only."""
    m = np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask) != 0
    if m.ndim != 2 or not 1 <= int(k) <= 31:
        raise ValueError("mask must be [H,W] and k in 1..31")
    H, W = m.shape
    before, after = k // 2, k - 1 - k // 2
    padded = np.zeros((H + before + after, W + before + after), dtype=bool)
    padded[before:before + H, before:before + W] = m
    out = np.zeros((H, W), dtype=bool)
    for dy in range(-before, after + 1):
        for dx in range(-before, after + 1):
            out |= padded[before + dy:before + dy + H, before + dx:before + dx + W]
    return out


def dilate_mask_torch(mask, k):
    """The same window with stock torch on the mask's device (the twin and the timing baseline): a max-pool over the asymmetrically padded mask."""
    m = (mask != 0).to(torch.float32)[None, None]
    before, after = k // 2, k - 1 - k // 2
    m = torch.nn.functional.pad(m, (before, after, before, after), value=0.0)
    return torch.nn.functional.max_pool2d(m, kernel_size=k, stride=1)[0, 0] > 0


def _threshold(value, like):
    """A Python float compared with a float32 tensor is compared as its float32 value; the float64 truth takes that very value."""
    return torch.tensor(float(value), dtype=torch.float32).to(device=like.device, dtype=like.dtype)


def instance_pixel_mask_torch(alpha_a, alpha_b, threshold=0.01, k=5, dtype=torch.float64, undilated=False):
    rendered_alpha, removed_rendered_alpha = alpha_a.to(dtype).reshape(1, *alpha_a.shape[-2:]), alpha_b.to(dtype).reshape(1, *alpha_b.shape[-2:])
    instance_pix_mask = (torch.abs(rendered_alpha - removed_rendered_alpha) > _threshold(threshold, rendered_alpha)).sum(0)
    return instance_pix_mask != 0 if undilated else dilate_mask_torch(instance_pix_mask, k)


def refill_mask_torch(render_a, render_b, mask, eps=2e-2, k=10, dtype=torch.float64, undilated=False):
    a, b = render_a.to(dtype), render_b.to(dtype)
    refill = ~((a - b).abs().sum(0) < _threshold(eps, a)) * (mask != 0)
    return refill if undilated else dilate_mask_torch(refill, k)


def quantise_torch(image):
    """torchvision's save_image on [C,H,W]: mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8) (torchvision is not a dependency:
    the line is restated).  -> (uint8 [H,W,C], 255 x + 0.5 before the clamp, [H,W,C]); a NaN becomes 0."""
    value = image.mul(255).add_(0.5)
    return torch.nan_to_num(value.clamp(0, 255), nan=0.0).permute(1, 2, 0).to(torch.uint8), value.permute(1, 2, 0)


def inpaint_conditions_torch(full, background, sky, threshold=0.01, k=5, dtype=torch.float64, values=False):
    """The checker of inpaint_conditions: the body of render_set for RENDER_WO_INSTANCE, line by line.  values=True: also the float values
    before the cast to uint8, under name + "_value"."""
    sky_image = sky.to(dtype)
    rendered_alpha = full["rend_alpha"].to(dtype)
    original_rgb = full["render"].to(dtype) + sky_image * (1 - rendered_alpha)
    background_rgb = background["render"].to(dtype) + sky_image * (1 - rendered_alpha)
    removed_rendered_alpha = background["rend_alpha"].to(dtype)
    depth = background["surf_depth"].to(dtype)
    raw_disparity = (1.0 / depth)
    raw_disparity[raw_disparity.isinf()] = 0.0
    disparity = torch.clamp(raw_disparity, 0.0, 1.0)
    normal = torch.clamp(background["rend_normal"].to(dtype) * 0.5 + 0.5, 0.0, 1.0)
    out = {"mask": instance_pixel_mask_torch(rendered_alpha, removed_rendered_alpha, threshold, k, dtype)}
    for name, image in (("original_rgb", original_rgb), ("inpainted_rgb", background_rgb), ("empty_opacity", rendered_alpha - removed_rendered_alpha),
                        ("inpainted_depth", disparity), ("inpainted_normal", normal)):
        out[name], value = quantise_torch(image)
        if values:
            out[name + "_value"] = value
    return out

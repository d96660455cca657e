"""TSDF fusion of the rendered depth maps -- the sdf the reference's unbounded mesh export hands to marching cubes -- as one HIP kernel
(csrc/tsdf.hip) [REF utils/mesh_utils.py:93-118 reconstruction, 181-234 compute_sdf_perframe + compute_unbounded_tsdf; render.py:132]:

    unbounded_tsdf_torch   the reference's lines 181-234 in the reference's order on plain tensors of any device and float dtype: in
                           float64 the checker, in float32 on the GPU with the maps resident the timing baseline
    TsdfViews              the depth (and colour) maps of V views on the device, packed once, with their full_proj_transforms
    unbounded_tsdf         the same result for a list of samples from one pass: one thread per sample, the views walked inside the kernel
    unbounded_tsdf_grid    the same on a regular grid whose samples the kernel generates, slab by slab (grid_coordinates states them)
    sdf_function           the closure a marching-cubes routine expects in place of the reference's `sdf_function`

What the reference computes, and so what all of these compute -- not what one might expect: `compute_unbounded_tsdf` overwrites `samples`
with the un-normalised WORLD points (line 200) before it tests `norm(samples) > 1` (line 201), so the adaptive truncation
`5 voxel_size / (2 - min(norm, 1.9))` is switched and scaled by the norm of the world point, not of the normalised point the contraction
is defined on.  The running averages start from tsdf = 1 with weight = 1 (a phantom observation of +1) and rgb = 0, and the normal map
the reference samples per view is never used.

Out of scope: the bounded path (`extract_mesh_bounded` is open3d's ScalableTSDFVolume).  Marching cubes on the grid this module fuses
is streetunveiler_amd.mesh.  There is no CPU path for the HIP entry points."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._call import call, ptr

_MAX_CALL = 1 << 30      # samples per launch (the C-ABI takes fewer than 2^31)


def unbounded_tsdf_torch(samples, depthmaps, rgbmaps, full_proj, voxel_size, center=None, radius=None, return_rgb=False, return_weight=False,
                         return_margin=False):
    """The reference's `compute_unbounded_tsdf(samples, inv_contraction, voxel_size, return_rgb)` with `compute_sdf_perframe`, line by
    line and in its order: `samples` [N,3], `depthmaps` [V,1,H,W], `rgbmaps` [V,3,H,W], `full_proj` [V,4,4] (each view's
    full_proj_transform), all of one device and float dtype.  With `center` ([3]) and `radius` the samples are in contracted space and
    `inv_contraction = unnormalize(uncontract(.))` as extract_mesh_unbounded builds it; with center None they are world points.
    -> tsdf [N], then rgb [N,3], weight [N] and margin [N] as asked for.

    `weight - 1` is the number of views that integrated the sample.  `margin` is this restatement's, not the reference's: the distance of
    the sample from its nearest decision, min over ALL views of |1 - |pix.x||, |1 - |pix.y||, |zc| and |sdf + trunc| / trunc, a NaN
    counting as 0."""
    dtype, dev = samples.dtype, samples.device
    samples = samples.detach()
    if center is not None:
        center = torch.as_tensor(center, dtype=dtype, device=dev)

        def uncontract(y):
            mag = torch.linalg.norm(y, ord=2, dim=-1)[..., None]
            return torch.where(mag < 1, y, (1 / (2 - mag) * (y / mag)))
        unnormalize = lambda x: (x * radius) + center
        samples = unnormalize(uncontract(samples))
        mask = torch.linalg.norm(samples, dim=-1) > 1
        # adaptive sdf_truncation
        sdf_trunc = 5 * voxel_size * torch.ones_like(samples[:, 0])
        sdf_trunc[mask] *= 1 / (2 - torch.linalg.norm(samples, dim=-1)[mask].clamp(max=1.9))
    else:
        sdf_trunc = 5 * voxel_size

    def compute_sdf_perframe(points, depthmap, rgbmap, full_proj_transform):
        new_points = torch.cat([points, torch.ones_like(points[..., :1])], dim=-1) @ full_proj_transform
        z = new_points[..., -1:]
        pix_coords = (new_points[..., :2] / new_points[..., -1:])
        mask_proj = ((pix_coords > -1.) & (pix_coords < 1.) & (z > 0)).all(dim=-1)
        sampled_depth = torch.nn.functional.grid_sample(depthmap[None], pix_coords[None, None], mode='bilinear', padding_mode='border',
                                                        align_corners=True).reshape(-1, 1)
        sampled_rgb = torch.nn.functional.grid_sample(rgbmap[None], pix_coords[None, None], mode='bilinear', padding_mode='border',
                                                      align_corners=True).reshape(3, -1).T
        sdf = (sampled_depth - z)
        return sdf, sampled_rgb, mask_proj, pix_coords, z

    tsdfs = torch.ones_like(samples[:, 0]) * 1
    rgbs = torch.zeros((samples.shape[0], 3), dtype=dtype, device=dev)
    weights = torch.ones_like(samples[:, 0])
    margin = torch.full_like(samples[:, 0], float("inf"))
    for i in range(full_proj.shape[0]):
        rgbmap = rgbmaps[i] if rgbmaps is not None else depthmaps[i].expand(3, -1, -1)
        sdf, rgb, mask_proj, pix, z = compute_sdf_perframe(samples, depthmaps[i], rgbmap, full_proj[i])
        # volume integration
        sdf = sdf.flatten()
        if return_margin:
            terms = torch.stack([(1 - pix[:, 0].abs()).abs(), (1 - pix[:, 1].abs()).abs(), z.flatten().abs(), (sdf + sdf_trunc).abs() / sdf_trunc])
            margin = torch.minimum(margin, torch.where(terms.isnan(), torch.zeros_like(terms), terms).min(dim=0).values)
        mask_proj = mask_proj & (sdf > -sdf_trunc)
        sdf = torch.clamp(sdf / sdf_trunc, min=-1.0, max=1.0)[mask_proj]
        w = weights[mask_proj]
        wp = w + 1
        tsdfs[mask_proj] = (tsdfs[mask_proj] * w + sdf) / wp
        rgbs[mask_proj] = (rgbs[mask_proj] * w[:, None] + rgb[mask_proj]) / wp[:, None]
        # update weight
        weights[mask_proj] = wp
    out = (tsdfs,) + ((rgbs,) if return_rgb else ()) + ((weights,) if return_weight else ()) + ((margin,) if return_margin else ())
    return out if len(out) > 1 else tsdfs


# ---- the op --------------------------------------------------------------------------------------------------------------------------
def _on_device(name, t):
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a tensor; got {type(t).__name__}")
    if not t.is_cuda:
        raise L.SurfelRasterError(f"{name} is on {t.device}: the TSDF fusion needs CUDA (ROCm) tensors; there is no CPU path "
                                  "(unbounded_tsdf_torch is the checker)")
    return t


class TsdfViews:
    """The maps of V views, resident on the device: `depthmaps` [V,1,H,W] (or [V,H,W]), `rgbmaps` [V,3,H,W] or None, `full_proj` [V,4,4].
    Any float dtype and any strides are taken; what is kept is float32 and contiguous: `depth` [V,H,W] for the sdf-only call, and with
    colours `packed` [V,H,W,4] = (depth, r, g, b) per pixel, so that a tap of the textured call is one 16-byte load.  Packed here, once."""

    def __init__(self, depthmaps, rgbmaps, full_proj):
        _on_device("depthmaps", depthmaps), _on_device("full_proj", full_proj)
        if depthmaps.dim() == 4 and depthmaps.shape[1] == 1:
            depthmaps = depthmaps[:, 0]
        if depthmaps.dim() != 3 or depthmaps.shape[0] < 1 or depthmaps.shape[1] < 2 or depthmaps.shape[2] < 2:
            raise ValueError(f"depthmaps must be [V,1,H,W] with V >= 1 and H, W >= 2; got {list(depthmaps.shape)}")
        V, H, W = depthmaps.shape
        if tuple(full_proj.shape) != (V, 4, 4):
            raise ValueError(f"full_proj must be [{V},4,4]; got {list(full_proj.shape)}")
        dev = depthmaps.device
        self.V, self.H, self.W, self.device = V, H, W, dev
        self.depth = depthmaps.detach().to(torch.float32).contiguous()
        self.full_proj = full_proj.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.packed = None
        if rgbmaps is not None:
            _on_device("rgbmaps", rgbmaps)
            if tuple(rgbmaps.shape) != (V, 3, H, W):
                raise ValueError(f"rgbmaps must be [{V},3,{H},{W}]; got {list(rgbmaps.shape)}")
            self.packed = torch.empty((V, H, W, 4), dtype=torch.float32, device=dev)
            self.packed[..., 0] = self.depth
            self.packed[..., 1:] = rgbmaps.detach().to(dev).permute(0, 2, 3, 1)

    @classmethod
    def from_renders(cls, cameras, render_fn):
        """Filled the way `GaussianExtractor.reconstruction` fills its lists -- `render_fn(camera)` is `render` with the model, pipe and
        background bound; its 'surf_depth' and 'render' are kept -- but on the GPU, and without the maps the fusion never reads."""
        with torch.no_grad():
            self = cls.__new__(cls)
            for i, cam in enumerate(cameras):
                pkg = render_fn(cam)
                depth, rgb = _on_device("surf_depth", pkg["surf_depth"]), pkg["render"]
                if i == 0:
                    (_, H, W), dev, V = depth.shape, depth.device, len(cameras)
                    self.V, self.H, self.W, self.device = V, H, W, dev
                    self.depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
                    self.packed = torch.empty((V, H, W, 4), dtype=torch.float32, device=dev)
                self.depth[i] = depth[0]
                self.packed[i, :, :, 0] = depth[0]
                self.packed[i, :, :, 1:] = rgb.permute(1, 2, 0)
            if not len(cameras):
                raise ValueError("no cameras")
            self.full_proj = torch.stack([cam.full_proj_transform for cam in cameras]).to(device=self.device, dtype=torch.float32).contiguous()
        return self

    def _c(self, colour):
        if colour and self.packed is None:
            raise ValueError("these views hold no colours (rgbmaps was None)")
        maps = self.packed if colour else self.depth
        return L.SrTsdfViews(maps.data_ptr(), self.full_proj.data_ptr(), self.V, self.H, self.W, 4 if colour else 1)


def _space(voxel_size, center, radius):
    if (center is None) != (radius is None):
        raise ValueError("center and radius go together (both None: world-space samples, constant truncation)")
    voxel_size = float(voxel_size)
    if not voxel_size > 0:
        raise ValueError(f"voxel_size = {voxel_size}: must be positive")
    if center is None:
        return L.SrTsdfSpace(voxel_size, 0, (C.c_float * 3)(0, 0, 0), 1.0)
    c = [float(v) for v in (center.detach().cpu().tolist() if torch.is_tensor(center) else center)]
    if len(c) != 3:
        raise ValueError("center must hold 3 values")
    return L.SrTsdfSpace(voxel_size, 1, (C.c_float * 3)(*c), float(radius))


def _pick(tsdf, rgb, weight, return_rgb, return_weight):
    out = (tsdf,) + ((rgb,) if return_rgb else ()) + ((weight,) if return_weight else ())
    return out if len(out) > 1 else tsdf


def unbounded_tsdf(samples, views, voxel_size, center=None, radius=None, return_rgb=False, return_weight=False):
    """`unbounded_tsdf_torch` for `samples` [N,3] (any float dtype and strides: converted to contiguous float32) on the device of `views`
    through csrc/tsdf.hip -> tsdf [N], then rgb [N,3] and weight [N] as asked for.  One launch on the current stream, no host read-back;
    without `return_rgb` the depth-only maps are read (4 bytes a tap), and the tsdf has the same bits either way."""
    _on_device("samples", samples)
    if samples.dim() != 2 or samples.shape[1] != 3:
        raise ValueError(f"samples must be [N,3]; got {list(samples.shape)}")
    if samples.device != views.device:
        raise ValueError(f"samples is on {samples.device}, the views on {views.device}")
    space, cv = _space(voxel_size, center, radius), views._c(return_rgb)
    pts = samples.detach().to(torch.float32).contiguous()
    N, dev = pts.shape[0], views.device
    tsdf = torch.empty((N,), dtype=torch.float32, device=dev)
    rgb = torch.empty((N, 3), dtype=torch.float32, device=dev) if return_rgb else None
    weight = torch.empty((N,), dtype=torch.float32, device=dev) if return_weight else None
    tail = lambda t, at: None if t is None else ptr(t[at:])
    for at in range(0, N, _MAX_CALL):
        call("sr_tsdf_fuse", dev, C.byref(cv), C.byref(space), min(_MAX_CALL, N - at), ptr(pts[at:]), ptr(tsdf[at:]), tail(rgb, at), tail(weight, at))
    return _pick(tsdf, rgb, weight, return_rgb, return_weight)


def _grid_steps(lo, hi, dims):
    lo, hi = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)
    dims = [int(d) for d in dims]
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"dims must be three positive sizes; got {dims}")
    step = np.array([(hi[a] - lo[a]) / np.float32(dims[a] - 1) if dims[a] > 1 else np.float32(0) for a in range(3)], dtype=np.float32)
    return lo, step, dims


def grid_coordinates(lo, hi, dims):
    """The samples of `unbounded_tsdf_grid`, float32 [nx,ny,nz,3] on the CPU: coordinate i of an axis is fmaf(i, step, lo) with
    step = (hi - lo) / (n - 1) computed in float32 -- the last one is hi only up to that rounding."""
    lo, step, dims = _grid_steps(lo, hi, dims)
    # i * step is exact in float64 and so is the sum for any grid a float32 step can resolve: one rounding, as the fused operation
    axes = [torch.from_numpy((np.arange(dims[a], dtype=np.float64) * np.float64(step[a]) + np.float64(lo[a])).astype(np.float32)) for a in range(3)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)


def unbounded_tsdf_grid(views, lo, hi, dims, voxel_size, center=None, radius=None, slab=None, return_rgb=False, return_weight=False):
    """`unbounded_tsdf` on the regular grid `grid_coordinates(lo, hi, dims)` without that tensor: the kernel generates each sample from
    its index.  `slab`: planes of the first axis per launch (None: as many as one launch takes) -- a 1024^3 grid runs in slabs and needs
    no 12 GB of coordinates.  -> tsdf [nx,ny,nz], then rgb [nx,ny,nz,3] and weight [nx,ny,nz] as asked for; bit for bit what the sample
    list gives."""
    lo, step, dims = _grid_steps(lo, hi, dims)
    nx, ny, nz = dims
    plane = ny * nz
    if plane > _MAX_CALL:
        raise ValueError(f"one plane of {ny} x {nz} samples is more than one launch takes ({_MAX_CALL})")
    slab = max(1, min(int(slab) if slab else nx, _MAX_CALL // plane))
    space, cv, dev = _space(voxel_size, center, radius), views._c(return_rgb), views.device
    c_dims, c_lo, c_step = (C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo.tolist()), (C.c_float * 3)(*step.tolist())
    tsdf = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
    rgb = torch.empty((nx, ny, nz, 3), dtype=torch.float32, device=dev) if return_rgb else None
    weight = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev) if return_weight else None
    tail = lambda t, x0: None if t is None else ptr(t[x0:])
    for x0 in range(0, nx, slab):
        call("sr_tsdf_fuse_grid", dev, C.byref(cv), C.byref(space), c_dims, c_lo, c_step, x0, min(nx, x0 + slab), ptr(tsdf[x0:]), tail(rgb, x0),
             tail(weight, x0))
    return _pick(tsdf, rgb, weight, return_rgb, return_weight)


def sdf_function(views, voxel_size, center=None, radius=None):
    """What the reference's `sdf_function = lambda x: compute_unbounded_tsdf(x, inv_contraction, voxel_size)` is to its marching cubes:
    x [n,3] in contracted space (world space with center None) -> tsdf [n].  A marching-cubes routine may call it chunk by chunk."""
    return lambda x: unbounded_tsdf(x, views, voxel_size, center, radius)

"""Fused allmap post-processing (HIP): one forward kernel and two backward kernels replace the
~25 full-image torch kernels (and the 25 MB per-call host->device upload of the pixel grid) of
[REF /root/reference/gaussian_renderer/__init__.py:152-177; /root/reference/utils/point_utils.py:9-37]."""
from __future__ import annotations

import torch

from . import _lib as L
from ._call import call, ptr


class _PostprocessAllmap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, allmap, viewmatrix, W, H, fovx, fovy, depth_ratio):
        if not allmap.is_cuda:
            raise L.SurfelRasterError("postprocess_allmap needs a CUDA (ROCm) tensor; there is no CPU path")
        allmap = allmap.contiguous().float()
        viewmatrix = viewmatrix.contiguous().float()
        dev = allmap.device
        e = lambda c: torch.empty((c, H, W), dtype=torch.float32, device=dev)
        rend_normal, surf_depth, surf_normal, surf_point = e(3), e(1), e(3), e(3)
        call("sr_postprocess_forward", dev, W, H, fovx, fovy, depth_ratio, ptr(viewmatrix), ptr(allmap), ptr(rend_normal), ptr(surf_depth),
             ptr(surf_normal), ptr(surf_point))
        ctx.save_for_backward(allmap, viewmatrix)
        ctx.cfg = (W, H, fovx, fovy, depth_ratio)
        return rend_normal, surf_depth, surf_normal, surf_point

    @staticmethod
    def backward(ctx, g_rend_normal, g_surf_depth, g_surf_normal, g_surf_point):
        allmap, viewmatrix = ctx.saved_tensors
        W, H, fovx, fovy, depth_ratio = ctx.cfg
        dev = allmap.device
        c = lambda g: None if g is None else g.contiguous().float()
        g_rend_normal, g_surf_depth, g_surf_normal, g_surf_point = c(g_rend_normal), c(g_surf_depth), c(g_surf_normal), c(g_surf_point)
        scratch = torch.empty((6, H, W), dtype=torch.float32, device=dev)
        g_allmap = torch.empty((7, H, W), dtype=torch.float32, device=dev)
        call("sr_postprocess_backward", dev, W, H, fovx, fovy, depth_ratio, ptr(viewmatrix), ptr(allmap), ptr(g_rend_normal), ptr(g_surf_depth),
             ptr(g_surf_normal), ptr(g_surf_point), ptr(scratch), ptr(g_allmap))
        return g_allmap, None, None, None, None, None, None


def postprocess_allmap_fused(viewpoint_camera, depth_ratio: float, allmap: torch.Tensor):
    """-> (rend_normal[3,H,W], surf_depth[1,H,W], surf_normal[3,H,W], surf_point[3,H,W]); differentiable w.r.t. allmap."""
    return _PostprocessAllmap.apply(allmap, viewpoint_camera.world_view_transform, int(viewpoint_camera.image_width),
                                    int(viewpoint_camera.image_height), float(viewpoint_camera.FoVx), float(viewpoint_camera.FoVy),
                                    float(depth_ratio))

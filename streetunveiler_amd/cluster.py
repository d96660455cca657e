"""Exact radius clustering of Gaussians on gfx950 (include/surfel_raster.h sr_cluster_radius, csrc/cluster.hip): the instance selection of
the reference, `GaussianModel.cluster_instance_with_mask` / `cluster_semantic_instance` [REF /root/reference/scene/gaussian_model.py:579-651;
called from inpainting_pipeline/1_selection/1_instance_visualization.py:68].

What those loops are after is the connected components of the graph that joins two active points when their float32 distance
`(abs(a - b) ** 2).sum(-1) ** 0.5` is below `threshold`, each component named by its smallest point index.  That is what the reference's
exact variant (`parallel=False`) computes and what this op returns.  The reference's default (`parallel=True`) is, in its own words, "not
strictly equivalent": it may split a component that this op keeps whole, and its result depends on the order of the points.
There is no CPU path.
"""
import torch

from . import _lib as L
from ._call import buf, call, ptr, workspace


def radius_components(xyz: torch.Tensor, threshold: float, mask: torch.Tensor = None) -> torch.Tensor:
    """int64 [P]: for a point that takes part (mask None or mask[i] true), the smallest index of the points it is connected to through steps
    shorter than `threshold`; -1 for a masked-out point; i for an active point with a NaN / inf coordinate (it is in range of nobody).
    Works on the current stream of xyz's device and reads nothing back to the host."""
    if not xyz.is_cuda or (mask is not None and not mask.is_cuda):
        raise L.SurfelRasterError("xyz and mask must be CUDA (ROCm) tensors; the clustering has no CPU path")
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise L.SurfelRasterError("xyz must have dimensions (num_points, 3)")
    if mask is not None and (mask.ndim != 1 or mask.shape[0] != xyz.shape[0]):
        raise L.SurfelRasterError("mask must have dimensions (num_points,)")
    pts = xyz.detach().float().contiguous()
    n = pts.shape[0]
    active = None if mask is None else (mask if mask.dtype == torch.bool else mask != 0).to(pts.device).contiguous()
    labels = torch.empty((n,), dtype=torch.int64, device=pts.device)
    ws = workspace("sr_cluster_workspace_bytes", pts.device, n)
    call("sr_cluster_radius", pts.device, n, ptr(pts), ptr(active), float(threshold), ptr(labels), *buf(ws))
    return labels


def cluster_instance_with_mask(xyz: torch.Tensor, valid_mask: torch.Tensor, threshold: float = 7e-2) -> torch.Tensor:
    """The `cluster_idx` of GaussianModel.cluster_instance_with_mask(valid_mask, threshold, parallel=False) before prune_invalid_cluster():
    the component's smallest global index where valid_mask holds, -1 elsewhere."""
    return radius_components(xyz, threshold, valid_mask)


def cluster_semantic_instance(xyz: torch.Tensor, semantics_32bit: torch.Tensor, semantic_mask_bit: int, threshold: float = 3e-2) -> torch.Tensor:
    """The `cluster_idx` of GaussianModel.cluster_semantic_instance(semantic_mask_bit, threshold, parallel=False) before
    prune_invalid_cluster(): the points whose semantics_32bit shares a bit with semantic_mask_bit take part."""
    return radius_components(xyz, threshold, (semantics_32bit & semantic_mask_bit) > 0)

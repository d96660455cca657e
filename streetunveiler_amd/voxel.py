"""LiDAR scene initialisation on the GPU (csrc/voxel.hip; include/surfel_raster.h states the semantics once more): the first minute of a
street scene in the reference.

    voxel_down_sample          SemanticPointCloud.voxel_down_sample [REF utils/pcd_utils.py:73-142]: one point per occupied voxel -- the means
                               of its members' positions, colours and normals, its most frequent label -- the voxels dropped whose label is not
                               80 % pure; ascending voxel index; two read-backs (the six bounds; {voxels, kept, bad labels})
    SemanticCloud              the reference class's attributes (points, colors, normals, semantics, semantics_dict) on the device, with its
                               voxel_down_sample(voxel_size) method, so a reader's lines work unchanged
    voxel_down_sample_torch    the checker: the reference's lines in the reference's order, vectorised (a stable sort, unique_consecutive,
                               index_add_ in `mean_dtype`, a [voxels, labels] bincount), on any device.  With mean_dtype=float64 the truth
                               for the means; in float32 on the GPU the stock-torch timing baseline
    create_from_pcd            GaussianModel.create_from_pcd [REF scene/gaussian_model.py:141-164] -> SurfelModel(raw=True)

The voxel of a point, with T the points' dtype (float32 or float64):
    lo = min(points, 0) - T(voxel_size * 0.5),  hi = max(points, 0) + T(voxel_size * 0.5)          (the scalar a Python float, cast to T)
    offset = int((max(hi) - min(lo) + 2 * voxel_size) / voxel_size)                                (host float64)
    c = trunc((p - lo) / T(voxel_size))          ONE IEEE subtraction and ONE IEEE division in T
    index = c.x + offset * c.y + offset**2 * c.z (int64)
A voxel's label is its most frequent one; it is kept iff 5 * max_count >= 4 * n_members in integers.  The reference tests
`1.0 * max / len < 0.8` in float32; the two agree for every voxel of fewer than 2**23 members (both operands are then exact in float32 and
the quotient, correctly rounded, is below float32(0.8) exactly when the true ratio is below 0.8: no ratio of such integers lies between
0.8 and its float32 neighbours; tests/test_voxel_host.py checks all (max, n) with n <= 200).  A tie for the mode needs a share of at
most 0.5, so a tied voxel is always dropped.  Without semantics every voxel is kept.

Deliberate differences from the reference: (1) on a GPU stock torch evaluates `tensor / python_scalar` as a product with the reciprocal;
the contract here is the true division the reference's lines compute on a CPU, so the checker divides by a TENSOR and means the same on
every device; (2) labels must lie in 0..255 (the model elsewhere shifts 1 << label): the kernel counts the others and the call raises;
(3) a NaN or infinite coordinate is refused (the reference silently produces garbage).  Also refused: offset >= 2**21 (offset**3 would
leave int64), a voxel_size that is not positive and finite, row counts that disagree, CPU tensors -- there is no CPU path.

Out of scope: the dataset readers themselves (colouring and labelling the LiDAR returns from the images -- getWaymoPointCloudSemanticFromImage*,
getCertainSemanticMask -- is lidar_label.py).  voxel_down_sample_with_no_grad is the same routine (nothing here records a graph) and is an alias."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from ._call import buf, call, ptr, workspace

MAX_OFFSET = 1 << 21
SH_C0 = 0.28209479177387814
_REAL = (torch.float32, torch.float64)
_NP = {torch.float32: np.float32, torch.float64: np.float64}


# ---- the host arithmetic both sides share -------------------------------------------------------------------------------------------------
def voxel_frame(mins, maxs, voxel_size, dtype):
    """(lo [3] numpy array of the points' dtype, offset int) from the six bounds, exactly as the reference's lines form them."""
    T = _NP[dtype]
    half = T(float(voxel_size) * 0.5)                      # a Python float, then cast
    lo = (np.asarray(mins, dtype=T) - half).astype(T)
    hi = (np.asarray(maxs, dtype=T) + half).astype(T)
    offset = int((float(hi.max()) - float(lo.min()) + 2 * float(voxel_size)) / float(voxel_size))
    return lo, offset


def keep_rule(max_count, members):
    """The purity rule in integers: kept iff the most frequent label holds at least 4/5 of the members."""
    return 5 * max_count >= 4 * members


def _check_voxel_size(voxel_size):
    v = float(voxel_size)
    if not (v > 0 and math.isfinite(v)):
        raise ValueError(f"voxel_size = {voxel_size}: must be positive and finite")
    return v


def _check_offset(offset):
    if offset >= MAX_OFFSET:
        raise ValueError(f"offset = {offset} >= 2**21: offset**3 would leave int64's safe range (a larger voxel_size, or the cloud in parts)")


def _check_rows(points, colors, normals, semantics):
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype not in _REAL:
        raise ValueError(f"points must be a float32 or float64 tensor [n,3]; got {getattr(points, 'dtype', type(points).__name__)} "
                         f"{list(getattr(points, 'shape', []))}")
    n = points.shape[0]
    for name, t in (("colors", colors), ("normals", normals)):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or t.dtype not in _REAL:
            raise ValueError(f"{name} must be a float32 or float64 tensor [n,3]; got {getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))}")
        if t.shape[0] != n:
            raise ValueError(f"{name} has {t.shape[0]} rows, points has {n}")
    if semantics is not None:
        if not torch.is_tensor(semantics) or semantics.dtype.is_floating_point or semantics.dtype.is_complex or semantics.dtype == torch.bool:
            raise ValueError(f"semantics must be an integer tensor [n]; got {getattr(semantics, 'dtype', type(semantics).__name__)}")
        if semantics.numel() != n:
            raise ValueError(f"semantics has {semantics.numel()} rows, points has {n}")
    if n >= 1 << 31:
        raise ValueError(f"{n} points: fewer than 2**31")
    return n


# ---- the container ------------------------------------------------------------------------------------------------------------------------
class SemanticCloud:
    """The reference's SemanticPointCloud on the device: points [n,3], colors / normals [n,3] or None, semantics int32 [n] or None,
    semantics_dict.  Arrays and CPU tensors are moved to `device`; device tensors are taken as they are."""

    def __init__(self, points, colors=None, normals=None, semantics=None, semantics_dict=None, device="cuda"):
        def to(t):
            if t is None:
                return None
            t = torch.as_tensor(t)
            return t if t.is_cuda else t.to(device)
        self.points, self.colors, self.normals = to(points), to(colors), to(normals)
        self.semantics = to(semantics)
        if self.semantics is not None:
            self.semantics = self.semantics.reshape(-1)
        self.semantics_dict = semantics_dict
        _check_rows(self.points, self.colors, self.normals, self.semantics)

    def voxel_down_sample(self, voxel_size):
        out = voxel_down_sample(self.points, voxel_size, self.colors, self.normals, self.semantics)
        out.semantics_dict = self.semantics_dict
        return out

    voxel_down_sample_with_no_grad = voxel_down_sample      # the same routine: nothing here records a graph

    def __len__(self):
        return int(self.points.shape[0])


def _empty_cloud(dev, colors, normals, semantics, return_counts, return_index):
    z3 = lambda: torch.zeros((0, 3), dtype=torch.float32, device=dev)
    cloud = SemanticCloud(z3(), None if colors is None else z3(), None if normals is None else z3(),
                          None if semantics is None else torch.zeros((0,), dtype=torch.int32, device=dev), device=dev)
    extra = []
    if return_counts:
        extra.append(torch.zeros((0,), dtype=torch.int32, device=dev))
    if return_index:
        extra.append(torch.zeros((0,), dtype=torch.int64, device=dev))
    return (cloud, *extra) if extra else cloud


# ---- the fused op -------------------------------------------------------------------------------------------------------------------------
def voxel_down_sample(points, voxel_size, colors=None, normals=None, semantics=None, return_counts=False, return_index=False):
    """-> SemanticCloud of float32 [m,3] tensors and int32 [m] labels on the points' device, rows in ascending voxel index; with
    return_counts also the members per kept voxel (int32 [m]), with return_index the voxel index (int64 [m]).  Runs on the current stream;
    two read-backs.  See the module docstring for the semantics and the refusals."""
    voxel_size = _check_voxel_size(voxel_size)
    n = _check_rows(points, colors, normals, semantics)
    for name, t in (("points", points), ("colors", colors), ("normals", normals), ("semantics", semantics)):
        if t is not None and not t.is_cuda:
            raise L.SurfelRasterError(f"{name} is on {t.device}: voxel_down_sample needs CUDA (ROCm) tensors; there is no CPU path "
                                      "(voxel_down_sample_torch is the checker)")
    dev = points.device
    for name, t in (("colors", colors), ("normals", normals), ("semantics", semantics)):
        if t is not None and t.device != dev:
            raise L.SurfelRasterError(f"{name} is on {t.device}, points on {dev}")
    if n == 0:
        return _empty_cloud(dev, colors, normals, semantics, return_counts, return_index)
    points = points.detach().contiguous()
    colors = None if colors is None else colors.detach().contiguous()
    normals = None if normals is None else normals.detach().contiguous()
    if semantics is not None:      # int32 and int64 go to the kernel as they are; every narrower integer widens to int32 without loss
        semantics = semantics.detach().reshape(-1)
        semantics = semantics.contiguous() if semantics.dtype in (torch.int32, torch.int64) else semantics.to(torch.int32)
    f64 = lambda t: int(t is not None and t.dtype == torch.float64)

    ws = workspace("sr_voxel_workspace_bytes", dev, n)
    bounds = torch.empty((7,), dtype=torch.float64, device=dev)
    call("sr_voxel_bounds", dev, n, ptr(points), f64(points), *buf(ws), ptr(bounds))
    b = bounds.cpu().numpy()                                # the first read-back
    if b[6] != 0 or not np.isfinite(b[:6]).all():
        raise ValueError(f"{int(b[6])} of the {n} points have a NaN or infinite coordinate: refused (the reference would produce garbage)")
    lo, offset = voxel_frame(b[0:3], b[3:6], voxel_size, points.dtype)
    _check_offset(offset)
    lo_host = (C.c_double * 3)(*[float(x) for x in lo])
    counts = torch.empty((3,), dtype=torch.int32, device=dev)
    call("sr_voxel_group", dev, n, ptr(points), f64(points), ptr(semantics), 0 if semantics is None else semantics.element_size(), lo_host,
         float(_NP[points.dtype](voxel_size)), offset, *buf(ws), ptr(counts))
    n_voxels, m, bad = (int(x) for x in counts.cpu().numpy().view(np.uint32))      # the second and last read-back
    if bad:
        raise ValueError(f"{bad} of the {n} labels lie outside 0..255: refused (the model shifts 1 << label)")

    out_points = torch.empty((m, 3), dtype=torch.float32, device=dev)
    out_colors = None if colors is None else torch.empty((m, 3), dtype=torch.float32, device=dev)
    out_normals = None if normals is None else torch.empty((m, 3), dtype=torch.float32, device=dev)
    out_labels = None if semantics is None else torch.empty((m,), dtype=torch.int32, device=dev)
    out_counts = torch.empty((m,), dtype=torch.int32, device=dev) if return_counts else None
    out_index = torch.empty((m,), dtype=torch.int64, device=dev) if return_index else None
    call("sr_voxel_emit", dev, n, ptr(points), f64(points), ptr(colors), f64(colors), ptr(normals), f64(normals), *buf(ws), n_voxels, m,
         ptr(out_points), ptr(out_colors), ptr(out_normals), ptr(out_labels), ptr(out_counts), ptr(out_index))
    cloud = SemanticCloud(out_points, out_colors, out_normals, out_labels, device=dev)
    extra = ([out_counts] if return_counts else []) + ([out_index] if return_index else [])
    return (cloud, *extra) if extra else cloud


# ---- the checker --------------------------------------------------------------------------------------------------------------------------
def voxel_index_torch(points, voxel_size):
    """-> (index int64 [n], offset): the reference's lines, the division by a tensor (the same IEEE division on every device)."""
    dtype = points.dtype
    mins, maxs = points.min(0)[0].cpu().numpy(), points.max(0)[0].cpu().numpy()
    lo, offset = voxel_frame(mins, maxs, voxel_size, dtype)
    lo_t = torch.from_numpy(lo).to(points.device)
    v_t = torch.full((1,), float(voxel_size), dtype=dtype, device=points.device)
    c = ((points - lo_t) / v_t).to(torch.int64)             # the conversion truncates
    scale = torch.tensor([1, offset, offset * offset], dtype=torch.int64, device=points.device)
    return (c * scale).sum(-1), offset


def voxel_down_sample_torch(points, voxel_size, colors=None, normals=None, semantics=None, mean_dtype=torch.float64, return_counts=False,
                            return_index=False, round_means=True):
    """The reference's voxel_down_sample, vectorised, on the tensors' device: -> (points, colors, normals, semantics) as float32 / int32
    tensors (None where not given), then the member counts and the voxel indices where asked for.  round_means=False leaves the means in
    `mean_dtype` (the float64 truth a test compares against).  Raises what voxel_down_sample raises."""
    voxel_size = _check_voxel_size(voxel_size)
    n = _check_rows(points, colors, normals, semantics)
    dev = points.device
    extra = lambda cnt, idx: ([cnt] if return_counts else []) + ([idx] if return_index else [])
    z3 = lambda t: None if t is None else torch.zeros((0, 3), dtype=torch.float32, device=dev)
    if n == 0:
        return (z3(points), z3(colors), z3(normals), None if semantics is None else torch.zeros((0,), dtype=torch.int32, device=dev),
                *extra(torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int64, device=dev)))
    if not bool(torch.isfinite(points).all()):
        raise ValueError("a point has a NaN or infinite coordinate: refused")
    index, offset = voxel_index_torch(points, voxel_size)
    _check_offset(offset)
    order = torch.sort(index, stable=True)[1]
    voxels, inverse, members = torch.unique_consecutive(index[order], return_inverse=True, return_counts=True)
    nv = voxels.shape[0]

    def mean(t):
        if t is None:
            return None
        s = torch.zeros((nv, 3), dtype=mean_dtype, device=dev)
        s.index_add_(0, inverse, t[order].to(mean_dtype))
        s = s / members.to(mean_dtype)[:, None]
        return s.to(torch.float32) if round_means else s

    keep = torch.ones((nv,), dtype=torch.bool, device=dev)
    labels = None
    if semantics is not None:
        sem = semantics.reshape(-1).to(torch.int64)
        if bool(((sem < 0) | (sem > 255)).any()):
            raise ValueError(f"{int(((sem < 0) | (sem > 255)).sum())} labels lie outside 0..255: refused")
        n_labels = int(sem.max()) + 1
        table = torch.bincount(inverse * n_labels + sem[order], minlength=nv * n_labels).reshape(nv, n_labels)
        most = table.max(1)[0]
        first = torch.where(table == most[:, None], torch.arange(n_labels, device=dev)[None, :], n_labels).min(1)[0]   # the lowest of equals
        labels = first.to(torch.int32)
        keep = keep_rule(most, members)
    sel = lambda t: None if t is None else t[keep]
    return (sel(mean(points)), sel(mean(colors)), sel(mean(normals)), sel(labels), *extra(members[keep].to(torch.int32), voxels[keep]))


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def initial_features(colors, max_sh_degree=3):
    """[P,(d+1)^2,3] in this project's one-leaf layout: the DC term RGB2SH(colors) = (colors - 0.5) / C0, the rest zero."""
    colors = colors.float()
    features = torch.zeros((colors.shape[0], (max_sh_degree + 1) ** 2, 3), dtype=torch.float32, device=colors.device)
    features[:, 0, :] = (colors - 0.5) / SH_C0
    return features


def initial_opacity(P, device):
    """inverse_sigmoid(0.1) = log(0.1 / 0.9), [P,1]."""
    x = 0.1 * torch.ones((P, 1), dtype=torch.float32, device=device)
    return torch.log(x / (1 - x))


def initial_scaling(dist2):
    """log(sqrt(clamp_min(dist2, 1e-7))), repeated to the surfel's two columns."""
    return torch.log(torch.sqrt(torch.clamp_min(dist2, 0.0000001)))[..., None].repeat(1, 2)


def create_from_pcd(cloud, spatial_lr_scale, max_sh_degree=3, generator=None):
    """GaussianModel.create_from_pcd [REF scene/gaussian_model.py:141-164] -> SurfelModel(raw=True) on the cloud's device: every parameter a
    leaf that requires grad, `_semantics` int32 [P] as SurfelModel's getters read it (None for a cloud without labels), `max_radii2D` zeros and
    `spatial_lr_scale` on the model, active_sh_degree 0.  The scales come from simple_knn.dist3knn; a cloud of fewer than four points takes
    what dist3knn documents for missing neighbours.  `generator`: a torch.Generator of the cloud's device for the random rotations."""
    from simple_knn._C import dist3knn
    from .gaussian_renderer import SurfelModel
    points = cloud.points
    if not points.is_cuda:
        raise L.SurfelRasterError(f"the cloud is on {points.device}: create_from_pcd needs CUDA (ROCm) tensors; there is no CPU path")
    if cloud.colors is None:
        raise ValueError("create_from_pcd needs a cloud with colours")
    dev = points.device
    xyz = points.detach().float().contiguous().clone()
    P = xyz.shape[0]
    features = initial_features(cloud.colors.detach().to(dev), max_sh_degree)
    scaling = initial_scaling(dist3knn(xyz)) if P > 0 else torch.zeros((0, 2), dtype=torch.float32, device=dev)
    rotation = torch.rand((P, 4), device=dev, generator=generator)
    opacity = initial_opacity(P, dev)
    semantics = None if cloud.semantics is None else cloud.semantics.reshape(-1).to(torch.int32)
    leaf = lambda t: t.contiguous().requires_grad_(True)
    model = SurfelModel(leaf(xyz), leaf(scaling), leaf(rotation), leaf(opacity), leaf(features), semantics=semantics, active_sh_degree=0,
                        max_sh_degree=max_sh_degree, raw=True)
    model.max_radii2D = torch.zeros((P,), dtype=torch.float32, device=dev)
    model.spatial_lr_scale = spatial_lr_scale
    return model

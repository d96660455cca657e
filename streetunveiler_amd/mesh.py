"""Marching cubes on the fused TSDF grid -- the step of the reference's unbounded mesh export that its tree does not hold
(`marching_cubes_with_contraction` of a missing utils.mcube_utils) [REF utils/mesh_utils.py:165-272] -- as four HIP kernels
(csrc/mesh.hip) over the case table tools/make_mc_table.py derives (csrc/mc_table.h, and its twin _mc_table.py read here):

    marching_cubes          a float32 volume [nx,ny,nz] resident on the GPU -> (vertices [Nv,3] float32, faces [Nf,3] int32), welded
    marching_cubes_numpy    the checker: the same table, ordering and sign rules in plain numpy, float64 (the truth) or float32 (the twin)
    extract_mesh_unbounded  views -> unbounded_tsdf_grid -> marching_cubes with the un-contraction -> vertex colours: a SurfelMesh
    contracted_bound        the half-width `R` of the grid the reference computes from the Gaussians' centres

The contract (include/surfel_raster.h states it once more): inside means value < level, strictly.  A grid point owns the vertex of each
of its three forward edges whose ends are finite and differ in `inside`; the vertex sits at t = (level - a) / (b - a) from the lower
end (value a) and is kept at t == 0 and t == 1, so zero-area triangles are legal and the topology stays closed.  The cell whose lowest
corner a grid point is yields its case's triangles iff its eight corners are finite.  Vertices ascend by (linear point index, axis x < y
< z), faces by (linear index of the cell's lowest corner, table order), normals point towards the larger values; no atomics, so equal
inputs give equal bits and the checker's faces can be compared integer for integer.  A grid with an axis of length 1 is an empty mesh.
There is no CPU path for marching_cubes."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import _mc_table as MC
from ._call import buf, call, ptr
from .tsdf import _grid_steps, unbounded_tsdf, unbounded_tsdf_grid

SurfelMesh = collections.namedtuple("SurfelMesh", "vertices faces colors")

_TRI_COUNT = np.array(MC.TRI_COUNT, dtype=np.int64)
_TRI_EDGES = np.array(MC.TRI_EDGES, dtype=np.int64).reshape(256, MC.MAX_TRIANGLES, 3)
_EDGE_OFFSET = np.array([o for o, _ in MC.EDGE_OWNER], dtype=np.int64)      # [12,3]
_EDGE_AXIS = np.array([a for _, a in MC.EDGE_OWNER], dtype=np.int64)


def _frame(lo, hi, dims):
    """-> (lo, step) float32 [3]: `unbounded_tsdf_grid`'s grid for lo and hi, index space (lo 0, step 1) without them."""
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi go together (both None: the vertices are in index space)")
    if lo is None:
        return np.zeros(3, dtype=np.float32), np.ones(3, dtype=np.float32)
    lo, step, _ = _grid_steps(lo, hi, dims)
    return lo, step


def _contraction(center, radius):
    """-> None, or (center float32 [3], radius float32)."""
    if (center is None) != (radius is None):
        raise ValueError("center and radius go together (both None: the vertices stay in grid coordinates)")
    if center is None:
        return None
    c = np.asarray(center.detach().cpu().tolist() if torch.is_tensor(center) else center, dtype=np.float32).reshape(-1)
    if c.shape[0] != 3:
        raise ValueError("center must hold 3 values")
    return c, np.float32(radius)


def marching_cubes(volume, level=0.0, lo=None, hi=None, center=None, radius=None):
    """`volume` [nx,ny,nz] on the GPU (any float dtype and strides: converted to contiguous float32) -> (vertices [Nv,3] float32, faces
    [Nf,3] int32) on its device.  `lo`, `hi`: the grid `unbounded_tsdf_grid(views, lo, hi, volume.shape, ...)` sampled; without them the
    vertices are in index space.  `center`, `radius`: the volume lives in contracted space and every vertex y becomes
    uncontract(y) * radius + center, the world point.  Four launches on the current stream and one read-back of the two counts between
    the second and the third; a workspace of 5 bytes per grid point is held during the call."""
    if not torch.is_tensor(volume):
        raise ValueError(f"volume must be a tensor; got {type(volume).__name__}")
    if not volume.is_cuda:
        raise L.SurfelRasterError(f"volume is on {volume.device}: marching_cubes needs a CUDA (ROCm) tensor; there is no CPU path "
                                  "(marching_cubes_numpy is the checker)")
    if volume.dim() != 3 or min(volume.shape) < 1 or not volume.dtype.is_floating_point:
        raise ValueError(f"volume must be a float tensor [nx,ny,nz] with every axis at least 1; got {volume.dtype} {list(volume.shape)}")
    level = float(level)
    if level != level:
        raise ValueError("level is NaN")
    vol, dev = volume.detach().to(torch.float32).contiguous(), volume.device
    dims = [int(d) for d in vol.shape]
    lo, step = _frame(lo, hi, dims)
    con = _contraction(center, radius)
    space = L.SrTsdfSpace(1.0, 0, (C.c_float * 3)(0, 0, 0), 1.0) if con is None else L.SrTsdfSpace(1.0, 1, (C.c_float * 3)(*con[0].tolist()), float(con[1]))
    c_dims, c_lo, c_step = (C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo.tolist()), (C.c_float * 3)(*step.tolist())
    nbytes = L.load().sr_mesh_workspace_bytes(c_dims)
    if nbytes == 0:
        raise L.SurfelRasterError(f"a volume of {dims[0]} x {dims[1]} x {dims[2]} samples: marching_cubes takes fewer than 2^31 (extract it in parts)")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    call("sr_mesh_count", dev, ptr(vol), c_dims, level, *buf(ws), ptr(counts))
    nv, nf = counts.tolist()      # the one synchronisation
    if nv < 0 or nf < 0:
        raise L.SurfelRasterError("the mesh of this volume has more vertices or face indices than int32 holds (extract it in parts)")
    vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    call("sr_mesh_emit", dev, ptr(vol), c_dims, level, c_lo, c_step, C.byref(space), *buf(ws), nv, nf, ptr(vertices), ptr(faces))
    return vertices, faces


def marching_cubes_numpy(volume, level=0.0, lo=None, hi=None, center=None, radius=None, dtype=np.float64):
    """The checker of `marching_cubes`, no GPU: `volume` (array or CPU tensor, read as float32 -- what the kernels see) -> (vertices [Nv,3]
    `dtype`, faces [Nf,3] int32).  Decisions (inside, finite) are taken on the float32 values and the float32 level, so they are the
    kernels' exactly and the faces must match integer for integer; the interpolation, the coordinates and the un-contraction run in
    `dtype`: float64 is the truth, float32 the twin that rounds where the kernels round (the coordinate is one fused multiply-add)."""
    dtype = np.dtype(dtype).type
    vol32 = np.ascontiguousarray(np.asarray(volume.detach().cpu() if torch.is_tensor(volume) else volume, dtype=np.float32))
    if vol32.ndim != 3 or min(vol32.shape) < 1:
        raise ValueError(f"volume must be [nx,ny,nz] with every axis at least 1; got {list(vol32.shape)}")
    dims = nx, ny, nz = vol32.shape
    lo32, step32 = _frame(lo, hi, dims)
    con = _contraction(center, radius)
    level32 = np.float32(level)
    if level32 != level32:
        raise ValueError("level is NaN")
    if min(dims) < 2:
        return np.zeros((0, 3), dtype=dtype), np.zeros((0, 3), dtype=np.int32)
    finite, inside = np.isfinite(vol32), vol32 < level32
    # ---- vertices: (owning point, axis) in ascending order ----
    owns = np.zeros(dims + (3,), dtype=bool)
    for a in range(3):
        low, high = [slice(None)] * 3, [slice(None)] * 3
        low[a], high[a] = slice(0, -1), slice(1, None)
        low, high = tuple(low), tuple(high)
        owns[low + (a,)] = finite[low] & finite[high] & (inside[low] != inside[high])
    flat = owns.reshape(-1)
    vertex_id = (np.cumsum(flat, dtype=np.int64) - 1).reshape(owns.shape)
    chosen = np.nonzero(flat)[0]
    point, axis = chosen // 3, chosen % 3
    index = np.stack(np.unravel_index(point, dims), axis=1)
    values = vol32.reshape(-1).astype(dtype)
    a_val, b_val = values[point], values[point + np.array([ny * nz, nz, 1], dtype=np.int64)[axis]]
    with np.errstate(all="ignore"):
        t = (dtype(level32) - a_val) / (b_val - a_val)
    position = index.astype(dtype)
    position[np.arange(len(point)), axis] += t
    if dtype is np.float32:      # fmaf: the product and the sum exact in float64, rounded once
        vertices = (position.astype(np.float64) * step32.astype(np.float64) + lo32.astype(np.float64)).astype(np.float32)
    else:
        vertices = position * step32.astype(dtype) + lo32.astype(dtype)
    if con is not None:
        x, y, z = vertices[:, 0], vertices[:, 1], vertices[:, 2]
        with np.errstate(all="ignore"):
            mag = np.sqrt(x * x + y * y + z * z)[:, None]
            vertices = np.where(mag < 1, vertices, (dtype(1) / (dtype(2) - mag)) * (vertices / mag))
        vertices = vertices * dtype(con[1]) + con[0].astype(dtype)
    # ---- faces: (cell, table order) in ascending order ----
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    whole = np.ones(case.shape, dtype=bool)
    for c in range(8):
        corner = tuple(slice(o, n - 1 + o) for o, n in zip((c & 1, (c >> 1) & 1, c >> 2), dims))
        case |= inside[corner].astype(np.int64) << c
        whole &= finite[corner]
    case[~whole] = 0
    cx, cy, cz = np.nonzero(_TRI_COUNT[case] > 0)      # C order: the linear index of the lowest corner ascends
    case = case[cx, cy, cz]
    count, cell = _TRI_COUNT[case], (cx * ny + cy) * nz + cz
    keys, rows = [], []
    for k in range(MC.MAX_TRIANGLES):
        has = count > k
        edges = _TRI_EDGES[case[has], k]      # [m,3]
        off = _EDGE_OFFSET[edges]             # [m,3,3]
        rows.append(vertex_id[cx[has, None] + off[..., 0], cy[has, None] + off[..., 1], cz[has, None] + off[..., 2], _EDGE_AXIS[edges]])
        keys.append(cell[has])
    keys, rows = np.concatenate(keys), np.concatenate(rows)
    faces = rows[np.argsort(keys, kind="stable")].astype(np.int32)
    return vertices.astype(dtype, copy=False), faces


def contracted_bound(xyz, center, radius):
    """[REF utils/mesh_utils.py:253-255] `R`, the half-width of the contracted-space grid: the 0.95 quantile of |contract((xyz - center) /
    radius)| over the Gaussians' centres `xyz` [P,3] plus 0.01, capped at 1.9."""
    xyz = xyz.detach()
    x = (xyz - torch.as_tensor(center, dtype=xyz.dtype, device=xyz.device)) / radius
    mag = torch.linalg.norm(x, ord=2, dim=-1)[..., None]
    contracted = torch.where(mag < 1, x, (2 - (1 / mag)) * (x / mag))
    R = np.quantile(contracted.norm(dim=-1).cpu().numpy(), q=0.95)
    return float(min(R + 0.01, 1.9))


def extract_mesh_unbounded(views, center, radius, bound, resolution=1024, level=0.0, max_range=None):
    """The reference's `extract_mesh_unbounded` from the fusion on: `views` (TsdfViews with colours), `center` and `radius` of the scene
    normalisation, `bound` = the reference's R (`contracted_bound`) -> SurfelMesh(vertices [Nv,3] float32 world points, faces [Nf,3] int32,
    colors [Nv,3] float32), all on the views' device.

    The TSDF is fused on the `resolution`^3 grid over [-bound, bound]^3 of contracted space with voxel_size = 2 radius / resolution
    (`unbounded_tsdf_grid`), meshed at `level` with every vertex un-contracted and un-normalised (`marching_cubes`), and coloured by the
    reference's texturing call: `unbounded_tsdf(vertices, views, voxel_size, return_rgb=True)` on the world points with the constant
    truncation.  `max_range` (off by default; the reference's own routine is not in its tree, so this is this port's choice): faces with a
    vertex farther than max_range from `center` are dropped and the vertices no face uses any more with them, the order kept.

    Memory: the volume (4 bytes a grid point) plus the marching-cubes workspace (5 bytes a grid point) plus the mesh: about 9 GiB at
    1024^3, which fits on one MI355X; the volume and the workspace are released before the colours are sampled."""
    if views.packed is None:
        raise ValueError("these views hold no colours (rgbmaps was None): the mesh's vertex colours need them")
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError(f"resolution = {resolution}: at least 2")
    bound = float(bound)
    if not bound > 0:
        raise ValueError(f"bound = {bound}: must be positive")
    voxel_size = float(radius) * 2 / resolution
    lo, hi = (-bound,) * 3, (bound,) * 3
    volume = unbounded_tsdf_grid(views, lo, hi, (resolution,) * 3, voxel_size, center, radius)
    vertices, faces = marching_cubes(volume, level, lo, hi, center, radius)
    del volume
    if max_range is not None:
        c = torch.as_tensor(_contraction(center, radius)[0], device=vertices.device)
        near = torch.linalg.norm(vertices - c, dim=-1) <= float(max_range)
        faces = faces[near[faces.long()].all(dim=1)]
        used = torch.zeros((vertices.shape[0],), dtype=torch.bool, device=vertices.device)
        used[faces.long().reshape(-1)] = True
        renumber = (torch.cumsum(used, dim=0) - 1).to(torch.int32)
        vertices, faces = vertices[used].contiguous(), renumber[faces.long()].contiguous()
    _, colors = unbounded_tsdf(vertices, views, voxel_size, return_rgb=True)
    return SurfelMesh(vertices, faces, colors)

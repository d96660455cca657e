"""Mesh post-processing on the GPU -- the last step of the reference's mesh export, `post_process_mesh(mesh, cluster_to_keep)` [REF
render.py:145, utils/mesh_utils.py:23-44], which there is six lines around open3d calls (cluster_connected_triangles,
remove_triangles_by_mask, remove_unreferenced_vertices, remove_degenerate_triangles) -- as HIP kernels (csrc/mesh_post.hip) on a mesh that
never leaves the device.  open3d is not needed and not used.

    connected_triangles        faces [nf,3] over n_vertices -> (triangle_clusters [nf] int32, cluster_n_triangles [C] int32): open3d's
                               first two results, by its names and in its order
    post_process_mesh          SurfelMesh or (vertices, faces[, colors]) -> SurfelMesh without the small components
    connected_triangles_numpy, post_process_mesh_numpy    the checkers: plain numpy / Python from the semantics below, no GPU

The semantics (include/surfel_raster.h states them once more):

Edges and components.  An edge of face (a, b, c) is the unordered index pair of (a, b), (b, c) or (c, a); a pair of equal indices is an edge
like any other.  Two faces are adjacent when they have an equal edge: in either winding, for any number of faces on one edge (non-manifold
fans) and for duplicate faces.  Sharing only a vertex joins nothing.  A component is named by its smallest face index (labels[f]); sizes[r]
is the face count of the component at its root r and 0 at every other face.  The dense cluster id of a component is the rank of its root
among the roots: the order in which a sweep over the faces from 0 upwards meets the components.  That should also be the order in which
open3d numbers them; it is UNVERIFIED: open3d is not among this project's dependencies, so nothing here could check it.

Threshold.  n is the k-th largest value of sizes over all nf entries, zeros included, with k = min(cluster_to_keep, nf); threshold =
max(n, min_triangles), min_triangles = 50 by default as in the reference.  A face goes when its component's size is < threshold, strictly,
so ties at the k-th place all stay.

Two deliberate differences from the reference: (1) with fewer components than cluster_to_keep the k-th value is 0 and the floor decides --
every component of at least min_triangles faces stays -- where the reference's np.sort(...)[-cluster_to_keep] raises IndexError;
(2) cluster_area, open3d's third result, is not computed: the reference does not read it.

Order of the removals, as open3d runs them: the faces of the small components; then the vertices no remaining face references, their
colours with them; then the faces with two equal indices.  A vertex that only a degenerate face of a kept component references therefore
stays.  Surviving vertices and faces keep their relative order, vertex and colour rows are copied bit for bit, equal inputs give equal bits.

A face with an index outside [0, n_vertices) is never used to address memory; the kernels count such faces and both entry points raise
ValueError when there is one -- the count comes back in the same read-back as the output counts.  3 nf must fit in int32.  nf == 0 or
nv == 0 is not an error: an empty mesh, no work.  There is no CPU path for the ops themselves."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._call import buf, call, ptr, workspace
from .mesh import SurfelMesh


def _device_faces(faces, what):
    """faces [nf,3] of any integer dtype and strides on the GPU -> contiguous int32 (an int64 index beyond int32 becomes -1: out of range)."""
    if not torch.is_tensor(faces):
        raise ValueError(f"faces must be a tensor; got {type(faces).__name__}")
    if not faces.is_cuda:
        raise L.SurfelRasterError(f"faces is on {faces.device}: {what} needs CUDA (ROCm) tensors; there is no CPU path ({what}_numpy is the checker)")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError(f"faces must be an integer tensor [nf,3]; got {faces.dtype} {list(faces.shape)}")
    faces = faces.detach()
    if faces.dtype != torch.int32:
        wide = faces.to(torch.int64)
        faces = torch.where((wide < 0) | (wide > 0x7FFFFFFF), torch.full_like(wide, -1), wide).to(torch.int32)
    faces = faces.contiguous()
    if 3 * faces.shape[0] > 0x7FFFFFFF:
        raise L.SurfelRasterError(f"{faces.shape[0]} faces: 3 nf does not fit in int32 (process the mesh in parts)")
    return faces


def _components(faces, nv):
    """-> (labels [nf] int32, sizes [nf] int32, n_out_of_range [1] int32, workspace), all on the device; nothing is read back."""
    dev, nf = faces.device, faces.shape[0]
    labels = torch.empty((nf,), dtype=torch.int32, device=dev)
    sizes = torch.empty((nf,), dtype=torch.int32, device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = workspace("sr_mesh_post_workspace_bytes", dev, nv, nf)
    call("sr_mesh_components", dev, ptr(faces), nv, nf, ptr(labels), ptr(sizes), ptr(bad), *buf(ws))
    return labels, sizes, bad, ws


def _out_of_range(n, nv):
    return ValueError(f"{n} face(s) hold a vertex index outside [0, {nv})")


def connected_triangles(faces, n_vertices):
    """`faces` [nf,3] integer tensor on the GPU (int64 or non-contiguous: converted), `n_vertices` -> (triangle_clusters [nf] int32: the
    dense cluster id of every face, cluster_n_triangles [C] int32: the face count of every cluster) on the faces' device, as open3d's
    cluster_connected_triangles names and orders its first two results (the module's docstring: the order is unverified against open3d).
    The components are found by the kernels; the renumbering of the roots to dense ids is a cumulative sum and one masked selection in
    torch, whose size is the call's read-back.  Runs on the current stream."""
    faces = _device_faces(faces, "connected_triangles")
    nv, nf, dev = int(n_vertices), faces.shape[0], faces.device
    if nv < 0:
        raise ValueError(f"n_vertices = {nv}: must not be negative")
    if nf == 0:
        return torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev)
    if nv == 0:
        raise _out_of_range(nf, nv)
    labels, sizes, bad, _ = _components(faces, nv)
    is_root = sizes > 0
    dense = (torch.cumsum(is_root, dim=0, dtype=torch.int32) - 1)
    clusters, counts = dense[labels.long()], sizes[is_root]      # (the masked selection synchronises)
    n_bad = int(bad.item())
    if n_bad:
        raise _out_of_range(n_bad, nv)
    return clusters, counts


def _mesh_parts(mesh):
    if isinstance(mesh, SurfelMesh):
        return mesh.vertices, mesh.faces, mesh.colors
    if isinstance(mesh, (tuple, list)) and len(mesh) in (2, 3):
        return mesh[0], mesh[1], (mesh[2] if len(mesh) == 3 else None)
    raise ValueError("mesh must be a SurfelMesh or a (vertices, faces[, colors]) tuple")


def post_process_mesh(mesh, cluster_to_keep=1000, min_triangles=50):
    """The reference's `post_process_mesh(mesh, cluster_to_keep)`: `mesh` -- a SurfelMesh or (vertices [nv,3], faces [nf,3][, colors [nv,3]
    or None]) on the GPU -- without the components smaller than the cluster_to_keep-th largest (and than `min_triangles`), without the
    vertices left unreferenced and without the degenerate faces: a SurfelMesh(vertices float32, faces int32, colors float32 or None) on the
    same device.  The module's docstring states the threshold, the order of the removals and the two deliberate differences.

    The k-th largest size is taken by torch.topk and stays on the device; the one read-back of the call is {nv_out, nf_out,
    n_out_of_range} between the counting and the emitting launches.  Runs on the current stream; a workspace of 28 bytes a face + 4 a
    vertex is held during the call."""
    vertices, faces, colors = _mesh_parts(mesh)
    cluster_to_keep, min_triangles = int(cluster_to_keep), int(min_triangles)
    if cluster_to_keep < 1:
        raise ValueError(f"cluster_to_keep = {cluster_to_keep}: at least 1")
    if min_triangles < 0:
        raise ValueError(f"min_triangles = {min_triangles}: must not be negative")
    for name, t in (("vertices", vertices), ("colors", colors)):
        if t is None and name == "colors":
            continue
        if not torch.is_tensor(t):
            raise ValueError(f"{name} must be a tensor; got {type(t).__name__}")
        if not t.is_cuda:
            raise L.SurfelRasterError(f"{name} is on {t.device}: post_process_mesh needs CUDA (ROCm) tensors; there is no CPU path "
                                      "(post_process_mesh_numpy is the checker)")
        if t.dim() != 2 or t.shape[1] != 3 or not t.dtype.is_floating_point:
            raise ValueError(f"{name} must be a float tensor [nv,3]; got {t.dtype} {list(t.shape)}")
    faces = _device_faces(faces, "post_process_mesh")
    dev = faces.device
    if vertices.device != dev or (colors is not None and colors.device != dev):
        raise ValueError("vertices, faces and colors must be on one device")
    if colors is not None and colors.shape[0] != vertices.shape[0]:
        raise ValueError(f"{colors.shape[0]} colour rows for {vertices.shape[0]} vertices")
    vertices = vertices.detach().to(torch.float32).contiguous()
    colors = None if colors is None else colors.detach().to(torch.float32).contiguous()
    nv, nf = vertices.shape[0], faces.shape[0]

    def empty():
        none = torch.zeros((0, 3), dtype=torch.float32, device=dev)
        return SurfelMesh(none, torch.zeros((0, 3), dtype=torch.int32, device=dev), None if colors is None else none.clone())

    if nf == 0 or nv == 0:
        return empty()
    labels, sizes, _, ws = _components(faces, nv)
    kth = torch.topk(sizes, min(cluster_to_keep, nf), sorted=True).values[-1:]
    threshold = torch.clamp(kth, min=min_triangles).to(torch.int32)      # stays on the device
    counts = torch.empty((3,), dtype=torch.int32, device=dev)
    call("sr_mesh_filter_count", dev, ptr(faces), nv, nf, ptr(labels), ptr(sizes), ptr(threshold), *buf(ws), ptr(counts))
    nv_out, nf_out, n_bad = counts.tolist()      # the one synchronisation
    if n_bad:
        raise _out_of_range(n_bad, nv)
    if nv_out == 0:
        return empty()
    out_v = torch.empty((nv_out, 3), dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty((nv_out, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((nf_out, 3), dtype=torch.int32, device=dev)
    call("sr_mesh_filter_emit", dev, ptr(faces), nv, nf, ptr(vertices), ptr(colors), *buf(ws), nv_out, nf_out, ptr(out_v), ptr(out_c), ptr(out_f))
    return SurfelMesh(out_v, out_f, out_c)


# ---- the checkers: from the semantics, not from the kernels ---------------------------------------------------------------------------
def _host_faces(faces):
    faces = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
        raise ValueError(f"faces must be an integer array [nf,3]; got {faces.dtype} {list(faces.shape)}")
    return faces.astype(np.int64)


def _labels_numpy(faces, nv):
    """labels [nf]: the smallest face index of every face's component, by an edge dictionary and a sequential union-find."""
    nf = faces.shape[0]
    bad = ((faces < 0) | (faces >= nv)).any(axis=1)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} face(s) hold a vertex index outside [0, {nv})")
    parent = list(range(nf))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first_on_edge = {}
    for f, (a, b, c) in enumerate(faces.tolist()):
        for u, w in ((a, b), (b, c), (c, a)):
            key = (u, w) if u < w else (w, u)
            g = first_on_edge.setdefault(key, f)
            if g != f:
                rf, rg = find(f), find(g)
                if rf != rg:
                    parent[max(rf, rg)] = min(rf, rg)
    return np.array([find(f) for f in range(nf)], dtype=np.int64)


def connected_triangles_numpy(faces, n_vertices):
    """The checker of `connected_triangles`, no GPU: -> (triangle_clusters [nf] int32, cluster_n_triangles [C] int32, labels [nf] int32 --
    the smallest face index of every face's component)."""
    faces = _host_faces(faces)
    labels = _labels_numpy(faces, int(n_vertices))
    roots, clusters, counts = np.unique(labels, return_inverse=True, return_counts=True)      # roots ascend: the sweep's order
    return clusters.reshape(-1).astype(np.int32), counts.astype(np.int32), labels.astype(np.int32)


def post_process_mesh_numpy(vertices, faces, colors=None, cluster_to_keep=1000, min_triangles=50):
    """The checker of `post_process_mesh`, no GPU: arrays or CPU tensors -> (vertices, faces int32, colors or None), rows copied."""
    to_numpy = lambda t: np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
    vertices, faces = to_numpy(vertices), _host_faces(faces)
    colors = None if colors is None else to_numpy(colors)
    if cluster_to_keep < 1 or min_triangles < 0:
        raise ValueError("cluster_to_keep must be at least 1 and min_triangles not negative")
    nv, nf = vertices.shape[0], faces.shape[0]
    if nf == 0 or nv == 0:
        return vertices[:0], np.zeros((0, 3), dtype=np.int32), None if colors is None else colors[:0]
    labels = _labels_numpy(faces, nv)
    sizes = np.bincount(labels, minlength=nf)
    kth = np.sort(sizes)[::-1][min(cluster_to_keep, nf) - 1]
    threshold = max(int(kth), int(min_triangles))
    remaining = faces[sizes[labels] >= threshold]                        # 1: the small components go
    used = np.zeros(nv, dtype=bool)
    used[remaining.reshape(-1)] = True                                   # 2: the vertices nothing references go
    renumber = np.cumsum(used) - 1
    remaining = renumber[remaining]
    a, b, c = remaining[:, 0], remaining[:, 1], remaining[:, 2]
    remaining = remaining[(a != b) & (b != c) & (c != a)]                # 3: the degenerate faces go
    return vertices[used], remaining.astype(np.int32), None if colors is None else colors[used]

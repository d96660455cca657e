"""-m gpu: marching cubes (csrc/mesh.hip) against the float64 checker under the bar of tests/mesh_cases.py on every case -- through the
module and through the raw C-ABI pair, two runs bit for bit -- and the whole export: extract_mesh_unbounded against the same pipeline
assembled from unbounded_tsdf_grid, the float64 checker and unbounded_tsdf, through the PLY writer and back."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from streetunveiler_amd import SurfelMesh, TsdfViews, extract_mesh_unbounded, marching_cubes, read_mesh_ply, unbounded_tsdf, unbounded_tsdf_grid, write_mesh_ply
from streetunveiler_amd import _lib as L
from streetunveiler_amd import mesh as M
from streetunveiler_amd._call import buf, call, ptr
from streetunveiler_amd.ply import mesh_colors_u8
from tests import mesh_cases as mc
from tests import tsdf_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _raw(c):
    """The case through sr_mesh_count / sr_mesh_emit themselves, every buffer the caller's."""
    vol = torch.from_numpy(c.volume).to(DEV)
    dims = list(vol.shape)
    lo, step = M._frame(c.lo, c.hi, dims)
    c_dims, c_lo, c_step = (C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo.tolist()), (C.c_float * 3)(*step.tolist())
    ws = torch.empty((L.load().sr_mesh_workspace_bytes(c_dims),), dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    call("sr_mesh_count", vol.device, ptr(vol), c_dims, c.level, *buf(ws), ptr(counts))
    nv, nf = counts.tolist()
    vertices, faces = torch.empty((nv, 3), dtype=torch.float32, device=DEV), torch.empty((nf, 3), dtype=torch.int32, device=DEV)
    space = None if c.center is None else C.byref(L.SrTsdfSpace(0.0, 1, (C.c_float * 3)(*c.center), c.radius))      # (voxel_size is not read)
    call("sr_mesh_emit", vol.device, ptr(vol), c_dims, c.level, c_lo, c_step, space, *buf(ws), nv, nf, ptr(vertices), ptr(faces))
    return vertices, faces


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_case_against_the_float64_checker(name):
    c, want = mc.case(name), mc.expected(name)
    vol = torch.from_numpy(c.volume).to(DEV)
    vertices, faces = marching_cubes(vol, c.level, c.lo, c.hi, c.center, c.radius)
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32 and vertices.device == vol.device and faces.device == vol.device
    mc.compare(vertices, faces, want, name)
    again = marching_cubes(vol, c.level, c.lo, c.hi, c.center, c.radius)      # no atomics: equal inputs, equal bits
    assert torch.equal(_bits(again[0]), _bits(vertices)) and torch.equal(again[1], faces)
    raw = _raw(c)
    mc.compare(raw[0], raw[1], want, f"{name}, the raw C-ABI pair")
    assert torch.equal(_bits(raw[0]), _bits(vertices)) and torch.equal(raw[1], faces)


def test_float64_and_non_contiguous_volumes_are_converted_and_any_stream_serves():
    c = mc.case("axes_5x4x3")
    vol = torch.from_numpy(c.volume).to(DEV)
    want = marching_cubes(vol, c.level, c.lo, c.hi)
    other = vol.double().permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert not other.is_contiguous() and other.shape == vol.shape
    got = marching_cubes(other, c.level, c.lo, c.hi)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        got = marching_cubes(vol, c.level, c.lo, c.hi)
    stream.synchronize()
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])


def test_argument_errors_leave_the_device_alone():
    mc.check_refusals(L.load())
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        marching_cubes(torch.zeros(3, 3, 3))
    with pytest.raises(ValueError, match="NaN"):
        marching_cubes(torch.zeros(3, 3, 3, device=DEV), float("nan"))
    vertices, faces = marching_cubes(torch.zeros(3, 3, 3, device=DEV))      # still in working order
    assert vertices.shape == (0, 3) and faces.shape == (0, 3)


RESOLUTION, BOUND = 32, 0.9


def test_extract_mesh_unbounded_end_to_end(tmp_path):
    c = tc.case("ring")
    views = TsdfViews(c.depth.to(DEV), c.rgb.to(DEV), c.full_proj.to(DEV))
    mesh = extract_mesh_unbounded(views, tc.CENTER, tc.RADIUS, BOUND, resolution=RESOLUTION)
    assert isinstance(mesh, SurfelMesh) and mesh.vertices.shape[0] > 100 and mesh.faces.shape[0] > 100 and mesh.colors.shape == mesh.vertices.shape
    # the same pipeline, assembled: the fused grid, the float64 checker on it, the reference's texturing call
    voxel_size = 2 * tc.RADIUS / RESOLUTION
    lo, hi = (-BOUND,) * 3, (BOUND,) * 3
    volume = unbounded_tsdf_grid(views, lo, hi, (RESOLUTION,) * 3, voxel_size, tc.CENTER, tc.RADIUS)
    assembled = mc._case(volume.cpu().numpy(), 0.0, lo, hi, tc.CENTER, tc.RADIUS)
    mc.compare(mesh.vertices, mesh.faces, mc.expectation(assembled), "extract_mesh_unbounded")
    _, colors = unbounded_tsdf(mesh.vertices, views, voxel_size, return_rgb=True)
    assert torch.equal(_bits(mesh.colors), _bits(colors)) and bool((mesh.colors > 0).any())
    path = os.path.join(tmp_path, "mesh.ply")
    write_mesh_ply(path, mesh)
    v, f, rgb = read_mesh_ply(path)
    assert np.array_equal(v.view(np.int32), mesh.vertices.cpu().numpy().view(np.int32)) and np.array_equal(f, mesh.faces.cpu().numpy())
    assert np.array_equal(rgb, mesh_colors_u8(mesh.colors.cpu().numpy()))
    # max_range, this port's clipping: faces that reach beyond it go, and the vertices only they used
    clipped = extract_mesh_unbounded(views, tc.CENTER, tc.RADIUS, BOUND, resolution=RESOLUTION, max_range=1.0)
    reach = torch.linalg.norm(clipped.vertices - torch.tensor(tc.CENTER, device=DEV), dim=1)
    assert 0 < clipped.faces.shape[0] < mesh.faces.shape[0] and float(reach.max()) <= 1.0 and clipped.colors.shape == clipped.vertices.shape
    assert int(clipped.faces.max()) == clipped.vertices.shape[0] - 1 and len(torch.unique(clipped.faces)) == clipped.vertices.shape[0]

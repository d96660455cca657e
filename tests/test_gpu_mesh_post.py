"""-m gpu: the mesh post-processing (csrc/mesh_post.hip) against the numpy checker on every case of tests/mesh_post_cases.py -- through
post_process_mesh, through connected_triangles and through the raw C-ABI calls with caller-owned buffers, two runs bit for bit -- the
conversions, a non-default stream, the errors, and the export end to end: extract_mesh_unbounded, post_process_mesh, the PLY writer and
back.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from streetunveiler_amd import SurfelMesh, TsdfViews, connected_triangles, extract_mesh_unbounded, post_process_mesh, read_mesh_ply, write_mesh_ply
from streetunveiler_amd import _lib as L
from streetunveiler_amd import mesh_post as MP
from streetunveiler_amd._call import buf, call, ptr
from streetunveiler_amd.ply import mesh_colors_u8
from tests import mesh_post_cases as pc
from tests import tsdf_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device(c):
    up = lambda a: torch.from_numpy(a.copy()).to(DEV)      # (the cases are read-only arrays)
    return up(c.vertices), up(c.faces), None if c.colors is None else up(c.colors)


def _bits(t):
    return None if t is None else t.contiguous().view(torch.int32)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _raw(c):
    """The case through the C-ABI calls themselves, every buffer the caller's: -> (labels, sizes, vertices, faces, colors)."""
    vertices, faces, colors = _device(c)
    nv, nf = vertices.shape[0], faces.shape[0]
    lib = L.load()
    ws = torch.empty((lib.sr_mesh_post_workspace_bytes(nv, nf),), dtype=torch.uint8, device=DEV)
    labels, sizes = torch.full((nf,), -7, dtype=torch.int32, device=DEV), torch.full((nf,), -7, dtype=torch.int32, device=DEV)
    bad = torch.zeros((1,), dtype=torch.int32, device=DEV)
    counts = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    dev = torch.device(DEV)
    if nf > 0 and nv > 0:
        call("sr_mesh_components", dev, ptr(faces), nv, nf, ptr(labels), ptr(sizes), ptr(bad), *buf(ws))
    k = min(c.cluster_to_keep, nf)
    kth = torch.topk(sizes, k).values[-1:] if k else torch.zeros((1,), dtype=torch.int32, device=DEV)
    threshold = torch.clamp(kth, min=c.min_triangles).to(torch.int32)
    call("sr_mesh_filter_count", dev, ptr(faces), nv, nf, ptr(labels), ptr(sizes), ptr(threshold), *buf(ws), ptr(counts))
    nv_out, nf_out, n_bad = counts.tolist()
    assert n_bad == 0 and int(bad.item()) == 0
    out_v = torch.empty((nv_out, 3), dtype=torch.float32, device=DEV)
    out_c = None if colors is None else torch.empty((nv_out, 3), dtype=torch.float32, device=DEV)
    out_f = torch.empty((nf_out, 3), dtype=torch.int32, device=DEV)
    call("sr_mesh_filter_emit", dev, ptr(faces), nv, nf, ptr(vertices), ptr(colors), *buf(ws), nv_out, nf_out, ptr(out_v), ptr(out_c), ptr(out_f))
    return labels, sizes, out_v, out_f, out_c


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case_against_the_checker(name):
    c, want = pc.case(name), pc.expected(name)
    vertices, faces, colors = _device(c)
    mesh = post_process_mesh((vertices, faces, colors), c.cluster_to_keep, c.min_triangles)
    assert isinstance(mesh, SurfelMesh) and mesh.vertices.device == vertices.device and mesh.faces.device == vertices.device
    pc.compare_mesh(mesh.vertices, mesh.faces, mesh.colors, want, name)
    again = post_process_mesh(SurfelMesh(vertices, faces, colors), c.cluster_to_keep, c.min_triangles)      # equal inputs, equal bits
    assert _same(again, mesh)
    clusters, counts = connected_triangles(faces, vertices.shape[0])
    pc.compare_clusters(clusters, counts, want, name)
    again = connected_triangles(faces, vertices.shape[0])
    assert torch.equal(again[0], clusters) and torch.equal(again[1], counts)
    labels, sizes, *raw = _raw(c)
    pc.compare_mesh(*raw, want, f"{name}, the raw C-ABI calls")
    assert _same(raw, (mesh.vertices, mesh.faces, mesh.colors))
    if faces.shape[0] and vertices.shape[0]:
        assert np.array_equal(labels.cpu().numpy(), want.labels), name
        assert np.array_equal(sizes.cpu().numpy(), np.bincount(want.labels, minlength=faces.shape[0])), name


def test_int64_and_non_contiguous_faces_are_converted_and_any_stream_serves():
    c, want = pc.case("with_colors"), pc.expected("with_colors")
    vertices, faces, colors = _device(c)
    wide = faces.long().t().contiguous().t()
    assert not wide.is_contiguous() and wide.dtype == torch.int64
    mesh = post_process_mesh((vertices, wide, colors), c.cluster_to_keep, c.min_triangles)
    pc.compare_mesh(mesh.vertices, mesh.faces, mesh.colors, want, "int64, non-contiguous faces")
    pc.compare_clusters(*connected_triangles(wide, vertices.shape[0]), want, "int64, non-contiguous faces")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        mesh = post_process_mesh((vertices, faces, colors), c.cluster_to_keep, c.min_triangles)
        clusters, counts = connected_triangles(faces, vertices.shape[0])
    stream.synchronize()
    pc.compare_mesh(mesh.vertices, mesh.faces, mesh.colors, want, "a non-default stream")
    pc.compare_clusters(clusters, counts, want, "a non-default stream")


def test_errors_leave_the_device_alone():
    pc.check_refusals(L.load())
    vertices = torch.zeros((5, 3), device=DEV)
    faces = torch.tensor([[0, 1, 2], [2, 1, 5], [2, 3, 4]], dtype=torch.int32, device=DEV)      # one index equal to nv
    with pytest.raises(ValueError, match=r"1 face\(s\) hold a vertex index outside \[0, 5\)"):
        post_process_mesh((vertices, faces), min_triangles=1)
    with pytest.raises(ValueError, match=r"1 face\(s\) hold a vertex index outside \[0, 5\)"):
        connected_triangles(faces, 5)
    with pytest.raises(ValueError, match="outside"):
        connected_triangles(torch.tensor([[0, 1, 1 << 40]], device=DEV), 5)      # beyond int32: out of range, not wrapped
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        post_process_mesh((vertices.cpu(), faces.cpu()))
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        connected_triangles(faces.cpu(), 5)
    c, want = pc.case("bow_tie"), pc.expected("bow_tie")      # still in working order
    mesh = post_process_mesh(_device(c), c.cluster_to_keep, c.min_triangles)
    pc.compare_mesh(mesh.vertices, mesh.faces, mesh.colors, want, "after the errors")


RESOLUTION, BOUND = 32, 0.9


def test_export_end_to_end(tmp_path):
    c = tc.case("ring")
    views = TsdfViews(c.depth.to(DEV), c.rgb.to(DEV), c.full_proj.to(DEV))
    raw = extract_mesh_unbounded(views, tc.CENTER, tc.RADIUS, BOUND, resolution=RESOLUTION)
    mesh = post_process_mesh(raw, cluster_to_keep=1, min_triangles=3)
    host = [t.cpu().numpy() for t in raw]
    vertices, faces, colors = MP.post_process_mesh_numpy(*host, cluster_to_keep=1, min_triangles=3)
    assert 0 < faces.shape[0] <= host[1].shape[0] and 0 < vertices.shape[0] <= host[0].shape[0]
    pc.compare_mesh(mesh.vertices, mesh.faces, mesh.colors, pc.Expectation(None, None, None, vertices, faces, colors), "the export")
    clusters, counts = connected_triangles(raw.faces, raw.vertices.shape[0])
    want = MP.connected_triangles_numpy(host[1], host[0].shape[0])
    pc.compare_clusters(clusters, counts, pc.Expectation(want[0], want[1], want[2], None, None, None), "the export")
    assert faces.shape[0] == int(counts.max())      # cluster_to_keep = 1: the largest component (a welded marching-cubes face names three vertices)
    path = os.path.join(tmp_path, "mesh_post.ply")
    write_mesh_ply(path, mesh)
    v, f, rgb = read_mesh_ply(path)
    assert np.array_equal(v.view(np.int32), vertices.view(np.int32)) and np.array_equal(f, faces)
    assert np.array_equal(rgb, mesh_colors_u8(colors))

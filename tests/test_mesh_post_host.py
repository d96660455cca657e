"""CPU: the numpy checkers of the mesh post-processing against the literal expectations of tests/mesh_post_cases.py, the properties of
the larger cases, and the C-ABI of csrc/mesh_post.hip as far as it goes without a GPU: refusals, workspace sizes, the prototype table
and the exported names."""
import os
import re

import numpy as np
import pytest
import torch

from streetunveiler_amd import mesh_post as MP
from tests import mesh_post_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(pc.LITERALS))
def test_checker_against_the_literals(name):
    c, want = pc.case(name), pc.expected(name)
    labels, kept_vertices, faces_out = pc.LITERALS[name]
    assert want.labels.tolist() == labels
    roots = sorted(set(labels))
    assert want.clusters.tolist() == [roots.index(l) for l in labels] and want.counts.tolist() == [labels.count(r) for r in roots]
    assert want.faces.tolist() == [list(f) for f in faces_out] and want.faces.dtype == np.int32
    assert pc.same_bits(want.vertices, c.vertices[kept_vertices])
    assert (want.colors is None) == (c.colors is None) and (c.colors is None or pc.same_bits(want.colors, c.colors[kept_vertices]))


def test_colors_do_not_change_the_mesh():
    a, b = pc.expected("with_colors"), pc.expected("without_colors")
    assert a.colors is not None and b.colors is None and np.array_equal(a.faces, b.faces) and pc.same_bits(a.vertices, b.vertices)


@pytest.mark.parametrize("name", ["empty", "empty_no_vertices", "everything_goes"])
def test_empty_results_have_shapes_0_3(name):
    c, want = pc.case(name), pc.expected(name)
    assert want.vertices.shape == (0, 3) and want.faces.shape == (0, 3) and want.faces.dtype == np.int32
    assert (want.colors is None) == (c.colors is None) and (want.colors is None or want.colors.shape == (0, 3))


def test_component_sizes_of_the_larger_cases():
    for name in ("strip_reversed", "strip_bit_reversed"):
        want = pc.expected(name)
        assert want.counts.tolist() == [5000] and want.labels.tolist() == [0] * 5000 and want.faces.shape == (5000, 3)
        assert sorted(map(tuple, want.faces.tolist())) == sorted(map(tuple, pc.case(name).faces.tolist()))      # every vertex is used: no renumbering
    hub = pc.expected("hub")
    assert hub.counts.tolist() == [3000] and np.array_equal(hub.faces, pc.case("hub").faces)
    for nf in (255, 256, 257, 2047, 2048, 2049, 4097):
        want, c = pc.expected(f"block_edges_{nf}"), pc.case(f"block_edges_{nf}")
        assert c.faces.shape == (nf, 3) and sorted(want.counts.tolist()) == [1] * (nf - 60) + [60]
        assert want.faces.shape == (60, 3) and want.vertices.shape == (62, 3) and want.faces.min() == 0 and want.faces.max() == 61
    assert pc.expected("floor_49_50_51").counts.tolist() == [49, 50, 51] and pc.expected("floor_49_50_51").faces.shape == (101, 3)      # strictly below 50 goes
    assert pc.expected("ties").counts.tolist() == [60, 60, 55, 60] and pc.expected("ties").faces.shape == (180, 3)                       # all three 60s stay
    assert pc.expected("keep_one").counts.tolist() == [70, 90, 80] and pc.expected("keep_one").faces.shape == (90, 3)
    assert pc.expected("keep_one").vertices.shape == (92, 3) and pc.same_bits(pc.expected("keep_one").vertices, pc.case("keep_one").vertices[72:164])


def test_three_spheres_are_three_components_of_decreasing_size():
    c, want = pc.case("three_spheres"), pc.expected("three_spheres")
    assert c.vertices.dtype == np.float32 and c.colors.shape == c.vertices.shape
    sizes = want.counts.tolist()
    assert len(sizes) == 3 and sizes[0] > sizes[1] > sizes[2] > 2, sizes
    assert sizes[0] + sizes[1] + sizes[2] == c.faces.shape[0] and want.faces.shape[0] == sizes[0] + sizes[1]      # cluster_to_keep = 2
    assert want.vertices.shape[0] < c.vertices.shape[0] and want.colors.shape == want.vertices.shape


def test_checker_is_independent_of_face_order_and_refuses_what_the_op_refuses():
    c = pc.case("ties")
    perm = np.random.default_rng(3).permutation(c.faces.shape[0])
    _, counts, labels = MP.connected_triangles_numpy(c.faces[perm], c.vertices.shape[0])
    assert sorted(counts.tolist()) == [55, 60, 60, 60] and all(labels[i] == min(np.flatnonzero(labels == labels[i])) for i in range(0, len(labels), 17))
    with pytest.raises(ValueError, match="outside"):
        MP.connected_triangles_numpy(np.array([[0, 1, 2], [0, 1, 3], [1, 2, 0]]), 3)
    with pytest.raises(ValueError, match="outside"):
        MP.post_process_mesh_numpy(np.zeros((3, 3), np.float32), np.array([[0, 1, -1]]))
    with pytest.raises(ValueError):
        MP.post_process_mesh_numpy(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), cluster_to_keep=0)


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from streetunveiler_amd import _lib
    from streetunveiler_amd.build import build
    build()
    return _lib.load()


NAMES = ("sr_mesh_post_workspace_bytes", "sr_mesh_components", "sr_mesh_filter_count", "sr_mesh_filter_emit")


def test_new_symbols_are_declared_exported_and_listed(lib):
    import streetunveiler_amd
    from streetunveiler_amd import _lib
    from streetunveiler_amd.build import SOURCES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "surfel_raster.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.sr_abi_version() == 10      # an addition: nothing that existed changed
    for name in ("connected_triangles", "post_process_mesh", "connected_triangles_numpy", "post_process_mesh_numpy"):
        assert name in streetunveiler_amd.__all__ and callable(getattr(streetunveiler_amd, name)), name
    assert "mesh_post.hip" in [s for s, _ in SOURCES]
    # the union-find exists once: in the header cluster.hip and mesh_post.hip share
    csrc = os.path.join(ROOT, "streetunveiler_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if re.search(r"\bint find_root\(", open(os.path.join(csrc, f)).read())]
    assert holders == ["union_find.h"]


def test_argument_refusals_without_gpu(lib):
    pc.check_refusals(lib)


def test_workspace_size_is_monotone_and_nonzero(lib):
    counts = [0, 1, 255, 256, 257, 4095, 4096, 4097, 100000, 10_000_000]
    for nv in counts:
        sizes = [lib.sr_mesh_post_workspace_bytes(nv, nf) for nf in counts]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (nv, sizes)
    for nf in counts:
        sizes = [lib.sr_mesh_post_workspace_bytes(nv, nf) for nv in counts]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (nf, sizes)
    most = (1 << 31) // 3
    assert lib.sr_mesh_post_workspace_bytes(2**31 - 1, most) >= 28 * most + 4 * (2**31 - 1)
    assert lib.sr_mesh_post_workspace_bytes(1, most + 1) == 0


def test_cpu_tensors_and_wrong_arguments_are_refused():
    from streetunveiler_amd._lib import SurfelRasterError
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        MP.post_process_mesh((v, f))
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        MP.connected_triangles(f, 3)
    with pytest.raises(ValueError, match="cluster_to_keep"):
        MP.post_process_mesh((v, f), cluster_to_keep=0)
    with pytest.raises(ValueError, match="min_triangles"):
        MP.post_process_mesh((v, f), min_triangles=-1)
    with pytest.raises(ValueError, match="SurfelMesh"):
        MP.post_process_mesh(v)
    with pytest.raises(ValueError, match="must be a tensor"):
        MP.connected_triangles(np.zeros((1, 3), np.int32), 3)

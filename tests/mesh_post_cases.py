"""The cases of the mesh post-processing (streetunveiler_amd/mesh_post.py, csrc/mesh_post.hip), by name, shared by the host and the GPU
tests.  Every comparison is exact: integers equal, vertex and colour rows equal bit for bit -- there is no tolerance in this feature.
The tiny cases carry their expected labels, kept faces and kept vertices as literal arrays (LITERALS), so the numpy checker itself is
pinned; the expectation of every case is computed once by that checker (expected) and shared."""
import collections
import ctypes
import functools

import numpy as np

from streetunveiler_amd import mesh_post as MP

Case = collections.namedtuple("Case", "vertices faces colors cluster_to_keep min_triangles")
Expectation = collections.namedtuple("Expectation", "clusters counts labels vertices faces colors")


def _rows(n, seed):
    """n rows of three float32 values, every row different; the first rows hold -0.0, a NaN with a payload, inf and a denormal, which only
    a word-for-word copy carries through."""
    rows = np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32)
    odd = np.array([0x80000000, 0x7FC01234, 0x7F800000, 0x00000001, 0xFFC00001], dtype=np.uint32).view(np.float32)
    flat = rows.reshape(-1)
    flat[:min(len(odd), flat.shape[0])] = odd[:flat.shape[0]]
    return rows


def _case(faces, nv=None, colors=False, cluster_to_keep=1000, min_triangles=50, seed=1):
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    nv = (int(faces.max()) + 1 if faces.size else 0) if nv is None else nv
    return Case(_rows(nv, seed), faces, _rows(nv, seed + 100) if colors else None, cluster_to_keep, min_triangles)


def strip(n, first=0):
    """A triangle strip of n faces over the vertices first .. first + n + 1, windings alternating as in a strip: one component."""
    return [(first + i, first + i + 1, first + i + 2) if i % 2 == 0 else (first + i + 1, first + i, first + i + 2) for i in range(n)]


def isolated(n, first=0):
    """n triangles with three vertices of their own each: n components."""
    return [(first + 3 * i, first + 3 * i + 1, first + 3 * i + 2) for i in range(n)]


def _strips(*lengths):
    faces, first = [], 0
    for n in lengths:
        faces += strip(n, first)
        first += n + 2
    return faces


def _bit_reversed(n):
    bits = max(1, (n - 1).bit_length())
    return sorted(range(n), key=lambda i: int(format(i, f"0{bits}b")[::-1], 2))


def _block_edges(nf):
    """isolated triangles, one strip of 60 faces in the middle of them: nf faces"""
    before = (nf - 60) // 2
    after = nf - 60 - before
    return isolated(before) + strip(60, 3 * before) + isolated(after, 3 * before + 62)


def _three_spheres():
    from streetunveiler_amd.mesh import marching_cubes_numpy
    x, y, z = np.meshgrid(np.arange(24.0), np.arange(20.0), np.arange(16.0), indexing="ij")
    volume = np.full(x.shape, np.inf)
    for (cx, cy, cz), r in (((7.3, 9.1, 7.8), 5.0), ((17.2, 5.9, 6.1), 3.0), ((19.1, 15.2, 11.3), 1.5)):
        volume = np.minimum(volume, np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r)
    vertices, faces = marching_cubes_numpy(volume.astype(np.float32), 0.0, dtype=np.float32)
    return Case(vertices, faces, _rows(vertices.shape[0], 7), 2, 2)


_SMALL = [(1, 2, 4), (4, 2, 5), (6, 7, 8), (8, 7, 9), (9, 7, 10), (3, 3, 0)]      # components of 2, 3 and 1 (degenerate) faces; vertex 11 unused

CASES = {
    "empty": lambda: _case([], nv=4),
    "empty_no_vertices": lambda: _case([], nv=0, colors=True),
    "one_triangle": lambda: _case([(0, 1, 2)], min_triangles=1),
    "shared_edge": lambda: _case([(0, 1, 2), (2, 1, 3)], min_triangles=1),            # the common edge 1-2 against 2-1
    "same_winding": lambda: _case([(0, 1, 2), (1, 2, 3)], min_triangles=1),           # the common edge 1-2 in both
    "bow_tie": lambda: _case([(0, 1, 2), (2, 3, 4), (4, 3, 5)], cluster_to_keep=1, min_triangles=1),      # face 0 touches the others in vertex 2 only
    "fan_on_one_edge": lambda: _case([(0, 1, 2), (1, 0, 3), (0, 1, 4), (0, 1, 5), (1, 0, 6)], min_triangles=1),
    "duplicate_faces": lambda: _case([(0, 1, 2), (0, 1, 2), (2, 1, 0), (3, 4, 5)], cluster_to_keep=1, min_triangles=1),
    # faces 2 (a, a, b), 3 (a, a, a) and 4 (a, a, b) hang on the two good faces through the edges 1-3 and 3-3; vertex 5 is used by face 4 alone;
    # vertex 4 by nothing; the triangle 6-7-8 is a component of its own and goes
    "degenerate_inside_kept": lambda: _case([(0, 1, 2), (2, 1, 3), (3, 3, 1), (3, 3, 3), (3, 3, 5), (6, 7, 8)], cluster_to_keep=1, min_triangles=1),
    "unreferenced_vertices": lambda: _case([(1, 2, 4), (4, 2, 5)], nv=8, colors=True, min_triangles=1),      # 0, 3, 6 and 7 are unused
    "strip_reversed": lambda: _case(strip(5000)[::-1]),
    "strip_bit_reversed": lambda: _case(np.array(strip(5000))[_bit_reversed(5000)]),
    "hub": lambda: _case([(0, 1 + i, 1 + (i + 1) % 3000) for i in range(3000)]),
    "floor_49_50_51": lambda: _case(_strips(49, 50, 51), colors=True),
    "ties": lambda: _case(_strips(60, 60, 55, 60), cluster_to_keep=2, min_triangles=2),
    "keep_one": lambda: _case(_strips(70, 90, 80), cluster_to_keep=1, min_triangles=2),
    "everything_goes": lambda: _case(_strips(10, 20) + isolated(5, 40), colors=True),
    "three_spheres": _three_spheres,
    "with_colors": lambda: _case(_SMALL, nv=12, colors=True, cluster_to_keep=1, min_triangles=2),
    "without_colors": lambda: _case(_SMALL, nv=12, colors=False, cluster_to_keep=1, min_triangles=2),
}
for _nf in (255, 256, 257, 2047, 2048, 2049, 4097):
    CASES[f"block_edges_{_nf}"] = functools.partial(lambda nf: _case(_block_edges(nf), colors=nf == 257), _nf)

# name -> (labels, kept vertices as indices into the input, the output faces), written down by hand from the semantics
LITERALS = {
    "one_triangle": ([0], [0, 1, 2], [(0, 1, 2)]),
    "shared_edge": ([0, 0], [0, 1, 2, 3], [(0, 1, 2), (2, 1, 3)]),
    "same_winding": ([0, 0], [0, 1, 2, 3], [(0, 1, 2), (1, 2, 3)]),
    "bow_tie": ([0, 1, 1], [2, 3, 4, 5], [(0, 1, 2), (2, 1, 3)]),
    "fan_on_one_edge": ([0, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5, 6], [(0, 1, 2), (1, 0, 3), (0, 1, 4), (0, 1, 5), (1, 0, 6)]),
    "duplicate_faces": ([0, 0, 0, 3], [0, 1, 2], [(0, 1, 2), (0, 1, 2), (2, 1, 0)]),
    "degenerate_inside_kept": ([0, 0, 0, 0, 0, 5], [0, 1, 2, 3, 5], [(0, 1, 2), (2, 1, 3)]),
    "unreferenced_vertices": ([0, 0], [1, 2, 4, 5], [(0, 1, 2), (2, 1, 3)]),
    "with_colors": ([0, 0, 2, 2, 2, 5], [6, 7, 8, 9, 10], [(0, 1, 2), (2, 1, 3), (3, 1, 4)]),      # the largest component alone: threshold 3
    "without_colors": ([0, 0, 2, 2, 2, 5], [6, 7, 8, 9, 10], [(0, 1, 2), (2, 1, 3), (3, 1, 4)]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for a in (c.vertices, c.faces, c.colors):
        if a is not None:
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """The checker's results for the case: computed once, shared, read-only."""
    c = case(name)
    clusters, counts, labels = MP.connected_triangles_numpy(c.faces, c.vertices.shape[0])
    vertices, faces, colors = MP.post_process_mesh_numpy(c.vertices, c.faces, c.colors, c.cluster_to_keep, c.min_triangles)
    for a in (clusters, counts, labels, vertices, faces, colors):
        if a is not None:
            a.setflags(write=False)
    return Expectation(clusters, counts, labels, vertices, faces, colors)


def _host(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def same_bits(got, want):
    got, want = np.ascontiguousarray(_host(got)), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def compare_mesh(vertices, faces, colors, want, what):
    """The output mesh against the expectation: exact."""
    assert _host(faces).dtype == np.int32 and _host(faces).shape == want.faces.shape and np.array_equal(_host(faces), want.faces), what
    assert same_bits(vertices, want.vertices), what
    assert (colors is None) == (want.colors is None), what
    if colors is not None:
        assert same_bits(colors, want.colors), what


def compare_clusters(clusters, counts, want, what):
    assert _host(clusters).dtype == np.int32 and np.array_equal(_host(clusters), want.clusters), what
    assert _host(counts).dtype == np.int32 and np.array_equal(_host(counts), want.counts), what


def check_refusals(lib):
    """Every refusal of the sr_mesh_* post-processing calls comes before the first HIP call: made here on dummy host pointers, no GPU
    needed."""
    INVALID, SHORT, UNSUPPORTED = -1, -3, -4
    dummy = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(dummy) + 255) & ~255
    big, too_many = 1 << 40, (1 << 31) // 3 + 1
    need = lib.sr_mesh_post_workspace_bytes(10, 20)
    assert need >= 28 * 20 + 4 * 10
    assert lib.sr_mesh_post_workspace_bytes(-1, 20) == 0 and lib.sr_mesh_post_workspace_bytes(10, -1) == 0 and lib.sr_mesh_post_workspace_bytes(10, too_many) == 0
    components = [((None, 10, 20, p, p, p, p, big, None), INVALID, b"faces is NULL"),
                  ((p, -1, 20, p, p, p, p, big, None), INVALID, b"negative"),
                  ((p, 10, -20, p, p, p, p, big, None), INVALID, b"negative"),
                  ((p, 10, too_many, p, p, p, p, big, None), UNSUPPORTED, b"int32"),
                  ((p, 10, 20, None, p, p, p, big, None), INVALID, b"labels / sizes is NULL"),
                  ((p, 10, 20, p, None, p, p, big, None), INVALID, b"labels / sizes is NULL"),
                  ((p, 10, 20, p, p, None, p, big, None), INVALID, b"n_out_of_range is NULL"),
                  ((p, 10, 20, p, p, p, None, big, None), INVALID, b"workspace is NULL"),
                  ((p, 10, 20, p, p, p, p, need - 1, None), SHORT, b"workspace"),
                  ((p, 10, 20, p, p, p, p + 4, big, None), INVALID, b"16-B aligned"),
                  ((p + 2, 10, 20, p, p, p, p, big, None), INVALID, b"4-B aligned"),
                  ((p, 0, 20, p, p, p, p, big, None), INVALID, b"without vertices")]
    count = [((None, 10, 20, p, p, p, p, big, p, None), INVALID, b"faces is NULL"),
             ((p, 10, -20, p, p, p, p, big, p, None), INVALID, b"negative"),
             ((p, 10, too_many, p, p, p, p, big, p, None), UNSUPPORTED, b"int32"),
             ((p, 10, 20, None, p, p, p, big, p, None), INVALID, b"labels / sizes is NULL"),
             ((p, 10, 20, p, None, p, p, big, p, None), INVALID, b"labels / sizes is NULL"),
             ((p, 10, 20, p, p, None, p, big, p, None), INVALID, b"threshold is NULL"),
             ((p, 10, 20, p, p, p, None, big, p, None), INVALID, b"workspace is NULL"),
             ((p, 10, 20, p, p, p, p, need - 1, p, None), SHORT, b"workspace"),
             ((p, 10, 20, p, p, p, p, big, None, None), INVALID, b"counts is NULL")]
    emit = [((None, 10, 20, p, p, p, big, 3, 1, p, p, p, None), INVALID, b"faces is NULL"),
            ((p, -10, 20, p, p, p, big, 3, 1, p, p, p, None), INVALID, b"negative"),
            ((p, 10, too_many, p, p, p, big, 3, 1, p, p, p, None), UNSUPPORTED, b"int32"),
            ((p, 10, 20, p, p, None, big, 3, 1, p, p, p, None), INVALID, b"workspace is NULL"),
            ((p, 10, 20, p, p, p, need - 1, 3, 1, p, p, p, None), SHORT, b"workspace"),
            ((p, 10, 20, p, p, p, big, -3, 1, p, p, p, None), INVALID, b"negative"),
            ((p, 10, 20, p, p, p, big, 3, -1, p, p, p, None), INVALID, b"negative"),
            ((p, 10, 20, p, p, p, big, 11, 1, p, p, p, None), INVALID, b"more than"),
            ((p, 10, 20, p, p, p, big, 3, 21, p, p, p, None), INVALID, b"more than"),
            ((p, 10, 20, p, p, p, big, 0, 1, p, p, p, None), INVALID, b"without vertices"),
            ((p, 10, 20, None, p, p, big, 3, 1, p, p, p, None), INVALID, b"vertices / vertices_out is NULL"),
            ((p, 10, 20, p, p, p, big, 3, 1, None, p, p, None), INVALID, b"vertices / vertices_out is NULL"),
            ((p, 10, 20, p, p, p, big, 3, 1, p, None, p, None), INVALID, b"colors_out is NULL"),
            ((p, 10, 20, p, None, p, big, 3, 1, p, None, None, None), INVALID, b"faces_out is NULL")]
    for fn, rows in ((lib.sr_mesh_components, components), (lib.sr_mesh_filter_count, count), (lib.sr_mesh_filter_emit, emit)):
        for args, code, fragment in rows:
            rc = fn(*args)
            assert rc == code and fragment in lib.sr_last_error(), (args, rc, fragment, lib.sr_last_error())
    # no face, no vertex, nothing to emit: no error and no work
    assert lib.sr_mesh_components(None, 10, 0, None, None, p, None, 0, None) == 0
    assert lib.sr_mesh_filter_emit(None, 10, 0, None, None, None, 0, 0, 0, None, None, None, None) == 0
    assert lib.sr_mesh_filter_emit(None, 0, 20, None, None, None, 0, 0, 0, None, None, None, None) == 0
    assert lib.sr_mesh_filter_emit(p, 10, 20, p, None, p, big, 0, 0, None, None, None, None) == 0

"""CPU: the marching-cubes case table is the one tools/make_mc_table.py derives now; the checker (marching_cubes_numpy) over it is held
to what no restatement can fake -- closed, consistently oriented surfaces on random sign volumes that exercise all 256 cases, the Euler
characteristic, the sign and size of the enclosed volume and vertices on the level set for a sphere and a torus; the bar of
tests/mesh_cases.py rejects the wrong implementations one can think of; the C-ABI is declared, exported and refuses bad arguments before
it touches a GPU; the mesh PLY survives a round trip."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from streetunveiler_amd import _mc_table as MC
from streetunveiler_amd import mesh as M
from streetunveiler_amd import ply
from tests import mesh_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# seeds whose 6 x 5 x 4 random cells together show every one of the 256 cases (asserted below)
SIGN_SEEDS = tuple(range(24))


def _generator():
    spec = importlib.util.spec_from_file_location("make_mc_table", os.path.join(ROOT, "tools", "make_mc_table.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_committed_table_is_what_the_generator_derives():
    g = _generator()
    table, max_tris = g.generate()
    header, twin = g.emit(table, max_tris)
    assert open(g.HEADER).read() == header and open(g.TWIN).read() == twin
    assert max_tris == MC.MAX_TRIANGLES == max(MC.TRI_COUNT) and len(MC.TRI_COUNT) == 256 and len(MC.TRI_EDGES) == 256 * 3 * max_tris
    assert [len(t) for t in table] == list(MC.TRI_COUNT) and MC.TRI_COUNT[0] == MC.TRI_COUNT[255] == 0
    for case, tris in enumerate(table):
        row = MC.TRI_EDGES[case * 3 * max_tris:(case + 1) * 3 * max_tris]
        assert list(row[:3 * len(tris)]) == [e for t in tris for e in t] and set(row[3 * len(tris):]) <= {255}
    # the header states the conventions the kernels and the checker read the table by
    text = open(g.HEADER).read()
    for phrase in ("corner c of a cell sits at offset", "edge e = 4 * axis + k", "inside means value < level, strictly", "owned by the grid point at its lower end"):
        assert phrase in text, phrase
    assert g.main(["--check"]) == 0


def _sign_volume(seed):
    """6 x 5 x 4 cells of random +-1 corners inside a shell of +1."""
    v = np.ones((9, 8, 7), dtype=np.float32)
    v[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).choice([-1.0, 1.0], size=(7, 6, 5))
    return v


def _cases_of(volume, level=0.0):
    inside = volume < level
    nx, ny, nz = volume.shape
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        case |= inside[(c & 1):nx - 1 + (c & 1), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c >> 2):nz - 1 + (c >> 2)].astype(np.int64) << c
    return case


def test_random_sign_volumes_are_closed_and_consistently_oriented_over_all_256_cases():
    seen = set()
    for seed in SIGN_SEEDS:
        v = _sign_volume(seed)
        seen |= set(_cases_of(v).reshape(-1).tolist())
        vertices, faces = M.marching_cubes_numpy(v)
        assert len(faces) and faces.min() == 0 and faces.max() == len(vertices) - 1 and len(np.unique(faces)) == len(vertices)
        und, counts, imbalance = mc.edge_counts(faces)
        assert imbalance == 0, f"seed {seed}: a directed edge occurs more often than its reverse"
        assert (counts % 2 == 0).all(), f"seed {seed}: an undirected edge occurs an odd number of times"
        assert mc.signed_volume(vertices, faces) > 0
    assert seen == set(range(256)), sorted(set(range(256)) - seen)


@pytest.mark.parametrize("shape", ["sphere", "torus"])
def test_analytic_surfaces(shape):
    n, h = mc.N_ANALYTIC, 2.0 / (mc.N_ANALYTIC - 1)
    if shape == "sphere":
        volume, chi, r = mc.sphere_volume(), 2, mc.SPHERE_R
        analytic = 4.0 / 3.0 * np.pi * r ** 3
        area = lambda d: 4.0 * np.pi * (r + d) ** 2
    else:
        volume, chi, r = mc.torus_volume(), 0, mc.TORUS_r
        analytic = 2.0 * np.pi ** 2 * mc.TORUS_R * r ** 2
        area = lambda d: 4.0 * np.pi ** 2 * mc.TORUS_R * (r + d)
    volume = volume.astype(np.float32)
    assert (volume != 0).all() and np.isfinite(volume).all()      # no sample equals the level
    vertices, faces = M.marching_cubes_numpy(volume, 0.0, (-1.0,) * 3, (1.0,) * 3)
    und, counts, imbalance = mc.edge_counts(faces)
    assert (counts == 2).all() and imbalance == 0
    assert mc.euler(vertices, faces) == chi
    # The volume is a distance function: along a line its second derivative is at most the largest curvature of the level set it crosses,
    # 1 / (r - h) within one cell of the surface (r the sphere's radius, the torus's minor radius; its other curvature is smaller since
    # r < R - r).  Linear interpolation along a cell edge of length h puts a vertex within h^2 / 8 * 1 / (r - h) of the surface, and a
    # triangle, whose edges are at most sqrt(3) h long, sags at most 3 h^2 / (8 r) below its vertices: the mesh stays within
    # delta = h^2 / (2 (r - h)) of the surface, and the volumes differ by at most delta times the area of the surface pushed out by delta.
    delta = h * h / (2.0 * (r - h))
    got = mc.signed_volume(vertices, faces)
    print(f"{shape}: volume {got:.6f}, analytic {analytic:.6f}, bound {delta * area(delta):.6f}; Nv {len(vertices)}, Nf {len(faces)}")
    assert got > 0 and abs(got - analytic) <= delta * area(delta)
    # every vertex lies on the level set of the trilinear interpolant (on a cell edge that is the linear one), to float64 rounding
    index_vertices, index_faces = M.marching_cubes_numpy(volume, 0.0)
    assert np.array_equal(index_faces, faces)
    on_edge = (index_vertices != np.round(index_vertices)).sum(axis=1)
    assert (on_edge == 1).all()      # two coordinates are grid indices, the third lies strictly between two of them
    assert np.abs(mc.trilinear(volume, index_vertices)).max() <= 1e-14 * n
    assert np.abs(index_vertices * h - 1.0 - vertices).max() <= 1e-6      # (step is the float32 quotient)


def test_what_the_named_cases_are_there_for():
    for name in mc.CASES:
        c, want = mc.case(name), mc.expected(name)
        assert c.volume.dtype == np.float32 and want.faces.dtype == np.int32 and want.vertices.dtype == np.float64
        if len(want.faces):
            assert want.faces.min() >= 0 and want.faces.max() < len(want.vertices)
    for name in ("flat_1x5x6", "flat_5x6x1", "all_above", "all_at_level"):
        assert len(mc.expected(name).vertices) == 0 and len(mc.expected(name).faces) == 0, name
    assert (mc.case("flat_1x5x6").volume < 0).any()      # there are crossed edges, but no cell
    assert len(mc.expected("one_cell").faces) >= 1 and len(mc.expected("noise_40").vertices) > 3 * 4096      # several chunks hold vertices
    assert mc.case("noise_40").volume.size > 4 * 4096
    c, want = mc.case("corners_at_level"), mc.expected("corners_at_level")
    assert (c.volume == 0).sum() > 20 and len(want.faces)
    a, b, d = (want.vertices[want.faces[:, k]] for k in range(3))
    assert (np.linalg.norm(np.cross(b - a, d - a), axis=1) == 0).any()      # vertices at t == 0 or t == 1 are kept: zero-area triangles
    und, counts, imbalance = mc.edge_counts(M.marching_cubes_numpy(np.pad(c.volume, 1, constant_values=1.0))[1])
    assert imbalance == 0 and (counts % 2 == 0).all()      # ... and inside a shell of +1 the surface is closed and consistently oriented
    c, want = mc.case("nan_and_inf"), mc.expected("nan_and_inf")
    clean = M.marching_cubes_numpy(np.nan_to_num(c.volume, nan=0.5, posinf=0.5))
    assert np.isnan(c.volume).sum() == 1 and np.isinf(c.volume).sum() == 1 and len(want.faces) < len(clean[1]) and len(want.vertices) < len(clean[0])
    assert np.isfinite(want.vertices).all()
    assert mc.case("level_0.25").level == 0.25 and len(mc.expected("level_0.25").faces)
    crossing = mc.expected("sphere_across_the_unit_ball")
    y = M.marching_cubes_numpy(mc.case("sphere_across_the_unit_ball").volume, 0.0, *mc.WIDE)[0]
    norms = np.linalg.norm(y, axis=1)
    assert (norms < 0.95).any() and (norms > 1.05).any() and norms.max() < 1.5 and len(crossing.vertices) == len(y)
    world = np.where(norms[:, None] < 1, y, y / norms[:, None] / (2 - norms[:, None])) * mc.RADIUS + np.array(mc.CENTER, dtype=np.float32).astype(np.float64)
    assert np.abs(world - crossing.vertices).max() <= 1e-12
    plain, moved = mc.expected("sphere"), mc.expected("sphere_uncontracted")
    assert np.array_equal(plain.faces, moved.faces)
    assert np.abs(plain.vertices * mc.RADIUS + np.array(mc.CENTER, dtype=np.float32).astype(np.float64) - moved.vertices).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_the_float32_twin_passes_the_bar(name):
    c, want = mc.case(name), mc.expected(name)
    v32, f32 = mc.run_checker(c, np.float32)
    mc.compare(v32, f32, want, f"{name}, the float32 checker")
    mc.compare(torch.from_numpy(v32), torch.from_numpy(f32), want, f"{name}, as tensors")


@pytest.mark.parametrize("name", sorted(mc.MUTANTS))
def test_the_bar_rejects_wrong_implementations(name):
    vertices, faces = mc.mutant(name)
    assert len(faces)
    with pytest.raises(AssertionError):
        mc.compare(vertices, faces, mc.expected(mc.MUTANTS[name]), f"{name} on {mc.MUTANTS[name]}")


def test_mesh_ply_round_trip(tmp_path):
    want = mc.expected("sphere")
    vertices, faces = want.vertices.astype(np.float32), want.faces
    colors = np.random.default_rng(3).uniform(-0.1, 1.1, size=vertices.shape).astype(np.float32)
    colors[0] = np.nan
    path = os.path.join(tmp_path, "mesh.ply")
    ply.write_mesh_ply(path, M.SurfelMesh(torch.from_numpy(vertices), torch.from_numpy(faces), torch.from_numpy(colors)))
    v, f, c = ply.read_mesh_ply(path)
    assert v.dtype == np.float32 and f.dtype == np.int32 and c.dtype == np.uint8
    assert np.array_equal(v.view(np.int32), vertices.view(np.int32)) and np.array_equal(f, faces) and np.array_equal(c, ply.mesh_colors_u8(colors))
    assert c.min() == 0 and c.max() == 255 and not c[0].any()
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode()
    assert "format binary_little_endian 1.0" in head and f"element vertex {len(v)}" in head and f"element face {len(f)}" in head
    assert "property list uchar int vertex_indices" in head and "property uchar red" in head
    assert os.path.getsize(path) == len(head) + len("end_header\n") + 15 * len(v) + 13 * len(f)
    ply.write_mesh_ply(path, (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), None))      # an empty mesh is a file too
    v, f, c = ply.read_mesh_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    with pytest.raises(ValueError, match="not the layout"):
        ply.save_ply(path, np.zeros((1, 3)), np.zeros((1, 1, 3)), np.zeros((1, 15, 3)), np.zeros((1, 1)), np.zeros((1, 2)), np.zeros((1, 4)), np.zeros(1))
        ply.read_mesh_ply(path)


def test_contracted_bound_is_the_reference_quantile():
    xyz = torch.from_numpy(np.random.default_rng(5).normal(size=(2001, 3)) * 3.0)
    center, radius = (0.5, -0.25, 1.0), 2.0
    x = (xyz.numpy() - np.array(center)) / radius
    mag = np.linalg.norm(x, axis=1, keepdims=True)
    norms = np.linalg.norm(np.where(mag < 1, x, (2 - 1 / mag) * (x / mag)), axis=1)
    assert abs(M.contracted_bound(xyz, center, radius) - min(np.quantile(norms, 0.95) + 0.01, 1.9)) < 1e-12
    assert M.contracted_bound(xyz * 100, center, radius) == 1.9 and 0.01 < M.contracted_bound(xyz * 1e-3, (0.0, 0.0, 0.0), radius) < 0.02


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from streetunveiler_amd import _lib
    from streetunveiler_amd.build import build
    build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_listed(lib):
    import streetunveiler_amd
    from streetunveiler_amd import _lib
    from streetunveiler_amd.build import SOURCES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "surfel_raster.h")).read(), flags=re.S)
    for name in ("sr_mesh_workspace_bytes", "sr_mesh_count", "sr_mesh_emit"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.sr_abi_version() == 10      # an addition: nothing that existed changed
    for name in ("marching_cubes", "marching_cubes_numpy", "extract_mesh_unbounded", "contracted_bound", "SurfelMesh", "write_mesh_ply", "read_mesh_ply"):
        assert name in streetunveiler_amd.__all__ and callable(getattr(streetunveiler_amd, name)), name
    assert ("mesh.hip", ["-ffp-contract=off"]) in [(s, list(f)) for s, f in SOURCES]


def test_argument_refusals_without_gpu(lib):
    mc.check_refusals(lib)


def test_cpu_tensors_and_wrong_arguments_are_refused():
    from streetunveiler_amd._lib import SurfelRasterError
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        M.marching_cubes(torch.zeros(3, 3, 3))
    with pytest.raises(ValueError, match="must be a tensor"):
        M.marching_cubes(np.zeros((3, 3, 3)))
    with pytest.raises(ValueError, match="go together"):
        M.marching_cubes_numpy(np.zeros((3, 3, 3)), 0.0, lo=(0, 0, 0))
    with pytest.raises(ValueError, match="go together"):
        M.marching_cubes_numpy(np.zeros((3, 3, 3)), 0.0, center=(0, 0, 0))
    with pytest.raises(ValueError, match="NaN"):
        M.marching_cubes_numpy(np.zeros((3, 3, 3)), float("nan"))
    with pytest.raises(ValueError, match="nx,ny,nz"):
        M.marching_cubes_numpy(np.zeros((3, 3)))

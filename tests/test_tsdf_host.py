"""CPU: the float64 checker of the TSDF fusion against a hand-written expectation and against an independent statement of the same
semantics on every case of tests/tsdf_cases.py; what the cases assume (the exclusion cap, float32 and float64 deciding alike, what the
planted samples are there for); the bar rejects the wrong implementations one can think of; the C-ABI of the op is declared, exported and
refuses bad arguments before it touches a GPU."""
import ctypes
import os
import re

import pytest
import torch

from streetunveiler_amd import tsdf as T
from tests import tsdf_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(tc.CASES)


def test_checker_against_a_hand_written_expectation():
    """Two views with pix = (x, y): zc = 1 in the first, zc = 2 (and pix halved) in the second; 2 x 2 maps, so pix = 0 is the mean of
    the four pixels.  trunc = 0.5."""
    f = torch.float64
    F0 = torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]], dtype=f)
    F1 = F0.clone(); F1[3, 3] = 2.0
    depth = torch.tensor([[[[1.0, 1.5], [1.5, 2.0]]], [[[1.0, 1.0], [1.0, 1.0]]]], dtype=f)      # means 1.5 and 1
    rgb = torch.stack([torch.full((3, 2, 2), 0.25, dtype=f), torch.full((3, 2, 2), 1.0, dtype=f)])
    samples = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [-0.5, 0.5, 7.0]], dtype=f)
    tsdf, colour, weight, margin = T.unbounded_tsdf_torch(samples, depth, rgb, torch.stack([F0, F1]), 0.1, return_rgb=True, return_weight=True,
                                                          return_margin=True)
    # sample 0: view 0 sdf = 0.5 -> s = 1: (1 + 1) / 2 = 1, rgb 0.125; view 1 sdf = 1 - 2 = -1 < -0.5: skipped
    # sample 1: pix.x = 1 is outside view 0 (strict); view 1 has pix.x = 0.5, sdf = -1: skipped
    # sample 2: view 0 at (-0.5, 0.5): depth = 0.25 * 1 + 0.25 * 1.5 * 0 ... = 0.75 * (0.25 * 1 + 0.75 * 1.5) + 0.25 * (0.25 * 1.5 + 0.75 * 2)
    d2 = 0.25 * (0.75 * 1.0 + 0.25 * 1.5) + 0.75 * (0.75 * 1.5 + 0.25 * 2.0)
    assert weight.tolist() == [2.0, 1.0, 2.0] and tsdf[1] == 1 and not colour[1].any()
    assert tsdf[0] == 1.0 and torch.equal(colour[0], torch.full((3,), 0.125, dtype=f))
    assert abs(float(tsdf[2]) - (1 + min((d2 - 1) / 0.5, 1.0)) / 2) < 1e-15
    assert margin[1] == 0 and abs(float(margin[0]) - 1.0) < 1e-15      # |1 - |pix.x|| = 0 in view 0; |sdf + trunc| / trunc = 1 in view 1
    only = T.unbounded_tsdf_torch(samples, depth, rgb, torch.stack([F0, F1]), 0.1)
    assert torch.equal(only, tsdf)


def test_adaptive_truncation_reads_the_norm_of_the_world_point():
    """center far from the origin, radius 1: every world point has a norm above 1.9, so trunc = 5 v / (2 - 1.9) for a sample whose
    normalised point is well inside the unit ball (the module docstring of streetunveiler_amd.tsdf)."""
    f = torch.float64
    F = torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]], dtype=f)[None]
    depth, rgb = torch.full((1, 1, 2, 2), 0.9, dtype=f), torch.zeros((1, 3, 2, 2), dtype=f)
    sample = torch.tensor([[0.1, 0.1, 0.0]], dtype=f)      # world point (0.1, 0.1, 5); pix = (0.1, 0.1), sdf = -0.1
    assert T.unbounded_tsdf_torch(sample, depth, rgb, F, 0.01, return_weight=True)[1][0] == 1      # plain: trunc 0.05, skipped
    tsdf, weight = T.unbounded_tsdf_torch(sample, depth, rgb, F, 0.01, center=(0.0, 0.0, 5.0), radius=1.0, return_weight=True)
    assert weight[0] == 2 and abs(float(tsdf[0]) - (1 - 0.1 / 0.5) / 2) < 1e-12      # trunc 0.5: s = -0.2


@pytest.mark.parametrize("name", ALL)
def test_checker_equals_the_second_statement_and_the_case_keeps_its_conditions(name):
    c, want = tc.case(name), tc.expected(name)
    n = c.samples.shape[0]
    excluded = int((~want.admitted).sum())
    print(f"{name}: {excluded} of {n} excluded; dev32 {want.dev32}")
    assert excluded <= tc.MAX_EXCLUDED * n and (excluded == 0 or not c.none_excluded) and bool(want.admitted[c.exact].all())
    # the float32 restatement takes no decision different from float64 on any admitted sample, planted ones included
    assert torch.equal(want.weight32[want.admitted], want.weight[want.admitted])
    tsdf, rgb, weight = tc.restate(c)
    assert torch.equal(weight, want.weight)
    for k, got in zip(tc.OUTPUTS, (tsdf, rgb[:, 0], rgb[:, 1], rgb[:, 2])):
        assert torch.allclose(got, want.want[k], rtol=0, atol=1e-12, equal_nan=True), k
    if n:
        tc.compare(*tc.restate(c, fused=True), want, f"{name}, the second statement with fused multiply-adds")
        # the sequential mean does not depend on the order of the views beyond rounding: nothing a bar could reject
        tc.compare(*tc.restate(c, torch.float32, reverse_loop=True), want, f"{name}, views walked last to first")


def test_what_the_named_cases_are_there_for():
    ring, plain = tc.expected("ring"), tc.expected("ring_plain")
    for e in (ring, plain):
        counts = torch.bincount((e.weight - 1).long())
        assert len(counts) >= 4 and counts[0] > 1000 and counts[1:].sum() > 5000      # unseen samples, and samples several views integrate
    assert tc.case("ring").center is not None and any(tc.CENTER) and tc.case("ring_plain").center is None
    assert [tc.case(f"tails_{n}").samples.shape[0] for n in tc.TAILS] == list(tc.TAILS) and tc.case("tails_65").full_proj.shape[0] == 1
    c, e = tc.case("nonfinite"), tc.expected("nonfinite")
    assert int(c.depth.isnan().sum()) == 1 and int(c.depth.isinf().sum()) == 1 and c.n_planted == 5
    q = torch.cat([c.samples[:2].double(), torch.ones(2, 1, dtype=torch.float64)], dim=1) @ c.full_proj.double()
    assert q[0, 0, 3] == 0 and bool((q[:, 1, 3] < 0).all())      # zc == 0 at the camera centre; behind every camera
    assert e.weight[:3].tolist() == [e.weight[0], 1.0, 1.0] and e.want["tsdf"][2] == 1 and all(e.want[k][2] == 0 for k in "rgb")
    _, _, w_without = T.unbounded_tsdf_torch(c.samples.double(), c.depth.double().nan_to_num(nan=3.0, posinf=3.0), c.rgb.double(), c.full_proj.double(),
                                             c.voxel_size, return_rgb=True, return_weight=True)
    assert w_without[3] == e.weight[3] + 1 and w_without[4] == e.weight[4] - 1      # the NaN pixel keeps view 0 out; +inf lets it in (s = 1)
    c, e = tc.case("exact_edge"), tc.expected("exact_edge")
    edge = float(c.samples.abs().max())
    assert edge < 1 and float(torch.tensor(edge) + 1) == 2.0 and bool(e.admitted.all())      # float32: ix == W - 1 exactly, the east tap has index W
    last = (c.samples[:, 0] == edge) & (c.samples[:, 1] == edge)
    assert bool((e.weight[last] == 2).all()) and bool((e.want["tsdf"][last] == 1).all())      # the last pixel of the last view: sdf >= 0
    tie = (c.samples[:, 0] == 0) & (c.samples[:, 1] == 0)
    assert int(tie.sum()) == 2 and bool((e.weight[tie] == 1).all()) and e.dev32["tsdf"] == 0.0
    g = tc.case("grid")
    assert g.samples.shape[0] == 5 * 7 * 9 and torch.equal(g.samples[1], T.grid_coordinates(tc.GRID_LO, tc.GRID_HI, tc.GRID_DIMS)[0, 0, 1])
    assert tc.GRID_DIMS[0] > tc.GRID_SLAB > 0 and tc.GRID_DIMS[0] % tc.GRID_SLAB      # two slabs, the second shorter


@pytest.mark.parametrize("mutant", sorted(tc.MUTANTS))
def test_the_bar_rejects_wrong_implementations(mutant):
    name = tc.MUTANTS[mutant]
    with pytest.raises(AssertionError):
        tc.compare(*tc.restate(tc.case(name), mutant=mutant), tc.expected(name), f"{mutant} on {name}")


def test_grid_coordinates_are_the_fused_ones():
    g = T.grid_coordinates((-1.0, 0.0, 0.25), (1.0, 0.0, 0.75), (5, 1, 3))
    assert g.shape == (5, 1, 3, 3) and g.dtype == torch.float32
    assert g[:, 0, 0, 0].tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0] and g[0, 0, :, 2].tolist() == [0.25, 0.5, 0.75] and not g[..., 1].any()


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
    for name in ("sr_tsdf_fuse", "sr_tsdf_fuse_grid"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.sr_abi_version() == 10      # an addition: nothing that existed changed
    for name in ("TsdfViews", "unbounded_tsdf", "unbounded_tsdf_grid", "unbounded_tsdf_torch", "sdf_function"):
        assert name in streetunveiler_amd.__all__ and callable(getattr(streetunveiler_amd, name))
    assert "tsdf.hip" in [s for s, _ in SOURCES]
    assert ctypes.sizeof(_lib.SrTsdfViews) == 32 and ctypes.sizeof(_lib.SrTsdfSpace) == 32


def test_argument_refusals_without_gpu(lib):
    """Every refusal comes before the first HIP call, or this test could not run here."""
    from streetunveiler_amd import _lib
    dummy = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(dummy) + 15) & ~15
    INVALID, UNSUPPORTED = -1, -4
    views = lambda maps=p, proj=p, V=6, H=37, W=53, ch=1: ctypes.byref(_lib.SrTsdfViews(maps, proj, V, H, W, ch))
    space = lambda v=0.02: ctypes.byref(_lib.SrTsdfSpace(v, 0, (ctypes.c_float * 3)(), 1.0))
    table = [((views(maps=None), space(), 5, p, p, None, None, None), INVALID, b"maps is NULL"),
             ((views(proj=None), space(), 5, p, p, None, None, None), INVALID, b"full_proj is NULL"),
             ((views(V=0), space(), 5, p, p, None, None, None), INVALID, b"at least one view"),
             ((views(H=1), space(), 5, p, p, None, None, None), INVALID, b"at least 2"),
             ((views(W=1), space(), 5, p, p, None, None, None), INVALID, b"at least 2"),
             ((views(ch=3), space(), 5, p, p, None, None, None), INVALID, b"channels"),
             ((views(maps=p + 4, ch=4), space(), 5, p, p, None, None, None), INVALID, b"aligned"),
             ((views(), space(0.0), 5, p, p, None, None, None), INVALID, b"voxel_size"),
             ((views(), space(-1.0), 5, p, p, None, None, None), INVALID, b"voxel_size"),
             ((views(), space(float("nan")), 5, p, p, None, None, None), INVALID, b"voxel_size"),
             ((views(), space(), 5, p, p, p, None, None), INVALID, b"depths only"),
             ((views(), space(), -1, p, p, None, None, None), INVALID, b"n < 0"),
             ((views(), space(), 5, None, p, None, None, None), INVALID, b"samples is NULL"),
             ((views(), space(), 5, p, None, None, None, None), INVALID, b"tsdf is NULL"),
             ((None, space(), 5, p, p, None, None, None), INVALID, b"views / space")]
    for args, code, fragment in table:
        rc = lib.sr_tsdf_fuse(*args)
        assert rc == code and fragment in lib.sr_last_error(), (rc, fragment, lib.sr_last_error())
    assert lib.sr_tsdf_fuse(views(), space(), 0, None, None, None, None, None) == 0      # no samples: no error, no work
    dims, lo, step = (ctypes.c_int32 * 3)(5, 7, 9), (ctypes.c_float * 3)(), (ctypes.c_float * 3)()
    grid = [((views(), space(), None, lo, step, 0, 5, p, None, None, None), INVALID, b"dims / lo / step"),
            ((views(), space(), (ctypes.c_int32 * 3)(5, 0, 9), lo, step, 0, 5, p, None, None, None), INVALID, b"at least one sample"),
            ((views(), space(), dims, lo, step, 3, 2, p, None, None, None), INVALID, b"slab"),
            ((views(), space(), dims, lo, step, 0, 6, p, None, None, None), INVALID, b"slab"),
            ((views(), space(), dims, lo, step, -1, 2, p, None, None, None), INVALID, b"slab"),
            ((views(), space(), (ctypes.c_int32 * 3)(2048, 2048, 2048), lo, step, 0, 2048, p, None, None, None), UNSUPPORTED, b"2^31"),
            ((views(), space(), (ctypes.c_int32 * 3)(4, 65536, 65536), lo, step, 0, 1, p, None, None, None), UNSUPPORTED, b"2^31"),
            ((views(W=1), space(), dims, lo, step, 0, 5, p, None, None, None), INVALID, b"at least 2"),
            ((views(), space(), dims, lo, step, 0, 5, None, None, None, None), INVALID, b"tsdf is NULL")]
    for args, code, fragment in grid:
        rc = lib.sr_tsdf_fuse_grid(*args)
        assert rc == code and fragment in lib.sr_last_error(), (rc, fragment, lib.sr_last_error())
    assert lib.sr_tsdf_fuse_grid(views(), space(), dims, lo, step, 2, 2, None, None, None, None) == 0      # an empty slab


def test_cpu_tensors_and_wrong_shapes_are_refused():
    from streetunveiler_amd._lib import SurfelRasterError
    c = tc.case("tails_65")
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        T.TsdfViews(c.depth, c.rgb, c.full_proj)
    views = T.TsdfViews.__new__(T.TsdfViews)
    views.device, views.packed = torch.device("cpu"), None
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        T.unbounded_tsdf(c.samples, views, 0.02)
    with pytest.raises(ValueError, match="go together"):
        T._space(0.02, (0.0, 0.0, 0.0), None)
    with pytest.raises(ValueError, match="voxel_size"):
        T._space(0.0, None, None)
    with pytest.raises(ValueError, match="dims"):
        T.grid_coordinates((0, 0, 0), (1, 1, 1), (3, 0, 3))

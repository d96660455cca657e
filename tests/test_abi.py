"""CPU: the C-ABI shared library loads and exports every symbol include/surfel_raster.h declares."""
import ctypes
import os
import sys
import re

import pytest

from streetunveiler_amd import _lib
from streetunveiler_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "surfel_raster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sr_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_are_exported(lib):
    declared = _declared_functions()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/surfel_raster.h but not exported"
    assert sorted(_lib.EXPORTS) == declared


def test_abi_version_and_sizes(lib):
    assert lib.sr_abi_version() == 10
    # pure host arithmetic (no GPU): image state = 3 float planes + 2 u32 planes, 256-B aligned
    assert lib.sr_image_bytes(1920, 1080) >= 1920 * 1080 * 20
    assert lib.sr_backward_workspace_bytes(1000, 5000, 3) >= 5000 * 97
    assert lib.sr_backward_workspace_bytes(1000, 5000, 6) >= 5000 * 97
    assert lib.sr_geom_bytes(1000) >= 1000 * (80 + 4 * 7 + 1)
    # the geometry scratch also holds pass X's [tile columns][blocks] histogram: one Gaussian in a frame 1024 tiles wide must fit
    assert lib.sr_geom_bytes(1) >= 1024 * 4


def test_struct_layouts_match_header():
    # field counts / order mirror the header; sizes follow the C layout rules (8-B pointers)
    assert ctypes.sizeof(_lib.SrFrame) == 8 * 4 + 4 * 8 + 2 * 4 + 4 + 4 + 8    # ... tile shape, flags (+ padding), blend_counters
    assert ctypes.sizeof(_lib.SrGaussians) == 4 * 4 + 8 * 8
    assert ctypes.sizeof(_lib.SrGradients) == 8 * 8
    assert [f[0] for f in _lib.SrFrame._fields_][:3] == ["image_height", "image_width", "tanfovx"]


def test_argument_errors_without_gpu(lib):
    fr = _lib.SrFrame(0, 0, 1.0, 1.0, 1.0, 0, 0, 0, None, None, None, None, 0, 0, 0, None)
    g = _lib.SrGaussians(0, 0, 0, 0, None, None, None, None, None, None, None, None)
    d = ctypes.c_uint32(7)
    rc = lib.sr_forward_plan(ctypes.byref(fr), ctypes.byref(g), None, 0, None, ctypes.byref(d), None)
    assert rc == -1 and b"image size" in lib.sr_last_error()


# ---- layout identity -------------------------------------------------------------------------------------------------------------------
# Recorded from the library of commit 6eaaa90 (before the layouts moved behind typed views), not computed here: the sizes the six *_bytes
# functions report and the offsets the three *_view functions report into one host buffer.  A buffer sized by one build of the library and
# carved by another, or a saved training state, depends on none of them moving.
GEOM_BYTES = {
    0: 9984, 1: 9984, 2047: 344576, 2048: 344576, 2049: 348928, 100000: 16557312}
BINNING_BYTES = {   # (D, W, H); P does not enter
    (0, 1, 1): 6144, (0, 203, 125): 12288, (0, 1920, 1080): 524800,
    (1, 1, 1): 6144, (1, 203, 125): 12288, (1, 1920, 1080): 524800,
    (5000, 1, 1): 76032, (5000, 203, 125): 82176, (5000, 1920, 1080): 595712}
IMAGE_BYTES = {
    (1, 1): 512, (203, 125): 507648, (1920, 1080): 41472000}
CLASS_IMAGE_BYTES = {   # (W, H, n_classes)
    (1, 1, 1): 1024, (1, 1, 6): 1024, (203, 125, 1): 411392,
    (203, 125, 6): 2466048, (1920, 1080, 1): 33566720, (1920, 1080, 6): 201398528}
CLASS_SHARED_BYTES = {   # (P, W, H, n_classes, D)
    (0, 1, 1, 1, 0): 1536, (0, 1, 1, 1, 1): 1536, (0, 1, 1, 1, 5000): 11520,
    (0, 1, 1, 6, 0): 1536, (0, 1, 1, 6, 1): 1536, (0, 1, 1, 6, 5000): 11520,
    (0, 203, 125, 1, 0): 411904, (0, 203, 125, 1, 1): 411904, (0, 203, 125, 1, 5000): 421888,
    (0, 203, 125, 6, 0): 2466560, (0, 203, 125, 6, 1): 2466560, (0, 203, 125, 6, 5000): 2476544,
    (0, 1920, 1080, 1, 0): 33567232, (0, 1920, 1080, 1, 1): 33567232, (0, 1920, 1080, 1, 5000): 33577216,
    (0, 1920, 1080, 6, 0): 201399040, (0, 1920, 1080, 6, 1): 201399040, (0, 1920, 1080, 6, 5000): 201409024,
    (1, 1, 1, 1, 0): 1536, (1, 1, 1, 1, 1): 1536, (1, 1, 1, 1, 5000): 11520,
    (1, 1, 1, 6, 0): 1536, (1, 1, 1, 6, 1): 1536, (1, 1, 1, 6, 5000): 11520,
    (1, 203, 125, 1, 0): 411904, (1, 203, 125, 1, 1): 411904, (1, 203, 125, 1, 5000): 421888,
    (1, 203, 125, 6, 0): 2466560, (1, 203, 125, 6, 1): 2466560, (1, 203, 125, 6, 5000): 2476544,
    (1, 1920, 1080, 1, 0): 33567232, (1, 1920, 1080, 1, 1): 33567232, (1, 1920, 1080, 1, 5000): 33577216,
    (1, 1920, 1080, 6, 0): 201399040, (1, 1920, 1080, 6, 1): 201399040, (1, 1920, 1080, 6, 5000): 201409024,
    (2047, 1, 1, 1, 0): 3328, (2047, 1, 1, 1, 1): 3328, (2047, 1, 1, 1, 5000): 13312,
    (2047, 1, 1, 6, 0): 3328, (2047, 1, 1, 6, 1): 3328, (2047, 1, 1, 6, 5000): 13312,
    (2047, 203, 125, 1, 0): 413696, (2047, 203, 125, 1, 1): 413696, (2047, 203, 125, 1, 5000): 423680,
    (2047, 203, 125, 6, 0): 2468352, (2047, 203, 125, 6, 1): 2468352, (2047, 203, 125, 6, 5000): 2478336,
    (2047, 1920, 1080, 1, 0): 33569024, (2047, 1920, 1080, 1, 1): 33569024, (2047, 1920, 1080, 1, 5000): 33579008,
    (2047, 1920, 1080, 6, 0): 201400832, (2047, 1920, 1080, 6, 1): 201400832, (2047, 1920, 1080, 6, 5000): 201410816,
    (2048, 1, 1, 1, 0): 3328, (2048, 1, 1, 1, 1): 3328, (2048, 1, 1, 1, 5000): 13312,
    (2048, 1, 1, 6, 0): 3328, (2048, 1, 1, 6, 1): 3328, (2048, 1, 1, 6, 5000): 13312,
    (2048, 203, 125, 1, 0): 413696, (2048, 203, 125, 1, 1): 413696, (2048, 203, 125, 1, 5000): 423680,
    (2048, 203, 125, 6, 0): 2468352, (2048, 203, 125, 6, 1): 2468352, (2048, 203, 125, 6, 5000): 2478336,
    (2048, 1920, 1080, 1, 0): 33569024, (2048, 1920, 1080, 1, 1): 33569024, (2048, 1920, 1080, 1, 5000): 33579008,
    (2048, 1920, 1080, 6, 0): 201400832, (2048, 1920, 1080, 6, 1): 201400832, (2048, 1920, 1080, 6, 5000): 201410816,
    (2049, 1, 1, 1, 0): 3584, (2049, 1, 1, 1, 1): 3584, (2049, 1, 1, 1, 5000): 13568,
    (2049, 1, 1, 6, 0): 3584, (2049, 1, 1, 6, 1): 3584, (2049, 1, 1, 6, 5000): 13568,
    (2049, 203, 125, 1, 0): 413952, (2049, 203, 125, 1, 1): 413952, (2049, 203, 125, 1, 5000): 423936,
    (2049, 203, 125, 6, 0): 2468608, (2049, 203, 125, 6, 1): 2468608, (2049, 203, 125, 6, 5000): 2478592,
    (2049, 1920, 1080, 1, 0): 33569280, (2049, 1920, 1080, 1, 1): 33569280, (2049, 1920, 1080, 1, 5000): 33579264,
    (2049, 1920, 1080, 6, 0): 201401088, (2049, 1920, 1080, 6, 1): 201401088, (2049, 1920, 1080, 6, 5000): 201411072,
    (100000, 1, 1, 1, 0): 101376, (100000, 1, 1, 1, 1): 101376, (100000, 1, 1, 1, 5000): 111360,
    (100000, 1, 1, 6, 0): 101376, (100000, 1, 1, 6, 1): 101376, (100000, 1, 1, 6, 5000): 111360,
    (100000, 203, 125, 1, 0): 511744, (100000, 203, 125, 1, 1): 511744, (100000, 203, 125, 1, 5000): 521728,
    (100000, 203, 125, 6, 0): 2566400, (100000, 203, 125, 6, 1): 2566400, (100000, 203, 125, 6, 5000): 2576384,
    (100000, 1920, 1080, 1, 0): 33667072, (100000, 1920, 1080, 1, 1): 33667072, (100000, 1920, 1080, 1, 5000): 33677056,
    (100000, 1920, 1080, 6, 0): 201498880, (100000, 1920, 1080, 6, 1): 201498880, (100000, 1920, 1080, 6, 5000): 201508864}
WORKSPACE_BYTES = {   # (D, colour channels); P does not enter
    (0, 3): 512, (0, 6): 512, (0, 9): 512,
    (1, 3): 512, (1, 6): 512, (1, 9): 512,
    (5000, 3): 485120, (5000, 6): 485120, (5000, 9): 565248}
GEOM_VIEW = {   # P: offsets of (splats, depth_keys, tiles_touched, clamped, sorted_gid, frame_counts)
    0: (0, 256, 512, 1024, 1536, 2564), 1: (0, 256, 512, 1024, 1536, 2564),
    2047: (0, 163840, 172032, 196608, 206848, 313348), 2048: (0, 163840, 172032, 196608, 206848, 313348),
    2049: (0, 164096, 172544, 197632, 208384, 315912), 100000: (0, 8000000, 8400128, 9600256, 10100480, 15301060)}
BINNING_VIEW = {   # (D, W, H): offsets of (point_list, ranges, tile_order)
    (0, 1, 1): (256, 768, 1024), (0, 203, 125): (256, 768, 4096), (0, 1920, 1080): (256, 768, 260096),
    (1, 1, 1): (256, 768, 1024), (1, 203, 125): (256, 768, 4096), (1, 1920, 1080): (256, 768, 260096),
    (5000, 1, 1): (40192, 70656, 70912), (5000, 203, 125): (40192, 70656, 73984), (5000, 1920, 1080): (40192, 70656, 329984)}
IMAGE_VIEW = {   # (W, H): offsets of (final_T, n_contrib)
    (1, 1): (0, 256), (203, 125): (0, 304640), (1920, 1080): (0, 24883200)}
LAYOUT_P = [0, 1, 2047, 2048, 2049, 100000]
LAYOUT_D = [0, 1, 5000]
LAYOUT_WH = [(1, 1), (203, 125), (1920, 1080)]
LAYOUT_CLASSES = [1, 6]
LAYOUT_CHANNELS = [3, 6, 9]


def test_state_buffer_sizes_are_the_recorded_ones(lib):
    assert sorted(GEOM_BYTES) == LAYOUT_P and len(CLASS_SHARED_BYTES) == 6 * 3 * 2 * 3
    for P in LAYOUT_P:
        assert lib.sr_geom_bytes(P) == GEOM_BYTES[P], P
        for D in LAYOUT_D:
            for W, H in LAYOUT_WH:
                assert lib.sr_binning_bytes(P, D, W, H) == BINNING_BYTES[(D, W, H)], (P, D, W, H)
                for n in LAYOUT_CLASSES:
                    assert lib.sr_class_shared_bytes(P, W, H, n, D) == CLASS_SHARED_BYTES[(P, W, H, n, D)], (P, W, H, n, D)
            for NC in LAYOUT_CHANNELS:
                assert lib.sr_backward_workspace_bytes(P, D, NC) == WORKSPACE_BYTES[(D, NC)], (P, D, NC)
    for W, H in LAYOUT_WH:
        assert lib.sr_image_bytes(W, H) == IMAGE_BYTES[(W, H)], (W, H)
        for n in LAYOUT_CLASSES:
            assert lib.sr_class_image_bytes(W, H, n) == CLASS_IMAGE_BYTES[(W, H, n)], (W, H, n)


def test_workspace_sizes_are_the_recorded_ones(lib):
    """Every *_bytes function over the table tools/record_workspace_sizes.py recorded from the library of commit 88b8564, before all
    layouts were carved by one Carver: byte for byte the same."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")) as f:
        recorded = json.load(f)
    assert recorded["recorded_from_source_digest"] != lib.sr_source_digest().decode()      # not recorded from the library under test
    assert {0, 1} <= set(recorded["counts"])
    for b in (256, 2048, 65536, 262144, 524288):
        assert {b - 1, b, b + 1} <= set(recorded["counts"]), b
    assert sorted(recorded["sizes"]) == sorted(
        ["sr_geom_bytes", "sr_binning_bytes", "sr_image_bytes", "sr_backward_workspace_bytes", "sr_class_image_bytes", "sr_class_shared_bytes",
         "sr_knn_workspace_bytes", "sr_cluster_workspace_bytes", "sr_densify_workspace_bytes", "sr_debug_radix_sort_temp_bytes"])
    for name, arg in (("sr_geom_bytes", 0), ("sr_knn_workspace_bytes", 1), ("sr_cluster_workspace_bytes", 0),
                      ("sr_densify_workspace_bytes", 0), ("sr_debug_radix_sort_temp_bytes", 0), ("sr_backward_workspace_bytes", 1),
                      ("sr_binning_bytes", 1)):
        assert {row[arg] for row in recorded["sizes"][name]} == set(recorded["counts"]), name
    assert {row[0] for row in recorded["sizes"]["sr_knn_workspace_bytes"]} == set(recorded["counts"])   # nq, 0 = the self search
    assert {row[1] for row in recorded["sizes"]["sr_knn_workspace_bytes"] if row[0] == 0} == set(recorded["counts"])
    for name, rows in recorded["sizes"].items():
        for *args, size in rows:
            assert getattr(lib, name)(*args) == size, (name, args)


def _view_offsets(view, base):
    return tuple(getattr(view, name) - base for name, _ in view._fields_)


def test_state_buffer_views_point_where_they_did(lib):
    for P in LAYOUT_P:
        n = lib.sr_geom_bytes(P)
        buf, view = ctypes.create_string_buffer(n), _lib.SrGeomView()
        assert lib.sr_geom_view(ctypes.addressof(buf), n, P, ctypes.byref(view)) == 0
        assert _view_offsets(view, ctypes.addressof(buf)) == GEOM_VIEW[P], P
        assert lib.sr_geom_view(ctypes.addressof(buf), n - 1, P, ctypes.byref(view)) == -3   # SR_ERR_BUFFER_TOO_SMALL
    for D in LAYOUT_D:
        for W, H in LAYOUT_WH:
            n = lib.sr_binning_bytes(2048, D, W, H)
            buf, view = ctypes.create_string_buffer(n), _lib.SrBinningView()
            assert lib.sr_binning_view(ctypes.addressof(buf), n, 2048, D, W, H, ctypes.byref(view)) == 0
            assert _view_offsets(view, ctypes.addressof(buf)) == BINNING_VIEW[(D, W, H)], (D, W, H)
    for W, H in LAYOUT_WH:
        n = lib.sr_image_bytes(W, H)
        buf, view = ctypes.create_string_buffer(n), _lib.SrImageView()
        assert lib.sr_image_view(ctypes.addressof(buf), n, W, H, ctypes.byref(view)) == 0
        assert _view_offsets(view, ctypes.addressof(buf)) == IMAGE_VIEW[(W, H)], (W, H)


# ---- refusal table ---------------------------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -4   # SR_ERR_INVALID_ARGUMENT, SR_ERR_UNSUPPORTED
ONE_WAVE, COOP, ROWS = _lib.SR_FLAG_ONE_WAVE_BACKWARD, _lib.SR_FLAG_COOP_BACKWARD, _lib.SR_FLAG_ROW_BACKWARD
# (flags, tile, colour channels, blend_counters set) -> (code, fragment of sr_last_error()); tile None = the default 16x16
PAIR_CONFLICTS = [((a, None, 3, False), (INVALID, "exclude each other")) for a in (ONE_WAVE | COOP, ONE_WAVE | ROWS, COOP | ROWS, ONE_WAVE | COOP | ROWS)]
ROW_PAIR_SHAPE = [((ROWS, (8, 8), 3, False), (UNSUPPORTED, "SR_FLAG_ROW_BACKWARD")),
                  ((ROWS, None, 6, False), (UNSUPPORTED, "SR_FLAG_ROW_BACKWARD")),
                  ((ROWS | _lib.SR_FLAG_NO_QUADRANT_CULL, None, 3, False), (UNSUPPORTED, "SR_FLAG_ROW_BACKWARD"))]
FORWARD_ONLY_REFUSALS = [((ROWS | _lib.SR_FLAG_QUADRANT_MAPPED_FORWARD, None, 3, False), (UNSUPPORTED, "SR_FLAG_ROW_BACKWARD")),
                         ((ROWS | _lib.SR_FLAG_FORWARD_ONLY, None, 3, False), (UNSUPPORTED, "SR_FLAG_ROW_BACKWARD")),
                         ((_lib.SR_FLAG_ROW_MAPPED_FORWARD | _lib.SR_FLAG_QUADRANT_MAPPED_FORWARD, None, 3, False), (INVALID, "exclude each other")),
                         ((_lib.SR_FLAG_ROW_MAPPED_FORWARD, (32, 16), 3, False), (UNSUPPORTED, "ROW_MAPPED")),
                         ((0, (16, 8), 3, True), (UNSUPPORTED, "blend_counters")),
                         ((_lib.SR_FLAG_FORWARD_ONLY, None, 3, True), (UNSUPPORTED, "blend_counters"))]


def test_refused_flag_combinations_without_gpu(lib):
    """Every combination of blend-pair flags, mapping flags, tile shape, channel count and counters that the library refuses, and the class
    passes' n_classes / SR_FLAG_BINNING_CAPACITY refusals: the code and the message fragment of commit 6eaaa90.  Only refused calls are made, on
    dummy host pointers -- a refusal comes before the first HIP call of its entry point, or this test could not run without a GPU."""
    dummy = ctypes.create_string_buffer(64)
    p, big, D = ctypes.addressof(dummy), 1 << 40, 10

    def frame(flags, tile=None, counters=False):
        tw, th = tile or (0, 0)
        return _lib.SrFrame(64, 96, 1.0, 1.0, 1.0, 0, 0, 0, p, p, p, p, tw, th, flags, p if counters else None)

    def gaussians(channels=3):   # precomputed colours: every channel count, and what the stand-alone class pass takes
        return _lib.SrGaussians(100, 0, channels, 0, p, p, p, p, None, p, None, None)

    grads = _lib.SrGradients(p, p, p, p, p, p, p, p)

    def check(rc, want, what):
        code, fragment = want
        assert rc == code and fragment.encode() in lib.sr_last_error(), (what, rc, lib.sr_last_error())

    for (flags, tile, channels, counters), want in PAIR_CONFLICTS + ROW_PAIR_SHAPE + FORWARD_ONLY_REFUSALS:
        fr, g = frame(flags, tile, counters), gaussians(channels)
        check(lib.sr_forward_render(ctypes.byref(fr), ctypes.byref(g), p, big, p, big, p, big, D, p, p, None), want, ("forward", flags, tile, channels, counters))
    for (flags, tile, channels, counters), want in PAIR_CONFLICTS + ROW_PAIR_SHAPE:   # (a backward call does not read the forward-only flags)
        fr, g = frame(flags, tile, counters), gaussians(channels)
        check(lib.sr_backward_blend(ctypes.byref(fr), ctypes.byref(g), p, big, p, big, p, big, D, p, p, p, big, None), want, ("backward_blend", flags, tile, channels))
        check(lib.sr_backward_geometry(ctypes.byref(fr), ctypes.byref(g), p, p, big, p, big, p, big, D, p, big, ctypes.byref(grads), None), want,
              ("backward_geometry", flags, tile, channels))

    def class_calls(fr, g, n):
        return [("class_forward_render", lib.sr_class_forward_render, (ctypes.byref(fr), ctypes.byref(g), n, p, big, p, big, p, big, D, p, None)),
                ("class_backward", lib.sr_class_backward, (ctypes.byref(fr), ctypes.byref(g), n, p, p, big, p, big, p, big, D, p, p, big, ctypes.byref(grads), None)),
                ("class_forward_shared", lib.sr_class_forward_shared, (ctypes.byref(fr), ctypes.byref(g), n, p, p, big, p, big, p, big, D, p, None)),
                ("class_backward_shared", lib.sr_class_backward_shared, (ctypes.byref(fr), ctypes.byref(g), n, p, big, p, big, p, big, D, p, p, big, None))]

    fr, g = frame(0), gaussians(3)
    for n in (0, 7):
        for name, fn, args in class_calls(fr, g, n):
            check(fn(*args), (UNSUPPORTED, "n_classes"), (name, n))
    fr = frame(_lib.SR_FLAG_BINNING_CAPACITY)
    for name, fn, args in class_calls(fr, g, 3):
        check(fn(*args), (UNSUPPORTED, "SR_FLAG_BINNING_CAPACITY"), (name, "capacity"))


# ---- workspace refusals ----------------------------------------------------------------------------------------------------------------
TOO_SMALL = -3   # SR_ERR_BUFFER_TOO_SMALL


def _workspace_calls(lib, p):
    """Every entry point that takes (workspace, workspace_bytes) as name -> (the bytes its *_bytes function reports, call(workspace, bytes)),
    with the smallest arguments it accepts otherwise: `p` is a 16-B aligned address inside a host buffer (nothing is launched, so nothing
    dereferences it on a device; the few host arrays -- dims, counts, lo, step, the segment -- are real)."""
    n = 10
    dims = (ctypes.c_int32 * 3)(3, 3, 3)
    f3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    d3 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    plan_counts = (ctypes.c_uint32 * 4)()
    apply_counts = (ctypes.c_uint32 * 4)(1, 0, 0, 0)
    segment = (_lib.SrDensifySegment * 1)(_lib.SrDensifySegment(p, p, 1, _lib.SR_DENSIFY_ROLE_COPY))
    aux = lib.sr_aux_loss_workspace_bytes(n)
    post = lib.sr_mesh_post_workspace_bytes(n, n)
    voxel = lib.sr_voxel_workspace_bytes(n)
    lidar = lib.sr_lidar_label_workspace_bytes(n, 1)
    return {
        "sr_knn_mean_dist2": (lib.sr_knn_workspace_bytes(0, n), lambda w, b: lib.sr_knn_mean_dist2(0, None, n, p, 3, 0, p, w, b, None)),
        "sr_cluster_radius": (lib.sr_cluster_workspace_bytes(n), lambda w, b: lib.sr_cluster_radius(n, p, None, 1.0, p, w, b, None)),
        "sr_image_loss_forward": (lib.sr_image_loss_workspace_bytes(16, 8, 3),
                                  lambda w, b: lib.sr_image_loss_forward(16, 8, 3, 0.2, p, p, None, None, w, b, p, None)),
        "sr_image_loss_backward": (lib.sr_image_loss_workspace_bytes(16, 8, 3),
                                   lambda w, b: lib.sr_image_loss_backward(16, 8, 3, 0.2, p, p, None, None, w, b, p, p, None, None, None)),
        "sr_semantic_ce_forward": (aux, lambda w, b: lib.sr_semantic_ce_forward(n, 1, 3, p, p, 1, None, w, b, p, None)),
        "sr_surface_reg_forward": (aux, lambda w, b: lib.sr_surface_reg_forward(n, 1, p, p, p, 0.05, 100.0, w, b, p, None)),
        "sr_opacity_shrink_forward": (aux, lambda w, b: lib.sr_opacity_shrink_forward(n, p, 0, w, b, p, None)),
        "sr_sky_backward": (lib.sr_sky_workspace_bytes(0),
                            lambda w, b: lib.sr_sky_backward(n, 1, *[p] * 10, 0, w, b, *[p] * 8, None)),
        "sr_densify_plan": (lib.sr_densify_workspace_bytes(n),
                            lambda w, b: lib.sr_densify_plan(n, p, p, p, p, 0.0002, 0.005, 0.01, -1.0, None, w, b, plan_counts, None)),
        "sr_densify_apply": (lib.sr_densify_workspace_bytes(n), lambda w, b: lib.sr_densify_apply(n, apply_counts, p, p, p, segment, 1, w, b, None)),
        "sr_mesh_count": (lib.sr_mesh_workspace_bytes(dims), lambda w, b: lib.sr_mesh_count(p, dims, 0.0, w, b, p, None)),
        "sr_mesh_emit": (lib.sr_mesh_workspace_bytes(dims), lambda w, b: lib.sr_mesh_emit(p, dims, 0.0, f3, f3, None, w, b, 1, 1, p, p, None)),
        "sr_mesh_components": (post, lambda w, b: lib.sr_mesh_components(p, n, n, p, p, p, w, b, None)),
        "sr_mesh_filter_count": (post, lambda w, b: lib.sr_mesh_filter_count(p, n, n, p, p, p, w, b, p, None)),
        "sr_mesh_filter_emit": (post, lambda w, b: lib.sr_mesh_filter_emit(p, n, n, p, None, w, b, 1, 1, p, None, p, None)),
        "sr_points_in_frame": (lib.sr_unveil_workspace_bytes(n, 1), lambda w, b: lib.sr_points_in_frame(n, p, p, p, p, w, b, p, None)),
        "sr_points_in_frame_emit": (lib.sr_unveil_workspace_bytes(n, 1), lambda w, b: lib.sr_points_in_frame_emit(n, p, p, p, w, b, 1, p, p, None)),
        "sr_frame_visibility": (lib.sr_unveil_workspace_bytes(n, 2), lambda w, b: lib.sr_frame_visibility(n, 2, p, p, p, w, b, p, p, None)),
        "sr_voxel_bounds": (voxel, lambda w, b: lib.sr_voxel_bounds(n, p, 0, w, b, p, None)),
        "sr_voxel_group": (voxel, lambda w, b: lib.sr_voxel_group(n, p, 1, None, 0, d3, 0.1, 100, w, b, p, None)),
        "sr_voxel_emit": (voxel, lambda w, b: lib.sr_voxel_emit(n, p, 0, None, 0, None, 0, w, b, 1, 1, p, None, None, None, None, None, None)),
        "sr_lidar_label_decide": (lidar, lambda w, b: lib.sr_lidar_label_decide(n, p, 1, None, 1, n, p, 1, 1, 3, 0, None, 0, w, b, p, None)),
        "sr_lidar_label_emit": (lidar, lambda w, b: lib.sr_lidar_label_emit(n, p, 1, None, 1, n, 1, w, b, 1, p, None, None, None, None, None)),
        "sr_lidar_vote": (lidar, lambda w, b: lib.sr_lidar_vote(n, p, 1, p, 1, 3, None, w, b, p, p, None)),
    }


# name -> what the library of commit 287dd84 (every entry point still in api.hip, every check written out) answers to a NULL workspace, to
# one a byte short, and to an address with & 15 == 8: (status, the whole text of sr_last_error()).  Mesh's short workspace is -1 where every
# other is -3.  None: that library has no alignment test there and, the other arguments being acceptable, nothing refuses the call before its
# first launch (knn, cluster, the image loss, the three auxiliary losses, the sky backward, sr_densify_apply) -- never called here.
_NULL, _MISALIGNED = (INVALID, "workspace is NULL"), (INVALID, "workspace is not 16-B aligned")
WORKSPACE_REFUSALS = {
    "sr_knn_mean_dist2": ((INVALID, "NULL argument"), (TOO_SMALL, "workspace 9983 < 9984"), None),
    "sr_cluster_radius": ((INVALID, "NULL argument"), (TOO_SMALL, "workspace 9215 < 9216"), None),
    "sr_image_loss_forward": ((INVALID, "image / gt / workspace is NULL"), (TOO_SMALL, "workspace 37375 < 37376"), None),
    "sr_image_loss_backward": ((INVALID, "image / gt / workspace is NULL"), (TOO_SMALL, "workspace 37375 < 37376"), None),
    "sr_semantic_ce_forward": ((INVALID, "sr_semantic_ce_forward: workspace is NULL"), (TOO_SMALL, "sr_semantic_ce_forward: workspace 15 < 16"), None),
    "sr_surface_reg_forward": ((INVALID, "sr_surface_reg_forward: workspace is NULL"), (TOO_SMALL, "sr_surface_reg_forward: workspace 15 < 16"), None),
    "sr_opacity_shrink_forward": ((INVALID, "sr_opacity_shrink_forward: workspace is NULL"), (TOO_SMALL, "sr_opacity_shrink_forward: workspace 15 < 16"), None),
    "sr_sky_backward": ((INVALID, "sr_sky_backward: workspace is NULL"), (TOO_SMALL, "sr_sky_backward: workspace 19666943 < 19666944"), None),
    "sr_densify_plan": (_NULL, (TOO_SMALL, "workspace 1023 < 1024"), _MISALIGNED),
    "sr_densify_apply": (_NULL, (TOO_SMALL, "workspace 1023 < 1024"), None),
    "sr_mesh_count": (_NULL, (INVALID, "workspace 767 < 768"), _MISALIGNED),
    "sr_mesh_emit": (_NULL, (INVALID, "workspace 767 < 768"), _MISALIGNED),
    "sr_mesh_components": (_NULL, (TOO_SMALL, "workspace 1023 < 1024"), _MISALIGNED),
    "sr_mesh_filter_count": (_NULL, (TOO_SMALL, "workspace 1023 < 1024"), _MISALIGNED),
    "sr_mesh_filter_emit": (_NULL, (TOO_SMALL, "workspace 1023 < 1024"), _MISALIGNED),
    "sr_points_in_frame": (_NULL, (TOO_SMALL, "workspace 767 < 768"), _MISALIGNED),
    "sr_points_in_frame_emit": (_NULL, (TOO_SMALL, "workspace 767 < 768"), _MISALIGNED),
    "sr_frame_visibility": (_NULL, (TOO_SMALL, "workspace 767 < 768"), _MISALIGNED),
    "sr_voxel_bounds": (_NULL, (TOO_SMALL, "workspace 11007 < 11008"), _MISALIGNED),
    "sr_voxel_group": (_NULL, (TOO_SMALL, "workspace 11007 < 11008"), _MISALIGNED),
    "sr_voxel_emit": (_NULL, (TOO_SMALL, "workspace 11007 < 11008"), _MISALIGNED),
    "sr_lidar_label_decide": (_NULL, (TOO_SMALL, "workspace 767 < 768"), _MISALIGNED),
    "sr_lidar_label_emit": (_NULL, (TOO_SMALL, "workspace 767 < 768"), _MISALIGNED),
    "sr_lidar_vote": (_NULL, (TOO_SMALL, "workspace 767 < 768"), _MISALIGNED),
}


def test_workspace_refusals_are_the_recorded_ones(lib):
    dummy = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(dummy) + (-ctypes.addressof(dummy)) % 16
    calls = _workspace_calls(lib, p)
    assert sorted(calls) == sorted(WORKSPACE_REFUSALS) and len(calls) == 24
    for name, (need, call) in calls.items():
        assert need >= 16, name
        for what, args, want in zip(("NULL", "short", "misaligned"), ((None, need), (p, need - 1), (p + 8, need)), WORKSPACE_REFUSALS[name]):
            if want is None:
                continue
            got = (call(*args), lib.sr_last_error().decode())
            assert got == want, (name, what, got)


# ---- state-buffer refusals -------------------------------------------------------------------------------------------------------------
# entry point -> the state buffers it takes: what tests/golden/state_buffer_refusals.json must hold a NULL and a short row for
STATE_BUFFERS = {
    "sr_geom_view": ["geom"], "sr_binning_view": ["binning"], "sr_image_view": ["image"],
    "sr_forward_plan": ["geom"], "sr_forward_render": ["geom", "binning", "image"],
    "sr_backward_blend": ["geom", "binning", "image", "workspace"], "sr_backward_geometry": ["geom", "binning", "image", "workspace"],
    "sr_backward": ["geom", "binning", "image", "workspace"], "sr_backward_colors": ["geom", "workspace"],
    "sr_class_forward_render": ["geom", "binning", "class_image"], "sr_class_backward": ["geom", "binning", "class_image", "workspace"],
    "sr_class_forward_shared": ["geom", "binning", "class_state"], "sr_class_backward_shared": ["geom", "binning", "class_state", "workspace"],
    "sr_debug_pair_decisions": ["geom", "binning"],
}


def test_state_buffer_refusals_are_the_recorded_ones(lib):
    """What every rasteriser entry point answers to a NULL or short state buffer, and to a NULL radii / grads / dL_* / out_* argument: status
    and whole text as tools/record_state_buffer_refusals.py recorded them from the library of commit d9479ec, whose api.hip is byte for byte
    that of 01339f2, the last commit with every entry point's argument resolution written out.  The calls are tests/state_buffer_cases.py's.
    Where that library said "NULL buffer argument", "state buffer too small" or "workspace too small", the row holds the text that names the
    buffer (and both sizes) instead, with the recorded one beside it as "recorded_text"; the status is the recorded one in every row."""
    import json
    from tests import state_buffer_cases as cases
    with open(os.path.join(ROOT, "tests", "golden", "state_buffer_refusals.json")) as f:
        recorded = json.load(f)
    assert recorded["recorded_from_source_digest"] != lib.sr_source_digest().decode()      # not recorded from the library under test
    key = lambda r: (r["entry"], r["argument"], r["fault"], r.get("case"), tuple(tuple(x) for x in r.get("also", ())))
    rows = {key(r): (r["status"], r["text"]) for r in recorded["refusals"]}
    assert len(rows) == len(recorded["refusals"])
    assert sorted(cases.ARGUMENTS) == sorted(STATE_BUFFERS) and len(STATE_BUFFERS) == 14
    for entry, buffers in STATE_BUFFERS.items():
        assert cases.buffers_of(entry) == buffers, entry
        for b in buffers:
            assert (entry, b, "null", None, ()) in rows and (entry, b, "short", None, ()) in rows, (entry, b)
        assert sorted(k[1:3] for k in rows if k[0] == entry and k[3:] == (None, ())) == sorted(cases.faults(entry)), entry      # the other pointers too, nothing else
    # the rows of another case are the ones without a recorded value ("recorded_text" null), the rows with two faults the listed ones, and
    # the rows whose recorded text named no buffer and was restated had one of those three texts
    assert sorted(k for k in rows if k[3] is not None) == sorted(cases.UNRECORDED) and sorted(k for k in rows if k[4]) == sorted(cases.DOUBLE_FAULTS)
    assert [key(r) for r in recorded["refusals"] if r.get("recorded_text", "") is None] == cases.UNRECORDED
    assert {r["recorded_text"] for r in recorded["refusals"] if r.get("recorded_text")} == {"NULL buffer argument", "state buffer too small", "workspace too small"}
    scene = cases.Scene(lib)
    for k, want in rows.items():
        assert scene.refusal(*k) == want, k


def test_cpu_tensors_are_rejected_loudly():
    import torch
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    r = GaussianRasterizer(s)
    with pytest.raises(Exception, match="excatly one"):
        r(means3D=torch.zeros(4, 3), means2D=torch.zeros(4, 3), opacities=torch.ones(4, 1), scales=torch.ones(4, 2), rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="exactly one"):
        r(means3D=torch.zeros(4, 3), means2D=torch.zeros(4, 3), opacities=torch.ones(4, 1), colors_precomp=torch.zeros(4, 3))
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        r(means3D=torch.zeros(4, 3), means2D=torch.zeros(4, 3), opacities=torch.ones(4, 1), colors_precomp=torch.zeros(4, 3),
          scales=torch.ones(4, 2), rotations=torch.ones(4, 4))


def test_every_tile_shape_is_accepted_by_the_multi_colour_and_class_passes():
    """The 6 / 9-channel passes and the per-class pass exist for every tile shape of BASELINE config 5's sweep, 32x16 included (round 5: K7
    walks a 32x16 tile's list once per 32x8 band for the wide records): nothing about `tile=` is refused in python -- the calls get as far
    as any CPU-tensor call does.  An unknown shape is refused by the library, by name."""
    import torch
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(9), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    z = lambda *shape: torch.zeros(*shape)
    geo = dict(means3D=z(4, 3), means2D=z(4, 3), opacities=torch.ones(4, 1), scales=torch.ones(4, 2), rotations=torch.ones(4, 4))
    for tile in [(32, 16), (8, 8), (16, 16)]:
        with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
            GaussianRasterizer(s, tile=tile)(colors_precomp=z(4, 6), **geo)
        with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
            GaussianRasterizer(s, tile=tile)(shs=z(4, 16, 3), extra_colors=z(4, 6), **geo)
        with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
            GaussianRasterizer(s, tile=tile).class_distortions(z(4, 3), z(4, 3), torch.ones(4, 1), torch.ones(4, 2), torch.ones(4, 4), torch.zeros(4, dtype=torch.int32), 5)


def test_no_kernel_uses_scratch_memory(tmp_path):
    """Every gfx950 kernel of the library keeps its per-lane state in registers: no private (scratch) segment, no spills.
    (A private array indexed with a run-time value, or a register budget forced too low, silently turns into scratch traffic.)"""
    import glob, re, shutil, subprocess
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not present")
    so = shutil.copy(_lib.LIB_PATH, os.path.join(tmp_path, "lib.so"))
    subprocess.run([objdump, "--offloading", so], check=True, capture_output=True)
    objs = glob.glob(so + ".*gfx950*")
    assert objs, "no gfx950 code object found in the library"
    kernels = 0
    for co in objs:
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split(".agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
            spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
            assert scratch == 0 and spills == 0, f"{name}: {scratch} B scratch, {spills} spilled VGPRs"
            kernels += 1
    assert kernels >= 40


def test_roctx_ranges_are_opt_in_and_balanced():
    """SURFEL_ROCTX=1 brackets every operator entry point with a roctx range (rocprofv3 --marker-trace); without it
    no tracing library is loaded.  Here: the shim loads libroctx64 only when asked, and a push is always matched by its pop."""
    import subprocess
    code = ("from diff_surfel_rasterization import _C\n"
            "lib = _C._roctx_lib()\n"
            "import os\n"
            "want = os.environ.get('SURFEL_ROCTX') == '1'\n"
            "assert bool(lib) == want, (lib, want)\n"
            "with _C._range('outer'):\n"
            "    with _C._range('inner'):\n"
            "        pass\n"
            "if want:\n"
            "    assert lib.roctxRangePop() < 0   # nothing left on the stack: every push above was popped\n"
            "print('roctx', want)\n")
    for flag in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SURFEL_ROCTX=flag), capture_output=True, text=True, timeout=300)
        if flag == "1" and "OSError" in r.stderr:
            pytest.skip("libroctx64 not present on this machine")
        assert r.returncode == 0 and f"roctx {flag == '1'}" in r.stdout, r.stdout + r.stderr[-2000:]


def test_library_carries_the_digest_of_the_tree(lib):
    """The prebuilt .so travels to the GPU box next to the sources: it must BE the build of those sources.  build() decides by this digest
    (content of csrc/*, include/*.h and the build script -- not time stamps), the loader refuses a mismatch, sr_source_digest() reports it."""
    from streetunveiler_amd import build as sb
    want = sb.source_digest()
    assert sb.embedded_digest(sb.LIB) == want
    assert lib.sr_source_digest().decode() == want
    assert sb.embedded_digest(__file__) is None   # (a file without the tag)


# ---- the binding against the header's text ---------------------------------------------------------------------------------------------
# _lib.PROTOTYPES, the Sr* structures and the mirrored SR_* constants are a second, hand-kept statement of include/surfel_raster.h: a wrong
# width or a missing size_t in an argument list corrupts the call frame silently, and only on the GPU machine.  Held here to the header
# itself, parsed with regular expressions (it is regular: one declarator per parameter, no function pointers, no nested structures).
_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
            "uint8_t": ctypes.c_uint8, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int}
_DECLARATOR = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)\s*(?:\[(\d+)\])?")


def _header_code():
    with open(os.path.join(ROOT, "include", "surfel_raster.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _header_prototypes():
    """{name: (return type text, [(base type, is pointer)])} of every function the header declares."""
    found = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w ]*?\*?)\s*\b(sr_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", _header_code(), flags=re.M):
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = _DECLARATOR.fullmatch(" ".join(p.split()))
            assert m and m.group(4) is None and "," not in m.group(3), (name, p)
            args.append((m.group(1), m.group(2) == "*"))
        assert name not in found, name
        found[name] = (" ".join(ret.split()), args)
    return found


def _header_structs():
    """{name: [(field, ctypes type)]}: a pointer field is a c_void_p, an array field the array type, a scalar itself."""
    found = {}
    for name, body in re.findall(r"typedef struct (Sr\w+) \{(.*?)\}\s*\1;", _header_code(), flags=re.S):
        fields = []
        for decl in body.split(";"):
            if not decl.strip():
                continue
            m = _DECLARATOR.fullmatch(" ".join(decl.split()))
            assert m, (name, decl)
            base, pointer, names, count = m.groups()
            ctype = ctypes.c_void_p if pointer else _SCALARS[base]
            for field in names.replace(" ", "").split(","):
                fields.append((field, ctype * int(count) if count else ctype))
        found[name] = fields
    return found


def test_prototype_table_matches_header():
    declared = _header_prototypes()
    assert sorted(declared) == _declared_functions() and list(declared) == list(_lib.PROTOTYPES)      # every function once, in the header's order
    returns = dict(_SCALARS, **{"void": None, "const char*": ctypes.c_char_p})
    for name, (ret, params) in declared.items():
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is returns[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, ((base, pointer), got) in enumerate(zip(params, argtypes)):
            if not pointer:
                allowed = [_SCALARS[base]]
            elif base.startswith("Sr"):
                allowed = [ctypes.POINTER(getattr(_lib, base))]
            elif base == "void":
                allowed = [ctypes.c_void_p]
            else:      # a device or host array of scalars: untyped, or typed by its pointee
                allowed = [ctypes.c_void_p, ctypes.POINTER(_SCALARS[base])]
            assert any(got is a for a in allowed), (name, k, base, pointer, got)
        if params and params[-1] == ("void", True) and not name.endswith(("_bytes", "_view")):
            assert argtypes[-1] is ctypes.c_void_p      # (the `void* stream` _call.call appends)


def test_prototypes_are_applied_to_the_library(lib):
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def _c_layout(fields):
    """(offsets, size) the C layout rules give: every member aligned to its own (element) size, the whole to the largest of them."""
    offsets, at, widest = [], 0, 1
    for _, ctype in fields:
        align = ctypes.sizeof(getattr(ctype, "_type_", ctype)) if hasattr(ctype, "_length_") else ctypes.sizeof(ctype)
        at = (at + align - 1) // align * align
        offsets.append(at)
        at += ctypes.sizeof(ctype)
        widest = max(widest, align)
    return offsets, (at + widest - 1) // widest * widest


def test_every_struct_matches_header():
    declared = _header_structs()
    bound = {name: t for name, t in vars(_lib).items() if isinstance(t, type) and issubclass(t, ctypes.Structure)}
    assert sorted(declared) == sorted(bound) and len(declared) == 13
    for name, fields in declared.items():
        got = bound[name]._fields_
        assert [f[0] for f in got] == [f[0] for f in fields], name
        for (field, want), (_, have) in zip(fields, got):
            same = (have._type_ is want._type_ and have._length_ == want._length_) if hasattr(want, "_length_") else have is want
            assert same, (name, field, want, have)
        offsets, size = _c_layout(fields)
        assert [getattr(bound[name], f).offset for f, _ in fields] == offsets and ctypes.sizeof(bound[name]) == size, name


def test_mirrored_constants_match_header():
    code = _header_code()
    defines = {name: int(value.rstrip("u"), 0) for name, value in re.findall(r"^#define (SR_\w+) (\w+)\b", code, flags=re.M)}
    mirrored = {name: v for name, v in vars(_lib).items() if name.startswith("SR_") and isinstance(v, int)}
    for family, count in (("SR_FLAG_", 11), ("SR_ACT_", 3), ("SR_MASK_FIXED_", 6), ("SR_DENSIFY_", 13), ("SR_ADAM_", 2), ("SR_ABI_VERSION", 1)):
        assert sum(name.startswith(family) for name in mirrored) == sum(name.startswith(family) for name in defines) == count, family
    for name, value in mirrored.items():
        assert defines.get(name) == value, (name, value, defines.get(name))
    stages = re.search(r"typedef enum SrStage \{(.*?)\} SrStage;", code, flags=re.S).group(1)
    stages = sorted((int(v), name) for name, v in re.findall(r"(SR_STAGE_\w+) = (\d+)", stages))
    assert [v for v, _ in stages] == list(range(len(stages))) and stages[-1] == (len(_lib.SR_STAGE_NAMES), "SR_STAGE_COUNT")
    assert _lib.SR_STAGE_NAMES == [name[len("SR_STAGE_"):].lower() for _, name in stages[:-1]]


def test_ptr_maps_nothing_to_null():
    import torch
    from streetunveiler_amd._call import buf, ptr
    assert ptr(None) is None and ptr(torch.empty(0)) is None and ptr(torch.empty((0, 3))) is None
    one = torch.zeros(1)
    assert isinstance(ptr(one), ctypes.c_void_p) and ptr(one).value == one.data_ptr()
    address, size = buf(torch.zeros(5, dtype=torch.uint8))
    assert isinstance(address, ctypes.c_void_p) and size == 5


@pytest.mark.gpu
def test_refusal_through_call_carries_name_and_message(lib):
    """An ARGUMENT refusal, taken before any launch (sr_opacity_shrink_forward checks P < 1 first): _call.call raises SurfelRasterError
    with the function's name and the text of sr_last_error()."""
    import torch
    from streetunveiler_amd._call import buf, call, ptr
    dev = torch.device("cuda:0")
    opacity, ws, out = torch.zeros(4, device=dev), torch.empty(256, dtype=torch.uint8, device=dev), torch.empty(1, device=dev)
    with pytest.raises(_lib.SurfelRasterError) as err:
        call("sr_opacity_shrink_forward", dev, 0, ptr(opacity), 0, *buf(ws), ptr(out))
    last = lib.sr_last_error().decode()
    assert last == "P 0 < 1" and "sr_opacity_shrink_forward" in str(err.value) and last in str(err.value)
    with pytest.raises(_lib.SurfelRasterError, match=r"sr_adam_step failed \(-1\): n_segments 0 not in 1\.\.8"):
        call("sr_adam_step", dev, (_lib.SrAdamSegment * 1)(), 0, 0.9, 0.999, 1e-8)

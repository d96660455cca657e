"""ctypes binding of include/surfel_raster.h (the C-ABI of the HIP library).

Fails loudly when the library is missing: there is NO CPU fallback in the product path.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SURFEL_RASTER_LIB: another BUILD of the same library -- one of the named-switch variants of include/surfel_switches.h
# (`python -m streetunveiler_amd.build --variant <name>` -> lib/variants/<name>/libsurfel_raster.so).  Same ABI, still no CPU path.
LIB_PATH = os.environ.get("SURFEL_RASTER_LIB") or os.path.join(HERE, "lib", "libsurfel_raster.so")

SR_ACT_EXP_SCALES, SR_ACT_SIGMOID_OPACITY, SR_ACT_NORMALIZE_ROTATIONS = 1, 2, 4
SR_FLAG_NO_QUADRANT_CULL = 1
SR_FLAG_BALLOT_RANKING = 2
SR_FLAG_ROW_MAPPED_FORWARD = 4
SR_FLAG_QUADRANT_MAPPED_FORWARD = 8
SR_FLAG_FORWARD_ONLY = 16
SR_FLAG_NO_PRECOMP_COLOR_GRAD = 32
SR_FLAG_BINNING_CAPACITY = 64
SR_FLAG_ONE_SWEEP_SORT = 128
SR_FLAG_ONE_WAVE_BACKWARD = 256
SR_FLAG_COOP_BACKWARD = 512
SR_FLAG_ROW_BACKWARD = 1024
SR_ABI_VERSION = 10
SR_STAGE_NAMES = ["preprocess", "depth_sort", "scan", "expand_x", "expand_y", "ranges", "blend_fwd", "blend_bwd",
                  "preprocess_bwd", "class_partition", "class_fwd", "class_bwd"]


class SrFrame(C.Structure):
    _fields_ = [("image_height", C.c_int32), ("image_width", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("scale_modifier", C.c_float), ("sh_degree", C.c_int32), ("prefiltered", C.c_int32), ("debug", C.c_int32),
                ("bg", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
                ("tile_width", C.c_int32), ("tile_height", C.c_int32), ("flags", C.c_uint32), ("blend_counters", C.c_void_p)]


class SrGaussians(C.Structure):
    _fields_ = [("P", C.c_int32), ("sh_coeffs", C.c_int32), ("color_channels", C.c_int32), ("activations", C.c_int32),
                ("means3D", C.c_void_p), ("opacities", C.c_void_p),
                ("scales", C.c_void_p), ("rotations", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
                ("transMat_precomp", C.c_void_p), ("mask", C.c_void_p)]


class SrGradients(C.Structure):
    _fields_ = [("dL_dmeans2D", C.c_void_p), ("dL_dcolors", C.c_void_p), ("dL_dopacity", C.c_void_p),
                ("dL_dmeans3D", C.c_void_p), ("dL_dtransMat", C.c_void_p), ("dL_dsh", C.c_void_p),
                ("dL_dscales", C.c_void_p), ("dL_drotations", C.c_void_p)]


class SrGeomView(C.Structure):
    _fields_ = [("splats", C.c_void_p), ("depth_keys", C.c_void_p), ("tiles_touched", C.c_void_p), ("clamped", C.c_void_p),
                ("sorted_gid", C.c_void_p), ("frame_counts", C.c_void_p)]


class SrBinningView(C.Structure):
    _fields_ = [("point_list", C.c_void_p), ("ranges", C.c_void_p), ("tile_order", C.c_void_p)]


class SrImageView(C.Structure):
    _fields_ = [("final_T", C.c_void_p), ("n_contrib", C.c_void_p)]


class SrAdamSegment(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_int64),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float)]


class SrAdamRowSegment(C.Structure):   # sr_adam_step_rows: SrAdamSegment (its layout is frozen) + the elements per row of the mask
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_int64),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("row_len", C.c_int64)]


class SrMaskTensors(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("features_dc", C.c_void_p), ("features_rest", C.c_void_p), ("opacity", C.c_void_p),
                ("scaling", C.c_void_p), ("rotation", C.c_void_p)]


class SrMaskEffective(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("features", C.c_void_p), ("opacity", C.c_void_p), ("scaling", C.c_void_p), ("rotation", C.c_void_p)]


SR_ADAM_MAX_SEGMENTS, SR_ADAM_CHUNK = 8, 4096
# the reference's MASK_PROPERTY bit order [REF scene/mask_gaussian.py:29-30]
SR_MASK_FIXED_XYZ, SR_MASK_FIXED_FEATURES_DC, SR_MASK_FIXED_FEATURES_REST, SR_MASK_FIXED_SCALING, SR_MASK_FIXED_ROTATION, SR_MASK_FIXED_OPACITY = \
    1, 2, 4, 8, 16, 32


class SrDensifySegment(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_words", C.c_int32), ("role", C.c_int32)]


class SrTsdfViews(C.Structure):
    _fields_ = [("maps", C.c_void_p), ("full_proj", C.c_void_p), ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32)]


class SrTsdfSpace(C.Structure):
    _fields_ = [("voxel_size", C.c_double), ("contract", C.c_int32), ("center", C.c_float * 3), ("radius", C.c_float)]


SR_DENSIFY_MAX_SEGMENTS = 8
SR_DENSIFY_FLAG_CLONE, SR_DENSIFY_FLAG_SPLIT, SR_DENSIFY_FLAG_KEEP_SELF, SR_DENSIFY_FLAG_KEEP_CHILD = 1, 2, 4, 8
SR_DENSIFY_KIND_ORIGINAL, SR_DENSIFY_KIND_CLONE, SR_DENSIFY_KIND_CHILD0, SR_DENSIFY_KIND_CHILD1 = 0, 1, 2, 3
SR_DENSIFY_ROLE_COPY, SR_DENSIFY_ROLE_MOMENT, SR_DENSIFY_ROLE_XYZ, SR_DENSIFY_ROLE_SCALING = 0, 1, 2, 3
SR_RESIZE_BINARISE, SR_RESIZE_F32_CHW = 1, 2      # sr_resize_u8_pass flags: the epilogue of a resize's last pass


# include/surfel_raster.h, once: every function it declares -> (return type, argument types), in the header's order (tests/test_abi.py holds
# this table, the structures and the constants above to the header's text).  A `void* stream` comes last wherever a call launches.
_i32, _i64, _u32, _sz, _f32, _f64, _int, _vp, _str = C.c_int32, C.c_int64, C.c_uint32, C.c_size_t, C.c_float, C.c_double, C.c_int, C.c_void_p, C.c_char_p
_P = C.POINTER
_FG = [_P(SrFrame), _P(SrGaussians)]
_GEOM = _BINNING = _IMAGE = _WS = [_vp, _sz]      # a state buffer or a workspace: its address and its size in bytes
PROTOTYPES = {
    "sr_abi_version": (_int, []),
    "sr_build_switches": (_u32, []),
    "sr_source_digest": (_str, []),
    "sr_last_error": (_str, []),
    "sr_geom_bytes": (_sz, [_i32]),
    "sr_binning_bytes": (_sz, [_i32, _u32, _i32, _i32]),
    "sr_image_bytes": (_sz, [_i32, _i32]),
    "sr_backward_workspace_bytes": (_sz, [_i32, _u32, _i32]),
    "sr_geom_view": (_int, _GEOM + [_i32, _P(SrGeomView)]),
    "sr_binning_view": (_int, _BINNING + [_i32, _u32, _i32, _i32, _P(SrBinningView)]),
    "sr_image_view": (_int, _IMAGE + [_i32, _i32, _P(SrImageView)]),
    "sr_forward_plan": (_int, _FG + _GEOM + [_vp, _P(_u32), _vp]),
    "sr_forward_render": (_int, _FG + _GEOM + _BINNING + _IMAGE + [_u32, _vp, _vp, _vp]),
    "sr_backward": (_int, _FG + [_vp] + _GEOM + _BINNING + _IMAGE + [_u32, _vp, _vp] + _WS + [_P(SrGradients), _vp]),
    "sr_backward_blend": (_int, _FG + _GEOM + _BINNING + _IMAGE + [_u32, _vp, _vp] + _WS + [_vp]),
    "sr_backward_colors": (_int, _FG + [_vp] + _GEOM + [_u32] + _WS + [_vp, _vp]),
    "sr_backward_geometry": (_int, _FG + [_vp] + _GEOM + _BINNING + _IMAGE + [_u32] + _WS + [_P(SrGradients), _vp]),
    "sr_class_image_bytes": (_sz, [_i32, _i32, _i32]),
    "sr_class_forward_render": (_int, _FG + [_i32] + _GEOM + _BINNING + _IMAGE + [_u32, _vp, _vp]),
    "sr_class_backward": (_int, _FG + [_i32, _vp] + _GEOM + _BINNING + _IMAGE + [_u32, _vp] + _WS + [_P(SrGradients), _vp]),
    "sr_class_shared_bytes": (_sz, [_i32, _i32, _i32, _i32, _u32]),
    "sr_class_forward_shared": (_int, _FG + [_i32, _vp] + _GEOM + _BINNING + _IMAGE + [_u32, _vp, _vp]),
    "sr_class_backward_shared": (_int, _FG + [_i32] + _GEOM + _BINNING + _IMAGE + [_u32, _vp] + _WS + [_vp]),
    "sr_sh_gradient_expand": (_int, [_i32] * 4 + [_vp] * 5),
    "sr_knn_workspace_bytes": (_sz, [_i32, _i32]),
    "sr_knn_mean_dist2": (_int, [_i32, _vp, _i32, _vp, _i32, _i32, _vp] + _WS + [_vp]),
    "sr_cluster_workspace_bytes": (_sz, [_i32]),
    "sr_cluster_radius": (_int, [_i32, _vp, _vp, _f32, _vp] + _WS + [_vp]),
    "sr_mark_visible": (_int, [_i32] + [_vp] * 5),
    "sr_postprocess_forward": (_int, [_i32, _i32, _f32, _f32, _f32] + [_vp] * 7),
    "sr_postprocess_backward": (_int, [_i32, _i32, _f32, _f32, _f32] + [_vp] * 9),
    "sr_image_loss_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "sr_image_loss_forward": (_int, [_i32, _i32, _i32, _f32] + [_vp] * 4 + _WS + [_vp, _vp]),
    "sr_image_loss_backward": (_int, [_i32, _i32, _i32, _f32] + [_vp] * 4 + _WS + [_vp] * 5),
    "sr_aux_loss_workspace_bytes": (_sz, [_i64]),
    "sr_semantic_ce_forward": (_int, [_i32] * 3 + [_vp, _vp, _i32, _P(_f32)] + _WS + [_vp, _vp]),
    "sr_semantic_ce_backward": (_int, [_i32] * 3 + [_vp, _vp, _i32, _P(_f32)] + [_vp] * 3),
    "sr_surface_reg_forward": (_int, [_i32, _i32] + [_vp] * 3 + [_f64, _f64] + _WS + [_vp, _vp]),
    "sr_surface_reg_backward": (_int, [_i32, _i32, _vp, _vp, _f64, _f64] + [_vp] * 5),
    "sr_opacity_shrink_forward": (_int, [_i64, _vp, _i32] + _WS + [_vp, _vp]),
    "sr_opacity_shrink_backward": (_int, [_i64, _vp, _i32, _vp, _vp, _vp]),
    "sr_sky_workspace_bytes": (_sz, [_i32]),
    "sr_sky_forward": (_int, [_i32, _i32] + [_vp] * 9 + [_i32, _vp, _vp]),
    "sr_sky_backward": (_int, [_i32, _i32] + [_vp] * 10 + [_i32] + _WS + [_vp] * 9),
    "sr_adam_step": (_int, [_P(SrAdamSegment), _i32, _f64, _f64, _f64, _vp]),
    "sr_adam_step_rows": (_int, [_P(SrAdamRowSegment), _i32, _i32, _vp, _f64, _f64, _f64, _vp]),
    "sr_mask_compose": (_int, [_i32, _i32, _P(SrMaskTensors), _P(SrMaskTensors), _vp, _u32, _P(SrMaskEffective), _vp]),
    "sr_mask_compose_backward": (_int, [_i32, _i32, _P(SrMaskEffective), _vp, _u32, _P(SrMaskTensors), _vp]),
    "sr_densification_stats": (_int, [_i32] + [_vp] * 6),
    "sr_densify_workspace_bytes": (_sz, [_i32]),
    "sr_densify_plan": (_int, [_i32] + [_vp] * 4 + [_f32] * 4 + [_vp] + _WS + [_P(_u32), _vp]),
    "sr_densify_apply": (_int, [_i32, _P(_u32), _vp, _vp, _vp, _P(SrDensifySegment), _i32] + _WS + [_vp]),
    "sr_tsdf_fuse": (_int, [_P(SrTsdfViews), _P(SrTsdfSpace), _i32] + [_vp] * 5),
    "sr_tsdf_fuse_grid": (_int, [_P(SrTsdfViews), _P(SrTsdfSpace), _P(_i32), _P(_f32), _P(_f32), _i32, _i32] + [_vp] * 4),
    "sr_mesh_workspace_bytes": (_sz, [_P(_i32)]),
    "sr_mesh_count": (_int, [_vp, _P(_i32), _f32] + _WS + [_vp, _vp]),
    "sr_mesh_emit": (_int, [_vp, _P(_i32), _f32, _P(_f32), _P(_f32), _P(SrTsdfSpace)] + _WS + [_i32, _i32, _vp, _vp, _vp]),
    "sr_mesh_post_workspace_bytes": (_sz, [_i32, _i32]),
    "sr_mesh_components": (_int, [_vp, _i32, _i32, _vp, _vp, _vp] + _WS + [_vp]),
    "sr_mesh_filter_count": (_int, [_vp, _i32, _i32, _vp, _vp, _vp] + _WS + [_vp, _vp]),
    "sr_mesh_filter_emit": (_int, [_vp, _i32, _i32, _vp, _vp] + _WS + [_i32, _i32, _vp, _vp, _vp, _vp]),
    "sr_unveil_workspace_bytes": (_sz, [_i32, _i32]),
    "sr_points_in_frame": (_int, [_i32] + [_vp] * 4 + _WS + [_vp, _vp]),
    "sr_points_in_frame_emit": (_int, [_i32] + [_vp] * 3 + _WS + [_i32, _vp, _vp, _vp]),
    "sr_frame_visibility": (_int, [_i32, _i32] + [_vp] * 3 + _WS + [_vp] * 3),
    "sr_semantic_mask_of_points": (_int, [_i32, _i32] + [_vp] * 4 + [_i32, _i32, _u32] + [_vp] * 3),
    "sr_dilate_mask": (_int, [_i32] * 3 + [_vp] * 3),
    "sr_instance_pixel_mask": (_int, [_i32, _i32, _vp, _vp, _f32, _i32, _vp, _vp]),
    "sr_refill_mask": (_int, [_i32] * 3 + [_vp] * 3 + [_f32, _i32, _vp, _vp]),
    "sr_inpaint_conditions": (_int, [_i32, _i32] + [_vp] * 7 + [_f32, _i32] + [_vp] * 7),
    "sr_voxel_workspace_bytes": (_sz, [_i32]),
    "sr_voxel_bounds": (_int, [_i32, _vp, _i32] + _WS + [_vp, _vp]),
    "sr_voxel_group": (_int, [_i32, _vp, _i32, _vp, _i32, _P(_f64), _f64, _i64] + _WS + [_vp, _vp]),
    "sr_voxel_emit": (_int, [_i32, _vp, _i32, _vp, _i32, _vp, _i32] + _WS + [_i32, _i32] + [_vp] * 7),
    "sr_lidar_label_workspace_bytes": (_sz, [_i32, _i32]),
    "sr_lidar_label_decide": (_int, [_i32, _vp, _i32, _vp, _i32, _i32, _vp] + [_i32] * 4 + [_vp, _i32] + _WS + [_vp, _vp]),
    "sr_lidar_label_emit": (_int, [_i32, _vp, _i32, _vp] + [_i32] * 3 + _WS + [_i32] + [_vp] * 6),
    "sr_lidar_vote": (_int, [_i32, _vp, _i32, _vp, _i32, _i32, _vp] + _WS + [_vp] * 3),
    "sr_resize_u8_pass": (_int, [_i32] * 4 + [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _i32, _u32, _vp, _vp]),
    "sr_resize_nearest": (_int, [_i32] * 4 + [_vp, _i64, _i64, _i32, _i32, _vp, _vp]),
    "sr_debug_pair_decisions":(_int, _FG + _GEOM + _BINNING + [_u32, _vp, _vp, _vp]),
    "sr_debug_radix_sort_temp_bytes": (_sz, [_u32]),
    "sr_debug_radix_sort": (_int, [_vp] * 4 + [_u32, _int] + _WS + [_u32, _vp]),
    "sr_rank_mode": (_int, [_vp]),
    "sr_debug_lds_atomic_ranks": (_int, [_vp, _vp, _u32, _int, _vp]),
    "sr_set_stage_timing": (None, [_int]),
    "sr_stage_stats": (_int, [_int, _P(_f32), _P(_int)]),
}
EXPORTS = list(PROTOTYPES)

_lib = None


class SurfelRasterError(RuntimeError):
    pass


def load():
    """Load libsurfel_raster.so; raise (never fall back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SurfelRasterError(
            f"{LIB_PATH} is missing: build it with `python -m streetunveiler_amd.build` "
            "(or __graft_entry__.build()). There is no CPU fallback for the rasterizer.")
    lib = C.CDLL(LIB_PATH)
    missing = []
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            missing.append(name)     # (reported after the digest comparison, whose message says what to do about it)
        else:
            fn.restype, fn.argtypes = restype, argtypes
    # the in-tree library must be the one built from the sources next to it (it travels prebuilt to the GPU box); SURFEL_RASTER_LIB -- a
    # variant or A/B build chosen on purpose -- is taken as it is
    if not os.environ.get("SURFEL_RASTER_LIB"):
        from .build import source_digest
        have, want = lib.sr_source_digest().decode(), source_digest()
        if have != want:
            raise SurfelRasterError(f"{LIB_PATH} was built from other sources (digest {have}, the tree's is {want}): rebuild it with "
                                    "`python -m streetunveiler_amd.build`")
    if missing:
        raise SurfelRasterError(f"{LIB_PATH} does not export {missing}")
    if lib.sr_abi_version() != SR_ABI_VERSION:
        raise SurfelRasterError(f"ABI version mismatch: library reports {lib.sr_abi_version()}, binding expects {SR_ABI_VERSION}")
    _lib = lib
    return lib


# include/surfel_switches.h: bit -> the switch that is NOT at its default in a library reporting that bit (sr_build_switches)
SWITCH_BITS = {1: "SR_TIGHTBBOX=1", 2: "SR_DETACH_WEIGHT=1", 4: "SR_RADIUS_FILTER_FLOOR=0", 8: "SR_MEDIAN_CONTRIBUTOR_MINUS_ONE=0",
               16: "SR_PROXY_DEPTH_VIEW_Z=1", 32: "SR_BACKWARD_WH_FROM_FOCAL=0", 64: "SR_REFERENCE_PZ_SKIP=0"}


def build_switches():
    """Non-default named switches of the loaded library, e.g. ['SR_DETACH_WEIGHT=1']; [] for the shipped configuration (= upstream's
    semantics as SURVEY.md Appendix A states them)."""
    bits = int(load().sr_build_switches())
    return [name for bit, name in SWITCH_BITS.items() if bits & bit]


def check(rc: int, what: str):
    if rc != 0:
        msg = load().sr_last_error().decode("utf-8", "replace")
        raise SurfelRasterError(f"{what} failed ({rc}): {msg}")


def stage_stats():
    """{stage name: (total_ms, launches)} since sr_set_stage_timing(1)."""
    lib = load()
    out = {}
    for i, name in enumerate(SR_STAGE_NAMES):
        ms, n = C.c_float(0), C.c_int(0)
        check(lib.sr_stage_stats(i, C.byref(ms), C.byref(n)), "sr_stage_stats")
        out[name] = (float(ms.value), int(n.value))
    return out

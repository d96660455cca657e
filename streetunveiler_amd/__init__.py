"""streetunveiler_amd -- MI355X-native 2D-Gaussian (surfel) splatting rasterizer.

Only what the hot path needs: csrc/ (HIP kernels + C-ABI), the ctypes loader,
the host-side mirror of the reference operator surface, a synthetic scene
generator for the benchmark, and the frame-sharded multi-GPU helper.
"""
__version__ = "0.1.0"

_IMAGE_LOSS = ("photometric_loss", "photometric_loss_torch", "image_loss_forward", "image_loss_backward", "image_loss_workspace")
_OPTIM = ("SurfelAdam", "adam_step", "adam_step_float64", "densification_stats", "densification_stats_torch")
_CLUSTER = ("radius_components", "cluster_instance_with_mask", "cluster_semantic_instance")
_DENSIFY = ("densify_and_prune", "prune_points", "densify_and_prune_tensors", "densify_and_prune_torch")
_TSDF = ("TsdfViews", "unbounded_tsdf", "unbounded_tsdf_grid", "unbounded_tsdf_torch", "sdf_function", "grid_coordinates")
_MASK_MODEL = ("MaskedSurfelModel", "compose_masked", "compose_masked_torch")
_AUX_LOSS = ("semantic_cross_entropy", "surface_regularisers", "opacity_shrink", "SemanticCrossEntropy", "semantic_cross_entropy_torch",
             "surface_regularisers_torch", "opacity_shrink_torch")
_SKY = ("SkyModel", "sky_rays_mlp", "sky_forward_torch", "position_features")
_MESH = ("marching_cubes", "marching_cubes_numpy", "extract_mesh_unbounded", "contracted_bound", "SurfelMesh")
_MESH_PLY = ("write_mesh_ply", "read_mesh_ply")
_MESH_POST = ("connected_triangles", "post_process_mesh", "connected_triangles_numpy", "post_process_mesh_numpy")
_UNVEIL = ("FrameCamera", "FrameCameras", "pack_cameras", "points_in_frame", "frame_visibility", "pick_view", "semantic_mask_of_points",
           "dilate_mask", "instance_pixel_mask", "refill_mask", "inpaint_conditions", "points_in_frame_torch", "frame_visibility_torch",
           "pick_view_torch", "semantic_mask_of_points_torch", "dilate_mask_numpy", "dilate_mask_torch", "instance_pixel_mask_torch",
           "refill_mask_torch", "inpaint_conditions_torch")
_VOXEL = ("SemanticCloud", "voxel_down_sample", "voxel_down_sample_torch", "create_from_pcd")
_LIDAR_LABEL = ("LabelViews", "LabelledSweeps", "label_sweeps", "vote_semantics", "label_sweeps_numpy", "vote_semantics_numpy", "label_sweeps_torch",
                "vote_semantics_torch", "in_frame_numpy", "certain_mask_numpy")
_FRAMES = ("resize_u8", "pil_to_torch", "frame_tensor", "resize_labels", "resize_u8_numpy", "resize_labels_numpy", "resize_tables")
__all__ = list(_IMAGE_LOSS + _OPTIM + _CLUSTER + _DENSIFY + _TSDF + _MASK_MODEL + _AUX_LOSS + _SKY + _MESH + _MESH_PLY + _MESH_POST + _UNVEIL + _VOXEL +
               _LIDAR_LABEL + _FRAMES)


def __getattr__(name):   # the fused image loss, the optimizer step, the radius clustering, densify / prune, the TSDF fusion and the masked model, imported on first use (this package does not import torch by itself)
    if name in _IMAGE_LOSS:
        from . import image_loss
        return getattr(image_loss, name)
    if name in _OPTIM:
        from . import optim
        return getattr(optim, name)
    if name in _CLUSTER:
        from . import cluster
        return getattr(cluster, name)
    if name in _DENSIFY:
        from . import densify
        return getattr(densify, name)
    if name in _TSDF:
        from . import tsdf
        return getattr(tsdf, name)
    if name in _MASK_MODEL:
        from . import mask_model
        return getattr(mask_model, name)
    if name in _AUX_LOSS:
        from . import aux_loss
        return getattr(aux_loss, name)
    if name in _SKY:
        from . import sky
        return getattr(sky, name)
    if name in _MESH:
        from . import mesh
        return getattr(mesh, name)
    if name in _MESH_PLY:
        from . import ply
        return getattr(ply, name)
    if name in _MESH_POST:
        from . import mesh_post
        return getattr(mesh_post, name)
    if name in _UNVEIL:
        from . import unveil
        return getattr(unveil, name)
    if name in _VOXEL:
        from . import voxel
        return getattr(voxel, name)
    if name in _LIDAR_LABEL:
        from . import lidar_label
        return getattr(lidar_label, name)
    if name in _FRAMES:
        from . import frames
        return getattr(frames, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

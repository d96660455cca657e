"""Host-side mirror of the reference's render operator.

    render / render_with_mask / render_semantic / render_semantic_with_mask

Same names, argument meaning, returned dict keys and error behaviour as
/root/reference/gaussian_renderer/__init__.py (render :18-188, render_with_mask :190-325,
render_semantic :327-460, render_semantic_with_mask :462-598), on top of the drop-in
`diff_surfel_rasterization` package.  `pc` is anything exposing the GaussianModel getters the reference
reads (get_xyz, get_opacity, get_scaling, get_rotation, get_features, active_sh_degree, max_sh_degree and,
for the semantic variants, get_semantics / get_semantics_32bit) -- scene.gaussian_model.GaussianModel and
scene.mask_gaussian.MaskGaussianModel qualify unchanged; `SurfelModel` below is a minimal stand-in for
tests and the benchmark.  `pipe` carries convert_SHs_python, compute_cov3D_python, depth_ratio, debug
[REF /root/reference/arguments/__init__.py:62-68].
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer

from .sh import eval_sh

# [REF /root/reference/utils/semantic_utils.py:100-102]
concerned_classes_list = ["road", "sidewalk", "building", "vegetation", "sky", "vehicle"]
concerned_classes_ind_map = {cn: i for i, cn in enumerate(concerned_classes_list)}
# colour of each of the 6 classes (first rows of the reference's semantic colour table, values 0..255)
_SEMANTIC_COLOR = torch.tensor([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255]])


@dataclass
class PipelineParams:
    convert_SHs_python: bool = False
    compute_cov3D_python: bool = False
    depth_ratio: float = 0.0
    debug: bool = False
    # extension: hand the operator the RAW _opacity / _scaling / _rotation and let K1 / K8 apply the
    # sigmoid / exp / normalize activations and their adjoints (3 elementwise passes + their backward less per call)
    fused_activations: bool = False
    # extension: masks (render_with_mask, semantic filters) go to the operator as a per-Gaussian bool instead of
    # boolean-indexing every parameter tensor first.  Same images; `radii`, `visibility_filter` and `viewspace_points` are then
    # FULL-size (zero / False where masked out) instead of subset-size, which is why it is opt-in.
    fused_mask: bool = False


class SurfelModel:
    """Minimal parameter container with the GaussianModel getter surface.  `raw=False`: activated values are stored
    directly; `raw=True`: `_scaling` / `_opacity` / `_rotation` are the reference's pre-activation parameters and the
    getters apply exp / sigmoid / normalize [REF scene/gaussian_model.py:63-75, 101-123] -- what a PLY checkpoint holds."""

    def __init__(self, xyz, scaling, rotation, opacity, features, semantics=None, active_sh_degree=3, max_sh_degree=3, raw=False):
        self._xyz, self._scaling, self._rotation, self._opacity, self._features = xyz, scaling, rotation, opacity, features
        self._semantics = semantics
        self.active_sh_degree, self.max_sh_degree = active_sh_degree, max_sh_degree
        self.raw = bool(raw)

    @classmethod
    def from_ply(cls, path, device="cuda", max_sh_degree=3):
        """Load a checkpoint in the reference's PLY layout [REF scene/gaussian_model.py:338-382] (raw parameters)."""
        from .ply import load_ply
        d = load_ply(path, max_sh_degree)
        t = lambda a: torch.tensor(a, dtype=torch.float32, device=device).requires_grad_(True)
        # one leaf [P,16,3] (the operator's layout) so that `_features.grad` exists after backward
        features = torch.cat([torch.tensor(d["features_dc"], dtype=torch.float32, device=device),
                              torch.tensor(d["features_rest"], dtype=torch.float32, device=device)], dim=1).requires_grad_(True)
        return cls(t(d["xyz"]), t(d["scaling"]), t(d["rotation"]), t(d["opacity"]), features,
                   semantics=torch.tensor(d["semantics"], dtype=torch.int32, device=device), active_sh_degree=max_sh_degree,
                   max_sh_degree=max_sh_degree, raw=True)

    def save_ply(self, path):
        from .ply import save_ply
        n = lambda x: x.detach().cpu().numpy()
        sem = self._semantics if self._semantics is not None else torch.zeros(self._xyz.shape[0], dtype=torch.int32)
        assert self.raw, "PLY checkpoints hold the raw (pre-activation) parameters"
        save_ply(path, n(self._xyz), n(self._features[:, :1]), n(self._features[:, 1:]), n(self._opacity), n(self._scaling),
                 n(self._rotation), n(sem))

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: torch.exp(s._scaling) if s.raw else s._scaling)
    get_rotation = property(lambda s: torch.nn.functional.normalize(s._rotation) if s.raw else s._rotation)
    get_opacity = property(lambda s: torch.sigmoid(s._opacity) if s.raw else s._opacity)
    get_features = property(lambda s: s._features)
    get_semantics = property(lambda s: s._semantics)
    get_semantics_32bit = property(lambda s: (1 << s._semantics.to(torch.int32)))

    def get_covariance(self, scaling_modifier=1):
        # the reference's producer indexes a third scale component and cannot run with 2-component surfel
        # scales (SURVEY.md 8b "dead inputs"); the operator slot itself takes a [P,9] transMat.
        raise NotImplementedError("compute_cov3D_python is a dead flag for 2D surfels (2-component scales)")


# ---------------------------------------------------------------------------------------------------
def postprocess_allmap(viewpoint_camera, pipe, allmap):
    """allmap[7,H,W] -> the regularisation maps of the render dict [REF gaussian_renderer/__init__.py:148-186;
    utils/point_utils.py:9-37], computed by the fused HIP kernels of csrc/postprocess.hip (the reference runs ~25
    full-image torch kernels here and re-uploads a 25 MB pixel grid from the host on every call)."""
    from .postprocess import postprocess_allmap_fused
    rend_normal, surf_depth, surf_normal, surf_point = postprocess_allmap_fused(viewpoint_camera, pipe.depth_ratio, allmap)
    return {"rend_alpha": allmap[1:2], "rend_normal": rend_normal, "rend_dist": allmap[6:7], "surf_depth": surf_depth,
            "surf_normal": surf_normal, "surf_point": surf_point}


def _settings(viewpoint_camera, pc, pipe, bg, scaling_modifier):
    return GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center, prefiltered=False, debug=pipe.debug)


def _screenspace_points(pc):
    # zero tensor whose .grad receives the screen-space (densification) gradient [REF :28-33]
    p = torch.zeros_like(pc.get_xyz, dtype=pc.get_xyz.dtype, requires_grad=True, device=pc.get_xyz.device) + 0
    try:
        p.retain_grad()
    except Exception:
        pass
    return p


def _sel(t, mask):
    return t if mask is None else t[mask]


def _plain_getters(pc):
    """True only for models whose opacity / scaling / rotation getters are exactly sigmoid / exp / normalize of `_opacity` /
    `_scaling` / `_rotation`: a SurfelModel with raw=True, or the reference's GaussianModel
    [REF scene/gaussian_model.py:63-75, 101-123].  NOT MaskGaussianModel: its getters activate `_x + _new_x * mask`
    [REF scene/mask_gaussian.py:140-176], so the raw tensors are not what it renders (and are frozen there); mask_model.MaskedSurfelModel
    serves that model and hands over what it renders through `raw_parameters()` (_offers_raw_parameters)."""
    if isinstance(pc, SurfelModel):
        return pc.raw
    return type(pc).__name__ == "GaussianModel" and getattr(pc, "fused_activations_ok", True)


def _offers_raw_parameters(pc):
    """A model whose getters are sigmoid / exp / normalize of something OTHER than `_opacity` / `_scaling` / `_rotation` says so with a
    `raw_parameters()` that returns those three pre-activation tensors with their graph (mask_model.MaskedSurfelModel: base + masked delta)."""
    return callable(getattr(pc, "raw_parameters", None))


def _fused_activations(pc, pipe):
    """Raw parameters go straight to the operator when asked for and when the model's getters are the plain activations of `_opacity` /
    `_scaling` / `_rotation` or of what its `raw_parameters()` returns; any other model (the reference's MaskGaussianModel, subclasses
    with extra terms) silently keeps the getter path."""
    if not getattr(pipe, "fused_activations", False) or pipe.compute_cov3D_python:
        return False
    return _offers_raw_parameters(pc) or (_plain_getters(pc) and all(hasattr(pc, a) for a in ("_opacity", "_scaling", "_rotation")))


def _raw_parameters(pc):
    return pc.raw_parameters() if _offers_raw_parameters(pc) else (pc._opacity, pc._scaling, pc._rotation)


def _geometry_inputs(pc, pipe, screenspace_points, mask, scaling_modifier):
    fused = _fused_activations(pc, pipe)
    raw_opacity, raw_scaling, raw_rotation = _raw_parameters(pc) if fused else (None, None, None)
    means3D, means2D = _sel(pc.get_xyz, mask), _sel(screenspace_points, mask)
    opacity = _sel(raw_opacity if fused else pc.get_opacity, mask)
    scales = rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = _sel(pc.get_covariance(scaling_modifier), mask)
    elif fused:
        scales, rotations = _sel(raw_scaling, mask), _sel(raw_rotation, mask)
    else:
        scales, rotations = _sel(pc.get_scaling, mask), _sel(pc.get_rotation, mask)
    try:
        means3D.retain_grad()
    except Exception:
        pass
    return means3D, means2D, opacity, scales, rotations, cov3D_precomp


def _color_inputs(viewpoint_camera, pc, pipe, mask, override_color):
    shs = colors_precomp = None
    if override_color is None:
        if pipe.convert_SHs_python:
            shs_view = pc.get_features.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = pc.get_xyz - viewpoint_camera.camera_center.repeat(pc.get_features.shape[0], 1)
            dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            sh2rgb = eval_sh(pc.active_sh_degree, shs_view, dir_pp_normalized)
            colors_precomp = _sel(torch.clamp_min(sh2rgb + 0.5, 0.0), mask)
        else:
            shs = _sel(pc.get_features, mask)
    else:
        colors_precomp = _sel(override_color, mask)
    return shs, colors_precomp


def _semantic_mask(pc, semantic_filter_bit, reverse_semantic):
    if semantic_filter_bit is None:
        return None
    assert reverse_semantic is not None
    m = (pc.get_semantics_32bit & int(semantic_filter_bit)) != 0
    return ~m if reverse_semantic is False else m


def _render_impl(viewpoint_camera, pc, pipe, bg_color, mask, scaling_modifier, override_color):
    kernel_mask = None
    if mask is not None and getattr(pipe, "fused_mask", False):
        kernel_mask, mask = mask, None   # the operator skips masked-out Gaussians itself: no gathered copies
    screenspace_points = _screenspace_points(pc)
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier),
                                    fused_activations=_fused_activations(pc, pipe))
    means3D, means2D, opacity, scales, rotations, cov3D_precomp = _geometry_inputs(pc, pipe, screenspace_points, mask, scaling_modifier)
    shs, colors_precomp = _color_inputs(viewpoint_camera, pc, pipe, mask, override_color)
    rendered_image, radii, allmap = rasterizer(means3D=means3D, means2D=means2D, shs=shs, colors_precomp=colors_precomp,
                                               opacities=opacity, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp,
                                               mask=kernel_mask)
    rets = {"render": rendered_image, "viewspace_points": means2D, "visibility_filter": radii > 0, "radii": radii}
    rets.update(postprocess_allmap(viewpoint_camera, pipe, allmap))
    return rets


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
           semantic_filter_bit: Optional[int] = None, reverse_semantic: Optional[bool] = None):
    """[REF gaussian_renderer/__init__.py:18-188]"""
    mask = _semantic_mask(pc, semantic_filter_bit, reverse_semantic)
    return _render_impl(viewpoint_camera, pc, pipe, bg_color, mask, scaling_modifier, override_color)


def render_with_mask(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, mask, scaling_modifier=1.0, override_color=None):
    """[REF gaussian_renderer/__init__.py:190-325]"""
    return _render_impl(viewpoint_camera, pc, pipe, bg_color, mask, scaling_modifier, override_color)


def _top2_margin(prob):
    """1 - (largest - second largest) over the class axis, and the argmax -- what the reference gets from `torch.topk(prob, k=2, dim=0)`
    and `torch.argmax` [REF gaussian_renderer/__init__.py:448-449, 586-587]; two `max` reductions give the same values (and gradients)
    and take 0.1 ms instead of topk's 5.4 ms on a [6,1080,1920] map."""
    top1, best = prob.max(dim=0)
    classes = torch.arange(prob.shape[0], device=prob.device).view(-1, 1, 1)
    top2 = prob.masked_fill(classes == best.unsqueeze(0), float("-inf")).max(dim=0).values
    return 1.0 - (top1 - top2), best


def _render_semantic_impl(viewpoint_camera, pc, pipe, mask, scaling_modifier):
    dev = pc.get_xyz.device
    kernel_mask = None
    if mask is not None and getattr(pipe, "fused_mask", False):
        kernel_mask, mask = mask, None
    screenspace_points = _screenspace_points(pc)
    n_cls = len(concerned_classes_list)
    bg_prob = [0.0] * n_cls
    bg_prob[concerned_classes_ind_map["sky"]] = 1.0
    means3D, means2D, opacity, scales, rotations, cov3D_precomp = _geometry_inputs(pc, pipe, screenspace_points, mask, scaling_modifier)
    semantics_tag = _sel(pc.get_semantics, mask)
    # The reference renders the 6 one-hot class channels as two 3-channel passes over identical geometry [REF :417-444];
    # here the operator blends 6 precomputed channels in ONE pass (preprocess, binning, sort and the
    # per-pixel alpha chain are shared), which gives bit-identical channel values.
    assert n_cls == 6, "the single-pass semantic render is built for the reference's 6 classes"
    bg = torch.tensor(bg_prob, dtype=torch.float32, device=dev)
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg, scaling_modifier),
                                    fused_activations=_fused_activations(pc, pipe))
    semantic_6 = (semantics_tag.view(-1, 1) == torch.arange(n_cls, device=dev).view(1, -1)).float()
    output_semantic, radii, allmap = rasterizer(means3D=means3D, means2D=means2D, shs=None, colors_precomp=semantic_6,
                                                opacities=opacity, scales=scales, rotations=rotations,
                                                cov3D_precomp=cov3D_precomp, mask=kernel_mask)
    uncertainty, best = _top2_margin(output_semantic)
    semantic_rgb = _SEMANTIC_COLOR.to(dev)[best].permute(2, 0, 1) / 255.0
    return {"render_semantics": output_semantic, "semantic_rgb": semantic_rgb, "semantic_uncertainty": uncertainty}


def render_and_semantic(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, mask=None):
    """`render()` and `render_semantic()` of the same view as ONE rasterization (extension; the reference's
    training iteration calls the two back to back on identical geometry [REF train.py:84-109]): the operator blends the SH colour
    and the six one-hot class channels together (9 channels).  Returns the union of the two result dicts; `render` is bit-identical
    to `render()`, `render_semantics` to `render_semantic()`."""
    assert not pipe.convert_SHs_python, "the 9-channel pass takes the SHs themselves"
    dev = pc.get_xyz.device
    kernel_mask = None
    if mask is not None and getattr(pipe, "fused_mask", False):
        kernel_mask, mask = mask, None
    screenspace_points = _screenspace_points(pc)
    n_cls = len(concerned_classes_list)
    assert n_cls == 6
    bg_prob = [0.0] * n_cls
    bg_prob[concerned_classes_ind_map["sky"]] = 1.0
    bg9 = torch.cat([bg_color.to(dev).float().reshape(3), torch.tensor(bg_prob, dtype=torch.float32, device=dev)])
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg9, scaling_modifier),
                                    fused_activations=_fused_activations(pc, pipe))
    means3D, means2D, opacity, scales, rotations, cov3D_precomp = _geometry_inputs(pc, pipe, screenspace_points, mask, scaling_modifier)
    semantic_6 = _one_hot_classes(pc.get_semantics, n_cls) if mask is None else \
        (pc.get_semantics[mask].view(-1, 1) == torch.arange(n_cls, device=dev).view(1, -1)).float()
    color9, radii, allmap = rasterizer(means3D=means3D, means2D=means2D, shs=_sel(pc.get_features, mask), opacities=opacity, scales=scales,
                                       rotations=rotations, cov3D_precomp=cov3D_precomp, mask=kernel_mask, extra_colors=semantic_6)
    rets = {"render": color9[:3], "viewspace_points": means2D, "visibility_filter": radii > 0, "radii": radii}
    rets.update(postprocess_allmap(viewpoint_camera, pipe, allmap))
    output_semantic = color9[3:]
    uncertainty, best = _top2_margin(output_semantic)
    rets.update({"render_semantics": output_semantic, "semantic_uncertainty": uncertainty,
                 "semantic_rgb": _SEMANTIC_COLOR.to(dev)[best].permute(2, 0, 1) / 255.0})
    return rets


def render_class_distortions(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, class_ids=None, scaling_modifier=1.0):
    """The per-class distortion maps of one view in ONE rasterization (extension).  The reference's training iteration
    obtains them with one full `render(..., semantic_filter_bit=1 << k, reverse_semantic=True)["rend_dist"]` per class
    [REF train.py:94-103]; here preprocess, sort and binning run once and the blend keeps one transmittance chain per class.
    `class_ids`: the classes wanted (default: every concerned class but the sky, as in the reference's loop).
    Returns {"rend_dist": [len(class_ids), 1, H, W], "viewspace_points", "visibility_filter", "radii"}; rend_dist[j] equals the
    reference call for class_ids[j]; gradients flow to xyz / opacity / scaling / rotation."""
    if class_ids is None:
        class_ids = [i for i, n in enumerate(concerned_classes_list) if n != "sky"]
    class_ids = [int(c) for c in class_ids]
    dev = pc.get_xyz.device
    screenspace_points = _screenspace_points(pc)
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier),
                                    fused_activations=_fused_activations(pc, pipe))
    means3D, means2D, opacity, scales, rotations, cov3D_precomp = _geometry_inputs(pc, pipe, screenspace_points, None, scaling_modifier)
    assert cov3D_precomp is None
    chain = _class_chain_ids(pc, class_ids, dev)
    dist, radii = rasterizer.class_distortions(means3D=means3D, means2D=means2D, opacities=opacity, scales=scales, rotations=rotations,
                                               classes=chain, n_classes=len(class_ids))
    return {"rend_dist": dist.unsqueeze(1), "viewspace_points": means2D, "visibility_filter": radii > 0, "radii": radii}


# Per-Gaussian class encodings derived from `pc.get_semantics` alone (the six one-hot channels, the class -> chain table look-up): a
# training loop asks for them every iteration while the semantics only change at densification.  The upstream model's getter returns
# `self._semantics.squeeze(-1)` -- a NEW view object on every call [REF scene/gaussian_model.py:126] -- so the cache is keyed on what is
# stable across views of one parameter: the storage's address, the tensor's in-place version, its shape / stride / offset / dtype.  (An
# `id()` + weak reference to the view -- round 5 -- never hit with the real model.)  One entry per kind of encoding: a densification step
# (new storage or a bumped version) replaces it, nothing stale stays alive (a [P,6] float one-hot is 72 MB at 3 M Gaussians).
# ~0.1 ms per call at 3 M Gaussians.
_SEM_CACHE = {}


def _semantics_key(sem: torch.Tensor):
    return (sem.untyped_storage().data_ptr(), sem._version, tuple(sem.shape), tuple(sem.stride()), sem.storage_offset(), sem.dtype, str(sem.device))


def _per_semantics(sem: torch.Tensor, key, make):
    kind = key[0]
    want = (_semantics_key(sem), key)
    hit = _SEM_CACHE.get(kind)
    if hit is not None and hit[0] == want:
        return hit[1]
    val = make()
    _SEM_CACHE[kind] = (want, val)   # at most one entry per kind
    return val


def _one_hot_classes(sem: torch.Tensor, n_cls: int) -> torch.Tensor:
    """[P] integer classes -> [P, n_cls] float one-hot (what render_semantic blends [REF gaussian_renderer/__init__.py:404-414])."""
    return _per_semantics(sem, ("one_hot", n_cls), lambda: (sem.view(-1, 1) == torch.arange(n_cls, device=sem.device).view(1, -1)).float())


def _class_chain_ids(pc, class_ids, dev):
    """class of a Gaussian -> its chain (position in class_ids), -1 = not rendered"""
    return _per_semantics(pc.get_semantics, ("chains", tuple(class_ids)), lambda: _class_chain_ids_uncached(pc, class_ids, dev))


def _class_chain_ids_uncached(pc, class_ids, dev):
    lut = torch.full((max(max(class_ids) + 1, len(concerned_classes_list)),), -1, dtype=torch.int32, device=dev)
    lut[torch.tensor(class_ids, device=dev)] = torch.arange(len(class_ids), dtype=torch.int32, device=dev)
    sem = pc.get_semantics.to(torch.int64).clamp(0, lut.numel() - 1)
    return torch.where((pc.get_semantics >= 0) & (pc.get_semantics < lut.numel()), lut[sem], torch.full_like(lut[sem], -1))


def render_train_view(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, class_ids=None, scaling_modifier=1.0):
    """Everything a late training iteration of the reference rasterizes for one view [REF train.py:84-109] -- `render()`,
    `render_semantic()` and the per-class `rend_dist` maps -- from ONE preprocess, ONE binning and ONE per-Gaussian backward
    (extension, SURVEY 8f N1 in full: `render_and_semantic` + `render_class_distortions` on a shared plan).  Returns the union of their
    dicts, with the per-class maps as `class_rend_dist` [len(class_ids), 1, H, W].  Maps bit-identical to the separate calls."""
    assert not pipe.convert_SHs_python, "the 9-channel pass takes the SHs themselves"
    if class_ids is None:
        class_ids = [i for i, n in enumerate(concerned_classes_list) if n != "sky"]
    class_ids = [int(c) for c in class_ids]
    dev = pc.get_xyz.device
    screenspace_points = _screenspace_points(pc)
    n_cls = len(concerned_classes_list)
    assert n_cls == 6
    bg_prob = [0.0] * n_cls
    bg_prob[concerned_classes_ind_map["sky"]] = 1.0
    bg9 = torch.cat([bg_color.to(dev).float().reshape(3), torch.tensor(bg_prob, dtype=torch.float32, device=dev)])
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg9, scaling_modifier),
                                    fused_activations=_fused_activations(pc, pipe))
    means3D, means2D, opacity, scales, rotations, cov3D_precomp = _geometry_inputs(pc, pipe, screenspace_points, None, scaling_modifier)
    assert cov3D_precomp is None
    semantic_6 = _one_hot_classes(pc.get_semantics, n_cls)
    color9, radii, allmap, dist = rasterizer.forward_with_class_distortions(
        means3D=means3D, means2D=means2D, opacities=opacity, scales=scales, rotations=rotations, classes=_class_chain_ids(pc, class_ids, dev),
        n_classes=len(class_ids), shs=pc.get_features, extra_colors=semantic_6)
    rets = {"render": color9[:3], "viewspace_points": means2D, "visibility_filter": radii > 0, "radii": radii}
    rets.update(postprocess_allmap(viewpoint_camera, pipe, allmap))
    output_semantic = color9[3:]
    uncertainty, best = _top2_margin(output_semantic)
    rets.update({"render_semantics": output_semantic, "semantic_uncertainty": uncertainty,
                 "semantic_rgb": _SEMANTIC_COLOR.to(dev)[best].permute(2, 0, 1) / 255.0, "class_rend_dist": dist.unsqueeze(1)})
    return rets


def render_semantic(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0,
                    semantic_filter_bit: Optional[int] = None, reverse_semantic: Optional[bool] = None):
    """[REF gaussian_renderer/__init__.py:327-460] (bg_color is accepted and, as in the reference, unused)."""
    return _render_semantic_impl(viewpoint_camera, pc, pipe, _semantic_mask(pc, semantic_filter_bit, reverse_semantic), scaling_modifier)


def render_semantic_with_mask(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, mask, scaling_modifier=1.0):
    """[REF gaussian_renderer/__init__.py:462-598].  Unlike render_semantic, the reference returns `semantic_uncertainty` with a
    leading unit axis here ([1,H,W], REF :588 `(1. - difference)[None, ...]` vs :450) -- kept."""
    out = _render_semantic_impl(viewpoint_camera, pc, pipe, mask, scaling_modifier)
    out["semantic_uncertainty"] = out["semantic_uncertainty"][None, ...]
    return out

"""The masked re-optimisation model of the unveiling stage [REF scene/mask_gaussian.py; inpainting_pipeline/3_reoptimization/
1_optimization.py]: after an object is removed the scene is re-optimised around the hole on a model that FREEZES the six parameter tensors
and trains six zero-initialised deltas `_new_*`; every getter returns `base + delta * mask[row]`, `get_features` also concatenates the two
SH parts.  Here (csrc/mask_model.hip, csrc/optimizer.hip):

    compose_masked         the five effective raw tensors of all six properties in ONE kernel launch, their backward in one more
    compose_masked_torch   the reference's getter lines in the reference's order on plain tensors: the checker and the timing baseline
    MaskedSurfelModel      shaped like the reference's MaskGaussianModel; the getters of one iteration share one compose, the optimizer is
                           a SurfelAdam that steps only the rows the mask selects

Two deliberate differences from the reference's arithmetic: a non-finite delta in a masked-out row does not reach the output (the
reference's `NaN * 0` yields NaN there), and a zero may differ in sign (`-0.0 + 0.0` is `+0.0`; the reference adds `delta * 0`, which is
`-0.0` for a negative delta).  Everything else is the same single float32 add, bit for bit."""
from __future__ import annotations

import math
from collections import namedtuple

import torch
from torch import nn

from . import _lib as L
from ._call import call, ptr
from .optim import SurfelAdam, row_mask_bytes

# the six tensors, in the order of the reference's training_setup (the order of `base` / `delta` everywhere in this module)
PROPERTIES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
# [REF scene/mask_gaussian.py:29-30]: the bit order of `mask_property_bit`
MASK_PROPERTY = ["xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"]
MASK_PROPERTY_BIT = {name: 1 << idx for idx, name in enumerate(MASK_PROPERTY)}
_BITS = tuple(MASK_PROPERTY_BIT[name] for name in PROPERTIES)
_UPSTREAM_OF = (0, 1, 1, 2, 3, 4)      # property -> the effective tensor it lands in

Effective = namedtuple("Effective", ["xyz", "features", "opacity", "scaling", "rotation"])


def fixed_bits(fixed) -> int:
    """`fixed` as the reference's `mask_property_bit`: an int is taken as it is, otherwise an iterable of MASK_PROPERTY names."""
    if isinstance(fixed, int):
        bits = fixed
    else:
        bits = 0
        for name in fixed:
            if name not in MASK_PROPERTY_BIT:
                raise ValueError(f"unknown property {name!r}: one of {MASK_PROPERTY}")
            bits |= MASK_PROPERTY_BIT[name]
    if not 0 <= bits < 64:
        raise ValueError(f"fixed = {bits}: bits beyond the six properties")
    return bits


def _six(tensors, what):
    if isinstance(tensors, dict):
        tensors = [tensors[name] for name in PROPERTIES]
    tensors = list(tensors)
    if len(tensors) != 6:
        raise ValueError(f"{what} must hold the six tensors {PROPERTIES}; got {len(tensors)}")
    return tensors


def _row_shapes(P, M):
    return [(P, 3), (P, 1, 3), (P, M - 1, 3), (P, 1), (P, 2), (P, 4)]


def _check(base, delta, mask):
    """-> (P, M); shapes, dtypes and devices of the twelve tensors and the mask."""
    xyz, dc = base[0], base[1]
    if xyz.dim() != 2 or base[2].dim() != 3:
        raise ValueError(f"base xyz must be [P,3] and features_rest [P,M-1,3]; got {tuple(xyz.shape)} and {tuple(base[2].shape)}")
    P, M = xyz.shape[0], base[2].shape[1] + 1
    for group, tensors in (("base", base), ("delta", delta)):
        for name, t, shape in zip(PROPERTIES, tensors, _row_shapes(P, M)):
            if tuple(t.shape) != shape:
                raise ValueError(f"{group} {name} must be {list(shape)}; got {list(t.shape)}")
            if t.dtype != dc.dtype or t.device != dc.device:
                raise ValueError(f"{group} {name} is {t.dtype} on {t.device}; the others are {dc.dtype} on {dc.device}")
    if mask.shape != (P,):
        raise ValueError(f"mask must be [{P}]; got {list(mask.shape)}")
    if mask.device != dc.device:
        raise ValueError(f"mask is on {mask.device}, the tensors on {dc.device}")
    return P, M


def compose_masked_torch(base, delta, mask, fixed=()):
    """The reference's getter lines before their activations [REF scene/mask_gaussian.py:139-176], in its order, on plain tensors of any
    device and float dtype: `base + delta * mask[..., None]` per property, a fixed property its base, the two SH parts concatenated.
    `mask`: bool or 0 / 1 float, as the reference multiplies by it.  -> Effective(xyz, features, opacity, scaling, rotation)"""
    base, delta = _six(base, "base"), _six(delta, "delta")
    bits = fixed_bits(fixed)
    _check(base, delta, mask)
    _xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation = base
    _new_xyz, _new_features_dc, _new_features_rest, _new_opacity, _new_scaling, _new_rotation = delta
    fixed_ = lambda name: bits & MASK_PROPERTY_BIT[name] != 0
    scaling = _scaling if fixed_("scaling") else _scaling + _new_scaling * mask[..., None]
    rotation = _rotation if fixed_("rotation") else _rotation + _new_rotation * mask[..., None]
    xyz = _xyz if fixed_("xyz") else _xyz + _new_xyz * mask[..., None]
    features_dc = _features_dc if fixed_("features_dc") else _features_dc + _new_features_dc * mask[..., None, None]
    features_rest = _features_rest if fixed_("features_rest") else _features_rest + _new_features_rest * mask[..., None, None]
    features = torch.cat((features_dc, features_rest), dim=1)
    opacity = _opacity if fixed_("opacity") else _opacity + _new_opacity * mask[..., None]
    return Effective(xyz, features, opacity, scaling, rotation)


# ---- the two kernel calls --------------------------------------------------------------------------------------------------------------
def _need_gpu(t, what):
    if t.dtype != torch.float32:
        raise ValueError(f"{what} needs float32 tensors; got {t.dtype} (compose_masked_torch takes any float dtype)")
    if not t.is_cuda:
        raise L.SurfelRasterError(f"{what} needs CUDA (ROCm) tensors; there is no CPU path (compose_masked_torch is the checker)")


def _compose_forward(base, delta, mask_u8, bits):
    """sr_mask_compose on contiguous tensors -> [xyz, features, opacity, scaling, rotation]; None where the property is fixed and the
    caller uses the base tensor itself (features are always written: they are a concatenation)."""
    _need_gpu(base[0], "compose_masked")
    P, M = base[0].shape[0], base[2].shape[1] + 1
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=base[0].device)
    out = [None if bits & MASK_PROPERTY_BIT["xyz"] else new(P, 3), new(P, M, 3), None if bits & MASK_PROPERTY_BIT["opacity"] else new(P, 1),
           None if bits & MASK_PROPERTY_BIT["scaling"] else new(P, 2), None if bits & MASK_PROPERTY_BIT["rotation"] else new(P, 4)]
    call("sr_mask_compose", base[0].device, P, M, L.SrMaskTensors(*map(ptr, base)), L.SrMaskTensors(*map(ptr, delta)), ptr(mask_u8), bits,
         L.SrMaskEffective(*map(ptr, out)))
    return out


def _compose_backward(upstream, mask_u8, bits, P, M, wanted):
    """sr_mask_compose_backward: `upstream` = the contiguous gradients of the five effective tensors (None: none), `wanted[k]`: the
    gradient of delta k is asked for -> the six delta gradients, None where not wanted."""
    dev = mask_u8.device
    d = [torch.empty(shape, dtype=torch.float32, device=dev) if want else None for shape, want in zip(_row_shapes(P, M), wanted)]
    if any(wanted):
        _need_gpu(next(g for g in upstream if g is not None), "compose_masked")
        call("sr_mask_compose_backward", dev, P, M, L.SrMaskEffective(*map(ptr, upstream)), ptr(mask_u8), bits, L.SrMaskTensors(*map(ptr, d)))
    return d


class _ComposeMasked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask_u8, bits, on_backward, *tensors):
        base, delta = [t.contiguous() for t in tensors[:6]], [t.contiguous() for t in tensors[6:]]
        out = _compose_forward(base, delta, mask_u8, bits)
        ctx.save_for_backward(mask_u8)      # (a bool mask is a view of the caller's: autograd raises if it is edited before the backward)
        ctx.bits, ctx.on_backward = bits, on_backward
        ctx.P, ctx.M = base[0].shape[0], base[2].shape[1] + 1
        ctx.set_materialize_grads(False)
        placeholders = [base[0].new_empty(0) if o is None else None for o in out]     # a fixed property: the caller takes the base tensor
        ctx.mark_non_differentiable(*[p for p in placeholders if p is not None])
        return tuple(p if o is None else o for o, p in zip(out, placeholders))

    @staticmethod
    def backward(ctx, *upstream):
        if ctx.on_backward is not None:
            ctx.on_backward()
        upstream = [None if g is None else g.contiguous() for g in upstream]
        wanted = [ctx.needs_input_grad[3 + 6 + k] and not ctx.bits & _BITS[k] and upstream[_UPSTREAM_OF[k]] is not None for k in range(6)]
        d = _compose_backward(upstream, ctx.saved_tensors[0], ctx.bits, ctx.P, ctx.M, wanted)
        return (None, None, None) + (None,) * 6 + tuple(d)      # the base is frozen in this model: no gradient for it


def compose_masked(base, delta, mask, fixed=(), _on_backward=None):
    """The effective raw (pre-activation) tensors of the masked model in one HIP kernel launch, differentiable in `delta` (one more
    launch): row i of every property is `base[i] + delta[i]` where `mask[i]` is set and `base[i] + 0.0` elsewhere; a property named in
    `fixed` (MASK_PROPERTY names, or the reference's `mask_property_bit`) is its base tensor itself.
    `base`, `delta`: the six float32 tensors in the order of PROPERTIES (or dicts by those names) on one GPU; `mask`: bool [P], or a
    float tensor taken as `!= 0`.  The base gets no gradient (the model freezes it).  Delta and upstream-gradient rows of masked-out
    Gaussians are never read.  -> Effective(xyz [P,3], features [P,M,3], opacity [P,1], scaling [P,2], rotation [P,4])"""
    base, delta = _six(base, "base"), _six(delta, "delta")
    bits = fixed_bits(fixed)
    _check(base, delta, mask)
    out = _ComposeMasked.apply(row_mask_bytes(mask), bits, _on_backward, *base, *delta)
    own = (base[0], None, base[3], base[4], base[5])
    return Effective(*[own[k] if own[k] is not None and bits & MASK_PROPERTY_BIT[name] else out[k]
                       for k, name in enumerate(("xyz", "features", "opacity", "scaling", "rotation"))])


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """The reference's position learning-rate schedule [REF utils/general_utils.py:29-62]: log-linear from lr_init at step 0 to lr_final
    at max_steps, times a sine ease-in from lr_delay_mult over the first lr_delay_steps."""
    def rate(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay = 1.0
        if lr_delay_steps > 0:
            delay = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
    return rate


class MaskedSurfelModel:
    """The reference's MaskGaussianModel [REF scene/mask_gaussian.py] on the fused kernels: the same attributes (`_xyz` ... `_opacity`
    frozen, `_new_xyz` ... `_new_opacity` trainable, `mask`, `mask_property_bit`, `optimizer`, `xyz_gradient_accum`, `denom`,
    `max_radii2D`, `_semantics`), the same getters and the same methods as far as the re-optimisation stage calls them (`refine()` calls
    none of `densify_*` / `reset_opacity*`, which are not here; `get_covariance` raises as SurfelModel's does: `compute_cov3D_python`
    cannot run on 2-component scales).  `mask` is held as bool (set_mask).

    The five getters of one iteration share ONE compose launch: the result is cached under the in-place versions of the deltas and the
    mask, the tensors' identities, `mask_property_bit` and the grad mode, and dropped when a backward has passed through it.  The
    optimizer's step moves the deltas' versions (optim.adam_step bumps them, as a torch in-place operation would), so a render after a
    step recomputes also where no backward lies between, under `no_grad` for instance.  Writing a delta through its raw pointer by any
    other route does not, and needs a `_drop_cache()`.
    `raw_parameters()` hands `gaussian_renderer.render` the raw opacity / scaling / rotation for `pipe.fused_activations`.
    The optimizer is a SurfelAdam with `row_mask=` this model's mask: masked-out rows have zero gradients and zero moments from
    `training_setup` on (`set_mask` precedes it, `reset_mask` builds a new optimizer), so skipping them equals the dense step.
    Tensors stay on the device of the model they come from (the reference moves everything to "cuda")."""

    def __init__(self, sh_degree: int):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        e = torch.empty(0)
        self._xyz = self._features_dc = self._features_rest = self._scaling = self._rotation = self._opacity = self._semantics = e
        self.max_radii2D = self.xyz_gradient_accum = self.denom = e
        self._new_xyz = self._new_features_dc = self._new_features_rest = self._new_scaling = self._new_rotation = self._new_opacity = e
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.mask = e
        self.mask_property_bit = 0
        self._cache = None

    # -- fixed properties [REF :78-100, 620-636]
    def _fixed(self, name):
        return MASK_PROPERTY_BIT[name] & self.mask_property_bit != 0

    def _set_fixed(self, name):
        self.mask_property_bit = self.mask_property_bit | MASK_PROPERTY_BIT[name]

    check_fixed_xyz = property(lambda s: s._fixed("xyz"))
    check_fixed_features_dc = property(lambda s: s._fixed("features_dc"))
    check_fixed_features_rest = property(lambda s: s._fixed("features_rest"))
    check_fixed_scaling = property(lambda s: s._fixed("scaling"))
    check_fixed_rotation = property(lambda s: s._fixed("rotation"))
    check_fixed_opacity = property(lambda s: s._fixed("opacity"))

    def set_fixed_xyz(self): self._set_fixed("xyz")
    def set_fixed_features_dc(self): self._set_fixed("features_dc")
    def set_fixed_features_rest(self): self._set_fixed("features_rest")
    def set_fixed_scaling(self): self._set_fixed("scaling")
    def set_fixed_rotation(self): self._set_fixed("rotation")
    def set_fixed_opacity(self): self._set_fixed("opacity")

    # -- set-up [REF :102-132, 238-249]
    def _base(self):
        return [self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation]

    def _delta(self):
        return [self._new_xyz, self._new_features_dc, self._new_features_rest, self._new_opacity, self._new_scaling, self._new_rotation]

    def from_gaussian_model(self, gaussians):
        take = lambda t: t.detach().clone().contiguous()
        self._xyz, self._features_dc, self._features_rest = take(gaussians._xyz), take(gaussians._features_dc), take(gaussians._features_rest)
        self._opacity, self._scaling, self._rotation = take(gaussians._opacity), take(gaussians._scaling), take(gaussians._rotation)
        self._semantics = gaussians._semantics
        self.max_radii2D = gaussians.max_radii2D
        self.active_sh_degree = gaussians.active_sh_degree
        self.spatial_lr_scale = gaussians.spatial_lr_scale
        self.set_nograd()
        return self

    def set_nograd(self):
        for t in self._base():
            t.requires_grad = False
        zeros = lambda t: nn.Parameter(torch.zeros_like(t).requires_grad_(True))
        self._new_xyz, self._new_features_dc, self._new_features_rest = zeros(self._xyz), zeros(self._features_dc), zeros(self._features_rest)
        self._new_scaling, self._new_rotation, self._new_opacity = zeros(self._scaling), zeros(self._rotation), zeros(self._opacity)
        self.set_mask(torch.ones(self.points_number, dtype=torch.bool, device=self._xyz.device))

    def set_mask(self, update_mask):
        """`mask` is kept as bool: a float 0 / 1 mask (the reference's set_nograd builds one) is taken as `!= 0` here, once, not at every
        compose and every optimizer step."""
        update_mask = update_mask.to(self._xyz.device)
        self.mask = update_mask if update_mask.dtype == torch.bool else update_mask != 0

    def reset_mask(self, update_mask, opt):
        """Fold the trained deltas into the base (one compose, no graph), take the new mask, zero the deltas and renew the optimizer.
        The new mask STAYS: the reference's reset_mask ends in set_nograd, whose last line replaces the mask it was just given by all
        ones [REF :129-131, 117] (its pipeline never calls reset_mask)."""
        with torch.no_grad():                # a fixed xyz stays unfolded (the reference folds `get_xyz`); every other property is
            eff = self._compose(self.mask_property_bit & MASK_PROPERTY_BIT["xyz"])      # folded, whatever is fixed [REF :123-128]
        self._xyz, self._opacity, self._scaling, self._rotation = eff.xyz, eff.opacity, eff.scaling, eff.rotation
        self._features_dc, self._features_rest = eff.features[:, :1].contiguous(), eff.features[:, 1:].contiguous()
        self.set_nograd()
        self.set_mask(update_mask)
        self.training_setup(opt)

    @property
    def points_number(self):
        return self._xyz.shape[0]

    # -- the getters: one compose per iteration
    def _compose(self, bits):
        return compose_masked(self._base(), self._delta(), self.mask, bits, _on_backward=self._drop_cache)

    def _drop_cache(self):
        self._cache = None

    def _effective(self):
        tensors = self._base() + self._delta() + [self.mask]
        key = (tuple(id(t) for t in tensors), tuple(t._version for t in tensors), self.mask_property_bit, torch.is_grad_enabled())
        if self._cache is None or self._cache[0] != key:
            self._cache = (key, self._compose(self.mask_property_bit), tensors)     # (the tensors: their ids stay theirs while cached)
        return self._cache[1]

    def raw_parameters(self):
        """(opacity, scaling, rotation) before their activations, with their graph: what `pipe.fused_activations` hands the rasterizer."""
        eff = self._effective()
        return eff.opacity, eff.scaling, eff.rotation

    get_xyz = property(lambda s: s._effective().xyz)
    get_features = property(lambda s: s._effective().features)
    get_opacity = property(lambda s: torch.sigmoid(s._effective().opacity))
    get_scaling = property(lambda s: torch.exp(s._effective().scaling))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s._effective().rotation))
    get_semantics = property(lambda s: s._semantics.squeeze(-1))
    get_semantics_32bit = property(lambda s: (1 << s._semantics.to(torch.int32)).squeeze(-1))

    def get_covariance(self, scaling_modifier=1):
        # as SurfelModel.get_covariance: the reference's producer [REF :187-189] indexes a third scale component
        raise NotImplementedError("compute_cov3D_python is a dead flag for 2D surfels (2-component scales)")

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # -- optimizer [REF :195-221]
    def training_setup(self, training_args):
        self.percent_dense = training_args.percent_dense
        P, dev = self.points_number, self._xyz.device
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        l = [
            {"params": [self._new_xyz], "lr": training_args.position_lr_init * self.spatial_lr_scale, "name": "new_xyz"},
            {"params": [self._new_features_dc], "lr": training_args.feature_lr, "name": "new_f_dc"},
            {"params": [self._new_features_rest], "lr": training_args.feature_lr / 20.0, "name": "new_f_rest"},
            {"params": [self._new_opacity], "lr": training_args.opacity_lr, "name": "new_opacity"},
            {"params": [self._new_scaling], "lr": training_args.scaling_lr, "name": "new_scaling"},
            {"params": [self._new_rotation], "lr": training_args.rotation_lr, "name": "new_rotation"},
        ]
        self.optimizer = SurfelAdam(l, lr=0.0, eps=1e-15, row_mask=lambda: self.mask)
        self.xyz_scheduler_args = expon_lr_func(lr_init=training_args.position_lr_init * self.spatial_lr_scale,
                                                lr_final=training_args.position_lr_final * self.spatial_lr_scale,
                                                lr_delay_mult=training_args.position_lr_delay_mult,
                                                max_steps=training_args.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        for param_group in self.optimizer.param_groups:
            if param_group["name"] == "new_xyz":
                lr = self.xyz_scheduler_args(iteration)
                param_group["lr"] = lr
                return lr

    # -- pruning [REF :315-331, 379-422]: once per stage, plain torch
    def _prune_optimizer(self, mask):
        optimizable_tensors = {}
        for group in self.optimizer.param_groups:
            stored_state = self.optimizer.state.get(group["params"][0], None)
            if stored_state is not None:
                stored_state["exp_avg"] = stored_state["exp_avg"][mask]
                stored_state["exp_avg_sq"] = stored_state["exp_avg_sq"][mask]
                del self.optimizer.state[group["params"][0]]
                group["params"][0] = nn.Parameter(group["params"][0][mask].requires_grad_(True))
                self.optimizer.state[group["params"][0]] = stored_state
            else:
                group["params"][0] = nn.Parameter(group["params"][0][mask].requires_grad_(True))
            optimizable_tensors[group["name"]] = group["params"][0]
        return optimizable_tensors

    def prune_points_with_mask(self, prune_mask):
        valid_points_mask = ~prune_mask
        if self.optimizer is not None:
            t = self._prune_optimizer(valid_points_mask)
            self._new_xyz, self._new_features_dc, self._new_features_rest = t["new_xyz"], t["new_f_dc"], t["new_f_rest"]
            self._new_opacity, self._new_scaling, self._new_rotation = t["new_opacity"], t["new_scaling"], t["new_rotation"]
        else:
            keep = lambda t: nn.Parameter(t.detach()[valid_points_mask].requires_grad_(True))
            self._new_xyz, self._new_features_dc, self._new_features_rest = keep(self._new_xyz), keep(self._new_features_dc), keep(self._new_features_rest)
            self._new_opacity, self._new_scaling, self._new_rotation = keep(self._new_opacity), keep(self._new_scaling), keep(self._new_rotation)
        self._xyz, self._features_dc, self._features_rest = self._xyz[valid_points_mask], self._features_dc[valid_points_mask], self._features_rest[valid_points_mask]
        self._opacity, self._scaling, self._rotation = self._opacity[valid_points_mask], self._scaling[valid_points_mask], self._rotation[valid_points_mask]
        self._semantics = self._semantics[valid_points_mask]
        self.mask = self.mask[valid_points_mask]
        for name in ("xyz_gradient_accum", "denom", "max_radii2D", "next_editable_pcd_mask", "already_in_frame_mask"):
            t = getattr(self, name, None)
            if t is not None and t.shape[0] != 0:
                setattr(self, name, t[valid_points_mask])
        return prune_mask

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        """[REF :614-618]: the statistics of the trainable Gaussians only (and, as there, of the first two gradient components)."""
        update_filter = (self.mask != 0) & update_filter
        self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1, keepdim=True)
        self.denom[update_filter] += 1

    def save_ply(self, path):
        """[REF :251-270]: every property folded, whatever is fixed."""
        from .ply import save_ply
        with torch.no_grad():
            eff = self._compose(0)
        n = lambda t: t.detach().cpu().numpy()
        save_ply(path, n(eff.xyz), n(eff.features[:, :1]), n(eff.features[:, 1:]), n(eff.opacity), n(eff.scaling), n(eff.rotation),
                 n(self._semantics).astype("int32"))

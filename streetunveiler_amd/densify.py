"""Densify-and-prune of the Gaussians and their Adam state as HIP kernels (csrc/densify.hip) [REF scene/gaussian_model.py:402-553;
train.py:171-191]:

    densify_and_prune_torch     the reference's lines in the reference's order on plain tensors of any device and float dtype: in float64
                                the checker, in float32 on the GPU the timing baseline
    densify_and_prune_tensors   the same result from one decision pass, one scan and one gather per parameter with its two moments
    densify_and_prune           `GaussianModel.densify_and_prune` on anything shaped like the reference's model
    prune_points                `GaussianModel.prune_points`, through the same pair of calls

What the reference computes, and so what all of these compute -- not what one might expect: `densification_postfix` sets
`max_radii2D` to zeros BEFORE the prune test reads it, so `max_radii2D > max_screen_size` never holds there.  A `max_screen_size` that
is not None (nor 0) only switches the world-size test `max(exp(_scaling)) > 0.1 * extent` on.  `max_radii2D` is an argument so that
the restatement can read it exactly where the reference does; no result depends on its values.

The rows come out as: the surviving originals that were not split in index order, the surviving clones, the surviving first children,
the surviving second children.  New rows have zero moments, the three statistics come back as zeros of the new size (prune_points
gathers them instead, as the reference does), every `step` counter stays.  There is no CPU path, and `torch.cuda.empty_cache()` is not
called."""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import torch
from torch import nn

from . import _lib as L
from ._call import buf, call, ptr, workspace

GROUP_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")      # the reference's training_setup
_ATTRIBUTE = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
              "rotation": "_rotation"}
_TAIL = {"xyz": (3,), "opacity": (1,), "scaling": (2,), "rotation": (4,)}     # f_dc and f_rest: any [P, ...]
_ROLE = {"xyz": L.SR_DENSIFY_ROLE_XYZ, "scaling": L.SR_DENSIFY_ROLE_SCALING}
FLAG_CLONE, FLAG_SPLIT, FLAG_KEEP_SELF, FLAG_KEEP_CHILD = (L.SR_DENSIFY_FLAG_CLONE, L.SR_DENSIFY_FLAG_SPLIT, L.SR_DENSIFY_FLAG_KEEP_SELF,
                                                           L.SR_DENSIFY_FLAG_KEEP_CHILD)
KIND_ORIGINAL, KIND_CLONE, KIND_CHILD0, KIND_CHILD1 = 0, 1, 2, 3

Densified = namedtuple("Densified", "params moments semantics extra_rows xyz_gradient_accum denom max_radii2D counts flags source kind")
Densified.__doc__ = """params {name: tensor}, moments {name: (exp_avg, exp_avg_sq) or None}, semantics, extra_rows (a tuple), the three
statistics, counts = (kept originals K, kept clones C, split-selected S, kept child pairs H), flags uint8 [P] (FLAG_* bits per input
row), and per output row its source index (int64) and kind (KIND_*)."""


def _build_rotation(r):
    """[REF utils/general_utils.py:78-99] on r's device and dtype."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device, dtype=r.dtype)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def densify_and_prune_torch(params, moments, semantics, xyz_gradient_accum, denom, max_radii2D, max_grad, min_opacity, extent,
                            max_screen_size, percent_dense, noise, extra_rows=(), bookkeeping=True):
    """The reference's `densify_and_prune` (with densify_and_clone, densify_and_split, densification_postfix, cat_tensors_to_optimizer,
    _prune_optimizer and prune_points), line by line and in its order, on plain tensors: `params` {name: [P, ...]} with the reference's
    group names, `moments` {name: (exp_avg, exp_avg_sq) or None} (None: no optimizer state yet), `semantics` [P,1], the three statistics,
    `extra_rows`: further per-Gaussian tensors (`cluster_idx`) that follow their rows like `semantics`.  The inputs are not changed.

    `noise` [2 S, 2] holds the standard normals of the split, S = the number of split-selected Gaussians: child k of the j-th of them
    reads row k S + j, so that `samples = stds * noise` has the layout of the reference's `stds.repeat(N, 1)`.

    As in the reference the statistics are zeroed by densification_postfix before the prune test reads `max_radii2D` (module
    docstring): `max_radii2D > max_screen_size` never holds, `max_screen_size` only switches the world-size test on.  -> Densified.

    `bookkeeping=False` leaves out what the reference does not do -- the source index and kind carried with every row, the flag byte
    and the counts, which cost two more tensors through every cat and prune and four host read-backs: `counts`, `flags`, `source` and
    `kind` are then None.  That is the form a timing baseline runs."""
    N = 2
    p = {k: v.detach() for k, v in params.items()}
    m = {k: (None if moments.get(k) is None else tuple(t.detach() for t in moments[k])) for k in p}
    dev, dtype = p["xyz"].device, p["xyz"].dtype
    P = p["xyz"].shape[0]
    riders = [semantics] + list(extra_rows)      # rows that ride along
    # the book-keeping of this restatement, not of the reference: source index and kind of every row
    book = [torch.arange(P, device=dev), torch.zeros(P, dtype=torch.int64, device=dev)] if bookkeeping else []
    stats = {}
    get_scaling = lambda: torch.exp(p["scaling"])
    get_opacity = lambda: torch.sigmoid(p["opacity"])

    def cat_tensors_to_optimizer(new):
        for k in p:
            if m[k] is not None:
                m[k] = tuple(torch.cat((s, torch.zeros_like(new[k])), dim=0) for s in m[k])
            p[k] = torch.cat((p[k], new[k]), dim=0)

    def densification_postfix(new, new_riders, new_book):
        cat_tensors_to_optimizer(new)
        riders[:] = [torch.cat([a, b], dim=0) for a, b in zip(riders, new_riders)]
        book[:] = [torch.cat([a, b], dim=0) for a, b in zip(book, new_book)]
        n = p["xyz"].shape[0]
        stats["xyz_gradient_accum"] = torch.zeros((n, 1), device=dev, dtype=dtype)
        stats["denom"] = torch.zeros((n, 1), device=dev, dtype=dtype)
        stats["max_radii2D"] = torch.zeros((n,), device=dev, dtype=dtype)

    def prune_points(mask):
        valid_points_mask = ~mask
        for k in p:
            if m[k] is not None:
                m[k] = tuple(s[valid_points_mask] for s in m[k])
            p[k] = p[k][valid_points_mask]
        riders[:] = [t[valid_points_mask] for t in riders]
        book[:] = [t[valid_points_mask] for t in book]
        for k in stats:
            stats[k] = stats[k][valid_points_mask]

    # densify_and_prune
    grads = xyz_gradient_accum.reshape(-1, 1) / denom.reshape(-1, 1)
    grads[grads.isnan()] = 0.0
    flags = torch.zeros(P, dtype=torch.uint8, device=dev) if bookkeeping else None
    kinds = lambda mask, *kind: [torch.cat([book[0][mask]] * len(kind)), torch.cat([torch.full((int(mask.sum()),), k, dtype=torch.int64, device=dev)
                                                                                       for k in kind])] if bookkeeping else []

    # densify_and_clone
    selected_pts_mask = torch.where(torch.norm(grads, dim=-1) >= max_grad, True, False)
    selected_pts_mask = torch.logical_and(selected_pts_mask, torch.max(get_scaling(), dim=1).values <= percent_dense * extent)
    if bookkeeping:
        flags[selected_pts_mask] |= FLAG_CLONE
    densification_postfix({k: v[selected_pts_mask] for k, v in p.items()}, [t[selected_pts_mask] for t in riders], kinds(selected_pts_mask, KIND_CLONE))

    # densify_and_split
    n_init_points = p["xyz"].shape[0]
    padded_grad = torch.zeros((n_init_points,), device=dev, dtype=dtype)
    padded_grad[:grads.shape[0]] = grads.squeeze(-1)
    selected_pts_mask = torch.where(padded_grad >= max_grad, True, False)
    selected_pts_mask = torch.logical_and(selected_pts_mask, torch.max(get_scaling(), dim=1).values > percent_dense * extent)
    if bookkeeping:
        flags[selected_pts_mask[:P]] |= FLAG_SPLIT
    S = int(selected_pts_mask.sum())      # (the reference reads this sum back too, for its prune_filter)
    if tuple(noise.shape) != (N * S, 2):
        raise ValueError(f"noise must be [{N * S},2] for {S} split-selected Gaussians; got {tuple(noise.shape)}")
    stds = get_scaling()[selected_pts_mask].repeat(N, 1)
    stds = torch.cat([stds, 0 * torch.ones_like(stds[:, :1])], dim=-1)
    samples = stds * torch.cat([noise.to(dtype), torch.zeros_like(stds[:, :1])], dim=-1)      # torch.normal(mean=0, std=stds) given its normals
    rots = _build_rotation(p["rotation"][selected_pts_mask]).repeat(N, 1, 1)
    new = {k: v[selected_pts_mask].repeat(N, *([1] * (v.dim() - 1))) for k, v in p.items()}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + p["xyz"][selected_pts_mask].repeat(N, 1)
    new["scaling"] = torch.log(get_scaling()[selected_pts_mask].repeat(N, 1) / (0.8 * N))
    new_riders = [t[selected_pts_mask].repeat(N, *([1] * (t.dim() - 1))) for t in riders]
    densification_postfix(new, new_riders, kinds(selected_pts_mask, KIND_CHILD0, KIND_CHILD1))
    prune_filter = torch.cat((selected_pts_mask, torch.zeros(N * S, device=dev, dtype=torch.bool)))
    prune_points(prune_filter)

    prune_mask = (get_opacity() < min_opacity).squeeze(-1)
    if max_screen_size:
        big_points_vs = stats["max_radii2D"] > max_screen_size
        big_points_ws = get_scaling().max(dim=1).values > 0.1 * extent
        prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws)
    prune_points(prune_mask)

    counts = source = kind = None
    if bookkeeping:
        source, kind = book
        flags[source[kind == KIND_ORIGINAL]] |= FLAG_KEEP_SELF
        flags[source[kind == KIND_CHILD0]] |= FLAG_KEEP_CHILD
        counts = (int((kind == KIND_ORIGINAL).sum()), int((kind == KIND_CLONE).sum()), S, int((kind == KIND_CHILD0).sum()))
    return Densified(p, m, riders[0], tuple(riders[1:]), stats["xyz_gradient_accum"], stats["denom"], stats["max_radii2D"], counts, flags, source, kind)


# ---- the op --------------------------------------------------------------------------------------------------------------------------
def _check_rows(name, t, P, float32=False, tail=None):
    """dtype, shape and contiguity of one per-Gaussian tensor (a ValueError names it); the device is checked after all of these."""
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a tensor; got {type(t).__name__}")
    if float32 and t.dtype != torch.float32:
        raise ValueError(f"{name} is {t.dtype}: only float32 is supported")
    if t.element_size() % 4:
        raise ValueError(f"{name} is {t.dtype}: rows move as 32-bit words")
    if t.dim() < 1 or t.shape[0] != P or (tail is not None and tuple(t.shape[1:]) != tail):
        want = f"[{P}, ...]" if tail is None else str([P] + list(tail))
        raise ValueError(f"{name} must be {want}; got {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} is not contiguous")


def _check_devices(named):
    """Every tensor on one CUDA (ROCm) device -> that device."""
    for name, t in named:
        if not t.is_cuda:
            raise L.SurfelRasterError(f"{name} is on {t.device}: densify / prune needs CUDA (ROCm) tensors; there is no CPU path "
                                      "(densify_and_prune_torch is the checker)")
    dev = named[0][1].device
    for name, t in named:
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, {named[0][0]} on {dev}")
    return dev


class _Plan:
    """The decision of one densify / prune over P Gaussians: the workspace sr_densify_plan filled, its four counts and what a child's
    position reads (the SOURCE rotation and scaling, the noise) -- and the gather of any [P, ...] tensor through it."""

    def __init__(self, opacity, scaling, rotation, accum, denom, max_grad, min_opacity, percent_dense_extent, ws_limit, prune_mask, noise, generator):
        dev = self.dev = opacity.device
        P = self.P = opacity.shape[0]
        self.scaling, self.rotation = scaling, rotation
        self.ws = workspace("sr_densify_workspace_bytes", dev, P)
        self.c_counts = counts = (C.c_uint32 * 4)()
        call("sr_densify_plan", dev, P, ptr(accum), ptr(denom), ptr(opacity), ptr(scaling), max_grad, min_opacity, percent_dense_extent, ws_limit,
             ptr(prune_mask), *buf(self.ws), counts)
        self.counts = K, Cl, S, H = tuple(int(c) for c in counts)
        self.P_out = K + Cl + 2 * H
        if noise is None:
            noise = torch.randn((2 * S, 2), device=dev, dtype=torch.float32, generator=generator)
        elif tuple(noise.shape) != (2 * S, 2) or noise.dtype != torch.float32 or noise.device != dev or not noise.is_contiguous():
            raise ValueError(f"noise must be a contiguous float32 [{2 * S},2] on {dev} for {S} split-selected Gaussians; got {noise.dtype} "
                             f"{list(noise.shape)} on {noise.device}")
        self.noise = noise

    def gather(self, tensors_and_roles):
        """[(tensor [P, ...], role)] (at most 8) -> the [P_out, ...] tensors, one launch."""
        outs, segs = [], []
        for t, role in tensors_and_roles:
            out = torch.empty((self.P_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            words = (t.numel() // self.P if self.P else math.prod(t.shape[1:])) * t.element_size() // 4
            segs.append(L.SrDensifySegment(t.data_ptr(), out.data_ptr(), words, role))
            outs.append(out)
        for at in range(0, len(segs), L.SR_DENSIFY_MAX_SEGMENTS):
            part = segs[at:at + L.SR_DENSIFY_MAX_SEGMENTS]
            call("sr_densify_apply", self.dev, self.P, self.c_counts, ptr(self.noise), ptr(self.rotation), ptr(self.scaling),
                 (L.SrDensifySegment * len(part))(*part), len(part), *buf(self.ws))
        return outs

    def views(self):
        """(flags uint8 [P], source int64 [P_out], kind int64 [P_out]) read from the workspace (the layout include/surfel_raster.h states)."""
        P, a = self.P, lambda n: (n + 255) // 256 * 256
        flags = self.ws[:P].clone()
        words = self.ws[a(P):a(P) + 4 * self.P_out].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return flags, words & 0x3FFFFFFF, words >> 30


def _group_order(names):
    """xyz first: a child's position reads the SOURCE scaling and rotation, so those two are gathered (and dropped) after it."""
    return sorted(names, key=lambda k: (k != "xyz", GROUP_NAMES.index(k) if k in GROUP_NAMES else len(GROUP_NAMES)))


def _thresholds(max_grad, min_opacity, extent, max_screen_size, percent_dense):
    max_grad = float(max_grad)
    if max_grad <= 0:
        raise ValueError(f"max_grad = {max_grad}: the threshold must be positive (the reference pads the gradient of fresh clones with 0, "
                         "so a threshold <= 0 would split them too)")
    return max_grad, float(min_opacity), float(percent_dense) * float(extent), (0.1 * float(extent) if max_screen_size else -1.0)


def _checked_inputs(params, moments, semantics, extra_rows, statistics=()):
    """Layouts first (ValueError, by name), then the devices (no CPU path) -> (device, P)."""
    missing = [k for k in GROUP_NAMES if k not in params]
    if missing:
        raise ValueError(f"params lacks the group(s) {missing}: it is keyed by the reference's group names {list(GROUP_NAMES)}")
    if not torch.is_tensor(params["xyz"]) or params["xyz"].dim() != 2:
        raise ValueError("xyz must be a [P,3] tensor")
    P, named = params["xyz"].shape[0], []
    for k, t in params.items():
        _check_rows(k, t, P, float32=True, tail=_TAIL.get(k))
        named.append((k, t))
        if moments.get(k) is not None:
            for key, s in zip(("exp_avg", "exp_avg_sq"), moments[k]):
                _check_rows(f"{key} of {k}", s, P, float32=True, tail=tuple(t.shape[1:]))
                named.append((f"{key} of {k}", s))
    for name, t in ([] if semantics is None else [("semantics", semantics)]) + [(f"extra_rows[{i}]", t) for i, t in enumerate(extra_rows)]:
        _check_rows(name, t, P)
        named.append((name, t))
    for name, t in statistics:
        _check_rows(name, t, P, float32=True)
        if t.numel() != P:
            raise ValueError(f"{name} must be [{P}] or [{P},1]; got {list(t.shape)}")
        named.append((name, t))
    return _check_devices(named), P


def densify_and_prune_tensors(params, moments, semantics, xyz_gradient_accum, denom, max_radii2D, max_grad, min_opacity, extent,
                              max_screen_size, percent_dense, noise=None, generator=None, extra_rows=()):
    """`densify_and_prune_torch` on float32 CUDA tensors through csrc/densify.hip: one decision pass with a single host read-back (the
    four counts), then one gather launch per parameter with its two moments.  `params` and `moments` are dicts keyed by the reference's
    group names; entries are popped from them as their group is done, so a caller that holds no other reference pays for one group of
    extra memory at a time, not for the whole model.  With `noise` None the normals are drawn once S is known:
    `torch.randn((2 S, 2), device=..., generator=generator)`.  `max_radii2D` is checked and otherwise unused (module docstring).
    -> Densified (flags, source and kind are read from the workspace)."""
    moments = moments if moments is not None else {}
    dev, P = _checked_inputs(params, moments, semantics, extra_rows,
                             (("xyz_gradient_accum", xyz_gradient_accum), ("denom", denom), ("max_radii2D", max_radii2D)))
    max_grad, min_opacity, pde, ws_limit = _thresholds(max_grad, min_opacity, extent, max_screen_size, percent_dense)
    plan = _Plan(params["opacity"], params["scaling"], params["rotation"], xyz_gradient_accum, denom, max_grad, min_opacity, pde, ws_limit,
                 None, noise, generator)
    out_p, out_m = _gather_groups(plan, params, moments)
    riders = plan.gather([(t, L.SR_DENSIFY_ROLE_COPY) for t in ([] if semantics is None else [semantics]) + list(extra_rows)])
    sem = riders.pop(0) if semantics is not None else None
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    flags, source, kind = plan.views()
    return Densified(out_p, out_m, sem, tuple(riders), zeros(plan.P_out, 1), zeros(plan.P_out, 1), zeros(plan.P_out), plan.counts, flags, source, kind)


def _gather_groups(plan, params, moments, install=None):
    """Every group of `params` with its moments through `plan`, xyz first, popping the sources as it goes."""
    out_p, out_m = {}, {}
    for k in _group_order(list(params)):
        t, st = params.pop(k), moments.pop(k, None)
        got = plan.gather([(t, _ROLE.get(k, L.SR_DENSIFY_ROLE_COPY))] + [(s, L.SR_DENSIFY_ROLE_MOMENT) for s in (st or ())])
        out_p[k], out_m[k] = got[0], (tuple(got[1:]) if st is not None else None)
        if install is not None:
            install(k, out_p[k], out_m[k])
        del t, st
    plan.scaling = plan.rotation = None
    return out_p, out_m


# ---- on a model shaped like the reference's GaussianModel ------------------------------------------------------------------------------
def _model_groups(model):
    """{name: param group} of model.optimizer, checked: the reference's six single-parameter groups, each holding the model's tensor."""
    groups = {}
    for group in model.optimizer.param_groups:
        name = group.get("name")
        if name not in _ATTRIBUTE or len(group["params"]) != 1:
            raise ValueError(f"optimizer group {name!r} with {len(group['params'])} parameter(s): densify / prune handles the reference's "
                             f"single-parameter groups {list(GROUP_NAMES)}")
        if group["params"][0] is not getattr(model, _ATTRIBUTE[name]):
            raise ValueError(f"optimizer group {name!r} does not hold the model's {_ATTRIBUTE[name]}")
        groups[name] = group
    missing = [k for k in GROUP_NAMES if k not in groups]
    if missing:
        raise ValueError(f"the optimizer lacks the group(s) {missing}")
    return groups


def _run_on_model(model, plan_of, keep_statistics):
    optimizer = getattr(model, "optimizer", None)
    params = {k: getattr(model, a).detach() for k, a in _ATTRIBUTE.items()}
    moments, groups = {}, {}
    if optimizer is not None:
        groups = _model_groups(model)
        for k, group in groups.items():
            stored_state = optimizer.state.get(group["params"][0], None)
            if stored_state is not None and "exp_avg" in stored_state:
                moments[k] = (stored_state["exp_avg"], stored_state["exp_avg_sq"])
    has_cluster = hasattr(model, "cluster_idx")
    riders = [model._semantics] + ([model.cluster_idx] if has_cluster else [])
    stat_names = [n for n in ("xyz_gradient_accum", "denom", "max_radii2D") if keep_statistics and getattr(model, n).shape[0] != 0]
    checked = stat_names if keep_statistics else ["xyz_gradient_accum", "denom"]
    dev, P = _checked_inputs(params, moments, model._semantics, riders[1:], [(n, getattr(model, n)) for n in checked])
    plan = plan_of(params, dev, P)

    def install(k, tensor, state):
        new = nn.Parameter(tensor.requires_grad_(True))
        if optimizer is not None:
            group = groups[k]
            stored_state = optimizer.state.get(group["params"][0], None)
            if stored_state is not None:
                if state is not None:
                    stored_state["exp_avg"], stored_state["exp_avg_sq"] = state
                del optimizer.state[group["params"][0]]
            group["params"][0] = new
            if stored_state is not None:
                optimizer.state[new] = stored_state
        setattr(model, _ATTRIBUTE[k], new)

    _gather_groups(plan, params, moments, install)
    stats = [getattr(model, n) for n in stat_names] if keep_statistics else []
    got = plan.gather([(t, L.SR_DENSIFY_ROLE_COPY) for t in riders + stats])
    model._semantics = got[0]
    if has_cluster:
        model.cluster_idx = got[1]
    if keep_statistics:
        for n, t in zip(stat_names, got[len(riders):]):
            setattr(model, n, t)
    else:
        model.xyz_gradient_accum = torch.zeros((plan.P_out, 1), dtype=torch.float32, device=dev)
        model.denom = torch.zeros((plan.P_out, 1), dtype=torch.float32, device=dev)
        model.max_radii2D = torch.zeros((plan.P_out,), dtype=torch.float32, device=dev)
    return plan.counts


def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, noise=None, generator=None):
    """`GaussianModel.densify_and_prune(max_grad, min_opacity, extent, max_screen_size)` of the reference on `model`: anything with
    `_xyz`, `_features_dc`, `_features_rest`, `_opacity`, `_scaling`, `_rotation`, `_semantics`, `xyz_gradient_accum`, `denom`,
    `max_radii2D`, `percent_dense`, an `optimizer` with the reference's named single-parameter groups (SurfelAdam or torch.optim.Adam,
    with state or before the first step) and optionally `cluster_idx`.  New `nn.Parameter`s are installed into the model and into
    `param_groups` group by group; each state dict moves, with its `step`, to the new parameter with gathered moments, exactly as
    `_prune_optimizer` and `cat_tensors_to_optimizer` leave it.  The statistics become zeros of the new size.  As in the reference a
    `max_screen_size` only switches the world-size test on (module docstring).  -> the counts (K, C, S, H)."""
    thresholds = _thresholds(max_grad, min_opacity, extent, max_screen_size, model.percent_dense)

    def plan_of(params, dev, P):
        return _Plan(params["opacity"], params["scaling"], params["rotation"], model.xyz_gradient_accum, model.denom, *thresholds, None, noise, generator)
    return _run_on_model(model, plan_of, keep_statistics=False)


def prune_points(model, mask):
    """`GaussianModel.prune_points(mask)` of the reference: the rows where `mask` ([P] bool) holds leave the parameters, the optimizer
    state, `_semantics`, `cluster_idx` and the three statistics (which keep their values, as in the reference).  Works with and without
    an optimizer on the model.  -> the counts (K, 0, 0, 0)."""
    def plan_of(params, dev, P):
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (P,):
            raise ValueError(f"mask must be a bool tensor [{P}]; got {getattr(mask, 'dtype', type(mask).__name__)} {list(getattr(mask, 'shape', []))}")
        _check_devices([("xyz", params["xyz"]), ("mask", mask)])
        return _Plan(params["opacity"], params["scaling"], params["rotation"], None, None, math.inf, -math.inf, math.inf, -1.0,
                     mask.contiguous(), None, None)
    return _run_on_model(model, plan_of, keep_statistics=True)

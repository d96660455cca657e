"""The tail of the reference's training iteration as HIP kernels (csrc/optimizer.hip) [REF train.py:165-200;
scene/gaussian_model.py:166-180, 555-557]:

    SurfelAdam            drop-in for the `torch.optim.Adam(l, lr=0.0, eps=1e-15)` of `training_setup`: the same `param_groups`, the same
                          per-parameter state (`step`, `exp_avg`, `exp_avg_sq`), one kernel launch per step for up to 8 tensors;
                          `row_mask=`: the step restricted to the rows a per-Gaussian mask selects (the masked re-optimisation model)
    adam_step             the raw call under it;  adam_step_float64: the same update in plain float64 torch, the checker
    densification_stats   `max_radii2D`, `xyz_gradient_accum` and `denom` of the visible Gaussians in one kernel, no boolean indexing;
                          densification_stats_torch: the reference's three lines, checker and timing baseline

The step is dense on purpose: Adam's moments decay and the parameters keep moving for Gaussians a view does not see (their gradient is
zero, their exp_avg is not), so skipping invisible rows would change the trajectory.  `row_mask` is for rows whose gradient AND moments
are zero for as long as the optimizer lives -- the masked-out rows of the reference's MaskGaussianModel -- where skipping changes nothing
(include/surfel_raster.h, sr_adam_step_rows, states the contract)."""
from __future__ import annotations

import torch

from . import _lib as L
from ._call import call, ptr

ADAM_CHUNK = L.SR_ADAM_CHUNK                    # elements a workgroup of adam_step_kernel handles per iteration
ADAM_MAX_SEGMENTS = L.SR_ADAM_MAX_SEGMENTS      # tensors per launch


def _bias_terms(lr, step, beta1, beta2):
    """(step_size, bc2_sqrt) in double, as torch's single-tensor Adam forms them."""
    step = float(step)
    return float(lr) / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5


def _check_adam_tensor(what, k, t, like=None):
    if t.is_sparse:
        raise ValueError(f"{what}[{k}] is sparse: SurfelAdam does not support sparse gradients")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}[{k}] is {t.dtype}: only float32 is supported")
    if like is not None and (t.device != like.device or t.numel() != like.numel()):
        raise ValueError(f"{what}[{k}]: {tuple(t.shape)} on {t.device} does not match its parameter ({tuple(like.shape)} on {like.device})")


def row_mask_bytes(mask):
    """A per-row mask as the kernels read it: uint8 [P], non-zero = selected.  bool is reinterpreted (no copy); anything else is taken
    as `!= 0` (the reference only ever builds 0 / 1 masks, as bool or as float)."""
    if mask.dim() != 1:
        raise ValueError(f"a row mask must be [P]; got {tuple(mask.shape)}")
    if mask.dtype != torch.bool:
        mask = mask != 0
    return mask.contiguous().view(torch.uint8)


def adam_step(params, grads, exp_avgs, exp_avg_sqs, lrs, steps, beta1, beta2, eps, row_mask=None):
    """One Adam update of `params`, `exp_avgs` and `exp_avg_sqs` in place, on the current stream of each tensor's device: one launch per
    device and 8 tensors.  `lrs[i]` is tensor i's learning rate and `steps[i]` its step count with this step included (1 for the first
    update); the bias corrections are formed from them in double.  float32, contiguous parameters and state; a non-contiguous
    gradient is made contiguous.
    The step writes through raw pointers, so it bumps the in-place version of every parameter and state tensor itself, as a torch
    in-place operation would: autograd and version-keyed caches (mask_model.MaskedSurfelModel's compose) see that they have changed.
    `row_mask` ([P], bool or 0 / 1): every tensor is [P, ...] and only the rows with a non-zero mask are updated; the other rows of the
    parameters and the state are neither read nor written, and what their gradient rows hold is never seen (sr_adam_step_rows)."""
    n = len(params)
    if row_mask is not None:
        row_mask = row_mask_bytes(row_mask)
        for k, p in enumerate(params):
            if p.dim() < 1 or p.shape[0] != row_mask.numel():
                raise ValueError(f"params[{k}] is {tuple(p.shape)}: with row_mask its leading dimension must be the mask's length {row_mask.numel()}")
            if p.device != row_mask.device:
                raise ValueError(f"params[{k}] is on {p.device}, row_mask on {row_mask.device}")
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(lrs) == len(steps) == n):
        raise ValueError("params, grads, exp_avgs, exp_avg_sqs, lrs and steps must have one entry per tensor")
    by_device = {}
    for k in range(n):
        p, g, m, v = params[k], grads[k], exp_avgs[k], exp_avg_sqs[k]
        _check_adam_tensor("params", k, p)
        _check_adam_tensor("grads", k, g, p)
        _check_adam_tensor("exp_avgs", k, m, p)
        _check_adam_tensor("exp_avg_sqs", k, v, p)
        if not p.is_cuda:
            raise L.SurfelRasterError("adam_step needs CUDA (ROCm) tensors; there is no CPU path (adam_step_float64 is the checker)")
        for what, t in (("params", p), ("exp_avgs", m), ("exp_avg_sqs", v)):
            if not t.is_contiguous():
                raise ValueError(f"{what}[{k}] is not contiguous: the step updates it in place")
        if float(steps[k]) < 1:
            raise ValueError(f"steps[{k}] = {steps[k]}: the step count includes this step, so it starts at 1")
        step_size, bc2_sqrt = _bias_terms(lrs[k], steps[k], beta1, beta2)
        g = g.contiguous()
        if row_mask is None:
            seg = L.SrAdamSegment(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step_size, bc2_sqrt)
        else:
            seg = L.SrAdamRowSegment(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step_size, bc2_sqrt,
                                     p.numel() // max(1, p.shape[0]))
        by_device.setdefault(p.device, []).append((seg, g, (p, m, v)))      # (g: a contiguous copy stays alive until the launch is enqueued)
    for dev, entries in by_device.items():
        for at in range(0, len(entries), ADAM_MAX_SEGMENTS):
            part = entries[at:at + ADAM_MAX_SEGMENTS]
            if row_mask is None:
                table = (L.SrAdamSegment * len(part))(*[e[0] for e in part])
                call("sr_adam_step", dev, table, len(part), float(beta1), float(beta2), float(eps))
            else:
                table = (L.SrAdamRowSegment * len(part))(*[e[0] for e in part])
                call("sr_adam_step_rows", dev, table, len(part), row_mask.numel(), ptr(row_mask), float(beta1), float(beta2), float(eps))
            for e in part:
                for t in e[2]:
                    torch.autograd.graph.increment_version(t)


def adam_step_float64(params, grads, exp_avgs, exp_avg_sqs, lrs, steps, beta1, beta2, eps):
    """The same update as a plain-torch statement in float64, in place on float64 tensors of any device: the checker."""
    for p, g, m, v, lr, step in zip(params, grads, exp_avgs, exp_avg_sqs, lrs, steps):
        if not (p.dtype == g.dtype == m.dtype == v.dtype == torch.float64):
            raise ValueError("adam_step_float64 is the float64 checker: every tensor must be float64")
        step_size, bc2_sqrt = _bias_terms(lr, step, beta1, beta2)
        m += (g - m) * (1 - beta1)
        v.mul_(beta2).add_((1 - beta2) * g * g)
        denom = v.sqrt() / bc2_sqrt + eps
        p -= step_size * (m / denom)


class SurfelAdam(torch.optim.Optimizer):
    """`torch.optim.Adam` for float32 parameters on the GPU with the whole step in one HIP kernel launch (per device and 8 tensors).

    Same constructor shape, `param_groups` keys and per-parameter state as torch's non-capturable Adam (`step`: a float32 scalar on the
    CPU; `exp_avg`, `exp_avg_sq`: `zeros_like(param)`, created at the first step that sees a gradient), so code that reaches into
    `optimizer.state[p]["exp_avg"]` or swaps `group["params"][0]` -- the reference's prune / densify surgery -- and `state_dict` /
    `load_state_dict` work unchanged, in both directions between this class and `torch.optim.Adam`.

    Refused with a ValueError that names the option: `weight_decay != 0`, `amsgrad`, `maximize`, `capturable`, `differentiable`,
    non-float32 parameters, sparse gradients, non-contiguous parameters or state.  `foreach` and `fused` are accepted and ignored
    (they pick one of torch's implementations of the same step).  CPU tensors raise SurfelRasterError: there is no CPU path.

    The learning rate and the bias corrections travel BY VALUE in each launch: `step()` is not meant to be captured into a HIP graph (a
    replay would repeat the captured step's step size).

    `row_mask` (not an Adam option; it is no part of `param_groups` or `state_dict`, so `load_state_dict` leaves it alone and a
    rebuilt optimizer has to be given it again; with a callable that is a lambda or closes over its model, as MaskedSurfelModel's does,
    the optimizer cannot be pickled and a deep copy keeps reading the ORIGINAL model's mask): a [P] tensor, or a callable returning the
    current one, read at every step.  Every parameter's leading dimension must then be P, and only the rows with a non-zero mask are stepped
    (sr_adam_step_rows): equal to the dense step as long as the other rows have zero gradients and zero moments, which is what the
    masked re-optimisation model guarantees (streetunveiler_amd.mask_model).  Without it nothing changes."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, row_mask=None):
        self.row_mask = row_mask
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        defaults = dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)

    @staticmethod
    def _check_group(group):
        if group.get("weight_decay", 0) != 0:
            raise ValueError(f"SurfelAdam does not support weight_decay (got {group['weight_decay']})")
        for option in ("amsgrad", "maximize", "capturable", "differentiable"):
            if group.get(option, False):
                raise ValueError(f"SurfelAdam does not support {option}=True")
        for p in group["params"]:
            if p.dtype != torch.float32:
                raise ValueError(f"SurfelAdam supports float32 parameters only (got {p.dtype})")

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for p in group["params"]:
                s = self.state.get(p, None)
                if s and not torch.is_tensor(s["step"]):
                    s["step"] = torch.tensor(float(s["step"]), dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        """One step for every parameter that has a `.grad`; a parameter without one keeps its state and its step count."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        row_mask = self.row_mask() if callable(self.row_mask) else self.row_mask
        calls = {}          # (beta1, beta2, eps) -> the argument lists of one adam_step call
        for group in self.param_groups:
            self._check_group(group)
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError("SurfelAdam does not support sparse gradients")
                if not p.is_cuda:
                    raise L.SurfelRasterError("SurfelAdam needs CUDA (ROCm) parameters; there is no CPU path")
                if not p.is_contiguous():
                    raise ValueError(f"SurfelAdam: a parameter of shape {tuple(p.shape)} is not contiguous")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                for key in ("exp_avg", "exp_avg_sq"):
                    s = state[key]
                    if s.dtype != torch.float32 or s.device != p.device or s.shape != p.shape or not s.is_contiguous():
                        raise ValueError(f"SurfelAdam: state {key!r} ({tuple(s.shape)}, {s.dtype}, {s.device}, contiguous={s.is_contiguous()}) "
                                         f"does not match its parameter ({tuple(p.shape)}, {p.dtype}, {p.device})")
                lists = calls.setdefault((float(beta1), float(beta2), float(group["eps"])), ([], [], [], [], [], []))
                for lst, item in zip(lists, (p, p.grad, state["exp_avg"], state["exp_avg_sq"], float(group["lr"]), state["step"])):
                    lst.append(item)
        for (beta1, beta2, eps), (params, grads, exp_avgs, exp_avg_sqs, lrs, steps) in calls.items():
            for s in steps:
                s += 1
            adam_step(params, grads, exp_avgs, exp_avg_sqs, lrs, [float(s) for s in steps], beta1, beta2, eps, row_mask=row_mask)
        return loss


def _stats_args(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D):
    P = radii.numel()
    if radii.dtype != torch.int32:
        raise ValueError(f"radii must be int32 as the rasterizer returns them (got {radii.dtype})")
    if viewspace_grad.shape != (P, 3):
        raise ValueError(f"viewspace_grad must be [{P},3]; got {tuple(viewspace_grad.shape)}")
    for name, t in (("xyz_gradient_accum", xyz_gradient_accum), ("denom", denom), ("max_radii2D", max_radii2D)):
        if t.numel() != P or t.dim() > 2:
            raise ValueError(f"{name} must be [{P}] or [{P},1]; got {tuple(t.shape)}")
    return P


def densification_stats(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D):
    """In place, for every Gaussian with `radii > 0` (the reference's `visibility_filter`), in one kernel on the current stream:

        max_radii2D[vis] = max(max_radii2D[vis], radii[vis]);  xyz_gradient_accum[vis] += |viewspace_grad[vis]|;  denom[vis] += 1

    `viewspace_grad` is `viewspace_point_tensor.grad` ([P,3]), `radii` the rasterizer's int32 [P]; `xyz_gradient_accum` and `denom` are
    the reference's [P,1] (or [P]), `max_radii2D` its [P].  Rows of invisible Gaussians are neither read nor written."""
    P = _stats_args(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D)
    if not radii.is_cuda:
        raise L.SurfelRasterError("densification_stats needs CUDA (ROCm) tensors; there is no CPU path (densification_stats_torch is the checker)")
    dev = radii.device
    for name, t in (("viewspace_grad", viewspace_grad), ("xyz_gradient_accum", xyz_gradient_accum), ("denom", denom), ("max_radii2D", max_radii2D)):
        if t.dtype != torch.float32 or t.device != dev:
            raise ValueError(f"{name} must be float32 on {dev}; got {t.dtype} on {t.device}")
    for name, t in (("xyz_gradient_accum", xyz_gradient_accum), ("denom", denom), ("max_radii2D", max_radii2D)):
        if not t.is_contiguous():
            raise ValueError(f"{name} is not contiguous: it is updated in place")
    viewspace_grad, radii = viewspace_grad.contiguous(), radii.contiguous()
    call("sr_densification_stats", dev, P, ptr(viewspace_grad), ptr(radii), ptr(xyz_gradient_accum), ptr(denom), ptr(max_radii2D))


def densification_stats_torch(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D):
    """The reference's three lines [REF train.py:168-169; scene/gaussian_model.py:555-557], in place, on any device and float dtype."""
    _stats_args(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D)
    visibility_filter = radii > 0
    max_radii2D[visibility_filter] = torch.max(max_radii2D[visibility_filter], radii[visibility_filter].to(max_radii2D.dtype))
    xyz_gradient_accum.view(-1, 1)[visibility_filter] += torch.norm(viewspace_grad[visibility_filter], dim=-1, keepdim=True)
    denom.view(-1, 1)[visibility_filter] += 1

"""The losses of a training iteration beside the image loss, fused (HIP, csrc/aux_loss.hip)
[REF train.py:87-88, 124-143; inpainting_pipeline/3_reoptimization/1_optimization.py:249-256]:

    semantic_cross_entropy(logits, target, weight)        F.cross_entropy(x[None], one_hot[None], weight=w) straight from the LABEL map
    surface_regularisers(rend_normal, surf_normal, rend_dist, lambda_normal, lambda_dist)
                                                          lambda_normal * mean(1 - sum_c rn_c sn_c) + lambda_dist * mean(rend_dist)
    opacity_shrink(raw_opacity)                           mean(sigmoid(raw_opacity))

Each is a differentiable operator (one forward kernel + a fixed-order reduction, one backward kernel; float64 arithmetic on float32
data, every value rounded once), has its two raw calls (`*_forward` / `*_backward`: no autograd, caller-owned buffers, capturable into a
HIP graph) and its `*_torch` twin: the reference's own lines on plain tensors -- in float64 the truth, in float32 the yardstick and the
timing baseline."""
from __future__ import annotations

import ctypes as C
import functools

import torch
import torch.nn.functional as F

from . import _lib as L
from ._call import buf, call, ptr, workspace as _workspace

MAX_CLASSES = 8
REFERENCE_CLASS_WEIGHT = (1.0, 1.0, 1.0, 1.0, 0.2, 1.0)   # [REF train.py:88]
_LABEL_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}


def _need_cuda(t, what):
    if not t.is_cuda:
        raise L.SurfelRasterError(f"{what} needs CUDA (ROCm) tensors; there is no CPU path ({what}_torch is the checker)")


def _upstream(g_loss, dev):
    """The upstream scalar as the kernels read it: one float32 on the device."""
    if g_loss.dtype == torch.float32 and g_loss.device == dev and g_loss.is_contiguous():
        return g_loss
    return g_loss.to(dev).contiguous().float()


def aux_loss_workspace(n, device):
    """The uint8 workspace of a forward over n pixels / Gaussians."""
    return _workspace("sr_aux_loss_workspace_bytes", device, int(n))


# ---- semantic cross-entropy ------------------------------------------------------------------------------------------------------------
def class_weights(weight, n_classes):
    """-> the n_classes weights as a tuple of float32-rounded Python floats; None = ones.  A sequence of Python floats costs nothing to
    read; a TENSOR is read here, every time (a device tensor: a host synchronisation) -- nothing is remembered about a tensor, whose
    address and version say nothing about its values.  To read one once, build a SemanticCrossEntropy from it."""
    if weight is None:
        return (1.0,) * n_classes
    if isinstance(weight, torch.Tensor):
        values = tuple(weight.detach().reshape(-1).to("cpu", torch.float32).tolist())
    else:
        values = tuple(C.c_float(float(v)).value for v in weight)
    if len(values) != n_classes:
        raise ValueError(f"weight must hold one value per class: {n_classes}; got {len(values)}")
    return values


@functools.lru_cache(maxsize=64)
def _weight_array(values):
    """The ctypes array of a tuple of VALUES (the key is the values themselves)."""
    return (C.c_float * len(values))(*values)


def _checked_logits(logits):
    _need_cuda(logits, "semantic_cross_entropy")
    if logits.dim() != 3 or not 1 <= logits.shape[0] <= MAX_CLASSES or logits.shape[1] < 1 or logits.shape[2] < 1:
        raise ValueError(f"logits must be [C,H,W] with 1 <= C <= {MAX_CLASSES} and H, W >= 1; got {tuple(logits.shape)}")


def _checked_ce(logits, target):
    """Contiguous float32 [C,H,W] logits and a target the kernels read -> (logits, target, label_bytes, (W, H, C))."""
    _checked_logits(logits)
    Cn, H, W = logits.shape
    target = target.to(logits.device)
    if target.is_floating_point():
        if target.shape != logits.shape:
            raise ValueError(f"a float target must be [C,H,W] like logits {tuple(logits.shape)}; got {tuple(target.shape)}")
        target, label_bytes = target.detach().contiguous().float(), 0
    else:
        if tuple(target.shape) != (H, W):
            raise ValueError(f"an integer target must be the [H,W] = [{H},{W}] label map; got {tuple(target.shape)}")
        if target.dtype == torch.bool:
            target = target.to(torch.uint8)
        elif target.dtype not in _LABEL_BYTES:
            target = target.to(torch.int32)           # int8 / int16: every value fits
        target = target.contiguous()
        label_bytes = _LABEL_BYTES[target.dtype]
    return logits.contiguous().float(), target, label_bytes, (int(W), int(H), int(Cn))


# The _launch_* functions take what a _checked_* function returned and check nothing again: the raw calls and the autograd functions
# both end here, each after checking once.
def _launch_ce_forward(logits, target, label_bytes, dims, weights, workspace=None, out=None):
    W, H, Cn = dims
    dev = logits.device
    if workspace is None:
        workspace = aux_loss_workspace(W * H, dev)
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=dev)
    call("sr_semantic_ce_forward", dev, W, H, Cn, ptr(logits), ptr(target), label_bytes, _weight_array(weights), *buf(workspace), ptr(out))
    return out


def _launch_ce_backward(logits, target, label_bytes, dims, weights, g_loss, out=None):
    W, H, Cn = dims
    dev = logits.device
    g_loss = _upstream(g_loss, dev)
    if out is None:
        out = torch.empty_like(logits)
    call("sr_semantic_ce_backward", dev, W, H, Cn, ptr(logits), ptr(target), label_bytes, _weight_array(weights), ptr(g_loss), ptr(out))
    return out


def semantic_ce_forward(logits, target, weight=None, workspace=None, out=None):
    """Raw forward on the current stream -> out[1] = {loss} on the device."""
    logits, target, label_bytes, dims = _checked_ce(logits, target)
    return _launch_ce_forward(logits, target, label_bytes, dims, class_weights(weight, dims[2]), workspace, out)


def semantic_ce_backward(logits, target, g_loss, weight=None, out=None):
    """Raw backward on the current stream: g_loss is the upstream scalar as a device tensor -> g_logits [C,H,W] (`out` to write into)."""
    logits, target, label_bytes, dims = _checked_ce(logits, target)
    return _launch_ce_backward(logits, target, label_bytes, dims, class_weights(weight, dims[2]), g_loss, out)


class _SemanticCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weights):
        logits_c, target_c, label_bytes, dims = _checked_ce(logits, target)
        out = _launch_ce_forward(logits_c, target_c, label_bytes, dims, weights)
        ctx.save_for_backward(logits_c, target_c)
        ctx.call, ctx.like = (label_bytes, dims, weights), (logits.shape, logits.dtype)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        logits, target = ctx.saved_tensors
        g = _launch_ce_backward(logits, target, *ctx.call, g_loss)
        return g.reshape(ctx.like[0]).to(ctx.like[1]), None, None


def semantic_cross_entropy(logits, target, weight=None):
    """-> the 0-dim loss, differentiable w.r.t. logits [C,H,W].  target: the integer [H,W] label map (`viewpoint_cam.semantic_map`; a
    label outside 0..C-1 adds nothing and still counts in the mean) or a float [C,H,W] image of probabilities.  weight: per class, a
    sequence of Python floats (free) or a tensor (read on every call: see class_weights; SemanticCrossEntropy reads it once); None =
    ones.  Replaces get_semantic_prob_image() and F.cross_entropy of the reference's train.py:87-88."""
    _checked_logits(logits)
    return _SemanticCrossEntropy.apply(logits, target, class_weights(weight, logits.shape[0]))


class SemanticCrossEntropy:
    """semantic_cross_entropy with its class weights read once, here: `ce = SemanticCrossEntropy(weight); loss = ce(logits, labels)`."""

    def __init__(self, weight=REFERENCE_CLASS_WEIGHT):
        self.weights = None if weight is None else class_weights(weight, len(weight))

    def __call__(self, logits, target):
        return semantic_cross_entropy(logits, target, self.weights)


def one_hot_image(labels, n_classes):
    """The reference's Camera.get_semantic_prob_image() [REF scene/cameras.py:77-83] on a label map: [C,H,W] float32."""
    prob = torch.zeros((n_classes,) + tuple(labels.shape), dtype=torch.float32, device=labels.device)
    for i in range(n_classes):
        prob[i, labels == i] = 1.0
    return prob


def semantic_cross_entropy_torch(logits, target, weight=None):
    """The reference's lines on plain tensors: an integer target goes through the one-hot image first.  The weights are float32 values,
    as the reference's torch.tensor([...]) holds them, whatever dtype the logits have."""
    n = logits.shape[0]
    if not target.is_floating_point():
        target = one_hot_image(target.to(logits.device), n)
    w = torch.ones(n) if weight is None else torch.as_tensor(weight).detach().to("cpu", torch.float32)
    return F.cross_entropy(logits.unsqueeze(0), target.to(logits).unsqueeze(0), weight=w.to(logits))


# ---- surface regularisers --------------------------------------------------------------------------------------------------------------
def _checked_reg(rend_normal, surf_normal, rend_dist):
    _need_cuda(rend_normal, "surface_regularisers")
    if rend_normal.dim() != 3 or rend_normal.shape[0] != 3 or surf_normal.shape != rend_normal.shape:
        raise ValueError(f"rend_normal and surf_normal must both be [3,H,W]; got {tuple(rend_normal.shape)} and {tuple(surf_normal.shape)}")
    _, H, W = rend_normal.shape
    if H < 1 or W < 1 or tuple(rend_dist.shape) not in ((1, H, W), (H, W)):
        raise ValueError(f"rend_dist must be [1,{H},{W}] with H, W >= 1; got {tuple(rend_dist.shape)}")
    c = lambda t: t.to(rend_normal.device).contiguous().float()
    return c(rend_normal), c(surf_normal), c(rend_dist), (int(W), int(H))


def _launch_reg_forward(rn, sn, rd, dims, lambda_normal, lambda_dist, workspace=None, out=None):
    W, H = dims
    dev = rn.device
    if workspace is None:
        workspace = aux_loss_workspace(W * H, dev)
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=dev)
    call("sr_surface_reg_forward", dev, W, H, ptr(rn), ptr(sn), ptr(rd), float(lambda_normal), float(lambda_dist), *buf(workspace), ptr(out))
    return out


def _launch_reg_backward(rn, sn, rd, dims, lambda_normal, lambda_dist, g_loss, want=(True, True, True), out=None):
    W, H = dims
    dev = rn.device
    g_loss = _upstream(g_loss, dev)
    if out is None:
        out = tuple(torch.empty_like(t) if w else None for t, w in zip((rn, sn, rd), want))
    call("sr_surface_reg_backward", dev, W, H, ptr(rn), ptr(sn), float(lambda_normal), float(lambda_dist), ptr(g_loss), ptr(out[0]), ptr(out[1]),
         ptr(out[2]))
    return out


def surface_reg_forward(rend_normal, surf_normal, rend_dist, lambda_normal, lambda_dist, workspace=None, out=None):
    """Raw forward on the current stream -> out[3] = {loss, lambda_normal * normal, lambda_dist * dist} on the device."""
    rn, sn, rd, dims = _checked_reg(rend_normal, surf_normal, rend_dist)
    return _launch_reg_forward(rn, sn, rd, dims, lambda_normal, lambda_dist, workspace, out)


def surface_reg_backward(rend_normal, surf_normal, rend_dist, lambda_normal, lambda_dist, g_loss, want=(True, True, True), out=None):
    """Raw backward on the current stream -> (g_rend_normal, g_surf_normal, g_rend_dist), None where `want` is False; `out`: the three
    tensors (or None) to write into instead."""
    rn, sn, rd, dims = _checked_reg(rend_normal, surf_normal, rend_dist)
    return _launch_reg_backward(rn, sn, rd, dims, lambda_normal, lambda_dist, g_loss, want, out)


class _SurfaceRegularisers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rend_normal, surf_normal, rend_dist, lambda_normal, lambda_dist):
        rn, sn, rd, dims = _checked_reg(rend_normal, surf_normal, rend_dist)
        out = _launch_reg_forward(rn, sn, rd, dims, lambda_normal, lambda_dist)
        ctx.save_for_backward(rn, sn, rd)
        ctx.dims = dims
        ctx.lambdas = (float(lambda_normal), float(lambda_dist))
        ctx.like = tuple((t.shape, t.dtype) for t in (rend_normal, surf_normal, rend_dist))
        loss, normal_loss, dist_loss = out[0], out[1], out[2]
        ctx.mark_non_differentiable(normal_loss, dist_loss)
        return loss, normal_loss, dist_loss

    @staticmethod
    def backward(ctx, g_loss, _g_normal, _g_dist):
        rn, sn, rd = ctx.saved_tensors
        grads = _launch_reg_backward(rn, sn, rd, ctx.dims, ctx.lambdas[0], ctx.lambdas[1], g_loss, want=ctx.needs_input_grad[:3])
        back = [None if g is None else g.reshape(like[0]).to(like[1]) for g, like in zip(grads, ctx.like)]
        return back[0], back[1], back[2], None, None


def surface_regularisers(rend_normal, surf_normal, rend_dist, lambda_normal, lambda_dist):
    """-> (loss, normal_loss, dist_loss), three 0-dim tensors on the device: loss = normal_loss + dist_loss is differentiable w.r.t. the
    three maps, the two parts are what the reference logs as loss_dict['Lnormal'] / ['Ldist'].  Replaces train.py:124-139."""
    return _SurfaceRegularisers.apply(rend_normal, surf_normal, rend_dist, float(lambda_normal), float(lambda_dist))


def surface_regularisers_torch(rend_normal, surf_normal, rend_dist, lambda_normal, lambda_dist):
    """The reference's lines [REF train.py:128-139] -> (loss, normal_loss, dist_loss)."""
    normal_error = (1 - (rend_normal * surf_normal).sum(dim=0))[None]
    normal_loss = lambda_normal * (normal_error).mean()
    dist_loss = lambda_dist * (rend_dist).mean()
    return normal_loss + dist_loss, normal_loss, dist_loss


# ---- opacity shrink --------------------------------------------------------------------------------------------------------------------
def _checked_opacity(opacity):
    _need_cuda(opacity, "opacity_shrink")
    if opacity.numel() < 1:
        raise ValueError(f"opacity must hold at least one Gaussian; got {tuple(opacity.shape)}")
    return opacity.contiguous().float()


def _launch_shrink_forward(opacity, activated, workspace=None, out=None):
    dev, P = opacity.device, opacity.numel()
    if workspace is None:
        workspace = aux_loss_workspace(P, dev)
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=dev)
    call("sr_opacity_shrink_forward", dev, P, ptr(opacity), int(bool(activated)), *buf(workspace), ptr(out))
    return out


def _launch_shrink_backward(opacity, g_loss, activated, out=None):
    dev = opacity.device
    g_loss = _upstream(g_loss, dev)
    if out is None:
        out = torch.empty_like(opacity)
    call("sr_opacity_shrink_backward", dev, opacity.numel(), ptr(opacity), int(bool(activated)), ptr(g_loss), ptr(out))
    return out


def opacity_shrink_forward(opacity, activated=False, workspace=None, out=None):
    """Raw forward on the current stream -> out[1] = {mean(sigmoid(opacity))} (activated: mean(opacity)) on the device."""
    return _launch_shrink_forward(_checked_opacity(opacity), activated, workspace, out)


def opacity_shrink_backward(opacity, g_loss, activated=False, out=None):
    """Raw backward on the current stream -> the gradient, shaped like opacity (`out` to write into)."""
    return _launch_shrink_backward(_checked_opacity(opacity), g_loss, activated, out)


class _OpacityShrink(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacity, activated):
        opacity_c = _checked_opacity(opacity)
        out = _launch_shrink_forward(opacity_c, activated)
        ctx.save_for_backward(opacity_c)
        ctx.activated, ctx.like = bool(activated), (opacity.shape, opacity.dtype)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        (opacity,) = ctx.saved_tensors
        g = _launch_shrink_backward(opacity, g_loss, ctx.activated)
        return g.reshape(ctx.like[0]).to(ctx.like[1]), None


def opacity_shrink(raw_opacity, activated=False):
    """-> the 0-dim mean of sigmoid(raw_opacity) over the P Gaussians, differentiable: `get_opacity.mean()` of train.py:142 from the RAW
    `_opacity` (what fused_activations and the masked model's raw_parameters() hand out).  activated=True: the values are opacities
    already, the mean alone."""
    return _OpacityShrink.apply(raw_opacity, bool(activated))


def opacity_shrink_torch(raw_opacity, activated=False):
    """The reference's lines [REF train.py:142; scene/gaussian_model.py:113-115]."""
    return (raw_opacity if activated else torch.sigmoid(raw_opacity)).mean()

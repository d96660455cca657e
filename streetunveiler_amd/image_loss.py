"""Fused photometric loss (HIP): the L1 + D-SSIM image loss that ends every training iteration of the reference
[REF train.py:113-119; utils/loss_utils.py:18-64], with the sky composite folded in:

    x    = image + sky * (1 - alpha)                      (only when sky and alpha are given)
    loss = (1 - lambda_dssim) * mean|x - gt| + lambda_dssim * (1 - ssim(x, gt))

`photometric_loss` is the differentiable operator (one forward kernel + a fixed-order reduction, one backward kernel),
`image_loss_forward` / `image_loss_backward` are the two raw calls, and `photometric_loss_torch` is the same function in
plain torch: the CPU checker (in float64: the truth) and the timing baseline on the GPU."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import _lib as L
from ._call import buf, call, ptr, workspace as _workspace

WINDOW_SIZE, WINDOW_SIGMA = 11, 1.5
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2


def _checked(image, gt, sky, alpha):
    """Contiguous float32 [C,H,W] inputs on one GPU -> (image, gt, sky, alpha, (W, H, C))."""
    if not image.is_cuda:
        raise L.SurfelRasterError("photometric_loss needs CUDA (ROCm) tensors; there is no CPU path (photometric_loss_torch is the checker)")
    if (sky is None) != (alpha is None):
        raise ValueError("sky and alpha go together: give both or neither")
    if image.dim() != 3 or gt.shape != image.shape:
        raise ValueError(f"image and gt must both be [C,H,W]; got {tuple(image.shape)} and {tuple(gt.shape)}")
    Cn, H, W = image.shape
    if sky is not None and (sky.shape != image.shape or alpha.numel() != H * W):
        raise ValueError(f"sky must be {tuple(image.shape)} and alpha [1,{H},{W}]; got {tuple(sky.shape)} and {tuple(alpha.shape)}")
    c = lambda t: None if t is None else t.to(image.device).contiguous().float()
    return c(image), c(gt), c(sky), c(alpha), (int(W), int(H), int(Cn))


def image_loss_workspace(image):
    """The uint8 workspace a forward / backward pair on a [C,H,W] image shares."""
    Cn, H, W = image.shape
    return _workspace("sr_image_loss_workspace_bytes", image.device, int(W), int(H), int(Cn))


def image_loss_forward(image, gt, lambda_dssim=0.2, sky=None, alpha=None, workspace=None, out=None):
    """Raw forward on the current stream -> (out[3] = {loss, l1, ssim} on the device, workspace for image_loss_backward)."""
    image, gt, sky, alpha, (W, H, Cn) = _checked(image, gt, sky, alpha)
    dev = image.device
    if workspace is None:
        workspace = image_loss_workspace(image)
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=dev)
    call("sr_image_loss_forward", dev, W, H, Cn, float(lambda_dssim), ptr(image), ptr(gt), ptr(sky), ptr(alpha), *buf(workspace), ptr(out))
    return out, workspace


def image_loss_backward(image, gt, workspace, g_loss, lambda_dssim=0.2, sky=None, alpha=None, out=None):
    """Raw backward on the current stream: g_loss is the upstream scalar as a device tensor, workspace what image_loss_forward filled
    for the same inputs -> (g_image, g_sky, g_alpha), the last two None without the composite.  out = the tensors to write into."""
    image, gt, sky, alpha, (W, H, Cn) = _checked(image, gt, sky, alpha)
    dev = image.device
    g_loss = g_loss.to(dev).contiguous().float()
    if out is None:
        out = (torch.empty_like(image), None if sky is None else torch.empty_like(sky), None if sky is None else torch.empty_like(alpha))
    g_image, g_sky, g_alpha = out
    call("sr_image_loss_backward", dev, W, H, Cn, float(lambda_dssim), ptr(image), ptr(gt), ptr(sky), ptr(alpha), *buf(workspace), ptr(g_loss),
         ptr(g_image), ptr(g_sky), ptr(g_alpha))
    return g_image, g_sky, g_alpha


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lambda_dssim, sky, alpha):
        image_c, gt_c, sky_c, alpha_c, _ = _checked(image, gt, sky, alpha)
        out, workspace = image_loss_forward(image_c, gt_c, lambda_dssim, sky_c, alpha_c)
        ctx.save_for_backward(image_c, gt_c, sky_c, alpha_c, workspace)
        ctx.lambda_dssim = float(lambda_dssim)
        ctx.like = tuple(None if t is None else (t.shape, t.dtype) for t in (image, sky, alpha))   # of the gradients to hand back
        loss, l1, ssim = out[0], out[1], out[2]
        ctx.mark_non_differentiable(l1, ssim)
        return loss, l1, ssim

    @staticmethod
    def backward(ctx, g_loss, _g_l1, _g_ssim):
        image, gt, sky, alpha, workspace = ctx.saved_tensors
        grads = image_loss_backward(image, gt, workspace, g_loss, ctx.lambda_dssim, sky, alpha)
        back = [None if (g is None or like is None) else g.reshape(like[0]).to(like[1]) for g, like in zip(grads, ctx.like)]
        return back[0], None, None, back[1], back[2]


def photometric_loss(image, gt, lambda_dssim=0.2, sky=None, alpha=None):
    """-> (loss, l1, ssim), three 0-dim tensors on the device; loss is differentiable w.r.t. image, sky and alpha, l1 and ssim are for
    logging.  Replaces the composite, l1_loss, ssim and their weighting of the reference's train.py:113-119 with one call."""
    return _PhotometricLoss.apply(image, gt, float(lambda_dssim), sky, alpha)


def _window(channels, dtype, device):
    """[C,1,11,11]: the normalised Gaussian taps in float32, their outer product in float32, then the cast -- the roundings of the
    reference's window, so that the float64 evaluation is the truth of what the reference computes."""
    taps = torch.tensor([math.exp(-(i - WINDOW_SIZE // 2) ** 2 / (2.0 * WINDOW_SIGMA ** 2)) for i in range(WINDOW_SIZE)], dtype=torch.float32)
    taps = taps / taps.sum()
    w2d = torch.outer(taps, taps)
    return w2d.expand(channels, 1, WINDOW_SIZE, WINDOW_SIZE).contiguous().to(device=device, dtype=dtype)


def photometric_loss_torch(image, gt, lambda_dssim=0.2, sky=None, alpha=None):
    """The same function in plain torch, on any device and in any float dtype: five grouped convolutions with the 2-D window, zero
    padding of 5 -> (loss, l1, ssim)."""
    if (sky is None) != (alpha is None):
        raise ValueError("sky and alpha go together: give both or neither")
    x = image if sky is None else image + sky * (1 - alpha)
    channels = x.shape[-3]
    w = _window(channels, x.dtype, x.device)
    blur = lambda t: F.conv2d(t, w, padding=WINDOW_SIZE // 2, groups=channels)
    mu1, mu2 = blur(x), blur(gt)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = blur(x * x) - mu1_sq
    s2 = blur(gt * gt) - mu2_sq
    s12 = blur(x * gt) - mu12
    ssim_map = ((2 * mu12 + SSIM_C1) * (2 * s12 + SSIM_C2)) / ((mu1_sq + mu2_sq + SSIM_C1) * (s1 + s2 + SSIM_C2))
    l1 = (x - gt).abs().mean()
    ssim = ssim_map.mean()
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim)
    return loss, l1, ssim

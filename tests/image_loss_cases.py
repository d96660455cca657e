"""Shared by tests/test_image_loss_golden.py, tests/test_gpu_image_loss.py and tools/image_loss_parity.py: the fixture cases of
tests/golden/image_loss_golden.npz (tools/make_image_loss_golden.py: the reference's own python), seeded cases of any size, and THE BAR.

The bar is a ratio against the reference's own rounding noise, per case and per quantity:
    scalars (loss, l1, ssim):  d = |value - truth|
    gradients:                 d = max|value - truth| / max|truth|
    d_ref = the same deviation of the reference's float32 run on the case (fixture: the stored run; other sizes: photometric_loss_torch
            in float32 on the CPU), truth = the float64 run
    ratio = d / max(d_ref, 1e-6 * scale)  <=  4          (scale = |truth| for a scalar, 1 for the already relative gradient figure)
4x because the kernels sum the window separably, in another order and with contraction (a separable float32 evaluation on the CPU sits at
0.3-0.6 x d_ref); a wrong or dropped term shows up at 1e-2 or more, thousands of times the bar."""
import os

import numpy as np
import torch

from streetunveiler_amd.image_loss import photometric_loss, photometric_loss_torch

BAR = 4.0
FLOOR = 1e-6
SCALARS = ("loss", "l1", "ssim")
GRADS = ("g_image", "g_sky", "g_alpha")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_loss_golden.npz")
# (W, H) of the GPU-only cases: one pixel, frames narrower / lower than the window, a size that is no multiple of the tile, the `-r 4`
# frame and the full frame
GPU_SIZES = ((1, 1), (5, 300), (300, 5), (129, 257), (480, 320), (1920, 1080))


def fixture_cases():
    """[{name, lambda_dssim, image, gt, sky, alpha (float32 tensors or None), ref: {...}, truth: {...} (numpy)}]"""
    z = np.load(GOLDEN)
    out = []
    for name in z["names"]:
        pre = str(name) + "/"
        t = lambda k: torch.tensor(z[pre + k]) if pre + k in z.files else None
        case = dict(name=str(name), lambda_dssim=float(z[pre + "lambda_dssim"]), image=t("image"), gt=t("gt"), sky=t("sky"), alpha=t("alpha"))
        for tag in ("ref", "truth"):
            case[tag] = {k: np.asarray(z[pre + tag + "_" + k], dtype=np.float64) for k in SCALARS + GRADS if pre + tag + "_" + k in z.files}
        out.append(case)
    return out


def seeded_case(W, H, composite, channels=3, lambda_dssim=0.2, seed=0):
    """A noisy image against its clean target (and a sky behind a soft alpha), float32 on the CPU; ref / truth not yet filled."""
    r = torch.Generator().manual_seed(1000003 * seed + 7919 * W + H + (1 if composite else 0))
    u = lambda c: torch.rand(c, H, W, generator=r)
    gt = u(channels)
    image = (gt + 0.1 * torch.randn(channels, H, W, generator=r)).clamp(0, 1)
    sky = alpha = None
    if composite:
        sky, alpha = u(channels), u(1)
        image = image * alpha
    return dict(name=f"seeded_{W}x{H}" + ("_sky" if composite else ""), lambda_dssim=lambda_dssim, image=image, gt=gt, sky=sky, alpha=alpha)


def _collect(case, outs, leaves):
    loss, l1, ssim = outs
    grads = torch.autograd.grad(loss, leaves)
    res = dict(loss=loss, l1=l1, ssim=ssim, g_image=grads[0])
    if case["sky"] is not None:
        res["g_sky"], res["g_alpha"] = grads[1], grads[2]
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


def _leaves(case, dtype, device):
    prep = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype, copy=True).requires_grad_()
    image, sky, alpha = prep(case["image"]), prep(case["sky"]), prep(case["alpha"])
    return image, case["gt"].to(device=device, dtype=dtype), sky, alpha, [t for t in (image, sky, alpha) if t is not None]


def run_torch(case, dtype, device="cpu"):
    """photometric_loss_torch and its autograd gradients -> {quantity: float64 numpy}"""
    image, gt, sky, alpha, leaves = _leaves(case, dtype, device)
    return _collect(case, photometric_loss_torch(image, gt, case["lambda_dssim"], sky, alpha), leaves)


def run_hip(case, device="cuda:0"):
    """photometric_loss (the HIP kernels) and its gradients -> {quantity: float64 numpy}"""
    image, gt, sky, alpha, leaves = _leaves(case, torch.float32, device)
    return _collect(case, photometric_loss(image, gt, case["lambda_dssim"], sky, alpha), leaves)


def with_cpu_reference(case):
    """Fills ref (float32) and truth (float64) of a seeded case with photometric_loss_torch on the CPU."""
    case["ref"], case["truth"] = run_torch(case, torch.float32), run_torch(case, torch.float64)
    return case


def deviation(value, truth, key):
    d = float(np.abs(np.asarray(value, dtype=np.float64) - truth).max())
    return d if key in SCALARS else d / float(np.abs(truth).max())


def ratios(got, case):
    """{quantity: deviation of `got` from the truth over max(d_ref, floor)}: the figure the bar bounds by 4."""
    out = {}
    for key, truth in case["truth"].items():
        scale = abs(float(truth)) if key in SCALARS else 1.0
        d_ref = deviation(case["ref"][key], truth, key)
        out[key] = deviation(got[key], truth, key) / max(d_ref, FLOOR * scale)
    return out


def assert_within_bar(got, case, what):
    r = ratios(got, case)
    print(f"{what} {case['name']}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= BAR}
    assert not bad, f"{what}, case {case['name']}: beyond {BAR} x the reference's own float32 deviation: {bad}"
    return r

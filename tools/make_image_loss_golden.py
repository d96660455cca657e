"""Writes tests/golden/image_loss_golden.npz: the photometric loss of seeded cases as the REFERENCE's own python computes it.

    python tools/make_image_loss_golden.py --reference <checkout of the reference>      (or STREETUNVEILER_REFERENCE=<checkout>)

Development-machine tool (CPU): imports the reference's utils/loss_utils.py from its checkout, forms the composite and the weighted
loss with the expressions of its train.py:115-119, and stores per case
    the inputs (float32), lambda_dssim,
    ref_{loss,l1,ssim} and ref_g_{image,sky,alpha}:     the reference's float32 run and its autograd gradients,
    truth_{loss,l1,ssim} and truth_g_{image,sky,alpha}: the same code on the same inputs in float64.
Only this data is committed; nothing of the reference's program text is."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "image_loss_golden.npz")


def load_loss_utils(reference):
    path = os.path.join(reference, "utils", "loss_utils.py")
    spec = importlib.util.spec_from_file_location("reference_loss_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth(t, passes):
    """Repeated 5x5 box blur with replicated borders: a low-pass image in [0, 1]."""
    for _ in range(passes):
        t = F.avg_pool2d(F.pad(t[None], (2, 2, 2, 2), mode="replicate"), 5, stride=1)[0]
    return t


def cases():
    """(name, lambda_dssim, image, gt, sky, alpha), all float32 and seeded."""
    r = torch.Generator().manual_seed(20240611)
    u = lambda *s: torch.rand(*s, generator=r)
    n = lambda *s: torch.randn(*s, generator=r)
    out = []
    out.append(("noise_7x9", 0.2, u(3, 7, 9), u(3, 7, 9), None, None))                 # smaller than the window
    out.append(("noise_37x53", 0.2, u(3, 37, 53), u(3, 37, 53), None, None))
    base = smooth(u(1, 64, 200), 3)
    base = (base - base.min()) / (base.max() - base.min())
    out.append(("smooth_c1_64x200", 0.2, (base + 0.02 * n(1, 64, 200)).clamp(0, 1), base.clone(), None, None))
    flat = torch.full((1, 48, 80), 0.25)
    flat[:, :, 37:] = 0.75                                                              # a step edge between two flat regions
    flat[:, 30:, :20] = 0.5
    out.append(("flat_step_c1_48x80", 0.5, flat + 1e-3 * n(1, 48, 80), flat + 1e-3 * n(1, 48, 80), None, None))
    H, W = 18, 29
    alpha = smooth(u(1, H, W), 1)
    out.append(("sky_18x29", 0.2, u(3, H, W) * alpha, u(3, H, W), u(3, H, W), alpha))
    H, W = 20, 33
    alpha = smooth(u(1, H, W), 1)
    alpha[:, :7, :] = 0.0                                                               # pure sky
    alpha[:, 13:, 10:] = 1.0                                                            # fully covered
    out.append(("sky_binary_alpha_20x33", 0.5, u(3, H, W) * alpha, smooth(u(3, H, W), 1), u(3, H, W), alpha))
    return out


def run_reference(lu, dtype, lam, image, gt, sky, alpha):
    leaves = [t.to(dtype).requires_grad_() for t in (image, sky, alpha) if t is not None]
    img = leaves[0]
    gt = gt.to(dtype)
    composite = img if sky is None else img + leaves[1] * (1 - leaves[2])
    l1 = lu.l1_loss(composite, gt)
    ssim = lu.ssim(composite, gt)
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    grads = torch.autograd.grad(loss, leaves)
    res = {"loss": loss, "l1": l1, "ssim": ssim, "g_image": grads[0]}
    if sky is not None:
        res["g_sky"], res["g_alpha"] = grads[1], grads[2]
    return {k: v.detach().numpy() for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("STREETUNVEILER_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not args.reference:
        sys.exit("give --reference (or STREETUNVEILER_REFERENCE): the checkout that holds utils/loss_utils.py")
    lu = load_loss_utils(args.reference)
    torch.set_num_threads(1)   # one summation order, whatever the machine
    data, names = {}, []
    for name, lam, image, gt, sky, alpha in cases():
        names.append(name)
        pre = name + "/"
        data[pre + "lambda_dssim"] = np.float64(lam)
        for key, t in (("image", image), ("gt", gt), ("sky", sky), ("alpha", alpha)):
            if t is not None:
                data[pre + key] = t.numpy().astype(np.float32)
        for tag, dtype in (("ref", torch.float32), ("truth", torch.float64)):
            for key, v in run_reference(lu, dtype, lam, image, gt, sky, alpha).items():
                data[pre + tag + "_" + key] = v
    data["names"] = np.array(names)
    np.savez_compressed(args.out, **data)
    print(args.out, os.path.getsize(args.out), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()

"""Times forward + backward of the fused photometric loss against the same loss as stock torch kernels, on one GPU in one call.

    python tools/time_image_loss.py [--out profiles/image_loss_time.json] [--rounds 7] [--iters 50]

Sizes 480x320, 1920x1080 and 3840x2160, with and without the sky composite.  Every (size, variant, implementation) is warmed first; then
the two implementations ALTERNATE round by round, each round being `iters` steps between two device events; the figures are the median
over the rounds and their spread (min, max).  Also: the bytes the fused design has to move per pixel-channel (computed from the shapes, see
`design_bytes`) and the rate that gives over the fused pair's time.  A kernel trace, if wanted, is a run of its own (rocprofv3
--kernel-trace --stats -- python tools/time_image_loss.py ...); the numbers here are taken with the profiler off."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from streetunveiler_amd.image_loss import photometric_loss, photometric_loss_torch  # noqa: E402
from tools import measure  # noqa: E402

SIZES = ((480, 320), (1920, 1080), (3840, 2160))


def design_bytes(W, H, C, composite):
    """HBM bytes the fused pair must move (each array once; halo re-reads are served by the caches): the forward reads image, gt
    (+ sky, alpha) and writes the three derivative planes; the backward reads those planes and the inputs again and writes the gradients."""
    n, a = W * H * C, W * H
    inputs = 2 * n + ((n + a) if composite else 0)
    fwd = inputs + 3 * n
    bwd = 3 * n + inputs + n + ((n + a) if composite else 0)
    return 4 * (fwd + bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_loss_time.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_image_loss.py measures on the GPU: there is none")
    dev = "cuda:0"
    rows = []
    for W, H in SIZES:
        for composite in (False, True):
            r = torch.Generator().manual_seed(W + H)
            mk = lambda c: torch.rand(c, H, W, generator=r).to(dev)
            image, gt = mk(3).requires_grad_(), mk(3)
            sky, alpha = (mk(3).requires_grad_(), mk(1).requires_grad_()) if composite else (None, None)
            leaves = [t for t in (image, sky, alpha) if t is not None]

            def step(fn):
                for t in leaves:
                    t.grad = None
                fn(image, gt, 0.2, sky, alpha)[0].backward()

            fns = dict(fused=lambda: step(photometric_loss), torch=lambda: step(photometric_loss_torch))
            iters = max(5, args.iters // 4) if W >= 3840 else args.iters
            # (the warm-up covers every shape: code objects, the convolution backend's choice of algorithm)
            ms = {k: measure.stats(v) for k, v in measure.alternating_rounds(fns, args.rounds, iters, warmup=5).items()}
            med = {k: v["median"] for k, v in ms.items()}
            nbytes = design_bytes(W, H, 3, composite)
            row = dict(width=W, height=H, channels=3, composite=composite, iters_per_round=iters, rounds=args.rounds,
                       fused_ms=ms["fused"], torch_ms=ms["torch"], torch_over_fused=med["torch"] / med["fused"],
                       design_bytes_per_pixel_channel=nbytes / (W * H * 3), design_bytes=nbytes,
                       fused_design_GBps=nbytes / (med["fused"] * 1e-3) / 1e9)
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = dict(measure.header(), what="forward + backward of the loss, per step, autograd included; device events around "
               "iters_per_round steps; median / min / max over the rounds; the two implementations alternate", results=rows)
    measure.write_record(args.out, doc)


if __name__ == "__main__":
    main()

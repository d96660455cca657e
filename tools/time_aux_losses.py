"""Times forward + backward of the fused auxiliary losses against their `*_torch` twins in float32, on one GPU in one process.

    python tools/time_aux_losses.py [--out profiles/aux_loss_time.json] [--rounds 9] [--iters 20]

At 1920x1080 (6 classes) and P = 3 M.  Every (op, implementation) is warmed first; then the two implementations ALTERNATE round by round,
each round being `iters` steps between two device events; the figures are the median over the rounds and their range.  The semantic
baseline is what the reference pays per iteration [REF train.py:87-88]: the one-hot image built from the label map, the upload of the
weight vector, F.cross_entropy and its backward.  Also: the bytes each fused pair has to move (each array once) and the rate that gives.
The numbers are taken with the profiler off."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from streetunveiler_amd import aux_loss as al  # noqa: E402
from tools import measure  # noqa: E402

W, H, CLASSES, P = 1920, 1080, 6, 3_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_loss_time.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_aux_losses.py measures on the GPU: there is none")
    dev = "cuda:0"
    r = torch.Generator().manual_seed(1)
    mk = lambda *shape: torch.rand(*shape, generator=r).to(dev)
    logits = mk(CLASSES, H, W).requires_grad_()
    labels = torch.randint(0, CLASSES, (H, W), generator=r).to(torch.uint8).to(dev)
    rn, sn, rd = mk(3, H, W).requires_grad_(), mk(3, H, W).requires_grad_(), mk(1, H, W).requires_grad_()
    raw = (4 * torch.randn(P, 1, generator=r)).to(dev).requires_grad_()
    weight = list(al.REFERENCE_CLASS_WEIGHT)
    ce = al.SemanticCrossEntropy(weight)
    px = W * H

    def reference_semantic():
        gt = al.one_hot_image(labels, CLASSES)                                       # viewpoint_cam.get_semantic_prob_image()
        return F.cross_entropy(logits.unsqueeze(0), gt.unsqueeze(0), weight=torch.tensor(weight).cuda())

    ops = {   # name: (leaves, fused, torch, bytes the fused pair moves)
        "semantic_cross_entropy": ([logits], lambda: ce(logits, labels), reference_semantic, 2 * (4 * CLASSES * px + px) + 4 * CLASSES * px),
        "surface_regularisers": ([rn, sn, rd], lambda: al.surface_regularisers(rn, sn, rd, 0.05, 100.0)[0],
                                 lambda: al.surface_regularisers_torch(rn, sn, rd, 0.05, 100.0)[0], 4 * px * (7 + 6 + 7)),
        "opacity_shrink": ([raw], lambda: al.opacity_shrink(raw), lambda: al.opacity_shrink_torch(raw), 4 * P * 3),
    }
    rows = []
    for name, (leaves, fused, stock, nbytes) in ops.items():
        def step(fn):
            for t in leaves:
                t.grad = None
            fn().backward()

        fns = dict(fused=lambda: step(fused), torch=lambda: step(stock))
        ms = {k: measure.stats(v) for k, v in measure.alternating_rounds(fns, args.rounds, args.iters, warmup=5).items()}
        med = {k: v["median"] for k, v in ms.items()}
        row = dict(op=name, width=W, height=H, classes=CLASSES, gaussians=P, iters_per_round=args.iters, rounds=args.rounds,
                   fused_ms=ms["fused"], torch_ms=ms["torch"], torch_over_fused=med["torch"] / med["fused"], design_bytes=nbytes, fused_design_GBps=nbytes / (med["fused"] * 1e-3) / 1e9)
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = dict(measure.header(), what="forward + backward of each loss, per step, autograd included; device events around "
               "iters_per_round steps; median / min / max over the rounds; the two implementations alternate; the semantic baseline includes "
               "the one-hot image and the weight upload of the reference's iteration", results=rows)
    measure.write_record(args.out, doc)


if __name__ == "__main__":
    main()

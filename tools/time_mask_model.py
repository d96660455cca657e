"""Times the per-iteration work of the masked re-optimisation model (streetunveiler_amd/mask_model.py) on one GPU in one process.

    python tools/time_mask_model.py [--out profiles/mask_model_time.json] [--gaussians 3000000] [--degree 3] [--shares 0.01,0.05,0.25,1.0]
                                    [--rounds 9] [--iters 10]

Per trainable share (a uniformly random row mask from seed 0 -- scattered rows, the least favourable layout for skipping them):
    compose            the five effective tensors:  fused = compose_masked (one launch), reference = the reference's getter lines in float32
                       torch (compose_masked_torch: twelve element-wise passes and a cat)
    compose_backward   the same plus the backward to the six delta gradients from fixed upstream gradients (torch.autograd.grad)
    adam               one optimizer step over the six deltas:  fused = SurfelAdam(row_mask=mask), reference = torch.optim.Adam(l, lr=0.0,
                       eps=1e-15) as the reference's training_setup builds it (dense: all P rows)
Everything is warmed first; then the two implementations ALTERNATE round by round, a round being `iters` calls between two device events.
Reported: the median over the rounds with its range (min, max), per call.  Taken with the profiler off."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from streetunveiler_amd.mask_model import PROPERTIES, compose_masked, compose_masked_torch  # noqa: E402
from streetunveiler_amd.optim import SurfelAdam  # noqa: E402
from tools import measure  # noqa: E402

LRS = (0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001)     # the reference's six groups


def _shapes(P, degree):
    M = (degree + 1) ** 2
    return [(P, 3), (P, 1, 3), (P, M - 1, 3), (P, 1), (P, 2), (P, 4)], [(P, 3), (P, M, 3), (P, 1), (P, 2), (P, 4)]


def _alternate(fns, rounds, iters):
    return measure.alternating_rounds(fns, rounds, iters, warmup=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_model_time.json"))
    ap.add_argument("--gaussians", type=int, default=3000000)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--shares", default="0.01,0.05,0.25,1.0")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mask_model.py measures on the GPU: there is none")
    dev, P = "cuda:0", args.gaussians
    rows_shapes, out_shapes = _shapes(P, args.degree)
    r = torch.Generator(device=dev).manual_seed(0)
    base = [torch.randn(s, generator=r, device=dev) for s in rows_shapes]
    upstream = [torch.randn(s, generator=r, device=dev) for s in out_shapes]
    floats_per_row = sum(int(torch.Size(s[1:]).numel()) for s in rows_shapes)
    results = []
    for share in (float(s) for s in args.shares.split(",")):
        mask = torch.rand(P, generator=r, device=dev) < share
        start = [0.01 * torch.randn(s, generator=r, device=dev) for s in rows_shapes]
        delta = {k: [d.clone().requires_grad_(True) for d in start] for k in ("fused", "reference")}       # equal values, own leaves
        float_mask = mask.float()          # the reference multiplies by a float mask

        def forward(which):
            if which == "fused":
                return compose_masked(base, delta["fused"], mask)
            return compose_masked_torch(base, delta["reference"], float_mask)

        def forward_only(which):
            with torch.no_grad():
                return forward(which)

        def with_backward(which):
            eff = forward(which)
            return torch.autograd.grad(list(eff), delta[which], grad_outputs=upstream)

        ms = _alternate({"compose_fused": lambda: forward_only("fused"), "compose_reference": lambda: forward_only("reference")}, args.rounds, args.iters)
        ms.update(_alternate({"compose_backward_fused": lambda: with_backward("fused"), "compose_backward_reference": lambda: with_backward("reference")},
                             args.rounds, args.iters))
        # same outputs on both sides, at the size that is timed
        with torch.no_grad():
            same = all(torch.equal(a, b) for a, b in zip(forward("fused"), forward("reference")))
        params = {k: [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in rows_shapes] for k in ("fused", "reference")}
        groups = lambda k: [dict(params=[p], lr=lr, name="new_" + n) for p, lr, n in zip(params[k], LRS, PROPERTIES)]
        opts = {"adam_fused": SurfelAdam(groups("fused"), lr=0.0, eps=1e-15, row_mask=mask),
                "adam_reference": torch.optim.Adam(groups("reference"), lr=0.0, eps=1e-15)}
        for k in ("fused", "reference"):
            for p, s in zip(params[k], rows_shapes):     # the gradient the compose backward leaves: zero in every masked-out row
                p.grad = 1e-3 * torch.randn(s, generator=r, device=dev) * mask.reshape((P,) + (1,) * (len(s) - 1))
        ms.update(_alternate({k: o.step for k, o in opts.items()}, args.rounds, args.iters))
        row = dict(gaussians=P, sh_degree=args.degree, floats_per_gaussian=floats_per_row, trainable_share=share,
                   trainable_rows=int(mask.sum()), mask="torch.rand(P, generator=manual_seed(0) on the GPU, drawn after the tensors) < share",
                   rounds=args.rounds, iters_per_round=args.iters, outputs_equal=bool(same), ms={k: measure.stats(v) for k, v in ms.items()})
        for what in ("compose", "compose_backward", "adam"):
            row[f"{what}_reference_over_fused"] = row["ms"][f"{what}_reference"]["median"] / row["ms"][f"{what}_fused"]["median"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del start, delta, params, opts, mask, float_mask
        torch.cuda.empty_cache()
    doc = dict(measure.header(), torch=torch.__version__,
               what="ms per call; device events around iters_per_round calls; median / min / max over the rounds; fused and reference alternate "
                    "round by round in one process; reference = the reference's getter lines and torch.optim.Adam in float32 torch on the same GPU",
               results=results)
    measure.write_record(args.out, doc)


if __name__ == "__main__":
    main()

"""Times forward + backward per autograd step of SkyModel.render_with_camera (the fused kernels of csrc/sky.hip) against sky_forward_torch
(the reference's lines: full 111-channel input, per-pixel grid lookups) in float32, on one GPU in one process.

    python tools/time_sky.py [--out profiles/sky_time.json] [--rounds 9] [--iters 5]

At 480x320, then 1920x1080; the file is written after each size.  Both implementations are warmed first; then they ALTERNATE round by
round, each round being `iters` steps between two device events; the figures are the median over the rounds and their range.  The torch
baseline at 1920x1080 gets 3 rounds of one step (SIZES says why); the file states the rounds and steps behind every figure.  Also: the peak memory each allocates beyond
what is held before the step.  Whatever is measured is reported, a size at which the fused path is slower included.  Profiler off."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from streetunveiler_amd import sky  # noqa: E402
from tools import measure  # noqa: E402

# (width, height, rounds of the torch baseline): small size first.  At 1920x1080 one step of the baseline gathers 268 M grid rows and its
# backward adds as many duplicates into 128 rows, which takes seconds: it gets 3 rounds of one step; the fused path always gets --rounds.
SIZES = [(480, 320, None), (1920, 1080, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_time.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5, help="steps per round of the fused path (the torch baseline at 1080p: 1)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_sky.py measures on the GPU: there is none")
    dev = "cuda:0"
    torch.manual_seed(1)
    model = sky.SkyModel(device=dev)
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.31, 0.62, 0.17])
    doc = dict(measure.header(), what="forward + backward of the sky image per autograd step (the loss is sum(image * g)); "
               "device events around `iters` steps; median / min / max over the rounds; the two implementations alternate while both have "
               "rounds left; peak_extra_bytes: the most a step allocates beyond what is held before it", results=[])
    for W, H, torch_rounds in SIZES:
        K = torch.tensor([[0.9 * W, 0.0, W / 2], [0.0, 0.9 * W, H / 2], [0.0, 0.0, 1.0]])
        g = torch.randn(3, H, W, device=dev)
        fns = dict(fused=lambda: model.render_with_camera(H, W, K, c2w),
                   torch=lambda: sky.sky_forward_torch(model.position_encoding.params, model.blocks.pairs(), H, W, K, c2w))
        rounds = dict(fused=args.rounds, torch=torch_rounds or args.rounds)
        iters = dict(fused=args.iters, torch=args.iters if torch_rounds is None else 1)

        def step(fn):
            model.optimizer.zero_grad(set_to_none=True)
            (fn() * g).sum().backward()

        peak = {}
        for k, fn in fns.items():                                                    # one step: warm-up and the peak memory
            model.optimizer.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(fn)
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - held
            print(f"{W}x{H} {k}: warmed, peak extra {peak[k]} bytes", flush=True)
        step(fns["fused"])
        ms = measure.alternating_rounds({k: lambda fn=fn: step(fn) for k, fn in fns.items()}, rounds, iters, warmup=0)      # (warmed above)
        print(f"{W}x{H} ms per step, by round:", {k: [round(t, 3) for t in v] for k, v in ms.items()}, flush=True)
        stat = lambda k: dict(measure.stats(ms[k]), rounds=rounds[k], iters_per_round=iters[k])
        row = dict(width=W, height=H, fused_ms=stat("fused"), torch_ms=stat("torch"), torch_over_fused=stat("torch")["median"] / stat("fused")["median"],
                   fused_peak_extra_bytes=peak["fused"], torch_peak_extra_bytes=peak["torch"])
        doc["results"].append(row)
        print(json.dumps(row), flush=True)
        measure.write_record(args.out, doc)                                          # after every size: what is measured is kept


if __name__ == "__main__":
    main()

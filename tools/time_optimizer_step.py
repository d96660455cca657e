"""Times one optimizer step and one densification-statistics call of the reference's training iteration, on one GPU in one process.

    python tools/time_optimizer_step.py [--out profiles/optimizer_step_time.json] [--sizes 3000000,1500000] [--rounds 9] [--iters 20]

Per size (Gaussians; the reference's six parameter shapes, 58 floats each):
    adam_reference   torch.optim.Adam(l, lr=0.0, eps=1e-15) exactly as training_setup builds it (torch picks its multi-tensor path)
    adam_fused       the same with fused=True, where this torch build accepts it
    surfel_adam      SurfelAdam (csrc/optimizer.hip: one launch)
    stats_reference  the reference's three boolean-indexed lines (densification_stats_torch)
    stats_fused      densification_stats (one kernel)
Everything is warmed first; then the implementations ALTERNATE round by round, a round being `iters` calls between two device events.
Reported: median, 10th and 90th percentile over the rounds, per call.  For surfel_adam also the bytes the step has to move (28 B per
element: read p, g, m, v, write p, m, v -- computed from the shapes) over its median time, beside the measured float4-copy rate of the
GPU's memory (6.29 TB/s).  Taken with the profiler off; a kernel trace is a run of its own."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from streetunveiler_amd.optim import SurfelAdam, densification_stats, densification_stats_torch  # noqa: E402
from tests.optim_cases import GROUPS  # noqa: E402  (the reference's six groups: name, row shape, learning rate)
from tools import measure  # noqa: E402

COPY_RATE = 6.29e12   # B/s, float4 copy on this GPU


def _optimizer(cls, P, dev, **kw):
    r = torch.Generator().manual_seed(P % 1000)
    groups = []
    for name, tail, lr in GROUPS:
        p = torch.nn.Parameter(torch.randn((P,) + tail, generator=r).to(dev))
        p.grad = (1e-3 * torch.randn((P,) + tail, generator=r)).to(dev)
        groups.append(dict(params=[p], lr=lr, name=name))
    return cls(groups, lr=0.0, eps=1e-15, **kw)


def _percentiles(v):
    q = statistics.quantiles(v, n=10, method="inclusive")
    return dict(median=statistics.median(v), p10=q[0], p90=q[-1])


def _alternate(fns, rounds, iters):
    return measure.alternating_rounds(fns, rounds, iters, warmup=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_step_time.json"))
    ap.add_argument("--sizes", default="3000000,1500000")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_optimizer_step.py measures on the GPU: there is none")
    dev = "cuda:0"
    rows = []
    for P in (int(s) for s in args.sizes.split(",")):
        opts = dict(adam_reference=_optimizer(torch.optim.Adam, P, dev))
        fused_note = None
        try:
            opts["adam_fused"] = _optimizer(torch.optim.Adam, P, dev, fused=True)
            opts["adam_fused"].step()
            torch.cuda.synchronize()
        except Exception as e:   # this torch build has no fused Adam for the device: reported, not timed
            opts.pop("adam_fused", None)
            fused_note = f"{type(e).__name__}: {e}"
        opts["surfel_adam"] = _optimizer(SurfelAdam, P, dev)
        ms = _alternate({k: o.step for k, o in opts.items()}, args.rounds, args.iters)
        del opts
        torch.cuda.empty_cache()
        r = torch.Generator().manual_seed(1)
        grad = (1e-4 * torch.randn(P, 3, generator=r)).to(dev)
        radii = (torch.randint(0, 40, (P,), generator=r, dtype=torch.int32) * (torch.rand(P, generator=r) < 0.4)).to(torch.int32).to(dev)
        state = {k: (torch.zeros(P, 1, device=dev), torch.zeros(P, 1, device=dev), torch.zeros(P, device=dev)) for k in ("stats_reference", "stats_fused")}
        ms.update(_alternate(dict(stats_reference=lambda: densification_stats_torch(grad, radii, *state["stats_reference"]),
                                  stats_fused=lambda: densification_stats(grad, radii, *state["stats_fused"])), args.rounds, args.iters))
        elements = P * sum(int(torch.Size(t).numel()) for _, t, _ in GROUPS)
        row = dict(gaussians=P, elements=elements, rounds=args.rounds, iters_per_round=args.iters, visible_fraction=float((radii > 0).float().mean()),
                   ms={k: _percentiles(v) for k, v in ms.items()}, adam_fused_unavailable=fused_note)
        step_bytes = 28 * elements
        t = row["ms"]["surfel_adam"]["median"] * 1e-3
        row["surfel_adam_bytes"] = step_bytes
        row["surfel_adam_TBps"] = step_bytes / t / 1e12
        row["surfel_adam_share_of_copy_rate"] = step_bytes / t / COPY_RATE
        a, c = row["ms"]["adam_reference"], row["ms"]["surfel_adam"]
        row["reference_over_surfel_adam"] = a["median"] / c["median"]
        row["faster_than_reference_beyond_both_spreads"] = bool(a["median"] - c["median"] > max(a["p90"] - a["p10"], c["p90"] - c["p10"]))
        if "adam_fused" in row["ms"]:
            row["torch_fused_over_surfel_adam"] = row["ms"]["adam_fused"]["median"] / c["median"]
        row["stats_reference_over_fused"] = row["ms"]["stats_reference"]["median"] / row["ms"]["stats_fused"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del grad, radii, state
        torch.cuda.empty_cache()
    doc = dict(measure.header(), torch=torch.__version__, copy_rate_Bps=COPY_RATE,
               what="ms per call; device events around iters_per_round calls; median / p10 / p90 over the rounds; the implementations alternate "
                    "round by round in one process", results=rows)
    measure.write_record(args.out, doc)


if __name__ == "__main__":
    main()

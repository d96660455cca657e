#!/usr/bin/env python
"""Densify-and-prune timing.  python tools/time_densify.py [--points N] [--json FILE]

Model: N Gaussians (default 3 M) with 16 SH coefficients (f_dc [N,1,3], f_rest [N,15,3]) and Adam state for every group, on a model shaped
like the reference's GaussianModel with SurfelAdam.  The statistics and scales are SYNTHETIC: set so that 5 % of the Gaussians are
cloned, 5 % split and 3 % pruned by opacity.  This mix is not taken from a real training run.

Timed, each as a caller sees it (allocations included), median of 9 runs with the range after 2 warm-up runs, between device events
that end in a synchronise, every run on a fresh copy of the model (the copy is outside the timed window):
    densify_and_prune (the op)         against  the reference's lines in float32 on the same GPU (densify_and_prune_torch with
                                                bookkeeping=False: none of the checker's source / kind / flag tracking; + the optimizer
                                                surgery; torch.cuda.empty_cache() is NOT part of either)
    prune_points (the op, 3 % mask)    against  the reference's prune_points lines
and torch.cuda.max_memory_allocated over each timed call, less what was allocated when it began.
Writes one record to FILE (default profiles/densify_time.json) with the library's source digest."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from streetunveiler_amd import SurfelAdam, densify_and_prune, prune_points
from tests import densify_cases as dc
from tools import measure

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--points", type=int, default=3000000); ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "densify_time.json"))
opt = ap.parse_args()
N, DEV = opt.points, "cuda:0"
assert torch.cuda.is_available(), "tools/time_densify.py measures on the GPU; there is no CPU path"
TH = dict(dc.DEFAULT)

# the synthetic mix: rows [0, 5 %) cloned, [5 %, 10 %) split, [10 %, 13 %) pruned by opacity, the rest untouched; then shuffled
c = dc.make_case(N, rest=45, state=True, seed=1, grad_range=(1e-6, 1e-5), scale_range=(0.005, 0.04), logit_range=(-3.0, 4.0))
n5, n3 = N // 20, (3 * N) // 100
c.accum[:2 * n5] = 1e-2 * c.denom[:2 * n5]
c.params["scaling"][n5:2 * n5] += 2.5            # x 12: 0.06 .. 0.49, beyond percent_dense * extent, children below 0.1 * extent
c.params["opacity"][2 * n5:2 * n5 + n3] = -7.0
perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
for d in (c.params, ):
    for k in d:
        d[k] = d[k][perm].contiguous()
c.moments = {k: tuple(s[perm].contiguous() for s in st) for k, st in c.moments.items()}
c.accum, c.denom, c.semantics, c.cluster_idx, c.max_radii2D = (t[perm].contiguous() for t in (c.accum, c.denom, c.semantics, c.cluster_idx, c.max_radii2D))
want = dc._decisions(c)
S = int(want.split.sum())
noise = torch.randn((2 * S, 2), generator=torch.Generator().manual_seed(1)).to(DEV)
mask = (torch.rand(N, generator=torch.Generator().manual_seed(2)) < 0.03).to(DEV)


def fresh():
    m = dc.Model(c, SurfelAdam, DEV, torch.float32)
    for name, p in m.named().items():
        m.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": c.moments[name][0].to(DEV), "exp_avg_sq": c.moments[name][1].to(DEV)}
    return m


def timed(fn, warmup=2, repeats=9):
    """every run is one per_call_events sample of its own, on a fresh model made outside the window; the first `warmup` runs are dropped"""
    ms, peak = [], []
    for it in range(warmup + repeats):
        m = fresh()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ms += measure.per_call_events(lambda: fn(m), 0, 1, sync_each=True)
        peak.append(torch.cuda.max_memory_allocated() - before)
        rows = m._xyz.shape[0]
        del m
    return dict(measure.stats_ms(ms[warmup:]), peak_extra_bytes=max(peak[warmup:]), rows_out=rows)


th = (TH["max_grad"], TH["min_opacity"], TH["extent"], TH["max_screen_size"])
record = {**measure.header(), "points": N,
          "sh_coefficients": 16, "adam_state": True, "model_bytes": N * 58 * 4 * 3,
          "mix": {"cloned": int(want.clone.sum()), "split": S, "pruned_by_opacity": int((~want.keep_self & ~want.split).sum()),
                  "note": "synthetic: 5 % cloned, 5 % split, 3 % pruned; not taken from a real training run"},
          "densify_and_prune": timed(lambda m: densify_and_prune(m, *th, noise=noise)),
          "densify_and_prune_torch_float32": timed(lambda m: m.reference_densify(*th, noise, bookkeeping=False)),
          "prune_points": timed(lambda m: prune_points(m, mask)),
          "prune_points_torch": timed(lambda m: m.reference_prune(mask))}
for a, b in (("densify_and_prune", "densify_and_prune_torch_float32"), ("prune_points", "prune_points_torch")):
    assert record[a]["rows_out"] == record[b]["rows_out"]
    record[a]["speedup_over_torch"] = round(record[b]["median_ms"] / record[a]["median_ms"], 2)
    print(f"{a}: median {record[a]['median_ms']} ms ({record[a]['min_ms']} .. {record[a]['max_ms']}), peak extra {record[a]['peak_extra_bytes'] / 2**20:.0f} MiB;  "
          f"{b}: median {record[b]['median_ms']} ms ({record[b]['min_ms']} .. {record[b]['max_ms']}), peak extra {record[b]['peak_extra_bytes'] / 2**20:.0f} MiB")
measure.write_record(opt.json, record)

#!/usr/bin/env python
"""Radius clustering timing on a street-like cloud.  python tools/time_cluster.py [--points N] [--baseline-points M] [--json FILE]

Scene: tests/knn_cases.lidar_cloud -- a sparse anisotropic background and a third of the points in dense blobs on a 1 m grid, the
"instances".  Active: 30 % of the blob points and 2 % of the background (a few hundred thousand of 3 M), radius 0.07, the default of
cluster_instance_with_mask.

Timed: streetunveiler_amd.radius_components, as a caller sees it (workspace allocation included): 2 warm-up calls, 9 timed calls between
device events; median, min and max.

Baseline: the reference's default loop (GaussianModel.cluster_instance_with_mask, parallel=True), restated below in torch on the same
device: per active point one distance pass over ALL active points, one min / scatter on the father array, and pointer jumping until a
host read-back says nothing moved.  It is run ON A SUBSAMPLE of the active points, small enough to finish, and reported AS MEASURED: total
seconds for that subsample and seconds per active point at that subsample size.  Nothing is extrapolated: the loop's cost per point grows
with the number of active points, so the per-point figure at the subsample is a lower bound of the per-point cost at the full size.
Writes one record to FILE (default profiles/cluster_time.json) with the library's source digest."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from streetunveiler_amd import radius_components
from tests.knn_cases import lidar_cloud
from tools import measure

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--points", type=int, default=3000000); ap.add_argument("--baseline-points", type=int, default=3000)
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cluster_time.json"))
opt = ap.parse_args()
N, M, RADIUS, DEV = opt.points, opt.baseline_points, 0.07, "cuda:0"
assert torch.cuda.is_available(), "tools/time_cluster.py measures on the GPU; there is no CPU path"

rng = np.random.default_rng(0)
pts = lidar_cloud(N, 0)
mask = np.zeros(N, bool)
mask[:N // 3] = rng.random(N // 3) < 0.30
mask[N // 3:] = rng.random(N - N // 3) < 0.02
perm = rng.permutation(N)                      # a model's points are in no spatial order
pts, mask = pts[perm], mask[perm]
xyz, active = torch.tensor(pts, device=DEV), torch.tensor(mask, device=DEV)


def timed(fn, warmup, repeats):
    return measure.stats_ms(measure.per_call_events(fn, warmup, repeats))


def reference_default_loop(xyz, valid_mask, threshold):
    """cluster_idx as the reference's parallel=True loop leaves it (before pruning)."""
    n = xyz.shape[0]
    father = torch.arange(n, device=xyz.device)

    def densify(father):
        while True:
            up = father[father]
            if bool((up == father).all().item()):
                return father
            father = up
    index = torch.arange(n, device=xyz.device)[valid_mask]
    sel = xyz[valid_mask]
    for i in range(index.shape[0] - 1):
        near = index[(torch.abs(sel[i] - sel) ** 2).sum(dim=-1) ** 0.5 < threshold]
        father[near] = father[near].min()
        father = densify(father)
    out = torch.full((n,), -1, dtype=torch.int64, device=xyz.device)
    out[valid_mask] = densify(father)[valid_mask]
    return out


record = {**measure.header(),
          "scene": f"tests/knn_cases.lidar_cloud({N}, 0), shuffled; active: 30 % of the blob points, 2 % of the background", "points": N,
          "active_points": int(mask.sum()), "radius": RADIUS}
op = timed(lambda: radius_components(xyz, RADIUS, active), warmup=2, repeats=9)
labels = radius_components(xyz, RADIUS, active)
record["radius_components"] = dict(op, components=int(torch.unique(labels[active]).numel()),
                                   us_per_active_point=round(op["median_ms"] * 1e3 / max(1, int(mask.sum())), 4))
print(f"radius_components: {N} points, {int(mask.sum())} active: median {op['median_ms']:.2f} ms (min {op['min_ms']:.2f}, max {op['max_ms']:.2f}), "
      f"{record['radius_components']['components']} components")

# the baseline on the first M active points (in index order, i.e. a random subsample of the active set: the cloud is shuffled)
sub = np.flatnonzero(mask)[:M]
sub_mask = np.zeros(N, bool); sub_mask[sub] = True
sub_active = torch.tensor(sub_mask, device=DEV)
reference_default_loop(xyz, torch.tensor(np.isin(np.arange(N), sub[:50]), device=DEV), RADIUS)      # warm-up of every torch kernel it uses
kept = {}
seconds = [ms / 1e3 for ms in measure.per_call_host(lambda: kept.update(ref=reference_default_loop(xyz, sub_active, RADIUS)), 0, 3)]
ref = kept["ref"]
ours = timed(lambda: radius_components(xyz, RADIUS, sub_active), warmup=2, repeats=9)
# the default loop may split what the exact op keeps whole: every group of the loop must lie inside one component of the op
g, r = radius_components(xyz, RADIUS, sub_active)[sub_active].cpu().numpy(), ref[sub_active].cpu().numpy()
inside = all(len(set(g[r == name].tolist())) == 1 for name in np.unique(r))
same_partition = bool(inside and len(np.unique(g)) == len(np.unique(r)))
record["baseline_groups_lie_inside_op_components"] = bool(inside)
record["reference_default_loop_on_subsample"] = {
    "active_points": len(sub), "seconds_median": round(statistics.median(seconds), 3), "seconds_min": round(min(seconds), 3),
    "seconds_max": round(max(seconds), 3), "repeats": len(seconds),
    "ms_per_active_point_at_this_size": round(statistics.median(seconds) * 1e3 / max(1, len(sub)), 4),
    "radius_components_same_mask": ours, "same_partition_as_radius_components": same_partition,
    "note": "measured at this subsample only; the loop's cost per point grows with the number of active points, nothing is extrapolated"}
print(f"reference default loop on {len(sub)} active points: median {statistics.median(seconds):.2f} s "
      f"({record['reference_default_loop_on_subsample']['ms_per_active_point_at_this_size']:.3f} ms per active point at this size); "
      f"radius_components on the same mask: median {ours['median_ms']:.2f} ms; same partition: {same_partition}")
measure.write_record(opt.json, record)

#!/usr/bin/env python
"""TSDF fusion timing.  python tools/time_tsdf.py [--views V] [--slab N] [--json FILE]

64 views of 1920x1080 (the maps of tests/tsdf_cases.py's ring construction at that size: cameras on a ring around a unit sphere, analytic
depth, random colours) and one 256 x 256 x 256 slab of a 1024^3 grid over [-1.5, 1.5]^3 of contracted space.  Timed, sdf-only and with
rgb, median of 9 runs with the range after 2 warm-up runs, between device events that end in a synchronise:
    unbounded_tsdf_grid (the fused kernel, samples generated)  and  unbounded_tsdf (the same samples read from a list)
    against unbounded_tsdf_torch in float32 on the same GPU WITH THE MAPS RESIDENT -- which favours the baseline: the reference uploads
    every map from the host again on every call, and also samples a normal map it never uses (left out here).
The baseline runs the slab in chunks of 2^22 samples (its temporaries are tens of full-length tensors per view); the chunking is inside
its timed window, as it would be for a caller.  Writes one record to FILE (default profiles/tsdf_time.json)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from streetunveiler_amd import TsdfViews, grid_coordinates, unbounded_tsdf, unbounded_tsdf_grid, unbounded_tsdf_torch
from tests import tsdf_cases as tc
from tools import measure

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--views", type=int, default=64); ap.add_argument("--slab", type=int, default=256)
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tsdf_time.json"))
opt = ap.parse_args()
V, S, DEV, W, H, RES = opt.views, opt.slab, "cuda:0", 1920, 1080, 1024
assert torch.cuda.is_available(), "tools/time_tsdf.py measures on the GPU; there is no CPU path"

depth, rgb, full = tc._views(tuple(360.0 * k / V for k in range(V)), 1, H, W)
depth, rgb, full = depth.to(DEV), rgb.to(DEV), full.to(DEV)
views = TsdfViews(depth, rgb, full)
voxel = tc.RADIUS * 2 / RES
step = 3.0 / (RES - 1)
lo, hi, dims = (-1.5 + 384 * step, -1.5 + 384 * step, -1.5 + 384 * step), (-1.5 + (384 + S - 1) * step,) * 3, (S, S, S)      # the middle of the 1024^3 grid
samples = grid_coordinates(lo, hi, dims).reshape(-1, 3).to(DEV)
n = samples.shape[0]
CHUNK = 1 << 22


def baseline(with_rgb):
    out = [unbounded_tsdf_torch(samples[at:at + CHUNK], depth, rgb, full, voxel, tc.CENTER, tc.RADIUS, return_rgb=with_rgb) for at in range(0, n, CHUNK)]
    return torch.cat([o[0] if with_rgb else o for o in out])


def timed(fn, warmup=2, repeats=9):
    return measure.stats_ms(measure.per_call_events(fn, warmup, repeats, sync_each=True))


record = {**measure.header(),
          "views": V, "map_size": [W, H], "samples": n, "slab_of_grid": [S, S, S, RES],
          "note": "the baseline reads maps that are already on the GPU; the reference uploads every map from the host on every call and samples "
                  "a normal map it never uses, so this setup favours the baseline",
          "bytes_per_sample_and_view": {"sdf_only": {"maps_requested_if_seen": 16, "view_matrix_wave_uniform": 48},
                                        "with_rgb": {"maps_requested_if_seen": 64, "view_matrix_wave_uniform": 48},
                                        "per_sample_once": {"sdf_only_grid": 4, "sdf_only_list": 16, "with_rgb_grid": 16, "with_rgb_list": 28}}}
tsdf_k = unbounded_tsdf_grid(views, lo, hi, dims, voxel, tc.CENTER, tc.RADIUS)
tsdf_b = baseline(False)
record["integrated_by_at_least_one_view"] = float((tsdf_k != 1).float().mean())      # the others lie inside the sphere or in free space beyond trunc
# (a sample within rounding of sdf == -trunc is integrated with s = -1 by one side and skipped by the other: such differences are of order 1)
record["fraction_differing_from_baseline_by_more_than_1e-3"] = float(((tsdf_k.reshape(-1) - tsdf_b).abs() > 1e-3).float().mean())
del tsdf_k, tsdf_b
for key, with_rgb in (("sdf_only", False), ("with_rgb", True)):
    r = {"fused_grid": timed(lambda: unbounded_tsdf_grid(views, lo, hi, dims, voxel, tc.CENTER, tc.RADIUS, return_rgb=with_rgb)),
         "fused_list": timed(lambda: unbounded_tsdf(samples, views, voxel, tc.CENTER, tc.RADIUS, return_rgb=with_rgb)),
         "torch_float32_maps_resident": timed(lambda: baseline(with_rgb), warmup=1, repeats=9)}
    r["speedup_grid_over_torch"] = round(r["torch_float32_maps_resident"]["median_ms"] / r["fused_grid"]["median_ms"], 2)
    r["fused_grid_ns_per_sample_and_view"] = round(r["fused_grid"]["median_ms"] * 1e6 / (n * V), 4)
    record[key] = r
    print(key, json.dumps(r))
measure.write_record(opt.json, record)

#!/usr/bin/env python
"""dist3knn / dist10knn timing at scene-initialisation sizes.  python tools/time_knn.py [n_points ...] [--json FILE] [--label NAME]

One warm-up call, then 7 timed calls per op and size (workspace allocation included, as a caller sees it): median and minimum in ms.
SURFEL_RASTER_LIB=<another build of the library> times that build instead (an A/B against a parent commit's library); --json appends
one record per run to FILE's "runs" list.  `--case NAME` times a cloud shape of tests/knn_cases.py instead of the synthetic scene."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from simple_knn._C import dist3knn, dist10knn
from streetunveiler_amd.synthetic import synthetic_gaussians
from tools import measure

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("n_points", nargs="*", type=int, default=[3_000_000]); ap.add_argument("--json"); ap.add_argument("--label", default=""); ap.add_argument("--case")
opt = ap.parse_args()
record = {"label": opt.label, **measure.header(), "ms": {}}
for n in opt.n_points:
    if opt.case:
        from tests import knn_cases
        pts = torch.tensor(knn_cases.shape_cloud(opt.case), device="cuda:0"); n = len(pts)
    else:
        pts = synthetic_gaussians(n, 1920, 1080, seed=0)["means3D"].to("cuda:0")
    for name, fn in (("dist3knn", dist3knn), ("dist10knn", dist10knn)):
        times = measure.per_call_events(lambda: fn(pts), 1, 7)
        record["ms"][f"{name}_{n}"] = {"median": round(statistics.median(times), 3), "min": round(min(times), 3)}
        print(f"{name}({n} points): median {statistics.median(times):.2f} ms, min {min(times):.2f} ms")
if opt.json:
    doc = json.load(open(opt.json)) if os.path.exists(opt.json) else {"runs": []}
    doc["runs"].append(record)
    measure.write_record(opt.json, doc)

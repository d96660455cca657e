#!/usr/bin/env python
"""dist3knn / dist10knn timing at scene-initialisation sizes.  python tools/time_knn.py [n_points ...] [--json FILE] [--label NAME]

One warm-up call, then 7 timed calls per op and size (workspace allocation included, as a caller sees it): median and minimum in ms.
SURFEL_RASTER_LIB=<another build of the library> times that build instead (an A/B against a parent commit's library); --json appends
one record per run to FILE's "runs" list.  `--case NAME` times a cloud shape of tests/knn_cases.py instead of the synthetic scene."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from simple_knn._C import dist3knn, dist10knn
from streetunveiler_amd import _lib
from streetunveiler_amd.synthetic import synthetic_gaussians

args = sys.argv[1:]
opt = {}
for flag in ("--json", "--label", "--case"):
    if flag in args:
        i = args.index(flag); opt[flag] = args[i + 1]; del args[i:i + 2]
sizes = [int(a) for a in args] or [3_000_000]
record = {"label": opt.get("--label", ""), "library": os.path.relpath(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0), "ms": {}}
for n in sizes:
    if "--case" in opt:
        from tests import knn_cases
        pts = torch.tensor(knn_cases.shape_cloud(opt["--case"]), device="cuda:0"); n = len(pts)
    else:
        pts = synthetic_gaussians(n, 1920, 1080, seed=0)["means3D"].to("cuda:0")
    for name, fn in (("dist3knn", dist3knn), ("dist10knn", dist10knn)):
        fn(pts); torch.cuda.synchronize()
        times = []
        for _ in range(7):
            t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
            t0.record(); fn(pts); t1.record(); torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1))
        record["ms"][f"{name}_{n}"] = {"median": round(statistics.median(times), 3), "min": round(min(times), 3)}
        print(f"{name}({n} points): median {statistics.median(times):.2f} ms, min {min(times):.2f} ms")
if "--json" in opt:
    doc = json.load(open(opt["--json"])) if os.path.exists(opt["--json"]) else {"runs": []}
    doc["runs"].append(record)
    json.dump(doc, open(opt["--json"], "w"), indent=1)

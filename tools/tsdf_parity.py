#!/usr/bin/env python
"""Per case of tests/tsdf_cases.py and per output (tsdf, r, g, b): the deviation of the fused kernel from the float64 checker over the
admitted samples, dev32 (the float32 checker's own deviation, both on the CPU), and their ratio -- the tests hold it to 2.
python tools/tsdf_parity.py [--json FILE]   (default profiles/tsdf_parity.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from streetunveiler_amd import TsdfViews, unbounded_tsdf
from streetunveiler_amd.build import source_digest
from tests import tsdf_cases as tc

out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "tsdf_parity.json")
DEV = "cuda:0"
assert torch.cuda.is_available(), "tools/tsdf_parity.py runs the op; there is no CPU path"
record = {"device": torch.cuda.get_device_name(0), "source_digest": source_digest(), "bar": tc.BAR, "margin": tc.MARGIN, "cases": {}}
worst = 0.0
for name in sorted(tc.CASES):
    c, want = tc.case(name), tc.expected(name)
    views = TsdfViews(c.depth.to(DEV), c.rgb.to(DEV), c.full_proj.to(DEV))
    got = unbounded_tsdf(c.samples.to(DEV), views, c.voxel_size, c.center, c.radius, return_rgb=True, return_weight=True)
    devs = tc.compare(*got, want, name)
    entry = {"samples": int(c.samples.shape[0]), "excluded": int((~want.admitted).sum())}
    for k, (dev, dev32) in devs.items():
        entry[k] = {"kernel": dev, "dev32": dev32, "ratio": (dev / dev32 if dev32 > 0 else (0.0 if dev == 0 else float("inf")))}
        worst = max(worst, entry[k]["ratio"])
    record["cases"][name] = entry
record["worst_ratio"] = worst
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(record, open(out, "w"), indent=1)
print("worst ratio", worst, "-- wrote", out)

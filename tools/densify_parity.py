#!/usr/bin/env python
"""Per case of tests/densify_cases.py: the deviation of the op's child xyz and child _scaling from the float64 checker, the float32 torch
restatement's own deviation on the same GPU, and the bound the tests hold (twice the latter, at least one float32 ulp of the largest
magnitude).  python tools/densify_parity.py [--json FILE]   (default profiles/densify_parity.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from streetunveiler_amd import densify_and_prune_tensors
from streetunveiler_amd.build import source_digest
from tests import densify_cases as dc

out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "densify_parity.json")
DEV = "cuda:0"
assert torch.cuda.is_available(), "tools/densify_parity.py runs the op; there is no CPU path"
record = {"device": torch.cuda.get_device_name(0), "source_digest": source_digest(), "cases": {}}
for name in sorted(dc.CASES):
    c, want = dc.case(name), dc.expected(name)
    to = lambda t: t.to(DEV)
    moments = {k: (None if st is None else tuple(to(s) for s in st)) for k, st in c.moments.items()}
    got = densify_and_prune_tensors({k: to(v) for k, v in c.params.items()}, moments, to(c.semantics), to(c.accum), to(c.denom), to(c.max_radii2D),
                                    c.th["max_grad"], c.th["min_opacity"], c.th["extent"], c.th["max_screen_size"], c.th["percent_dense"],
                                    noise=to(dc.noise_for(c, want.counts[2])), extra_rows=(to(c.cluster_idx),))
    devs = dc.compare(got, want, dc.run_checker(c, torch.float32, DEV), name)
    record["cases"][name] = {"counts": list(want.counts), **{k: {"op": v[0], "torch_float32": v[1], "bound": v[2]} for k, v in devs.items()}}
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(record, open(out, "w"), indent=1)
print("wrote", out)

#!/usr/bin/env python
"""Marching-cubes parity.  python tools/mesh_parity.py [--json FILE]

Every case of tests/mesh_cases.py through streetunveiler_amd.marching_cubes on the GPU against the float64 checker under the bar of
tests/mesh_cases.py (`compare`: faces integer for integer, vertices within 4 x max(the float32 checker's deviation, 1e-6 of the scale)).
Records per case Nv, Nf, the deviation, the float32 checker's, the bound and their ratio, and the worst ratio of all; a case that misses
the bar is recorded with its message and makes the exit status 1.  Writes FILE (default profiles/mesh_parity.json)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from streetunveiler_amd import _lib, marching_cubes
from streetunveiler_amd.build import source_digest
from tests import mesh_cases as mc

args = sys.argv[1:]
out = args[args.index("--json") + 1] if "--json" in args else os.path.join(ROOT, "profiles", "mesh_parity.json")
assert torch.cuda.is_available(), "tools/mesh_parity.py measures on the GPU; there is no CPU path"
record = {"device": torch.cuda.get_device_name(0), "source_digest": source_digest(), "library": os.path.relpath(_lib.LIB_PATH, ROOT),
          "bar": {"factor": mc.BAR, "floor_of_scale": mc.FLOOR}, "cases": {}}
worst, failed = 0.0, []
for name in sorted(mc.CASES):
    c, want = mc.case(name), mc.expected(name)
    vertices, faces = marching_cubes(torch.from_numpy(c.volume).to("cuda:0"), c.level, c.lo, c.hi, c.center, c.radius)
    row = {"shape": list(c.volume.shape), "Nv": int(vertices.shape[0]), "Nf": int(faces.shape[0]), "float32_checker_deviation": want.dev32,
           "scale": want.scale, "bound": want.bound}
    try:
        dev, bound = mc.compare(vertices, faces, want, name)
        row.update(deviation=dev, ratio_to_bound=dev / bound, faces_equal=True)
        worst = max(worst, dev / bound)
    except AssertionError as e:
        row["failed"] = str(e)
        failed.append(name)
    record["cases"][name] = row
record["worst_ratio_to_bound"], record["failed"] = worst, failed
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(record, open(out, "w"), indent=1)
print("worst ratio to the bound", worst, "failed", failed, "-> wrote", out)
sys.exit(1 if failed else 0)

"""The worst ratio of every auxiliary-loss case to the bar of tests/aux_loss_cases.py, per op and case, on one GPU.

    python tools/aux_loss_parity.py [--out profiles/aux_loss_parity.json]

ratio = |fused - truth| / max(2 x |float32 twin - truth|, half a float32 ulp of the truth), the maximum over the elements of each
quantity: <= 1 passes.  `fused_ulps` is the same deviation in float32 ulps of the truth, `twin_ulps` the float32 twin's: how far the
factor 2 is from being needed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import aux_loss_cases as ac  # noqa: E402


def ulps(value, truth):
    truth = np.asarray(truth, dtype=np.float64)
    fin = np.isfinite(truth)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(value, dtype=np.float64) - truth) / ac.ulp32(truth)
    d = np.where(fin & np.isfinite(d), d, 0.0)
    return float(d.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_loss_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aux_loss_parity.py measures on the GPU: there is none")
    dev = "cuda:0"
    rows = []
    for op, cases, reference, run in (("semantic_cross_entropy", ac.SEMANTIC, ac.semantic_reference, ac.run_hip_semantic),
                                      ("surface_regularisers", ac.SURFACE, ac.surface_reference, ac.run_hip_surface),
                                      ("opacity_shrink", ac.SHRINK, ac.shrink_reference, ac.run_hip_shrink)):
        for case in cases:
            truth, yard = reference(case)
            got = run(case, dev)
            rows.append(dict(op=op, case=case["name"], ratio=ac.worst(got, truth, yard),
                             fused_ulps={k: ulps(got[k], truth[k]) for k in truth}, twin_ulps={k: ulps(yard[k], truth[k]) for k in truth}))
            print(json.dumps(rows[-1]), flush=True)
    worst = {op: max(max(r["ratio"].values()) for r in rows if r["op"] == op) for op in {r["op"] for r in rows}}
    doc = dict(device=torch.cuda.get_device_name(0), bar=ac.BAR, floor="half a float32 ulp of the truth", worst_ratio_per_op=worst,
               worst_fused_ulps=max(max(r["fused_ulps"].values()) for r in rows), worst_twin_ulps=max(max(r["twin_ulps"].values()) for r in rows),
               cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("->", args.out)


if __name__ == "__main__":
    main()

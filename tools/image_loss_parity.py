"""Writes profiles/image_loss_parity.json: every ratio the bar of tests/image_loss_cases.py bounds, measured on the GPU.

    python tools/image_loss_parity.py [--out profiles/image_loss_parity.json]

Per case and per quantity: (deviation of the HIP kernels from the float64 truth) / max(d_ref, floor), d_ref = the deviation of the
reference's own float32 run (fixture cases) or of photometric_loss_torch in float32 on the CPU (the other sizes).  The same cases, the same
functions as tests/test_gpu_image_loss.py; the tests assert ratio <= 4, this tool records the figures.

The edge cases (ilc.EDGE_CASES) follow under "edge_cases", each with the ratios of both bars: "per_element" (e = |v - truth| / (|truth| + u),
u = 1 / (C*H*W); max and 99.9th percentile over the twin's same statistic or the floor; scalars as above) and "max_norm" (the rule above, on
the quantities it can judge: a finite truth that is not identically zero).  null: no ratio exists (a NaN scalar, an all-zero truth)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import image_loss_cases as ilc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_loss_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("image_loss_parity.py measures the HIP kernels: it needs a GPU")
    cases = ilc.fixture_cases()
    for W, H in ilc.GPU_SIZES:
        cases += [ilc.with_cpu_reference(ilc.seeded_case(W, H, composite)) for composite in ((True,) if (W, H) == ilc.GPU_SIZES[-1] else (False, True))]
    rows, worst = [], ("", "", 0.0)
    for case in cases:
        r = ilc.ratios(ilc.run_hip(case), case)
        d_ref = {k: ilc.deviation(case["ref"][k], case["truth"][k], k) for k in r}
        rows.append(dict(case=case["name"], shape=list(case["image"].shape), lambda_dssim=case["lambda_dssim"], ratio=r, d_ref=d_ref))
        for k, v in r.items():
            if v > worst[2]:
                worst = (case["name"], k, v)
        print(case["name"], {k: round(v, 3) for k, v in r.items()}, flush=True)
    edge_rows, edge_worst = [], ("", "", "", 0.0)
    for name in ilc.EDGE_CASES:
        case = ilc.edge_case(name)
        got = ilc.run_hip(case)
        per_element = ilc.edge_ratios(got, case)
        max_norm = ilc.ratios(*ilc.where_the_old_rule_applies(got, case))
        edge_rows.append(dict(case=name, shape=list(case["image"].shape), lambda_dssim=case["lambda_dssim"], per_element=per_element, max_norm=max_norm,
                              violations=[list(v) for v in ilc.edge_violations(got, case)]))
        for k, v in per_element.items():
            for stat, r in (v.items() if isinstance(v, dict) else [("", v)] if v is not None else []):
                if r > edge_worst[3]:
                    edge_worst = (name, k, stat, r)
        print(name, per_element, {k: round(v, 3) for k, v in max_norm.items()}, flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), bar=ilc.BAR, floor=ilc.FLOOR, largest=dict(case=worst[0], quantity=worst[1], ratio=worst[2]), cases=rows,
               largest_per_element=dict(case=edge_worst[0], quantity=edge_worst[1], statistic=edge_worst[2], ratio=edge_worst[3]), edge_cases=edge_rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("largest ratio %.3f (%s, %s); largest per-element ratio %.3f (%s, %s %s) -> %s" % (worst[2], worst[0], worst[1], edge_worst[3], *edge_worst[:3], args.out))


if __name__ == "__main__":
    main()

"""Records, for every case of tests/sky_cases.py, the ratio of each tensor's deviation to the bar (<= 1 passes), through
SkyModel.render_with_camera + autograd and through the raw C-ABI pair.

    python tools/sky_parity.py [--out profiles/sky_parity.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import sky_cases as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sky_parity.py runs the kernels: there is no GPU")
    dev, rows = "cuda:0", []
    for case in sc.CASES:
        truth, yard = sc.reference(case)
        row = dict(case=case["name"], model=sc.ratios(sc.run_model(case, dev), truth, yard),
                   raw=sc.ratios(sc.run_raw(case, dev), sc.fused_view(truth), sc.fused_view(yard)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    worst = max(v for row in rows for part in ("model", "raw") for v in row[part].values())
    doc = dict(device=torch.cuda.get_device_name(0), bar=sc.BAR, floor=sc.FLOOR, what="per case and tensor: max|got - truth| / (bar x max(max|float32 "
               "twin - truth|, floor x max|truth|)); <= 1 passes", worst=worst, results=rows)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("worst", worst, "->", args.out)


if __name__ == "__main__":
    main()

"""Writes profiles/optimizer_parity.json: the ratios the accuracy bar of tests/optim_cases.py bounds, measured on the GPU.

    python tools/optimizer_parity.py [--out profiles/optimizer_parity.json]

Two runs of the reference's six parameter groups at P = 1037 with gradients spanning 1e-6 .. 1e1 (a seventh of them zero): 50 steps, and
3 + 3 steps around the reference's prune / concatenate / replace surgery.  Per run and per quantity (p, m, v): the largest absolute
deviation of SurfelAdam from the float64 checker, that of torch.optim.Adam(foreach=False) in float32 on the same GPU, and their ratio.
The same functions as tests/test_gpu_optim.py; the tests assert ratio <= 4, this tool records the figures."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import optim_cases as oc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optimizer_parity.py measures the HIP kernel: it needs a GPU")
    dev = "cuda:0"
    rows = []
    d_hip, d_ref, r = oc.accuracy_run(dev)
    rows.append(dict(run="50 steps", P=1037, surfel_adam=d_hip, torch_float32=d_ref, ratio=r))
    P_of = lambda o: o.param_groups[0]["params"][0].shape[0]
    opts = list(oc.three_optimizers(1037, dev, seed=2))
    oc.run_steps(opts, P_of, 1, 3, seed=5)
    for opt in opts:
        oc.surgery(opt, seed=2)
    oc.run_steps(opts, P_of, 4, 3, seed=5)
    d_hip, d_ref = oc.deviations(opts[0], opts[2]), oc.deviations(opts[1], opts[2])
    rows.append(dict(run="3 steps, prune / concatenate / replace, 3 steps", P=P_of(opts[0]), surfel_adam=d_hip, torch_float32=d_ref, ratio=oc.ratios(d_hip, d_ref)))
    largest = max(v for row in rows for v in row["ratio"].values())
    doc = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, bar=oc.BAR, betas=list(oc.BETAS), eps=oc.EPS,
               what="largest |value - float64 checker| over the six parameter groups, per quantity", largest_ratio=largest, runs=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for row in rows:
        print(row["run"], {k: round(v, 3) for k, v in row["ratio"].items()})
    print("largest ratio %.3f -> %s" % (largest, args.out))


if __name__ == "__main__":
    main()

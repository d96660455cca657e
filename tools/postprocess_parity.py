"""Writes profiles/postprocess_parity.json: every figure the bar of tests/postprocess_cases.py bounds, measured on the GPU.

    python tools/postprocess_parity.py [--out profiles/postprocess_parity.json]

Per case (size x depth ratio x camera x upstream set) and per quantity (output map, gradient channel): the statistics of csrc/postprocess.hip
against the float64 truth (max and 99.9th percentile of |value - truth| / (|truth| + f_c)), the same statistics of the float32 restatement
on the CPU, their ratio over max(restatement, floor) -- the tests assert ratio <= 4, this tool records the figures -- and, per gradient
channel, what the single tolerance 2e-4 * max|g| over all seven channels would have accepted, as a multiple of that channel's own largest
value.  The same cases and functions as tests/test_gpu_postprocess.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import postprocess_cases as pc  # noqa: E402

VIEWS = ("rend_alpha", "rend_dist")     # slices of the input, not written by a kernel


def _r(x):
    return float("%.4g" % x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postprocess_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("postprocess_parity.py measures the HIP kernels: it needs a GPU")
    rows, largest = [], {}
    for a in pc.all_cases():
        c = pc.case(*a)
        got = pc.run_hip(c["cam"], c["ratio"], c["allmap"], c["upstream"])
        s, sr = pc.stats(got, c["truth"]), pc.stats(c["ref"], c["truth"])
        g = np.nan_to_num(c["truth"]["g_allmap"], nan=0.0, posinf=0.0, neginf=0.0)
        old_tolerance = 2e-4 * float(np.abs(g).max())
        q = {}
        for k in s:
            if k in VIEWS:
                continue
            q[k] = {"hip": [_r(s[k][n]) for n in pc.STATS], "float32": [_r(sr[k][n]) for n in pc.STATS],
                    "ratio": [_r(s[k][n] / max(sr[k][n], pc.FLOOR)) for n in pc.STATS], "zero": s[k]["zero"], "exact_zero": s[k]["exact_zero"]}
            if k.startswith("g_allmap"):
                cmax = float(np.abs(g[int(k[9])]).max())
                q[k]["old_tolerance_over_channel_max"] = _r(old_tolerance / cmax) if cmax else None
            for n, r in zip(pc.STATS, q[k]["ratio"]):
                if r > largest.get((k, n), ("", -1.0))[1]:
                    largest[(k, n)] = (c["name"], r)
        rows.append(dict(case=c["name"], old_tolerance=_r(old_tolerance), within_bar=not pc.violations(got, c["truth"], c["ref"]), quantities=q))
        print(c["name"], {k: [float("%.3g" % r) for r in v["ratio"]] for k, v in q.items()}, flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), bar=pc.BAR, floor=pc.FLOOR, statistics=list(pc.STATS),
               largest_ratio={k: {n: dict(case=largest[(k, n)][0], ratio=largest[(k, n)][1]) for n in pc.STATS} for k in sorted({k for k, _ in largest})},
               cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    for k, v in doc["largest_ratio"].items():
        print("largest ratio", k, {n: "%.3f (%s)" % (v[n]["ratio"], v[n]["case"]) for n in pc.STATS})
    print("all within the bar:", all(r["within_bar"] for r in rows), "->", args.out)


if __name__ == "__main__":
    main()

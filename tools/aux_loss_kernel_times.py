"""Reduces a kernel trace of tools/time_aux_losses.py to profiles/aux_loss_kernel_times.json: the device-side time of each form.

    rocprofv3 --kernel-trace --stats -d <dir> -o aux -- python tools/time_aux_losses.py --rounds 3 --iters 10 --out <dir>/time.json
    python tools/aux_loss_kernel_times.py <dir>/aux_results.db [--out profiles/aux_loss_kernel_times.json]

Reads the `kernels` view of the trace database (name, start, duration in ns).  Per fused kernel (`sr::...`): the median duration.  Per
op, the stock kernels of one step of the float32 twin: the timing tool runs its ops one after the other and, inside an op, blocks of
steps of the fused form and of the twin in turn, so every run of more than 20 kernels that are not the library's, between two of the
library's, is one block of twin steps (5 warm-up steps, then `--iters` per round); its summed duration over its steps is one sample."""
import argparse
import json
import os
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = (("semantic", "semantic_cross_entropy"), ("surface", "surface_regularisers"), ("opacity", "opacity_shrink"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("database")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_loss_kernel_times.json"))
    ap.add_argument("--iters", type=int, default=10, help="the --iters the traced run of time_aux_losses.py was given")
    ap.add_argument("--warmup", type=int, default=5, help="its warm-up steps per form")
    args = ap.parse_args()
    rows = sqlite3.connect(args.database).execute("select name, duration from kernels order by start").fetchall()
    if not rows:
        sys.exit("no kernel in the trace")
    fused, blocks, op, run = {}, {}, None, []

    def close():
        if op and len(run) > 20:
            blocks.setdefault(op, []).append(sum(run))
        run.clear()

    for name, duration in rows:
        if "sr::" in name:
            close()
            op = next((full for key, full in OPS if key in name), op)       # (the finalize kernel belongs to the op around it)
            fused.setdefault(name.replace("void ", ""), []).append(duration)
        else:
            run.append(duration)
    close()
    stock = {}
    for name, sums in blocks.items():
        per_step = [t / steps / 1e3 for t, steps in zip(sums, [args.warmup] + [args.iters] * (len(sums) - 1))]
        stock[name] = dict(blocks=len(per_step), stock_us_per_step_median=statistics.median(per_step), min=min(per_step), max=max(per_step))
    doc = dict(what=f"tools/aux_loss_kernel_times.py over a rocprofv3 --kernel-trace of tools/time_aux_losses.py --rounds 3 --iters {args.iters} "
                    "(1920x1080, 6 classes, uint8 labels; P = 3 M): median duration of each fused kernel in microseconds, and the summed "
                    "duration of the stock kernels of one forward + backward step of each float32 twin (semantic: one-hot image and weight "
                    "upload included)",
               kernels={k: dict(median_us=statistics.median(v) / 1e3, calls=len(v)) for k, v in sorted(fused.items())},
               stock_kernels_of_the_torch_twins=stock)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(stock), "->", args.out)


if __name__ == "__main__":
    main()

"""Times the LiDAR voxel downsample (streetunveiler_amd/voxel.py) on one GPU and writes profiles/voxel_init_time.json: the median of 9 runs
with their range, in milliseconds, host clock around work that ends in a device synchronise -- read-backs and allocations included.

The scene is a synthetic street: a ground strip and two facade planes of 400 m, about 20 M float32 points with colours and 6 labels,
voxel_size 0.1.  Rows:
    fused               voxel_down_sample
    torch_float32       voxel_down_sample_torch(mean_dtype=float32) on the same GPU: the stock-torch baseline
    loop_per_voxel      the reference's way -- a Python loop over the voxels, once per attribute, torch.mode and torch.unique per voxel --
                        restated here and run on the CPU on a SUBSAMPLE of about 20 000 voxels: reported as time per voxel, NOT extrapolated
Peak extra device memory of the two GPU rows is torch.cuda.max_memory_allocated() above what was allocated before the call.

    python tools/time_voxel_init.py [--points 20000000] [--out profiles/voxel_init_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from streetunveiler_amd import voxel as V  # noqa: E402
from tools import measure  # noqa: E402

DEV = "cuda:0"
REPEATS = 9
VOXEL = 0.1


def timed(fn, warmup=2):
    return {k + "_ms": v for k, v in measure.stats(measure.per_call_host(fn, warmup, REPEATS)).items()}


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def street(n, seed=0):
    """Ground: 400 m x 20 m, 2 cm of noise in z.  Facades: y = -10 and y = +10, 10 m high, 2 cm of noise in y.  Labels by region (two lanes,
    each facade in two halves), 5 % of them redrawn."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    u = lambda k: torch.rand((k,), device=DEV, generator=g)
    nrm = lambda k: torch.randn((k,), device=DEV, generator=g)
    ng = n // 2
    nf = (n - ng) // 2
    parts, labels = [], []
    x, y = u(ng) * 400, u(ng) * 20 - 10
    parts.append(torch.stack([x, y, nrm(ng) * 0.02], 1))
    labels.append((y > 0).to(torch.int32))
    for side, k in ((-1.0, nf), (1.0, n - ng - nf)):
        x = u(k) * 400
        parts.append(torch.stack([x, side * 10 + nrm(k) * 0.02, u(k) * 10], 1))
        labels.append((2 if side < 0 else 4) + (x > 200).to(torch.int32))
    pts, sem = torch.cat(parts), torch.cat(labels)
    noisy = torch.rand((n,), device=DEV, generator=g) < 0.05
    sem = torch.where(noisy, torch.randint(0, 6, (n,), device=DEV, generator=g, dtype=torch.int32), sem)
    order = torch.randperm(n, device=DEV, generator=g)
    return pts[order].contiguous(), torch.rand((n, 3), device=DEV, generator=g), sem[order].contiguous()


def loop_per_voxel(points, colors, semantics, voxel_size):
    """The reference's way on the CPU: sort, unique, then a Python loop over the voxels per attribute."""
    index, _ = V.voxel_index_torch(points, voxel_size)
    order = torch.sort(index)[1]
    voxels, counts = torch.unique(index[order], return_counts=True)
    groups = torch.split(torch.arange(index.shape[0]), tuple(counts.tolist()))
    out_points, out_colors = torch.zeros((voxels.shape[0], 3)), torch.zeros((voxels.shape[0], 3))
    for attr, out in ((points[order], out_points), (colors[order], out_colors)):
        for k, members in enumerate(groups):
            out[k] = attr[members].mean(0)
    labels, valid = torch.zeros((voxels.shape[0],), dtype=torch.int32), torch.ones((voxels.shape[0],), dtype=torch.bool)
    sem = semantics[order]
    for k, members in enumerate(groups):
        own = sem[members]
        labels[k] = torch.mode(own, dim=0).values.item()
        if 1.0 * torch.unique(own, return_counts=True)[1].max() / len(own) < 0.8:
            valid[k] = False
    return out_points[valid], out_colors[valid], labels[valid], int(voxels.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--loop-voxels", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_init_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_voxel_init.py measures on a GPU; there is nothing to time without one"
    pts, col, sem = street(args.points)
    fused = lambda: V.voxel_down_sample(pts, VOXEL, col, None, sem, return_counts=True)
    twin = lambda: V.voxel_down_sample_torch(pts, VOXEL, col, None, sem, mean_dtype=torch.float32, return_counts=True)
    cloud, counts = fused()
    ref = twin()
    rows = {"scene": {"points": args.points, "voxel_size": VOXEL, "labels": 6, "dtype": "float32", "colors": True,
                      "kept_voxels": int(cloud.points.shape[0]), "largest_voxel_members": int(counts.max()),
                      "occupied_voxels": int(torch.unique(V.voxel_index_torch(pts, VOXEL)[0]).shape[0]),
                      "same_rows_as_torch_float32": bool(ref[0].shape[0] == cloud.points.shape[0] and torch.equal(ref[3], cloud.semantics))}}
    del cloud, counts, ref
    rows["fused"] = dict(timed(fused), peak_extra_bytes=peak_extra_bytes(fused))
    rows["torch_float32"] = dict(timed(twin), peak_extra_bytes=peak_extra_bytes(twin))
    # the loop, on the CPU, on a slab of the street that holds about --loop-voxels voxels
    occupied = rows["scene"]["occupied_voxels"]
    slab = 400.0 * min(1.0, args.loop_voxels / max(occupied, 1))
    pick = pts[:, 0] < slab
    p, c, s = pts[pick].cpu(), col[pick].cpu(), sem[pick].cpu()
    kept = {}
    seconds = measure.per_call_host(lambda: kept.update(voxels=loop_per_voxel(p, c, s, VOXEL)[-1]), 0, 1)[0] / 1e3
    n_voxels = kept["voxels"]
    rows["loop_per_voxel"] = {"device": "cpu", "points": int(p.shape[0]), "voxels": n_voxels, "seconds": seconds, "runs": 1,
                              "ms_per_voxel": 1e3 * seconds / max(n_voxels, 1), "extrapolated": False}
    rows.update(measure.header())
    print(json.dumps(rows, indent=1))
    measure.write_record(args.out, rows)


if __name__ == "__main__":
    main()

"""Times the LiDAR colouring and labelling on the GPU and writes profiles/lidar_label_time.json.

    python tools/time_lidar_label.py [--sweeps 200] [--returns 170000] [--vote-points 1000000] [--vote-views 600] [--rounds 9]

A synthetic street: a vehicle drives along x at a world offset of 1e5 m; per sweep `returns` points in a box round it and three cameras
(ahead, 45 degrees left and right) of 1920x1280 with random pictures and label maps of 6 labels in patches of about 100 pixels.  Measured,
read-backs and allocations included, median of `rounds` with range:
    label_sweeps (merge and per_view) over all sweeps in one call, against label_sweeps_torch in float64 on the same GPU;
    vote_semantics of `vote-points` points through `vote-views` views, against vote_semantics_torch;
    the numpy checker (the reference's two helpers restated) on this machine's CPU for ONE sweep -- one run, not extrapolated.
The twins loop over the views in Python as the reference does; they are stock-torch baselines, not an estimate of anything else."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from streetunveiler_amd import lidar_label as LL      # noqa: E402
from tools import measure      # noqa: E402

DEV = "cuda:0"
H, W = 1280, 1920


def scene(n_sweeps, returns, cameras, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    origin = np.array([1.0e5, -2.0e5, 30.0])
    w2c, K, pts = [], [], []
    k = np.array([[2000.0, 0.0, W / 2], [0.0, 2000.0, H / 2], [0.0, 0.0, 1.0]])
    for s in range(n_sweeps):
        pos = origin + np.array([0.5 * s, 0.0, 1.8])
        box = torch.rand((returns, 3), generator=g, device=DEV, dtype=torch.float64) * torch.tensor([80.0, 80.0, 8.0], device=DEV, dtype=torch.float64) - \
            torch.tensor([40.0, 40.0, 3.0], device=DEV, dtype=torch.float64)
        pts.append(box + torch.from_numpy(pos).to(DEV))
        for c in range(cameras):
            yaw = (0.0, np.pi / 4, -np.pi / 4)[c % 3] + 0.01 * (c // 3)
            fwd, left, up = np.array([np.cos(yaw), np.sin(yaw), 0.0]), np.array([-np.sin(yaw), np.cos(yaw), 0.0]), np.array([0.0, 0.0, 1.0])
            R = np.stack([-left, -up, fwd])                # camera x right, y down, z ahead
            m = np.eye(4)
            m[:3, :3], m[:3, 3] = R, -R @ pos
            w2c.append(m)
            K.append(k)
    return torch.cat(pts), np.stack(w2c), np.stack(K)


def pictures(n, with_images, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows, cols = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    maps = [((rows // 97 * 3 + cols // 131 + f) % 6).to(torch.uint8) for f in range(n)]
    images = [torch.randint(0, 256, (H, W, 3), generator=g, device=DEV, dtype=torch.uint8) for _ in range(n)] if with_images else None
    return images, maps


def timed(fn, rounds):
    return dict({k + "_ms": v for k, v in measure.stats(measure.per_call_host(fn, 1, rounds)).items()}, rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--returns", type=int, default=170000)
    ap.add_argument("--vote-points", type=int, default=1000000)
    ap.add_argument("--vote-views", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--baseline-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_label_time.json"))
    a = ap.parse_args()
    result = {**measure.header(), "picture": [H, W], "labels": 6, "check_range": 10}

    points, w2c, K = scene(a.sweeps, a.returns, 3)
    images, maps = pictures(a.sweeps * 3, True)
    views = LL.LabelViews(w2c, K, [(H, W)] * (a.sweeps * 3), images, maps)
    offsets = np.arange(a.sweeps + 1, dtype=np.int64) * a.returns
    sweeps = {"sweeps": a.sweeps, "returns_per_sweep": a.returns, "cameras_per_sweep": 3}
    for mode in ("merge", "per_view"):
        out = LL.label_sweeps(points, offsets, views, 3, mode)
        twin = LL.label_sweeps_torch(points, offsets, views, 3, mode)
        same = all(torch.equal(x, y) for x, y in zip(out, twin))
        sweeps[mode] = {"rows": int(out.index.shape[0]), "equal_to_the_twin": bool(same),
                        "fused": timed(lambda: LL.label_sweeps(points, offsets, views, 3, mode), a.rounds),
                        "torch_float64_twin": timed(lambda: LL.label_sweeps_torch(points, offsets, views, 3, mode), a.baseline_rounds)}
        print(mode, json.dumps(sweeps[mode]), flush=True)
    one = LL.LabelViews(w2c[:3], K[:3], [(H, W)] * 3, [p.cpu() for p in images[:3]], [p.cpu() for p in maps[:3]])
    first = points[:a.returns].cpu().numpy()
    sweeps["numpy_checker_one_sweep_cpu_ms"] = measure.per_call_host(lambda: LL.label_sweeps_numpy(first, [0, a.returns], one, 3, "merge"), 0, 1)[0]
    result["label_sweeps"] = sweeps
    del images, maps, views, points
    torch.cuda.empty_cache()

    n_sweeps = (a.vote_views + 2) // 3
    _, w2c, K = scene(n_sweeps, 1, 3)
    w2c, K = w2c[:a.vote_views], K[:a.vote_views]
    g = torch.Generator(device=DEV).manual_seed(5)
    span = torch.tensor([0.5 * n_sweeps + 80.0, 80.0, 8.0], device=DEV, dtype=torch.float64)
    points = torch.rand((a.vote_points, 3), generator=g, device=DEV, dtype=torch.float64) * span + torch.tensor([1.0e5 - 40.0, -2.0e5 - 40.0, 28.8], device=DEV,
                                                                                                                dtype=torch.float64)
    _, maps = pictures(a.vote_views, False)
    views = LL.LabelViews(w2c, K, [(H, W)] * a.vote_views, None, maps)
    xyz, tag, valid = LL.vote_semantics(points, views)
    txyz, ttag, tvalid = LL.vote_semantics_torch(points, views)
    result["vote_semantics"] = {"points": a.vote_points, "views": a.vote_views, "valid": int(valid.sum()),
                                "equal_to_the_twin": bool(torch.equal(tag, ttag) and torch.equal(valid, tvalid) and torch.equal(xyz, txyz)),
                                "fused": timed(lambda: LL.vote_semantics(points, views), a.rounds),
                                "torch_float64_twin": timed(lambda: LL.vote_semantics_torch(points, views), a.baseline_rounds)}
    print("vote", json.dumps(result["vote_semantics"]), flush=True)
    measure.write_record(a.out, result)


if __name__ == "__main__":
    main()

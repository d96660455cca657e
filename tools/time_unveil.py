"""Times the frame masks of the unveiling stage (streetunveiler_amd/unveil.py) on one GPU against what the reference does, and writes
profiles/unveil_time.json: the median of 9 runs with their range, in milliseconds, host clock around work that ends in a device
synchronise, read-backs included.

    semantic_mask_of_points, frame_visibility   3 M points, 200 frames of 1920x1080 (resident maps) -- against the reference's loop over
                                                the frames as the float32 twin on the same GPU
    dilate_mask                                 1920x1080, k = 5, 10, 15 -- against (1) a stock-torch GPU dilation (max_pool2d over the
                                                asymmetrically padded mask) and (2) the reference's route with its two host copies, with
                                                scipy.ndimage.maximum_filter STANDING IN for cv2.dilate where scipy is present: that row is
                                                not cv2 and not an estimate of it
    inpaint_conditions                          1920x1080 -- against the float32 twin

    python tools/time_unveil.py [--points 3000000] [--frames 200] [--out profiles/unveil_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from streetunveiler_amd import unveil as U  # noqa: E402
from tools import measure  # noqa: E402

DEV = "cuda:0"
REPEATS = 9


def timed(fn, warmup=2):
    return {k + "_ms": v for k, v in measure.stats(measure.per_call_host(fn, warmup, REPEATS)).items()}


def street(P, F, H, W, seed=0):
    """A street: cameras driving along +x looking ahead, the cloud a corridor around their path."""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-10, 2.0 * F * 0.5 + 60, P), rng.uniform(-15, 15, P), rng.uniform(-2, 8, P)], axis=1).astype(np.float32)
    w2c = np.zeros((F, 4, 4), dtype=np.float32)
    R = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], dtype=np.float32)      # camera z = world x, camera x = -world y, camera y = -world z
    for f in range(F):
        centre = np.array([0.5 * f, 0.0, 1.5], dtype=np.float32)
        w2c[f, :3, :3], w2c[f, :3, 3], w2c[f, 3, 3] = R, -R @ centre, 1.0
    K = np.tile(np.array([[0.6 * W, 0, 0.5 * W], [0, 0.6 * W, 0.5 * H], [0, 0, 1]], dtype=np.float32), (F, 1, 1))
    cameras = U.FrameCameras(torch.from_numpy(w2c), torch.from_numpy(K), [(H, W)] * F, None, None)
    return torch.from_numpy(xyz).to(DEV), cameras


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=3_000_000)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unveil_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_unveil.py measures on a GPU; there is nothing to time without one"
    H, W = 1080, 1920
    rows = {}

    xyz, cameras = street(args.points, args.frames, H, W)
    packed = U.pack_cameras(cameras, torch.device(DEV))
    maps = torch.randint(0, 19, (args.frames, H, W), dtype=torch.uint8, device=DEV)
    bit = 0b1001_0010_0100

    mask, outside = U.semantic_mask_of_points(xyz, packed, maps, bit)
    twin, _ = U.semantic_mask_of_points_torch(xyz, cameras, maps, bit, torch.float32)
    rows["semantic_mask_of_points"] = {
        "shape": f"{args.points} points, {args.frames} frames of {W}x{H}", "set": int(mask.sum()), "differs_from_twin": int((mask != twin).sum()),
        "hip": timed(lambda: U.semantic_mask_of_points(xyz, packed, maps, bit)[1].item()),
        "float32_twin": timed(lambda: U.semantic_mask_of_points_torch(xyz, cameras, maps, bit, torch.float32), warmup=1)}

    count, depth_sum = U.frame_visibility(xyz, packed)
    twin_count, _ = U.frame_visibility_torch(xyz, cameras, "keep", torch.float32)
    rows["frame_visibility"] = {
        "shape": rows["semantic_mask_of_points"]["shape"], "admitted_pairs": int(count.sum()), "frames_whose_count_differs_from_twin": int((count != twin_count).sum()),
        "hip": timed(lambda: [t.cpu() for t in U.frame_visibility(xyz, packed)]),
        "float32_twin": timed(lambda: [t.cpu() for t in U.frame_visibility_torch(xyz, cameras, "keep", torch.float32)], warmup=1)}
    del maps

    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    m = torch.rand(H, W, device=DEV) < 0.02
    for k in (5, 10, 15):
        row = {"shape": f"{W}x{H}, k = {k}", "differs_from_twin": int((U.dilate_mask(m, k) != U.dilate_mask_torch(m, k)).sum()),
               "hip": timed(lambda: U.dilate_mask(m, k)), "torch_max_pool2d": timed(lambda: U.dilate_mask_torch(m, k))}
        if ndimage is not None:
            def host_route():
                host = m.cpu().numpy().astype(np.uint8)
                return torch.from_numpy(ndimage.maximum_filter(host, size=k, mode="constant", cval=0)).to(DEV).bool()
            row["host_route_with_scipy_standing_in_for_cv2"] = timed(host_route)
        else:
            row["host_route_with_scipy_standing_in_for_cv2"] = "not measured: scipy is not present"
        rows[f"dilate_mask_k{k}"] = row

    r = lambda *s: torch.rand(*s, device=DEV)
    full = {"render": r(3, H, W), "rend_alpha": r(1, H, W)}
    bg = {"render": r(3, H, W), "rend_alpha": full["rend_alpha"] * (r(1, H, W) > 0.1), "surf_depth": r(1, H, W) * 20, "rend_normal": r(3, H, W) * 2 - 1}
    sky = r(3, H, W)
    got, twin = U.inpaint_conditions(full, bg, sky), U.inpaint_conditions_torch(full, bg, sky, 0.01, 5, torch.float32)
    rows["inpaint_conditions"] = {
        "shape": f"{W}x{H}", "bytes_differing_from_twin": {n: int((got[n] != twin[n]).sum()) for n, _ in U.CONDITION_IMAGES},
        "mask_pixels_differing_from_twin": int((got["mask"] != twin["mask"]).sum()),
        "hip": timed(lambda: U.inpaint_conditions(full, bg, sky)), "float32_twin": timed(lambda: U.inpaint_conditions_torch(full, bg, sky, 0.01, 5, torch.float32))}

    out = {**measure.header(), "repeats": REPEATS,
           "method": "host clock around the call and a device synchronise, read-backs included; median, min and max of the repeats", "rows": rows}
    print(json.dumps(out, indent=1))
    measure.write_record(args.out, out)


if __name__ == "__main__":
    main()

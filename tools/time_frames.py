"""Times the frame resize (streetunveiler_amd/frames.py) on one GPU against what the reference does, and writes profiles/frames_time.json:
the median of 9 runs with their range, in milliseconds, host clock around work that ends in a device synchronise, allocations included.

    1920x1280x3 -> 480x320 and -> 960x640, float [3,h,w]     scene load at -r 4 and -r 2 [REF utils/camera_utils.py:53]
    512x768x3 -> 1920x1280, float [3,h,w]                    the unveiling stage's upscale [REF 3_reoptimization/1_optimization.py:140-199]
    the label map 1920x1280 -> 480x320                       [REF utils/camera_utils.py:64-65]
Baselines on the same machine: (1) the reference's own route -- Pillow on the CPU, the division, the upload -- where Pillow is importable,
otherwise recorded as absent, never estimated; (2) F.interpolate(mode="bicubic", antialias=True) plus the division in float32 on the same
GPU, which does NOT produce the same bits (another cubic, float arithmetic, no 8-bit intermediate): its largest difference is recorded.
Every HIP row is also checked against the numpy checker, byte for byte.

    python tools/time_frames.py [--out profiles/frames_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from streetunveiler_amd import frames as F  # noqa: E402
from tools import measure  # noqa: E402

DEV = "cuda:0"
REPEATS = 9


def timed(fn, warmup=2):
    return {k + "_ms": v for k, v in measure.stats(measure.per_call_host(fn, warmup, REPEATS)).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_frames.py measures on a GPU; there is nothing to time without one"
    try:
        from PIL import Image
        import PIL
        pillow = PIL.__version__
    except ImportError:
        Image, pillow = None, None
    rng = np.random.default_rng(0)
    rows = {}
    for name, (H, W), (h, w) in [("scene_load_r4", (1280, 1920), (320, 480)), ("scene_load_r2", (1280, 1920), (640, 960)),
                                 ("stage_upscale", (512, 768), (1280, 1920))]:
        host = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img = torch.from_numpy(host).to(DEV)
        got = F.resize_u8(img, (w, h), out="f32_chw")
        want = F.resize_u8_numpy(host, (w, h), out="f32_chw")
        as_float = img.permute(2, 0, 1)[None].float()
        stock = lambda: torch.nn.functional.interpolate(as_float, size=(h, w), mode="bicubic", antialias=True)[0].clamp(0, 255) / 255.0
        row = {"shape": f"{W}x{H}x3 -> {w}x{h}, float32 [3,h,w]", "bytes_differing_from_checker": int((got.cpu().numpy() != want).sum()),
               "hip": timed(lambda: F.resize_u8(img, (w, h), out="f32_chw")),
               "hip_uint8_output": timed(lambda: F.resize_u8(img, (w, h))),
               "torch_interpolate_bicubic_antialias_not_the_same_bits": timed(stock),
               "torch_interpolate_largest_difference_in_255ths": float((stock() - got).abs().max() * 255.0),
               "torch_interpolate_fraction_of_samples_differing": float(((stock() * 255.0).round() != (got * 255.0).round()).float().mean())}
        if Image is not None:
            pil = Image.fromarray(host)

            def reference_route():
                resized = torch.from_numpy(np.array(pil.resize((w, h), resample=Image.Resampling.BICUBIC))) / 255.0
                return resized.permute(2, 0, 1).to(DEV)
            row["pillow_on_the_cpu_with_upload"] = timed(reference_route)
            row["bytes_differing_from_pillow"] = int((reference_route().cpu().numpy() != got.cpu().numpy()).sum())
        else:
            row["pillow_on_the_cpu_with_upload"] = "not measured: Pillow is not present"
        rows[name] = row

    H, W, h, w = 1280, 1920, 320, 480
    host = rng.integers(0, 19, (H, W), dtype=np.uint8)
    maps = torch.from_numpy(host).to(DEV)
    got = F.resize_labels(maps, (w, h))
    rows["label_map"] = {"shape": f"{W}x{H} uint8 -> {w}x{h}", "bytes_differing_from_checker": int((got.cpu().numpy() != F.resize_labels_numpy(host, (w, h))).sum()),
                         "hip": timed(lambda: F.resize_labels(maps, (w, h))),
                         "torch_interpolate_nearest": timed(lambda: torch.nn.functional.interpolate(maps[None, None], size=(h, w), mode="nearest")[0, 0]),
                         "differs_from_torch_interpolate_nearest": int((torch.nn.functional.interpolate(maps[None, None], size=(h, w), mode="nearest")[0, 0] != got).sum())}

    out = {**measure.header(), "repeats": REPEATS, "pillow": pillow,
           "method": "host clock around the call and a device synchronise, output allocations included; median, min and max of the repeats; "
                     "the tables are computed and uploaded by the warm-up calls and cached", "rows": rows}
    print(json.dumps(out, indent=1))
    measure.write_record(args.out, out)


if __name__ == "__main__":
    main()

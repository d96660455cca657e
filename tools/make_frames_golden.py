"""Writes tests/golden/frames_golden.npz: Pillow's own `Image.resize` output for every case of tests/frames_cases.py, and the version of
the Pillow that made them.  Needs Pillow; the tests that read the file do not.

    python tools/make_frames_golden.py [--out tests/golden/frames_golden.npz]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import frames_cases as fc  # noqa: E402


def pillow_resize(array, wh, resample):
    """One picture [H,W] ("L") or [H,W,3] ("RGB") through Image.resize."""
    from PIL import Image
    how = {"bicubic": Image.Resampling.BICUBIC, "bilinear": Image.Resampling.BILINEAR}[resample]
    return np.array(Image.fromarray(array).resize(wh, resample=how))


def pillow_case(case):
    a = fc.image(case)
    if case.size.frames:
        frames = [pillow_resize(frame[..., 0] if case.channels == 1 else frame, case.wh, case.resample) for frame in a]
        return np.stack(frames)[..., None] if case.channels == 1 else np.stack(frames)
    return pillow_resize(a, case.wh, case.resample)


def main():
    import PIL
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=fc.GOLDEN)
    args = ap.parse_args()
    arrays = {c.name: pillow_case(c) for c in fc.CASES}
    arrays["pillow_version"] = np.array(PIL.__version__)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print(f"{len(fc.CASES)} cases, Pillow {PIL.__version__}, {os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()

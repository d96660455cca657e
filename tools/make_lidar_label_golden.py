"""Writes tests/golden/lidar_label_golden.npz: seeded clouds, cameras and label maps, and what the REFERENCE's own
getCullMaskPointCloudInFrame and getCertainSemanticMask make of them on the CPU.

    python tools/make_lidar_label_golden.py --reference <checkout of the reference>      (or STREETUNVEILER_REFERENCE=<checkout>)

Development-machine tool (CPU): loads scene/dataset_readers/projection_utils.py from the reference's checkout by its path (the module
needs numpy alone; the readers beside it do not import without their datasets' packages) and runs its two helpers on every (sweep, view)
pair of a few cases of tests/lidar_label_cases.py.  Stored per sweep `<case>/sweep<s>/xyz` [n,3] in the case's dtype (the reference is handed
it widened to float64) and per pair `<case>/<view>/`:
    sweep, w2c [4,4], K [3,3], hw [2], map [h,w] uint8 (the lut applied), check_range;
    mask [n] bool, valid_pix [m,2] int32 and certain_mask [m] bool: the reference's own returns.
The reference multiplies through BLAS; the stored decisions are those of this machine's numpy.  Every stored point is exact by construction or
robust by the bound of tests/lidar_label_cases.py, so another summation order decides the same (the tool refuses to write otherwise).
Only this data is committed; nothing of the reference's program text is."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lidar_label_golden.npz")
CASES = ("merge_N65_S3_C3_r3", "merge_N4097_S3_C3_r3_offset", "merge_N4097_S1_C3_r3_lut", "merge_N4097_S3_C3_r1_f32", "per_view_N64_S3_C32_r10_f32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("STREETUNVEILER_REFERENCE"))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not args.reference:
        sys.exit("--reference <checkout of the reference> (or STREETUNVEILER_REFERENCE) is needed")
    path = os.path.join(args.reference, "scene", "dataset_readers", "projection_utils.py")
    spec = importlib.util.spec_from_file_location("reference_projection_utils", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    sys.path.insert(0, ROOT)
    from tests import lidar_label_cases as lc

    out = {}
    for name in CASES:
        c = lc.case(name)
        if lc.non_robust_pairs(c):
            sys.exit(f"{name}: {lc.non_robust_pairs(c)} (point, view) pairs are not robust: the reference's decision there is its BLAS's")
        for g, (a, b, f0, f1) in enumerate(lc.groups(c)):
            out[f"{name}/sweep{g}/xyz"] = c.points[a:b]
            for f in range(f0, f1):
                xyz = c.points[a:b].astype(np.float64)
                homo = np.concatenate([xyz, np.ones((b - a, 1))], axis=1)
                intr = np.zeros((3, 4))
                intr[:3, :3] = c.views.K[f]
                h, w = (int(x) for x in c.views.hw[f])
                semantic_map = c.views.map_numpy(f)
                with np.errstate(all="ignore"):
                    mask, valid_pix = ref.getCullMaskPointCloudInFrame(h, w, homo, c.views.w2c[f], intr)
                    certain = ref.getCertainSemanticMask(semantic_map, valid_pix, c.check_range)
                key = f"{name}/{f}/"
                out.update({key + "sweep": np.array(g), key + "w2c": c.views.w2c[f], key + "K": c.views.K[f], key + "hw": np.array([h, w]), key + "map": semantic_map,
                            key + "check_range": np.array(c.check_range), key + "mask": np.asarray(mask, dtype=bool),
                            key + "valid_pix": np.asarray(valid_pix, dtype=np.int32).reshape(-1, 2), key + "certain_mask": np.asarray(certain, dtype=bool)})
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {sum(k.endswith('/mask') for k in out)} (sweep, view) pairs of {len(CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()

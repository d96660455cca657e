"""Writes tests/golden/voxel_init_golden.npz: seeded point clouds and what the REFERENCE's own SemanticPointCloud.voxel_down_sample makes
of them on the CPU.

    python tools/make_voxel_init_golden.py --reference <checkout of the reference>      (or STREETUNVEILER_REFERENCE=<checkout>)

Development-machine tool (CPU): imports utils/pcd_utils.py from the reference's checkout, runs its class on a few clouds of at most a few
thousand points -- float32 and float64, with and without colours, normals and labels -- and stores per case
    the inputs (points, voxel_size and whichever of colors, normals, semantics the case has),
    out_{points,colors,normals,semantics}: what the reference's class returns (float32 / int32),
    out_index: the voxel index of every returned row.  The class does not return it: it is formed here with the class's own bounds
               methods and compute_voxel_index, the unique indices ascending, under the purity test in the reference's own expression,
               and its length is checked against the rows the class returned.
Only this data is committed; nothing of the reference's program text is."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "voxel_init_golden.npz")


def cases():
    """(name, voxel_size, points, colors, normals, semantics): numpy arrays, seeded."""
    r = np.random.default_rng(20240917)

    def cloud(n, dtype, extent, centre=(0.0, 0.0, 0.0), cluster=True):
        k = n // 3 if cluster else 0
        uni = r.random((n - k, 3)) * np.array(extent)
        clu = np.array(extent) * 0.5 + r.normal(size=(k, 3)) * 0.05      # a tight cluster: voxels of many members
        return (np.concatenate([uni, clu])[r.permutation(n)] + np.array(centre)).astype(dtype)

    def labels(p, noise):
        s = (p[:, 0] > np.median(p[:, 0])).astype(np.int32) + 2 * (p[:, 1] > np.median(p[:, 1])).astype(np.int32)
        flip = r.random(p.shape[0]) < noise
        s[flip] = r.integers(0, 6, size=int(flip.sum()))
        return s.astype(np.int32)

    def unit(n, dtype):
        v = r.normal(size=(n, 3))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(dtype)

    out = []
    p = cloud(2000, np.float32, (6.0, 5.0, 2.0))
    out.append(("f32_all", 0.25, p, r.random((2000, 3)).astype(np.float32), unit(2000, np.float32), labels(p, 0.15)))
    p = cloud(1500, np.float64, (5.0, 5.0, 2.0), centre=(-3.0, 120.0, 1.0))
    out.append(("f64_all", 0.3, p, r.random((1500, 3)), unit(1500, np.float64), labels(p, 0.2)))
    out.append(("f32_points_only", 0.2, cloud(1000, np.float32, (3.0, 3.0, 1.0), centre=(-1.5, -1.5, 0.0)), None, None, None))
    p = cloud(1200, np.float64, (4.0, 4.0, 1.5))
    out.append(("f64_labels_only", 0.25, p, None, None, labels(p, 0.3)))
    # (The reference adds a voxel's members in the INPUT's dtype: for the float32 clouds its own means are up to a few float32 ulps off the
    # float64 truth -- 1.33 ulps of the largest member measured for a voxel of three members.  tests/test_voxel_host.py bounds that by the
    # member count for float32 inputs and holds the float64 clouds to one ulp.)
    p = cloud(1200, np.float32, (4.0, 3.0, 1.0), centre=(-2.0, -1.5, 0.0), cluster=False)
    out.append(("f32_colors", 0.2, p, r.random((1200, 3)).astype(np.float32), None, None))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("STREETUNVEILER_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not args.reference:
        sys.exit("give --reference (or STREETUNVEILER_REFERENCE): the checkout that holds utils/pcd_utils.py")
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils.pcd_utils import SemanticPointCloud      # the reference's class
    assert not torch.cuda.is_available(), "run on a machine without a GPU: the reference's class moves its tensors to one when it finds it"
    torch.set_num_threads(1)
    data, names = {}, []
    for name, voxel_size, points, colors, normals, semantics in cases():
        names.append(name)
        pre = name + "/"
        data[pre + "voxel_size"] = np.float64(voxel_size)
        for key, a in (("points", points), ("colors", colors), ("normals", normals), ("semantics", semantics)):
            if a is not None:
                data[pre + key] = a
        pcd = SemanticPointCloud(points, colors, normals, semantics)
        with contextlib.redirect_stdout(io.StringIO()):
            got = pcd.voxel_down_sample(voxel_size)
        # the index of every point by the reference's own lines and method, then the rows its purity mask kept: a voxel is in the output iff
        # its label is `pure`, which the reference decides from the same per-voxel label counts -- recomputed here in its own expression
        min_bound = pcd.compute_min_bound() - voxel_size * 0.5
        max_bound = pcd.compute_max_bound() + voxel_size * 0.5
        offset = int((torch.max(max_bound).item() - torch.min(min_bound).item() + 2 * voxel_size) / voxel_size)
        index = pcd.compute_voxel_index((pcd.points - min_bound) / voxel_size, offset)
        voxels = torch.unique(index)
        if semantics is not None:
            keep = []
            for vox in voxels:
                lab = pcd.semantics[index == vox]
                keep.append(not (1.0 * torch.unique(lab, return_counts=True)[1].max() / len(lab) < 0.8))
            voxels = voxels[torch.tensor(keep)]
        assert voxels.shape[0] == got.points.shape[0], (name, voxels.shape, got.points.shape)
        data[pre + "out_index"] = voxels.numpy().astype(np.int64)
        for key in ("points", "colors", "normals", "semantics"):
            t = getattr(got, key)
            if t is not None:
                data[pre + "out_" + key] = t.numpy()
        print(name, points.dtype, points.shape[0], "points ->", got.points.shape[0], "of", int(torch.unique(index).shape[0]), "voxels")
    data["names"] = np.array(names)
    np.savez_compressed(args.out, **data)
    print(args.out, os.path.getsize(args.out), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()

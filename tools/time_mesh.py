#!/usr/bin/env python
"""Marching-cubes timing.  python tools/time_mesh.py [--sizes 256,512,1024] [--views V] [--resolution N] [--json FILE]

marching_cubes alone on an analytic volume -- a sphere of radius 0.7 plus low-frequency noise (three sines, amplitude 0.05), resident on
the GPU -- at each size that fits, and extract_mesh_unbounded end to end on the synthetic views tools/time_tsdf.py builds (cameras on a
ring around a unit sphere).  Median of 9 runs with the range after 2 warm-up runs, between device events that end in a synchronise; the
call's one read-back of the counts and its allocations are inside the window, as they are for a caller.

Bytes the passes must move: the count pass and each emission pass read the volume once (4 N bytes each; the stencil's other seven reads
are the neighbours' and hit the caches), the vertex pass writes 5 bytes per owning grid point and 12 per vertex, the face pass reads those
back per referenced edge and writes 12 per face: 12 N + 17 Nv + 24 Nf at the least, N the grid points.  That over the time is set beside
the rate of a device-to-device copy of the volume measured in the same process (which moves 8 N bytes).

No baseline exists where this runs -- the original's CPU routine is not installed -- so no speed-up is claimed and nothing passes or fails
on time.  If skimage imports, its time on the same volume (host arrays, its default method) is reported beside ours, else null.
Writes FILE (default profiles/mesh_time.json)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from streetunveiler_amd import TsdfViews, extract_mesh_unbounded, marching_cubes
from tests import tsdf_cases as tc
from tools import measure

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--sizes", default="256,512,1024"); ap.add_argument("--views", type=int, default=16); ap.add_argument("--resolution", type=int, default=512)
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "mesh_time.json"))
opt = ap.parse_args()
DEV = "cuda:0"
assert torch.cuda.is_available(), "tools/time_mesh.py measures on the GPU; there is no CPU path"
try:
    from skimage import measure as sk_measure
except Exception:
    sk_measure = None


def timed(fn, warmup=2, repeats=9):
    """every call starts from a synchronised device on which the call before it has freed its result"""
    return measure.stats_ms(measure.per_call_events(fn, warmup, repeats, sync_each=True))


def analytic(n):
    g = torch.linspace(-1.0, 1.0, n, device=DEV)
    x, y, z = g[:, None, None], g[None, :, None], g[None, None, :]
    return (torch.sqrt(x * x + y * y + z * z) - 0.7 + 0.05 * (torch.sin(5 * x + 1) * torch.sin(4 * y + 2) * torch.sin(3 * z + 3))).contiguous()


record = {**measure.header(),
          "note": "no baseline is installed where this ran: no speed-up is claimed and nothing passes or fails on time", "marching_cubes": {}}
for n in [int(s) for s in opt.sizes.split(",")]:
    N = n ** 3
    free = torch.cuda.mem_get_info(0)[0]
    if N >= 2 ** 31 or 4 * N * 2 + 5 * N + (1 << 30) > free:      # the volume, its copy for the rate, the workspace, room for the mesh
        record["marching_cubes"][str(n)] = None
        continue
    vol = analytic(n)
    copy = timed(lambda: vol.clone())
    row = timed(lambda: marching_cubes(vol, 0.0, (-1.0,) * 3, (1.0,) * 3))
    vertices, faces = marching_cubes(vol, 0.0, (-1.0,) * 3, (1.0,) * 3)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    moved = 12 * N + 17 * nv + 24 * nf
    copy_rate = 8 * N / (copy["median_ms"] * 1e-3)
    row.update(Nv=nv, Nf=nf, grid_points=N, bytes_the_passes_must_move=moved, device_copy=copy, device_copy_GBps=round(copy_rate / 1e9, 1),
               achieved_GBps=round(moved / (row["median_ms"] * 1e-3) / 1e9, 1), fraction_of_copy_rate=round(moved / (row["median_ms"] * 1e-3) / copy_rate, 3))
    row["skimage"] = None
    if sk_measure is not None and n <= 512:
        host = vol.cpu().numpy()
        row["skimage"] = {"method": "skimage.measure.marching_cubes, default method (lewiner), one run on the host array",
                          "ms": round(measure.per_call_host(lambda: sk_measure.marching_cubes(host, 0.0), 0, 1)[0], 1)}
    record["marching_cubes"][str(n)] = row
    print(n, json.dumps(row))
    del vol, vertices, faces

V, RES, W, H = opt.views, opt.resolution, 1920, 1080
depth, rgb, full = tc._views(tuple(360.0 * k / V for k in range(V)), 1, H, W)
views = TsdfViews(depth.to(DEV), rgb.to(DEV), full.to(DEV))
del depth, rgb
row = timed(lambda: extract_mesh_unbounded(views, tc.CENTER, tc.RADIUS, 1.5, resolution=RES), warmup=1, repeats=9)
mesh = extract_mesh_unbounded(views, tc.CENTER, tc.RADIUS, 1.5, resolution=RES)
row.update(views=V, map_size=[W, H], resolution=RES, bound=1.5, Nv=int(mesh.vertices.shape[0]), Nf=int(mesh.faces.shape[0]))
record["extract_mesh_unbounded"] = row
print("extract_mesh_unbounded", json.dumps(row))
measure.write_record(opt.json, record)

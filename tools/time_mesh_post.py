#!/usr/bin/env python
"""Mesh post-processing timing.  python tools/time_mesh_post.py [--size N] [--json FILE]

Input: the mesh marching_cubes makes of a synthetic N^3 volume (default 256): a lattice of spheres, one in every cell of 32^3 voxels, whose
radii run from below one voxel to 14 voxels -- many components of mixed size, the floaters and the surfaces of a street scene.  The
script states the mesh's face, vertex and component counts.

Timed, as a caller sees them (allocations and the read-back included), 2 warm-up calls and 9 timed rounds between device events; median,
min and max: streetunveiler_amd.connected_triangles and streetunveiler_amd.post_process_mesh(cluster_to_keep=50, min_triangles=50).
The breakdown is per C-ABI call, from events around each call on the same stream (the launches of one call are not separated):
sr_mesh_components (degree, 3 scan launches, fill, unite, labels), the k-th largest size (torch.topk + clamp), sr_mesh_filter_count
(flags, 6 scan launches), the read-back of the three counts, sr_mesh_filter_emit (vertices, faces).  If the k-th-largest selection is
more than a third of the total the record says so.  The hub case of the tests (a closed fan of 3000 faces round one vertex) is timed too:
the valence cliff of the bucket scheme.

Baseline: THE SAME WORK AS STOCK TORCH KERNELS on the same GPU -- edge keys matched by torch.unique (a sort), minimum-label propagation
with scatter_reduce and pointer jumping until a host read-back says nothing changed, boolean-mask compaction.  It is not open3d and not
an estimate of open3d (which runs a single-threaded search on the host).  Its result is compared with the op's, bit for bit.
Writes one record to FILE (default profiles/mesh_post_time.json) with the library's source digest."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from streetunveiler_amd import connected_triangles, marching_cubes, post_process_mesh
from streetunveiler_amd._call import buf, call, ptr, workspace
from tools import measure

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--size", type=int, default=256); ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "mesh_post_time.json"))
opt = ap.parse_args()
N, DEV, CELL, KEEP, FLOOR = opt.size, torch.device("cuda:0"), 32, 50, 50
assert torch.cuda.is_available(), "tools/time_mesh_post.py measures on the GPU; there is no CPU path"


def sphere_lattice(n):
    g = torch.Generator().manual_seed(0)
    cells = (n + CELL - 1) // CELL
    radius = (0.6 + 13.4 * torch.rand((cells,) * 3, generator=g) ** 2).to(DEV)
    jitter = (torch.rand((3,) + (cells,) * 3, generator=g) * 3 - 1.5).to(DEV)
    i = torch.arange(n, device=DEV)
    cell, inside = i // CELL, (i % CELL).float() - CELL / 2 + 0.5
    cx, cy, cz = cell[:, None, None], cell[None, :, None], cell[None, None, :]
    dx = inside[:, None, None] - jitter[0][cx, cy, cz]
    dy = inside[None, :, None] - jitter[1][cx, cy, cz]
    dz = inside[None, None, :] - jitter[2][cx, cy, cz]
    return torch.sqrt(dx * dx + dy * dy + dz * dz) - radius[cx, cy, cz]


def timed(fn, warmup=2, repeats=9):
    return measure.stats_ms(measure.per_call_events(fn, warmup, repeats))


def breakdown(vertices, faces, repeats=9):
    """events around every C-ABI call of post_process_mesh, the buffers allocated beforehand"""
    nv, nf = vertices.shape[0], faces.shape[0]
    labels, sizes = torch.empty((nf,), dtype=torch.int32, device=DEV), torch.empty((nf,), dtype=torch.int32, device=DEV)
    bad, counts = torch.empty((1,), dtype=torch.int32, device=DEV), torch.empty((3,), dtype=torch.int32, device=DEV)
    ws = workspace("sr_mesh_post_workspace_bytes", DEV, nv, nf)
    clock = measure.TorchBackend()
    steps = {name: [] for name in ("sr_mesh_components", "kth_largest_topk", "sr_mesh_filter_count", "read_back", "sr_mesh_filter_emit")}
    for round_ in range(2 + repeats):
        marks = [clock.event() for _ in range(6)]
        marks[0].record()
        call("sr_mesh_components", DEV, ptr(faces), nv, nf, ptr(labels), ptr(sizes), ptr(bad), *buf(ws))
        marks[1].record()
        threshold = torch.clamp(torch.topk(sizes, min(KEEP, nf)).values[-1:], min=FLOOR).to(torch.int32)
        marks[2].record()
        call("sr_mesh_filter_count", DEV, ptr(faces), nv, nf, ptr(labels), ptr(sizes), ptr(threshold), *buf(ws), ptr(counts))
        marks[3].record()
        nv_out, nf_out, _ = counts.tolist()
        marks[4].record()
        out_v, out_f = torch.empty((nv_out, 3), device=DEV), torch.empty((nf_out, 3), dtype=torch.int32, device=DEV)
        call("sr_mesh_filter_emit", DEV, ptr(faces), nv, nf, ptr(vertices), None, *buf(ws), nv_out, nf_out, ptr(out_v), None, ptr(out_f))
        marks[5].record()
        torch.cuda.synchronize()
        if round_ >= 2:
            for k, name in enumerate(steps):
                steps[name].append(marks[k].elapsed_time(marks[k + 1]))
    return {name: round(statistics.median(ms), 3) for name, ms in steps.items()}


def torch_baseline(vertices, faces, keep, floor):
    """the same work as stock torch kernels -> (vertices, faces, labels)"""
    nv, nf = vertices.shape[0], faces.shape[0]
    f = faces.long()
    u, w = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    edge = torch.unique(torch.minimum(u, w) * nv + torch.maximum(u, w), return_inverse=True)[1]
    face_of = torch.arange(nf, device=faces.device).repeat_interleave(3)
    labels = torch.arange(nf, device=faces.device)
    while True:
        on_edge = torch.full((int(edge.max()) + 1,), nf, dtype=torch.int64, device=faces.device).scatter_reduce(0, edge, labels[face_of], "amin")
        new = labels.scatter_reduce(0, face_of, on_edge[edge], "amin")
        new = new[new]
        if bool((new == labels).all().item()):
            break
        labels = new
    sizes = torch.bincount(labels, minlength=nf)
    threshold = torch.clamp(torch.topk(sizes, min(keep, nf)).values[-1], min=floor)
    remaining = f[sizes[labels] >= threshold]
    used = torch.zeros((nv,), dtype=torch.bool, device=faces.device)
    used[remaining.reshape(-1)] = True
    remaining = (torch.cumsum(used, 0) - 1)[remaining]
    good = (remaining[:, 0] != remaining[:, 1]) & (remaining[:, 1] != remaining[:, 2]) & (remaining[:, 2] != remaining[:, 0])
    return vertices[used], remaining[good].to(torch.int32), labels


vertices, faces = marching_cubes(sphere_lattice(N))
nv, nf = vertices.shape[0], faces.shape[0]
clusters, counts = connected_triangles(faces, nv)
out = post_process_mesh((vertices, faces), KEEP, FLOOR)
record = {**measure.header(),
          "scene": f"marching_cubes of a {N}^3 volume: one sphere per {CELL}^3 cell, radii 0.6 .. 14 voxels", "vertices": nv, "faces": nf,
          "components": int(counts.shape[0]), "largest_component": int(counts.max()), "smallest_component": int(counts.min()),
          "cluster_to_keep": KEEP, "min_triangles": FLOOR, "vertices_out": int(out.vertices.shape[0]), "faces_out": int(out.faces.shape[0])}
print(f"mesh: {nf} faces, {nv} vertices, {record['components']} components of {record['smallest_component']} .. {record['largest_component']} faces; "
      f"kept: {record['faces_out']} faces, {record['vertices_out']} vertices")
record["connected_triangles"] = timed(lambda: connected_triangles(faces, nv))
record["post_process_mesh"] = timed(lambda: post_process_mesh((vertices, faces), KEEP, FLOOR))
steps = breakdown(vertices, faces)
total = sum(steps.values())
record["post_process_mesh_per_call_median_ms"] = steps
record["kth_largest_share_of_total"] = round(steps["kth_largest_topk"] / total, 3)
record["kth_largest_is_more_than_a_third"] = bool(steps["kth_largest_topk"] > total / 3)


measure.write_record(opt.json, record)      # (what is measured so far, should the baseline not run)
base_v, base_f, base_labels = torch_baseline(vertices, faces, KEEP, FLOOR)
same = bool(torch.equal(base_f, out.faces) and torch.equal(base_v.view(torch.int32), out.vertices.view(torch.int32)))
record["baseline_stock_torch_kernels"] = dict(timed(lambda: torch_baseline(vertices, faces, KEEP, FLOOR), warmup=1, repeats=9), same_result_as_the_op=same,
                                              note="edge keys by torch.unique, minimum-label propagation by scatter_reduce with pointer jumping and a host "
                                                   "read-back per round, boolean-mask compaction; not open3d and not an estimate of open3d")
hub = torch.tensor([(0, 1 + i, 1 + (i + 1) % 3000) for i in range(3000)], dtype=torch.int32, device=DEV)
record["hub_3000_faces_connected_triangles"] = timed(lambda: connected_triangles(hub, 3001))
strip = torch.tensor([(i, i + 1, i + 2) for i in range(3000)], dtype=torch.int32, device=DEV)
record["strip_3000_faces_connected_triangles"] = timed(lambda: connected_triangles(strip, 3002))
for name in ("connected_triangles", "post_process_mesh", "baseline_stock_torch_kernels", "hub_3000_faces_connected_triangles", "strip_3000_faces_connected_triangles"):
    r = record[name]
    print(f"{name}: median {r['median_ms']:.3f} ms (min {r['min_ms']:.3f}, max {r['max_ms']:.3f})")
print("per call:", steps, "k-th largest share:", record["kth_largest_share_of_total"], "baseline same result:", same)
measure.write_record(opt.json, record)

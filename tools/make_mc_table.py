"""Derives the marching-cubes case table and writes it in its two forms, streetunveiler_amd/csrc/mc_table.h (the kernels of csrc/mesh.hip)
and streetunveiler_amd/_mc_table.py (the numpy checker of streetunveiler_amd/mesh.py):

    python tools/make_mc_table.py            writes both files
    python tools/make_mc_table.py --check    exits 1 if a committed file differs from what is generated now

Nothing here is recalled from a published table.  Conventions (stated again in the header's comment):
    corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) along (x, y, z) from the cell's lowest grid point;
    edge e = 4 * axis + k runs along `axis` from the corner at offset (o1, o2) = (k & 1, k >> 1) along the two OTHER axes in
    ascending order (axis x: (y, z); axis y: (x, z); axis z: (x, y)) -- it is owned by the grid point at its lower end and by its axis;
    bit c of a case is set iff corner c is inside, and inside means value < level, strictly.

Per case: the crossed edges are those whose ends differ.  On each of the six faces the crossings are paired by one rule that reads only
that face's four corner signs: every maximal run of inside corners around the face is cut off by one segment, so on a face with four
crossings (inside corners diagonally opposite) each inside corner is cut off on its own -- the two cells sharing the face see the same
four signs and draw the same two segments.  A segment is directed so that, seen from outside the cell, it runs from the face edge in
front of the run (counter-clockwise) to the face edge behind it; every crossed edge then has one segment arriving and one leaving, the
segments chain into closed directed loops, each loop is rotated to start at its smallest edge id and fan-triangulated from there, and the
direction chosen makes every triangle's normal (right-hand rule) point away from the inside corners, towards the larger values.  The same
face seen from the neighbouring cell is walked the other way round, so the neighbour's segments are the reverses: in the mesh every
directed triangle edge inside a face meets its reverse, which is what closedness and consistent orientation mean."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "streetunveiler_amd", "csrc", "mc_table.h")
TWIN = os.path.join(ROOT, "streetunveiler_amd", "_mc_table.py")

OTHER_AXES = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_at(offset):
    return offset[0] | (offset[1] << 1) | (offset[2] << 2)


def edge_owner(e):
    """(offset of the owning corner, axis) of edge e."""
    axis, k = divmod(e, 4)
    off = [0, 0, 0]
    a1, a2 = OTHER_AXES[axis]
    off[a1], off[a2] = k & 1, k >> 1
    return tuple(off), axis


def edge_corners(e):
    off, axis = edge_owner(e)
    hi = list(off)
    hi[axis] = 1
    return corner_at(off), corner_at(tuple(hi))


EDGE_BETWEEN = {frozenset(edge_corners(e)): e for e in range(12)}


def faces():
    """The six faces as four corners each, counter-clockwise seen from outside the cell."""
    out = []
    for axis in range(3):
        a1, a2 = OTHER_AXES[axis]
        for side in (0, 1):
            ring = []
            for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[axis], off[a1], off[a2] = side, u, v
                ring.append(corner_at(tuple(off)))
            # (e_a1 x e_a2) points along +axis for axis 0 and 2 and along -axis for axis 1 ((x, z) is left-handed about y): the ring as
            # built is counter-clockwise seen from that side; seen from the other side it is the reverse
            ccw_from_positive = axis != 1
            out.append(ring if (side == 1) == ccw_from_positive else ring[::-1])
    return out


FACES = faces()


def face_segments(case, ring):
    """Directed segments (edge id -> edge id) on one face, from that face's four corner signs alone."""
    inside = [(case >> c) & 1 for c in ring]
    if sum(inside) in (0, 4):
        return []
    face_edge = [EDGE_BETWEEN[frozenset((ring[k], ring[(k + 1) % 4]))] for k in range(4)]      # face edge k joins ring[k] and ring[k + 1]
    segs = []
    for k in range(4):
        if inside[k] and not inside[k - 1]:      # a run of inside corners starts at ring[k]
            m = k
            while inside[(m + 1) % 4]:
                m += 1
            segs.append((face_edge[(k - 1) % 4], face_edge[m % 4]))
    return segs


def loops_of(case):
    nxt, arrivals = {}, {}
    for ring in FACES:
        for a, b in face_segments(case, ring):
            assert a not in nxt and b not in arrivals, (case, a, b)      # one segment leaves and one arrives at every crossed edge
            nxt[a], arrivals[b] = b, a
    crossed = {e for e in range(12) if ((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1}
    assert set(nxt) == crossed == set(arrivals), case
    loops, seen = [], set()
    for start in sorted(crossed):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3, (case, loop)
        loops.append(loop)      # begins at its smallest edge id: `start` ascends and a loop is consumed whole
    return loops


def edge_midpoint(e):
    off, axis = edge_owner(e)
    p = [float(v) for v in off]
    p[axis] = 0.5
    return p


def triangles_of(case):
    tris = []
    for loop in loops_of(case):
        for k in range(1, len(loop) - 1):
            tris.append((loop[0], loop[k], loop[k + 1]))      # in the loop's direction: normals away from the inside corners
    return tris


def _normal(tri):
    a, b, c = (edge_midpoint(e) for e in tri)
    u, v = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def generate():
    table = [triangles_of(case) for case in range(256)]
    assert table[0] == [] and table[255] == []
    for c in range(8):      # one corner inside: one triangle whose normal points away from it; one corner outside: towards it
        away = [1 - 2 * v for v in corner_offset(c)]
        for case, sign in ((1 << c, 1), (255 ^ (1 << c), -1)):
            assert len(table[case]) == 1 and sign * sum(n * a for n, a in zip(_normal(table[case][0]), away)) > 0, case
    max_tris = max(len(t) for t in table)
    assert max_tris == 5, max_tris      # the separating rule never needs more; the tables below are sized by it
    for case in range(256):      # closed inside the cell up to the faces: every directed triangle edge either meets its reverse or lies in a face
        directed = {}
        for t in table[case]:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                directed[(a, b)] = directed.get((a, b), 0) + 1
        on_faces = {(a, b) for ring in FACES for a, b in face_segments(case, ring)}
        for (a, b), n in directed.items():
            assert n == 1 and (((b, a) in directed) != ((a, b) in on_faces)), (case, a, b)
        assert on_faces <= set(directed), case
    return table, max_tris


def _rows(values, per_line, fmt):
    return ",\n".join("    " + ", ".join(fmt(v) for v in values[k:k + per_line]) for k in range(0, len(values), per_line))


def emit(table, max_tris):
    counts = [len(t) for t in table]
    flat = []
    for t in table:
        row = [e for tri in t for e in tri]
        flat += row + [255] * (3 * max_tris - len(row))
    owners = [edge_owner(e) for e in range(12)]
    conventions = [
        "corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) along (x, y, z) from the cell's lowest grid point (ix, iy, iz)",
        "edge e = 4 * axis + k runs along `axis` from the corner at offset (k & 1, k >> 1) along the two other axes in ascending order",
        "    (axis x: (y, z); axis y: (x, z); axis z: (x, y)); kMcEdgeOwner[e] = that corner's offset (dx | dy << 1 | dz << 2) | axis << 3",
        "edge e of cell (ix, iy, iz) is owned by the grid point at its lower end, (ix + dx, iy + dy, iz + dz), and by its axis",
        "bit c of a case is set iff corner c is inside, and inside means value < level, strictly",
        "kMcTriCount[case] triangles; triangle k of a case is kMcTriEdges[15 case + 3 k .. + 2] (edge ids, 255 = unused), its normal",
        "    (right-hand rule) pointing towards the larger values; a face with four crossings cuts off each inside corner on its own",
    ]
    h = ["// mc_table.h -- the marching-cubes case table.  GENERATED by tools/make_mc_table.py (which derives it: see its docstring): do not edit.",
         "// Conventions:"]
    h += ["//   " + line for line in conventions]
    h += ["// (device arrays: csrc/mesh.hip stages them in LDS; the Python twin is streetunveiler_amd/_mc_table.py)", "#pragma once", "#include <hip/hip_runtime.h>", "#include <cstdint>", "", "namespace sr {", "",
          f"constexpr int kMcMaxTriangles = {max_tris};",
          "static __device__ const uint8_t kMcEdgeOwner[12] = {" + ", ".join(str(corner_at(o) | (a << 3)) for o, a in owners) + "};",
          "static __device__ const uint8_t kMcTriCount[256] = {", _rows(counts, 32, str), "};",
          f"static __device__ const uint8_t kMcTriEdges[256 * {3 * max_tris}] = {{", _rows(flat, 3 * max_tris, lambda v: "%3d" % v), "};",
          "", "}  // namespace sr", ""]
    p = ['"""The marching-cubes case table.  GENERATED by tools/make_mc_table.py (which derives it: see its docstring): do not edit.',
         "Conventions:"]
    p += ["  " + line for line in conventions]
    p += ['"""', f"MAX_TRIANGLES = {max_tris}",
          "EDGE_OWNER = (" + ", ".join(f"(({o[0]}, {o[1]}, {o[2]}), {a})" for o, a in owners) + ")      # edge -> (owner's offset, axis)",
          "TRI_COUNT = (", _rows(counts, 32, str) + ",", ")",
          "TRI_EDGES = (", _rows(flat, 3 * max_tris, lambda v: "%3d" % v) + ",", ")", ""]
    return "\n".join(h), "\n".join(p)


def main(argv):
    header, twin = emit(*generate())
    if "--check" in argv:
        stale = [path for path, text in ((HEADER, header), (TWIN, twin)) if not os.path.exists(path) or open(path).read() != text]
        for path in stale:
            print(f"{os.path.relpath(path, ROOT)} differs from what tools/make_mc_table.py generates")
        return 1 if stale else 0
    for path, text in ((HEADER, header), (TWIN, twin)):
        with open(path, "w") as f:
            f.write(text)
        print("wrote", os.path.relpath(path, ROOT))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

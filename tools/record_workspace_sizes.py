"""Records what every *_bytes function of the library reports over a table of shapes -> tests/golden/workspace_sizes.json.

Pure host arithmetic, no GPU.  Run it on the library whose sizes are the reference (SURFEL_RASTER_LIB=<a build of the commit to hold
later ones to>), never on the one under test: it refuses a library that carries this tree's source digest, the file names the digest
it was recorded from, and tests/test_abi.py compares every later build with the file.
    SURFEL_RASTER_LIB=.../libsurfel_raster.so python tools/record_workspace_sizes.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from streetunveiler_amd import _lib  # noqa: E402

# 0 and 1, and one below, at and one above: the scan's chunk (256), its block (2048), 256 blocks of 256 densify rows (65,536), of 1024
# pass-X inputs (262,144) and of 2048 scan or sort items (524,288)
COUNTS = [0, 1] + [b + d for b in (256, 2048, 65536, 262144, 524288) for d in (-1, 0, 1)]
FRAMES = [(1, 1), (64, 64), (203, 125), (255, 257), (1920, 1080)]


def table(lib):
    rows = {}

    def rec(name, *args):
        rows.setdefault(name, []).append(list(args) + [int(getattr(lib, name)(*args))])

    for n in COUNTS:
        rec("sr_geom_bytes", n)
        rec("sr_cluster_workspace_bytes", n)
        rec("sr_densify_workspace_bytes", n)
        rec("sr_debug_radix_sort_temp_bytes", n)
        for other in (0, 1, 2049, 524289):       # every count as nq (0: the self search) and as nr, against a few of the other
            rec("sr_knn_workspace_bytes", n, other)
            if n not in (0, 1, 2049, 524289):
                rec("sr_knn_workspace_bytes", other, n)
        for channels in (3, 6, 9):
            rec("sr_backward_workspace_bytes", 0, n, channels)
        for W, H in FRAMES:
            rec("sr_binning_bytes", 0, n, W, H)
        for classes in (1, 6):
            rec("sr_class_shared_bytes", n, 203, 125, classes, 5000)
            rec("sr_class_shared_bytes", 2049, 203, 125, classes, n)
    for W, H in FRAMES:
        rec("sr_image_bytes", W, H)
        for classes in (1, 6):
            rec("sr_class_image_bytes", W, H, classes)
    return rows


if __name__ == "__main__":
    from streetunveiler_amd.build import source_digest
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "workspace_sizes.json")
    lib = _lib.load()
    digest = lib.sr_source_digest().decode()
    if digest == source_digest():
        sys.exit("this library was built from the sources of this tree: it is the one under test, not a reference (set SURFEL_RASTER_LIB)")
    rows = table(lib)
    with open(out, "w") as f:      # one row per line, so that a change of the file can be read
        f.write('{"recorded_from_source_digest": "%s",\n "counts": %s,\n "sizes": {\n' % (digest, json.dumps(COUNTS)))
        f.write(",\n".join('  "%s": [\n%s]' % (name, ",\n".join("   " + json.dumps(r) for r in rs)) for name, rs in rows.items()))
        f.write("}}\n")
    print(out)

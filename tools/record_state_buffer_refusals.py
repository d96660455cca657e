"""Records what the rasteriser's entry points answer to a NULL or short state buffer and to a NULL pointer argument: the status and the
whole sr_last_error() text of every call tests/state_buffer_cases.py lists -> tests/golden/state_buffer_refusals.json.

Pure host code, no GPU: every refusal recorded here comes before its entry point's first HIP call (the one that comes after one,
sr_backward's NULL radii, is left out: state_buffer_cases.AFTER_A_HIP_CALL).  Run it on the library whose refusals are the reference
(SURFEL_RASTER_LIB=<a build of the commit to hold later ones to>), never on the one under test: it refuses a library that carries this
tree's source digest, the file names the digest it was recorded from, and tests/test_abi.py compares every later build with the file.
    SURFEL_RASTER_LIB=.../libsurfel_raster.so python tools/record_state_buffer_refusals.py [out.json]

The committed file is this tool's output for the library of commit d9479ec with two kinds of rows edited by hand since, in the commit
that resolved every call's buffers in one place (tools/notes_resolve_once.md): the rows that library answered with a text naming no
buffer now hold the naming text ("recorded_text": what it said), and the rows of state_buffer_cases.UNRECORDED were added
("recorded_text": null -- that library went on to a launch there).  A fresh recording has neither.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from streetunveiler_amd import _lib  # noqa: E402
from tests import state_buffer_cases as cases  # noqa: E402


def table(lib):
    scene = cases.Scene(lib)
    rows = []
    single = [(entry, argument, fault, None, ()) for entry in cases.ARGUMENTS for argument, fault in cases.faults(entry)]
    for entry, argument, fault, case, also in single + cases.DOUBLE_FAULTS:
        status, text = scene.refusal(entry, argument, fault, case, also)
        if status not in (-1, -3):   # SR_ERR_INVALID_ARGUMENT, SR_ERR_BUFFER_TOO_SMALL: anything else got as far as a HIP call
            sys.exit(f"{entry}: {argument} {fault} {also} was not refused as an argument ({status}: {text})")
        rows.append(dict({"entry": entry, "argument": argument, "fault": fault, "status": status, "text": text}, **({"also": also} if also else {})))
    return rows


if __name__ == "__main__":
    from streetunveiler_amd.build import source_digest
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "state_buffer_refusals.json")
    lib = _lib.load()
    digest = lib.sr_source_digest().decode()
    if digest == source_digest():
        sys.exit("this library was built from the sources of this tree: it is the one under test, not a reference (set SURFEL_RASTER_LIB)")
    rows = table(lib)
    with open(out, "w") as f:      # one row per line, so that a change of the file can be read
        f.write('{"recorded_from_source_digest": "%s",\n "refusals": [\n' % digest)
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("]}\n")
    print(out)

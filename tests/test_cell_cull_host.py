"""CPU: the staging lane's cell culling, compiled for the host, against the blend's acceptance rule (tests/cell_cull_host.cpp).

streetunveiler_amd/csrc/footprint_cull.h is plain C++ behind its intrinsic wrappers; the program includes it, draws a few thousand seeded
splats per run (isotropic; 20:1 at 0 / 45 / 90 / 135 degrees and arbitrary angles; centres far outside the tile; opacities from 1/255 to 1;
c22 near 0 from both sides; zero scales; NaN / inf rows), evaluates intersect()'s float expressions at the 256 pixel centres of a 16x16 tile
and compares the 4x4 cells that hold an accepted pixel with the cells the slab-extent test (what the row-mapped forward stages with) and
the octagon test (what it staged with before) keep.  Required: the slab test drops no cell with an accepted pixel -- as one 16x16 tile and
as the kernel's two 16x8 bands -- and keeps fewer cells without one than the octagon does, over everything and in the elongated family,
where the octagon is loose."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINITE = ["isotropic", "elongated", "far_centres", "c22_near_zero", "zero_scale"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("cell_cull") / "cell_cull_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "streetunveiler_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cell_cull_host.cpp"), "-o", exe, "-lm"], check=True)
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_slab_test_keeps_every_accepted_cell_and_fewer_empty_ones_than_the_octagon(program, seed):
    r = subprocess.run([program, str(seed)], capture_output=True, text=True)
    print(r.stdout, r.stderr[-4000:])
    rep = json.loads(r.stdout)
    a = rep["all"]
    assert a["splats"] >= 3000 and a["accepted_cells"] > 5000
    for fam, t in rep.items():
        assert t["splats"] > 0 and (fam == "nan_inf" or t["accepted_cells"] > 0), fam
        assert t["missed_slab"] == 0 and t["missed_band"] == 0, (fam, t)
    for fam in FINITE:   # (the yardstick is held too where its inputs are finite)
        assert rep[fam]["missed_octagon"] == 0, (fam, rep[fam])
    assert r.returncode == 0
    assert a["false_slab"] < a["false_octagon"], a
    assert rep["elongated"]["false_slab"] < rep["elongated"]["false_octagon"], rep["elongated"]

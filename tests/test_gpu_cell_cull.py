"""GPU (-m gpu): the row-mapped forward's cell culling (slab extents, csrc/footprint_cull.h) changes no bit of any result.

Two small frames -- 64x48, and 40x24 with partial tiles at both edges -- of 3000 / 2000 Gaussians from the families tests/cell_cull_host.cpp
draws in the image plane, here as 3-D parameters: isotropic splats, 20:1 splats turned by 0 / 45 / 90 degrees and by arbitrary rotations,
centres far outside the frustum, opacities from 1/255 to 1, splats whose cutoff disc almost reaches (or just crosses) the camera plane
(c22 near 0 from both sides), zero scales, NaN / inf parameters.  The forward with the row mapping forced and with the per-frame choice
(culling on) against the same call with quadrant_cull off: colour, the seven maps, radii, n_contrib and final_T bit for bit; one forward +
backward through each, every gradient bit for bit; the counter variant: no exact (entry, cell) hit dropped by the staging test ([14] == 0),
and no more pairs kept than the octagon test keeps on the same scene ([10] <= [15], both counted by the same launch)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCENES = {"64x48": (64, 48, 3000, 5), "40x24": (40, 24, 2000, 6)}
GRADS = ["dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh", "dL_dmeans2D"]
_cache = {}


def _scene(name):
    """(cam, gaussians, bg, upstream gradients), drawn once on the CPU from the scene's seed."""
    if name in _cache:
        return _cache[name]
    from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians, synthetic_upstream_grads
    W, H, P, seed = SCENES[name]
    cam = synthetic_camera(W, H)
    g = synthetic_gaussians(P, W, H, seed=seed, scale_lo=5e-3, scale_hi=1.5e-1)
    gen = torch.Generator().manual_seed(seed + 100)
    rnd = lambda *s: torch.rand(*s, generator=gen)
    z = g["means3D"][:, 2].clone()
    n = P // 8
    fam = lambda k: slice(k * n, (k + 1) * n)
    zrot = lambda a: torch.stack([torch.cos(a / 2), torch.zeros_like(a), torch.zeros_like(a), torch.sin(a / 2)], dim=1)   # (w, x, y, z)
    # 0: isotropic
    g["scales"][fam(0), 1] = g["scales"][fam(0), 0]
    # 1: 20:1, facing the camera, turned by 0 / 45 / 90 / 135 degrees;  2: 20:1 under arbitrary rotations (the base quaternions)
    for k in (1, 2):
        g["scales"][fam(k), 0] = z[fam(k)] * (0.03 + 0.3 * rnd(n))
        g["scales"][fam(k), 1] = g["scales"][fam(k), 0] / 20.0
    g["rotations"][fam(1)] = zrot(torch.randint(0, 4, (n,), generator=gen).float() * (math.pi / 4))
    # 3: centres far outside the frustum, long enough to reach back into it
    out = 1.5 + 6.0 * rnd(n)
    g["means3D"][fam(3), 0] *= out
    g["means3D"][fam(3), 1] *= 1.5 + 6.0 * rnd(n)
    g["scales"][fam(3), 0] = z[fam(3)] * out * (0.1 + 0.4 * rnd(n))
    g["scales"][fam(3), 1] = g["scales"][fam(3), 0] / (1.0 + 30.0 * rnd(n))
    # 4: opacities 1/255 .. 1, both ends and a value just below the floor included
    op = (1.0 / 255.0) * torch.pow(torch.tensor(255.0), rnd(n))
    op[0], op[1], op[2] = 1.0 / 255.0, 1.0, 0.0039
    g["opacities"][fam(4), 0] = op
    # 5: the cutoff disc sqrt(thr) s |t_z| ~ z_c: v axis tilted by phi towards the camera, s_v = f z_c / (sqrt(thr) sin phi), f around 1
    phi = 0.3 + 1.1 * rnd(n)
    thr = 2.0 * torch.log(255.0 * g["opacities"][fam(5), 0]).clamp_min(0.05)
    f = torch.where(rnd(n) < 0.5, 0.9 + 0.2 * rnd(n), 1.0 + 2e-3 * (rnd(n) - 0.5))
    g["means3D"][fam(5), :2] *= 0.5
    g["rotations"][fam(5)] = torch.stack([torch.cos(phi / 2), torch.sin(phi / 2), torch.zeros(n), torch.zeros(n)], dim=1)
    g["scales"][fam(5), 1] = f * z[fam(5)] / (thr.sqrt() * torch.sin(phi))
    g["scales"][fam(5), 0] = z[fam(5)] * (0.01 + 0.1 * rnd(n))
    # 6: zero scale -- one axis, the other, both
    g["scales"][6 * n: 7 * n: 3, 0] = 0.0
    g["scales"][6 * n + 1: 7 * n: 3, 1] = 0.0
    g["scales"][6 * n + 2: 7 * n: 3, :] = 0.0
    # 7: NaN / inf parameters (every fourth of the family; the others stay plain splats)
    i0 = 7 * n
    for j, (field, val) in enumerate([("scales", float("nan")), ("scales", float("inf")), ("opacities", float("nan")), ("opacities", float("inf")),
                                      ("rotations", float("nan")), ("means3D", float("nan")), ("means3D", float("inf"))]):
        g[field][i0 + j: i0 + n: 28, 0] = val
    dc, da = synthetic_upstream_grads(W, H)
    _cache[name] = (cam, g, np.array([0.1, 0.2, 0.3], np.float32), dc, da)
    return _cache[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _raw(name, **kw):
    key = (name, "raw", tuple(sorted(kw.items())))
    if key not in _cache:
        from tests.gpu_util import run_hip_raw
        cam, g, bg, _, _ = _scene(name)
        _cache[key] = run_hip_raw(g, cam, bg, 3, **kw)
    return _cache[key]


def _grads(name, **kw):
    key = (name, "grads", tuple(sorted(kw.items())))
    if key not in _cache:
        from tests.gpu_util import run_hip
        cam, g, bg, dc, da = _scene(name)
        _cache[key] = run_hip(g, cam, bg, 3, dc, da, **kw)
    return _cache[key]


@pytest.mark.parametrize("mapping", ["rows", "auto"])
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_bits_do_not_depend_on_the_cell_culling(name, mapping):
    got = _raw(name, row_mapped=True if mapping == "rows" else None)
    ref = _raw(name, quadrant_cull=False)
    assert got["D"] == ref["D"] and got["D"] > 1000
    assert ref["allmap"].shape[0] == 7
    for k in ("color", "allmap", "radii"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    for k in ("n_contrib", "final_T"):
        assert np.array_equal(_bits(got["img"][k]), _bits(ref["img"][k])), k
    assert (ref["img"]["n_contrib"][0] > 0).mean() > 0.5   # the frame is covered: the comparison is about blended pixels


@pytest.mark.parametrize("mapping", ["rows", "auto"])
@pytest.mark.parametrize("name", list(SCENES))
def test_gradient_bits_do_not_depend_on_the_cell_culling(name, mapping):
    got = _grads(name, row_mapped=True if mapping == "rows" else None)
    ref = _grads(name, quadrant_cull=False)
    for k in ("color", "allmap", "radii"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    for k in GRADS:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    finite = np.isfinite(ref["dL_dmeans3D"]).all(axis=1)
    assert np.abs(ref["dL_dmeans3D"][finite]).sum() > 0


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("name", list(SCENES))
def test_counters_staging_test_drops_no_hit_and_keeps_no_more_than_the_octagon(name, cull):
    """cull = False: every (entry, quadrant) pair is tested, so [14] sees every exact hit of the frame."""
    from diff_surfel_rasterization import GaussianRasterizer
    from tests.gpu_util import DEV, settings_for
    cam, g, bg, _, _ = _scene(name)
    d = {k: v.to(DEV) for k, v in g.items()}
    counters = torch.zeros(16, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        GaussianRasterizer(settings_for(cam, bg, 3), blend_counters=counters, quadrant_cull=cull)(
            means3D=d["means3D"], means2D=torch.zeros(len(d["means3D"]), 3, device=DEV), shs=d["shs"], opacities=d["opacities"],
            scales=d["scales"], rotations=d["rotations"])
    torch.cuda.synchronize()
    st = counters.tolist()
    print(name, "cull" if cull else "no cull", "exact pairs", st[8], "kept by the staging test", st[10], "by the octagon", st[15], "dropped hits", st[14])
    assert st[0] > 1000 and st[8] > 0
    assert st[14] == 0
    assert st[8] <= st[10] <= st[15]
    assert st[9] <= st[11]

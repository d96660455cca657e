"""-m gpu: the LiDAR voxel downsample (csrc/voxel.hip) on every case of tests/voxel_cases.py under its bars -- through voxel_down_sample
and through the raw C-ABI sequence with caller-owned, sentinel-filled buffers, two runs bit for bit, on a non-default stream -- the
refusals, and create_from_pcd end to end: downsample, model, one render."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from streetunveiler_amd import _lib as L
from streetunveiler_amd import voxel as V
from streetunveiler_amd._call import buf, call, ptr, workspace
from tests import voxel_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _run(c):
    cloud, counts, index = V.voxel_down_sample(_up(c["points"]), c["voxel_size"], _up(c["colors"]), _up(c["normals"]), _up(c["semantics"]),
                                               return_counts=True, return_index=True)
    return {"points": _np(cloud.points), "colors": _np(cloud.colors), "normals": _np(cloud.normals), "semantics": _np(cloud.semantics),
            "counts": _np(counts), "index": _np(index)}


@pytest.mark.parametrize("name", vc.NAMES)
def test_every_case_through_the_function_twice(name):
    c = vc.case(name)
    first = _run(c)
    vc.compare(name, first, "voxel_down_sample")
    again = _run(c)
    for key, a in first.items():                            # equal inputs, equal bits
        assert (a is None and again[key] is None) or a.tobytes() == again[key].tobytes(), (name, key)


def _raw(c):
    """The C-ABI sequence a caller without the wrapper makes: bounds, the host arithmetic, group, the read-back, emit."""
    dev = torch.device(DEV)
    pts, col, nrm, sem = _up(c["points"]), _up(c["colors"]), _up(c["normals"]), _up(c["semantics"])
    n = pts.shape[0]
    if sem is not None and sem.dtype not in (torch.int32, torch.int64):
        sem = sem.to(torch.int32)
    f64 = lambda t: int(t is not None and t.dtype == torch.float64)
    ws = workspace("sr_voxel_workspace_bytes", dev, n)
    ws.fill_(0xA5)
    counts = torch.full((3,), -7, dtype=torch.int32, device=dev)
    lo, offset = np.zeros(3), 3
    if n:
        bounds = torch.full((7,), float("nan"), dtype=torch.float64, device=dev)
        call("sr_voxel_bounds", dev, n, ptr(pts), f64(pts), *buf(ws), ptr(bounds))
        b = bounds.cpu().numpy()
        assert b[6] == 0 and np.array_equal(b[:3], c["points"].min(0).astype(np.float64)) and np.array_equal(b[3:6], c["points"].max(0).astype(np.float64))
        lo, offset = V.voxel_frame(b[:3], b[3:6], c["voxel_size"], pts.dtype)
    call("sr_voxel_group", dev, n, ptr(pts), f64(pts), ptr(sem), 0 if sem is None else sem.element_size(), (C.c_double * 3)(*[float(x) for x in lo]),
         float(c["points"].dtype.type(c["voxel_size"])), offset, *buf(ws), ptr(counts))
    nv, m, bad = (int(x) for x in counts.cpu().numpy())
    assert bad == 0 and 0 <= m <= nv <= n
    pad = 3                                                 # rows past m stay untouched
    out = {"points": torch.full((m + pad, 3), -7.0, device=dev),
           "colors": None if col is None else torch.full((m + pad, 3), -7.0, device=dev),
           "normals": None if nrm is None else torch.full((m + pad, 3), -7.0, device=dev),
           "semantics": None if sem is None else torch.full((m + pad,), -7, dtype=torch.int32, device=dev),
           "counts": torch.full((m + pad,), -7, dtype=torch.int32, device=dev), "index": torch.full((m + pad,), -7, dtype=torch.int64, device=dev)}
    call("sr_voxel_emit", dev, n, ptr(pts), f64(pts), ptr(col), f64(col), ptr(nrm), f64(nrm), *buf(ws), nv, m, ptr(out["points"]), ptr(out["colors"]),
         ptr(out["normals"]), ptr(out["semantics"]), ptr(out["counts"]), ptr(out["index"]))
    got = {}
    for key, t in out.items():
        if t is None:
            got[key] = None
            continue
        assert bool((t[m:] == -7).all()), f"{c['name']}: {key} written past row m"
        got[key] = t[:m].cpu().numpy()
        if key in ("counts", "index"):
            assert (got[key] >= 0).all(), f"{c['name']}: a row of {key} was not written"
    return got


@pytest.mark.parametrize("name", vc.NAMES)
def test_every_case_through_the_raw_c_abi(name):
    vc.compare(name, _raw(vc.case(name)), "sr_voxel_*")


def test_refusals():
    for name, kw, fragment in vc.refusals():
        args = {k: (_up(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        with pytest.raises(ValueError, match=fragment):
            V.voxel_down_sample(**args)
    c = vc.case("negative")
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        V.voxel_down_sample(torch.from_numpy(c["points"]), 0.3)
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        V.voxel_down_sample(_up(c["points"]), 0.3, colors=torch.from_numpy(c["colors"]))
    # a float16 cloud is neither of the two dtypes
    with pytest.raises(ValueError, match="float32 or float64"):
        V.voxel_down_sample(_up(c["points"]).half(), 0.3)


def test_non_default_stream_and_non_contiguous_inputs():
    c = vc.case("mix_20000_f32")
    want = _run(c)
    wide = _up(np.repeat(c["points"], 2, axis=1))
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        cloud, counts, index = V.voxel_down_sample(strided, c["voxel_size"], _up(c["colors"]), _up(c["normals"]), _up(c["semantics"]),
                                                   return_counts=True, return_index=True)
    stream.synchronize()
    got = {"points": _np(cloud.points), "colors": _np(cloud.colors), "normals": _np(cloud.normals), "semantics": _np(cloud.semantics),
           "counts": _np(counts), "index": _np(index)}
    for key, a in want.items():
        assert a.tobytes() == got[key].tobytes(), key


def test_cloud_method_and_plain_return():
    c = vc.case("negative")
    cloud = V.SemanticCloud(c["points"].astype(np.float64), c["colors"], c["normals"], c["semantics"][:, None], {"road": 0}, device=DEV)
    assert cloud.points.is_cuda and cloud.points.dtype == torch.float64
    down = cloud.voxel_down_sample(0.3)
    assert isinstance(down, V.SemanticCloud) and down.semantics_dict == {"road": 0}
    assert down.points.dtype == torch.float32 and down.semantics.dtype == torch.int32 and down.points.shape[0] == down.semantics.shape[0] > 0
    same = cloud.voxel_down_sample_with_no_grad(0.3)
    assert torch.equal(same.points, down.points) and torch.equal(same.semantics, down.semantics)


def test_create_from_pcd_end_to_end():
    """3 000 points -> downsample -> model -> one 64 x 64 render: a finite image, and _scaling is the formula applied to dist3knn of the points."""
    from simple_knn._C import dist3knn
    from streetunveiler_amd.gaussian_renderer import PipelineParams, render
    from streetunveiler_amd.synthetic import synthetic_camera
    r = np.random.default_rng(8)
    W = H = 64
    pts = np.stack([r.random(3000) * 4 - 2, r.random(3000) * 4 - 2, 4 + r.random(3000) * 3], 1)         # in front of a camera at the origin
    sem = (pts[:, 0] > 0).astype(np.int32)
    down = V.SemanticCloud(pts, r.random((3000, 3)), None, sem, device=DEV).voxel_down_sample(0.25)
    P = down.points.shape[0]
    assert 100 < P < 3000
    g = torch.Generator(device=DEV).manual_seed(3)
    model = V.create_from_pcd(down, 2.5, max_sh_degree=3, generator=g)
    assert model.raw and model.spatial_lr_scale == 2.5 and model.active_sh_degree == 0 and model.max_sh_degree == 3
    for t, shape in ((model._xyz, (P, 3)), (model._scaling, (P, 2)), (model._rotation, (P, 4)), (model._opacity, (P, 1)), (model._features, (P, 16, 3))):
        assert t.is_leaf and t.requires_grad and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_cuda
    assert model._semantics.dtype == torch.int32 and tuple(model._semantics.shape) == (P,) and torch.equal(model._semantics, down.semantics)
    assert tuple(model.max_radii2D.shape) == (P,) and not bool(model.max_radii2D.any())
    assert torch.equal(model._xyz.detach(), down.points)
    want = torch.log(torch.sqrt(torch.clamp_min(dist3knn(down.points), 0.0000001)))[..., None].repeat(1, 2)
    assert torch.equal(model._scaling.detach(), want)
    assert torch.equal(model._features.detach()[:, 0, :], (down.colors - 0.5) / 0.28209479177387814) and not bool(model._features.detach()[:, 1:, :].any())
    assert float((model._opacity.detach() - math.log(0.1 / 0.9)).abs().max()) < 1e-6
    g2 = torch.Generator(device=DEV).manual_seed(3)
    assert torch.equal(model._rotation.detach(), torch.rand((P, 4), device=DEV, generator=g2))
    cam = synthetic_camera(W, H).to(DEV)
    out = render(cam, model, PipelineParams(), torch.zeros(3, device=DEV))
    image = out["render"]
    assert tuple(image.shape) == (3, H, W) and bool(torch.isfinite(image).all()) and float(image.detach().max()) > 0
    image.sum().backward()
    assert model._xyz.grad is not None and bool(torch.isfinite(model._xyz.grad).all())

"""-m gpu: the frame masks of the unveiling stage (csrc/unveil.hip) on every case of tests/unveil_cases.py under its bars -- through the
Python functions and through the raw C-ABI calls with caller-owned, sentinel-filled buffers, two runs bit for bit, on a non-default
stream, against the float32 twin on the same GPU where a case is all-robust -- the error paths, the out-of-range counter on an undersized
map, and one synthetic scene end to end: render, render_with_mask, inpaint_conditions against the checker fed the same two dicts."""
import numpy as np
import pytest
import torch

from streetunveiler_amd import _lib as L
from streetunveiler_amd import unveil as U
from streetunveiler_amd._call import buf, call, ptr
from tests import unveil_cases as uc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _sentinel(shape, dtype=torch.uint8):
    return torch.full(shape, SENTINEL, dtype=torch.uint8, device=DEV) if dtype == torch.uint8 else torch.full(shape, -7, dtype=dtype, device=DEV)


# ---- the dilation ---------------------------------------------------------------------------------------------------------------------
def _raw_dilate(m, k):
    t = _up(m)
    out = _sentinel(t.shape)
    call("sr_dilate_mask", torch.device(DEV), t.shape[0], t.shape[1], k, ptr(t), ptr(out))
    assert bool((out <= 1).all()), "a byte was not written (or is neither 0 nor 1)"
    return out.bool().cpu().numpy()


def test_dilate_every_case():
    uc.compare_dilation(lambda m, k: U.dilate_mask(_up(m), k).cpu().numpy(), "dilate_mask")
    uc.compare_dilation(_raw_dilate, "sr_dilate_mask")


def test_dilate_bool_non_contiguous_stream_and_repeat():
    for H, W in ((37, 53), (40, 130)):
        m = uc.mask_case("random_50", H, W)
        wide = _up(np.repeat(m, 2, axis=1))
        strided = wide[:, ::2]                                   # uint8, non-contiguous
        assert not strided.is_contiguous()
        transposed = _up(np.ascontiguousarray(m.T != 0)).T       # bool, non-contiguous
        assert not transposed.is_contiguous() and transposed.dtype == torch.bool
        stream = torch.cuda.Stream()
        for k in uc.KS:
            want = uc.dilated("random_50", H, W, k)
            first = U.dilate_mask(strided, k)
            assert np.array_equal(first.cpu().numpy(), want) and np.array_equal(U.dilate_mask(transposed, k).cpu().numpy(), want)
            assert torch.equal(U.dilate_mask(strided, k), first)                      # equal inputs, equal bits
            with torch.cuda.stream(stream):
                on_stream = U.dilate_mask(strided, k)
            stream.synchronize()
            assert torch.equal(on_stream, first)
            assert torch.equal(U.dilate_mask_torch(strided, k), first)                # the stock-torch twin on the same GPU


def _gpu_threshold(op, raw):
    def run(a, b, mask, k):
        a, b, mask = _up(a), _up(b), _up(mask)
        if not raw:
            return (U.instance_pixel_mask(a, b, 0.01, k) if op == "instance" else U.refill_mask(a, b, mask, 2e-2, k)).cpu().numpy()
        H, W = a.shape[1:]
        out = _sentinel((H, W))
        if op == "instance":
            call("sr_instance_pixel_mask", torch.device(DEV), H, W, ptr(a), ptr(b), 0.01, k, ptr(out))
        else:
            call("sr_refill_mask", torch.device(DEV), H, W, a.shape[0], ptr(a), ptr(b), ptr(mask), 2e-2, k, ptr(out))
        assert bool((out <= 1).all())
        return out.bool().cpu().numpy()
    return run


@pytest.mark.parametrize("op", ["instance", "refill"])
def test_fused_threshold_masks(op):
    uc.compare_threshold(op, _gpu_threshold(op, False), op)
    uc.compare_threshold(op, _gpu_threshold(op, True), "sr_" + op)
    c = uc.threshold_case(op, 37, 53)      # against the float32 twin on the same GPU (every compared pixel) and twice
    a, b, mask = _up(c.a), _up(c.b), _up(c.mask)
    for k in (1, 5, 10):
        if op == "instance":
            got, twin = U.instance_pixel_mask(a, b, 0.01, k), U.instance_pixel_mask_torch(a, b, 0.01, k, torch.float32)
            again = U.instance_pixel_mask(a[0], b[0], 0.01, k)      # [H,W] as well as [1,H,W]
        else:
            got, twin = U.refill_mask(a, b, mask, 2e-2, k), U.refill_mask_torch(a, b, mask, 2e-2, k, torch.float32)
            again = U.refill_mask(a, b, mask != 0, 2e-2, k)         # a bool mask as well as uint8
        assert torch.equal(got, again)
        if k == 1:
            keep = _up(c.compare)
            assert torch.equal(got[keep], twin[keep])


# ---- the condition images -------------------------------------------------------------------------------------------------------------
def _raw_conditions(full, bg, sky, H, W):
    out = {"mask": _sentinel((H, W))}
    for name, channels in U.CONDITION_IMAGES:
        out[name] = _sentinel((H, W, channels))
    c = lambda t: t.contiguous()
    call("sr_inpaint_conditions", torch.device(DEV), H, W, ptr(c(full["render"])), ptr(c(full["rend_alpha"])), ptr(c(bg["render"])), ptr(c(bg["rend_alpha"])),
         ptr(c(bg["surf_depth"])), ptr(c(bg["rend_normal"])), ptr(c(sky)), 0.01, 5, ptr(out["mask"]), *(ptr(out[name]) for name, _ in U.CONDITION_IMAGES))
    assert bool((out["mask"] <= 1).all())
    out["mask"] = out["mask"].bool()
    return out


@pytest.mark.parametrize("size", uc.CONDITION_SIZES)
def test_inpaint_conditions(size):
    H, W = size
    full, bg, sky = uc.condition_tensors(H, W, DEV)
    got = U.inpaint_conditions(full, bg, sky, 0.01, 5)
    uc.compare_conditions({k: v.cpu().numpy() for k, v in got.items()}, H, W, "inpaint_conditions")
    raw = _raw_conditions(full, bg, sky, H, W)
    again = U.inpaint_conditions(full, bg, sky, 0.01, 5)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        on_stream = U.inpaint_conditions(full, bg, sky, 0.01, 5)
    stream.synchronize()
    twin = U.inpaint_conditions_torch(full, bg, sky, 0.01, 5, torch.float32)
    for key in got:
        assert torch.equal(got[key], raw[key]) and torch.equal(got[key], again[key]) and torch.equal(got[key], on_stream[key]), key
    assert torch.equal(got["mask"], twin["mask"])
    for name, _ in U.CONDITION_IMAGES:      # the float32 twin on the same GPU: one byte at most, and only where the truth says a byte may move
        diff = (got[name].int() - twin[name].int()).abs()
        assert int(diff.max()) <= 1, name


# ---- points ---------------------------------------------------------------------------------------------------------------------------
def _raw_points(xyz, camera, coords):
    dev = torch.device(DEV)
    P = xyz.shape[0]
    cam = U.pack_cameras(camera, dev)
    mask = _sentinel((P,))
    ws = torch.empty((L.load().sr_unveil_workspace_bytes(P, 1),), dtype=torch.uint8, device=DEV)
    count = _sentinel((1,), torch.int32)
    call("sr_points_in_frame", dev, P, ptr(xyz), ptr(cam.cams), ptr(cam.hw), ptr(mask), *buf(ws), ptr(count) if coords else None)
    assert bool((mask <= 1).all())
    if not coords:
        return mask.bool()
    n = int(count.item())
    pix, depth = _sentinel((n, 2), torch.int64), _sentinel((n,), torch.float32)
    call("sr_points_in_frame_emit", dev, P, ptr(xyz), ptr(cam.cams), ptr(cam.hw), *buf(ws), n, ptr(pix), ptr(depth))
    return mask.bool(), pix, depth


@pytest.mark.parametrize("name", uc.POINT_CASES)
def test_points_in_frame(name):
    c = uc.point_case(name)
    xyz, cloud = uc.xyz_tensor(c, DEV), _up(uc.robust_cloud(name))
    stream = torch.cuda.Stream()
    for f in range(len(c.cameras)):
        camera = c.cameras.frame(f)
        mask = U.points_in_frame(xyz, camera)
        uc.compare_in_frame(name, f, mask.cpu().numpy(), "points_in_frame")
        with_coords = U.points_in_frame(xyz, camera, coords=True)
        assert torch.equal(with_coords[0], mask) and torch.equal(_raw_points(xyz, camera, False), mask)
        assert with_coords[1].shape == (int(mask.sum()), 2) and with_coords[2].shape == (int(mask.sum()),)
        # the all-robust cloud: mask, order and pix exactly, depth under its bar; raw, twice, on a stream, and the float32 twin on this GPU
        got = U.points_in_frame(cloud, camera, coords=True)
        uc.compare_lists(cloud.cpu().numpy(), camera, *(t.cpu().numpy() for t in got), f"points_in_frame {name} frame {f}")
        raw, again = _raw_points(cloud, camera, True), U.points_in_frame(cloud, camera, coords=True)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            on_stream = U.points_in_frame(cloud, camera, coords=True)
        stream.synchronize()
        twin = U.points_in_frame_torch(cloud, camera, True, torch.float32)
        for k in range(3):
            assert torch.equal(got[k], raw[k]) and torch.equal(got[k], again[k]) and torch.equal(got[k], on_stream[k]), k
        assert torch.equal(got[0], twin[0]) and torch.equal(got[1], twin[1])


@pytest.mark.parametrize("name", uc.POINT_CASES)
def test_frame_visibility(name):
    c = uc.point_case(name)
    cloud = _up(uc.robust_cloud(name))
    P, F = cloud.shape[0], len(c.cameras)
    count, depth_sum = U.frame_visibility(cloud, c.cameras)
    uc.compare_visibility(cloud.cpu().numpy(), c.cameras, count.cpu().numpy(), depth_sum.cpu().numpy(), f"frame_visibility {name}")
    dev = torch.device(DEV)
    packed = U.pack_cameras(c.cameras, dev)
    raw_count, raw_sum = _sentinel((F,), torch.int64), _sentinel((F,), torch.float64)
    ws = torch.empty((L.load().sr_unveil_workspace_bytes(P, F),), dtype=torch.uint8, device=DEV)
    call("sr_frame_visibility", dev, P, F, ptr(cloud), ptr(packed.cams), ptr(packed.hw), *buf(ws), ptr(raw_count), ptr(raw_sum))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        on_stream = U.frame_visibility(cloud, packed)      # the packed form is accepted as well
    stream.synchronize()
    again = U.frame_visibility(cloud, c.cameras)
    for a, b in ((raw_count, raw_sum), on_stream, again):
        assert torch.equal(a, count) and torch.equal(b.view(torch.int64), depth_sum.view(torch.int64))      # bit for bit
    assert torch.equal(count, U.frame_visibility_torch(cloud, c.cameras, "keep", torch.float32)[0])         # the float32 twin on this GPU


def test_frame_visibility_is_one_sum_whatever_the_block_count():
    """More than one block of 2048 points per frame, and a point count that is no multiple of anything: against the per-frame lists."""
    c = uc.point_case("general_P4097_F3_v1")
    cloud = _up(uc.robust_cloud(c.name))
    assert cloud.shape[0] > 2048
    count, depth_sum = U.frame_visibility(cloud, c.cameras)
    for f in range(3):
        _, _, depth = U.points_in_frame(cloud, c.cameras.frame(f), coords=True)
        assert int(count[f]) == depth.shape[0] > 0
        # the same float32 depths added as doubles in another order: n 2^-53 of the sum apart at most
        assert abs(float(depth_sum[f]) - float(depth.double().sum())) <= 4097 * 2.0 ** -53 * float(depth.double().sum())


@pytest.mark.parametrize("name", uc.PICK_CASES)
def test_pick_view(name):
    xyz, cameras = uc.pick_case(name)
    assert U.pick_view(_up(xyz).reshape(-1, 3), cameras, 10.0) == uc.pick_expected(name)


@pytest.mark.parametrize("name", uc.POINT_CASES)
def test_semantic_mask_of_points(name):
    c = uc.point_case(name)
    xyz, cloud = uc.xyz_tensor(c, DEV), _up(uc.robust_cloud(name)).reshape(-1, 3)
    dev = torch.device(DEV)
    for undersized in (False, True):      # undersized: nothing is read outside the map, and the count is the checker's
        maps = uc.semantic_maps(name, undersized)
        padded = torch.full((maps.shape[0], maps.shape[1] + 2, maps.shape[2] + 2), 2, dtype=torch.uint8, device=DEV)      # label 2 remains: a read
        padded[:, 1:-1, 1:-1] = _up(maps)                                                                              # outside the map would set a point
        resident = padded[:, 1:-1, 1:-1].contiguous()
        want, _ = uc.semantic_expected(c.xyz, c.cameras, maps)
        mask, _ = U.semantic_mask_of_points(xyz, c.cameras, resident, uc.REMAIN_BIT)
        robust = c.robust.all(axis=0)
        assert np.array_equal(mask.cpu().numpy()[robust], want[robust])
        want, want_outside = uc.semantic_expected(cloud.cpu().numpy(), c.cameras, maps)
        mask, outside = U.semantic_mask_of_points(cloud, c.cameras, resident, uc.REMAIN_BIT)
        assert np.array_equal(mask.cpu().numpy(), want) and int(outside.item()) == want_outside
        assert want_outside == 0 or undersized
        P, F = cloud.shape[0], len(c.cameras)
        packed = U.pack_cameras(c.cameras, dev, None)
        raw_mask, raw_outside = _sentinel((P,)), _sentinel((1,), torch.int64)
        call("sr_semantic_mask_of_points", dev, P, F, ptr(cloud), ptr(packed.cams), ptr(packed.hw), ptr(resident), resident.shape[1], resident.shape[2],
             uc.REMAIN_BIT & 0xFFFFFFFF, ptr(raw_mask), ptr(raw_outside))
        assert torch.equal(raw_mask.bool(), mask) and bool((raw_mask <= 1).all()) and torch.equal(raw_outside, outside)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            on_stream = U.semantic_mask_of_points(cloud, c.cameras, resident, uc.REMAIN_BIT)
        stream.synchronize()
        assert torch.equal(on_stream[0], mask) and torch.equal(on_stream[1], outside)
        twin, twin_outside = U.semantic_mask_of_points_torch(cloud, c.cameras, resident, uc.REMAIN_BIT, torch.float32)      # on this GPU
        assert torch.equal(twin, mask) and twin_outside == want_outside


def test_semantic_labels_of_31_and_more_match_nothing():
    c = uc.point_case("mixed_P65_F1_v0")
    cloud = _up(uc.robust_cloud(c.name))
    in_frame = U.points_in_frame(cloud, c.cameras.frame(0)._replace(max_z=None))
    assert bool(in_frame.any())
    for label, bit, hit in ((31, 0xFFFFFFFF, False), (40, 0xFFFFFFFF, False), (255, 0xFFFFFFFF, False), (30, 1 << 30, True), (30, 1 << 29, False), (0, 1, True)):
        maps = torch.full((1, 32, 64), label, dtype=torch.uint8, device=DEV)
        mask, outside = U.semantic_mask_of_points(cloud, c.cameras, maps, bit)
        assert torch.equal(mask, in_frame if hit else torch.zeros_like(mask)) and int(outside.item()) == 0, (label, bit)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = uc.point_case("mixed_P65_F3_v0")
    xyz = uc.xyz_tensor(c, DEV)
    m = _up(uc.mask_case("random_50", 37, 53))
    a = torch.rand(1, 37, 53, device=DEV)
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        U.dilate_mask(m.cpu(), 5)
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        U.points_in_frame(xyz.cpu(), c.cameras.frame(0))
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        U.instance_pixel_mask(a.cpu(), a.cpu())
    with pytest.raises(L.SurfelRasterError, match="resident"):
        U.semantic_mask_of_points(xyz, c.cameras, torch.zeros(3, 60, 100, dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="float32"):
        U.points_in_frame(xyz.double(), c.cameras.frame(0))
    with pytest.raises(ValueError, match="bool or torch.uint8|uint8"):
        U.dilate_mask(m.float(), 5)
    with pytest.raises(ValueError, match="float32"):
        U.instance_pixel_mask(a.double(), a.double())
    with pytest.raises(ValueError, match="uint8"):
        U.semantic_mask_of_points(xyz, c.cameras, torch.zeros(3, 60, 100, dtype=torch.int32, device=DEV), 1)
    for k in (0, 32):
        with pytest.raises(ValueError, match="1..31"):
            U.dilate_mask(m, k)
        with pytest.raises(ValueError, match="1..31"):
            U.instance_pixel_mask(a, a, 0.01, k)
        out = torch.empty_like(m)
        with pytest.raises(L.SurfelRasterError, match=r"sr_dilate_mask failed \(-1\): k = %d not in 1..31" % k):
            call("sr_dilate_mask", torch.device(DEV), 37, 53, k, ptr(m), ptr(out))
    # packed cameras go to the kernels as addresses: another device, dtype or shape is refused by every per-point entry
    maps = torch.zeros(3, 60, 100, dtype=torch.uint8, device=DEV)
    on_host = U.pack_cameras(c.cameras, "cpu")
    good = U.pack_cameras(c.cameras, DEV)
    assert good.cams.device == xyz.device and U.pack_cameras(good, DEV) is good
    wrong = {"no CPU path": on_host,
             r"float32 tensor \[F,24\]": U.PackedCameras(good.cams.double(), good.hw),
             r"float32 tensor \[F,24\] ": U.PackedCameras(good.cams[:, :23], good.hw),
             r"contiguous float32": U.PackedCameras(good.cams.repeat(1, 2)[:, ::2], good.hw),
             r"int32 tensor \[\d,2\]": U.PackedCameras(good.cams, good.hw.long()),
             r"int32 tensor \[3,2\]": U.PackedCameras(good.cams, good.hw[:2]),
             "the call is on": U.PackedCameras(good.cams, good.hw.cpu())}
    for message, packed in wrong.items():
        error = L.SurfelRasterError if packed.cams.device != xyz.device or packed.hw.device != xyz.device else ValueError
        ops = [lambda p: U.frame_visibility(xyz, p), lambda p: U.pick_view(xyz, p), lambda p: U.semantic_mask_of_points(xyz, p, maps, 1)]
        if packed.hw.shape[0] == 3:      # (one camera of the pack: a pack with too few (h, w) rows has nothing wrong in its first)
            ops.append(lambda p: U.points_in_frame(xyz, U.PackedCameras(p.cams[:1], p.hw[:1])))
        for op in ops:
            with pytest.raises(error, match=message.strip()):
                op(packed)
    if torch.cuda.device_count() > 1:      # resident, but on another GPU than the points
        with pytest.raises(L.SurfelRasterError, match="device of the call"):
            U.semantic_mask_of_points(xyz, c.cameras, maps.to("cuda:1"), 1)
        with pytest.raises(L.SurfelRasterError, match="the call is on"):
            U.frame_visibility(xyz, U.pack_cameras(c.cameras, "cuda:1"))
    # shapes the dilation's launch cannot address are refused by name, before any HIP call
    out = torch.empty_like(m)
    for H, W, what in ((32 * 65535 + 1, 1, "rows"), (1, 2 ** 31 - 128, "columns"), (65536, 65536, "int32")):
        with pytest.raises(L.SurfelRasterError, match=r"sr_dilate_mask failed \(-4\): .*" + what):
            call("sr_dilate_mask", torch.device(DEV), H, W, 5, ptr(m), ptr(out))
    with pytest.raises(ValueError, match="2 semantic maps for 3 cameras"):
        U.semantic_mask_of_points(xyz, c.cameras, torch.zeros(2, 60, 100, dtype=torch.uint8, device=DEV), 1)
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        U.frame_visibility(xyz[:, :2], c.cameras)
    with pytest.raises(ValueError, match="one camera"):
        U.points_in_frame(xyz, c.cameras)
    with pytest.raises(ValueError):
        U.refill_mask(torch.rand(3, 37, 53, device=DEV), torch.rand(3, 37, 52, device=DEV), m)
    with pytest.raises(L.SurfelRasterError, match="workspace"):
        packed = U.pack_cameras(c.cameras, torch.device(DEV))
        count, depth_sum = torch.empty(3, dtype=torch.int64, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV)
        ws = torch.empty(16, dtype=torch.uint8, device=DEV)
        call("sr_frame_visibility", torch.device(DEV), 65, 3, ptr(xyz), ptr(packed.cams), ptr(packed.hw), *buf(ws), ptr(count), ptr(depth_sum))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
class _Cloud:
    """A trained model's getters, from the synthetic scene."""

    def __init__(self, g):
        self.get_xyz, self.get_features = g["means3D"].to(DEV), g["shs"].to(DEV)
        self.get_opacity, self.get_scaling, self.get_rotation = g["opacities"].to(DEV), g["scales"].to(DEV), g["rotations"].to(DEV)
        self.active_sh_degree = self.max_sh_degree = 3


def test_synthetic_scene_end_to_end():
    from streetunveiler_amd.gaussian_renderer import PipelineParams, render, render_with_mask
    from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians
    W, H, P = 80, 56, 300
    pc = _Cloud(synthetic_gaussians(P, W, H, seed=11, scale_lo=3e-3, scale_hi=5e-2))
    cam, bg, pipe = synthetic_camera(W, H).to(DEV), torch.zeros(3, device=DEV), PipelineParams()
    removed = (torch.arange(P, device=DEV) % 4) == 0
    sky = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        full, background = render(cam, pc, pipe, bg), render_with_mask(cam, pc, pipe, bg, ~removed)
    got = U.inpaint_conditions(full, background, sky)
    want = U.inpaint_conditions_torch(full, background, sky, 0.01, 5, torch.float64, values=True)
    raw = U.instance_pixel_mask_torch(full["rend_alpha"], background["rend_alpha"], 0.01, 5, torch.float64, undilated=True)
    assert 0 < int(raw.sum()) < H * W, "the scene must have an instance to remove"
    d = (full["rend_alpha"].double() - background["rend_alpha"].double()).abs()
    sure = ((d - float(np.float32(0.01))).abs() > 4 * float(np.spacing(np.float32(0.01)))).all()
    if bool(sure):
        assert torch.equal(got["mask"], want["mask"])
    assert torch.equal(got["mask"], U.dilate_mask(U.instance_pixel_mask(full["rend_alpha"], background["rend_alpha"], 0.01, 1), 5))
    for name, channels in U.CONDITION_IMAGES:
        g, w, v = got[name].cpu().numpy(), want[name].cpu().numpy(), want[name + "_value"].cpu().numpy()
        diff = np.abs(g.astype(np.int32) - w.astype(np.int32))
        assert g.shape == (H, W, channels) and diff.max() <= 1 and not diff[~uc.byte_band(v)].any(), name
        # (an empty pixel's normal is exactly 0: 255 * 0.5 + 0.5 = 128 is an integer, exact for everyone -- the share is taken over the rest)
        counted = (background["rend_normal"] != 0).permute(1, 2, 0).cpu().numpy() if name == "inpainted_normal" else np.ones_like(v, dtype=bool)
        assert counted.any() and uc.byte_band(v)[counted].mean() <= uc.BYTE_EXCLUDED_SHARE, name
    assert got["empty_opacity"].max() > 0 and got["inpainted_depth"].max() > 0

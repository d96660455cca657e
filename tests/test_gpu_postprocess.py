"""GPU (-m gpu): csrc/postprocess.hip -- the forward kernel and the two backward kernels -- held per output map and per gradient channel to
the bar of tests/postprocess_cases.py (float64 truth, the float32 restatement's own deviation as the yardstick), at every size x depth ratio
x camera of that module; and the paths autograd never takes: null upstream gradients at the C-ABI, buffers whose previous content must not
matter, borrowed / float64 inputs, and the elements around every output at the sizes without an interior."""
import numpy as np
import pytest
import torch

from streetunveiler_amd._call import call, ptr
from streetunveiler_amd.gaussian_renderer import PipelineParams, postprocess_allmap
from tests import postprocess_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UPS = ("rend_normal", "surf_depth", "surf_normal", "surf_point")     # the C-ABI's order
GUARD = 1024                                                         # floats on either side of a guarded buffer (a multiple of the 256 B line)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("cam_name", pc.CAMERAS)
@pytest.mark.parametrize("ratio", pc.RATIOS)
@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maps_and_gradient_within_bar(size, ratio, cam_name):
    """Forward maps and the allmap gradient: with seeded upstream gradients on all four maps, and with surf_normal's alone (the stencil
    path standing by itself)."""
    for which in pc.UPSTREAMS:
        c = pc.case(size[0], size[1], ratio, cam_name, which)
        got = pc.run_hip(c["cam"], ratio, c["allmap"], c["upstream"], DEV)
        assert all(np.isfinite(v).all() for v in got.values()), c["name"]
        pc.assert_within_bar(got, c["truth"], c["ref"], "postprocess.hip " + c["name"])


def _guarded(n, fill=float("nan")):
    """-> (whole buffer, the n floats in its middle)"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_untouched(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


def _abi_forward(cam, ratio, allmap, outs=None):
    """sr_postprocess_forward on caller-owned buffers -> (rend_normal, surf_depth, surf_normal, surf_point)"""
    W, H = cam.image_width, cam.image_height
    view = cam.world_view_transform.to(DEV).contiguous().float()
    if outs is None:
        outs = [torch.full((ch * H * W,), float("nan"), device=DEV) for ch in (3, 1, 3, 3)]
    call("sr_postprocess_forward", view.device, W, H, cam.FoVx, cam.FoVy, ratio, ptr(view), ptr(allmap), *map(ptr, outs))
    torch.cuda.synchronize()
    return outs


def _abi_backward(cam, ratio, allmap, ups, scratch=None, g_allmap=None, scratch_fill=float("nan")):
    """sr_postprocess_backward with `ups` = the four upstream gradients in the C-ABI's order (None = a null pointer); the scratch buffer
    and g_allmap start out as NaN unless handed in."""
    W, H = cam.image_width, cam.image_height
    view = cam.world_view_transform.to(DEV).contiguous().float()
    scratch = torch.full((6 * H * W,), scratch_fill, device=DEV) if scratch is None else scratch
    g_allmap = torch.full((7 * H * W,), float("nan"), device=DEV) if g_allmap is None else g_allmap
    call("sr_postprocess_backward", view.device, W, H, cam.FoVx, cam.FoVy, ratio, ptr(view), ptr(allmap), *map(ptr, ups), ptr(scratch), ptr(g_allmap))
    torch.cuda.synchronize()
    return g_allmap


def _inputs(W, H, cam_name, which="all"):
    c = pc.case(W, H, 0.4, cam_name, which)
    return c, c["allmap"].to(DEV).contiguous(), [c["upstream"][k].to(DEV).contiguous() for k in UPS]


@pytest.mark.parametrize("size", ((3, 3), (65, 5), (131, 77)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_null_upstream_pointers_equal_zero_tensors(size):
    """Each upstream pointer null in turn, and all but one null: the bits of the same call with a zero tensor in that place.  Scratch and
    g_allmap start as NaN: every element of g_allmap must have been written, and what the scratch held must not matter."""
    c, allmap, ups = _inputs(size[0], size[1], "scaled")
    zeros = [torch.zeros_like(u) for u in ups]
    full = _abi_backward(c["cam"], c["ratio"], allmap, ups)
    assert torch.isfinite(full).all()
    np.testing.assert_array_equal(full.reshape(7, size[1], size[0]).cpu().numpy(), pc.run_hip(c["cam"], c["ratio"], c["allmap"], c["upstream"], DEV)["g_allmap"])
    patterns = [[j != i for j in range(4)] for i in range(4)] + [[j == i for j in range(4)] for i in range(4)]      # True = given
    for given in patterns:
        with_null = _abi_backward(c["cam"], c["ratio"], allmap, [u if g else None for u, g in zip(ups, given)])
        with_zero = _abi_backward(c["cam"], c["ratio"], allmap, [u if g else z for u, z, g in zip(ups, zeros, given)], scratch_fill=0.0)
        assert torch.isfinite(with_null).all(), given
        assert _same_bits(with_null, with_zero), given
    # all four given differs from every pattern above wherever an upstream matters (the null branches are not the only ones taken)
    assert not _same_bits(full, with_null)


@pytest.mark.parametrize("cam_name", ("posed", "scaled"))
def test_two_runs_from_equal_inputs_give_equal_bits(cam_name):
    c, allmap, ups = _inputs(131, 77, cam_name)
    fwd = [_abi_forward(c["cam"], c["ratio"], allmap) for _ in range(2)]
    bwd = [_abi_backward(c["cam"], c["ratio"], allmap, ups, scratch_fill=fill) for fill in (float("nan"), 7.0)]
    assert all(_same_bits(a, b) for a, b in zip(*fwd)) and _same_bits(*bwd)
    assert all(torch.isfinite(o).all() for o in fwd[0]) and torch.isfinite(bwd[0]).all()


def test_borrowed_and_float64_inputs_give_the_bits_of_the_contiguous_float32_call():
    """A channel slice of a larger tensor (a storage offset), a strided view, and a float64 allmap."""
    W, H = 65, 5
    c = pc.case(W, H, 0.4, "posed", "all")
    cam, pipe = c["cam"].to(DEV), PipelineParams(depth_ratio=c["ratio"])

    def run(a):
        a = a.requires_grad_()
        out = postprocess_allmap(cam, pipe, a)
        sum((out[k] * v.to(DEV)).sum() for k, v in c["upstream"].items()).backward()
        return [out[k].detach() for k in pc.ALL_MAPS], a.grad

    maps, grad = run(c["allmap"].to(DEV))
    big = torch.full((12, H, W), float("nan"), device=DEV)
    big[2:9] = c["allmap"].to(DEV)
    big.requires_grad_()
    out = postprocess_allmap(cam, pipe, big[2:9])
    sum((out[k] * v.to(DEV)).sum() for k, v in c["upstream"].items()).backward()
    assert all(_same_bits(a, b) for a, b in zip(maps, [out[k].detach() for k in pc.ALL_MAPS]))
    assert _same_bits(big.grad[2:9], grad) and not big.grad[:2].any() and not big.grad[9:].any()
    strided = c["allmap"].to(DEV).permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not strided.is_contiguous()
    maps_s, grad_s = run(strided.detach())
    assert all(_same_bits(a, b) for a, b in zip(maps, maps_s)) and _same_bits(grad, grad_s)
    maps_d, grad_d = run(c["allmap"].double().to(DEV))
    for k, a, b in zip(pc.ALL_MAPS, maps, maps_d):
        assert _same_bits(a, b.float()), k      # rend_alpha / rend_dist are views of the float64 input: equal values
    assert _same_bits(grad, grad_d.float())


@pytest.mark.parametrize("size", [s for s in pc.SIZES if s[0] < 16 or s[1] < 16], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nothing_written_outside_the_outputs_at_the_tiny_sizes(size):
    """Every output sits inside a larger NaN-filled buffer: the elements on both sides stay untouched.  The allmap and the upstream
    gradients sit inside NaN-filled buffers too and the results keep the bits of the plain call -- a neighbour read across the edge of
    the image would have brought a NaN in."""
    W, H = size
    c, allmap, ups = _inputs(W, H, "posed")
    plain_fwd = _abi_forward(c["cam"], c["ratio"], allmap)
    plain_bwd = _abi_backward(c["cam"], c["ratio"], allmap, ups)
    a_buf, a_in = _guarded(7 * H * W)
    a_in.copy_(allmap.reshape(-1))
    u_in = []
    for u in ups:
        _, v = _guarded(u.numel())
        v.copy_(u.reshape(-1))
        u_in.append(v)
    bufs = [_guarded(ch * H * W) for ch in (3, 1, 3, 3)]
    outs = _abi_forward(c["cam"], c["ratio"], a_in, [mid for _, mid in bufs])
    for (buf, mid), plain in zip(bufs, plain_fwd):
        assert _guards_untouched(buf) and torch.isfinite(mid).all() and _same_bits(mid, plain)
    (s_buf, s_mid), (g_buf, g_mid) = _guarded(6 * H * W), _guarded(7 * H * W)
    _abi_backward(c["cam"], c["ratio"], a_in, u_in, scratch=s_mid, g_allmap=g_mid)
    assert _guards_untouched(s_buf) and _guards_untouched(g_buf)
    assert torch.isfinite(s_mid).all() and torch.isfinite(g_mid).all() and _same_bits(g_mid, plain_bwd)
    assert torch.equal(_bits(a_buf[GUARD:-GUARD]), _bits(allmap.reshape(-1)))      # inputs are not written to

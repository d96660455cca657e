"""-m gpu: the fused photometric loss (csrc/image_loss.hip) against the reference's own numbers and against the float64 truth, under the
bar of tests/image_loss_cases.py (4 x the reference's own float32 deviation, per case and per quantity); run-to-run bit identity; the raw
forward + backward pair inside a HIP graph; and the parameter gradients of the rasterizer through it.

The edge cases of tests/image_loss_cases.py (tile seams, window-sized frames, 1 / 2 / 6 channels, more tiles than forward workgroups, lambda
0 and 1, planted degenerate content, a NaN pixel) run under the per-element bar and the max-norm rule both, through the operator and through
the raw pair on an oversized workspace with every buffer poisoned; upstream scalars 1, -2.5 and 0; a second backward on one workspace; the
wrapper's conversions (permuted views, [H,W] alpha, float64) against the contiguous float32 call's bits.  On image == gt the max-norm figure
is the ratio of two rounding residues over a truth of 7e-18 (the kernels' is 2.0 x the twin's): it holds, and says little; the per-element
bar is the judge there."""
import math

import pytest
import torch

from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
from streetunveiler_amd import _lib
from streetunveiler_amd.image_loss import (image_loss_backward, image_loss_forward, image_loss_workspace, photometric_loss,
                                           photometric_loss_torch)
from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians
from tests import image_loss_cases as ilc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = ilc.fixture_cases()


@pytest.mark.parametrize("case", FIXTURE, ids=[c["name"] for c in FIXTURE])
def test_hip_matches_the_reference_fixture(case):
    """Every fixture case: loss, l1, ssim and every gradient, against the float64 truth in units of the reference's own float32 deviation."""
    ilc.assert_within_bar(ilc.run_hip(case, DEV), case, "HIP vs truth")


@pytest.mark.parametrize("composite", [False, True], ids=["plain", "sky"])
@pytest.mark.parametrize("size", ilc.GPU_SIZES[:-1], ids=[f"{w}x{h}" for w, h in ilc.GPU_SIZES[:-1]])
def test_hip_matches_the_float64_truth(size, composite):
    """One pixel, frames narrower / lower than the window, a size that is no multiple of the tile, the `-r 4` frame: truth and d_ref from
    photometric_loss_torch on the CPU (float64 / float32)."""
    case = ilc.with_cpu_reference(ilc.seeded_case(size[0], size[1], composite))
    ilc.assert_within_bar(ilc.run_hip(case, DEV), case, "HIP vs truth")


def test_hip_matches_the_float64_truth_at_1920x1080():
    """The full frame, once, with the composite (every kernel path: sky, alpha and the three gradients)."""
    W, H = ilc.GPU_SIZES[-1]
    case = ilc.with_cpu_reference(ilc.seeded_case(W, H, True))
    ilc.assert_within_bar(ilc.run_hip(case, DEV), case, "HIP vs truth")


@pytest.mark.parametrize("composite", [False, True], ids=["plain", "sky"])
def test_two_runs_give_the_same_bits(composite):
    """No float atomics: fixed-order partial sums, one writer per output element."""
    case = ilc.seeded_case(1001, 611, composite, seed=3)
    runs = []
    for _ in range(2):
        leaves = [None if case[k] is None else case[k].to(DEV).requires_grad_() for k in ("image", "sky", "alpha")]
        out = photometric_loss(leaves[0], case["gt"].to(DEV), 0.2, leaves[1], leaves[2])
        grads = torch.autograd.grad(out[0], [t for t in leaves if t is not None])
        runs.append([o.detach().clone() for o in out] + list(grads))
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), f"output {k} differs between two runs"
    assert not out[1].requires_grad and not out[2].requires_grad and out[0].requires_grad     # l1, ssim: logging only


@pytest.mark.parametrize("composite", [False, True], ids=["plain", "sky"])
def test_forward_backward_pair_captures_into_a_hip_graph(composite):
    """No host read-back, no allocation by the library, no process-wide state: the raw pair is captured into a HIP graph (side-stream
    warm-up, a linear chain, no autograd inside the capture) and every replay returns the eager call's bits."""
    case = ilc.seeded_case(333, 201, composite, seed=5)
    image, gt = case["image"].to(DEV), case["gt"].to(DEV)
    sky, alpha = (None, None) if not composite else (case["sky"].to(DEV), case["alpha"].to(DEV))
    g = torch.tensor(0.75, device=DEV)
    ws, out3 = image_loss_workspace(image), torch.empty(3, device=DEV)
    grads = (torch.empty_like(image), None if sky is None else torch.empty_like(sky), None if sky is None else torch.empty_like(alpha))

    def pair():
        image_loss_forward(image, gt, 0.3, sky, alpha, workspace=ws, out=out3)
        image_loss_backward(image, gt, ws, g, 0.3, sky, alpha, out=grads)

    pair()
    torch.cuda.synchronize()
    outs = [out3] + [t for t in grads if t is not None]
    ref = [t.clone() for t in outs]
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()                                        # warm-up on a side stream, as torch's capture rules ask
    torch.cuda.current_stream().wait_stream(side); torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair()
    for _ in range(3):
        for o in outs: o.fill_(float("nan"))
        ws.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(ref, outs)):
            assert torch.equal(a, b), f"graph replay: output {k} differs from the eager call"
    # the upstream scalar is read from device memory at replay time: another g, other gradients, no new capture
    g.fill_(1.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out3, ref[0]) and torch.allclose(grads[0], 2.0 * ref[1], rtol=1e-6, atol=0)


EDGE = tuple(ilc.EDGE_CASES)
WALK = tuple(n for n in EDGE if n.startswith("walk_"))


def _assert_under_both_bars(got, case, what):
    """The per-element bar, and the max-norm rule on every quantity it can judge (a finite truth that is not identically zero)."""
    ilc.assert_within_edge_bar(got, case, what)
    old_got, old_case = ilc.where_the_old_rule_applies(got, case)
    ilc.assert_within_bar(old_got, old_case, what)


def _on_device(case):
    return [None if case[k] is None else case[k].to(DEV) for k in ("image", "gt", "sky", "alpha")]


def _operator(case, g_loss=1.0, inputs=None):
    """photometric_loss and its gradients under g_loss -> [loss, l1, ssim, g_image(, g_sky, g_alpha)] on the device"""
    image, gt, sky, alpha = _on_device(case) if inputs is None else inputs
    leaves = [t.requires_grad_() for t in (image, sky, alpha) if t is not None]
    out = photometric_loss(image, gt, case["lambda_dssim"], sky, alpha)
    grads = torch.autograd.grad(out[0], leaves, torch.tensor(g_loss, device=DEV, dtype=out[0].dtype))
    return [o.detach() for o in out] + list(grads)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", EDGE)
def test_edge_case_through_the_operator_under_both_bars(name):
    """Tile seams, window-sized frames, 1 / 2 / 6 channels, the forward's second trip through its tile walk, lambda 0 and 1, planted
    content (image == gt, all black, x == gt and alpha 0 / 1 across a seam, flat steps, values in [-50, 50]) and a NaN pixel, whose
    non-finite set must be the float64 checker's (tests/test_image_loss_host.py pins it) with the bar holding on every other element."""
    case = ilc.edge_case(name)
    _assert_under_both_bars(ilc.run_hip(case, DEV), case, "HIP vs truth")


@pytest.mark.parametrize("name", EDGE)
def test_edge_case_through_the_raw_pair_with_poisoned_buffers(name):
    """image_loss_forward / image_loss_backward on a workspace larger than required and full of NaN bytes, out3 and the gradient tensors
    NaN-filled before their call: the operator's bits, and no NaN left (a slot read before it was written, or an element never written,
    would show as one).  The NaN cases compare bits only."""
    case = ilc.edge_case(name)
    image, gt, sky, alpha = _on_device(case)
    want = _operator(case)
    need = image_loss_workspace(image).numel()
    ws = torch.full((need + 4096 + 12,), 0xFF, dtype=torch.uint8, device=DEV)
    nan_like = lambda t: None if t is None else torch.full_like(t, float("nan"))
    out3 = torch.full((3,), float("nan"), device=DEV)
    image_loss_forward(image, gt, case["lambda_dssim"], sky, alpha, workspace=ws, out=out3)
    grads = (nan_like(image), nan_like(sky), nan_like(alpha))
    image_loss_backward(image, gt, ws, torch.ones((), device=DEV), case["lambda_dssim"], sky, alpha, out=grads)
    torch.cuda.synchronize()
    got = [out3[0], out3[1], out3[2]] + [g for g in grads if g is not None]
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert _same_bits(a, b), f"{name}: output {k} of the raw pair differs from the operator's"
        assert ilc.EDGE_CASES[name][5] == "nan" or not torch.isnan(a).any(), f"{name}: a NaN is left in output {k}"
    assert bool((ws[need:] == 0xFF).all()), "the pair wrote past the workspace it asked for"


@pytest.mark.parametrize("g_loss", [1.0, -2.5, 0.0])
def test_upstream_scalar(g_loss):
    """g_loss = 0: every gradient element is zero; g_loss = -2.5: within the bar of -2.5 x the truth (u = 2.5 / N)."""
    case = ilc.with_upstream(ilc.edge_case(ilc.G_LOSS_CASE), g_loss)
    got = ilc.run_hip(case, DEV, g_loss=g_loss)
    if g_loss == 0.0:
        for k in ilc.GRADS:
            assert not case["truth"][k].any() and not got[k].any(), k
    _assert_under_both_bars(got, case, f"HIP vs truth, g_loss {g_loss}")


def test_backward_twice_on_one_workspace_gives_equal_bits():
    case = ilc.edge_case(ilc.G_LOSS_CASE)
    image, gt, sky, alpha = _on_device(case)
    out3, ws = image_loss_forward(image, gt, 0.2, sky, alpha)
    g = torch.tensor(-2.5, device=DEV)
    first = [t.clone() for t in image_loss_backward(image, gt, ws, g, 0.2, sky, alpha)]
    second = image_loss_backward(image, gt, ws, g, 0.2, sky, alpha)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(first, second)):
        assert _same_bits(a, b) and not torch.isnan(a).any(), k


@pytest.mark.parametrize("how", ["permuted_views", "alpha_hw", "float64"])
def test_wrapper_conversions_give_the_contiguous_float32_bits(how):
    """image and sky as permuted views of [H,W,C] storage, alpha as [H,W], float64 inputs: the contiguous float32 call's bits, and the
    gradients in the caller's shape and dtype."""
    case = ilc.edge_case(ilc.G_LOSS_CASE)
    want = _operator(case, -2.5)
    image, gt, sky, alpha = _on_device(case)
    if how == "permuted_views":
        image, sky = (t.permute(1, 2, 0).contiguous().permute(2, 0, 1) for t in (image, sky))
        assert not image.is_contiguous() and not sky.is_contiguous()
    elif how == "alpha_hw":
        alpha = alpha[0].clone()
    else:
        image, gt, sky, alpha = (t.double() for t in (image, gt, sky, alpha))
    got = _operator(case, -2.5, inputs=[image, gt, sky, alpha])
    for k, (a, b, src) in enumerate(zip(got, want, [None, None, None, image, sky, alpha])):
        if src is not None:
            assert a.shape == src.shape and a.dtype == src.dtype, (how, k, a.shape, a.dtype)
        assert _same_bits(a.float().reshape(b.shape), b), (how, k)
        if how == "float64" and src is not None:
            assert torch.equal(a, b.double()), (how, k)


@pytest.mark.parametrize("name", WALK)
def test_two_runs_of_the_tile_walk_give_the_same_bits(name):
    case = ilc.edge_case(name)
    a, b = _operator(case), _operator(case)
    for k, (p, q) in enumerate(zip(a, b)):
        assert _same_bits(p, q), (name, k)


def test_cuda_entry_points_refuse_bad_shapes():
    image = torch.rand(3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="sky and alpha"):
        photometric_loss(image, image, 0.2, sky=image)
    with pytest.raises(ValueError, match=r"\[C,H,W\]"):
        photometric_loss(image, image[:, :4], 0.2)
    with pytest.raises(_lib.SurfelRasterError, match="workspace"):
        image_loss_forward(image, image, 0.2, workspace=torch.empty(16, dtype=torch.uint8, device=DEV))


def test_rasterizer_gradients_through_the_fused_loss():
    """Behind the real operator: d loss / d (Gaussian parameters) through photometric_loss against the same through photometric_loss_torch
    on the GPU.  The rasterizer's backward is linear in the image gradient it is handed; the two image gradients agree within the bar
    (<= 4 x ~1e-5 of their maximum), and each parameter gradient sums thousands of pixel terms with float atomics in an order of its own,
    so two runs of ONE path already differ in the last bits: 1e-3 of the largest entry (a fifth of smoke()'s 5e-3 for the operator
    against its oracle) separates that from a wrong or dropped term, which shows at 1e-2 or more."""
    W, H, P = 160, 96, 4000
    cam = synthetic_camera(W, H, index=3)
    g = synthetic_gaussians(P, W, H, seed=7, scale_lo=2e-3, scale_hi=3e-2)
    settings = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.tensor([0.1, 0.2, 0.3], device=DEV), 1.0,
                                             cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), 3, cam.camera_center.to(DEV),
                                             False, False)
    r = torch.Generator().manual_seed(11)
    sky = torch.rand(3, H, W, generator=r).to(DEV).requires_grad_()
    noise = 0.1 * torch.randn(3, H, W, generator=r).to(DEV)
    names = ("means3D", "opacities", "scales", "rotations", "shs")

    def grads(loss_fn):
        t = {k: g[k].to(DEV).requires_grad_() for k in names}
        means2D = torch.zeros(P, 3, device=DEV, requires_grad=True)
        color, radii, allmap = GaussianRasterizer(settings)(means3D=t["means3D"], means2D=means2D, shs=t["shs"], opacities=t["opacities"],
                                                            scales=t["scales"], rotations=t["rotations"])
        gt = (color.detach() + noise).clamp(0, 1)
        loss = loss_fn(color, gt, 0.2, sky, allmap[1:2])[0]           # allmap[1] = rend_alpha
        return float(loss.detach()), torch.autograd.grad(loss, [t[k] for k in names] + [means2D, sky])

    loss_hip, g_hip = grads(photometric_loss)
    loss_torch, g_torch = grads(photometric_loss_torch)
    assert abs(loss_hip - loss_torch) <= 1e-5 * abs(loss_torch)
    for name, a, b in zip(names + ("means2D", "sky"), g_hip, g_torch):
        assert torch.isfinite(a).all() and float(b.abs().max()) > 0, name
        e = float((a - b).abs().max() / b.abs().max())
        print(f"{name}: {e:.2e}")
        assert e < 1e-3, (name, e)

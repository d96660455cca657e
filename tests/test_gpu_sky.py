"""-m gpu: the fused sky operator (csrc/sky.hip) and SkyModel.render_with_camera against the float64 twin, to the bar of sky_cases.py."""
import numpy as np
import pytest
import torch

import sky_cases as sc
from streetunveiler_amd import sky
from streetunveiler_amd.image_loss import photometric_loss, photometric_loss_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c["name"] for c in sc.CASES]


def _case(name):
    return next(c for c in sc.CASES if c["name"] == name)


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_model_is_inside_the_bar(case):
    truth, yard = sc.reference(case)
    sc.assert_within_bar(sc.run_model(case, DEV), truth, yard, "model " + case["name"])


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_raw_pair_is_inside_the_bar(case):
    truth, yard = sc.reference(case)
    sc.assert_within_bar(sc.run_raw(case, DEV), sc.fused_view(truth), sc.fused_view(yard), "raw " + case["name"])


def test_same_bits_twice_and_workgroup_counts_within_the_bar():
    case = _case("shape_263x251_wg3")
    a, b = sc.run_raw(case, DEV), sc.run_raw(case, DEV)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    default = sc.run_raw(dict(case, max_workgroups=0), DEV)
    assert all(np.array_equal(default[k], sc.run_raw(dict(case, max_workgroups=0), DEV)[k]) for k in default)
    assert np.array_equal(a["image"], default["image"])              # the forward has no sum across pixels
    truth, yard = sc.reference(case)
    sc.assert_within_bar(default, sc.fused_view(truth), sc.fused_view(yard), "raw, default workgroups")


def test_unwanted_gradients_are_none_and_nothing_else_is_written():
    case = _case("shape_67x129_wg0")
    want = (True, False, False, True, True, False, True, False)
    full, part = sc.run_raw(case, DEV), sc.run_raw(case, DEV, want=want)
    assert set(part) == {"image"} | {k for k, w in zip(sc.WEIGHT_GRADS, want) if w}
    assert all(np.array_equal(part[k], full[k]) for k in part)
    # guard bands: every output sits inside a larger buffer filled with a sentinel, which must survive around it
    cam, weights = sc.fused_inputs(case, DEV)
    H, W, GUARD, SENTINEL = case["H"], case["W"], 1024, -7.5
    def guarded(shape):
        n = int(np.prod(shape))
        whole = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
        return whole, whole[GUARD:GUARD + n].view(shape)
    whole_img, img = guarded((3, H, W))
    sky.sky_forward(cam, H, W, *weights, out=img)
    outs = [guarded(shape) for shape in sky.WEIGHT_SHAPES]
    ws = sky.sky_workspace(DEV, 2)
    sky.sky_backward(cam, H, W, *weights, g_out=case["g_out"].to(DEV), max_workgroups=2, workspace=ws, out=tuple(view for _, view in outs))
    torch.cuda.synchronize()
    for whole, view in [(whole_img, img)] + outs:
        assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())
        assert not bool((view == SENTINEL).any())
    through_autograd = sc.run_model(case, DEV)
    assert np.isfinite(through_autograd["g_params"]).all()
    # autograd: an input that needs no gradient gets None
    leaves = [t.clone().requires_grad_(w) for t, w in zip(weights, want)]
    image = sky.sky_rays_mlp(cam, H, W, *leaves)
    grads = torch.autograd.grad(image.sum(), [t for t, w in zip(leaves, want) if w])
    assert len(grads) == sum(want) and all(g is not None for g in grads)


def test_empty_image():
    """H * W == 0 is no error and no work: the raw forward, the raw backward (which writes nothing) and the autograd path (zeros)."""
    cam, weights = sc.fused_inputs(_case("shape_5x7_wg0"), DEV)
    assert sky.sky_forward(cam, 0, 7, *weights).shape == (3, 0, 7)
    sentinel = tuple(torch.full(shape, -7.5, device=DEV) for shape in sky.WEIGHT_SHAPES)
    sky.sky_backward(cam, 0, 7, *weights, g_out=torch.empty(3, 0, 7, device=DEV), out=sentinel)
    torch.cuda.synchronize()
    assert all(bool((t == -7.5).all()) for t in sentinel)
    leaves = [t.clone().requires_grad_() for t in weights]
    image = sky.sky_rays_mlp(cam, 7, 0, *leaves)
    assert image.shape == (3, 7, 0)
    grads = torch.autograd.grad(image.sum(), leaves)
    assert all(g.shape == t.shape and not bool(g.any()) for g, t in zip(grads, leaves))


def test_side_stream_and_graph_replay():
    case = _case("shape_67x129_wg0")
    H, W = case["H"], case["W"]
    want = sc.run_raw(case, DEV)
    cam, weights = sc.fused_inputs(case, DEV)
    g_out = case["g_out"].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        image = sky.sky_forward(cam, H, W, *weights)
        grads = sky.sky_backward(cam, H, W, *weights, g_out=g_out)
    side.synchronize()
    assert np.array_equal(image.double().cpu().numpy(), want["image"])
    assert all(np.array_equal(g.double().cpu().numpy(), want[k]) for k, g in zip(sc.WEIGHT_GRADS, grads))
    # capture the raw pair on static buffers, replay on changed inputs
    other = _case("fx_ne_fy")
    other = dict(other, H=H, W=W, g_out=torch.randn(3, H, W, generator=torch.Generator().manual_seed(5)))
    static_cam, static_w, static_g = cam.clone(), [t.clone() for t in weights], g_out.clone()
    out = torch.empty(3, H, W, device=DEV)
    gbufs = tuple(torch.empty(shape, device=DEV) for shape in sky.WEIGHT_SHAPES)
    ws = sky.sky_workspace(DEV)
    sky.sky_forward(static_cam, H, W, *static_w, out=out)                       # warm-up outside the capture
    sky.sky_backward(static_cam, H, W, *static_w, g_out=static_g, workspace=ws, out=gbufs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sky.sky_forward(static_cam, H, W, *static_w, out=out)
        sky.sky_backward(static_cam, H, W, *static_w, g_out=static_g, workspace=ws, out=gbufs)
    cam2, weights2 = sc.fused_inputs(other, DEV)
    static_cam.copy_(cam2)
    for dst, src in zip(static_w, weights2):
        dst.copy_(src)
    static_g.copy_(other["g_out"].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    want2 = sc.run_raw(other, DEV)
    assert np.array_equal(out.double().cpu().numpy(), want2["image"])
    assert all(np.array_equal(g.double().cpu().numpy(), want2[k]) for k, g in zip(sc.WEIGHT_GRADS, gbufs))


def test_composite_path_gives_the_twins_gradients():
    case = _case("shape_67x129_wg0")
    H, W = case["H"], case["W"]
    g = torch.Generator().manual_seed(77)
    gt, alpha = torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g)
    render = torch.rand(3, H, W, generator=g) * alpha

    def twin(dtype):
        params, layers = sc.layers_of(case["state"], dtype, "cpu", grad=True)
        image = sky.sky_forward_torch(params, layers, H, W, case["K"], case["c2w"])
        loss = photometric_loss_torch(render.to(dtype), gt.to(dtype), 0.2, image, alpha.to(dtype))[0]
        leaves = [params] + [t for pair in layers for t in pair]
        return {k: v.double().numpy() for k, v in zip(sc.MODEL_GRADS, torch.autograd.grad(loss, leaves))}

    model = sky.SkyModel(device=DEV)
    model.load_state_dict(sc.state_dict_of(case["state"]))
    loss = photometric_loss(render.to(DEV), gt.to(DEV), 0.2, sky=model.render_with_camera(H, W, case["K"], case["c2w"]), alpha=alpha.to(DEV))[0]
    loss.backward()
    leaves = [model.position_encoding.params] + [t for pair in model.blocks.pairs() for t in pair]
    assert all(p.grad is not None for p in leaves)
    got = {k: p.grad.double().cpu().numpy() for k, p in zip(sc.MODEL_GRADS, leaves)}
    sc.assert_within_bar(got, twin(torch.float64), twin(torch.float32), "composite")


def test_fit_follows_the_twin():
    """30 Adam steps on a 48x64 vertical colour gradient, fused against the float32 twin on the CPU from the same state.  The loss falls;
    the curves agree to 1e-3 of the loss.  That bound is this file's own (tests/test_gpu_fit.py asserts a falling loss and has no bound
    between two curves to inherit), argued as follows: Adam's first steps move every parameter by ~lr = 1e-4 whatever its gradient's size, so a
    gradient element whose sign differs between two float32 evaluations (only one near zero can) moves its parameter 2e-4 apart per
    step -- far below 1e-3 of a loss of order 0.1 after 30 steps, while a wrong gradient term changes the curve by percents."""
    H, W, steps = 48, 64, 30
    K, c2w = sc.camera(H, W, seed=40)
    ramp = torch.linspace(0, 1, H)[None, :, None].expand(3, H, W)
    target = torch.stack([0.2 + 0.6 * ramp[0], 0.5 * ramp[1], 1.0 - 0.7 * ramp[2]])
    state = sc.state_dict_of(sc.make_state(3))
    curves = []
    for dev in (DEV, "cpu"):
        model = sky.SkyModel(device=dev)
        model.load_state_dict(state)
        tgt, losses = target.to(dev), []
        for _ in range(steps):
            if dev == "cpu":
                image = sky.sky_forward_torch(model.position_encoding.params, model.blocks.pairs(), H, W, K, c2w)
            else:
                image = model.render_with_camera(H, W, K, c2w)
            loss = (image - tgt).abs().mean()
            model.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            model.optimizer.step()
            losses.append(float(loss.detach()))
        curves.append(np.array(losses))
    fused, twin = curves
    assert fused[-1] < fused[0] and np.isfinite(fused).all(), fused
    assert np.abs(fused - twin).max() <= 1e-3 * twin.max(), (fused, twin)

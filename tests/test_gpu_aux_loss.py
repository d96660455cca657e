"""-m gpu: the fused auxiliary losses (csrc/aux_loss.hip) under the bar of tests/aux_loss_cases.py -- every case, forward and backward,
through the differentiable operators and through the raw calls; run-to-run bit identity; unwanted gradients; a side stream; the three
forward / backward pairs inside one HIP graph; and a training step's parameter gradients through them."""
import numpy as np
import pytest
import torch

from streetunveiler_amd import _lib
from streetunveiler_amd import aux_loss as al
from tests import aux_loss_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ids = lambda cases: [c["name"] for c in cases]
by_name = lambda cases, name: next(c for c in cases if c["name"] == name)


@pytest.mark.parametrize("case", ac.SEMANTIC, ids=ids(ac.SEMANTIC))
def test_semantic_cross_entropy_within_the_bar(case):
    truth, yard = ac.semantic_reference(case)
    got = ac.run_hip_semantic(case, DEV)
    ac.assert_within_bar(got, truth, yard, case["name"])
    if case["kind"] == ac.NEG_INF_LABEL:                           # deliberate difference 1: finite where torch's one-hot product is NaN
        assert np.isfinite(got["loss"]) and np.isfinite(got["g_logits"]).all()
    if case["name"] == "neg_inf_soft" or case["name"].startswith("nan_"):
        assert np.isnan(got["loss"])                               # the probability form does what torch does; a NaN logit is never lost
    if case["name"] == "all_out_of_range":
        assert float(got["loss"]) == 0.0 and not got["g_logits"].any()


@pytest.mark.parametrize("case", ac.SURFACE, ids=ids(ac.SURFACE))
def test_surface_regularisers_within_the_bar(case):
    truth, yard = ac.surface_reference(case)
    ac.assert_within_bar(ac.run_hip_surface(case, DEV), truth, yard, case["name"])


@pytest.mark.parametrize("case", ac.SHRINK, ids=ids(ac.SHRINK))
def test_opacity_shrink_within_the_bar(case):
    truth, yard = ac.shrink_reference(case)
    got = ac.run_hip_shrink(case, DEV)
    ac.assert_within_bar(got, truth, yard, case["name"])
    assert np.isfinite(got["g_opacity"]).all()
    if case["name"] == "saturated":
        assert not got["g_opacity"][case["opacity"].numpy() == 100.0].any()      # 1 - s == 0: the gradient is 0, not NaN


RAW = [(ac.SEMANTIC, ac.semantic_reference, ac.run_hip_semantic, n) for n in ("unit_263x251", "out_of_range_u8", "pm1e4_i32", "eight_classes_soft")] + \
      [(ac.SURFACE, ac.surface_reference, ac.run_hip_surface, n) for n in ("maps_263x251", "border_zeros")] + \
      [(ac.SHRINK, ac.shrink_reference, ac.run_hip_shrink, n) for n in ("raw_65537", "saturated", "activated_65")]


@pytest.mark.parametrize("cases,reference,run,name", RAW, ids=[r[3] for r in RAW])
def test_raw_calls_within_the_bar(cases, reference, run, name):
    """The C-ABI pairs themselves (no autograd.Function between the test and the library)."""
    case = by_name(cases, name)
    truth, yard = reference(case)
    ac.assert_within_bar(run(case, DEV, raw=True), truth, yard, "raw " + name)


def test_two_calls_give_the_same_bits():
    """Fixed-order sums, one writer per element: no float atomics anywhere."""
    for cases, run, name in ((ac.SEMANTIC, ac.run_hip_semantic, "unit_263x251"), (ac.SEMANTIC, ac.run_hip_semantic, "soft_big"),
                             (ac.SURFACE, ac.run_hip_surface, "maps_263x251"), (ac.SHRINK, ac.run_hip_shrink, "raw_65537")):
        a, b = run(by_name(cases, name), DEV), run(by_name(cases, name), DEV)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


WANTS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True) if a or b or c]


@pytest.mark.parametrize("want", WANTS, ids=["".join("ynd"[i] if w else "-" for i, w in enumerate(want)) for want in WANTS])
def test_only_the_wanted_gradients_are_computed(want):
    """Every subset of (rend_normal, surf_normal, rend_dist) that needs a gradient: the others come back None (run_hip_surface asserts
    it), the wanted ones pass the bar, through autograd and through the raw call."""
    case = by_name(ac.SURFACE, "border_zeros")
    truth, yard = ac.surface_reference(case)
    for raw in (False, True):
        got = ac.run_hip_surface(case, DEV, raw=raw, want=want)
        assert set(got) == {"loss", "normal_loss", "dist_loss"} | {k for k, w in zip(ac.SURFACE_GRADS, want) if w}
        ac.assert_within_bar(got, {k: truth[k] for k in got}, {k: yard[k] for k in got}, f"want={want} raw={raw}")


def test_nothing_is_written_beside_the_wanted_gradients():
    """The raw backward with g_surf_normal not wanted: the two wanted gradients sit in one buffer between guard bands, which stay as
    they were -- so does every input."""
    case = by_name(ac.SURFACE, "maps_130x70")
    maps = [case[k].to(DEV) for k in ("rend_normal", "surf_normal", "rend_dist")]
    kept = [m.clone() for m in maps]
    n, guard = maps[2].numel(), 4096
    buf = torch.full((guard + 3 * n + guard + n + guard,), -7.0, device=DEV)
    g_rn, g_rd = buf[guard:guard + 3 * n].view(3, *maps[0].shape[1:]), buf[2 * guard + 3 * n:2 * guard + 4 * n].view(maps[2].shape)
    out = al.surface_reg_backward(*maps, 0.05, 100.0, torch.tensor(ac.UPSTREAM, device=DEV), out=(g_rn, None, g_rd))
    torch.cuda.synchronize()
    assert out[1] is None
    for lo, hi in ((0, guard), (guard + 3 * n, 2 * guard + 3 * n), (2 * guard + 4 * n, buf.numel())):
        assert bool((buf[lo:hi] == -7.0).all()), (lo, hi)
    truth, yard = ac.surface_reference(case)
    got = dict(g_rend_normal=g_rn.cpu().numpy(), g_rend_dist=g_rd.cpu().numpy())
    ac.assert_within_bar(got, {k: truth[k] for k in got}, {k: yard[k] for k in got}, "guarded")
    assert all(torch.equal(a, b) for a, b in zip(maps, kept))


def test_semantic_target_and_weight_get_no_gradient_and_dtypes_come_back():
    case = by_name(ac.SEMANTIC, "soft_unnormalised")
    x = case["x"].to(DEV).double().requires_grad_()                         # another float dtype and a strided view are converted
    t = case["target"].to(DEV).requires_grad_()
    strided = x.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not strided.is_contiguous()
    loss = al.semantic_cross_entropy(strided, t, torch.tensor(case["weight"], device=DEV))
    g_x, g_t = torch.autograd.grad(loss, [x, t], torch.tensor(ac.UPSTREAM, device=DEV), allow_unused=True)
    assert g_t is None and g_x.dtype == torch.float64 and g_x.shape == x.shape and loss.dim() == 0 and loss.dtype == torch.float32
    truth, yard = ac.semantic_reference(case)
    ac.assert_within_bar(dict(loss=loss.detach().cpu().numpy(), g_logits=g_x.cpu().numpy()), truth, yard, "float64 leaves")
    o = by_name(ac.SHRINK, "raw_65")["opacity"].to(DEV).half().requires_grad_()
    al.opacity_shrink(o).backward()
    assert o.grad.dtype == torch.float16 and o.grad.shape == o.shape


def test_python_entry_points_refuse_bad_shapes():
    x, lab = torch.rand(6, 8, 9, device=DEV), torch.zeros(8, 9, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="logits"):
        al.semantic_cross_entropy(torch.rand(9, 8, 9, device=DEV), lab)
    with pytest.raises(ValueError, match="logits"):
        al.semantic_cross_entropy(x[0], lab)
    with pytest.raises(ValueError, match="integer target"):
        al.semantic_cross_entropy(x, lab[:4])
    with pytest.raises(ValueError, match="float target"):
        al.semantic_cross_entropy(x, torch.rand(5, 8, 9, device=DEV))
    with pytest.raises(ValueError, match="weight"):
        al.semantic_cross_entropy(x, lab, [1.0, 2.0])
    with pytest.raises(ValueError, match="rend_normal and surf_normal"):
        al.surface_regularisers(x[:3], x[:2], x[:1], 0.05, 100.0)
    with pytest.raises(ValueError, match="rend_dist"):
        al.surface_regularisers(x[:3], x[3:], x[:2], 0.05, 100.0)
    with pytest.raises(ValueError, match="opacity"):
        al.opacity_shrink(torch.empty(0, 1, device=DEV))
    with pytest.raises(_lib.SurfelRasterError, match="workspace"):
        al.semantic_ce_forward(x, lab, workspace=torch.empty(8, dtype=torch.uint8, device=DEV))


def _three_pairs(case_s, case_r, case_o):
    """The raw forward / backward pairs of the three ops on preallocated buffers -> (the call, its outputs)."""
    x, t = case_s["x"].to(DEV), case_s["target"].to(DEV)
    maps = [case_r[k].to(DEV) for k in ("rend_normal", "surf_normal", "rend_dist")]
    o = case_o["opacity"].to(DEV)
    g = torch.tensor(ac.UPSTREAM, device=DEV)
    ws = [al.aux_loss_workspace(n, DEV) for n in (t.numel(), maps[2].numel(), o.numel())]
    out = [torch.empty(1, device=DEV), torch.empty(3, device=DEV), torch.empty(1, device=DEV)]
    grads = [torch.empty_like(x), tuple(torch.empty_like(m) for m in maps), torch.empty_like(o)]

    def run():
        al.semantic_ce_forward(x, t, case_s["weight"], workspace=ws[0], out=out[0])
        al.semantic_ce_backward(x, t, g, case_s["weight"], out=grads[0])
        al.surface_reg_forward(*maps, case_r["lambda_normal"], case_r["lambda_dist"], workspace=ws[1], out=out[1])
        al.surface_reg_backward(*maps, case_r["lambda_normal"], case_r["lambda_dist"], g, out=grads[1])
        al.opacity_shrink_forward(o, False, workspace=ws[2], out=out[2])
        al.opacity_shrink_backward(o, g, False, out=grads[2])

    return run, out + [grads[0]] + list(grads[1]) + [grads[2]], ws, g


def test_ops_work_on_a_side_stream():
    run, outs, ws, _ = _three_pairs(by_name(ac.SEMANTIC, "unit_263x251"), by_name(ac.SURFACE, "maps_263x251"), by_name(ac.SHRINK, "raw_65537"))
    run()
    torch.cuda.synchronize()
    ref = [t.clone() for t in outs]
    for t in outs + ws:
        t.fill_(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    side.synchronize()                                                       # the side stream alone: the work was queued THERE
    for k, (a, b) in enumerate(zip(ref, outs)):
        assert torch.equal(a, b), f"output {k} differs on the side stream"


def test_three_pairs_capture_into_one_hip_graph():
    """No host read-back, no allocation by the library, the class weights inside the launch: the six raw calls are captured into ONE HIP
    graph (side-stream warm-up, a linear chain) and every replay returns the eager call's bits; the upstream scalar is read at replay."""
    run, outs, ws, g = _three_pairs(by_name(ac.SEMANTIC, "out_of_range_i32"), by_name(ac.SURFACE, "maps_130x70"), by_name(ac.SHRINK, "raw_65"))
    run()
    torch.cuda.synchronize()
    ref = [t.clone() for t in outs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(3):
        for t in outs:
            t.fill_(float("nan"))
        for w in ws:
            w.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(ref, outs)):
            assert torch.equal(a, b), f"graph replay: output {k} differs from the eager call"
    g.fill_(2 * ac.UPSTREAM)                                                 # a power of two times g: every gradient doubles exactly
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(ref, outs)):
        assert torch.equal(a if k < 3 else 2 * a, b), f"graph replay with another g: output {k}"


def test_training_step_parameter_gradients():
    """A step shaped like the reference's train.py:84-146 -- render_train_view, semantic cross-entropy on the label map, the image loss,
    the two regularisers, the opacity shrink, one backward -- three times: with the fused ops, with their `*_torch` twins in float32, and
    with the twins evaluated in float64 on the same float32 maps (the truth of the loss part).  photometric_loss and the rasterizer are
    the same HIP code in all three.
    The bar is the one of tests/aux_loss_cases.py, per ELEMENT of every parameter gradient: |fused - truth| <= 2 x |float32 twins -
    truth|, floor half a float32 ulp of the element's true value.  The rasterizer's backward has no float atomics and is bit-identical
    from run to run, so the three steps differ only by what the loss part hands it.  The weights of the terms (1/2, 2^-7) are exact in
    float32: the float32 steps hand each op the same upstream scalar as the float64 step."""
    import math
    from streetunveiler_amd.gaussian_renderer import PipelineParams, SurfelModel, render_train_view
    from streetunveiler_amd.image_loss import photometric_loss
    from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians
    W, H, P = 67, 45, 3000
    cam = synthetic_camera(W, H, index=3).to(DEV)
    g = synthetic_gaussians(P, W, H, seed=9, scale_lo=4e-3, scale_hi=5e-2)
    r = torch.Generator().manual_seed(13)
    sem = torch.randint(0, 6, (P,), generator=r).to(DEV)
    labels = torch.randint(0, 8, (H, W), generator=r).to(torch.uint8).to(DEV)       # 6, 7: pixels the reference has no channel for
    gt = torch.rand(3, H, W, generator=r).to(DEV)
    raw = dict(xyz=g["means3D"], scaling=torch.log(g["scales"]), rotation=g["rotations"],
               opacity=torch.logit(g["opacities"].clamp(1e-3, 1 - 1e-3)), features=g["shs"])
    names = tuple(raw)
    pipe, bg = PipelineParams(), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    weight, sem_ratio, ln, ld, shrink = ac.REF_WEIGHT, 0.5, 0.05, 100.0, 2.0 ** -7

    def step(kind):
        t = {k: v.float().to(DEV).requires_grad_() for k, v in raw.items()}
        pc = SurfelModel(t["xyz"], t["scaling"], t["rotation"], t["opacity"], t["features"], sem, 3, 3, raw=True)
        pkg = render_train_view(cam, pc, pipe, bg)
        up = (lambda m: m.double()) if kind == "torch64" else (lambda m: m)
        maps = [up(pkg[k]) for k in ("render_semantics", "rend_normal", "surf_normal", "rend_dist")]
        image = photometric_loss(pkg["render"], gt, 0.2)[0]
        if kind == "hip":
            loss = sem_ratio * al.semantic_cross_entropy(maps[0], labels, weight) + image + \
                al.surface_regularisers(maps[1], maps[2], maps[3], ln, ld)[0] + shrink * al.opacity_shrink(t["opacity"])
        else:
            loss = sem_ratio * al.semantic_cross_entropy_torch(maps[0], labels, weight) + image + \
                al.surface_regularisers_torch(maps[1], maps[2], maps[3], ln, ld)[0] + shrink * al.opacity_shrink_torch(up(t["opacity"]))
        loss.backward()
        assert math.isfinite(float(loss.detach()))
        return [t[k].grad.double().cpu().numpy() for k in names]

    truth, yard, got = (dict(zip(names, step(kind))) for kind in ("torch64", "torch32", "hip"))
    for name in names:
        assert np.abs(truth[name]).max() > 0, name
    ac.assert_within_bar(got, truth, yard, "training step")

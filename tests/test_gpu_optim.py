"""-m gpu: the fused Adam step and the densification statistics (csrc/optimizer.hip) -- every path of the kernel against the float64
checker under the one-step rounding bound of tests/optim_cases.py, run-to-run bit identity, the 50-step accuracy bar (4 x the deviation of
torch's own float32 Adam on the same GPU), the drop-in contract with the reference's tensor surgery, the statistics, and both inside the
optimisation loop of tests/test_gpu_fit.py."""
import copy
import math

import pytest
import torch

from streetunveiler_amd.gaussian_renderer import PipelineParams, SurfelModel, render
from streetunveiler_amd.optim import (ADAM_CHUNK, ADAM_MAX_SEGMENTS, SurfelAdam, adam_step, densification_stats,
                                      densification_stats_torch)
from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians
from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B1, B2 = oc.BETAS


def _offset_view(t, offset):
    """A contiguous view of `t`'s values that starts `offset` elements into a fresh storage on the GPU."""
    flat = torch.empty(t.numel() + offset, device=DEV)
    flat[offset:] = t.reshape(-1).to(DEV)
    return flat[offset:].view(t.shape)


def _run_raw(state, grads, lrs, steps, eps=oc.EPS, offset=0):
    """adam_step on GPU copies of the CPU tensors -> [(p, m, v)] after the step (on the GPU)."""
    dev = [[_offset_view(t, offset) for t in pmv] for pmv in state]
    g = [_offset_view(t, offset) for t in grads]
    adam_step([d[0] for d in dev], g, [d[1] for d in dev], [d[2] for d in dev], lrs, steps, B1, B2, eps)
    torch.cuda.synchronize()
    return dev


def _check_raw(state, grads, lrs, steps, what, eps=oc.EPS, offset=0):
    """One step, twice from equal inputs: equal bits, and every tensor within the one-step bound of the float64 checker."""
    first, second = (_run_raw(state, grads, lrs, steps, eps, offset) for _ in range(2))
    for k, ((p0, m0, v0), g) in enumerate(zip(state, grads)):
        for a, b in zip(first[k], second[k]):
            assert torch.equal(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())), f"{what}[{k}]: two runs differ"
        oc.assert_one_step_within_bounds(first[k], (p0, g, m0, v0), lrs[k], steps[k], f"{what}[{k}]", eps=eps)
    return first


EDGE_SIZES = (1, 3, 4, 5, ADAM_CHUNK - 1, ADAM_CHUNK, ADAM_CHUNK + 1, 3 * ADAM_CHUNK + 2)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_kernel_edges(n):
    """One tensor of n elements: below a group of four, the n mod 4 tail, one short of / exactly / one past a chunk, several chunks."""
    state = oc.seeded_state([(n,)], seed=n)
    _check_raw(state, [oc.seeded_gradient((n,), n)], [0.01], [3], f"n={n}")


def test_every_edge_size_in_one_unaligned_call():
    """The same sizes together (8 tensors: one launch), every pointer one element into its storage: the scalar path."""
    state = oc.seeded_state([(n,) for n in EDGE_SIZES], seed=1)
    grads = [oc.seeded_gradient((n,), 50 + n) for n in EDGE_SIZES]
    assert len(state) == ADAM_MAX_SEGMENTS
    out = _check_raw(state, grads, [0.01 * (k + 1) for k in range(8)], [k + 1 for k in range(8)], "unaligned", offset=1)
    assert all(t.data_ptr() % 16 == 4 for pmv in out for t in pmv)


@pytest.mark.parametrize("P", [1, 1037])
def test_reference_shapes_in_one_call(P):
    """[P,3], [P,1,3], [P,15,3], [P,1], [P,2], [P,4]: a learning rate and a step count per tensor."""
    shapes = oc.reference_shapes(P)
    state = oc.seeded_state(shapes, seed=P)
    grads = [oc.seeded_gradient(s, 7 + k) for k, s in enumerate(shapes)]
    _check_raw(state, grads, [lr for _, _, lr in oc.GROUPS], [1, 2, 30, 4, 500, 6], f"P={P}")


def test_nine_tensors_take_two_launches():
    shapes = [(ADAM_CHUNK + 3 * k + 1,) for k in range(9)]
    state = oc.seeded_state(shapes, seed=9)
    grads = [oc.seeded_gradient(s, 90 + k) for k, s in enumerate(shapes)]
    _check_raw(state, grads, [0.002 * (k + 1) for k in range(9)], [k + 1 for k in range(9)], "nine")


def test_one_unaligned_tensor_beside_aligned_ones():
    """Param, grad, m and v of the middle tensor are views starting one element into their storage; its neighbours are 16-B aligned."""
    shapes = [(ADAM_CHUNK + 7,), (2 * ADAM_CHUNK + 5,), (1037, 3)]
    state = oc.seeded_state(shapes, seed=21)
    grads = [oc.seeded_gradient(s, 210 + k) for k, s in enumerate(shapes)]
    lrs, steps = [0.01, 0.02, 0.03], [2, 3, 4]
    dev = [[_offset_view(t, 1 if k == 1 else 0) for t in pmv] for k, pmv in enumerate(state)]
    g = [_offset_view(t, 1 if k == 1 else 0) for k, t in enumerate(grads)]
    assert dev[1][0].data_ptr() % 16 == 4 and g[1].data_ptr() % 16 == 4 and dev[0][0].data_ptr() % 16 == 0
    adam_step([d[0] for d in dev], g, [d[1] for d in dev], [d[2] for d in dev], lrs, steps, B1, B2, oc.EPS)
    for k, ((p0, m0, v0), gk) in enumerate(zip(state, grads)):
        oc.assert_one_step_within_bounds(dev[k], (p0, gk, m0, v0), lrs[k], steps[k], f"mixed[{k}]")


def test_a_noncontiguous_gradient_is_made_contiguous_and_noncontiguous_state_is_refused():
    (p0, m0, v0), = oc.seeded_state([(300, 3)], seed=3)
    g = oc.seeded_gradient((3, 300), 31)
    dev = [t.to(DEV) for t in (p0, m0, v0)]
    adam_step([dev[0]], [g.to(DEV).t()], [dev[1]], [dev[2]], [0.01], [1], B1, B2, oc.EPS)
    oc.assert_one_step_within_bounds(dev, (p0, g.t(), m0, v0), 0.01, 1, "transposed gradient")
    with pytest.raises(ValueError, match="not contiguous"):
        adam_step([dev[0]], [dev[0]], [torch.zeros(3, 300, device=DEV).t()], [dev[2]], [0.01], [1], B1, B2, oc.EPS)


def test_parameter_without_gradient_keeps_its_state():
    tensors = [p for p, _, _ in oc.seeded_state(oc.reference_shapes(65), seed=5)]
    opt, params = oc.make_optimizer(SurfelAdam, tensors, DEV, torch.float32)
    grads = {name: oc.seeded_gradient((65,) + tail, k) for k, (name, tail, _) in enumerate(oc.GROUPS)}
    oc.set_grads(opt, grads)
    opt.step()
    before = {k: v.clone() for k, v in opt.state[params["scaling"]].items()}
    p_before = params["scaling"].detach().clone()
    oc.set_grads(opt, dict(grads, scaling=None))
    opt.step()
    after = opt.state[params["scaling"]]
    assert torch.equal(params["scaling"].detach(), p_before) and all(torch.equal(before[k], after[k]) for k in before)
    assert float(after["step"]) == 1 and float(opt.state[params["xyz"]]["step"]) == 2
    assert after["step"].device.type == "cpu" and after["step"].dtype == torch.float32
    fresh = SurfelAdam([torch.nn.Parameter(torch.zeros(4, 3, device=DEV))])
    fresh.step()                                                       # no gradient anywhere: no state, no launch
    assert len(fresh.state) == 0


def test_zero_learning_rate_leaves_the_parameter_bits():
    state = oc.seeded_state([(ADAM_CHUNK + 5,)], seed=6)
    grads = [oc.seeded_gradient((ADAM_CHUNK + 5,), 61)]
    (p, m, v), = _check_raw(state, grads, [0.0], [4], "lr=0")
    assert torch.equal(p.cpu(), state[0][0]) and not torch.equal(m.cpu(), state[0][1]) and not torch.equal(v.cpu(), state[0][2])


def test_zero_gradient_decays_the_moments():
    n = ADAM_CHUNK + 5
    state = oc.seeded_state([(n,)], seed=8)
    (p, m, v), = _check_raw(state, [torch.zeros(n)], [0.01], [10], "g=0")
    m0, v0 = state[0][1], state[0][2]
    assert bool((m.cpu().abs() < m0.abs()).all()) and bool((v.cpu() < v0).all()) and not torch.equal(p.cpu(), state[0][0])


def test_zero_gradient_on_zero_state_with_tiny_eps():
    n = ADAM_CHUNK + 5
    state = oc.seeded_state([(n,)], seed=10, moments=False)
    (p, m, v), = _check_raw(state, [torch.zeros(n)], [0.01], [1], "0/eps", eps=1e-15)
    assert torch.equal(p.cpu(), state[0][0]) and not m.any() and not v.any()
    assert all(bool(torch.isfinite(t).all()) for t in (p, m, v))


def test_nan_and_inf_gradients_stay_in_their_elements():
    n = 64
    state = oc.seeded_state([(n,)], seed=12)
    g = oc.seeded_gradient((n,), 121)
    g[9], g[10] = float("nan"), float("inf")             # elements 1 and 2 of the aligned group 8..11
    (p, m, v), = _check_raw(state, [g], [0.01], [2], "nan/inf")
    bad = torch.zeros(n, dtype=torch.bool); bad[9] = bad[10] = True
    for t in (p, m, v):
        assert torch.equal(~torch.isfinite(t.cpu()), bad)


def test_accuracy_bar_over_50_steps():
    """Gradients spanning 1e-6 .. 1e1, a seventh of them zero, the reference's six groups at P = 1037, 50 steps: per quantity, the largest
    deviation of SurfelAdam from the float64 checker is at most 4 x that of torch.optim.Adam(foreach=False) in float32 on this GPU."""
    d_hip, d_ref, r = oc.accuracy_run(DEV)
    print("SurfelAdam", d_hip, "torch float32", d_ref, "ratios", r)
    assert all(d > 0 for d in d_ref.values()), d_ref
    assert all(v <= oc.BAR for v in r.values()), f"beyond {oc.BAR} x torch's own float32 deviation: {r} (SurfelAdam {d_hip}, torch {d_ref})"


def test_drop_in_contract_with_the_references_tensor_surgery():
    """3 steps, the reference's prune / concatenate / replace patterns on `optimizer.state` and `param_groups`, 3 more steps -- on
    SurfelAdam, on torch's float32 Adam and on the float64 truth alike: the same bar, the same step counts, the same shapes."""
    P_of = lambda o: o.param_groups[0]["params"][0].shape[0]
    hip, ref, truth = oc.three_optimizers(1037, DEV, seed=2)
    opts = [hip, ref, truth]
    oc.run_steps(opts, P_of, 1, 3, seed=5)
    for opt in opts:
        oc.surgery(opt, seed=2)
    assert P_of(hip) == P_of(ref) == P_of(truth) and P_of(hip) != 1037
    oc.run_steps(opts, P_of, 4, 3, seed=5)
    d_hip, d_ref = oc.deviations(hip, truth), oc.deviations(ref, truth)
    r = oc.ratios(d_hip, d_ref)
    print("SurfelAdam", d_hip, "torch float32", d_ref, "ratios", r)
    assert all(v <= oc.BAR for v in r.values()), f"beyond {oc.BAR} x torch's own float32 deviation: {r}"
    for name, p in oc.named_params(hip).items():
        s, s_ref = hip.state[p], ref.state[oc.named_params(ref)[name]]
        assert float(s["step"]) == float(s_ref["step"]) == 6.0 and s["step"].device.type == "cpu" and s["step"].dtype == s_ref["step"].dtype
        assert s.keys() == s_ref.keys() and s["exp_avg"].shape == p.shape == s["exp_avg_sq"].shape


def test_state_dict_round_trips_into_both_optimizers():
    P = 65
    hip = oc.three_optimizers(P, DEV, seed=3)[0]
    oc.run_steps([hip], lambda o: P, 1, 2)
    sd = hip.state_dict()
    tensors = [p.detach().cpu() for p in oc.named_params(hip).values()]
    again = oc.make_optimizer(SurfelAdam, tensors, DEV, torch.float32)[0]
    theirs = oc.make_optimizer(torch.optim.Adam, tensors, DEV, torch.float32, foreach=False)[0]
    for other in (again, theirs):
        other.load_state_dict(copy.deepcopy(sd))          # (a copy each, as from a checkpoint on disk: load_state_dict keeps the tensors it is handed)
        for name, p in oc.named_params(other).items():
            s, s0 = other.state[p], hip.state[oc.named_params(hip)[name]]
            assert float(s["step"]) == 2.0 and s["step"].device.type == "cpu"
            assert torch.equal(s["exp_avg"], s0["exp_avg"]) and torch.equal(s["exp_avg_sq"], s0["exp_avg_sq"])
        assert [{k: v for k, v in g.items() if k != "params"} for g in other.param_groups] == [{k: v for k, v in g.items() if k != "params"} for g in hip.param_groups]
    oc.run_steps([hip, again, theirs], lambda o: P, 3, 1)
    for name, p in oc.named_params(hip).items():
        assert torch.equal(p, oc.named_params(again)[name]), name                      # the same kernel on the same bits
        q = oc.named_params(theirs)[name]
        assert float(theirs.state[q]["step"]) == 3.0 and bool(torch.isfinite(q).all()) and not torch.equal(q.detach().cpu(), tensors[list(oc.named_params(hip)).index(name)])
    back = oc.make_optimizer(SurfelAdam, tensors, DEV, torch.float32)[0]
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))                                           # ... and from torch's Adam into SurfelAdam
    oc.run_steps([theirs, back], lambda o: P, 4, 1)
    assert all(float(back.state[p]["step"]) == 4.0 for p in oc.named_params(back).values())


@pytest.mark.parametrize("visible", ["none", "all", "third"])
@pytest.mark.parametrize("P", [1, 64, 65, 1037])
def test_densification_statistics(P, visible):
    grad, radii, accum, denom, max_radii = oc.stats_case(P, visible)
    ref = [t.to(DEV).clone() for t in (accum, denom, max_radii)]
    densification_stats_torch(grad.to(DEV), radii.to(DEV), *ref)
    got = [t.to(DEV).clone() for t in (accum, denom, max_radii)]
    densification_stats(grad.to(DEV), radii.to(DEV), *got)
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    vis = radii > 0
    want = accum.double().clone()
    want[vis] += grad[vis].double().pow(2).sum(-1, keepdim=True).sqrt()
    assert bool(torch.isfinite(got[0]).all())
    assert float(((got[0].cpu().double() - want).abs() / want.abs()).max()) <= 1e-6
    for a, b in zip(got, (accum, denom, max_radii)):                                    # invisible rows: the bits they had
        assert torch.equal(a.cpu()[~vis], b[~vis])
    once = [t.clone() for t in got]
    densification_stats(grad.to(DEV), radii.to(DEV), *got)                              # a second view accumulates
    assert torch.equal(got[1].cpu()[vis], denom[vis] + 2) and torch.equal(got[2], once[2])
    twice = accum.double().clone(); twice[vis] += 2 * grad[vis].double().pow(2).sum(-1, keepdim=True).sqrt()
    assert float(((got[0].cpu().double() - twice).abs() / twice.abs()).max()) <= 2e-6   # two accumulations: twice the bound of one


def test_densification_statistics_accept_flat_shapes():
    grad, radii, accum, denom, max_radii = oc.stats_case(65, "third")
    a = [t.to(DEV).clone() for t in (accum, denom, max_radii)]
    b = [accum.reshape(-1).to(DEV).clone(), denom.reshape(-1).to(DEV).clone(), max_radii.reshape(-1, 1).to(DEV).clone()]
    densification_stats(grad.to(DEV), radii.to(DEV), *a)
    densification_stats(grad.to(DEV), radii.to(DEV), *b)
    assert all(torch.equal(x.reshape(-1), y.reshape(-1)) for x, y in zip(a, b))


def _raw_model(g, noise, seed):
    """The reference's raw parameter set for Gaussians `g`, perturbed by `noise` (0: exactly g) -- as in tests/test_gpu_fit.py."""
    r = torch.Generator().manual_seed(seed)
    n = lambda t, s: t + s * noise * torch.randn(t.shape, generator=r)
    z = g["means3D"][:, 2:3]
    xyz = n(g["means3D"], 0.004 * z)
    scaling = n(torch.log(g["scales"]), 0.4)
    opacity = n(torch.logit(g["opacities"].clamp(1e-3, 1 - 1e-3)), 1.0)
    rotation = n(g["rotations"], 0.3)
    feats = g["shs"].clone(); feats[:, 0] = n(feats[:, 0], 0.5)
    leaf = lambda t: t.float().to(DEV).requires_grad_()
    return SurfelModel(leaf(xyz), leaf(scaling), leaf(rotation), leaf(opacity), leaf(feats), None, 3, 3, raw=True)


def test_toy_scene_is_fitted_with_the_fused_tail():
    """The loop of tests/test_gpu_fit.py at its sizes with SurfelAdam and densification_stats in the place of torch.optim.Adam and the
    boolean-indexed statistics: the same end conditions."""
    P, W, H, iters = 6000, 320, 180, 120
    g = synthetic_gaussians(P, W, H, seed=5, scale_lo=4e-3, scale_hi=4e-2)
    cams = [synthetic_camera(W, H, index=k).to(DEV) for k in (2, 3, 4, 5)]
    pipe = PipelineParams(depth_ratio=0.0, fused_activations=True)
    bg = torch.tensor([0.05, 0.05, 0.05], device=DEV)
    with torch.no_grad():
        truth = _raw_model(g, 0.0, 0)
        targets = [render(c, truth, pipe, bg)["render"].clone() for c in cams]
    pc = _raw_model(g, 1.0, 1)
    opt = SurfelAdam([dict(params=[pc._xyz], lr=2e-3), dict(params=[pc._features], lr=1e-2), dict(params=[pc._opacity], lr=5e-2),
                      dict(params=[pc._scaling], lr=1e-2), dict(params=[pc._rotation], lr=1e-2)], eps=1e-15)
    accum, denom, max_radii = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV), torch.zeros(P, device=DEV)
    l1_first, l1_last = [], []
    for it in range(iters):
        k = it % len(cams)
        out = render(cams[k], pc, pipe, bg)
        l1 = (out["render"] - targets[k]).abs().mean()
        normal_error = (1.0 - (out["rend_normal"] * out["surf_normal"]).sum(dim=0)).mean()
        loss = l1 + 0.05 * normal_error + 10.0 * out["rend_dist"].mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        densification_stats(out["viewspace_points"].grad, out["radii"], accum, denom, max_radii)
        opt.step()
        (l1_first if it < len(cams) else l1_last if it >= iters - len(cams) else []).append(l1.detach())
    assert all(bool(torch.isfinite(p).all()) for grp in opt.param_groups for p in grp["params"]), "non-finite parameter"
    first, last = float(sum(l1_first)) / len(l1_first), float(sum(l1_last)) / len(l1_last)
    assert math.isfinite(last) and last < 0.45 * first, f"L1 {first:.4f} -> {last:.4f} after {iters} Adam steps"
    seen = denom > 0
    assert float(seen.float().mean()) > 0.7 and float((accum[seen] / denom[seen]).mean()) > 0, "densification statistics stayed empty"
    assert bool((max_radii[seen.reshape(-1)] > 0).all()) and not max_radii[~seen.reshape(-1)].any()

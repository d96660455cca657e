"""CPU: the float64 checker of the fused Adam step is torch.optim.Adam; what SurfelAdam refuses; the argument errors of the two C-ABI entry
points (no GPU needed: they are raised before any launch)."""
import ctypes

import pytest
import torch

from streetunveiler_amd import _lib
from streetunveiler_amd.build import build
from streetunveiler_amd.optim import (ADAM_CHUNK, SurfelAdam, adam_step, adam_step_float64, densification_stats,
                                      densification_stats_torch)
from tests import optim_cases as oc


def test_float64_checker_is_torch_adam():
    """20 steps of the reference's six row widths at P = 37 on float64 CPU tensors: a learning rate per group, a starting step count per
    tensor, eps = 1e-15 -> p, m and v of adam_step_float64 within 1e-12 (relative to each tensor's largest magnitude) of torch.optim.Adam."""
    P = 37
    state = [tuple(t.double() for t in pmv) for pmv in oc.seeded_state(oc.reference_shapes(P), seed=4)]
    start = [0, 3, 11, 1, 250, 7]
    params = [torch.nn.Parameter(p.clone()) for p, _, _ in state]
    opt = torch.optim.Adam([dict(params=[p], lr=lr, name=name) for p, (name, _, lr) in zip(params, oc.GROUPS)], lr=0.0, eps=oc.EPS)
    for p, (_, m, v), t in zip(params, state, start):
        opt.state[p] = dict(step=torch.tensor(float(t)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    mine = [[p.clone() for p, _, _ in state], [m.clone() for _, m, _ in state], [v.clone() for _, _, v in state]]
    lrs = [lr for _, _, lr in oc.GROUPS]
    for it in range(1, 21):
        grads = [oc.seeded_gradient(p.shape, 100 * it + k).double() for k, p in enumerate(params)]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
        adam_step_float64(mine[0], grads, mine[1], mine[2], lrs, [t + it for t in start], *oc.BETAS, oc.EPS)
    for k, p in enumerate(params):
        assert float(opt.state[p]["step"]) == start[k] + 20
        for name, a, b in (("p", mine[0][k], p.detach()), ("m", mine[1][k], opt.state[p]["exp_avg"]), ("v", mine[2][k], opt.state[p]["exp_avg_sq"])):
            e = float((a - b).abs().max() / b.abs().max())
            assert e <= 1e-12, (oc.GROUPS[k][0], name, e)


def test_float64_checker_refuses_float32():
    t = torch.zeros(3)
    with pytest.raises(ValueError, match="float64"):
        adam_step_float64([t], [t], [t], [t], [1e-3], [1], 0.9, 0.999, 1e-8)


@pytest.mark.parametrize("kw, match", [(dict(weight_decay=0.1), "weight_decay"), (dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"),
                                       (dict(capturable=True), "capturable"), (dict(differentiable=True), "differentiable"),
                                       (dict(lr=-1.0), "learning rate"), (dict(eps=-1.0), "epsilon"), (dict(betas=(1.0, 0.9)), "beta")])
def test_constructor_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        SurfelAdam([torch.nn.Parameter(torch.zeros(4, 3))], **kw)


def test_constructor_refuses_other_dtypes_and_keeps_adams_groups():
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="float32"):
            SurfelAdam([torch.nn.Parameter(torch.zeros(4, 3, dtype=dtype))])
    p = torch.nn.Parameter(torch.zeros(4, 3))
    mine, theirs = SurfelAdam([dict(params=[p], lr=0.5, name="xyz")], lr=0.0, eps=1e-15), torch.optim.Adam([dict(params=[p], lr=0.5, name="xyz")], lr=0.0, eps=1e-15)
    assert mine.state_dict()["param_groups"] == theirs.state_dict()["param_groups"]
    assert mine.param_groups[0].keys() == theirs.param_groups[0].keys()


def test_options_smuggled_into_a_group_are_refused_at_the_step():
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.ones(4, 3)
    opt = SurfelAdam([p])
    opt.param_groups[0]["weight_decay"] = 0.01
    with pytest.raises(ValueError, match="weight_decay"):
        opt.step()


def test_cpu_tensors_are_refused_and_leave_no_state():
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.ones(4, 3)
    opt = SurfelAdam([p])
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        opt.step()
    assert len(opt.state) == 0
    t = torch.zeros(5)
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        adam_step([t], [t], [t], [t], [1e-3], [1], 0.9, 0.999, 1e-8)
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        densification_stats(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32), torch.zeros(5, 1), torch.zeros(5, 1), torch.zeros(5))


def test_raw_call_refusals():
    t = torch.zeros(5)
    with pytest.raises(ValueError, match="float32"):
        adam_step([t.double()], [t.double()], [t.double()], [t.double()], [1e-3], [1], 0.9, 0.999, 1e-8)
    with pytest.raises(ValueError, match="one entry per tensor"):
        adam_step([t], [t], [t], [t], [1e-3], [], 0.9, 0.999, 1e-8)
    with pytest.raises(ValueError, match="sparse"):
        adam_step([t], [t.to_sparse()], [t], [t], [1e-3], [1], 0.9, 0.999, 1e-8)
    with pytest.raises(ValueError, match="does not match"):
        adam_step([t], [torch.zeros(4)], [t], [t], [1e-3], [1], 0.9, 0.999, 1e-8)
    with pytest.raises(ValueError, match="int32"):
        densification_stats(torch.zeros(5, 3), torch.zeros(5), torch.zeros(5, 1), torch.zeros(5, 1), torch.zeros(5))
    with pytest.raises(ValueError, match=r"\[5,3\]"):
        densification_stats(torch.zeros(5, 2), torch.zeros(5, dtype=torch.int32), torch.zeros(5, 1), torch.zeros(5, 1), torch.zeros(5))
    with pytest.raises(ValueError, match="denom"):
        densification_stats(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32), torch.zeros(5, 1), torch.zeros(4, 1), torch.zeros(5))


def test_statistics_checker_is_the_references_three_lines():
    """densification_stats_torch on the CPU against the statement written out row by row in float64."""
    grad, radii, accum, denom, max_radii = oc.stats_case(65, "third")
    want = [t.double().clone() for t in (accum, denom, max_radii)]
    for i in range(65):
        if radii[i] > 0:
            want[0][i, 0] += grad[i].double().pow(2).sum().sqrt()
            want[1][i, 0] += 1
            want[2][i] = max(want[2][i], float(radii[i]))
    densification_stats_torch(grad, radii, accum, denom, max_radii)
    assert torch.equal(denom.double(), want[1]) and torch.equal(max_radii.double(), want[2])
    assert torch.allclose(accum.double(), want[0], rtol=1e-6, atol=0)


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def test_adam_step_argument_errors_without_gpu(lib):
    assert ctypes.sizeof(_lib.SrAdamSegment) == 4 * 8 + 8 + 2 * 4 and ADAM_CHUNK == 4096
    args = (0.9, 0.999, 1e-15, None)
    seg = lambda p=64, g=128, m=192, v=256, n=4: _lib.SrAdamSegment(p, g, m, v, n, 1e-3, 1.0)
    table = lambda *segs: (_lib.SrAdamSegment * len(segs))(*segs)

    def refused(segments, n, *rest, text):
        rc = lib.sr_adam_step(segments, n, *(rest or args))
        assert rc == -1 and text in lib.sr_last_error(), (rc, lib.sr_last_error())

    refused(None, 1, text=b"segments is NULL")
    refused(table(seg()), 0, text=b"n_segments 0 not in 1..8")
    refused(table(*[seg()] * 9), 9, text=b"n_segments 9 not in 1..8")
    refused(table(seg(), seg(n=-1)), 2, text=b"segment 1: n -1 is negative")
    refused(table(seg(p=None)), 1, text=b"segment 0: param is NULL")
    refused(table(seg(g=None)), 1, text=b"segment 0: grad is NULL")
    refused(table(seg(), seg(), seg(m=None)), 3, text=b"segment 2: exp_avg is NULL")
    refused(table(seg(v=None)), 1, text=b"segment 0: exp_avg_sq is NULL")
    refused(table(seg(v=258)), 1, text=b"segment 0: exp_avg_sq is not 4-B aligned")
    refused(table(seg(p=65)), 1, text=b"segment 0: param is not 4-B aligned")
    refused(table(seg()), 1, 1.0, 0.999, 1e-15, None, text=b"beta1")
    refused(table(seg()), 1, 0.9, -0.1, 1e-15, None, text=b"beta2")
    refused(table(seg()), 1, 0.9, 0.999, -1.0, None, text=b"eps")
    assert lib.sr_adam_step(table(seg(n=0), seg(n=0)), 2, *args) == 0       # nothing to do: no launch, no device needed


def test_densification_stats_argument_errors_without_gpu(lib):
    ok = [64, 128, 192, 256, 320]
    names = [b"viewspace_grad", b"radii", b"xyz_gradient_accum", b"denom", b"max_radii2D"]
    assert lib.sr_densification_stats(-1, *ok, None) == -1 and b"P < 0" in lib.sr_last_error()
    assert lib.sr_densification_stats(0, None, None, None, None, None, None) == 0
    for k, name in enumerate(names):
        ptrs = list(ok); ptrs[k] = None
        assert lib.sr_densification_stats(8, *ptrs, None) == -1 and name + b" is NULL" in lib.sr_last_error()
        ptrs[k] = ok[k] + 2
        assert lib.sr_densification_stats(8, *ptrs, None) == -1 and b"not 4-B aligned" in lib.sr_last_error()

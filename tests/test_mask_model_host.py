"""CPU: the checker of the masked model against the literal statement; the model's groups, state, mask bits, reset, prune and compose
cache as the reference's class states them [REF scene/mask_gaussian.py]; the argument errors of the three C-ABI entry points (no GPU
needed: they are raised before any launch)."""
import ctypes
import os
import re

import pytest
import torch

from streetunveiler_amd import _lib, mask_model as mm
from streetunveiler_amd.build import build
from streetunveiler_amd.optim import SurfelAdam, adam_step
from tests import mask_model_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checker_is_the_literal_statement():
    """compose_masked_torch on CPU float64 against `base + delta * mask[..., None]` written out here, on every case."""
    for c in mc.cases():
        base, delta = mc.make_tensors(c.P, c.degree, dtype=torch.float64)
        mask = mc.make_mask(c.P, c.mask_kind, c.mask_dtype)
        eff = mm.compose_masked_torch(base, delta, mask, c.fixed)
        want = []
        for name, b, d in zip(mm.PROPERTIES, base, delta):
            m = mask.double().reshape((c.P,) + (1,) * (b.dim() - 1))
            want.append(b if name in c.fixed else b + d * m)
        want = [want[0], torch.cat((want[1], want[2]), dim=1), want[3], want[4], want[5]]
        for name, a, b in zip(mm.Effective._fields, eff, want):
            assert a.dtype == torch.float64 and torch.equal(a, b), (c, name)


def test_fixed_bits_are_the_references():
    assert mm.MASK_PROPERTY == ["xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"]
    assert mm.MASK_PROPERTY_BIT == {"xyz": 1, "features_dc": 2, "features_rest": 4, "scaling": 8, "rotation": 16, "opacity": 32}
    assert mm.fixed_bits(()) == 0 and mm.fixed_bits(("opacity", "xyz")) == 33 and mm.fixed_bits(63) == 63
    assert (_lib.SR_MASK_FIXED_XYZ, _lib.SR_MASK_FIXED_FEATURES_DC, _lib.SR_MASK_FIXED_FEATURES_REST, _lib.SR_MASK_FIXED_SCALING,
            _lib.SR_MASK_FIXED_ROTATION, _lib.SR_MASK_FIXED_OPACITY) == (1, 2, 4, 8, 16, 32)
    with pytest.raises(ValueError, match="unknown property"):
        mm.fixed_bits(("colour",))
    with pytest.raises(ValueError, match="beyond"):
        mm.fixed_bits(64)


def _model(P=11, degree=3):
    src = mc.SourceModel(P, degree)
    model = mm.MaskedSurfelModel(degree).from_gaussian_model(src)
    return src, model


def test_model_groups_state_and_bits():
    src, model = _model()
    assert model.points_number == 11 and model.active_sh_degree == 3 and model.max_sh_degree == 3 and model.spatial_lr_scale == 2.5
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        frozen, delta = getattr(model, name), getattr(model, "_new" + name)
        assert torch.equal(frozen, getattr(src, name).detach()) and frozen.data_ptr() != getattr(src, name).data_ptr() and not frozen.requires_grad
        assert isinstance(delta, torch.nn.Parameter) and delta.requires_grad and delta.shape == frozen.shape and not delta.any()
    assert model.mask.shape == (11,) and model.mask.dtype == torch.bool and bool(model.mask.all())      # set_nograd: every Gaussian trainable
    mask = torch.arange(11) % 3 == 0
    model.set_mask(mask)
    model.training_setup(mc.TrainingArgs)
    assert isinstance(model.optimizer, SurfelAdam)
    a = mc.TrainingArgs
    want = [("new_xyz", model._new_xyz, a.position_lr_init * 2.5), ("new_f_dc", model._new_features_dc, a.feature_lr),
            ("new_f_rest", model._new_features_rest, a.feature_lr / 20.0), ("new_opacity", model._new_opacity, a.opacity_lr),
            ("new_scaling", model._new_scaling, a.scaling_lr), ("new_rotation", model._new_rotation, a.rotation_lr)]
    assert len(model.optimizer.param_groups) == 6
    for group, (name, p, lr) in zip(model.optimizer.param_groups, want):
        assert group["name"] == name and group["params"][0] is p and group["lr"] == lr and group["eps"] == 1e-15 and group["betas"] == (0.9, 0.999)
    assert model.optimizer.row_mask() is model.mask                              # the model's own mask, read at every step
    assert model.xyz_gradient_accum.shape == (11, 1) and model.denom.shape == (11, 1) and model.percent_dense == a.percent_dense
    # the schedule of the reference: lr_init at 0, lr_final at max_steps, log-linear between
    assert model.update_learning_rate(0) == pytest.approx(a.position_lr_init * 2.5, rel=1e-12)
    assert model.update_learning_rate(a.position_lr_max_steps) == pytest.approx(a.position_lr_final * 2.5, rel=1e-12)
    assert model.update_learning_rate(15000) == pytest.approx(2.5 * (a.position_lr_init * a.position_lr_final) ** 0.5, rel=1e-12)
    assert model.optimizer.param_groups[0]["lr"] == model.update_learning_rate(15000)
    # mask_property_bit
    assert model.mask_property_bit == 0 and not any(getattr(model, "check_fixed_" + n) for n in mm.MASK_PROPERTY)
    for k, n in enumerate(mm.MASK_PROPERTY):
        getattr(model, "set_fixed_" + n)()
        assert getattr(model, "check_fixed_" + n) and model.mask_property_bit == (2 << k) - 1
    model.active_sh_degree = 2
    model.oneupSHdegree(); model.oneupSHdegree()
    assert model.active_sh_degree == 3
    sem = src._semantics
    assert torch.equal(model.get_semantics, sem.squeeze(-1)) and torch.equal(model.get_semantics_32bit, (1 << sem.to(torch.int32)).squeeze(-1))


def _cpu_stub(calls):
    """In place of the kernel: the checker's arithmetic on the CPU, and a count."""
    def forward(base, delta, mask_u8, bits):
        calls.append(bits)
        eff = mm.compose_masked_torch(base, delta, mask_u8.bool(), bits)
        own = (mm.MASK_PROPERTY_BIT["xyz"], 0, mm.MASK_PROPERTY_BIT["opacity"], mm.MASK_PROPERTY_BIT["scaling"], mm.MASK_PROPERTY_BIT["rotation"])
        return [None if bits & own[k] else e.clone() for k, e in enumerate(eff)]

    def backward(upstream, mask_u8, bits, P, M, wanted):
        m = mask_u8.bool()
        g = [upstream[0], None if upstream[1] is None else upstream[1][:, :1], None if upstream[1] is None else upstream[1][:, 1:]] + list(upstream[2:])
        return [(g[k] * m.reshape((P,) + (1,) * (g[k].dim() - 1))).contiguous() if wanted[k] else None for k in range(6)]
    return forward, backward


@pytest.fixture
def stubbed(monkeypatch):
    calls = []
    forward, backward = _cpu_stub(calls)
    monkeypatch.setattr(mm, "_compose_forward", forward)
    monkeypatch.setattr(mm, "_compose_backward", backward)
    return calls


def test_one_compose_per_iteration_and_dropped_after_backward(stubbed):
    _, model = _model()
    model.set_mask(torch.arange(11) % 2 == 0)
    getters = lambda: (model.get_xyz, model.get_features, model.get_opacity, model.get_scaling, model.get_rotation, model.raw_parameters())
    first = getters()
    getters()
    assert len(stubbed) == 1                                    # ten getters and two raw_parameters: one compose
    assert model.get_features.shape == (11, 16, 3) and model.get_xyz is first[0]
    loss = sum(t.sum() for t in first[:5])
    loss.backward()
    assert model._cache is None                                 # a backward has passed through it
    assert torch.equal(model._new_xyz.grad, (torch.arange(11) % 2 == 0).float()[:, None].expand(11, 3))
    getters()
    assert len(stubbed) == 2                                    # a render after the backward recomputes
    with torch.no_grad():
        assert not model.get_xyz.requires_grad
        assert len(stubbed) == 3                                # the grad mode is part of the key
        model._new_xyz.add_(1.0)
        model.get_opacity
        assert len(stubbed) == 4                                # an in-place update of a delta (a torch one here; that the optimizer's
                                                                # step counts as one is tests/test_gpu_mask_model.py's to show)
        model.mask[0] = False
        model.get_opacity
        assert len(stubbed) == 5                                # ... of the mask
        model.set_mask(torch.ones(11))
        model.get_opacity
        assert len(stubbed) == 6 and model.mask.dtype == torch.bool and bool(model.mask.all())      # a new mask: float 0 / 1 -> bool, once
        model.set_fixed_opacity()
        assert torch.equal(model.get_opacity, torch.sigmoid(model._opacity)) and stubbed[-1] == 32 and len(stubbed) == 7
        model.get_rotation
        assert len(stubbed) == 7


def test_mask_edited_between_forward_and_backward_raises(stubbed):
    """The backward masks with the rows the forward used: the mask is saved for it, so autograd refuses a mask edited in place since."""
    _, model = _model()
    model.set_mask(torch.arange(11) % 2 == 0)
    loss = model.get_xyz.sum()
    model.mask[1] = True
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


@pytest.mark.parametrize("fixed", ["scaling", "xyz"])
def test_reset_mask_folds_zeroes_and_renews(stubbed, fixed):
    _, model = _model()
    old_mask = torch.arange(11) % 2 == 0
    model.set_mask(old_mask)
    model.training_setup(mc.TrainingArgs)
    getattr(model, "set_fixed_" + fixed)()
    base = [t.clone() for t in model._base()]
    with torch.no_grad():
        for k, d in enumerate(model._delta()):
            d.copy_(torch.full_like(d, 0.25 * (k + 1)))
    delta = [d.detach().clone() for d in model._delta()]
    old_optimizer = model.optimizer
    model.optimizer.state[model._new_xyz] = dict(step=torch.tensor(3.0), exp_avg=torch.ones(11, 3), exp_avg_sq=torch.ones(11, 3))
    new_mask = torch.arange(11) < 4
    n = len(stubbed)
    model.reset_mask(new_mask, mc.TrainingArgs)
    # ONE compose.  Every property is folded, a fixed one too [REF :124-128], but for xyz: the reference folds `get_xyz` [REF :123],
    # which is the base alone while xyz is fixed
    assert len(stubbed) == n + 1 and stubbed[-1] == (1 if fixed == "xyz" else 0)
    want = mm.compose_masked_torch(base, delta, old_mask, ("xyz",) if fixed == "xyz" else ())
    got = [model._xyz, torch.cat((model._features_dc, model._features_rest), dim=1), model._opacity, model._scaling, model._rotation]
    for a, b in zip(got, want):
        assert torch.equal(a, b) and not a.requires_grad
    assert model._features_dc.shape == (11, 1, 3) and model._features_rest.shape == (11, 15, 3)
    assert all(isinstance(d, torch.nn.Parameter) and not d.any() for d in model._delta())
    assert model.optimizer is not old_optimizer and len(model.optimizer.state) == 0
    assert all(g["params"][0] is d for g, d in zip(model.optimizer.param_groups, model._delta()))
    assert torch.equal(model.mask, new_mask) and not model.xyz_gradient_accum.any()


def test_prune_keeps_every_row_tensor_aligned():
    _, model = _model(P=13)
    mask = torch.arange(13) % 2 == 0
    model.set_mask(mask)
    model.training_setup(mc.TrainingArgs)
    rows = torch.arange(13.0)
    with torch.no_grad():
        for t in model._base() + model._delta():
            t.copy_(rows.reshape((13,) + (1,) * (t.dim() - 1)).expand_as(t))
    model._semantics = torch.arange(13).reshape(13, 1)
    model.max_radii2D = rows.clone()
    model.xyz_gradient_accum, model.denom = rows.reshape(13, 1).clone(), rows.reshape(13, 1).clone()
    model.next_editable_pcd_mask = torch.arange(13) > 6
    for p in model._delta():
        model.optimizer.state[p] = dict(step=torch.tensor(2.0), exp_avg=p.detach().clone(), exp_avg_sq=p.detach().clone())
    prune = torch.zeros(13, dtype=torch.bool)
    prune[[0, 5, 12]] = True
    assert model.prune_points_with_mask(prune) is prune
    keep = rows[~prune]
    assert model.points_number == 10
    for t in model._base() + model._delta():
        assert t.shape[0] == 10 and torch.equal(t.reshape(10, -1)[:, 0], keep)
    for group, p in zip(model.optimizer.param_groups, model._delta()):
        assert group["params"][0] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad
        state = model.optimizer.state[p]
        assert float(state["step"]) == 2.0 and torch.equal(state["exp_avg"].reshape(10, -1)[:, 0], keep) and torch.equal(state["exp_avg_sq"].reshape(10, -1)[:, 0], keep)
    assert len(model.optimizer.state) == 6
    assert torch.equal(model._semantics.reshape(-1).float(), keep) and torch.equal(model.max_radii2D, keep)
    assert torch.equal(model.xyz_gradient_accum.reshape(-1), keep) and torch.equal(model.denom.reshape(-1), keep)
    assert torch.equal(model.mask, mask[~prune]) and torch.equal(model.next_editable_pcd_mask, (torch.arange(13) > 6)[~prune])


def test_densification_stats_are_masked():
    _, model = _model()
    model.set_mask((torch.arange(11) % 2 == 0).float())
    model.training_setup(mc.TrainingArgs)
    points = torch.zeros(11, 3)
    points.grad = torch.tensor([3.0, 4.0, 100.0]).expand(11, 3).clone()
    visible = torch.arange(11) < 6
    model.add_densification_stats(points, visible)
    want = ((torch.arange(11) % 2 == 0) & visible).float()[:, None]
    assert torch.equal(model.xyz_gradient_accum, 5.0 * want) and torch.equal(model.denom, want)      # the norm of the first TWO components


def test_save_ply_writes_the_folded_model(tmp_path, stubbed):
    from streetunveiler_amd.ply import load_ply
    _, model = _model()
    model.set_mask(torch.arange(11) % 2 == 0)
    with torch.no_grad():
        model._new_xyz.fill_(1.0)
    model.set_fixed_xyz()                                       # save_ply folds every property, as the reference's does
    model.save_ply(os.path.join(tmp_path, "m.ply"))
    d = load_ply(os.path.join(tmp_path, "m.ply"), 3)
    want = mm.compose_masked_torch(model._base(), [t.detach() for t in model._delta()], model.mask, ())
    assert torch.equal(torch.tensor(d["xyz"]), want.xyz) and torch.equal(torch.tensor(d["features_rest"]), want.features[:, 1:])
    assert torch.equal(torch.tensor(d["semantics"]).reshape(-1), model._semantics.reshape(-1).to(torch.int32))


def test_cpu_tensors_are_refused():
    base, delta = mc.make_tensors(5, 1)
    mask = mc.make_mask(5, "alternating")
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        mm.compose_masked(base, delta, mask)
    _, model = _model()
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        model.get_xyz
    model.training_setup(mc.TrainingArgs)
    model._new_xyz.grad = torch.ones(11, 3)
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        model.optimizer.step()
    t = torch.zeros(5, 3)
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        adam_step([t], [t], [t], [t], [1e-3], [1], 0.9, 0.999, 1e-8, row_mask=mask)


def test_python_argument_refusals():
    base, delta = mc.make_tensors(5, 1)
    mask = mc.make_mask(5, "alternating")
    with pytest.raises(ValueError, match="six tensors"):
        mm.compose_masked(base[:5], delta, mask)
    with pytest.raises(ValueError, match=r"delta opacity must be \[5, 1\]"):
        mm.compose_masked(base, delta[:3] + [delta[3].reshape(5)] + delta[4:], mask)
    with pytest.raises(ValueError, match=r"mask must be \[5\]"):
        mm.compose_masked(base, delta, mask[:4])
    with pytest.raises(ValueError, match="float32"):
        mm.compose_masked([t.double() for t in base], [t.double() for t in delta], mask)
    t = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="leading dimension"):
        adam_step([t], [t], [t], [t], [1e-3], [1], 0.9, 0.999, 1e-8, row_mask=torch.ones(4))
    with pytest.raises(ValueError, match=r"row mask must be \[P\]"):
        adam_step([t], [t], [t], [t], [1e-3], [1], 0.9, 0.999, 1e-8, row_mask=torch.ones(5, 1))
    assert SurfelAdam([torch.nn.Parameter(t)]).row_mask is None               # without it nothing changes


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_listed(lib):
    header = open(os.path.join(ROOT, "include", "surfel_raster.h")).read()
    for name in ("sr_mask_compose", "sr_mask_compose_backward", "sr_adam_step_rows"):
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.EXPORTS and hasattr(lib, name)
    assert header.count("Added without a new SR_ABI_VERSION") >= 5 and lib.sr_abi_version() == _lib.SR_ABI_VERSION
    assert ctypes.sizeof(_lib.SrAdamSegment) == 48 and ctypes.sizeof(_lib.SrAdamRowSegment) == 56      # the old layout is untouched
    assert ctypes.sizeof(_lib.SrMaskTensors) == 48 and ctypes.sizeof(_lib.SrMaskEffective) == 40


def test_adam_step_rows_argument_errors_without_gpu(lib):
    args = (0.9, 0.999, 1e-15, None)
    seg = lambda p=64, g=128, m=192, v=256, n=12, row_len=3: _lib.SrAdamRowSegment(p, g, m, v, n, 1e-3, 1.0, row_len)
    table = lambda *segs: (_lib.SrAdamRowSegment * len(segs))(*segs)

    def refused(segments, n, P, mask, *rest, text):
        rc = lib.sr_adam_step_rows(segments, n, P, mask, *(rest or args))
        assert rc == -1 and text in lib.sr_last_error(), (rc, lib.sr_last_error())

    refused(None, 1, 4, 512, text=b"segments is NULL")
    refused(table(seg()), 0, 4, 512, text=b"n_segments 0 not in 1..8")
    refused(table(*[seg()] * 9), 9, 4, 512, text=b"n_segments 9 not in 1..8")
    refused(table(seg()), 1, -1, 512, text=b"P < 0")
    refused(table(seg()), 1, 4, None, text=b"mask is NULL")
    refused(table(seg(row_len=0)), 1, 4, 512, text=b"row_len 0 not in")
    refused(table(seg(row_len=1 << 30, n=4 << 30)), 1, 4, 512, text=b"row_len 1073741824 not in")
    refused(table(seg(), seg(n=13)), 2, 4, 512, text=b"segment 1: n 13 is not P * row_len = 4 * 3")
    refused(table(seg(n=-3, row_len=3)), 1, -1, 512, text=b"P < 0")
    refused(table(seg(p=None)), 1, 4, 512, text=b"segment 0: param is NULL")
    refused(table(seg(g=None)), 1, 4, 512, text=b"segment 0: grad is NULL")
    refused(table(seg(m=None)), 1, 4, 512, text=b"segment 0: exp_avg is NULL")
    refused(table(seg(v=258)), 1, 4, 512, text=b"segment 0: exp_avg_sq is not 4-B aligned")
    refused(table(seg()), 1, 4, 512, 1.0, 0.999, 1e-15, None, text=b"beta1")
    refused(table(seg()), 1, 4, 512, 0.9, -0.1, 1e-15, None, text=b"beta2")
    refused(table(seg()), 1, 4, 512, 0.9, 0.999, -1.0, None, text=b"eps")
    assert lib.sr_adam_step_rows(table(seg(n=0), seg(n=0, row_len=45)), 2, 0, None, *args) == 0      # P == 0: no launch, no device needed
    assert lib.sr_adam_step_rows(table(seg(n=0, p=None, g=None, m=None, v=None)), 1, 0, None, *args) == 0


def test_mask_compose_argument_errors_without_gpu(lib):
    six = lambda **kw: _lib.SrMaskTensors(*[kw.get(n, 64 * (k + 1)) for k, n in enumerate(mm.PROPERTIES)])
    five = lambda **kw: _lib.SrMaskEffective(*[kw.get(n, 1024 + 64 * k) for k, n in enumerate(mm.Effective._fields)])
    ref = ctypes.byref

    def compose(P=4, M=16, base=six(), delta=six(), mask=512, bits=0, out=five()):
        return lib.sr_mask_compose(P, M, ref(base) if base else None, ref(delta) if delta else None, mask, bits, ref(out) if out else None, None)

    def backward(P=4, M=16, upstream=five(), mask=512, bits=0, d=six()):
        return lib.sr_mask_compose_backward(P, M, ref(upstream) if upstream else None, mask, bits, ref(d) if d else None, None)

    def refused(rc, text, code=-1):
        assert rc == code and text in lib.sr_last_error(), (rc, lib.sr_last_error())

    for call in (compose, backward):
        refused(call(P=-1), b"P < 0")
        refused(call(M=0), b"sh_coeffs 0 < 1")
        refused(call(bits=64), b"fixed_bits 64")
        refused(call(mask=None), b"mask is NULL")
        refused(call(P=1 << 30, M=16), b"reaches 2^31", code=-4)                 # SR_ERR_UNSUPPORTED
        assert call(P=0, mask=None) == 0                                        # no work, no device needed
    assert lib.sr_mask_compose(0, 1, None, None, None, 0, None, None) == 0 and lib.sr_mask_compose_backward(0, 1, None, None, 0, None, None) == 0
    refused(compose(base=None), b"base / delta / out is NULL")
    refused(compose(out=None), b"base / delta / out is NULL")
    refused(compose(base=six(scaling=None)), b"base.scaling is NULL")
    refused(compose(delta=six(rotation=None)), b"delta.rotation is NULL")
    refused(compose(delta=six(features_rest=None)), b"delta.features_rest is NULL")
    refused(compose(base=six(xyz=66)), b"base.xyz is not 4-B aligned")
    refused(compose(out=five(opacity=None)), b"out.opacity is NULL")
    refused(compose(out=five(features=None), bits=2), b"out.features is NULL")       # only ONE half is fixed
    refused(compose(out=five(rotation=1027)), b"out.rotation is not 4-B aligned")
    refused(backward(upstream=None), b"upstream / d_delta is NULL")
    refused(backward(d=None), b"upstream / d_delta is NULL")
    refused(backward(bits=8), b"d_delta.scaling is asked for, but the property is fixed")
    refused(backward(upstream=five(features=None)), b"d_delta.features_dc is asked for without upstream.features")
    refused(backward(d=six(opacity=70)), b"d_delta.opacity is not 4-B aligned")

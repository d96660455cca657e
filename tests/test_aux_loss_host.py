"""CPU: what tests/test_gpu_aux_loss.py stands on.  The float64 twins of streetunveiler_amd/aux_loss.py ARE the reference's lines; the
gradients include/surfel_raster.h states are the twins' autograd gradients; the bar of tests/aux_loss_cases.py turns away the wrong
restatements a kernel could plausibly be; the C-ABI refuses bad arguments before its first HIP call."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from streetunveiler_amd import _lib
from streetunveiler_amd import aux_loss as al
from streetunveiler_amd.build import build
from tests import aux_loss_cases as ac

FINITE = [c for c in ac.SEMANTIC if c["kind"] == "regular" and bool(torch.isfinite(c["x"]).all())]
by_name = lambda cases, name: next(c for c in cases if c["name"] == name)


def test_the_cases_are_the_ones_the_sizes_were_derived_for():
    assert al.MAX_CLASSES == 8 and ac.BLOCK == 256
    blocks = lambda n: -(-n // ac.BLOCK)
    assert blocks(ac.BIG[0] * ac.BIG[1]) == ac.BLOCK + 2 and blocks(ac.SHRINK_P[-1]) == ac.BLOCK + 1
    assert blocks(130 * 70) > 1 and (130 * 70) % ac.BLOCK != 0 and 67 % 64 != 0
    dtypes = {c["target"].dtype for c in ac.SEMANTIC}
    assert {torch.uint8, torch.int32, torch.int64, torch.float32} <= dtypes
    mixed = by_name(ac.SEMANTIC, "out_of_range_u8")["target"]
    assert {6, 7, 255} <= set(mixed.unique().tolist()) and set(range(6)) <= set(mixed.unique().tolist())
    assert {c["x"].shape[0] for c in ac.SEMANTIC} == {1, 6, 8}
    soft = by_name(ac.SEMANTIC, "soft_unnormalised")["target"].sum(0)
    assert float((soft - 1).abs().min()) > 1e-4
    assert len({c["name"] for c in ac.SEMANTIC + ac.SURFACE + ac.SHRINK}) == len(ac.SEMANTIC + ac.SURFACE + ac.SHRINK)


@pytest.mark.parametrize("name", ["unit_130x70", "out_of_range_i64", "negative_label_i32", "soft_unnormalised", "zero_weight", "all_out_of_range"])
def test_float64_twin_is_the_references_cross_entropy(name):
    """semantic_cross_entropy_torch == F.cross_entropy on the one-hot image the reference's camera builds, with the reference's float32
    weight tensor: labels, soft targets, labels the reference has no channel for."""
    case = by_name(ac.SEMANTIC, name)
    x, t = case["x"].double(), case["target"]
    if not t.is_floating_point():                                  # [REF scene/cameras.py:77-83]
        prob = torch.zeros((6, x.shape[1], x.shape[2]), dtype=torch.float32)
        for i in range(6):
            prob[i, t == i] = 1.0
        t = prob
    ref = F.cross_entropy(x.unsqueeze(0), t.double().unsqueeze(0), weight=torch.tensor(case["weight"]).double())   # [REF train.py:88]
    twin = al.semantic_cross_entropy_torch(x, case["target"], case["weight"])
    assert float(twin) == float(ref)
    # ... which divides by the pixel count: the header's sum of terms / N
    assert float(twin) == pytest.approx(float(ac.semantic_analytic(case)["loss"]), rel=1e-13, abs=1e-300)
    if name == "all_out_of_range":
        assert float(twin) == 0.0


@pytest.mark.parametrize("case", FINITE, ids=[c["name"] for c in FINITE])
def test_stated_semantic_gradient_is_autograds(case):
    truth, stated = ac.semantic_reference(case)[0], ac.semantic_analytic(case)
    np.testing.assert_allclose(stated["loss"], truth["loss"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(stated["g_logits"], truth["g_logits"], rtol=1e-9, atol=1e-18)


def test_class_index_form_is_the_one_hot_form_where_both_are_finite():
    """What the -inf case is held to: with every label in range and finite logits, the gathered form and the one-hot product agree."""
    case = by_name(ac.SEMANTIC, "unit_130x70")
    a = ac.class_index_loss(case["x"].double(), case["target"], case["weight"])
    assert float(a) == pytest.approx(float(ac.semantic_reference(case)[0]["loss"]), rel=1e-13)
    inf_case = by_name(ac.SEMANTIC, "neg_inf_beside_label")
    truth = ac.semantic_reference(inf_case)[0]
    assert np.isfinite(truth["loss"]) and np.isfinite(truth["g_logits"]).all()
    assert torch.isnan(al.semantic_cross_entropy_torch(inf_case["x"].double(), inf_case["target"], inf_case["weight"]))   # torch: 0 * -inf
    assert torch.isnan(al.semantic_cross_entropy_torch(inf_case["x"].double(), al.one_hot_image(inf_case["target"], 6), inf_case["weight"]))
    for name in ("nan_labels", "nan_soft", "nan_first_class"):
        assert np.isnan(ac.semantic_reference(by_name(ac.SEMANTIC, name))[0]["loss"]), name


@pytest.mark.parametrize("case", ac.SURFACE, ids=[c["name"] for c in ac.SURFACE])
def test_stated_surface_gradients_are_autograds(case):
    truth, stated = ac.surface_reference(case)[0], ac.surface_analytic(case)
    for k in truth:
        np.testing.assert_allclose(stated[k], truth[k], rtol=1e-12, atol=1e-300, err_msg=k)


@pytest.mark.parametrize("case", ac.SHRINK, ids=[c["name"] for c in ac.SHRINK])
def test_stated_shrink_gradient_is_autograds(case):
    truth, stated = ac.shrink_reference(case)[0], ac.shrink_analytic(case)
    for k in truth:
        np.testing.assert_allclose(stated[k], truth[k], rtol=1e-12, atol=1e-300, err_msg=k)
    assert np.isfinite(truth["g_opacity"]).all()


def test_the_bar_accepts_the_stated_functions_rounded_once():
    """The float64 statements rounded to float32 pass (so does the yardstick itself, by construction)."""
    for case in FINITE:
        truth, yard = ac.semantic_reference(case)
        ac.assert_within_bar(ac.as_float32(ac.semantic_analytic(case)), truth, yard, case["name"])
        ac.assert_within_bar(yard, truth, yard, case["name"] + " (yardstick)")
    for case in ac.SURFACE:
        truth, yard = ac.surface_reference(case)
        ac.assert_within_bar(ac.as_float32(ac.surface_analytic(case)), truth, yard, case["name"])
    for case in ac.SHRINK:
        truth, yard = ac.shrink_reference(case)
        ac.assert_within_bar(ac.as_float32(ac.shrink_analytic(case)), truth, yard, case["name"])


def _rejected(res, truth, yard):
    return [k for k, v in ac.worst(ac.as_float32(res), truth, yard).items() if not v <= 1.0]


def test_the_bar_rejects_wrong_semantic_losses():
    case = by_name(ac.SEMANTIC, "out_of_range_u8")
    truth, yard = ac.semantic_reference(case)
    good = ac.semantic_analytic(case)
    x, lab = case["x"].double(), case["target"].long()
    N = lab.numel()
    w = torch.tensor(case["weight"]).double()
    inside = lab < 6
    safe = lab.clamp(max=5)
    logp_l = F.log_softmax(x, 0).gather(0, safe[None])[0]
    terms = torch.where(inside, -w[safe] * logp_l, torch.zeros_like(logp_l))
    assert float(terms.sum() / N) == pytest.approx(float(truth["loss"]), rel=1e-13)
    wrong = {
        "divided by the weight sum (torch's class-index reduction)": terms.sum() / w[safe][inside].sum(),
        "out-of-range pixels dropped from N": terms.sum() / inside.sum(),
        "weight applied after the mean": w.mean() * torch.where(inside, -logp_l, torch.zeros_like(logp_l)).sum() / N,
    }
    for what, loss in wrong.items():
        assert "loss" in _rejected(dict(good, loss=loss.numpy()), truth, yard), what
    assert "g_logits" in _rejected(ac.semantic_analytic(case, drop_s=True), truth, yard), "softmax gradient without S"
    assert not _rejected(good, truth, yard)


def test_the_bar_rejects_wrong_regularisers_and_shrink():
    case = by_name(ac.SURFACE, "maps_130x70")
    truth, yard = ac.surface_reference(case)
    assert set(_rejected(ac.surface_analytic(case, swap=True), truth, yard)) == {"g_rend_normal", "g_surf_normal"}
    assert _rejected(ac.surface_analytic(case, drop_dist=True), truth, yard) == ["loss"]
    assert not _rejected(ac.surface_analytic(case), truth, yard)
    case = by_name(ac.SHRINK, "raw_65")
    truth, yard = ac.shrink_reference(case)
    assert _rejected(ac.shrink_analytic(case, plain_s=True), truth, yard) == ["g_opacity"]
    assert not _rejected(ac.shrink_analytic(case), truth, yard)


def test_the_bar_is_per_element_and_knows_non_finite_truths():
    truth = dict(v=np.array([1.0, 1.0, np.nan, np.inf, 0.0]))
    yard = dict(v=np.array([1.0, 1.0 + 2.0 ** -22, np.nan, np.inf, 0.0], dtype=np.float64))
    half = 2.0 ** -24
    assert ac.worst(dict(v=np.array([1.0 + half, 1.0 + 2.0 ** -21, np.nan, np.inf, 2.0 ** -150])), truth, yard)["v"] == 1.0
    for k, bad in enumerate([1.0 + 1.01 * half, 1.0 + 1.01 * 2.0 ** -21, 0.0, 1e38, 2.0 ** -149]):
        got = np.array([1.0, 1.0, np.nan, np.inf, 0.0])
        got[k] = bad
        assert ac.worst(dict(v=got), truth, yard)["v"] > 1.0, k
    assert ac.worst(dict(v=np.array([np.nan, 1.0, np.nan, np.inf, 0.0])), truth, yard)["v"] == np.inf


# ---- the C-ABI, without a GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


INVALID, TOO_SMALL = -1, -3


def test_argument_errors_without_gpu(lib):
    """Every refusal comes before the first HIP call of its entry point: only refused calls are made, on dummy host pointers."""
    dummy = ctypes.create_string_buffer(64)
    p, big = ctypes.addressof(dummy), 1 << 40
    w = (ctypes.c_float * 8)(*([1.0] * 8))

    def check(rc, code, fragment, what):
        assert rc == code and fragment.encode() in lib.sr_last_error(), (what, rc, lib.sr_last_error())

    fwd = lambda W=4, H=4, Cn=6, x=p, t=p, lb=1, ws=p, n=big, out=p: lib.sr_semantic_ce_forward(W, H, Cn, x, t, lb, w, ws, n, out, None)
    bwd = lambda W=4, H=4, Cn=6, x=p, t=p, lb=1, g=p, gx=p: lib.sr_semantic_ce_backward(W, H, Cn, x, t, lb, w, g, gx, None)
    for name, call in (("forward", fwd), ("backward", bwd)):
        check(call(Cn=9), INVALID, "classes", name + " C > 8")
        check(call(Cn=0), INVALID, "classes", name + " C < 1")
        check(call(W=0), INVALID, "image size", name + " W < 1")
        check(call(H=-3), INVALID, "image size", name + " H < 1")
        for lb in (2, 3, 16, -1):
            check(call(lb=lb), INVALID, "label_bytes", name + f" label width {lb}")
        check(call(x=None), INVALID, "NULL", name + " logits")
        check(call(t=None), INVALID, "NULL", name + " target")
    check(fwd(out=None), INVALID, "NULL", "forward out1")
    check(fwd(ws=None), INVALID, "NULL", "forward workspace")
    check(fwd(n=8), TOO_SMALL, "workspace", "forward short workspace")
    check(bwd(g=None), INVALID, "NULL", "backward g_loss")
    check(bwd(gx=None), INVALID, "NULL", "backward g_logits")

    reg_f = lambda W=4, H=4, rn=p, sn=p, rd=p, ws=p, n=big, out=p: lib.sr_surface_reg_forward(W, H, rn, sn, rd, 0.05, 100.0, ws, n, out, None)
    reg_b = lambda W=4, H=4, rn=p, sn=p, g=p, a=p, b=p, c=p: lib.sr_surface_reg_backward(W, H, rn, sn, 0.05, 100.0, g, a, b, c, None)
    check(reg_f(W=0), INVALID, "image size", "reg forward W")
    check(reg_f(H=0), INVALID, "image size", "reg forward H")
    for kw in ("rn", "sn", "rd", "out", "ws"):
        check(reg_f(**{kw: None}), INVALID, "NULL", "reg forward " + kw)
    check(reg_f(n=8), TOO_SMALL, "workspace", "reg forward short workspace")
    check(reg_b(W=0), INVALID, "image size", "reg backward W")
    check(reg_b(g=None), INVALID, "NULL", "reg backward g_loss")
    check(reg_b(sn=None), INVALID, "without surf_normal", "reg backward g_rend_normal without surf_normal")
    check(reg_b(rn=None), INVALID, "without rend_normal", "reg backward g_surf_normal without rend_normal")
    assert reg_b(a=None, b=None, c=None) == 0                       # nothing wanted: no error, no launch

    shr_f = lambda P=10, o=p, ws=p, n=big, out=p: lib.sr_opacity_shrink_forward(P, o, 0, ws, n, out, None)
    shr_b = lambda P=10, o=p, act=0, g=p, go=p: lib.sr_opacity_shrink_backward(P, o, act, g, go, None)
    check(shr_f(P=0), INVALID, "P", "shrink forward P")
    check(shr_b(P=-1), INVALID, "P", "shrink backward P")
    for kw in ("o", "out", "ws"):
        check(shr_f(**{kw: None}), INVALID, "NULL", "shrink forward " + kw)
    check(shr_f(P=1000, n=8), TOO_SMALL, "workspace", "shrink forward short workspace")
    check(shr_b(o=None), INVALID, "NULL", "shrink backward opacity")
    check(shr_b(g=None), INVALID, "NULL", "shrink backward g_loss")
    check(shr_b(go=None), INVALID, "NULL", "shrink backward g_opacity")


def test_workspace_size_and_exports(lib):
    assert lib.sr_aux_loss_workspace_bytes(0) == 0 and lib.sr_aux_loss_workspace_bytes(-5) == 0
    for n in (1, 255, 256, 257, 1920 * 1080, 3_000_000):
        assert lib.sr_aux_loss_workspace_bytes(n) == -(-n // ac.BLOCK) * 16, n        # a pair of float64 partial sums per workgroup
    for name in ("sr_aux_loss_workspace_bytes", "sr_semantic_ce_forward", "sr_semantic_ce_backward", "sr_surface_reg_forward",
                 "sr_surface_reg_backward", "sr_opacity_shrink_forward", "sr_opacity_shrink_backward"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    from tests.test_abi import _declared_functions
    assert sorted(_lib.EXPORTS) == _declared_functions()


def test_python_ops_refuse_cpu_tensors_and_bad_shapes():
    import streetunveiler_amd as sa
    x, lab = torch.rand(6, 4, 5), torch.zeros(4, 5, dtype=torch.int64)
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        sa.semantic_cross_entropy(x, lab)
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        sa.surface_regularisers(torch.rand(3, 4, 5), torch.rand(3, 4, 5), torch.rand(1, 4, 5), 0.05, 100.0)
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        sa.opacity_shrink(torch.rand(7, 1))
    assert sa.semantic_cross_entropy_torch is al.semantic_cross_entropy_torch and sa.SemanticCrossEntropy().weights == al.class_weights(ac.REF_WEIGHT, 6)
    with pytest.raises(ValueError, match="one value per class"):
        al.class_weights([1.0, 2.0], 6)
    assert al.class_weights(torch.tensor([1.0, 0.2]), 2) == (1.0, float(np.float32(0.2))) == al.class_weights([1.0, 0.2], 2)
    assert al.class_weights(None, 3) == (1.0, 1.0, 1.0)


def test_every_weight_tensor_gives_its_own_values():
    """Nothing is remembered about a weight TENSOR: temporaries created one after the other (the allocator hands the same address back,
    the version counter starts at 0 again), a tensor written in place and one whose `.data` is replaced all give the values they hold."""
    for i in range(200):
        assert al.class_weights(torch.full((6,), float(i)), 6) == (float(i),) * 6, i
    w = torch.tensor([1.0, 1.0, 1.0, 1.0, 0.2, 1.0])
    assert al.class_weights(w, 6) == al.class_weights(ac.REF_WEIGHT, 6)
    w[1] = 3.0
    assert al.class_weights(w, 6)[1] == 3.0
    w.data = torch.full((6,), 7.0)
    assert al.class_weights(w, 6) == (7.0,) * 6
    # an instance reads its weights when it is built, and keeps THOSE
    ce = al.SemanticCrossEntropy(torch.tensor([2.0, 4.0]))
    assert ce.weights == (2.0, 4.0) and al.SemanticCrossEntropy(torch.tensor([4.0, 2.0])).weights == (4.0, 2.0) and ce.weights == (2.0, 4.0)

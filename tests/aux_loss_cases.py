"""Cases, references and THE bar of the auxiliary losses (streetunveiler_amd/aux_loss.py, csrc/aux_loss.hip), shared by
tests/test_aux_loss_host.py, tests/test_gpu_aux_loss.py and tools/aux_loss_parity.py.

The bar (the project's own, as in tests/postprocess_cases.py and tests/tsdf_cases.py):
  truth      the `*_torch` twin -- the reference's lines -- in float64, on the CPU;
  yardstick  the same twin in float32 on the same inputs, on the CPU.  Never the code under test;
  a result passes when |result - truth| <= BAR x |yardstick - truth|, per element of a gradient and per scalar of a loss, with a floor
  of half a float32 ulp OF THE TRUE VALUE (a yardstick that happens to round exactly must not set the bar to 0; no float32 number is
  closer to a truth that sits between two of them).  BAR = 2: a different, equally valid float32 evaluation order.
  Where the truth is NaN the result must be NaN, where it is infinite the result must equal it; a yardstick that is not finite where the
  truth is contributes nothing (the floor alone).
Every case is compared in full.  The only exemptions are the two deliberate differences from torch that include/surfel_raster.h states,
and they are held to their stated behaviour: `NEG_INF_LABEL` cases (an -inf logit beside the label: finite) are held to the same bar
against the class-index form of the same loss, which gathers the label's log-probability instead of multiplying a one-hot row.

Sizes: the kernels run one pixel / Gaussian per thread in workgroups of BLOCK = 256 and the finalize workgroup has BLOCK threads, thread t
adding the partials of blocks t, t + 256, ...  So: one pixel; 3x5; 67x9 (a width that is no multiple of the 64-lane wave); 130x70 (36
blocks, the last one ragged); and BIG = 263x251 = 66013 pixels = 258 blocks, with which every finalize thread adds at least one partial
and threads 0 and 1 add two.  For the opacities: P = 1, 63, 64, 65 and 256 * 256 + 1 = 65537 (257 blocks: thread 0 adds two)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from streetunveiler_amd import aux_loss as al

BAR = 2.0
BLOCK = 256
SIZES = [(1, 1), (3, 5), (67, 9), (130, 70)]      # (W, H)
BIG = (263, 251)
assert -(-BIG[0] * BIG[1] // BLOCK) == BLOCK + 2
SHRINK_P = [1, 63, 64, 65, BLOCK * BLOCK + 1]
REF_WEIGHT = list(al.REFERENCE_CLASS_WEIGHT)
UPSTREAM = 0.75                                   # the scalar handed to every backward: exact in float32
NEG_INF_LABEL = "neg_inf_label"


# ---- the bar ---------------------------------------------------------------------------------------------------------------------------
def ulp32(truth):
    """The float32 spacing at |truth| (float64 array): 2^(e - 23), e = the exponent of truth, no smaller than the denormals' 2^-149."""
    a = np.abs(np.asarray(truth, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.where((a > 0) & np.isfinite(a), a, 1.0)))
    e = np.where(a > 0, np.maximum(e, -126.0), -126.0)
    return np.exp2(e - 23.0)


def limits(truth, yard):
    truth = np.asarray(truth, dtype=np.float64)
    d = np.abs(np.asarray(yard, dtype=np.float64) - truth)
    return np.maximum(BAR * np.where(np.isfinite(d), d, 0.0), 0.5 * ulp32(truth))


def ratio(got, truth, yard):
    """Per element: |got - truth| / limit; inf where got is not what a non-finite truth demands or is not finite where the truth is."""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = np.abs(got - truth) / limits(truth, yard)
    fin = np.isfinite(truth)
    r = np.where(fin, np.where(np.isfinite(got), r, np.inf), 0.0)
    same = np.where(np.isnan(truth), np.isnan(got), got == truth)
    return np.where(~fin & ~same, np.inf, r)


def worst(got, truth, yard):
    """{quantity: the worst ratio}; passes when every one is <= 1."""
    return {k: float(np.max(ratio(got[k], truth[k], yard[k]))) for k in truth}


def assert_within_bar(got, truth, yard, what):
    assert set(got) == set(truth) == set(yard), (what, sorted(got), sorted(truth))
    w = worst(got, truth, yard)
    print(what + ": " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    bad = {k: v for k, v in w.items() if not v <= 1.0}
    assert not bad, f"{what}: beyond {BAR} x the float32 twin's own deviation (floor: half an ulp), as a multiple of that limit: {bad}"
    return w


# ---- semantic cross-entropy ------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _labels(W, H, seed, dtype, lo=0, hi=6):
    return torch.randint(lo, hi, (H, W), generator=_gen(seed)).to(dtype)


def semantic_cases():
    cases = []

    def add(name, x, target, weight=REF_WEIGHT, kind="regular"):
        cases.append(dict(name=name, x=x.float().contiguous(), target=target, weight=weight, kind=kind))

    for k, (W, H) in enumerate(SIZES + [BIG]):     # the real regime: rendered class probabilities in [0, 1]
        add(f"unit_{W}x{H}", torch.rand(6, H, W, generator=_gen(10 + k)), _labels(W, H, 20 + k, torch.int64))
    W, H = SIZES[2]
    add("pm80_u8", 160 * torch.rand(6, H, W, generator=_gen(30)) - 80, _labels(W, H, 31, torch.uint8))
    add("pm1e4_i32", 2e4 * torch.rand(6, H, W, generator=_gen(32)) - 1e4, _labels(W, H, 33, torch.int32))
    add("pm1e4_soft", 2e4 * torch.rand(6, H, W, generator=_gen(34)) - 1e4, torch.rand(6, H, W, generator=_gen(35)))
    add("all_equal", torch.full((6, 5, 3), 0.25), _labels(3, 5, 36, torch.int64))
    W, H = SIZES[3]
    mixed = _labels(W, H, 40, torch.int64, 0, 9)                       # 0..5 and 6, 7, then 8 -> 255
    mixed[mixed == 8] = 255
    for dtype, tag in ((torch.uint8, "u8"), (torch.int32, "i32"), (torch.int64, "i64")):
        add(f"out_of_range_{tag}", torch.rand(6, H, W, generator=_gen(41)), mixed.to(dtype))
    negative = mixed.clone()
    negative[negative == 7] = -1
    add("negative_label_i32", torch.rand(6, H, W, generator=_gen(42)), negative.to(torch.int32))
    add("all_out_of_range", torch.rand(6, 9, 67, generator=_gen(43)), torch.full((9, 67), 6, dtype=torch.uint8))
    add("zero_weight", torch.rand(6, H, W, generator=_gen(44)), _labels(W, H, 45, torch.uint8), [1.0, 0.0, 2.5, 1.0, 0.2, 1.0])
    add("no_weight", torch.rand(6, H, W, generator=_gen(46)), _labels(W, H, 47, torch.int64), None)
    add("soft_unnormalised", torch.rand(6, H, W, generator=_gen(48)), 1.7 * torch.rand(6, H, W, generator=_gen(49)))
    add("soft_one_hot", torch.rand(6, H, W, generator=_gen(50)), al.one_hot_image(mixed, 6))
    add("soft_big", torch.rand(6, BIG[1], BIG[0], generator=_gen(51)), torch.rand(6, BIG[1], BIG[0], generator=_gen(52)))
    add("one_class_labels", torch.randn(1, 9, 67, generator=_gen(53)), _labels(67, 9, 54, torch.int64, 0, 2), [0.7])
    add("one_class_soft", torch.randn(1, 9, 67, generator=_gen(55)), torch.rand(1, 9, 67, generator=_gen(56)), [0.7])
    w8 = [1.0, 0.5, 2.0, 1.0, 0.2, 1.0, 3.0, 0.25]
    add("eight_classes_labels", 4 * torch.randn(8, H, W, generator=_gen(57)), _labels(W, H, 58, torch.uint8, 0, 10), w8)
    add("eight_classes_soft", 4 * torch.randn(8, H, W, generator=_gen(59)), torch.rand(8, H, W, generator=_gen(60)), w8)
    # the deliberate differences: an -inf logit beside the label (finite with labels, NaN with probabilities), a NaN logit (NaN in both)
    x = torch.rand(6, 9, 67, generator=_gen(61))
    lab = _labels(67, 9, 62, torch.int64)
    lab[4, 11] = 2
    x_inf = x.clone(); x_inf[3, 4, 11] = float("-inf")
    add("neg_inf_beside_label", x_inf, lab, kind=NEG_INF_LABEL)
    add("neg_inf_soft", x_inf, al.one_hot_image(lab, 6))
    x_nan = x.clone(); x_nan[3, 4, 11] = float("nan")
    add("nan_labels", x_nan, lab)
    add("nan_soft", x_nan, al.one_hot_image(lab, 6))
    x_nan0 = x.clone(); x_nan0[0, 0, 0] = float("nan")                  # in class 0, where a max that starts there could keep or lose it
    add("nan_first_class", x_nan0, lab)
    return cases


SEMANTIC = semantic_cases()


def class_index_loss(x, labels, weight):
    """The label form as the header states it, every label in range: -w[l] (x[l] - lse(x)) gathered, mean over the pixels."""
    logp = F.log_softmax(x, dim=0)
    lab = labels.to(torch.int64)
    w = torch.as_tensor([1.0] * x.shape[0] if weight is None else weight, dtype=torch.float32).to(x.dtype)
    return (-w[lab] * logp.gather(0, lab[None])[0]).mean()


def semantic_twin(case, dtype):
    x = case["x"].clone().to(dtype).requires_grad_()
    if case["kind"] == NEG_INF_LABEL:
        loss = class_index_loss(x, case["target"], case["weight"])
    else:
        loss = al.semantic_cross_entropy_torch(x, case["target"], case["weight"])
    (g,) = torch.autograd.grad(loss, x, torch.tensor(UPSTREAM, dtype=dtype))
    return dict(loss=loss.detach().numpy(), g_logits=g.numpy())


@functools.lru_cache(maxsize=None)
def _semantic_reference(i):
    return semantic_twin(SEMANTIC[i], torch.float64), semantic_twin(SEMANTIC[i], torch.float32)


def semantic_reference(case):
    """(truth, yardstick), computed once per case and shared."""
    return _semantic_reference(next(i for i, c in enumerate(SEMANTIC) if c is case))


def semantic_analytic(case, drop_s=False):
    """The header's statement, in float64: loss = sum of terms / N; g_x = (g / N) (softmax S - w t)."""
    x = case["x"].double()
    Cn, N = x.shape[0], x.shape[1] * x.shape[2]
    w = torch.as_tensor([1.0] * Cn if case["weight"] is None else case["weight"], dtype=torch.float32).double().reshape(-1, 1, 1)
    t = case["target"]
    t = (t if t.is_floating_point() else al.one_hot_image(t, Cn)).double()
    lse = torch.logsumexp(x, dim=0, keepdim=True)
    S = (w * t).sum(0, keepdim=True)
    loss = -(w * t * (x - lse)).sum() / N
    g = UPSTREAM / N * (torch.softmax(x, 0) * (1.0 if drop_s else S) - w * t)
    return dict(loss=loss.numpy(), g_logits=g.numpy())


def run_hip_semantic(case, dev, raw=False):
    x, target = case["x"].to(dev), case["target"].to(dev)
    if raw:
        loss = al.semantic_ce_forward(x, target, case["weight"])[0]
        g = al.semantic_ce_backward(x, target, torch.tensor(UPSTREAM, device=dev), case["weight"])
    else:
        x.requires_grad_()
        loss = al.semantic_cross_entropy(x, target, case["weight"])
        (g,) = torch.autograd.grad(loss, x, torch.tensor(UPSTREAM, device=dev))
    return dict(loss=loss.detach().cpu().numpy(), g_logits=g.cpu().numpy())


# ---- surface regularisers --------------------------------------------------------------------------------------------------------------
def _normals(W, H, seed):
    """Unit normals times a coverage in [0, 1], as rend_normal (the blend's alpha-weighted sum) and surf_normal (normal x alpha) are."""
    r = _gen(seed)
    n = F.normalize(torch.randn(3, H, W, generator=r), dim=0)
    return (n * torch.rand(1, H, W, generator=r)).contiguous()


def surface_cases():
    cases = []

    def add(name, rn, sn, rd, ln=0.05, ld=100.0):
        cases.append(dict(name=name, rend_normal=rn, surf_normal=sn, rend_dist=rd, lambda_normal=ln, lambda_dist=ld))

    for k, (W, H) in enumerate(SIZES + [BIG]):
        add(f"maps_{W}x{H}", _normals(W, H, 100 + k), _normals(W, H, 110 + k), 1e-3 * torch.rand(1, H, W, generator=_gen(120 + k)))
    W, H = SIZES[3]
    zero = torch.zeros(3, H, W)
    add("empty_pixels", zero, zero.clone(), torch.zeros(1, H, W))
    sn = _normals(W, H, 130)
    sn[:, 0, :] = 0; sn[:, -1, :] = 0; sn[:, :, 0] = 0; sn[:, :, -1] = 0      # the zero border the post-processing writes
    add("border_zeros", _normals(W, H, 131), sn, 1e-3 * torch.rand(1, H, W, generator=_gen(132)))
    add("lambda_normal_zero", _normals(W, H, 133), _normals(W, H, 134), torch.rand(1, H, W, generator=_gen(135)), 0.0, 100.0)
    add("lambda_dist_zero", _normals(W, H, 136), _normals(W, H, 137), torch.rand(1, H, W, generator=_gen(138)), 0.05, 0.0)
    add("stage_weights", _normals(W, H, 139), _normals(W, H, 140), torch.rand(1, H, W, generator=_gen(141)), 0.05, 1000.0)
    return cases


SURFACE = surface_cases()
SURFACE_GRADS = ("g_rend_normal", "g_surf_normal", "g_rend_dist")


def surface_twin(case, dtype):
    maps = [case[k].clone().to(dtype).requires_grad_() for k in ("rend_normal", "surf_normal", "rend_dist")]
    loss, normal_loss, dist_loss = al.surface_regularisers_torch(*maps, case["lambda_normal"], case["lambda_dist"])
    grads = torch.autograd.grad(loss, maps, torch.tensor(UPSTREAM, dtype=dtype))
    out = dict(loss=loss.detach().numpy(), normal_loss=normal_loss.detach().numpy(), dist_loss=dist_loss.detach().numpy())
    out.update({k: g.numpy() for k, g in zip(SURFACE_GRADS, grads)})
    return out


@functools.lru_cache(maxsize=None)
def _surface_reference(i):
    return surface_twin(SURFACE[i], torch.float64), surface_twin(SURFACE[i], torch.float32)


def surface_reference(case):
    return _surface_reference(next(i for i, c in enumerate(SURFACE) if c is case))


def surface_analytic(case, swap=False, drop_dist=False):
    rn, sn, rd = (case[k].double() for k in ("rend_normal", "surf_normal", "rend_dist"))
    ln, ld, N = case["lambda_normal"], case["lambda_dist"], rd.numel()
    normal_loss, dist_loss = ln * (1 - (rn * sn).sum(0)).mean(), ld * rd.mean()
    k = -(UPSTREAM * ln / N)
    g_rn, g_sn = (k * rn, k * sn) if swap else (k * sn, k * rn)
    return dict(loss=(normal_loss if drop_dist else normal_loss + dist_loss).numpy(), normal_loss=normal_loss.numpy(), dist_loss=dist_loss.numpy(),
                g_rend_normal=g_rn.numpy(), g_surf_normal=g_sn.numpy(), g_rend_dist=torch.full_like(rd, UPSTREAM * ld / N).numpy())


def run_hip_surface(case, dev, raw=False, want=(True, True, True)):
    """The results that `want` asks for; a gradient that is not wanted must come back None."""
    maps = [case[k].to(dev) for k in ("rend_normal", "surf_normal", "rend_dist")]
    ln, ld = case["lambda_normal"], case["lambda_dist"]
    if raw:
        out = al.surface_reg_forward(*maps, ln, ld)
        grads = al.surface_reg_backward(*maps, ln, ld, torch.tensor(UPSTREAM, device=dev), want=want)
    else:
        for m, w in zip(maps, want):
            m.requires_grad_(w)
        out = al.surface_regularisers(*maps, ln, ld)
        assert out[0].requires_grad == any(want) and not out[1].requires_grad and not out[2].requires_grad
        wanted = [m for m, w in zip(maps, want) if w]
        got = iter(torch.autograd.grad(out[0], wanted, torch.tensor(UPSTREAM, device=dev)) if wanted else ())
        grads = [next(got) if w else None for w in want]
    res = dict(loss=out[0].detach().cpu().numpy(), normal_loss=out[1].detach().cpu().numpy(), dist_loss=out[2].detach().cpu().numpy())
    for k, g, w in zip(SURFACE_GRADS, grads, want):
        assert (g is not None) == bool(w), k
        if w:
            res[k] = g.cpu().numpy()
    return res


# ---- opacity shrink --------------------------------------------------------------------------------------------------------------------
def shrink_cases():
    cases = []
    for k, P in enumerate(SHRINK_P):
        cases.append(dict(name=f"raw_{P}", opacity=4 * torch.randn(P, 1, generator=_gen(200 + k)), activated=False))
    sat = torch.tensor([100.0, -100.0, 0.0, 30.0, -30.0, 88.0, -88.0, -104.0, 17.0]).repeat(29)[:, None].contiguous()
    cases.append(dict(name="saturated", opacity=sat, activated=False))
    cases.append(dict(name="minus_100_alone", opacity=torch.full((65, 1), -100.0), activated=False))
    for k, P in enumerate((65, BLOCK * BLOCK + 1)):
        cases.append(dict(name=f"activated_{P}", opacity=torch.rand(P, 1, generator=_gen(210 + k)), activated=True))
    return cases


SHRINK = shrink_cases()


def shrink_twin(case, dtype):
    o = case["opacity"].clone().to(dtype).requires_grad_()
    loss = al.opacity_shrink_torch(o, case["activated"])
    (g,) = torch.autograd.grad(loss, o, torch.tensor(UPSTREAM, dtype=dtype))
    return dict(loss=loss.detach().numpy(), g_opacity=g.numpy())


@functools.lru_cache(maxsize=None)
def _shrink_reference(i):
    return shrink_twin(SHRINK[i], torch.float64), shrink_twin(SHRINK[i], torch.float32)


def shrink_reference(case):
    return _shrink_reference(next(i for i, c in enumerate(SHRINK) if c is case))


def shrink_analytic(case, plain_s=False):
    o = case["opacity"].double()
    P = o.numel()
    if case["activated"]:
        return dict(loss=o.mean().numpy(), g_opacity=torch.full_like(o, UPSTREAM / P).numpy())
    s = torch.sigmoid(o)
    return dict(loss=s.mean().numpy(), g_opacity=(UPSTREAM / P * (s if plain_s else s * (1 - s))).numpy())


def run_hip_shrink(case, dev, raw=False):
    o = case["opacity"].to(dev)
    if raw:
        loss = al.opacity_shrink_forward(o, case["activated"])[0]
        g = al.opacity_shrink_backward(o, torch.tensor(UPSTREAM, device=dev), case["activated"])
    else:
        o.requires_grad_()
        loss = al.opacity_shrink(o, case["activated"])
        (g,) = torch.autograd.grad(loss, o, torch.tensor(UPSTREAM, device=dev))
    return dict(loss=loss.detach().cpu().numpy(), g_opacity=g.cpu().numpy())


def as_float32(res):
    """A float64 restatement as a float32 implementation would hand it back: every value rounded once."""
    return {k: np.asarray(v, dtype=np.float64).astype(np.float32) for k, v in res.items()}

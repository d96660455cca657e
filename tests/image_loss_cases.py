"""Shared by tests/test_image_loss_golden.py, tests/test_image_loss_host.py, tests/test_gpu_image_loss.py and tools/image_loss_parity.py:
the fixture cases of tests/golden/image_loss_golden.npz (tools/make_image_loss_golden.py: the reference's own python), seeded cases of any
size, THE BAR, and (second half of the file) the per-element bar with the EDGE_CASES it is applied to.

The bar is a ratio against the reference's own rounding noise, per case and per quantity:
    scalars (loss, l1, ssim):  d = |value - truth|
    gradients:                 d = max|value - truth| / max|truth|
    d_ref = the same deviation of the reference's float32 run on the case (fixture: the stored run; other sizes: photometric_loss_torch
            in float32 on the CPU), truth = the float64 run
    ratio = d / max(d_ref, 1e-6 * scale)  <=  4          (scale = |truth| for a scalar, 1 for the already relative gradient figure)
4x because the kernels sum the window separably, in another order and with contraction (a separable float32 evaluation on the CPU sits at
0.3-0.6 x d_ref); a wrong or dropped term shows up at 1e-2 or more, thousands of times the bar."""
import functools
import os

import numpy as np
import torch

from streetunveiler_amd.image_loss import photometric_loss, photometric_loss_torch

BAR = 4.0
FLOOR = 1e-6
SCALARS = ("loss", "l1", "ssim")
GRADS = ("g_image", "g_sky", "g_alpha")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_loss_golden.npz")
# (W, H) of the GPU-only cases: one pixel, frames narrower / lower than the window, a size that is no multiple of the tile, the `-r 4`
# frame and the full frame
GPU_SIZES = ((1, 1), (5, 300), (300, 5), (129, 257), (480, 320), (1920, 1080))


def fixture_cases():
    """[{name, lambda_dssim, image, gt, sky, alpha (float32 tensors or None), ref: {...}, truth: {...} (numpy)}]"""
    z = np.load(GOLDEN)
    out = []
    for name in z["names"]:
        pre = str(name) + "/"
        t = lambda k: torch.tensor(z[pre + k]) if pre + k in z.files else None
        case = dict(name=str(name), lambda_dssim=float(z[pre + "lambda_dssim"]), image=t("image"), gt=t("gt"), sky=t("sky"), alpha=t("alpha"))
        for tag in ("ref", "truth"):
            case[tag] = {k: np.asarray(z[pre + tag + "_" + k], dtype=np.float64) for k in SCALARS + GRADS if pre + tag + "_" + k in z.files}
        out.append(case)
    return out


def seeded_case(W, H, composite, channels=3, lambda_dssim=0.2, seed=0):
    """A noisy image against its clean target (and a sky behind a soft alpha), float32 on the CPU; ref / truth not yet filled."""
    r = torch.Generator().manual_seed(1000003 * seed + 7919 * W + H + (1 if composite else 0))
    u = lambda c: torch.rand(c, H, W, generator=r)
    gt = u(channels)
    image = (gt + 0.1 * torch.randn(channels, H, W, generator=r)).clamp(0, 1)
    sky = alpha = None
    if composite:
        sky, alpha = u(channels), u(1)
        image = image * alpha
    return dict(name=f"seeded_{W}x{H}" + ("_sky" if composite else ""), lambda_dssim=lambda_dssim, image=image, gt=gt, sky=sky, alpha=alpha)


def _collect(case, outs, leaves, g_loss=None):
    loss, l1, ssim = outs
    grads = torch.autograd.grad(loss, leaves, None if g_loss is None else torch.tensor(g_loss, dtype=loss.dtype, device=loss.device))
    res = dict(loss=loss, l1=l1, ssim=ssim, g_image=grads[0])
    if case["sky"] is not None:
        res["g_sky"], res["g_alpha"] = grads[1], grads[2]
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


def _leaves(case, dtype, device):
    prep = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype, copy=True).requires_grad_()
    image, sky, alpha = prep(case["image"]), prep(case["sky"]), prep(case["alpha"])
    return image, case["gt"].to(device=device, dtype=dtype), sky, alpha, [t for t in (image, sky, alpha) if t is not None]


def run_torch(case, dtype, device="cpu", g_loss=None):
    """photometric_loss_torch and its autograd gradients (under the upstream scalar g_loss, 1 if None) -> {quantity: float64 numpy}"""
    image, gt, sky, alpha, leaves = _leaves(case, dtype, device)
    return _collect(case, photometric_loss_torch(image, gt, case["lambda_dssim"], sky, alpha), leaves, g_loss)


def run_hip(case, device="cuda:0", g_loss=None):
    """photometric_loss (the HIP kernels) and its gradients -> {quantity: float64 numpy}"""
    image, gt, sky, alpha, leaves = _leaves(case, torch.float32, device)
    return _collect(case, photometric_loss(image, gt, case["lambda_dssim"], sky, alpha), leaves, g_loss)


def with_cpu_reference(case):
    """Fills ref (float32) and truth (float64) of a seeded case with photometric_loss_torch on the CPU."""
    case["ref"], case["truth"] = run_torch(case, torch.float32), run_torch(case, torch.float64)
    return case


def deviation(value, truth, key):
    d = float(np.abs(np.asarray(value, dtype=np.float64) - truth).max())
    return d if key in SCALARS else d / float(np.abs(truth).max())


def ratios(got, case):
    """{quantity: deviation of `got` from the truth over max(d_ref, floor)}: the figure the bar bounds by 4."""
    out = {}
    for key, truth in case["truth"].items():
        scale = abs(float(truth)) if key in SCALARS else 1.0
        d_ref = deviation(case["ref"][key], truth, key)
        out[key] = deviation(got[key], truth, key) / max(d_ref, FLOOR * scale)
    return out


def assert_within_bar(got, case, what):
    r = ratios(got, case)
    print(f"{what} {case['name']}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= BAR}
    assert not bad, f"{what}, case {case['name']}: beyond {BAR} x the reference's own float32 deviation: {bad}"
    return r


# ---- the per-element bar and the edge cases ----------------------------------------------------------------------------------------------
# Beside the rule above, which keeps its meaning for the fixture and the GPU_SIZES cases.  Per gradient tensor, after the precedent of
# tests/postprocess_cases.py:
#     e_i = |v_i - truth_i| / (|truth_i| + u),   u = |g_loss| / (C*H*W)
#     max(e) and the 99.9th percentile of e, over the elements where the float64 truth is finite,
#         <=  BAR * max(the float32 twin's same statistic on the same case, FLOOR)
# u is derived, not measured: every element's L1 term is 0 or +-(1 - lambda) * g / N and its SSIM term is O(lambda * g / N), so g / N is the
# natural size of one gradient element whatever the content.  It stays meaningful where the truth cancels to 1e-17 (image == gt) or is
# exactly zero, where max|v - truth| / max|truth| is 1e9 or a division by zero, and it is per element, so an error confined to a tile seam
# cannot ride under a larger deviation elsewhere.  A tensor whose truth is identically zero must be zero in every element (either sign).
# The twin is photometric_loss_torch in float32 on the CPU, never the code under test.
#
# Scalars keep the rule above, d <= BAR * max(d_ref, FLOOR * |truth|), with one addition where that rule has no unit: when the loss has
# cancelled below FLOOR times the size of its own terms, |loss| < FLOOR * s with s = (1 - lambda) * |l1| + lambda * |ssim| (all black, or
# image == gt: l1 = 0 and ssim = 1 to rounding, the truth is 0 or 1e-17 and a twin that happens to land on it leaves d_ref = 0), |truth| is
# replaced by s: loss is computed FROM l1 and ssim and inherits their float32 rounding, FLOOR relative to each.  No case with content
# comes near that condition (loss / s is 0.1 .. 1 there).  A scalar whose truth is NaN must be NaN.
# Measured on an MI355X (profiles/image_loss_parity.json): the kernels' largest per-element ratio is 2.47, g_alpha of the 1025-channel composite
# (one float32 sum over 1025 channels in channel order); image == gt sits at 2.0 .. 2.3, every other case at or under 1.0, and the all-black loss, one float32 ulp of ssim off
# its truth of exactly 0, sits at 0.12 of the unit its terms give it.

# csrc/image_loss.hip: kLossTW x kLossTH pixel tiles, a halo of kLossR, at most kLossMaxBlocks forward workgroups.  The sizes of EDGE_CASES
# are built from these four; tests/test_image_loss_host.py compares them with the kernel source, so a change there makes the table stale.
TILE_W, TILE_H, HALO, MAX_BLOCKS = 32, 16, 5, 4096
STATS = ("max", "p999")
SEAM_SIZES = ((TILE_W - 1, TILE_H - 1), (TILE_W, TILE_H), (TILE_W + 1, TILE_H + 1), (2 * TILE_W + 1, 2 * TILE_H + 1),
              (4, 4), (HALO, 2 * HALO + 1), (2 * HALO + 1, HALO))       # ..., and frames no larger than the 11 x 11 window
ONE = (TILE_W + 1, TILE_H + 1)            # 33 x 17: 2 x 2 tiles, the second of each one pixel wide
TWO = (2 * TILE_W + 1, 2 * TILE_H + 1)    # 65 x 33: 3 x 3 tiles, a full tile in the middle
WALK_CHANNELS = MAX_BLOCKS // 4 + 1       # 33 x 17 x 1025: 4 tiles per channel, 4100 tiles: 4 workgroups take a second tile, in another channel
NAN_AT = (1, TILE_H, TILE_W)              # (c, y, x): the first pixel of the middle tile of 65 x 33; its 21 x 21 footprint lies on four tiles


def _edge_table():
    """{name: (W, H, channels, composite, lambda_dssim, content)}"""
    t = {}
    sky = lambda composite: "_sky" if composite else ""
    for W, H in SEAM_SIZES:
        for comp in (False, True):
            t[f"seam_{W}x{H}{sky(comp)}"] = (W, H, 3, comp, 0.2, "noise")
    for Cn in (1, 2, 6):
        for comp in (False, True):
            t[f"chan{Cn}_{ONE[0]}x{ONE[1]}{sky(comp)}"] = (*ONE, Cn, comp, 0.2, "noise")
    for comp in (False, True):
        t[f"walk_{ONE[0]}x{ONE[1]}_c{WALK_CHANNELS}{sky(comp)}"] = (*ONE, WALK_CHANNELS, comp, 0.2, "noise")
    t[f"walk_1x1_c{MAX_BLOCKS + 1}"] = (1, 1, MAX_BLOCKS + 1, False, 0.2, "noise")
    for lam, tag in ((0.0, "0"), (1.0, "1"), (0.2, "02")):
        t[f"lam{tag}_{ONE[0]}x{ONE[1]}_sky"] = (*ONE, 3, True, lam, "noise")
    for W, H in (ONE, TWO):
        t[f"half_{W}x{H}"] = (W, H, 3, False, 0.2, "half")                       # image == gt == 0.5
        t[f"black_{W}x{H}_sky"] = (W, H, 3, True, 0.2, "black")                   # everything black: every gradient is exactly zero
        t[f"equal_patch_{W}x{H}"] = (W, H, 3, False, 0.2, "equal_patch")          # noise with x == gt on a patch across the seams
        t[f"alpha_patches_{W}x{H}_sky"] = (W, H, 3, True, 0.2, "alpha_patches")   # alpha exactly 0 and exactly 1 across the seams
        t[f"step_{W}x{H}"] = (W, H, 1, False, 0.5, "step")                        # the fixture's flat-step regime, at a seam
        t[f"wide_{W}x{H}_sky"] = (W, H, 3, True, 0.2, "wide")                     # values in [-50, 50]: an unclamped render
    for comp in (False, True):
        t[f"nan_{TWO[0]}x{TWO[1]}{sky(comp)}"] = (*TWO, 3, comp, 0.2, "nan")
    return t


EDGE_CASES = _edge_table()
G_LOSS_CASE = f"seam_{ONE[0]}x{ONE[1]}_sky"      # the 33 x 17 composite with C = 3: upstream scalars, the wrapper's conversions


def edge_input(name):
    """The inputs of one edge case (float32 on the CPU), ref / truth not filled."""
    W, H, Cn, comp, lam, content = EDGE_CASES[name]
    case = seeded_case(W, H, comp, channels=Cn, lambda_dssim=lam, seed=11)
    case["name"] = name
    r = torch.Generator().manual_seed(424243 + 7919 * W + H)
    ys, xs = slice(max(TILE_H - 3, 0), TILE_H + 3), slice(max(TILE_W - 3, 0), TILE_W + 3)     # up to 6 x 6 across both seams, clipped to the frame
    if content == "half":
        case["image"], case["gt"] = torch.full((Cn, H, W), 0.5), torch.full((Cn, H, W), 0.5)
    elif content == "black":
        case["image"], case["gt"], case["sky"] = torch.zeros(Cn, H, W), torch.zeros(Cn, H, W), torch.zeros(Cn, H, W)
    elif content == "equal_patch":
        case["image"][:, ys, xs] = case["gt"][:, ys, xs]
    elif content == "alpha_patches":
        case["alpha"][:, ys, max(TILE_W - 4, 0):TILE_W + 2] = 0.0
        case["alpha"][:, max(TILE_H - 2, 0):TILE_H + 2, TILE_W // 4:TILE_W // 2] = 1.0
        case["alpha"][:, 2:6, xs] = 1.0
    elif content == "step":
        flat = torch.full((Cn, H, W), 0.25)
        flat[:, :, W // 2:] = 0.75                  # 65 x 33: the step is the seam at column 32
        flat[:, TILE_H:, :W // 4] = 0.5
        case["image"] = flat + 1e-3 * torch.randn(Cn, H, W, generator=r)
        case["gt"] = flat + 1e-3 * torch.randn(Cn, H, W, generator=r)
    elif content == "wide":
        wide = lambda c: torch.rand(c, H, W, generator=r) * 100.0 - 50.0
        case["gt"], case["sky"] = wide(Cn), wide(Cn)
        case["image"] = (case["gt"] + 5.0 * torch.randn(Cn, H, W, generator=r)).clamp(-50.0, 50.0) * case["alpha"]
    elif content == "nan":
        case["image"][NAN_AT] = float("nan")
    else:
        assert content == "noise", content
    return case


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """One edge case with its float64 truth and its float32 twin; computed once per process, shared, never written to."""
    return with_cpu_reference(edge_input(name))


def with_upstream(case, g_loss):
    """The same case under another upstream scalar: truth = g_loss x the truth's gradients, ref = the float32 twin run with that g_loss."""
    ref = run_torch(case, torch.float32, g_loss=g_loss)
    truth = {k: (v if k in SCALARS else g_loss * v) for k, v in case["truth"].items()}
    return dict(case, name=f"{case['name']}_g{g_loss}", ref=ref, truth=truth, g_loss=g_loss)


def unit(case):
    """u = |g_loss| / (C*H*W)"""
    return abs(case.get("g_loss", 1.0)) / case["image"].numel()


def element_stats(value, truth, u):
    """One gradient tensor -> dict(max, p999 of e over the elements with a finite truth; zero: the truth is identically zero there;
    exact_zero: so is the value; same_nonfinite: the value is non-finite exactly where the truth is)."""
    value, truth = np.asarray(value, dtype=np.float64).ravel(), np.asarray(truth, dtype=np.float64).ravel()
    fin = np.isfinite(truth)
    v, t = value[fin], truth[fin]
    zero = not t.any()
    out = dict(zero=zero, exact_zero=bool((v == 0).all()), same_nonfinite=bool(np.array_equal(~np.isfinite(value), ~fin)), max=0.0, p999=0.0)
    if not zero and v.size:
        with np.errstate(invalid="ignore"):
            e = np.abs(v - t) / (np.abs(t) + u)
        e = np.where(np.isfinite(e), e, np.inf)         # a non-finite value where the truth is finite is infinitely wrong
        out["max"], out["p999"] = float(e.max()), float(np.percentile(e, 99.9))
    return out


def scalar_limit(case, key):
    """(d_ref, the unit BAR multiplies) of loss, l1 or ssim: the rule at the top of this file, and the cancelled loss's unit from its terms."""
    truth = float(case["truth"][key])
    scale = abs(truth)
    if key == "loss":
        lam = case["lambda_dssim"]
        terms = (1.0 - lam) * abs(float(case["truth"]["l1"])) + lam * abs(float(case["truth"]["ssim"]))
        if scale < FLOOR * terms:
            scale = terms
    d_ref = abs(float(case["ref"][key]) - truth)
    return d_ref, max(d_ref, FLOOR * scale)


def edge_ratios(got, case):
    """{scalar: ratio, gradient: {max: ratio, p999: ratio}}: what the per-element bar bounds by BAR.  None where no ratio exists (a NaN
    scalar, a tensor whose truth is identically zero: edge_violations judges those)."""
    out, u = {}, unit(case)
    for key, truth in case["truth"].items():
        if key in SCALARS:
            if not np.isfinite(truth):
                out[key] = None
                continue
            d, lim = abs(float(got[key]) - float(truth)), scalar_limit(case, key)[1]
            out[key] = 0.0 if d == 0 else (d / lim if lim > 0 else float("inf"))     # lim == 0: truth and twin exactly 0 (l1 of a black pair)
        else:
            s, sr = element_stats(got[key], truth, u), element_stats(case["ref"][key], truth, u)
            out[key] = None if s["zero"] else {n: s[n] / max(sr[n], FLOOR) for n in STATS}
    return out


def edge_violations(got, case):
    """[(quantity, what, value, limit)] of everything beyond the per-element bar; empty when `got` passes."""
    bad, r, u = [], edge_ratios(got, case), unit(case)
    for key, truth in case["truth"].items():
        if key in SCALARS:
            if not np.isfinite(truth):
                if not np.isnan(float(got[key])):
                    bad.append((key, "NaN like the truth", float(got[key]), float("nan")))
            elif not r[key] <= BAR:
                bad.append((key, "ratio", r[key], BAR))
            continue
        s = element_stats(got[key], truth, u)
        if not s["same_nonfinite"]:
            bad.append((key, "non-finite exactly where the truth is", float("nan"), 0.0))
        if s["zero"]:
            if not s["exact_zero"]:
                bad.append((key, "exactly zero", float(np.abs(np.nan_to_num(got[key])).max()), 0.0))
            continue
        bad += [(key, n, r[key][n], BAR) for n in STATS if not r[key][n] <= BAR]
    return bad


def assert_within_edge_bar(got, case, what):
    r = edge_ratios(got, case)
    fmt = lambda v: "-" if v is None else (f"{v:.3f}" if not isinstance(v, dict) else "/".join(f"{v[n]:.3f}" for n in STATS))
    print(f"{what} {case['name']} (per element): " + ", ".join(f"{k} {fmt(v)}" for k, v in r.items()))
    bad = edge_violations(got, case)
    assert not bad, f"{what}, case {case['name']}: beyond {BAR} x max(the float32 twin's own figure, {FLOOR}): {bad}"
    return r


def where_the_old_rule_applies(got, case):
    """(got, case) cut down to the quantities the max-norm rule at the top can judge: a finite truth with max|truth| > 0; a tensor with
    non-finite truth elements (the NaN case) is judged on the others."""
    g, c = {}, dict(case, truth={}, ref={})
    for key, truth in case["truth"].items():
        fin = np.isfinite(truth)
        if key in SCALARS:
            if not fin or float(truth) == 0.0:
                continue
            g[key], c["truth"][key], c["ref"][key] = got[key], truth, case["ref"][key]
        elif fin.any() and np.abs(truth[fin]).max() > 0 and np.isfinite(np.asarray(got[key])[fin]).all():
            g[key], c["truth"][key], c["ref"][key] = np.asarray(got[key])[fin], truth[fin], case["ref"][key][fin]
    return g, c

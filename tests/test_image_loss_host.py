"""CPU: the per-element bar of tests/image_loss_cases.py has teeth, and its edge cases are what the GPU tests assume.

  * the table's sizes are built from the kernel's own constants (read from csrc/image_loss.hip), and it holds every case it promises;
  * the float32 twin stays inside its own unit on every edge case, and no truth element is non-finite outside the NaN cases;
  * the NaN cases: which elements of which outputs of the float64 checker are non-finite -- what the GPU test then demands of the kernels;
  * twelve subtly wrong losses, each evaluated in float64 so that only the mistake is measured, are each rejected on a case named here;
  * what the earlier max-norm rule says about a backward halo that is one short, on the fixture's flat-step content."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from streetunveiler_amd.image_loss import SSIM_C1, SSIM_C2, WINDOW_SIGMA, WINDOW_SIZE, _window
from tests import image_loss_cases as ilc

NAMES = tuple(ilc.EDGE_CASES)
NAN_NAMES = tuple(n for n in NAMES if ilc.EDGE_CASES[n][5] == "nan")
ONE, TWO = "%dx%d" % ilc.ONE, "%dx%d" % ilc.TWO

# mutant -> the edge case on which the per-element bar must reject it
MUTANTS = {"window_renormalised_at_the_border": f"seam_{ONE}",
           "reflect_padding": f"seam_{ONE}",
           "outer_taps_dropped": f"seam_{TWO}",
           "outer_taps_dropped_at_the_tile_edges": f"seam_{TWO}_sky",
           "c1_and_c2_swapped": f"seam_{ONE}",
           "sign_of_zero_is_plus_one": f"equal_patch_{ONE}",
           "means_over_one_channel": f"chan2_{ONE}",
           "alpha_for_one_minus_alpha": f"alpha_patches_{ONE}_sky",
           "g_sky_without_one_minus_alpha": f"alpha_patches_{ONE}_sky",
           "g_alpha_from_channel_0": f"chan2_{ONE}_sky",
           "g_alpha_sign": f"seam_4x4_sky",
           "last_tile_missing_from_the_sums": f"walk_1x1_c{ilc.MAX_BLOCKS + 1}"}


class _Blur(torch.autograd.Function):
    """The zero-padded window; its backward (the same convolution: the window is symmetric) drops the two outermost taps where `short`."""
    @staticmethod
    def forward(ctx, t, w, w_short, short):
        ctx.save_for_backward(w, w_short, short)
        return F.conv2d(t, w, padding=WINDOW_SIZE // 2, groups=t.shape[-3])

    @staticmethod
    def backward(ctx, g):
        w, w_short, short = ctx.saved_tensors
        conv = lambda k: F.conv2d(g, k, padding=WINDOW_SIZE // 2, groups=g.shape[-3])
        return torch.where(short, conv(w_short), conv(w)), None, None, None


def evaluate(case, mutant=None):
    """The loss of streetunveiler_amd.image_loss.photometric_loss_torch and its gradients in float64, with one mistake switched on by
    `mutant` -> {quantity: float64 numpy}.  The gradients are formed as the kernels form them, from dL/dx of the composite x."""
    d = lambda t: None if t is None else t.double()
    image, gt, sky, alpha = d(case["image"]), d(case["gt"]), d(case["sky"]), d(case["alpha"])
    lam, (Cn, H, W) = case["lambda_dssim"], image.shape
    composite = sky is not None
    keep = (alpha if mutant == "alpha_for_one_minus_alpha" else 1 - alpha) if composite else None
    x = (image + sky * keep if composite else image).clone().requires_grad_()
    w = _window(Cn, torch.float64, "cpu")
    w_short = w.clone()
    w_short[:, :, (0, -1), :] = 0.0
    w_short[:, :, :, (0, -1)] = 0.0
    pad = WINDOW_SIZE // 2
    if mutant == "outer_taps_dropped":
        w = w_short
    if mutant == "reflect_padding":
        blur = lambda t: F.conv2d(F.pad(t[None], (pad,) * 4, mode="reflect")[0], w, groups=Cn)
    elif mutant == "window_renormalised_at_the_border":
        norm = F.conv2d(torch.ones_like(gt), w, padding=pad, groups=Cn)
        blur = lambda t: F.conv2d(t, w, padding=pad, groups=Cn) / norm
    elif mutant == "outer_taps_dropped_at_the_tile_edges":
        xs, ys = torch.arange(W) % ilc.TILE_W, torch.arange(H) % ilc.TILE_H
        short = (((xs == 0) | (xs == ilc.TILE_W - 1))[None, :] | ((ys == 0) | (ys == ilc.TILE_H - 1))[:, None]).expand(Cn, H, W)
        blur = lambda t: _Blur.apply(t, w, w_short, short)
    elif mutant == "adjoint_written_out":       # no mistake: _Blur with nothing marked short must be the truth
        blur = lambda t: _Blur.apply(t, w, w_short, torch.zeros(Cn, H, W, dtype=torch.bool))
    else:
        blur = lambda t: F.conv2d(t, w, padding=pad, groups=Cn)
    c1, c2 = (SSIM_C2, SSIM_C1) if mutant == "c1_and_c2_swapped" else (SSIM_C1, SSIM_C2)
    mu1, mu2 = blur(x), blur(gt)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(x * x) - mu1_sq, blur(gt * gt) - mu2_sq, blur(x * gt) - mu12
    ssim_map = ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))
    absdiff = (x - gt).abs()
    n = H * W if mutant == "means_over_one_channel" else Cn * H * W
    sum_l1, sum_ssim = absdiff.sum(), ssim_map.sum()
    if mutant == "last_tile_missing_from_the_sums":      # tile index C * tiles - 1: the last channel's last tile
        ty, tx = (H - 1) // ilc.TILE_H * ilc.TILE_H, (W - 1) // ilc.TILE_W * ilc.TILE_W
        sum_l1, sum_ssim = sum_l1 - absdiff[-1, ty:, tx:].sum().detach(), sum_ssim - ssim_map[-1, ty:, tx:].sum().detach()
    l1, ssim = sum_l1 / n, sum_ssim / n
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    g_x = torch.autograd.grad(loss, x)[0]
    if mutant == "sign_of_zero_is_plus_one":
        g_x = g_x + (1.0 - lam) / n * (x.detach() == gt)
    res = dict(loss=loss, l1=l1, ssim=ssim, g_image=g_x)
    if composite:
        res["g_sky"] = g_x if mutant == "g_sky_without_one_minus_alpha" else keep * g_x
        chain = sky * g_x
        g_alpha = -(chain[:1] if mutant == "g_alpha_from_channel_0" else chain.sum(0, keepdim=True))
        if mutant in ("g_alpha_sign", "alpha_for_one_minus_alpha"):      # (the latter: d(alpha)/d(alpha) = +1, the mutant's own chain)
            g_alpha = -g_alpha
        res["g_alpha"] = g_alpha
    return {k: v.detach().numpy() for k, v in res.items()}


def test_the_table_is_built_from_the_kernel_constants():
    src = open(os.path.join(os.path.dirname(os.path.abspath(ilc.__file__)), "..", "streetunveiler_amd", "csrc", "image_loss.hip")).read()
    const = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, src).group(1))
    assert (const("kLossTW"), const("kLossTH"), const("kLossR"), const("kLossMaxBlocks")) == (ilc.TILE_W, ilc.TILE_H, ilc.HALO, ilc.MAX_BLOCKS)
    assert 2 * ilc.HALO + 1 == WINDOW_SIZE and WINDOW_SIGMA == 1.5
    tiles = lambda W, H, Cn: -(-W // ilc.TILE_W) * -(-H // ilc.TILE_H) * Cn
    shape = lambda n: ilc.EDGE_CASES[n][:3]
    walk = [n for n in NAMES if n.startswith("walk_")]
    assert sorted(tiles(*shape(n)) - ilc.MAX_BLOCKS for n in walk) == [1, 4, 4]          # a second trip for 1 and for 4 workgroups
    assert {ilc.EDGE_CASES[n][3] for n in walk if shape(n)[0] > 1} == {False, True}
    assert all(tiles(*shape(n)) <= ilc.MAX_BLOCKS for n in NAMES if n not in walk)
    assert {shape(n)[:2] for n in NAMES if n.startswith("seam_")} == {(31, 15), (32, 16), (33, 17), (65, 33), (4, 4), (5, 11), (11, 5)}
    assert {shape(n)[2] for n in NAMES if n.startswith("chan")} == {1, 2, 6}
    assert {ilc.EDGE_CASES[n][4] for n in NAMES if n.startswith("lam")} == {0.0, 0.2, 1.0}
    assert len(NAN_NAMES) == 2 and ilc.EDGE_CASES[ilc.G_LOSS_CASE] == (33, 17, 3, True, 0.2, "noise")
    for n in NAMES:                                                                       # a few thousand to a few hundred thousand elements
        W, H, Cn = shape(n)
        assert W * H * Cn <= 600_000, n


def test_planted_content_is_where_the_table_says():
    for size in (ONE, TWO):
        c = ilc.edge_input(f"equal_patch_{size}")
        eq = (c["image"] == c["gt"]).all(0)
        assert eq[ilc.TILE_H - 1, ilc.TILE_W - 1] and eq[ilc.TILE_H, ilc.TILE_W] and 0 < int(eq.sum()) <= 36 + 8      # both sides of both seams
        a = ilc.edge_input(f"alpha_patches_{size}_sky")["alpha"][0]
        for v in (0.0, 1.0):
            on = a == v
            assert on[:, ilc.TILE_W - 1].any() and on[:, ilc.TILE_W].any(), (size, v)
        wide = ilc.edge_input(f"wide_{size}_sky")
        assert float(wide["gt"].min()) < -45 and float(wide["gt"].max()) > 45 and float(wide["sky"].abs().max()) > 45
        black = ilc.edge_case(f"black_{size}_sky")
        assert all(not black["truth"][k].any() for k in ilc.GRADS) and float(black["truth"]["loss"]) == 0.0 and float(black["truth"]["ssim"]) == 1.0
        half = ilc.edge_case(f"half_{size}")
        assert float(np.abs(half["truth"]["g_image"]).max()) < 1e-9 * ilc.unit(half)      # the truth cancels: the case the old rule cannot hold
    c = ilc.edge_input(NAN_NAMES[0])
    assert int(torch.isnan(c["image"]).sum()) == 1 and bool(torch.isnan(c["image"][ilc.NAN_AT]))


@pytest.mark.parametrize("name", NAMES)
def test_twin_is_within_its_own_unit_and_the_truth_is_finite(name):
    case = ilc.edge_case(name)
    assert not ilc.edge_violations(case["ref"], case), name
    for k, v in ilc.edge_ratios(case["ref"], case).items():        # the twin against itself: ratio <= 1 by construction
        for r in ([] if v is None else (list(v.values()) if isinstance(v, dict) else [v])):
            assert r <= 1.0, (name, k, v)
    if name not in NAN_NAMES:
        for k, v in case["truth"].items():
            assert np.isfinite(v).all(), (name, k)
            assert np.isfinite(case["ref"][k]).all(), (name, k)
        got = evaluate(case)                                      # the evaluator the mutants are cut from, unmutated: the truth to rounding
        for k in ilc.GRADS:
            if k in got:
                assert ilc.element_stats(got[k], case["truth"][k], ilc.unit(case))["max"] <= 1e-9, (name, k)
        for k in ilc.SCALARS:
            assert abs(float(got[k]) - float(case["truth"][k])) <= 1e-12 * max(1.0, abs(float(case["truth"][k]))), (name, k)


@pytest.mark.parametrize("name", NAN_NAMES)
def test_nan_case_nonfinite_set_of_the_checker(name):
    """One NaN pixel in channel 1: loss, l1 and ssim are NaN; g_image (and g_sky) are NaN on the 21 x 21 neighbourhood of the pixel in
    channel 1 and finite elsewhere; g_alpha is NaN on the same footprint.  Taken from the float64 checker, and the float32 twin agrees."""
    case = ilc.edge_case(name)
    c, y, x = ilc.NAN_AT
    r = 2 * ilc.HALO
    foot = np.zeros(case["truth"]["g_image"].shape, dtype=bool)
    foot[c, y - r:y + r + 1, x - r:x + r + 1] = True
    assert foot.sum() == 21 * 21                                   # the footprint is clear of the border
    for run in (case["truth"], case["ref"]):
        for k in ilc.SCALARS:
            assert np.isnan(run[k]), (name, k)
        np.testing.assert_array_equal(~np.isfinite(run["g_image"]), foot)
        assert np.isnan(run["g_image"][foot]).all()
        if "g_sky" in run:
            np.testing.assert_array_equal(~np.isfinite(run["g_sky"]), foot)
            np.testing.assert_array_equal(~np.isfinite(run["g_alpha"]), foot[c:c + 1])


HALO_FRAME = "%dx%d" % (ilc.HALO, 2 * ilc.HALO + 1)


def test_evaluator_with_its_adjoint_written_out_is_the_truth():
    for name in (f"seam_{TWO}_sky", f"seam_{HALO_FRAME}"):
        case = ilc.edge_case(name)
        got = evaluate(case, "adjoint_written_out")
        assert not ilc.edge_violations(got, case)
        assert ilc.element_stats(got["g_image"], case["truth"]["g_image"], ilc.unit(case))["max"] <= 1e-9


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bar_rejects_mutant(mutant):
    """Each wrong loss, in float64, is beyond the per-element bar on the case named for it."""
    case = ilc.edge_case(MUTANTS[mutant])
    bad = ilc.edge_violations(evaluate(case, mutant), case)
    print(f"{mutant} on {case['name']}: {bad}")
    assert bad, (mutant, case["name"])


def test_sums_mutant_is_the_size_the_scalar_bar_must_see():
    """One tile of 4097 missing is 2.4e-4 of each sum; the scalar bar is at most 4 x max(d_ref, 1e-6 |truth|)."""
    case = ilc.edge_case(MUTANTS["last_tile_missing_from_the_sums"])
    got = evaluate(case, "last_tile_missing_from_the_sums")
    bad = {k for k, *_ in ilc.edge_violations(got, case)}
    assert {"l1", "ssim"} <= bad and not bad & set(ilc.GRADS)
    for k in ("l1", "ssim"):
        d_ref, lim = ilc.scalar_limit(case, k)
        assert ilc.BAR * lim < 0.1 * abs(float(got[k]) - float(case["truth"][k]))


# The earlier rule, max|v - truth| / max|truth| <= 4 x max(d_ref, 1e-6), on the backward halo that is one short: does it accept it on flat-step
# content (the two step cases and the fixture's own flat_step_c1_48x80)?  MEASURED, not forced.
OLD_RULE_ACCEPTS_SHORT_HALO = {f"step_{ONE}": False, f"step_{TWO}": False, "flat_step_c1_48x80": False}


@pytest.mark.parametrize("name", sorted(OLD_RULE_ACCEPTS_SHORT_HALO))
def test_what_the_old_rule_says_about_a_short_halo_on_flat_step_content(name):
    """The old max-norm rule REJECTS the short halo here too, so this content is no evidence that it lets a seam error through: its
    ratio is 4.7 (step_33x17), 6.5 (step_65x33) and 6.8 (flat_step_c1_48x80) against the 4, where the twin's own d_ref is 2.7e-4 .. 3.7e-4,
    the largest of any case.  The per-element bar rejects it at 11 / 10 / 6.0 on the max, no more clearly.  What separates the two rules is
    the content the old one cannot judge at all (image == gt, all black: test_planted_content_is_where_the_table_says), not this mutant;
    on noise (seam_65x33_sky) both are thousands of times beyond."""
    case = ilc.edge_case(name) if name in ilc.EDGE_CASES else next(c for c in ilc.fixture_cases() if c["name"] == name)
    got = evaluate(case, "outer_taps_dropped_at_the_tile_edges")
    old, new = ilc.ratios(got, case), ilc.edge_ratios(got, case)
    print(name, "old rule:", old["g_image"], "per element:", new["g_image"])
    assert (old["g_image"] <= ilc.BAR) == OLD_RULE_ACCEPTS_SHORT_HALO[name]
    assert any(k == "g_image" for k, *_ in ilc.edge_violations(got, case))

"""Shared by tests/test_postprocess_host.py, tests/test_gpu_postprocess.py, tests/test_gpu_render_api.py and tools/postprocess_parity.py:
the seeded cases of the fused map post-processing (csrc/postprocess.hip), the truth, and THE BAR.

    truth  = oracle.postprocess_torch.postprocess_allmap in float64 on the CPU, with its autograd gradient
    d_ref  = the same function in float32 on the CPU (deterministic, never the code under test)

Per output map and per channel c of the allmap gradient, over the elements where the truth is finite:
    e      = |value - truth| / (|truth| + f_c),   f_c = median |truth_c| over its non-zero elements (1 if there are none)
    max(e) and the 99.9th percentile of e  <=  BAR * max(the float32 restatement's same statistic, FLOOR)
and a channel whose truth is identically zero must be exactly zero.  One tolerance over all seven channels cannot do this: channel 1 carries
-ge * a0 / alpha^2 and reaches 1e5 where alpha ~ 0.01 while channels 2-5 are O(1), so `2e-4 * max|g|` accepted any value at all there.

BAR = 4, the project's margin for another equally valid float32 order with contraction (image_loss_cases.BAR, optim_cases.BAR).

FLOOR = 1e-6.  Over all 90 cases x 2 upstream sets the float32 restatement shows two populations on the CPU.  The quantities with no stencil
in them (rend_normal, surf_depth, gradient channels 2-4) sit between 0 (copied or exactly representable at the tiny sizes) and 9.2e-7, a few
float32 epsilons of 1.2e-7; the floor is the next round figure above that range, so it only steps in where the restatement happens to be
exact or an ulp off.  The stencil quantities (surf_normal, surf_point, channels 0, 1, 5) reach 8e-6 .. 1.5e-3 at the max and 2.3e-4 at the
99.9th percentile where 1 / |cross product| is large and four neighbour terms cancel; there the restatement's own figure is the yardstick and
the floor plays no part.  BAR * FLOOR = 4e-6 is 2500 times under 1e-2, the size of a dropped term.  Measured on an MI355X
(profiles/postprocess_parity.json) the kernels' largest ratio is 3.7 on the max and on the percentile alike, so the max keeps the same 4x.

Elements where the truth is not finite are left out (torch gives 0 * inf = NaN at alpha == 0; the kernel gives 0 and must be finite there);
they are at most MAX_EXCLUDED of a case's elements, checked by tests/test_postprocess_host.py.  Sizes under 16 x 16 get no such pixel.
-inf never appears: torch.nan_to_num(x, 0, 0) maps it to the lowest finite float, the kernel to 0, and depths are never negative."""
import functools

import numpy as np
import torch

from oracle.postprocess_torch import postprocess_allmap as postprocess_allmap_torch
from streetunveiler_amd.camera import SimpleCamera
from streetunveiler_amd.synthetic import posed_scene, synthetic_camera

BAR = 4.0
FLOOR = 1e-6
MAX_EXCLUDED = 0.05
STATS = ("max", "p999")
OUT_MAPS = ("rend_normal", "surf_depth", "surf_normal", "surf_point")      # what the kernels write (rend_alpha / rend_dist are views)
ALL_MAPS = ("rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal", "surf_point")
MAP_CHANNELS = dict(rend_alpha=1, rend_normal=3, rend_dist=1, surf_depth=1, surf_normal=3, surf_point=3)
# (W, H): no interior (W < 3 or H < 3), the smallest interior, one 64x4 block less a column / exactly / plus a column and a row, three blocks
# across and down with odd W (W/2 fractional), the size of the earlier test, an odd pair
SIZES = ((1, 1), (2, 7), (7, 2), (3, 3), (63, 3), (64, 4), (65, 5), (129, 9), (200, 120), (131, 77))
RATIOS = (0.0, 0.4, 1.0)
CAMERAS = ("synthetic", "posed", "scaled")
UPSTREAMS = ("all", "surf_normal_only")
SCALE = 1.25


def camera(name, W, H):
    """synthetic: at the origin, yawed; posed: general position, fx != fy; scaled: a posed camera whose world-view 3x3 is a rotation times
    1.25 (no rigid motion: its inverse is no longer its transpose, so the normals' rotation and the points' inverse differ)."""
    if name == "synthetic":
        return synthetic_camera(W, H, index=6)
    if name == "posed":
        return posed_scene(1, W, H, seed=12, spread=20.0)[0]
    assert name == "scaled", name
    cam = posed_scene(1, W, H, seed=5, spread=6.0)[0]
    proj_t = cam.world_view_transform.inverse() @ cam.full_proj_transform
    wvt = cam.world_view_transform.clone()
    wvt[:3, :3] *= SCALE
    full = wvt @ proj_t
    return SimpleCamera(W, H, cam.FoVx, cam.FoVy, wvt.contiguous(), full.contiguous(), wvt.inverse()[3, :3].contiguous())


def seeded_allmap(W, H, seed=4):
    """depth 1-21, alpha 0.01-0.99; from 16 x 16 on also: an alpha == 0 patch in the corner (0/0) and one inside, a +inf patch (a0 > 0,
    alpha == 0), NaN and +inf medians, and pixels whose left and right neighbours have depth 0 (their cross product is exactly 0 with a
    non-zero row difference: the eps branch of the normalisation).  All patches are a few pixels, inside, next to finite pixels."""
    g = torch.Generator().manual_seed(seed + 7919 * W + H)
    allmap = torch.rand(7, H, W, generator=g)
    allmap[0] = allmap[0] * 20 + 1
    allmap[5] = allmap[5] * 20 + 1
    allmap[1] = allmap[1] * 0.98 + 0.01
    if W >= 16 and H >= 16:
        y, x = H // 4, W // 4
        allmap[:, :3, :5] = 0.0                          # empty corner: 0 / 0
        allmap[:, y:y + 2, x:x + 3] = 0.0                # empty inside
        allmap[1, y + 4:y + 6, x:x + 3] = 0.0            # a0 > 0, alpha == 0: +inf expected depth
        allmap[5, y + 8, x:x + 2] = float("nan")
        allmap[5, y + 8, x + 3:x + 5] = float("inf")
        allmap[5, y + 9, x + 1] = float("inf")
        allmap[0, y + 9, x + 1] = 0.0                    # ... and a pixel whose both depths vanish / are dropped
        for yy, xx in ((H // 2, W // 2), (H // 2 + 3, W // 3)):   # (yy, xx): b = 0, a != 0, |c| = 0
            allmap[0, yy, xx - 1] = allmap[0, yy, xx + 1] = 0.0
            allmap[5, yy, xx - 1] = allmap[5, yy, xx + 1] = 0.0
    return allmap


def legacy_allmap(W=200, H=120):
    """The input of the earlier test_fused_postprocess_matches_torch_restatement, unchanged: what the old assertion is judged on."""
    g = torch.Generator().manual_seed(4)
    allmap = torch.rand(7, H, W, generator=g)
    allmap[0] = allmap[0] * 20 + 1; allmap[5] = allmap[5] * 20 + 1
    allmap[1] = allmap[1] * 0.98 + 0.01
    allmap[:, :5, :9] = 0.0
    grads = {k: torch.randn(c, H, W, generator=g) for k, c in [("rend_normal", 3), ("surf_depth", 1), ("surf_normal", 3), ("surf_point", 3)]}
    return allmap, grads


def seeded_upstream(W, H, which="all", seed=4):
    g = torch.Generator().manual_seed(seed + 104729 * W + 31 * H)
    up = {k: torch.randn(MAP_CHANNELS[k], H, W, generator=g) for k in OUT_MAPS}
    if which == "surf_normal_only":     # the stencil path alone, not a small correction to the depth gradient
        up = {k: (v if k == "surf_normal" else torch.zeros_like(v)) for k, v in up.items()}
    return up


def run(fn, cam, ratio, allmap, upstream, dtype, device="cpu"):
    """fn(cam, ratio, allmap) -> dict of maps; -> {map: float64 numpy} + {"g_allmap": [7,H,W] float64 numpy}"""
    a = allmap.detach().to(device=device, dtype=dtype, copy=True).requires_grad_()
    out = fn(cam.to(device), ratio, a)
    loss = sum((out[k] * v.to(device=device, dtype=dtype)).sum() for k, v in upstream.items())
    res = {k: out[k].detach().double().cpu().numpy() for k in ALL_MAPS if k in out}
    if loss.requires_grad:
        res["g_allmap"] = torch.autograd.grad(loss, a)[0].double().cpu().numpy()
    else:                               # nothing of the output depends on the allmap (a mutant may cut every path)
        res["g_allmap"] = np.zeros(tuple(a.shape))
    return res


def kernel_like(res):
    """A torch result with its non-finite gradient elements (0 * inf at alpha == 0) set to 0, as the kernels give them."""
    return dict(res, g_allmap=np.nan_to_num(res["g_allmap"], nan=0.0, posinf=0.0, neginf=0.0))


def run_hip(cam, ratio, allmap, upstream, device="cuda:0"):
    """The HIP kernels through the autograd wrapper the renderer uses."""
    from streetunveiler_amd.gaussian_renderer import PipelineParams, postprocess_allmap
    return run(lambda c, r, a: postprocess_allmap(c, PipelineParams(depth_ratio=r), a), cam, ratio, allmap, upstream, torch.float32, device)


@functools.lru_cache(maxsize=None)
def case(W, H, ratio, cam_name, which="all"):
    """-> dict(name, cam, ratio, allmap, upstream, truth, ref); computed once per process, shared, never written to."""
    cam, allmap, up = camera(cam_name, W, H), seeded_allmap(W, H), seeded_upstream(W, H, which)
    return dict(name=f"{W}x{H}_r{ratio}_{cam_name}_{which}", W=W, H=H, cam=cam, ratio=ratio, allmap=allmap, upstream=up,
                truth=run(postprocess_allmap_torch, cam, ratio, allmap, up, torch.float64),
                ref=run(postprocess_allmap_torch, cam, ratio, allmap, up, torch.float32))


def all_cases(which=UPSTREAMS):
    return [(W, H, r, c, u) for (W, H) in SIZES for r in RATIOS for c in CAMERAS for u in which]


def channel_stats(value, truth):
    """One map or one gradient channel -> dict(max, p999, f, zero, excluded, finite_outside)"""
    value, truth = np.asarray(value, dtype=np.float64).ravel(), np.asarray(truth, dtype=np.float64).ravel()
    fin = np.isfinite(truth)
    t, v = truth[fin], value[fin]
    nz = np.abs(t[t != 0])
    f = float(np.median(nz)) if nz.size else 1.0
    with np.errstate(invalid="ignore"):
        e = np.abs(v - t) / (np.abs(t) + f)
    e = np.where(np.isfinite(e), e, np.inf)             # a non-finite value where the truth is finite is infinitely wrong
    return dict(max=float(e.max()) if e.size else 0.0, p999=float(np.percentile(e, 99.9)) if e.size else 0.0, f=f, zero=not nz.size,
                exact_zero=bool((v == 0).all()), excluded=float(1.0 - fin.mean()), finite_outside=bool(np.isfinite(value[~fin]).all()))


def quantities(res):
    """{name: array}: each output map present, and the seven gradient channels."""
    q = {k: res[k] for k in ALL_MAPS if k in res}
    q.update({f"g_allmap[{c}]": res["g_allmap"][c] for c in range(7)})
    return q


def stats(got, truth):
    tq = quantities(truth)
    return {k: channel_stats(v, tq[k]) for k, v in quantities(got).items() if k in tq}


def violations(got, truth, ref):
    """[(quantity, statistic, value, limit)] of everything beyond the bar; empty when `got` passes."""
    s, sr, bad = stats(got, truth), stats(ref, truth), []
    for k, st in s.items():
        if not st["finite_outside"]:
            bad.append((k, "finite where the truth is not", float("nan"), 0.0))
        if st["zero"] and not st["exact_zero"]:
            bad.append((k, "exactly zero", st["max"], 0.0))
        for name in STATS:
            limit = BAR * max(sr[k][name], FLOOR)
            if not st[name] <= limit:
                bad.append((k, name, st[name], limit))
    return bad


def assert_within_bar(got, truth, ref, what):
    s, sr = stats(got, truth), stats(ref, truth)
    print(what + ": " + ", ".join(f"{k} {s[k]['max']:.2e}/{sr[k]['max']:.2e} {s[k]['p999']:.2e}/{sr[k]['p999']:.2e}" for k in s))
    bad = violations(got, truth, ref)
    assert not bad, f"{what}: beyond {BAR} x max(the float32 restatement's own figure, {FLOOR}): {bad}"
    return s, sr


def legacy_accepts(g, g_truth):
    """The assertion this bar replaces as the judge of the gradient: max|d| <= 2e-4 * max|g| over all seven channels at once."""
    t = np.nan_to_num(g_truth, nan=0.0, posinf=0.0, neginf=0.0)
    return bool(np.isfinite(g).all() and np.abs(g - t).max() <= 2e-4 * np.abs(t).max())

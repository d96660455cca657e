#!/usr/bin/env python
"""Randomised parity sweep: HIP operator vs CPU oracle over many small random scenes (sizes, cameras, SH degree, tile shape,
opacity / scale regimes, precomputed colours / transMat).  Exits non-zero if a scene misses the parity bars of
tests/gpu_util.py.  python tools/fuzz_parity.py [n_scenes] [first_seed]   (FUZZ_SEEDS=a,b,c: exactly these scenes; tools/fuzz_diagnose.py
prints one scene in detail, the float32 oracle beside the kernels; seeds >= 100000: cameras in general position)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians, synthetic_upstream_grads
from tests.gpu_util import (assert_close_frac, assert_free_parity, assert_strict_parity, check_allmap, forced_f64_reference, free_f64_reference, run_hip,
                            run_hip_raw, run_oracle)
from tools.blend_pairs import blend_variants
from tests.test_gpu_parity import _check_binning

big = int(os.environ.get("FUZZ_BIG", "1"))   # FUZZ_BIG=4: images up to 4x wider/higher, 16x the Gaussians
shapes = [(16, 16)] * 4 + [(8, 8), (16, 8), (32, 8), (32, 16)]
WIDE_FOV_FROM = 500_000  # ... and from here up fx is drawn from 0.15 .. 6 W (FoVx 147 .. 10 degrees) instead of 0.55 .. 1.4 W
NEEDLES_FROM = 400_000   # ... and from here up half of the surfels are needles (axis ratio 10 .. 1000)
SURROUND_FROM = 200_000  # ... and from here up the camera is INSIDE the cloud: 30-80 % of the Gaussians behind it
POSED_FROM = 100_000    # seeds from here up draw a camera in general position (the scenes of the seeds below stay what they were)


def make_scene(seed):
    rng = np.random.default_rng(seed)
    W, H = int(rng.integers(17, 330 * big)), int(rng.integers(9, 200 * big))
    P = int(rng.integers(1, 9000 * big * big))
    lo = float(10 ** rng.uniform(-3.3, -1.5)); hi = lo * float(10 ** rng.uniform(0.3, 1.5))
    deg = int(rng.integers(0, 4))
    tile = shapes[int(rng.integers(0, len(shapes)))]
    cam = synthetic_camera(W, H, index=int(rng.integers(0, 8)))
    regime = int(rng.integers(0, 4))
    posed = seed >= POSED_FROM
    if posed:   # a camera in general position (any rotation, centre 0.5 .. 200 units out, FoVx unrelated to FoVy) instead of the origin / yaw-only ones
        from streetunveiler_amd.synthetic import posed_scene
        cam, g = posed_scene(P, W, H, seed=seed, scale_lo=lo, scale_hi=hi, spread=float(10 ** rng.uniform(-0.3, 2.3)), near_third=regime == 3,
                             behind_fraction=float(rng.uniform(0.3, 0.8)) if seed >= SURROUND_FROM else 0.0,
                             focal_range=(0.15, 6.0) if seed >= WIDE_FOV_FROM else (0.55, 1.4))
    else:
        g = synthetic_gaussians(P, W, H, seed=seed, scale_lo=lo, scale_hi=hi)
    if NEEDLES_FROM <= seed < WIDE_FOV_FROM:   # what trained surfels look like: half of them 10 .. 1000 times thinner along one axis than along the other
        # (FUZZ_NEEDLE_MAX_LOG10: the largest axis ratio, default 3 -- 1000 : 1; the ratio is set outright, whatever the two scales drawn above)
        ratio = torch.tensor(10.0 ** rng.uniform(1.0, float(os.environ.get("FUZZ_NEEDLE_MAX_LOG10", "3")), P), dtype=torch.float32)
        axis = torch.tensor(rng.integers(0, 2, P)); half = torch.tensor(rng.random(P) < 0.5)
        idx = torch.arange(P)[half]
        g["scales"][idx, axis[half]] = g["scales"][idx, 1 - axis[half]] / ratio[half]
    if regime == 1: g["opacities"] = g["opacities"] * 0.05                       # translucent: deep lists
    if regime == 2: g["opacities"] = (g["opacities"] * 0.2 + 0.8).clamp(max=1.0)  # opaque: early saturation
    if regime == 3 and not posed: g["means3D"][: P // 3, 2] = torch.rand(P // 3) * 0.5 - 0.1     # around / behind the near plane
    bg = rng.random(3).astype(np.float32)
    dc, da = synthetic_upstream_grads(W, H, seed=seed)
    colors = rng.random((P, 3)).astype(np.float32) if rng.random() < 0.25 else None
    tag = f"(seed {seed}): P={P} {W}x{H} deg={deg} tile={tile} regime={regime}{' posed' if posed else ''}{' surrounded' if seed >= SURROUND_FROM else ''}{' needles' if NEEDLES_FROM <= seed < WIDE_FOV_FROM else ''}{' wide-fov-range' if seed >= WIDE_FOV_FROM else ''} scales[{lo:.1e},{hi:.1e}] colors={'pre' if colors is not None else 'sh'}"
    return dict(g=g, cam=cam, bg=bg, deg=deg, dc=dc, da=da, colors=colors, tile=tile, regime=regime, P=P, tag=tag)


def main():
  n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 40
  seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
  seeds = [seed0 + k for k in range(n_scenes)]
  if os.environ.get("FUZZ_SEEDS"):   # exactly these scenes (regressions the sweep found)
    seeds = [int(x) for x in os.environ["FUZZ_SEEDS"].split(",")]; n_scenes = len(seeds)
  bad = both_checked = 0
  for k in range(n_scenes):
    sc = make_scene(seeds[k])
    g, cam, bg, deg, dc, da, colors, tile, regime, P = (sc[x] for x in ("g", "cam", "bg", "deg", "dc", "da", "colors", "tile", "regime", "P"))
    tag = f"scene {k} " + sc["tag"]
    try:
        fwd, bwd = run_oracle(g, cam, bg, deg, dc, da, colors=colors, tile=tile)
        raw = run_hip_raw(g, cam, bg, deg, colors=colors, tile=tile if tile != (16, 16) else None, decisions=True)
        _check_binning(raw, fwd)
        # the float64 references, once per scene: free-running (its own decisions) and with the kernels' decisions forced (the forward -- the
        # decisions' source -- is the same for every blend pair: blend_variants)
        xfwd, xbwd, margins = free_f64_reference(g, cam, bg, deg, dc, da, colors=colors, tile=tile, base=fwd, kernel_decisions=raw["decisions"])
        _, sfwd, sbwd = forced_f64_reference(g, cam, bg, deg, dc, da, tile=tile, colors=colors, base=fwd, raw=raw)
        if regime != 3:
            _, sfwd32, sbwd32 = forced_f64_reference(g, cam, bg, deg, dc, da, tile=tile, colors=colors, base=fwd, raw=raw, f64=False)
        # the 16x16 tile: BOTH blend pairs (the one-wave kernel of the large frames, the cooperative one of these), each held to every check
        # below; the default equals the one the tile-count rule picks, bit for bit (tools/blend_pairs.py)
        if tile == (16, 16):
            outs = list(zip(("one_wave", "coop"), blend_variants(g, cam, bg, deg, dc, da, colors=colors)))
            both_checked += 1
        else:
            outs = [("default", run_hip(g, cam, bg, deg, dc, da, colors=colors, tile=tile))]
        for kname, out in outs:
          try:
            # images: 1e-4 for all but a small fraction of the pixels; the rest is bounded by what ONE flipped contributor at the
            # alpha = 1/255 threshold can move: 1/255 of the channel's per-splat magnitude (rgb, depth, unit normal, ...)
            assert_close_frac(out["color"], fwd["color"], 1e-4, 1e-4, 1e-3, None, "color")
            check_allmap(out["allmap"], fwd["allmap"], "allmap", max_bad_frac=2e-3, hard=None)
            # (every pixel, against the float32 oracle OR the free-running float64 reference, whichever is closer: the reference's
            # `if (p.z == 0) continue` fires where the ORACLE's float32 p.z lands on exactly 0 -- rounding noise of a ray nearly parallel to the
            # splat's plane -- and there the kernels blend the pair through its 2-D filter footprint like exact arithmetic does: blend_common.h)
            flip = 1.5 / 255.0
            zmax = float(fwd["depths"][fwd["radii"] > 0].max()) if (fwd["radii"] > 0).any() else 1.0
            cmax = max(1.0, float(fwd["rgb"].max()))
            both = lambda a, r32, r64: np.minimum(np.abs(a - r32), np.abs(a - r64)).max()
            # (not in the camera-plane regime: there the flipped decision is `depth < near` of a splat at full opacity, not one at the alpha floor)
            if regime != 3:
                assert both(out["color"], fwd["color"], xfwd["color"]) <= flip * cmax + 1e-3, "color beyond one flipped contributor"
                for ch, mag in ((0, zmax), (1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0), (6, 1.0)):
                    e = both(out["allmap"][ch], fwd["allmap"][ch], xfwd["allmap"][ch])
                    assert e <= flip * mag + 1e-3 * max(1.0, mag), f"allmap[{ch}] err {e:.3e} beyond one flipped contributor ({flip * mag:.3e})"
            # ... and the free-running float64 reference (its own decisions): on every ROBUST pixel the kernels stop at the same entry, pick
            # the same median and agree within 1e-4; on every robust Gaussian the strict row bars hold.  (Random regimes -- translucent deep
            # lists, splats around the near plane -- make many pixels non-robust: the fraction is reported, not bounded, here.)
            rep = {}
            # regime 3 puts splats around the camera plane: p.z -> 0 inside a footprint makes the VALUE of the ray-splat intersection
            # ill-conditioned in float32 (not a decision): the value bars get a factor 5 there, the identical-decision checks none
            # Non-robust elements (a decision within float32 rounding of its threshold: either implementation may take it either way, and one
            # flipped contributor moves a few-pixel splat's whole gradient) only have to be finite here -- they are pinned below with the
            # decisions FORCED.  A robust-row bar reads "within the bar, or at least twice as accurate as the float32 oracle on those rows":
            # some random scenes (translucent deep lists of large splats) put float32 itself 1e-2 from the float64 reference.
            assert_free_parity(out, raw["img"]["n_contrib"], xfwd, xbwd, margins, scene=(g, cam), report=rep, pixel_budget=1.0, gaussian_budget=1.0,
                               value_slack=5.0 if regime == 3 else 1.0, nonrobust_pixel_cap=None, nonrobust_row_cap=None, oracle32=bwd, oracle32_fwd=fwd,
                               differing_cap=1e-4 if big == 1 else 5e-4)   # (FUZZ_BIG: pixels thousands of contributors deep -- tests/gpu_util.py assert_free_parity)
            # ... and EVERY element, robust or not, with the kernels' own decisions forced on a float64 evaluation (blend and K8 in double):
            # 1e-4 (1 + |v|) at every pixel of colour and aux maps, the strict row bars on every visible Gaussian
            # (row bars: within the bar, or no worse than the float32 oracle under the same forced decisions -- some random scenes cancel badly)
            if regime != 3:
                assert_strict_parity(out, sfwd, sbwd, scene=(g, cam), oracle32=sbwd32, oracle32_fwd=sfwd32, value_noise=margins["value_noise"])
            names = ["dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D", "dL_dcolors" if colors is not None else "dL_dsh"]
            # Per GAUSSIAN, against the float32 oracle: any gradient element of a ROBUST Gaussian off by more than 2e-3 of its tensor's scale
            # marks it.  (A flipped decision moves the whole gradient of a few-pixel splat: those Gaussians are the non-robust ones, checked
            # above against the float64 reference's looser bound.)  What is left is the float32 oracle's own conditioning on grazing splats:
            # more than max(3, 0.1 %) marked Gaussians is a failure.
            marked = np.zeros(P, bool)
            for n in names:
                ref = np.asarray(bwd[n], np.float64).reshape(P, -1); got = np.asarray(out[n], np.float64).reshape(P, -1)
                scale = np.abs(ref).max()
                if scale > 0:
                    marked |= (np.abs(got - ref) / scale > 2e-3).any(axis=1) & (margins["gaussian"] > 1.0)   # (float32 oracle; robust Gaussians only)
                    assert np.isfinite(got).all(), n + " not finite"
            assert marked.sum() <= max(3, int(1e-3 * P)), f"{int(marked.sum())} Gaussians with out-of-tolerance gradients: {np.nonzero(marked)[0][:8]}"
          except AssertionError as e:
            raise AssertionError(f"[{kname}] {e}") from e
        vis = fwd["radii"] > 0
        print("ok  ", tag, f"D={fwd['num_rendered']} robust px {(margins['pixel'] > 1).mean():.4f} gaussians {((margins['gaussian'] > 1) & vis).sum() / max(1, vis.sum()):.3f}", flush=True)
    except AssertionError as e:
        bad += 1
        print("FAIL", tag, "\n     ", str(e).splitlines()[0][:300], flush=True)
  print(f"{n_scenes - bad}/{n_scenes} scenes within the parity bars")
  print(f"one-wave and cooperative K7 both checked on {both_checked} scenes")
  sys.exit(1 if bad else 0)


if __name__ == "__main__":
  main()

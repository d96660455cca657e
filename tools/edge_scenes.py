#!/usr/bin/env python
"""The catalogue of edge scenes: the inputs on which kernels go wrong while benign scenes pass -- thousands of equal depth keys per tile,
one list of more than 20 000 entries, frames smaller than a tile, zero / sub-denormal / huge scales, zero quaternions, opacity exactly 0
and 1, NaN / Inf parameters, frames where nothing survives culling, and a frame whose last 32x16 tile row is cut inside its lower band.
The parity tests (tests/gpu_util.py re-exports this module) and tools/fuzz_parity.py build their scenes here, so that every blend-kernel
instantiation can be held to the oracle on the SAME scenes (tests/test_gpu_blend_matrix.py).

A builder returns an EdgeScene: it unpacks as `(cam, g, bg, sh_degree, (dc, da), budgets)` -- `budgets` = the non-robust budgets
assert_free_parity gets on that scene ({} = the defaults) -- and carries, seeded per scene, what the 6- / 9-channel passes need on the same
geometry: `extra` [P,6] colours, `bg9` (bg + six more entries) and `dc9` [9,H,W] (dc + six more channels of upstream gradient).

    python tools/edge_scenes.py        # sha256 of every input tensor of every scene (CPU only): equal before and after a refactoring"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians, synthetic_upstream_grads


class EdgeScene(tuple):
    """(cam, g, bg, sh_degree, (dc, da), budgets) + .name, .extra, .bg9, .dc9, and for `non_finite` .poisoned (indices) / .field."""

    def __new__(cls, name, cam, g, bg, deg, dc, da, budgets=None, **attrs):
        bg = np.asarray(bg, np.float32)
        self = super().__new__(cls, (cam, g, bg, int(deg), (dc, da), dict(budgets or {})))
        self.name = name
        P, (H, W) = g["means3D"].shape[0], dc.shape[1:]
        seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")   # (of the name: stable across processes)
        rng = np.random.default_rng(seed)
        self.extra = rng.random((P, 6)).astype(np.float32)
        self.bg9 = np.concatenate([bg, rng.random(6).astype(np.float32)])
        self.dc9 = torch.cat([dc, torch.randn(6, H, W, generator=torch.Generator().manual_seed(seed))], 0).contiguous()
        for k, v in attrs.items():
            setattr(self, k, v)
        return self

    cam = property(lambda s: s[0]); g = property(lambda s: s[1]); bg = property(lambda s: s[2]); deg = property(lambda s: s[3])
    dc = property(lambda s: s[4][0]); da = property(lambda s: s[4][1]); budgets = property(lambda s: s[5])


def plain_scene(P, W, H, seed, lo, hi, cam_index=None):
    """The benchmark-style scene of the parity tests -> (cam, g)."""
    return synthetic_camera(W, H, index=cam_index), synthetic_gaussians(P, W, H, seed=seed, scale_lo=lo, scale_hi=hi)


def ties():
    """Densification clones Gaussians in place: every position shared by 8 Gaussians, a third of the scene on four depth planes (thousands
    of equal depth keys per tile).  Eight co-located Gaussians per position make every pixel's list eight times as dense in near-threshold
    decisions: 2.8 % of the pixels are non-robust against ~1 % on the plain small scenes -- hence the budgets."""
    P, W, H = 24000, 320, 200
    cam, g = plain_scene(P, W, H, 77, 3e-3, 4e-2, 4)
    base = g["means3D"][: P // 8].clone()
    g["means3D"] = base.repeat(8, 1).contiguous()                       # Gaussian i and i + k P/8 share a position
    third = P // 3
    planes = torch.tensor([2.0, 5.0, 11.0, 23.0])[torch.arange(third) % 4]
    world_z_axis = cam.world_view_transform[:3, 2]                      # view depth = p . column 2 (camera at the origin)
    p = g["means3D"][:third]
    depth = p @ world_z_axis
    g["means3D"][:third] = p * (planes / depth)[:, None]                 # along the ray: same pixel, new depth ...
    g["scales"][:third] = g["scales"][:third] * (planes / depth)[:, None]   # ... and the same footprint
    dc, da = synthetic_upstream_grads(W, H, seed=77)
    return EdgeScene("ties", cam, g, [0.1, 0.5, 0.2], 3, dc, da, dict(pixel_budget=5e-2, gaussian_budget=0.6))


def long_list():
    """40 k translucent splats over a 24x20 image: one tile, > 600 staging rounds of 64, contributor counts past 16 bits."""
    P, W, H = 40000, 24, 20
    cam, g = plain_scene(P, W, H, 41, 2e-2, 2e-1, 0)
    g["opacities"] = g["opacities"] * 0.02          # nothing saturates: every pixel walks (almost) the whole list
    dc, da = synthetic_upstream_grads(W, H, seed=5)
    return EdgeScene("long_list", cam, g, [0.3, 0.6, 0.9], 2, dc, da)


TINY_FRAMES = ((5, 3), (1, 1), (17, 1))


def tiny(w, h):
    """Frames smaller than a tile / a single pixel / a single row."""
    cam, g = plain_scene(300, w, h, 42, 5e-2, 5e-1, 1)
    dc, da = synthetic_upstream_grads(w, h, seed=6)
    return EdgeScene(f"tiny_{w}x{h}", cam, g, [0.3, 0.6, 0.9], 1, dc, da)


def degenerate():
    """Zero / sub-denormal / gigantic scales, zero quaternions, opacity exactly 0 and 1."""
    P, W, H = 6000, 240, 136
    cam, g = plain_scene(P, W, H, 77, 3e-3, 5e-2, 2)
    idx = np.random.default_rng(0).permutation(P)
    g["scales"][idx[:60], 0] = 0.0; g["scales"][idx[60:120]] = 0.0
    g["opacities"][idx[120:180]] = 0.0; g["opacities"][idx[180:240]] = 1.0
    g["rotations"][idx[240:300]] = 0.0
    g["scales"][idx[300:360]] = 1e-12; g["scales"][idx[360:420]] = 50.0
    dc, da = synthetic_upstream_grads(W, H, seed=3)
    return EdgeScene("degenerate", cam, g, np.zeros(3, np.float32), 3, dc, da)


NON_FINITE_VARIANTS = [("means3D", float("nan")), ("means3D", float("inf")), ("scales", float("nan")), ("scales", float("inf")), ("rotations", float("nan")),
                       ("opacities", float("nan")), ("opacities", float("inf")), ("shs", float("nan"))]


def non_finite(field, val):
    """Every 50th Gaussian with a NaN / Inf in `field` (.poisoned = their indices): a diverging training run's parameters."""
    P, W, H = 6000, 240, 136
    cam, g = plain_scene(P, W, H, 3, 3e-3, 5e-2, 2)
    dc, da = synthetic_upstream_grads(W, H, seed=3)
    idx = torch.arange(0, P, 50)
    gg = {k: v.clone() for k, v in g.items()}
    if field == "means3D": gg[field][idx, 2] = val
    elif field == "shs": gg[field][idx, 0, 0] = val
    else: gg[field][idx, 0] = val
    return EdgeScene(f"non_finite_{field}_{val}", cam, gg, [0.1, 0.2, 0.3], 3, dc, da, poisoned=idx.numpy(), field=field, value=val)


OPACITY_EXTREME_SIZES = [(30000, 384, 216, 5e-4, 5e-3, None), (8000, 200, 150, 5e-3, 8e-2, 6), (3000, 160, 96, 2e-2, 3e-1, 1)]


def opacity_extremes(k):
    """Opacity 0.003 (below 1/255: can never contribute) and exactly 1.0 sprinkled in: thin, medium and huge splats (k = 0, 1, 2)."""
    P, W, H, lo, hi, idx = OPACITY_EXTREME_SIZES[k]
    cam, g = plain_scene(P, W, H, P + 1, lo, hi, idx)
    g["opacities"][::7] = 0.003   # below 1/255: can never contribute
    g["opacities"][::11] = 1.0
    dc, da = synthetic_upstream_grads(W, H, seed=P)
    return EdgeScene(f"opacity_extremes_{k}", cam, g, [0.2, 0.4, 0.6], 3, dc, da)


def _culled_frame():
    W, H = 64, 48
    return W, H, synthetic_camera(W, H), np.array([0.1, 0.2, 0.3], np.float32), synthetic_upstream_grads(W, H)


def no_gaussians():
    """P == 0."""
    W, H, cam, bg, (dc, da) = _culled_frame()
    g0 = {k: v[:0] for k, v in synthetic_gaussians(4, W, H).items()}
    return EdgeScene("no_gaussians", cam, g0, bg, 3, dc, da)


def all_culled():
    """Everything behind the camera: D == 0."""
    W, H, cam, bg, (dc, da) = _culled_frame()
    g = synthetic_gaussians(100, W, H)
    g["means3D"][:, 2] *= -1
    return EdgeScene("all_culled", cam, g, bg, 3, dc, da)


RAGGED_BANDS_FRAME = (203, 125)   # a multiple of no tile shape; 125 = 7 x 16 + 13: the last 32x16 tile row holds 8 + 5 rows, its lower 32x8 band is cut


def ragged_bands():
    """The banded walk of the 32x16 tile with 6 / 9 channels (two 32x8 bands per tile, the second walk adding to the first one's records or
    storing its own): splats from a pixel to a third of the frame wide, so that list entries exist that reach the upper band only, the
    lower band only, and both -- in the cut last tile row too (band_coverage() states it; the matrix test asserts it from the kernels'
    own pair decisions)."""
    W, H = RAGGED_BANDS_FRAME
    assert all(W % t for t in (8, 16, 32)) and all(H % t for t in (8, 16)) and 9 <= H % 16 <= 15
    P = 3000
    cam, g = plain_scene(P, W, H, 29, 2e-3, 6e-2, 5)
    g["opacities"][::9] = 1.0
    dc, da = synthetic_upstream_grads(W, H, seed=29)
    return EdgeScene("ragged_bands", cam, g, [0.25, 0.1, 0.4], 3, dc, da)


def band_coverage(valid, ranges, n_contrib, W, H, tile=(32, 16)):
    """From the kernels' pair decisions of a 32x16 frame (run_hip_raw(..., decisions=True, tile=(32, 16)): `valid` u64[D, 8], one ballot per
    (list entry, 8x8 quadrant), lane = (x & 7) + 8 (y & 7)) and the per-pixel stopping positions `n_contrib`[H, W]: which list entries
    blend into a pixel of the upper 32x8 band of their tile, of the lower one, of both.  -> {(last_row, "upper" | "lower" | "both"): count}
    with last_row = the entry's tile lies in the last tile row (cut by the image edge)."""
    tw, th = tile
    assert (tw, th) == (32, 16)
    gx, gy = (W + tw - 1) // tw, (H + th - 1) // th
    valid = np.asarray(valid).view(np.uint64).reshape(-1, 8)
    bits = ((valid[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)   # [D, quadrant, lane]
    out = {}
    ranges = np.asarray(ranges).view(np.uint32).reshape(-1, 2)
    for t in range(gx * gy):
        r0, r1 = int(ranges[t][0]), int(ranges[t][1])
        if r1 <= r0:
            continue
        x0, y0 = (t % gx) * tw, (t // gx) * th
        reach = np.zeros((r1 - r0, 2), bool)
        pos = np.arange(r1 - r0)
        for q in range(8):
            for lane in range(64):
                px, py = x0 + (q % 4) * 8 + (lane & 7), y0 + (q // 4) * 8 + (lane >> 3)
                if px < W and py < H:
                    reach[:, q // 4] |= bits[r0:r1, q, lane] & (pos < int(n_contrib[py, px]))
        for key, m in (("upper", reach[:, 0] & ~reach[:, 1]), ("lower", ~reach[:, 0] & reach[:, 1]), ("both", reach[:, 0] & reach[:, 1])):
            k = (t // gx == gy - 1, key)
            out[k] = out.get(k, 0) + int(m.sum())
    return out


def catalogue():
    """name -> builder (no arguments), in the order of the matrix test."""
    c = {"ties": ties, "long_list": long_list}
    for (w, h) in TINY_FRAMES:
        c[f"tiny_{w}x{h}"] = (lambda w=w, h=h: tiny(w, h))
    c["degenerate"] = degenerate
    for field, val in NON_FINITE_VARIANTS:
        c[f"non_finite_{field}_{val}"] = (lambda field=field, val=val: non_finite(field, val))
    for k in range(len(OPACITY_EXTREME_SIZES)):
        c[f"opacity_extremes_{k}"] = (lambda k=k: opacity_extremes(k))
    c.update(no_gaussians=no_gaussians, all_culled=all_culled, ragged_bands=ragged_bands)
    return c


def scene_hashes(sc, extras=True):
    """sha256 (first 16 hex digits) of every input of a scene: the Gaussians' tensors, bg, dc, da, the camera's matrices."""
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else np.asarray(a)).tobytes()).hexdigest()[:16]
    cam, g, bg, deg, (dc, da), budgets = sc
    out = {k: h(v) for k, v in sorted(g.items())}
    out.update(bg=h(np.asarray(bg, np.float32)), dc=h(dc), da=h(da), view=h(cam.world_view_transform), proj=h(cam.full_proj_transform),
               campos=h(cam.camera_center), size=f"{cam.image_width}x{cam.image_height}", deg=deg, budgets=sorted(budgets.items()))
    if extras:
        out.update(extra=h(sc.extra), bg9=h(sc.bg9), dc9=h(sc.dc9))
    return out


if __name__ == "__main__":
    import json
    print(json.dumps({name: scene_hashes(build(), extras="--no-extras" not in sys.argv) for name, build in catalogue().items()}, indent=1, sort_keys=True))

"""Shared by tests/test_tsdf_host.py, tests/test_gpu_tsdf.py, tools/tsdf_parity.py and tools/time_tsdf.py: the seeded cases of the TSDF
fusion, their expectation (streetunveiler_amd.tsdf.unbounded_tsdf_torch in float64 on the CPU, computed once per case, with its float32
run and the decision margins), a second, independent statement of the same semantics (own bilinear taps instead of grid_sample; it also
produces the wrong implementations the bar must reject, and, with `fused=True`, evaluates the projection and the taps with fused
multiply-adds the way the kernel does), and THE BAR (`compare`):

  * per case and per output (tsdf, r, g, b) dev32 = the largest |float32 checker - float64 checker| over the admitted samples, both on
    the CPU; an implementation must stay within 2 dev32 of the float64 checker on EVERY admitted sample (two float32 evaluations of one
    expression that differ in rounding order only -- the kernel contracts the projection and the taps with FMAs);
  * its weight (1 + the number of views that integrated the sample) must equal the float64 checker's exactly on every admitted sample.

A sample is admitted iff its float64 margin (unbounded_tsdf_torch, return_margin) is at least MARGIN, or the case PLANTS it: the
decisions of a planted sample are exact by construction -- zc == 0 at a camera centre, pix = 1 - 2^-24, sdf == -trunc, a NaN pixel -- so
the margin, which is 0 there by its definition, says nothing about it; that float32 and float64 decide alike on every admitted sample,
planted ones included, is asserted by tests/test_tsdf_host.py.  At most MAX_EXCLUDED of a case may be excluded, none of `exact_edge`,
of `grid`, or of the planted samples."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from streetunveiler_amd import tsdf as T

MARGIN = 1e-4
MAX_EXCLUDED = 0.005
BAR = 2.0
V, H, W, N = 6, 37, 53, 20001      # neither a wave multiple nor a float4 multiple
TAN_Y = 0.4
TAN_X = TAN_Y * W / H
DISTANCE, FAR = 4.0, 6.0           # the cameras' distance from the origin; the depth where a ray misses the sphere
SPHERE = (0.3, 0.1, -0.2)          # centre of the unit sphere the cameras look at (off the origin: every view differs)
CENTER, RADIUS, VOXEL = (0.1, -0.05, 0.15), 2.0, 0.02
RING = tuple(60.0 * k for k in range(V))
ARC = tuple(20.0 * k for k in range(V))      # 100 degrees: there is a point behind every camera
TAILS = (0, 1, 63, 64, 65, N)
OUTPUTS = ("tsdf", "r", "g", "b")


def _views(angles, seed, h=H, w=W):
    """Cameras at DISTANCE from the origin, yawed by `angles` and looking at it; full_proj = (P W2C)^T as the reference's Camera
    builds it, computed in float64 and rounded once; the depth maps are the analytic depth of the sphere, the colours random."""
    r = torch.Generator().manual_seed(seed)
    tan_x = TAN_Y * w / h
    P = torch.zeros(4, 4, dtype=torch.float64)
    P[0, 0], P[1, 1], P[3, 2], P[2, 2], P[2, 3] = 1 / tan_x, 1 / TAN_Y, 1.0, 100 / 99.99, -100 * 0.01 / 99.99
    jj, ii = torch.meshgrid(torch.arange(w, dtype=torch.float64), torch.arange(h, dtype=torch.float64), indexing="xy")
    d = torch.stack([(2 * jj / (w - 1) - 1) * tan_x, (2 * ii / (h - 1) - 1) * TAN_Y, torch.ones_like(jj)], dim=-1)      # rays, z = 1
    full, depth = [], []
    for a in angles:
        c, s = (1.0, 0.0) if a == 0 else (math.cos(math.radians(a)), math.sin(math.radians(a)))
        R = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)      # camera to world; the camera sits at R (0, 0, -DISTANCE)
        w2c = torch.eye(4, dtype=torch.float64)
        w2c[:3, :3], w2c[2, 3] = R.T, DISTANCE
        full.append((P @ w2c).T)
        o = w2c[:3, :3] @ torch.tensor(SPHERE, dtype=torch.float64) + w2c[:3, 3]      # the sphere's centre in camera coordinates
        dd, do = (d * d).sum(-1), (d * o).sum(-1)
        disc = do * do - dd * ((o * o).sum() - 1)
        depth.append(torch.where(disc >= 0, (do - torch.sqrt(disc.clamp(min=0))) / dd, torch.full_like(dd, FAR)))
    n = len(angles)
    return torch.stack(depth).reshape(n, 1, h, w).float(), torch.rand((n, 3, h, w), generator=r), torch.stack(full).float()


def _case(depth, rgb, full_proj, samples, voxel_size=VOXEL, center=None, radius=None, planted=(), none_excluded=False):
    exact = torch.zeros(samples.shape[0], dtype=torch.bool)
    exact[list(planted)] = True
    return SimpleNamespace(depth=depth, rgb=rgb, full_proj=full_proj, samples=samples.float().contiguous(), voxel_size=voxel_size, center=center,
                           radius=radius, exact=exact, none_excluded=none_excluded, n_planted=len(planted))


def _uniform(n, seed):
    return torch.rand((n, 3), generator=torch.Generator().manual_seed(seed)) * 3 - 1.5


def _ring(n=N, v=V):
    depth, rgb, full = _views(RING, 1)
    return _case(depth[:v], rgb[:v], full[:v], _uniform(n, 2), center=CENTER, radius=RADIUS)


def _ring_plain():
    return _case(*_views(RING, 1), _uniform(N, 3))


def _pixel_point(i, j, zc):
    """The world point that view 0 of ARC / RING (no rotation) sees at row i, column j (fractional) and depth zc."""
    return [(2 * j / (W - 1) - 1) * TAN_X * zc, (2 * i / (H - 1) - 1) * TAN_Y * zc, zc - DISTANCE]


def _nonfinite():
    depth, rgb, full = _views(ARC, 4)
    depth[0, 0, 10, 20], depth[0, 0, 25, 40] = float("nan"), float("inf")
    m = math.radians(50.0)      # the middle of the arc: 10 units behind it, every camera has the point at its back
    planted = [[0.0, 0.0, -DISTANCE],                               # the centre of camera 0: q = (0, 0, ., 0), pix = 0 / 0
               [-10 * math.sin(m), 0.0, -10 * math.cos(m)],        # behind every camera
               [0.0, 50.0, 0.0],                                    # in front of all of them, far above every frame: nobody sees it
               _pixel_point(10.3, 20.3, 3.2),                       # on the NaN pixel of view 0
               _pixel_point(24.7, 39.6, 3.2)]                       # on the +inf pixel of view 0
    samples = torch.cat([torch.tensor(planted, dtype=torch.float64).float(), _uniform(N - len(planted), 5)])
    return _case(depth, rgb, full, samples, planted=range(len(planted)))


EDGE_TRUNC_VOXEL = 0.025      # trunc = 0.125 exactly


def _exact_edge(tie_depth=0.875):
    """pix = (x, y) and zc = 1 exactly in the last view; the five views before it have zc = -1.  Depths, colours and coordinates are
    dyadic.  x, y in {1 - 2^-24, -(1 - 2^-24), 0.5, -0.25, 0}: at 1 - 2^-24 float32 gives ix == W - 1 exactly, the east (south) tap
    has index W (H) -- in the last row of the last view that is past the allocation.  (0, 0) sits on pixel (18, 26), whose depth is
    1 - trunc: sdf == -trunc, not integrated (`>`)."""
    r = torch.Generator().manual_seed(6)
    depth = torch.randint(8, 24, (V, 1, H, W), generator=r).float() / 8      # 1 .. 2.875: sdf >= 0
    rgb = torch.randint(0, 17, (V, 3, H, W), generator=r).float() / 16
    depth[V - 1, 0, 18, 26] = tie_depth
    full = torch.zeros(V, 4, 4)
    full[:, 3, 3] = -1.0
    full[V - 1] = torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]])
    e = float(np.nextafter(np.float32(1), np.float32(0)))
    values = [e, -e, 0.5, -0.25, 0.0]
    samples = torch.tensor([[x, y, z] for x in values for y in values for z in (0.0, 0.5)], dtype=torch.float64)
    return _case(depth, rgb, full, samples, voxel_size=EDGE_TRUNC_VOXEL, planted=range(len(samples)), none_excluded=True)


GRID_LO, GRID_HI, GRID_DIMS, GRID_SLAB = (-1.2, -1.1, -1.3), (1.3, 1.2, 1.1), (5, 7, 9), 3


def _grid():
    depth, rgb, full = _views(RING, 1)
    return _case(depth, rgb, full, T.grid_coordinates(GRID_LO, GRID_HI, GRID_DIMS).reshape(-1, 3), center=CENTER, radius=RADIUS, none_excluded=True)


CASES = {"ring": _ring, "ring_plain": _ring_plain, "nonfinite": _nonfinite, "exact_edge": _exact_edge, "grid": _grid}
for _n in TAILS:
    CASES[f"tails_{_n}"] = functools.partial(_ring, _n, 1)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def run_checker(c, dtype=torch.float64, device="cpu"):
    """unbounded_tsdf_torch on the case's tensors in `dtype` on `device` -> (tsdf, rgb, weight, margin)."""
    to = lambda t: t.to(device=device, dtype=dtype)
    return T.unbounded_tsdf_torch(to(c.samples), to(c.depth), to(c.rgb), to(c.full_proj), c.voxel_size, c.center, c.radius, return_rgb=True,
                                  return_weight=True, return_margin=True)


def _outputs(tsdf, rgb):
    rgb = rgb.detach().cpu().double()
    return {"tsdf": tsdf.detach().cpu().double(), "r": rgb[:, 0], "g": rgb[:, 1], "b": rgb[:, 2]}


def expectation(c):
    """-> want (the float64 checker's outputs), weight, admitted, dev32 {output: float}, the float32 checker's weight."""
    tsdf, rgb, weight, margin = run_checker(c)
    tsdf32, rgb32, weight32, _ = run_checker(c, torch.float32)
    admitted = (margin >= MARGIN) | c.exact
    want, ref = _outputs(tsdf, rgb), _outputs(tsdf32, rgb32)
    dev32 = {k: (float((ref[k] - want[k])[admitted].abs().max()) if admitted.any() else 0.0) for k in OUTPUTS}
    return SimpleNamespace(want=want, weight=weight, admitted=admitted, dev32=dev32, weight32=weight32.double(), margin=margin)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The expectation of a case, computed once and shared; left unchanged by everyone."""
    return expectation(case(name))


def compare(tsdf, rgb, weight, want, what=""):
    """THE BAR of the module docstring: an implementation's outputs (any device, float32 or float64; rgb may be None) against `want`
    (`expected(name)`).  Prints every figure before it asserts.  -> {output: (deviation, dev32)}."""
    n = want.weight.shape[0]
    assert tuple(tsdf.shape) == (n,) and tuple(weight.shape) == (n,) and (rgb is None or tuple(rgb.shape) == (n, 3)), f"{what}: shapes"
    a = want.admitted
    got = _outputs(tsdf, rgb if rgb is not None else torch.stack([want.want[k] for k in "rgb"], dim=1))
    out, failed = {}, []
    wrong = int((weight.detach().cpu().double() != want.weight)[a].sum())
    print(f"{what}: {int(a.sum())} of {n} samples admitted, {wrong} weight(s) differ from the float64 checker's")
    for k in OUTPUTS:
        g, w = got[k][a], want.want[k][a]
        assert torch.equal(torch.isfinite(g), torch.isfinite(w)), f"{what}: {k} is non-finite at other samples than the float64 checker"
        dev = float((g - w)[torch.isfinite(w)].abs().max()) if torch.isfinite(w).any() else 0.0
        out[k] = (dev, want.dev32[k])
        print(f"{what}: {k}: deviation {dev:.3e}, float32 checker {want.dev32[k]:.3e}, bound {BAR * want.dev32[k]:.3e}")
        if dev > BAR * want.dev32[k]:
            failed.append(f"{k} off by {dev:.3e}, beyond {BAR} x {want.dev32[k]:.3e}")
    assert wrong == 0, f"{what}: {wrong} admitted sample(s) were integrated by other views than in the float64 checker"
    assert not failed, f"{what}: " + "; ".join(failed)
    return out


# ---- the second statement, and the wrong implementations -----------------------------------------------------------------------------
MUTANTS = {"align_corners=False": "ring", "maps in reverse view order": "ring", "weights starting at 0": "ring", "tsdf starting at 0": "ring",
           "constant truncation": "ring", "contraction test on the normalised point": "ring", "sdf >= -trunc": "exact_edge",
           "colour averaged without the weight": "ring"}


def restate(c, dtype=torch.float64, mutant=None, fused=False, reverse_loop=False):
    """The semantics per sample with explicit bilinear taps (nw, ne, sw, se; an out-of-bounds tap contributes nothing and is not read)
    -> (tsdf, rgb, weight).  `fused`: float32 with the projection and the taps accumulated by fused multiply-adds (the product and the
    sum taken in float64, rounded once), as csrc/tsdf.hip does.  `reverse_loop`: the views walked last to first -- the same mean, so
    nothing a bar could reject; the mutant 'maps in reverse view order' pairs view v's matrix with the maps of view V - 1 - v."""
    if fused:
        dtype = torch.float32
        fma = lambda a, b, acc: (a.double() * b.double() + acc.double()).float()
    else:
        fma = lambda a, b, acc: a * b + acc
    p = c.samples.to(dtype)
    trunc = torch.full((p.shape[0],), 5 * c.voxel_size, dtype=dtype)
    if c.center is not None:
        mag = torch.sqrt((p * p).sum(dim=1, keepdim=True))
        u = torch.where(mag < 1, p, (1 / (2 - mag)) * (p / mag))
        p = u * c.radius + torch.tensor(c.center, dtype=dtype)
        norm = torch.sqrt(((u if mutant == "contraction test on the normalised point" else p) ** 2).sum(dim=1))
        if mutant != "constant truncation":
            trunc = torch.where(norm > 1, trunc * (1 / (2 - norm.clamp(max=1.9))), trunc)
    x, y, z = p.unbind(dim=1)
    n_views = c.full_proj.shape[0]
    tsdf = torch.full_like(x, 0.0 if mutant == "tsdf starting at 0" else 1.0)
    weight = torch.full_like(x, 0.0 if mutant == "weights starting at 0" else 1.0)
    rgb = torch.zeros((x.shape[0], 3), dtype=dtype)
    order = range(n_views - 1, -1, -1) if reverse_loop else range(n_views)
    for v in order:
        F = c.full_proj[v].to(dtype)
        m = n_views - 1 - v if mutant == "maps in reverse view order" else v
        rec = torch.cat([c.depth[m], c.rgb[m]]).to(dtype).reshape(4, -1)
        col = lambda k: fma(z, F[2, k], fma(y, F[1, k], fma(x, F[0, k], F[3, k].expand_as(x))))
        qx, qy, zc = col(0), col(1), col(3)
        px, py = qx / zc, qy / zc
        mask = (px > -1) & (px < 1) & (py > -1) & (py < 1) & (zc > 0)
        if mutant == "align_corners=False":
            fx, fy = (((px + 1) * W - 1) / 2).clamp(0, W - 1), (((py + 1) * H - 1) / 2).clamp(0, H - 1)
        else:
            fx, fy = (px + 1) / 2 * (W - 1), (py + 1) / 2 * (H - 1)
        fx, fy = torch.where(mask, fx, torch.zeros_like(fx)), torch.where(mask, fy, torch.zeros_like(fy))      # masked out: no fetch
        x0, y0 = torch.floor(fx), torch.floor(fy)
        ex, ey, dx, dy = (x0 + 1) - fx, (y0 + 1) - fy, fx - x0, fy - y0
        acc = torch.zeros((4, x.shape[0]), dtype=dtype)
        for xi, yi, wgt in ((x0, y0, ex * ey), (x0 + 1, y0, dx * ey), (x0, y0 + 1, ex * dy), (x0 + 1, y0 + 1, dx * dy)):
            inb = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            at = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
            acc = torch.where(inb, fma(rec[:, at], wgt.expand(4, -1), acc), acc)
        sdf = acc[0] - zc
        integrate = mask & ((sdf >= -trunc) if mutant == "sdf >= -trunc" else (sdf > -trunc))
        s = (sdf / trunc).clamp(-1.0, 1.0)
        wp = weight + 1
        tsdf = torch.where(integrate, (tsdf * weight + s) / wp, tsdf)
        colour_weight = torch.ones_like(weight) if mutant == "colour averaged without the weight" else weight
        rgb = torch.where(integrate[:, None], (rgb * colour_weight[:, None] + acc[1:].T) / wp[:, None], rgb)
        weight = torch.where(integrate, wp, weight)
    return tsdf, rgb, weight

#!/usr/bin/env python
"""Are two builds of the library bit-identical in their results?  Renders one scene fwd + bwd with each (a subprocess per build,
SURFEL_RASTER_LIB) and compares every output and gradient bit for bit.
    python tools/ab_identical.py ab/libA.so ab/libB.so [P W H] [--deg D] [--coeffs M] [--misalign]
--deg / --coeffs: the active SH degree and the coefficients per row (M != 16 takes K1 / K8 off their LDS-staged path); --misalign: the SH
tensor is a view 4 bytes into its storage (contiguous, not 16-byte aligned: off the staged path as well)."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--worker")
ap.add_argument("--size", nargs=3, default=["400000", "1280", "720"], metavar=("P", "W", "H"))   # (how the worker is told; the command line gives it as P W H)
ap.add_argument("pos", nargs="*")
ap.add_argument("--deg", type=int, default=3)
ap.add_argument("--coeffs", type=int, default=16)
ap.add_argument("--misalign", action="store_true")
a = ap.parse_args()
size = a.pos[2:5] if len(a.pos) >= 5 else a.size

if a.worker:
    import torch
    from tests.gpu_util import DEV, run_hip
    from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians, synthetic_upstream_grads
    P, W, H = (int(v) for v in size)
    cam = synthetic_camera(W, H, index=3); g = synthetic_gaussians(P, W, H, seed=5)
    shs = g["shs"][:, :a.coeffs].contiguous().to(DEV)
    if a.misalign:
        buf = torch.zeros(shs.numel() + 1, device=DEV)
        buf[1:].view(shs.shape).copy_(shs)
        shs = buf[1:].view(shs.shape)
        assert shs.data_ptr() % 16 != 0
    g["shs"] = shs
    dc, da = synthetic_upstream_grads(W, H)
    out = run_hip(g, cam, [0.1, 0.2, 0.3], a.deg, dc, da)
    np.savez(a.worker, **{k: v for k, v in out.items() if v is not None})
    sys.exit(0)

res = []
for i, lib in enumerate(a.pos[:2]):
    out = f"/tmp/ab_identical_{i}.npz"
    subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", out, "--size"] + size + ["--deg", str(a.deg), "--coeffs", str(a.coeffs)] +
                   (["--misalign"] if a.misalign else []), check=True, cwd=ROOT, env=dict(os.environ, SURFEL_RASTER_LIB=os.path.abspath(lib)))
    res.append(dict(np.load(out)))
bad = [k for k in res[0] if not np.array_equal(res[0][k], res[1][k], equal_nan=True)]
for k in res[0]:
    x, y = res[0][k].astype(np.float64), res[1][k].astype(np.float64)
    d = np.abs(x - y)
    rel = (d / np.maximum(np.abs(x), 1e-30))[d > 0].max(initial=0.0)
    print(f"{k:16s} {'identical' if k not in bad else 'DIFFERS'}  max |a - b| = {d.max():.3e}  max |a - b| / |a| = {rel:.3e}  nonzero {np.count_nonzero(x)}")
print(f"P={size[0]} {size[1]}x{size[2]} deg={a.deg} M={a.coeffs} misalign={a.misalign}: " + ("BIT-IDENTICAL" if not bad else f"NOT identical: {bad}"))
sys.exit(1 if bad else 0)

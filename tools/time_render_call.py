#!/usr/bin/env python
"""render() (operator + fused map post-processing + the python around it) vs the bare operator, fwd+bwd at the C3 size.
    python tools/time_render_call.py [P W H calls]   -- e.g. 1000 160 96 2000: a size at which the host binds, so the figure is host time per call"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
from streetunveiler_amd.gaussian_renderer import PipelineParams, SurfelModel, render
from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians
from tools import measure
P, W, H, N = (int(a) for a in sys.argv[1:5]) if len(sys.argv) > 4 else (3_000_000, 1920, 1080, 10)
dev = "cuda:0"
cam = synthetic_camera(W, H).to(dev)
g = {k: v.to(dev).requires_grad_() for k, v in synthetic_gaussians(P, W, H).items()}
pc = SurfelModel(g["means3D"], g["scales"], g["rotations"], g["opacities"], g["shs"], None, 3, 3)
bg = torch.zeros(3, device=dev); pipe = PipelineParams()
s = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), bg, 1.0, cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
def full():
    for t in g.values(): t.grad = None
    o = render(cam, pc, pipe, bg)
    (o["render"].sum() + o["rend_dist"].sum() + o["rend_alpha"].sum() + (o["rend_normal"] * o["surf_normal"]).sum()).backward()
def bare():
    for t in g.values(): t.grad = None
    c, r, a = GaussianRasterizer(s)(means3D=g["means3D"], means2D=m2d, shs=g["shs"], opacities=g["opacities"], scales=g["scales"], rotations=g["rotations"])
    (c.sum() + a.sum()).backward()
for name, fn in (("bare operator + sum losses", bare), ("render() + regulariser-style losses", full)):
    ms = measure.alternating_rounds({name: fn}, rounds=1, iters=N, warmup=3)[name][0]
    print(f"{name}: {ms:.4f} ms fwd+bwd")

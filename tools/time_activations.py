#!/usr/bin/env python
"""parameter activations (exp / sigmoid / normalize) as torch ops in front of the operator (what the
reference's GaussianModel getters do) vs fused into K1 / K8, one fwd+bwd at the C3 size.  python tools/time_activations.py"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians, synthetic_upstream_grads
from tools import measure
P, W, H, dev = 3_000_000, 1920, 1080, "cuda:0"
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
cam = synthetic_camera(W, H)
g = synthetic_gaussians(P, W, H)
raw = dict(means3D=g["means3D"], shs=g["shs"], scaling=torch.log(g["scales"]), opacity=torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)),
           rotation=g["rotations"] * 2.0)
raw = {k: v.to(dev).requires_grad_() for k, v in raw.items()}
dc, da = [t.to(dev) for t in synthetic_upstream_grads(W, H)]
m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
s = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.zeros(3, device=dev), 1.0,
                                  cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 3, cam.camera_center.to(dev), False, False)
def step(fused):
    for t in raw.values(): t.grad = None
    if fused:
        o, sc, ro = raw["opacity"], raw["scaling"], raw["rotation"]
    else:
        o, sc, ro = torch.sigmoid(raw["opacity"]), torch.exp(raw["scaling"]), torch.nn.functional.normalize(raw["rotation"])
    c, r, a = GaussianRasterizer(s, fused_activations=fused)(means3D=raw["means3D"], means2D=m2d, shs=raw["shs"], opacities=o, scales=sc, rotations=ro)
    torch.autograd.backward([c, a], [dc, da])
for name, fused in (("torch activations in front of the operator", False), ("activations fused into K1/K8", True)):
    ms = measure.alternating_rounds({name: lambda: step(fused)}, rounds=1, iters=steps, warmup=3)[name][0]
    print(f"{name}: {ms:.3f} ms per fwd+bwd")

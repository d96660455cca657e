"""Shared by tests/test_optim_host.py, tests/test_gpu_optim.py and tools/optimizer_parity.py: the reference's six parameter shapes and
groups, seeded tensors and gradients, the float64 truth of a run of Adam steps, the per-step rounding bound and THE BAR of a long run.

The bar of a run (test_gpu_optim.py: 50 steps; the drop-in contract: 3 + 3 steps around the reference's tensor surgery): for each of
p, m, v the largest absolute deviation of the HIP step from the float64 checker, over every tensor of the run, is at most 4 x the
largest deviation of `torch.optim.Adam(foreach=False)` in float32 on the same GPU from the same checker.  4x admits another, equally valid
rounding order (torch's kernels contract into fma, the HIP kernel does not); a wrong formula is off by orders of magnitude.

The bound of ONE step from float32-representable inputs (the edge cases), with u = 2^-24 the unit roundoff, S = max(|m0|, |g|),
w = 1 - beta and every float32 operation within u of its exact result (correctly rounded division and square root included):
    m:  fl(g - m0) [u 2S] . fl(w) [u] . product [u] . sum [u S]                     <=  7 u S            -> tol_m = 8 u S
    v:  fl(beta2) v0 [2u] + fl(w2) g g [3u] , sum [u]                                <=  4 u v            -> tol_v = 8 u v
    denom = sqrt(v) / bc2_sqrt + eps: relative  tol_v / (2 v) + 4u;   q = m / denom:  tol_m / denom + |q| (tol_v / (2 v) + 5u)
    p:  step_size [u] . q [u] , difference [u |p|]       -> tol_p = 2 u |p| + step_size (tol_m / denom + |q| (tol_v / (2 v) + 8u))
(the counted bounds are worst cases; tol_m, tol_v and the last factor carry the small margins shown)."""
import math

import torch

from streetunveiler_amd.optim import SurfelAdam, adam_step, adam_step_float64

BAR = 4.0
U = 2.0 ** -24
BETAS, EPS = (0.9, 0.999), 1e-15
# the six groups of the reference's training_setup [REF scene/gaussian_model.py:171-178], learning rates of its arguments/__init__.py
GROUPS = (("xyz", (3,), 0.00016), ("f_dc", (1, 3), 0.0025), ("f_rest", (15, 3), 0.0025 / 20.0), ("opacity", (1,), 0.05),
          ("scaling", (2,), 0.005), ("rotation", (4,), 0.001))


def reference_shapes(P):
    return [(P,) + tail for _, tail, _ in GROUPS]


def seeded_gradient(shape, seed, lo=1e-6, hi=1e1, zero_every=7):
    """float32 on the CPU: magnitudes log-uniform in [lo, hi], random signs, every `zero_every`-th element exactly zero."""
    r = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    mag = torch.exp(torch.rand(n, generator=r, dtype=torch.float64) * math.log(hi / lo) + math.log(lo))
    g = (mag * (torch.randint(0, 2, (n,), generator=r) * 2 - 1)).float()
    if zero_every:
        g[(torch.arange(n) + seed) % zero_every == 0] = 0.0
    return g.reshape(shape)


def seeded_state(shapes, seed, moments=True):
    """[(p, m, v)] float32 on the CPU; moments=False: zero state (the first step of a parameter)."""
    r = torch.Generator().manual_seed(seed)
    out = []
    for shape in shapes:
        p = torch.randn(shape, generator=r)
        m = 0.1 * torch.randn(shape, generator=r) if moments else torch.zeros(shape)
        v = 0.01 * torch.rand(shape, generator=r) if moments else torch.zeros(shape)
        out.append((p, m, v))
    return out


def step_tolerances(p0, g, m0, v0, lr, step, beta1, beta2, eps):
    """float64 (p, m, v) after one step and the rounding bounds (tol_p, tol_m, tol_v) of the module docstring, element-wise."""
    p, g, m, v = (t.detach().double().cpu().clone() for t in (p0, g, m0, v0))
    S = torch.maximum(m.abs(), g.abs())
    adam_step_float64([p], [g], [m], [v], [lr], [step], beta1, beta2, eps)
    step_size, bc2_sqrt = lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5
    tol_m, tol_v = 8 * U * S, 8 * U * v
    denom = v.sqrt() / bc2_sqrt + eps
    rel_v = torch.where(v > 0, tol_v / (2 * v).clamp_min(1e-300), torch.zeros_like(v))
    tol_p = 2 * U * p.abs() + step_size * (tol_m / denom + (m / denom).abs() * (rel_v + 8 * U))
    return (p, m, v), (tol_p, tol_m, tol_v)


def assert_one_step_within_bounds(got, inputs, lr, step, what, beta1=BETAS[0], beta2=BETAS[1], eps=EPS):
    """got = (p, m, v) after the HIP step, inputs = (p0, g, m0, v0) before it; elements that are non-finite in the float64 checker must be
    non-finite in `got` and the other way round."""
    want, tols = step_tolerances(*inputs, lr, step, beta1, beta2, eps)
    for name, a, b, tol in zip("pmv", got, want, tols):
        a = a.detach().double().cpu().reshape(b.shape)
        finite = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), finite), f"{what}: {name} is non-finite at other elements than the float64 checker"
        over = ((a - b).abs() - tol)[finite]
        assert over.numel() == 0 or float(over.max()) <= 0, f"{what}: {name} off by {float((a - b).abs()[finite].max()):.3e}, {float(over.max()):.3e} beyond its bound"


def make_optimizer(cls, tensors, device, dtype, **kw):
    """`cls` over the reference's six named groups; tensors = [p] in GROUPS order -> (optimizer, {name: parameter})."""
    params = {name: torch.nn.Parameter(t.detach().to(device=device, dtype=dtype, copy=True)) for (name, _, _), t in zip(GROUPS, tensors)}
    groups = [dict(params=[params[name]], lr=lr, name=name) for name, _, lr in GROUPS]
    return cls(groups, lr=0.0, eps=EPS, **kw), params


def named_params(opt):
    return {g["name"]: g["params"][0] for g in opt.param_groups}


def set_grads(opt, grads):
    """grads: {name: float32 CPU tensor or None}"""
    for group in opt.param_groups:
        p = group["params"][0]
        g = grads.get(group["name"])
        p.grad = None if g is None else g.to(device=p.device, dtype=p.dtype)


def deviations(opt, truth):
    """{p, m, v: largest |value - truth| over the six groups} of an optimizer against the float64 one."""
    out = dict(p=0.0, m=0.0, v=0.0)
    t_params = named_params(truth)
    for name, p in named_params(opt).items():
        tp = t_params[name]
        for key, a, b in (("p", p, tp), ("m", opt.state[p]["exp_avg"], truth.state[tp]["exp_avg"]), ("v", opt.state[p]["exp_avg_sq"], truth.state[tp]["exp_avg_sq"])):
            out[key] = max(out[key], float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max()))
    return out


def ratios(dev_hip, dev_torch):
    return {k: dev_hip[k] / dev_torch[k] for k in dev_hip}


def three_optimizers(P, device, seed=0):
    """SurfelAdam and torch.optim.Adam(foreach=False) in float32 on `device`, torch.optim.Adam in float64 on the CPU (the truth:
    tests/test_optim_host.py pins adam_step_float64 to it at 1e-12), from equal parameters."""
    tensors = [p for p, _, _ in seeded_state(reference_shapes(P), seed)]
    hip = make_optimizer(SurfelAdam, tensors, device, torch.float32)[0]
    ref = make_optimizer(torch.optim.Adam, tensors, device, torch.float32, foreach=False)[0]
    truth = make_optimizer(torch.optim.Adam, tensors, "cpu", torch.float64, foreach=False)[0]
    return hip, ref, truth


def run_steps(opts, P_of, first_step, count, seed=0):
    """`count` steps of every optimizer in `opts` on the same seeded gradients (step numbers first_step ...)."""
    for it in range(first_step, first_step + count):
        P = P_of(opts[0])
        grads = {name: seeded_gradient((P,) + tail, 1000 * it + k + seed) for k, (name, tail, _) in enumerate(GROUPS)}
        for opt in opts:
            set_grads(opt, grads)
            opt.step()


def accuracy_run(device, P=1037, steps=50):
    """The 50-step run of the accuracy bar -> (deviation of SurfelAdam, deviation of torch float32, ratios)."""
    hip, ref, truth = three_optimizers(P, device)
    run_steps([hip, ref, truth], lambda o: o.param_groups[0]["params"][0].shape[0], 1, steps)
    d_hip, d_ref = deviations(hip, truth), deviations(ref, truth)
    return d_hip, d_ref, ratios(d_hip, d_ref)


# ---- the reference's tensor surgery on an optimizer [REF scene/gaussian_model.py:384-472], restated ----------------------------------
def replace_tensor_to_optimizer(opt, tensor, name):
    out = {}
    for group in opt.param_groups:
        if group["name"] == name:
            stored_state = opt.state.get(group["params"][0], None)
            if stored_state is not None:
                if "exp_avg" in stored_state:
                    stored_state["exp_avg"] = torch.zeros_like(tensor)
                if "exp_avg_sq" in stored_state:
                    stored_state["exp_avg_sq"] = torch.zeros_like(tensor)
                del opt.state[group["params"][0]]
                group["params"][0] = torch.nn.Parameter(tensor.requires_grad_(True))
                opt.state[group["params"][0]] = stored_state
            out[group["name"]] = group["params"][0]
    return out


def prune_optimizer(opt, mask):
    out = {}
    for group in opt.param_groups:
        stored_state = opt.state.get(group["params"][0], None)
        if stored_state is not None:
            stored_state["exp_avg"] = stored_state["exp_avg"][mask]
            stored_state["exp_avg_sq"] = stored_state["exp_avg_sq"][mask]
            del opt.state[group["params"][0]]
            group["params"][0] = torch.nn.Parameter(group["params"][0][mask].requires_grad_(True))
            opt.state[group["params"][0]] = stored_state
        else:
            group["params"][0] = torch.nn.Parameter(group["params"][0][mask].requires_grad_(True))
        out[group["name"]] = group["params"][0]
    return out


def cat_tensors_to_optimizer(opt, tensors_dict):
    out = {}
    for group in opt.param_groups:
        assert len(group["params"]) == 1
        extension_tensor = tensors_dict[group["name"]]
        stored_state = opt.state.get(group["params"][0], None)
        if stored_state is not None:
            stored_state["exp_avg"] = torch.cat((stored_state["exp_avg"], torch.zeros_like(extension_tensor)), dim=0)
            stored_state["exp_avg_sq"] = torch.cat((stored_state["exp_avg_sq"], torch.zeros_like(extension_tensor)), dim=0)
            del opt.state[group["params"][0]]
            group["params"][0] = torch.nn.Parameter(torch.cat((group["params"][0], extension_tensor), dim=0).requires_grad_(True))
            opt.state[group["params"][0]] = stored_state
        else:
            group["params"][0] = torch.nn.Parameter(torch.cat((group["params"][0], extension_tensor), dim=0).requires_grad_(True))
        out[group["name"]] = group["params"][0]
    return out


def surgery(opt, seed=0):
    """Prune a fifth of the rows, append 53 new ones, reset the opacities: the same on every optimizer (masks and values from the seed)."""
    P = opt.param_groups[0]["params"][0].shape[0]
    r = torch.Generator().manual_seed(seed + 17)
    like = opt.param_groups[0]["params"][0]
    keep = torch.rand(P, generator=r) > 0.2
    prune_optimizer(opt, keep.to(like.device))
    new = {name: torch.randn((53,) + tail, generator=r).to(device=like.device, dtype=like.dtype) for name, tail, _ in GROUPS}
    cat_tensors_to_optimizer(opt, new)
    opacity = named_params(opt)["opacity"]
    replace_tensor_to_optimizer(opt, torch.full_like(opacity.detach(), -2.0), "opacity")


# ---- densification statistics --------------------------------------------------------------------------------------------------------
def stats_case(P, visible, seed=0):
    """visible in {"none", "all", "third"} -> float32 / int32 CPU tensors (viewspace_grad, radii, accum [P,1], denom [P,1], max_radii2D [P]);
    the gradient rows of invisible Gaussians hold NaN."""
    r = torch.Generator().manual_seed(seed + P)
    radii = torch.randint(1, 200, (P,), generator=r, dtype=torch.int32)
    if visible == "none":
        radii[:] = 0
    elif visible == "third":
        radii[torch.arange(P) % 3 != 0] = 0
    grad = seeded_gradient((P, 3), seed + 3, lo=1e-8, hi=1e-2, zero_every=0)
    grad[radii == 0] = float("nan")
    accum = torch.rand(P, 1, generator=r)
    denom = torch.randint(0, 50, (P, 1), generator=r).float()
    max_radii = torch.randint(0, 200, (P,), generator=r).float()
    return grad, radii, accum, denom, max_radii

"""Cases, references and THE bar of the sky model (streetunveiler_amd/sky.py, csrc/sky.hip), shared by tests/test_sky_host.py,
tests/test_gpu_sky.py and tools/sky_parity.py.

  truth      sky_forward_torch -- the reference's lines, full 111-channel input, per-pixel grid lookups -- in float64 and its autograd;
  yardstick  the same function in float32 on the CPU.  Never the code under test;
  the bar    per case and per TENSOR (the image, every weight gradient, the grid's gradient):
                 max|got - truth| <= BAR x max(max|yardstick - truth|, FLOOR x max|truth|)
             the form and the figures of tests/image_loss_cases.py: BAR = 4 for another, equally valid float32 evaluation order (the
             kernels sum 64 pixels in a fma chain and the rest in float64; torch sums in blocks), FLOOR = 1e-6 of the tensor's scale.
             Per tensor, not per element: a ReLU whose float32 pre-activation falls on the other side of zero from the float64 one moves
             one pixel's contribution, in the yardstick as in the kernels.
  Kinks: a hidden unit whose float64 pre-activation lies within KINK = 1e-6 of zero (and is not exactly zero) can fall on either side in
  float32 -- the two twins differ by up to 3.4e-7 there on these cases, and they disagree about 1 to 2 of the 12.7 M signs of a 263x251
  case -- and each such sign moves that pixel's whole contribution to the gradients below it, by more than any rounding bar.  Which side
  is taken is not a property of the model, so the upstream gradient g_out of such a pixel is zero in every case: chosen from the float64
  truth alone: 4 of the 4096 pixels of 64x64, 15 of the 8643 of 67x129, 76 and 63 of the 66013 of the two 263x251 cases, none of any other
  case.  So no case checks the backward ON such a pixel; the forward is checked on all of them.  An exactly zero pre-activation (all-zero weights) is no such case: relu'(0) = 0 everywhere.
  Where the truth is NaN (a NaN in c2w) the result must be NaN in the same places; nothing else is asked of that case.

Sizes: the kernels take 256 pixels per workgroup in waves of 64, the backward hands one wave's pixels at a time to the weight-gradient
sums and a workgroup sweeps the image in strides of (workgroups x 256).  1x1; 1x65 (one pixel past a wave); 5x7; 64x64 (16 full
workgroups); 67x129 (ragged in both axes); 263x251 with max_workgroups 3 (86 sweeps, a three-term fixed-order sum) and 1 (one workgroup
sweeps everything).  The camera and weight cases run at 19x23 = 437 pixels: two workgroups, the second ragged, its last wave partly
empty."""
import functools

import numpy as np
import torch

from streetunveiler_amd import sky

BAR = 4.0
FLOOR = 1e-6
KINK = 1e-6
# exactly on a vertex of level 0 -- and, the scales being odd, of every level: 0.5 * (16 * 2^l - 1) + 0.5 = 8 * 2^l, exact in float32 and float64
VERTEX = [0.5, 0.5, 0.5]
SHAPES = [(1, 1, 0), (1, 65, 0), (5, 7, 0), (64, 64, 0), (67, 129, 0), (263, 251, 3), (263, 251, 1)]     # (H, W, max_workgroups)
SMALL = (19, 23)
WEIGHT_GRADS = tuple("g_" + n for n in sky.WEIGHT_NAMES)
MODEL_GRADS = ("g_params", "g_w0", "g_b0", "g_w1", "g_b1", "g_w2", "g_b2", "g_w3", "g_b3")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_state(seed=0, grid_scale=1.0):
    """{params, w0 [64,111], b0, w1, b1, w2, b2, w3, b3} float32: nn.Linear's default initialisation, the grid uniform in +-1e-4."""
    g = _gen(1000 + seed)
    state = {"params": (torch.rand(sky.GRID_PARAMS, generator=g) * 2 - 1) * 1e-4 * grid_scale}
    for k, (fan_out, fan_in) in enumerate([(64, sky.INPUT_CHANNELS), (64, 64), (64, 64), (3, 64)]):
        bound = 1.0 / fan_in ** 0.5
        state[f"w{k}"] = (torch.rand(fan_out, fan_in, generator=g) * 2 - 1) * bound
        state[f"b{k}"] = (torch.rand(fan_out, generator=g) * 2 - 1) * bound
    return state


def camera(H, W, fx=None, fy=None, cx=None, cy=None, seed=0, rotation=True):
    g = _gen(2000 + seed)
    fx = 0.9 * W if fx is None else fx
    K = torch.tensor([[fx, 0.0, W / 2 if cx is None else cx], [0.0, fx if fy is None else fy, H / 2 if cy is None else cy], [0.0, 0.0, 1.0]])
    m = torch.randn(3, 3, generator=g)
    c2w = torch.eye(4)
    c2w[:3, :3] = torch.linalg.qr(m)[0] if rotation else m
    c2w[:3, 3] = torch.tensor([0.31, 0.62, 0.17])
    return K, c2w


def unambiguous_pixels(H, W, state, K, c2w):
    """[H,W] bool: False where a hidden pre-activation of the float64 truth is within KINK of zero without being zero."""
    params, layers = layers_of(state, torch.float64, "cpu")
    _, rays_d = sky.get_rays(H, W, K, c2w, "cpu", torch.float64)
    feat = sky.position_features(params, c2w[:3, 3].double())
    x = torch.cat([sky.sh_encode(rays_d.reshape(-1, 3)), feat.expand(H * W, -1)], -1)
    keep = torch.ones(H * W, dtype=torch.bool)
    for weight, bias in layers[:3]:
        z = torch.nn.functional.linear(x, weight, bias)
        keep &= ~((z.abs() < KINK) & (z != 0)).any(1)
        x = torch.relu(z)
    return keep.reshape(H, W)


def _on_vertex(position, dtype):
    """True if `position` has frac == 0 on every axis of every level when evaluated in `dtype`."""
    _, weights = sky.grid_rows_and_weights(torch.tensor([position], dtype=dtype))
    return bool(((weights == 0) | (weights == 1)).all()) and bool((weights.sum(-1) == 1).all())


assert _on_vertex(VERTEX, torch.float32) and _on_vertex(VERTEX, torch.float64) and not _on_vertex([0.31, 0.62, 0.17], torch.float64)


def _case(name, H, W, state, K, c2w, max_workgroups=0, seed=0):
    g_out = torch.randn(3, H, W, generator=_gen(3000 + seed)) * unambiguous_pixels(H, W, state, K, c2w)
    return dict(name=name, H=H, W=W, state=state, K=K, c2w=c2w, max_workgroups=max_workgroups, g_out=g_out)


def _scaled(state, factor):
    return {k: (v * factor if k != "params" else v) for k, v in state.items()}


def cases():
    out = []
    default = make_state(0)
    for k, (H, W, wg) in enumerate(SHAPES):
        out.append(_case(f"shape_{H}x{W}_wg{wg}", H, W, default, *camera(H, W, seed=k), max_workgroups=wg, seed=k))
    H, W = SMALL
    out.append(_case("fx_ne_fy", H, W, default, *camera(H, W, fx=31.0, fy=17.0, seed=10), seed=10))
    out.append(_case("principal_point_outside", H, W, default, *camera(H, W, fx=8.0, cx=-60.0, cy=75.0, seed=11), seed=11))
    out.append(_case("c2w_not_a_rotation", H, W, default, *camera(H, W, seed=12, rotation=False), seed=12))
    K, c2w = camera(H, W, seed=13)
    c2w[1, 2] = float("nan")
    out.append(_case("nan_in_c2w", H, W, default, K, c2w, seed=13))
    for k, pos in enumerate(([0.31, 0.62, 0.17], VERTEX, [-0.7, -2.5, -0.01], [1e3, -1e3, 1e3])):
        K, c2w = camera(H, W, seed=20 + k)
        c2w[:3, 3] = torch.tensor(pos)
        out.append(_case(("position_inside", "position_on_vertex", "position_negative", "position_1e3")[k], H, W, make_state(1, grid_scale=1e4),
                         K, c2w, seed=20 + k))
    out.append(_case("weights_zero", H, W, {k: (torch.zeros_like(v) if k != "b3" else torch.tensor([0.3, -1.2, 2.0])) for k, v in default.items()},
                     *camera(H, W, seed=30), seed=30))
    dead = dict(default, b0=torch.full((64,), -100.0))
    out.append(_case("first_layer_dead", H, W, dead, *camera(H, W, seed=31), seed=31))
    out.append(_case("weights_x50", H, W, _scaled(default, 50.0), *camera(H, W, seed=32), seed=32))
    huge = dict(default, b1=default["b1"].clone())
    huge["b1"][5] = 1e4
    out.append(_case("one_huge_bias", H, W, huge, *camera(H, W, seed=33), seed=33))
    return out


def layers_of(state, dtype=None, device=None, grad=False):
    """(params, [(w, b)] * 4) as leaves of the given dtype / device."""
    prep = lambda t: t.detach().to(device=device, dtype=dtype, copy=True).requires_grad_(grad)
    return prep(state["params"]), [(prep(state[f"w{k}"]), prep(state[f"b{k}"])) for k in range(4)]


def twin(case, dtype):
    """sky_forward_torch and its autograd on the CPU -> {image, g_params, g_w0 [64,111], g_b0, ..., g_w3, g_b3} as float64 numpy."""
    params, layers = layers_of(case["state"], dtype, "cpu", grad=True)
    image = sky.sky_forward_torch(params, layers, case["H"], case["W"], case["K"], case["c2w"])
    leaves = [params] + [t for pair in layers for t in pair]
    grads = torch.autograd.grad((image * case["g_out"].to(dtype)).sum(), leaves)
    out = {"image": image}
    out.update(dict(zip(MODEL_GRADS, grads)))
    return {k: v.detach().double().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _reference(i):
    return twin(CASES[i], torch.float64), twin(CASES[i], torch.float32)


def reference(case):
    """(truth, yardstick), computed once per case and shared."""
    return _reference(next(i for i, c in enumerate(CASES) if c is case))


def fused_view(res):
    """The twin's results as the fused operator names them: g_w0sh = g_w0[:, :16], g_c = g_b0."""
    out = {"image": res["image"], "g_w0sh": res["g_w0"][:, :sky.SH_CHANNELS], "g_c": res["g_b0"]}
    out.update({k: res[k] for k in WEIGHT_GRADS[2:]})
    return out


def ratios(got, truth, yard):
    """{tensor: max|got - truth| / (BAR x max(max|yard - truth|, FLOOR x max|truth|))}: passes when <= 1.  NaN truth: 0 if got is NaN
    exactly where the truth is, else inf."""
    out = {}
    for key, t in truth.items():
        g, y = np.asarray(got[key], dtype=np.float64), yard[key]
        if np.isnan(t).any():
            out[key] = 0.0 if np.array_equal(np.isnan(g), np.isnan(t)) else float("inf")
            continue
        if t.size == 0:
            out[key] = 0.0
            continue
        if not np.isfinite(g).all():
            out[key] = float("inf")
            continue
        limit = BAR * max(float(np.abs(y - t).max()), FLOOR * float(np.abs(t).max()), 1e-45)
        out[key] = float(np.abs(g - t).max()) / limit
    return out


def assert_within_bar(got, truth, yard, what):
    assert set(got) == set(truth), (what, sorted(got), sorted(truth))
    r = ratios(got, truth, yard)
    print(what + ": " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{what}: beyond {BAR} x max(the float32 twin's own deviation, {FLOOR} x scale), as a multiple of that limit: {bad}"
    return r


# ---- the code under test ---------------------------------------------------------------------------------------------------------------
def run_model(case, dev):
    """SkyModel.render_with_camera + autograd on `dev` -> the twin's keys."""
    model = sky.SkyModel(device=dev)
    model.load_state_dict(state_dict_of(case["state"]))
    model.max_workgroups = case["max_workgroups"]
    image = model.render_with_camera(case["H"], case["W"], case["K"], case["c2w"])
    leaves = [model.position_encoding.params] + [t for pair in model.blocks.pairs() for t in pair]
    grads = torch.autograd.grad((image * case["g_out"].to(dev)).sum(), leaves)
    out = {"image": image}
    out.update(dict(zip(MODEL_GRADS, grads)))
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def fused_inputs(case, dev):
    """(cam, [w0sh, c, w1, b1, w2, b2, w3, b3]) on `dev`: c formed in float64 and rounded once, so it is not what is under test."""
    s = case["state"]
    feat = sky.position_features(s["params"].double(), case["c2w"][:3, 3].double())
    c = (s["w0"][:, sky.SH_CHANNELS:].double() @ feat + s["b0"].double()).float()
    weights = [s["w0"][:, :sky.SH_CHANNELS].contiguous(), c, s["w1"], s["b1"], s["w2"], s["b2"], s["w3"], s["b3"]]
    return sky.camera_tensor(case["K"], case["c2w"], dev), [t.to(dev) for t in weights]


def run_raw(case, dev, want=(True,) * 8):
    """The raw C-ABI pair -> {image, g_w0sh, g_c, ...}: the wanted gradients only."""
    cam, weights = fused_inputs(case, dev)
    image = sky.sky_forward(cam, case["H"], case["W"], *weights, max_workgroups=case["max_workgroups"])
    grads = sky.sky_backward(cam, case["H"], case["W"], *weights, g_out=case["g_out"].to(dev), want=want, max_workgroups=case["max_workgroups"])
    out = {"image": image}
    for k, g, w in zip(WEIGHT_GRADS, grads, want):
        assert (g is not None) == bool(w), k
        if w:
            out[k] = g
    return {k: v.double().cpu().numpy() for k, v in out.items()}


def state_dict_of(state):
    """The reference's names: position_encoding.params, blocks.layers.{k}.weight / .bias."""
    out = {"position_encoding.params": state["params"]}
    for k in range(4):
        out[f"blocks.layers.{k}.weight"], out[f"blocks.layers.{k}.bias"] = state[f"w{k}"], state[f"b{k}"]
    return out


CASES = cases()

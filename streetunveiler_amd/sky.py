"""The sky model of a training iteration [REF scene/env_map.py; train.py:114-115, 199-200]: SH-encoded ray directions, a hash-grid and
a frequency encoding of the ray origin, and a 111 -> 64 -> 64 -> 64 -> 3 MLP with a sigmoid.

    SkyModel                         the reference's module: forward(v, position), render_with_camera(H, W, K, c2w), save / load,
                                     .optimizer, and its state_dict() names and shapes (a sky_params.pt of either side loads into the other)
    position_features(params, x)     the 95 channels that depend on the ray origin alone: 32 of the grid, 63 of the embedding (plain torch)
    sky_rays_mlp(cam, H, W, ...)     the fused operator (HIP, csrc/sky.hip) for what differs per pixel; sky_forward / sky_backward are its
                                     two raw calls (no autograd, caller-owned buffers, capturable into a HIP graph)
    sky_forward_torch(...)           the reference's lines in the reference's order, with the full 111-channel input and per-pixel grid
                                     lookups: in float64 the truth, in float32 the yardstick and the timing baseline

render_with_camera gives every pixel the same origin (rays_o = c2w[:3, 3]), so the 95 position channels are ONE vector per frame and
fold into the first layer's bias, c = W0[:, 16:] feat + b0 (torch, autograd); the kernels do the direction, its 16 SH values, the four
layers and the sigmoid.  Deliberate differences from the CUDA original: the grid's parameters and features are float32 (tiny-cuda-nn
rounds them to float16), and the float -> uint32 conversion of a grid cell is written out as the saturating one."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from ._call import buf, call, ptr, workspace as _workspace

SH_DEGREE, SH_CHANNELS = 4, 16
N_LEVELS, FEATURES_PER_LEVEL, LOG2_HASHMAP_SIZE, BASE_RESOLUTION, PER_LEVEL_SCALE = 16, 2, 16, 16, 2.0
EMBED_FREQS, EMBED_CHANNELS = 10, 63
HIDDEN, GRID_CHANNELS = 64, N_LEVELS * FEATURES_PER_LEVEL
INPUT_CHANNELS = SH_CHANNELS + GRID_CHANNELS + EMBED_CHANNELS      # 111, in this order
_HASH_PRIMES = (1, 2654435761, 805459861)
_U32 = 0xFFFFFFFF


def grid_levels():
    """[(scale, resolution, rows, first row, hashed)] of the 16 levels: tiny-cuda-nn's Grid in 3-D with the reference's settings."""
    out, first = [], 0
    for level in range(N_LEVELS):
        scale = BASE_RESOLUTION * PER_LEVEL_SCALE ** level - 1.0
        res = int(math.ceil(scale)) + 1
        rows = min((res ** 3 + 7) // 8 * 8, 1 << LOG2_HASHMAP_SIZE)
        stride = 1
        for _ in range(3):
            if stride <= 1 << LOG2_HASHMAP_SIZE:
                stride *= res
        out.append((scale, res, rows, first, stride > 1 << LOG2_HASHMAP_SIZE))
        first += rows
    return out


GRID_LEVELS = grid_levels()
GRID_ROWS = sum(level[2] for level in GRID_LEVELS)
GRID_PARAMS = GRID_ROWS * FEATURES_PER_LEVEL                       # 1 908 736


_LEVEL_TENSORS = {}


def _level_tensors(device, dtype):
    """The levels' constants as tensors on `device`, built once: scale [16] in `dtype`; res, rows, first [16] int64; hashed [16] bool;
    the corners' bits [8,3] bool."""
    key = (str(device), dtype)
    if key not in _LEVEL_TENSORS:
        i64 = lambda k: torch.tensor([level[k] for level in GRID_LEVELS], dtype=torch.int64, device=device)
        _LEVEL_TENSORS[key] = (torch.tensor([level[0] for level in GRID_LEVELS], dtype=dtype, device=device), i64(1), i64(2), i64(3),
                               torch.tensor([level[4] for level in GRID_LEVELS], device=device),
                               torch.tensor([[(corner >> d) & 1 for d in range(3)] for corner in range(8)], dtype=torch.bool, device=device))
    return _LEVEL_TENSORS[key]


def grid_rows_and_weights(x):
    """x [N,3] -> (rows [N,16,8] int64 into the [GRID_ROWS, 2] table, weights [N,16,8]).  A cell is floor(p) converted to uint32 with
    saturation: negative or NaN -> 0, >= 2^32 -> 2^32 - 1; a NaN coordinate keeps its NaN in the weights.  All levels and corners at
    once: a dozen tensor operations whatever N is (per frame this runs on ONE position, where launches are the whole cost)."""
    scale, res, n_rows, first, hashed, bits = _level_tensors(x.device, x.dtype)
    p = x[:, None, :] * scale[None, :, None] + 0.5                                   # [N,16,3]
    fl = torch.floor(p)
    frac = p - fl
    # (NaN >= 0 is False.)  The upper limit is applied to the INTEGER: 2^32 - 1 is no float32 number, a float32 clamp would stop at 2^32
    cell = torch.where(fl >= 0, fl, torch.zeros_like(fl)).clamp(max=float(_U32 + 1)).to(torch.int64).clamp(max=_U32)
    c = (cell[:, :, None, :] + bits.to(torch.int64)[None, None]) & _U32              # [N,16,8,3]
    r = res[None, :, None]
    dense = (c[..., 0] + c[..., 1] * r + c[..., 2] * (r * r)) & _U32
    hashed_index = c[..., 0] ^ ((c[..., 1] * _HASH_PRIMES[1]) & _U32) ^ ((c[..., 2] * _HASH_PRIMES[2]) & _U32)
    rows = torch.where(hashed[None, :, None], hashed_index, dense) % n_rows[None, :, None] + first[None, :, None]
    per_axis = torch.where(bits[None, None], frac[:, :, None, :], 1 - frac[:, :, None, :])   # [N,16,8,3]
    return rows, per_axis[..., 0] * per_axis[..., 1] * per_axis[..., 2]


def grid_encode(params, x):
    """tiny-cuda-nn's Grid encoding, linear interpolation: params [GRID_PARAMS] (level-major, 2 features per row), x [N,3] -> [N,32]."""
    rows, weights = grid_rows_and_weights(x)
    table = params.reshape(GRID_ROWS, FEATURES_PER_LEVEL)
    return (table[rows] * weights[..., None].to(params.dtype)).sum(2).reshape(x.shape[0], GRID_CHANNELS)


def frequency_embed(x):
    """get_embedder(10, 0): [x, sin(x 1), cos(x 1), sin(x 2), cos(x 2), ..., sin(x 512), cos(x 512)], x [N,3] -> [N,63]."""
    a = x[:, None, :] * (2.0 ** torch.arange(EMBED_FREQS, dtype=x.dtype, device=x.device))[None, :, None]      # [N,10,3]
    return torch.cat([x, torch.stack([torch.sin(a), torch.cos(a)], 2).reshape(x.shape[0], 2 * 3 * EMBED_FREQS)], -1)


def sh_encode(d):
    """torch-ngp's shencoder, degree 4, on the direction as it is (not normalised): d [N,3] -> [N,16]."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
        0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)], -1)


def position_features(params, position):
    """The frame-constant part: position [3] -> [95] = [grid 32 | embedding 63].  Plain torch on a handful of elements; its backward is
    autograd's (an index_add into at most 128 rows of the grid)."""
    x = position.reshape(1, 3).to(params.dtype)
    return torch.cat([grid_encode(params, x), frequency_embed(x)], -1)[0]


def get_rays(H, W, K, c2w, device, dtype):
    """The reference's get_rays [REF scene/env_map.py:113-123] -> (rays_o [H,W,3], rays_d [H,W,3])."""
    K, c2w = torch.as_tensor(K).to(device=device, dtype=dtype), torch.as_tensor(c2w).to(device=device, dtype=dtype)
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=device, dtype=dtype), torch.linspace(0, H - 1, H, device=device, dtype=dtype),
                          indexing="ij")
    i, j = i.t(), j.t()
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    return c2w[:3, -1].expand(rays_d.shape), rays_d


def mlp_torch(layers, x):
    """FCBlock(111, 3, D=3, W=64, relu, sigmoid): layers = [(weight, bias)] * 4."""
    for k, (weight, bias) in enumerate(layers):
        x = F.linear(x, weight, bias)
        x = torch.relu(x) if k < len(layers) - 1 else torch.sigmoid(x)
    return x


def sky_points_torch(params, layers, v, position):
    """SkyModel.forward on flat [N,3] directions and positions, the reference's lines: the full 111-channel input."""
    network_input = torch.cat([sh_encode(v), grid_encode(params, position), frequency_embed(position)], -1)
    return mlp_torch(layers, network_input)


def sky_forward_torch(params, layers, H, W, K, c2w):
    """render_with_camera as the reference writes it, in the dtype and on the device of `params` -> [3,H,W]."""
    rays_o, rays_d = get_rays(H, W, K, c2w, params.device, params.dtype)
    return sky_points_torch(params, layers, rays_d.reshape(-1, 3), rays_o.reshape(-1, 3)).reshape(H, W, 3).permute(2, 0, 1)


# ---- the fused operator ----------------------------------------------------------------------------------------------------------------
WEIGHT_SHAPES = ((HIDDEN, SH_CHANNELS), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (3, HIDDEN), (3,))
WEIGHT_NAMES = ("w0sh", "c", "w1", "b1", "w2", "b2", "w3", "b3")


def camera_tensor(K, c2w, device):
    """[fx, fy, cx, cy, R(9)] as one float32 tensor on `device`, from CPU or GPU K [3,3] and c2w [4,4] ([3,4]): torch ops only, nothing is
    read back to the host."""
    K, c2w = torch.as_tensor(K), torch.as_tensor(c2w)
    intr = torch.stack([K[0][0], K[1][1], K[0][2], K[1][2]]).to(device=device, dtype=torch.float32)
    return torch.cat([intr, c2w[:3, :3].reshape(9).to(device=device, dtype=torch.float32)])


def _checked(cam, H, W, weights):
    if not cam.is_cuda:
        raise L.SurfelRasterError("sky_rays_mlp needs CUDA (ROCm) tensors; there is no CPU path (sky_forward_torch is the checker)")
    if cam.numel() != 13 or H < 0 or W < 0:
        raise ValueError(f"cam must hold [fx, fy, cx, cy, R(9)] and H, W be >= 0; got {tuple(cam.shape)}, H {H}, W {W}")
    if len(weights) != 8:
        raise ValueError("the eight weights are w0sh, c, w1, b1, w2, b2, w3, b3")
    for name, t, shape in zip(WEIGHT_NAMES, weights, WEIGHT_SHAPES):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}; got {tuple(t.shape)}")
    prep = lambda t: t.detach().to(cam.device).contiguous().float()
    return prep(cam), [prep(t) for t in weights]


def sky_workspace(device, max_workgroups=0):
    """The uint8 workspace of a backward with that many workgroups (0: the library's default); its size does not depend on H * W."""
    return _workspace("sr_sky_workspace_bytes", device, int(max_workgroups))


def _launch_forward(cam, H, W, weights, max_workgroups=0, out=None):
    if out is None:
        out = torch.empty((3, H, W), dtype=torch.float32, device=cam.device)
    call("sr_sky_forward", cam.device, W, H, ptr(cam), *[ptr(t) for t in weights], int(max_workgroups), ptr(out))
    return out


def _launch_backward(cam, H, W, weights, g_out, want, max_workgroups=0, workspace=None, out=None):
    dev = cam.device
    if out is None:
        out = tuple(torch.empty(shape, dtype=torch.float32, device=dev) if w else None for shape, w in zip(WEIGHT_SHAPES, want))
    if workspace is None:
        workspace = sky_workspace(dev, max_workgroups)
    call("sr_sky_backward", dev, W, H, ptr(cam), *[ptr(t) for t in weights], ptr(g_out), int(max_workgroups), *buf(workspace), *[ptr(g) for g in out])
    return out


def sky_forward(cam, H, W, *weights, max_workgroups=0, out=None):
    """Raw forward on the current stream -> out [3,H,W] (`out` to write into)."""
    cam, weights = _checked(cam, H, W, weights)
    return _launch_forward(cam, H, W, weights, max_workgroups, out)


def sky_backward(cam, H, W, *weights, g_out, want=(True,) * 8, max_workgroups=0, workspace=None, out=None):
    """Raw backward on the current stream: g_out [3,H,W] -> the eight weight gradients, None where `want` is False (`out`: the eight
    tensors, or None, to write into).  With H * W == 0 nothing is written."""
    cam, weights = _checked(cam, H, W, weights)
    return _launch_backward(cam, H, W, weights, g_out.detach().to(cam.device).contiguous().float(), want, max_workgroups, workspace, out)


class _SkyRaysMlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cam, H, W, max_workgroups, *weights):
        cam_c, weights_c = _checked(cam, H, W, weights)
        out = _launch_forward(cam_c, H, W, weights_c, max_workgroups)
        ctx.save_for_backward(cam_c, *weights_c)
        ctx.call = (H, W, max_workgroups)
        ctx.like = tuple(t.dtype for t in weights)
        return out

    @staticmethod
    def backward(ctx, g_out):
        cam, *weights = ctx.saved_tensors
        H, W, max_workgroups = ctx.call
        want = tuple(ctx.needs_input_grad[4:])
        if H * W == 0:
            grads = [torch.zeros_like(t) if w else None for t, w in zip(weights, want)]
        elif any(want):
            grads = _launch_backward(cam, H, W, weights, g_out.contiguous().float(), want, max_workgroups)
        else:
            grads = [None] * 8
        return (None, None, None, None) + tuple(None if g is None else g.to(dtype) for g, dtype in zip(grads, ctx.like))


def sky_rays_mlp(cam, H, W, w0sh, c, w1, b1, w2, b2, w3, b3, max_workgroups=0):
    """-> [3,H,W]: per pixel the ray direction of camera `cam` (camera_tensor), its 16 SH values, relu(w0sh sh + c), two 64 -> 64 ReLU
    layers, the 64 -> 3 layer and a sigmoid.  Differentiable w.r.t. the eight weights, not the camera.  max_workgroups bounds the
    workgroups of both kernels (0: the library's default); the backward's sum order, not its value, depends on it."""
    return _SkyRaysMlp.apply(cam, int(H), int(W), int(max_workgroups), w0sh, c, w1, b1, w2, b2, w3, b3)


# ---- the module ------------------------------------------------------------------------------------------------------------------------
class _GridEncoding(nn.Module):
    """Holds `params` under the name tiny-cuda-nn's Encoding gives it; uniform in +-1e-4, tiny-cuda-nn's default."""

    def __init__(self, device):
        super().__init__()
        self.params = nn.Parameter((torch.rand(GRID_PARAMS, dtype=torch.float32, device=device) * 2 - 1) * 1e-4)

    def forward(self, x):
        return grid_encode(self.params, x)


class _FCBlock(nn.Module):
    """The reference's FCBlock(111, 3, D=3, W=64): `layers`, four nn.Linear with torch's default initialisation."""

    def __init__(self, device):
        super().__init__()
        widths = [INPUT_CHANNELS, HIDDEN, HIDDEN, HIDDEN, 3]
        self.layers = nn.ModuleList([nn.Linear(widths[k], widths[k + 1], device=device, dtype=torch.float32) for k in range(4)])

    def pairs(self):
        return [(layer.weight, layer.bias) for layer in self.layers]

    def forward(self, x):
        return mlp_torch(self.pairs(), x)


class SkyModel(nn.Module):
    def __init__(self, dir_embed_cfg: dict = {"degree": 4}, D=3, W=64, skips=[], activation="relu", output_activation="sigmoid",
                 num_levels: int = 16, features_per_level: int = 2, weight_norm=False, dtype=torch.float, device=torch.device("cuda")):
        super().__init__()
        given = dict(dir_embed_cfg=dict(dir_embed_cfg), D=D, W=W, skips=list(skips), activation=activation, output_activation=output_activation,
                     num_levels=num_levels, features_per_level=features_per_level, weight_norm=weight_norm, dtype=dtype)
        default = dict(dir_embed_cfg={"degree": 4}, D=3, W=64, skips=[], activation="relu", output_activation="sigmoid", num_levels=16,
                       features_per_level=2, weight_norm=False, dtype=torch.float)
        other = [name for name in default if given[name] != default[name]]
        if other:
            raise ValueError(f"SkyModel is built for the reference's constructor defaults only; not supported: {', '.join(other)}")
        self.position_encoding = _GridEncoding(device)
        self.blocks = _FCBlock(device)
        self.optimizer = torch.optim.Adam(self.parameters(), lr=1e-4)
        self.max_workgroups = 0

    def forward(self, v: torch.Tensor, position: torch.Tensor):
        """Arbitrary per-pixel positions: the torch restatement (nothing in the reference calls the model this way on its hot path)."""
        h, w, _ = v.shape
        return sky_points_torch(self.position_encoding.params, self.blocks.pairs(), v.reshape(-1, 3), position.reshape(-1, 3)).reshape(h, w, 3)

    def render_with_camera(self, H, W, intr, extr):
        params = self.position_encoding.params
        (w0, b0), (w1, b1), (w2, b2), (w3, b3) = self.blocks.pairs()
        extr = torch.as_tensor(extr)
        feat = position_features(params, extr[:3, -1].to(params.device))
        c = w0[:, SH_CHANNELS:] @ feat + b0
        cam = camera_tensor(intr, extr, params.device)
        return sky_rays_mlp(cam, H, W, w0[:, :SH_CHANNELS], c, w1, b1, w2, b2, w3, b3, self.max_workgroups)

    def save(self, path: str):
        torch.save(self.state_dict(), path)

    def load(self, path: str):
        self.load_state_dict(torch.load(path))

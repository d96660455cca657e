"""Shared by tests/test_mask_model_host.py and tests/test_gpu_mask_model.py: the cases of the masked re-optimisation model.

Every comparison on these cases is `==` on every element (torch.equal): the inputs are finite, so an effective value is ONE float32 add
and the mask multiplies by exactly 0 or 1; there is no tolerance to choose.

    P        1, 5, 63, 64, 65, 100, 4097   (100 rows x 45 floats cross the 4096-element Adam chunk in mid-row; 5 rows with an alternating
                                            mask make 16-byte groups straddle selected and unselected rows; 4097 rows: several workgroups)
    degree   0, 1, 2, 3                    (features_rest rows of 0, 9, 24, 45 floats)
    mask     all ones, all zeros, alternating, only the last row, random 10 %, each as bool and as float 0 / 1
    fixed    none, each single property, all six
    offset   one case per degree whose twelve tensors start 4 bytes off a 16-byte boundary (slices of larger buffers): the scalar paths
"""
from collections import namedtuple

import torch

from streetunveiler_amd.mask_model import MASK_PROPERTY, PROPERTIES

PS = (1, 5, 63, 64, 65, 100, 4097)
DEGREES = (0, 1, 2, 3)
MASK_KINDS = ("ones", "zeros", "alternating", "last", "random10")
MASK_DTYPES = (torch.bool, torch.float32)
FIXED = ((),) + tuple((name,) for name in MASK_PROPERTY) + (tuple(MASK_PROPERTY),)

Case = namedtuple("Case", ["P", "degree", "mask_kind", "mask_dtype", "fixed", "offset"])


def cases(P=None):
    """Every (P, degree, mask, mask dtype) with `fixed` cycling through its eight values; every (mask, fixed) pair at P = 5 and 100,
    degree 3; the misaligned cases.  `P`: only the cases of that size."""
    out, k = [], 0
    for p in PS:
        for degree in DEGREES:
            for kind in MASK_KINDS:
                for dtype in MASK_DTYPES:
                    out.append(Case(p, degree, kind, dtype, FIXED[k % len(FIXED)], 0))
                    k += 3      # (3 and 8 are coprime: every fixed set meets every mask kind and dtype)
    for p in (5, 100):
        for kind in MASK_KINDS:
            for fixed in FIXED:
                out.append(Case(p, 3, kind, torch.bool, fixed, 0))
    for degree in DEGREES:
        out.append(Case(65, degree, "alternating", torch.bool, (), 1))
    out.append(Case(100, 3, "random10", torch.float32, ("opacity",), 1))
    return [c for c in out if P is None or c.P == P]


def shapes(P, degree):
    M = (degree + 1) ** 2
    return [(P, 3), (P, 1, 3), (P, M - 1, 3), (P, 1), (P, 2), (P, 4)]


def make_mask(P, kind, dtype=torch.bool, seed=0):
    if kind == "ones":
        m = torch.ones(P, dtype=torch.bool)
    elif kind == "zeros":
        m = torch.zeros(P, dtype=torch.bool)
    elif kind == "alternating":
        m = torch.arange(P) % 2 == 0
    elif kind == "last":
        m = torch.arange(P) == P - 1
    else:
        m = torch.rand(P, generator=torch.Generator().manual_seed(seed + P)) < 0.1
    return m.to(dtype)


def _placed(t, offset, device):
    """`t` on `device`, starting `offset` floats behind the start of its allocation (allocations are at least 16-byte aligned)."""
    if not offset:
        return t.to(device).contiguous()
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=device)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert t.numel() == 0 or view.data_ptr() % 16 == 4 * offset
    return view


def make_tensors(P, degree, device="cpu", dtype=torch.float32, seed=0, offset=0):
    """-> (base, delta): six finite seeded tensors each, in the order of PROPERTIES; drawn on the CPU and moved."""
    r = torch.Generator().manual_seed(1000 * seed + 10 * P + degree)
    base = [_placed(torch.randn(s, generator=r).to(dtype), offset, device) for s in shapes(P, degree)]
    delta = [_placed((0.1 * torch.randn(s, generator=r)).to(dtype), offset, device) for s in shapes(P, degree)]
    return base, delta


def make_upstream(P, degree, device="cpu", dtype=torch.float32, seed=0, offset=0):
    """Seeded gradients of the five effective tensors (xyz, features, opacity, scaling, rotation)."""
    M = (degree + 1) ** 2
    r = torch.Generator().manual_seed(7000 + 1000 * seed + 10 * P + degree)
    return [_placed(torch.randn(s, generator=r).to(dtype), offset, device) for s in [(P, 3), (P, M, 3), (P, 1), (P, 2), (P, 4)]]


def as_leaves(delta):
    return [d.detach().requires_grad_(True) for d in delta]


def delta_gradients(effective, delta, upstream):
    """Gradients of the six deltas for the loss sum(effective * upstream), None where a delta does not reach the outputs."""
    terms = [(e * g).sum() for e, g in zip(effective, upstream) if e.requires_grad]
    if not terms:
        return [None] * 6
    return list(torch.autograd.grad(sum(terms), delta, allow_unused=True))


class TrainingArgs:
    """The fields of the reference's OptimizationParams that training_setup reads [REF arguments/__init__.py]."""
    percent_dense = 0.01
    position_lr_init, position_lr_final, position_lr_delay_mult, position_lr_max_steps = 0.00016, 0.0000016, 0.01, 30000
    feature_lr, opacity_lr, scaling_lr, rotation_lr = 0.0025, 0.05, 0.005, 0.001


class SourceModel:
    """What from_gaussian_model reads of a trained GaussianModel."""

    def __init__(self, P, degree=3, device="cpu", seed=0):
        base, _ = make_tensors(P, degree, device=device, seed=seed)
        self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation = [torch.nn.Parameter(t) for t in base]
        r = torch.Generator().manual_seed(seed + 5)
        self._semantics = torch.randint(0, 6, (P, 1), generator=r).to(device)
        self.max_radii2D = torch.rand(P, generator=r).to(device)
        self.active_sh_degree, self.spatial_lr_scale = degree, 2.5


assert len(PROPERTIES) == 6

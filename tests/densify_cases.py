"""Shared by tests/test_densify_host.py, tests/test_gpu_densify.py, tools/densify_parity.py and tools/time_densify.py: the seeded cases of
the densify-and-prune op, their expectation (streetunveiler_amd.densify.densify_and_prune_torch in float64 on the CPU, computed once per
case), a second, index-based statement of the same semantics (which also produces the wrong implementations the bars must reject), and
THE BARS (`compare`):

  * counts, flags and the source map equal the float64 checker's exactly;
  * copied rows are bit-identical to their source rows: originals, clones, the children's copied attributes, both moments of every
    original, `_semantics` and `cluster_idx`; new rows' moments and all three statistics are exact zeros;
  * child xyz and child _scaling, per case and tensor: the largest deviation from the float64 checker is at most twice the float32 torch
    restatement's own deviation from it on that case (two float32 evaluations of the same handful of operations differ in rounding order
    only), with a floor of one float32 ulp of the largest magnitude in that tensor of the case, all its rows taken (the restatement may
    happen to land nearer than float32 arithmetic can promise, and a child scale log(exp(s) / 1.6) carries the rounding of
    exp(s) / 1.6 as an ABSOLUTE error, whatever its own size.  exact_ties is that case: every child scale is log(1.3 / 1.6) = -0.21;
    the kernel and the restatement take the same correctly rounded exp, the kernel then divides by 1.6 (the IEEE division; torch on the
    CPU gives the same value, 8.0e-8 off), torch's GPU kernel multiplies by the rounded reciprocal of the Python scalar 1.6 and at
    this input lands on the correctly rounded end result (5.4e-9 off): luck at one number, not the same operations).
    Non-finite values (an all-zero rotation gives NaN positions) must be non-finite in the same places.

Every case keeps each compared quantity at least MARGIN (relative) away from its threshold, except the rows a case names as exact ties:
a condition on the inputs, asserted on the float64 values by `assert_margins` -- zero non-robust rows per case."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from streetunveiler_amd import densify as D
from streetunveiler_amd.optim import adam_step_float64
from tests import optim_cases as oc

MARGIN = 1e-4
SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 5000)      # wave edges, scan-block edges, several scan blocks
F32 = lambda x: float(np.float32(x))
DEFAULT = dict(max_grad=F32(0.0002), min_opacity=F32(0.005), extent=F32(5.0), max_screen_size=20, percent_dense=F32(0.01))


def _away(x, threshold, factor=1.01):
    """x (positive) with every element within 1e-3 (relative) of `threshold` moved off it."""
    near = (x / threshold - 1).abs() < 1e-3
    return torch.where(near, x * factor, x)


def make_case(P, rest=45, state=True, seed=0, grad_range=(1e-6, 1e-2), scale_range=(0.005, 2.0), logit_range=(-8.0, 4.0), ties=None, **thresholds):
    """float32 / int tensors on the CPU.  Gradients, scales and opacities log-uniform / uniform over ranges that straddle the thresholds."""
    th = dict(DEFAULT, **thresholds)
    r = torch.Generator().manual_seed(1000 * seed + P)
    rand = lambda *s: torch.rand(*s, generator=r, dtype=torch.float64)
    randn = lambda *s: torch.randn(*s, generator=r)
    log_uniform = lambda lo, hi, *s: torch.exp(rand(*s) * math.log(hi / lo) + math.log(lo))
    pde, ws = th["percent_dense"] * th["extent"], 0.1 * th["extent"]
    denom = torch.randint(1, 50, (P, 1), generator=r).float()
    grad = _away(log_uniform(*grad_range, P, 1), th["max_grad"])
    accum = (grad * denom.double()).float()
    scale = log_uniform(*scale_range, P, 2)
    for t in (pde, ws, 1.6 * ws):
        scale = _away(scale, t)
    opacity = rand(P, 1) * (logit_range[1] - logit_range[0]) + logit_range[0]
    opacity = torch.where((torch.sigmoid(opacity) / th["min_opacity"] - 1).abs() < 1e-3, opacity + 0.05, opacity)
    params = {"xyz": 3 * randn(P, 3), "f_dc": randn(P, 1, 3), "f_rest": randn(P, rest // 3, 3), "opacity": opacity.float(),
              "scaling": torch.log(scale).float(), "rotation": randn(P, 4)}
    moments = {k: ((0.1 * randn(*v.shape), 0.01 * rand(*v.shape).float()) if state else None) for k, v in params.items()}
    return SimpleNamespace(P=P, params=params, moments=moments, semantics=torch.randint(0, 1 << 20, (P, 1), generator=r, dtype=torch.int32),
                           cluster_idx=torch.randint(-1, P + 1, (P,), generator=r, dtype=torch.int64), accum=accum, denom=denom,
                           max_radii2D=torch.randint(0, 200, (P,), generator=r).float(), th=th, ties=dict(ties or {}), noise_seed=seed + 7)


def _set_scale(c, rows, value):
    c.params["scaling"][rows] = torch.log(torch.as_tensor(value, dtype=torch.float64)).float()


def _special_values():
    c = make_case(700, seed=3)
    c.denom[:40] = 0
    c.accum[:20] = 0                                     # 0/0 -> 0: not selected
    c.accum[20:40] = torch.linspace(1e-9, 3.0, 20).reshape(-1, 1)      # x/0 -> +inf: selected
    _set_scale(c, slice(20, 30), 0.3)                    # ... and split (0.05 < 0.3, 0.3 / 1.6 < 0.5) ...
    _set_scale(c, slice(30, 40), 0.01)                   # ... or cloned
    c.params["opacity"][20:40] = 2.0
    c.params["rotation"][20:25] *= 10.0                  # far from unit length on split parents
    c.params["rotation"][25:28] = 0.0                    # |q| = 0: NaN positions, in the checker too
    c.accum[40:60] = -1.0                                # a negative quotient (-1/0 = -inf in rows 50..59): the clone tests its norm,
    c.denom[50:60] = 0                                   # the split its signed value
    _set_scale(c, slice(40, 60, 2), 0.3)                 # ... so these are not split ...
    _set_scale(c, slice(41, 60, 2), 0.01)                # ... and these are cloned
    c.params["opacity"][40:60] = 2.0
    return c


def _exact_ties():
    """accum = t * denom with denom in {1, 2, 4}: >= selects.  _scaling = 0 with percent_dense * extent == 1.0: clone, not split.
    _opacity = 0 with min_opacity = 0.5: kept."""
    t = F32(0.0002)
    c = make_case(300, seed=4, max_grad=t, min_opacity=0.5, extent=2.0, percent_dense=0.5, max_screen_size=None, scale_range=(0.005, 0.5))
    assert c.th["percent_dense"] * c.th["extent"] == 1.0
    rows = torch.arange(0, 90, 3)
    c.denom[rows] = torch.tensor([1.0, 2.0, 4.0]).repeat(10).reshape(-1, 1)
    c.accum[rows] = np.float32(t) * c.denom[rows]
    assert torch.equal((c.accum[rows].double() / c.denom[rows].double()), torch.full((30, 1), t, dtype=torch.float64))
    c.params["scaling"][rows[:15]] = 0.0                 # exp(0) = 1 <= 1.0: clone
    _set_scale(c, rows[15:], 1.3)                        # split
    c.params["opacity"][rows[::2]] = 0.0                 # sigmoid(0) = 0.5, not < 0.5: kept
    c.params["opacity"][rows[1::2]] = 1.0
    c.ties = {"grad": rows, "scale": rows[:15], "opacity": rows[::2]}
    return c


def _clone_and_pruned():
    c = make_case(700, seed=5, grad_range=(1e-3, 1e-2), scale_range=(0.005, 0.04))      # everything clone-selected
    c.params["opacity"][::2] = -7.0                      # sigmoid(-7) < 0.005: the parent goes, and its clone with it
    return c


def _screen(max_screen_size):
    c = make_case(700, seed=6, scale_range=(0.005, 0.4), max_screen_size=max_screen_size)       # nothing beyond 0.1 * extent
    c.max_radii2D[:] = 1000.0
    return c


CASES = {
    "nothing": lambda: make_case(700, seed=1, grad_range=(1e-6, 1e-5), logit_range=(-4.0, 4.0), max_screen_size=None),
    "all_cloned": lambda: make_case(700, seed=2, grad_range=(1e-3, 1e-2), scale_range=(0.005, 0.04), logit_range=(-4.0, 4.0)),
    "all_split": lambda: make_case(700, seed=2, grad_range=(1e-3, 1e-2), scale_range=(0.06, 0.4), logit_range=(-4.0, 4.0)),
    "all_pruned": lambda: make_case(700, seed=2, logit_range=(-9.0, -6.0)),
    "clone_and_pruned": _clone_and_pruned,
    "children_still_big": lambda: make_case(700, seed=2, grad_range=(1e-3, 1e-2), scale_range=(0.9, 2.0), logit_range=(-4.0, 4.0)),
    "screen_none": lambda: _screen(None),
    "screen_20": lambda: _screen(20),
    "special_values": _special_values,
    "exact_ties": _exact_ties,
}
for _P in SIZES:
    for _rest in (45, 0):
        for _state in (True, False):
            CASES[f"P{_P}_rest{_rest}_{'state' if _state else 'nostate'}"] = functools.partial(make_case, _P, _rest, _state, seed=10)
# the two loops only a large model enters: more than 256 blocks of 256 Gaussians (the carry of the totals scan), and more than 4096 chunks
# of 4096 words in one gather launch (its grid stride: f_rest with both moments, nothing pruned)
CASES["P70000_rest0_nostate"] = functools.partial(make_case, 70000, 0, False, seed=11)
for _P in (65536, 65537):      # 256 and 257 blocks: the last item of the totals scan's first chunk, the first of its second
    CASES[f"P{_P}_rest0_nostate"] = functools.partial(make_case, _P, 0, False, seed=13)
CASES["P131073_rest45_state"] = functools.partial(make_case, 131073, 45, True, seed=12, scale_range=(0.005, 0.4), logit_range=(-4.0, 4.0))
MIXES = [n for n in CASES if not n.startswith("P")]


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    assert_margins(c, name)
    return c


def noise_for(c, S):
    return torch.randn((2 * S, 2), generator=torch.Generator().manual_seed(c.noise_seed))


def _decisions(c, dtype=torch.float64, mutant=None):
    """The masks of the semantics, stated per input row (ISSUE points 1-5): clone, split, keep_self, keep_child, and the quantities
    they compare."""
    th = c.th
    g = c.accum.to(dtype).reshape(-1) / c.denom.to(dtype).reshape(-1)
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    above = (lambda x: x > th["max_grad"]) if mutant == "> for >=" else (lambda x: x >= th["max_grad"])
    clone_selected, split_selected = above(g.abs()), above(g)      # the reference: the norm for the clone, the signed value for the split
    e = torch.exp(c.params["scaling"].to(dtype))
    big = e.max(dim=1).values if c.P else e.new_zeros(0)
    pde, ws = th["percent_dense"] * th["extent"], 0.1 * th["extent"]
    clone, split = clone_selected & (big <= pde), split_selected & (big > pde)
    alpha = torch.sigmoid(c.params["opacity"].to(dtype)).reshape(-1)
    pruned = alpha < th["min_opacity"]
    child_scaling = torch.log(e / (0.8 if mutant == "scale / 0.8" else 1.6))
    child_big = torch.exp(child_scaling).max(dim=1).values if c.P else big
    world = bool(th["max_screen_size"])
    self_pruned = pruned | (world & (big > ws))
    child_pruned = pruned | (world & (child_big > ws))
    if mutant == "max_radii2D honoured" and world:
        self_pruned = self_pruned | (c.max_radii2D > th["max_screen_size"])
        child_pruned = child_pruned | (c.max_radii2D > th["max_screen_size"])
    return SimpleNamespace(grad=g.abs(), big=big, child_big=child_big, alpha=alpha, clone=clone, split=split, keep_self=~split & ~self_pruned,
                           keep_child=split & ~child_pruned, child_scaling=child_scaling, pde=pde, ws=ws, world=world)


def assert_margins(c, what=""):
    """Every compared quantity at least MARGIN (relative) from its threshold, the rows named in c.ties excepted: zero non-robust rows."""
    d = _decisions(c)
    exempt = lambda key: torch.zeros(c.P, dtype=torch.bool).index_fill_(0, torch.as_tensor(c.ties.get(key, []), dtype=torch.int64), True)
    checks = [("grad", d.grad, c.th["max_grad"], "grad"), ("scale", d.big, d.pde, "scale"), ("opacity", d.alpha, c.th["min_opacity"], "opacity")]
    if d.world:
        checks += [("scale vs world size", d.big, d.ws, None), ("child scale vs world size", d.child_big, d.ws, None)]
    for label, x, threshold, key in checks:
        near = ((x / threshold - 1).abs() < MARGIN) & ~(exempt(key) if key else torch.zeros(c.P, dtype=torch.bool))
        assert not near.any(), f"{what}: {int(near.sum())} non-robust row(s) for {label}: {near.nonzero().reshape(-1)[:5].tolist()}"
    for key, x, threshold in (("grad", d.grad, c.th["max_grad"]), ("scale", d.big, d.pde), ("opacity", d.alpha, c.th["min_opacity"])):
        rows = torch.as_tensor(c.ties.get(key, []), dtype=torch.int64)
        assert bool((x[rows] == threshold).all()), f"{what}: the {key} ties are not exact"


def by_index(c, dtype=torch.float64, mutant=None):
    """The same semantics as one gather per tensor (ISSUE points 1-7), independent of the line-by-line checker; `mutant` names one of the
    wrong implementations of MUTANTS."""
    d = _decisions(c, dtype, mutant)
    idx = torch.arange(c.P)
    kept, clones, children = idx[d.keep_self], idx[d.keep_self & d.clone], idx[d.keep_child]
    H = len(children)
    if mutant == "children parent by parent":
        pairs, pair_kind = children.repeat_interleave(2), torch.tensor([D.KIND_CHILD0, D.KIND_CHILD1]).repeat(H)
    else:
        pairs, pair_kind = children.repeat(2), torch.tensor([D.KIND_CHILD0] * H + [D.KIND_CHILD1] * H)
    source = torch.cat([kept, clones, pairs])
    kind = torch.cat([torch.full((len(kept),), D.KIND_ORIGINAL), torch.full((len(clones),), D.KIND_CLONE), pair_kind]).to(torch.int64)
    S = int(d.split.sum())
    rank = torch.cumsum(d.split, 0) - 1                  # j of a split-selected row
    noise = noise_for(c, S).to(dtype)
    p = {k: v.to(dtype)[source] for k, v in c.params.items()}
    is_child = kind >= D.KIND_CHILD0
    par, k_of = source[is_child], kind[is_child] - D.KIND_CHILD0
    n = noise[k_of * S + rank[par]]
    q = c.params["rotation"].to(dtype)[par]
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    r, x, y, z = q.unbind(dim=1)
    e = torch.exp(c.params["scaling"].to(dtype)[par])
    v0, v1 = e[:, 0] * n[:, 0], e[:, 1] * n[:, 1]
    offset = torch.stack([(1 - 2 * (y * y + z * z)) * v0 + 2 * (x * y - r * z) * v1, 2 * (x * y + r * z) * v0 + (1 - 2 * (x * x + z * z)) * v1,
                          2 * (x * z - r * y) * v0 + 2 * (y * z + r * x) * v1], dim=1)
    p["xyz"][is_child] = offset + c.params["xyz"].to(dtype)[par]
    p["scaling"][is_child] = d.child_scaling[par]
    new = kind != D.KIND_ORIGINAL
    if mutant == "moments of clones copied":
        new = kind >= D.KIND_CHILD0
    m = {}
    for k, st in c.moments.items():
        m[k] = None if st is None else tuple(torch.where(new.reshape([-1] + [1] * (s.dim() - 1)), torch.zeros((), dtype=dtype), s.to(dtype)[source]) for s in st)
    flags = (d.clone * D.FLAG_CLONE + d.split * D.FLAG_SPLIT + d.keep_self * D.FLAG_KEEP_SELF + d.keep_child * D.FLAG_KEEP_CHILD).to(torch.uint8)
    n_out = len(source)
    return D.Densified(p, m, c.semantics[source], (c.cluster_idx[source],), torch.zeros(n_out, 1, dtype=dtype), torch.zeros(n_out, 1, dtype=dtype),
                       torch.zeros(n_out, dtype=dtype), (len(kept), len(clones), S, H), flags, source, kind)


MUTANTS = ("children parent by parent", "max_radii2D honoured", "moments of clones copied", "> for >=", "scale / 0.8")


def run_checker(c, dtype=torch.float64, device="cpu"):
    """densify_and_prune_torch on the case's tensors in `dtype` on `device`."""
    to = lambda t: t.to(device=device, dtype=dtype)
    S = int(_decisions(c).split.sum())
    moments = {k: (None if st is None else tuple(to(s) for s in st)) for k, st in c.moments.items()}
    return D.densify_and_prune_torch({k: to(v) for k, v in c.params.items()}, moments, c.semantics.to(device), to(c.accum), to(c.denom),
                                     to(c.max_radii2D), c.th["max_grad"], c.th["min_opacity"], c.th["extent"], c.th["max_screen_size"],
                                     c.th["percent_dense"], to(noise_for(c, S)), extra_rows=(c.cluster_idx.to(device),))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The float64 checker's result for a case, computed once and shared."""
    return run_checker(case(name))


# ---- the bars ------------------------------------------------------------------------------------------------------------------------
def _cpu32(t):
    t = t.detach().cpu()
    return t.float() if t.dtype == torch.float64 else t


def _same_bits(a, b, what):
    a, b = _cpu32(a), _cpu32(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype} {list(a.shape)} against {b.dtype} {list(b.shape)}"
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    assert torch.equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} element(s) differ in their bits"


def _within_bar(got, want, ref, largest, what):
    """-> (deviation of got, deviation of ref, bound); asserts the bar of the module docstring.  `largest`: the largest finite magnitude
    of the whole tensor in the checker's result."""
    got, want = _cpu32(got).double(), want.detach().cpu().double()
    finite = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~finite].nan_to_num(), want[~finite].nan_to_num()), \
        f"{what}: non-finite at other elements than the float64 checker"
    if not finite.any():
        return 0.0, 0.0, 0.0
    dev = float((got - want)[finite].abs().max())
    dev_ref = 0.0
    if ref is not None:
        diff = (_cpu32(ref).double() - want)[finite]
        dev_ref = float(diff[torch.isfinite(diff)].abs().max()) if torch.isfinite(diff).any() else 0.0
    floor = float(np.spacing(np.float32(largest)))
    bound = max(2.0 * dev_ref, floor)
    print(f"{what}: deviation {dev:.3e}, float32 restatement {dev_ref:.3e}, one ulp {floor:.3e}, bound {bound:.3e}")
    assert dev <= bound, f"{what}: off by {dev:.3e} from the float64 checker, beyond {bound:.3e} (float32 restatement: {dev_ref:.3e}, one ulp: {floor:.3e})"
    return dev, dev_ref, bound


def compare(got, want, ref32=None, what=""):
    """The bars of the module docstring: `got` (the op's Densified, or a wrong implementation's) against `want` (the float64 checker's);
    `ref32`: the float32 torch restatement's result on the same case, or None (then the bar of the computed rows is its one-ulp floor).
    -> {tensor: (deviation, deviation of ref32, bound)} for the two computed tensors."""
    assert tuple(got.counts) == tuple(want.counts), f"{what}: counts {tuple(got.counts)} against {tuple(want.counts)}"
    for name in ("flags", "source", "kind"):
        a, b = getattr(got, name).cpu(), getattr(want, name).cpu()
        assert a.shape == b.shape and torch.equal(a.to(torch.int64), b.to(torch.int64)), f"{what}: {name} differs from the checker's"
    if ref32 is not None:
        assert torch.equal(ref32.source.cpu(), want.source) and torch.equal(ref32.kind.cpu(), want.kind), f"{what}: the float32 restatement decided otherwise"
    child = want.kind.cpu() >= D.KIND_CHILD0
    out = {}
    assert sorted(got.params) == sorted(want.params) and sorted(got.moments) == sorted(want.moments), f"{what}: group names"
    for k, w in want.params.items():
        g = got.params[k]
        assert g.shape == w.shape, f"{what}: {k} is {list(g.shape)}, the checker's {list(w.shape)}"
        if k in ("xyz", "scaling"):
            _same_bits(g.detach().cpu()[~child], w[~child], f"{what}: copied rows of {k}")
            largest = float(w[torch.isfinite(w)].abs().max()) if torch.isfinite(w).any() else 0.0
            out[k] = _within_bar(g.detach().cpu()[child], w[child], None if ref32 is None else ref32.params[k].detach().cpu()[child], largest,
                                 f"{what}: child {k}")
        else:
            _same_bits(g, w, f"{what}: {k}")
        assert (got.moments[k] is None) == (want.moments[k] is None), f"{what}: moments of {k} present / absent"
        if want.moments[k] is not None:
            for key, a, b in zip(("exp_avg", "exp_avg_sq"), got.moments[k], want.moments[k]):
                _same_bits(a, b, f"{what}: {key} of {k}")
    _same_bits(got.semantics, want.semantics, f"{what}: semantics")
    assert len(got.extra_rows) == len(want.extra_rows)
    for i, (a, b) in enumerate(zip(got.extra_rows, want.extra_rows)):
        _same_bits(a, b, f"{what}: extra_rows[{i}]")
    for name in ("xyz_gradient_accum", "denom", "max_radii2D"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and not _cpu32(a).view(torch.int32).any(), f"{what}: {name} is not zeros of the new size"
    return out


# ---- a model shaped like the reference's GaussianModel -----------------------------------------------------------------------------------
class CheckerAdam(torch.optim.Optimizer):
    """Adam whose step is streetunveiler_amd.optim.adam_step_float64, with torch.optim.Adam's state layout."""

    def __init__(self, params, lr=1e-3, betas=oc.BETAS, eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state["step"], state["exp_avg"], state["exp_avg_sq"] = torch.tensor(0.0), torch.zeros_like(p), torch.zeros_like(p)
                state["step"] += 1
                adam_step_float64([p], [p.grad], [state["exp_avg"]], [state["exp_avg_sq"]], [group["lr"]], [float(state["step"])],
                                  *group["betas"], group["eps"])


class Model:
    """The attributes densify_and_prune / prune_points read and write, over an optimizer with the reference's six named groups."""

    def __init__(self, c, optimizer_class, device, dtype, with_optimizer=True, **kw):
        tensors = [c.params[name] for name, _, _ in oc.GROUPS]
        self.optimizer, named = oc.make_optimizer(optimizer_class, tensors, device, dtype, **kw)
        for name, p in named.items():
            setattr(self, D._ATTRIBUTE[name], p)
        if not with_optimizer:
            self.optimizer = None
        self._semantics, self.cluster_idx = c.semantics.to(device), c.cluster_idx.to(device)
        self.xyz_gradient_accum, self.denom = c.accum.to(device=device, dtype=dtype), c.denom.to(device=device, dtype=dtype)
        self.max_radii2D = c.max_radii2D.to(device=device, dtype=dtype)
        self.percent_dense = c.th["percent_dense"]

    def named(self):
        return {name: getattr(self, attr) for name, attr in D._ATTRIBUTE.items()}

    def moments(self):
        out = {}
        for name, p in self.named().items():
            state = None if self.optimizer is None else self.optimizer.state.get(p, None)
            out[name] = (state["exp_avg"], state["exp_avg_sq"]) if state else None
        return out

    def _install(self, params, moments):
        for group in (self.optimizer.param_groups if self.optimizer is not None else []):
            name, old = group["name"], group["params"][0]
            stored_state = self.optimizer.state.get(old, None)
            new = torch.nn.Parameter(params[name].requires_grad_(True))
            if stored_state is not None:
                stored_state["exp_avg"], stored_state["exp_avg_sq"] = moments[name]
                del self.optimizer.state[old]
                self.optimizer.state[new] = stored_state
            group["params"][0] = new
            params[name] = new
        for name, t in params.items():
            setattr(self, D._ATTRIBUTE[name], t if isinstance(t, torch.nn.Parameter) else torch.nn.Parameter(t.requires_grad_(True)))

    def reference_densify(self, max_grad, min_opacity, extent, max_screen_size, noise, bookkeeping=True):
        """The reference's densify_and_prune on this model, through densify_and_prune_torch in the model's dtype."""
        named = self.named()
        r = D.densify_and_prune_torch(named, self.moments(), self._semantics, self.xyz_gradient_accum, self.denom, self.max_radii2D, max_grad,
                                      min_opacity, extent, max_screen_size, self.percent_dense, noise.to(named["xyz"].device), extra_rows=(self.cluster_idx,),
                                      bookkeeping=bookkeeping)
        self._install(dict(r.params), r.moments)
        self._semantics, (self.cluster_idx,) = r.semantics, r.extra_rows
        self.xyz_gradient_accum, self.denom, self.max_radii2D = r.xyz_gradient_accum, r.denom, r.max_radii2D
        return r

    def reference_prune(self, mask):
        """The reference's prune_points(mask) on this model [REF scene/gaussian_model.py:402-450]."""
        valid = ~mask.to(self._xyz.device)
        moments = {k: (None if st is None else tuple(s[valid] for s in st)) for k, st in self.moments().items()}
        self._install({k: p.detach()[valid] for k, p in self.named().items()}, moments)
        self._semantics, self.cluster_idx = self._semantics[valid], self.cluster_idx[valid]
        self.xyz_gradient_accum, self.denom, self.max_radii2D = self.xyz_gradient_accum[valid], self.denom[valid], self.max_radii2D[valid]


def model_case_from(model, th):
    """The case a float64 CPU model stands for right now (for assert_margins before a model-level densification)."""
    params = {k: p.detach() for k, p in model.named().items()}
    return SimpleNamespace(P=params["xyz"].shape[0], params=params, accum=model.xyz_gradient_accum, denom=model.denom, max_radii2D=model.max_radii2D,
                           th=th, ties={})

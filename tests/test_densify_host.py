"""CPU: the float64 checker of the densify-and-prune op against a hand-written expectation and against an independent, index-based
statement of the same semantics on every case of tests/densify_cases.py; the bars reject the wrong implementations one can think of; the
C-ABI of the op is declared, exported and refuses bad arguments before it touches a GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

from streetunveiler_amd import densify as D
from tests import densify_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(dc.CASES)


def test_checker_against_a_hand_written_expectation():
    """Six Gaussians: kept, cloned, split, pruned, cloned and pruned, split with pruned children.  max_grad 0.5, min_opacity 0.1,
    percent_dense * extent = 0.1, world-size limit 0.1 * extent = 1."""
    f = torch.float64
    grads = torch.tensor([0.1, 1.0, 2.0, 0.1, 1.0, 2.0], dtype=f)
    denom = torch.tensor([1.0, 2.0, 4.0, 1.0, 3.0, 5.0], dtype=f).reshape(-1, 1)
    scales = torch.tensor([[0.05, 0.02], [0.05, 0.08], [0.4, 0.2], [0.05, 0.02], [0.05, 0.08], [2.0, 0.3]], dtype=f)
    opacity = torch.tensor([2.0, 2.0, 2.0, -3.0, -3.0, 2.0], dtype=f).reshape(-1, 1)
    xyz = torch.tensor([[0.0, 0, 0], [10, 11, 12], [1, 2, 3], [7, 7, 7], [8, 8, 8], [9, 9, 9]], dtype=f)
    rotation = torch.tensor([[1.0, 0, 0, 0]] * 6, dtype=f)
    rotation[2] = torch.tensor([1.0, 0, 0, 1.0])       # a quarter turn about z, not normalised: (v0, v1, 0) -> (-v1, v0, 0)
    f_dc, f_rest = torch.arange(18, dtype=f).reshape(6, 1, 3), torch.arange(36, dtype=f).reshape(6, 2, 3)
    params = {"xyz": xyz, "f_dc": f_dc, "f_rest": f_rest, "opacity": opacity, "scaling": torch.log(scales), "rotation": rotation}
    moments = {k: (v + 100, v + 200) for k, v in params.items()}
    semantics = torch.tensor([[10], [11], [12], [13], [14], [15]], dtype=torch.int32)
    cluster = torch.tensor([20, 21, 22, 23, 24, 25])
    noise = torch.tensor([[1.0, 2.0], [9.0, 9.0], [-1.0, 0.5], [9.0, 9.0]], dtype=f)      # rows k * S + j: j = 0 is Gaussian 2, j = 1 Gaussian 5
    r = D.densify_and_prune_torch(params, moments, semantics, grads.reshape(-1, 1) * denom, denom, torch.full((6,), 1000.0, dtype=f), 0.5, 0.1,
                                  10.0, 20, 0.01, noise, extra_rows=(cluster,))
    assert r.counts == (2, 1, 2, 1)
    assert r.source.tolist() == [0, 1, 1, 2, 2] and r.kind.tolist() == [0, 0, 1, 2, 3]
    C, S, KS, KC = D.FLAG_CLONE, D.FLAG_SPLIT, D.FLAG_KEEP_SELF, D.FLAG_KEEP_CHILD
    assert r.flags.tolist() == [KS, C | KS, S | KC, 0, C, S]
    want_xyz = torch.tensor([[0.0, 0, 0], [10, 11, 12], [10, 11, 12], [1 - 0.2 * 2, 2 + 0.4 * 1, 3], [1 - 0.2 * 0.5, 2 - 0.4 * 1, 3]], dtype=f)
    assert torch.allclose(r.params["xyz"], want_xyz, rtol=0, atol=1e-14) and torch.equal(r.params["xyz"][:3], want_xyz[:3])
    want_scaling = torch.log(torch.tensor([[0.05, 0.02], [0.05, 0.08], [0.05, 0.08], [0.25, 0.125], [0.25, 0.125]], dtype=f))
    assert torch.allclose(r.params["scaling"], want_scaling, rtol=0, atol=1e-14) and torch.equal(r.params["scaling"][:3], torch.log(scales)[[0, 1, 1]])
    rows = [0, 1, 1, 2, 2]
    for k in ("f_dc", "f_rest", "opacity", "rotation"):
        assert torch.equal(r.params[k], params[k][rows]), k
    for k in params:
        for which, (got, src) in enumerate(zip(r.moments[k], moments[k])):
            assert torch.equal(got[:2], src[:2]) and not got[2:].any() and got.shape == r.params[k].shape, (k, which)
    assert r.semantics.tolist() == [[10], [11], [11], [12], [12]] and r.semantics.dtype == torch.int32
    assert r.extra_rows[0].tolist() == [20, 21, 21, 22, 22]
    for t, shape in ((r.xyz_gradient_accum, (5, 1)), (r.denom, (5, 1)), (r.max_radii2D, (5,))):
        assert tuple(t.shape) == shape and not t.any()
    # without a max_screen_size the world-size test is off: the children of Gaussian 5 survive too
    r2 = D.densify_and_prune_torch(params, {k: None for k in params}, semantics, grads.reshape(-1, 1) * denom, denom, torch.zeros(6, dtype=f), 0.5, 0.1,
                                   10.0, None, 0.01, noise)
    assert r2.counts == (2, 1, 2, 2) and r2.source.tolist() == [0, 1, 1, 2, 5, 2, 5] and all(v is None for v in r2.moments.values())
    with pytest.raises(ValueError, match="noise"):
        D.densify_and_prune_torch(params, moments, semantics, grads.reshape(-1, 1) * denom, denom, torch.zeros(6, dtype=f), 0.5, 0.1, 10.0, 20, 0.01, noise[:2])


@pytest.mark.parametrize("name", ALL)
def test_checker_equals_the_index_statement(name):
    """Two statements of the semantics, written independently (the reference's lines in order; one gather per tensor), agree on every
    case under the bars themselves -- and the inputs keep their margins (asserted when the case is built)."""
    c, want = dc.case(name), dc.expected(name)
    other = dc.by_index(c)
    dc.compare(other, want, None, name)      # (rounds the float64 values to float32, as for the op)
    assert want.params["xyz"].shape[0] == want.counts[0] + want.counts[1] + 2 * want.counts[3]
    for k in ("xyz", "scaling"):             # the computed rows, in float64
        assert torch.allclose(other.params[k], want.params[k], rtol=1e-13, atol=1e-13, equal_nan=True), k


def test_what_the_named_cases_are_there_for():
    P = 700
    nothing, c = dc.expected("nothing"), dc.case("nothing")
    assert nothing.counts == (P, 0, 0, 0) and all(torch.equal(nothing.params[k], c.params[k].double()) for k in c.params)
    assert dc.expected("all_cloned").counts[2:] == (0, 0) and dc.expected("all_cloned").flags.bitwise_and(D.FLAG_CLONE).all()
    assert dc.expected("all_split").counts[:3] == (0, 0, P) and dc.expected("all_split").counts[3] > 0
    assert dc.expected("all_pruned").counts in ((0, 0, s, 0) for s in range(P + 1)) and dc.expected("all_pruned").params["xyz"].shape[0] == 0
    cp = dc.expected("clone_and_pruned")
    assert cp.counts[0] == cp.counts[1] < P and cp.flags.bitwise_and(D.FLAG_CLONE).all() and not cp.flags[::2].bitwise_and(D.FLAG_KEEP_SELF).any()
    big = dc.expected("children_still_big")
    assert big.counts == (0, 0, P, 0)
    a, b = dc.expected("screen_none"), dc.expected("screen_20")
    assert a.counts == b.counts and a.counts[3] > 0 and torch.equal(a.source, b.source) and all(torch.equal(a.params[k], b.params[k]) for k in a.params)
    sp = dc.expected("special_values")
    assert not sp.flags[:20].bitwise_and(D.FLAG_CLONE | D.FLAG_SPLIT).any()                  # 0/0 -> 0
    assert sp.flags[20:30].bitwise_and(D.FLAG_SPLIT).all() and sp.flags[30:40].bitwise_and(D.FLAG_CLONE).all()      # x/0 -> +inf
    assert int(torch.isnan(sp.params["xyz"]).all(dim=1).sum()) == 6                          # three parents without a rotation, two children each
    assert not sp.flags[40:60:2].bitwise_and(D.FLAG_CLONE | D.FLAG_SPLIT).any() and sp.flags[41:60:2].bitwise_and(D.FLAG_CLONE).all()   # negative quotients
    ties, tc = dc.expected("exact_ties"), dc.case("exact_ties")
    rows = tc.ties["grad"]
    assert ties.flags[rows[:15]].bitwise_and(D.FLAG_CLONE).all() and ties.flags[rows[15:]].bitwise_and(D.FLAG_SPLIT).all()
    assert ties.flags[rows[:15:2]].bitwise_and(D.FLAG_KEEP_SELF).all()
    assert (70000 + 255) // 256 > 256                                                        # the totals scan carries between its rounds
    rows_out = dc.expected("P131073_rest45_state").params["xyz"].shape[0]
    assert 3 * ((rows_out + 4096 // 45 - 1) // (4096 // 45)) > 4096                        # f_rest with its moments: the gather grid strides
    for P_ in dc.SIZES:
        assert dc.expected(f"P{P_}_rest45_state").flags.shape == (P_,)
    mixed = dc.expected("P5000_rest45_state").counts
    assert all(n > 100 for n in mixed) and sum(mixed[:1]) < 5000


@pytest.mark.parametrize("mutant", dc.MUTANTS)
def test_the_bars_reject_wrong_implementations(mutant):
    failed = []
    for name in dc.MIXES + ["P5000_rest45_state"]:
        try:
            dc.compare(dc.by_index(dc.case(name), mutant=mutant), dc.expected(name), None, name)
        except AssertionError:
            failed.append(name)
    print(f"{mutant}: fails {len(failed)} cases: {failed}")
    assert failed, f"no case tells '{mutant}' from the checker"


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from streetunveiler_amd import _lib
    from streetunveiler_amd.build import build
    build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_listed(lib):
    import streetunveiler_amd
    from streetunveiler_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "surfel_raster.h")).read(), flags=re.S)
    for name in ("sr_densify_workspace_bytes", "sr_densify_plan", "sr_densify_apply"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.sr_abi_version() == 10      # an addition: nothing that existed changed
    for name in ("densify_and_prune", "prune_points", "densify_and_prune_tensors", "densify_and_prune_torch"):
        assert name in streetunveiler_amd.__all__ and callable(getattr(streetunveiler_amd, name))
    from streetunveiler_amd.build import SOURCES
    assert ("densify.hip", ["-ffp-contract=off"]) in [(s, list(f)) for s, f in SOURCES]
    for name in ("SR_DENSIFY_MAX_SEGMENTS", "SR_DENSIFY_FLAG_KEEP_CHILD", "SR_DENSIFY_KIND_CHILD1", "SR_DENSIFY_ROLE_SCALING"):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == getattr(_lib, name), name
    assert ctypes.sizeof(_lib.SrDensifySegment) == 24


def test_workspace_size_grows_with_the_model(lib):
    sizes = [lib.sr_densify_workspace_bytes(n) for n in (-5, 0, 1, 255, 256, 257, 100000, 3000000)]
    assert sizes[0] == sizes[1] > 0 and sizes == sorted(sizes)
    assert 13 * 3000000 <= sizes[-1] <= 14 * 3000000      # flags, two map words and one rank word per Gaussian, the block totals


def test_argument_refusals_without_gpu(lib):
    """Every refusal comes before the first HIP call, or this test could not run here."""
    from streetunveiler_amd import _lib
    dummy = ctypes.create_string_buffer(256)
    p, big = ctypes.addressof(dummy), 1 << 40
    counts = (ctypes.c_uint32 * 4)()
    INVALID, TOO_SMALL, UNSUPPORTED, inf = -1, -3, -4, math.inf
    plan = [((-1, p, p, p, p, 1.0, 0.0, 1.0, -1.0, None, p, big, counts, None), INVALID, b"P < 0"),
            ((5, p, p, p, p, 1.0, 0.0, 1.0, -1.0, None, p, big, None, None), INVALID, b"counts_out"),
            ((5, None, p, p, p, 1.0, 0.0, 1.0, -1.0, None, p, big, counts, None), INVALID, b"accum"),
            ((5, p, None, p, p, 1.0, 0.0, 1.0, -1.0, None, p, big, counts, None), INVALID, b"denom"),
            ((5, None, None, None, p, inf, 0.0, 1.0, -1.0, None, p, big, counts, None), INVALID, b"opacity"),
            ((5, p, p, p, None, 1.0, 0.0, 1.0, -1.0, None, p, big, counts, None), INVALID, b"scaling"),
            ((5, p, p, p, p, 1.0, 0.0, 1.0, -1.0, None, None, big, counts, None), INVALID, b"workspace"),
            ((5, p, p, p, p, 1.0, 0.0, 1.0, -1.0, None, p, lib.sr_densify_workspace_bytes(5) - 1, counts, None), TOO_SMALL, b"workspace"),
            ((1 << 30, p, p, p, p, 1.0, 0.0, 1.0, -1.0, None, p, big, counts, None), UNSUPPORTED, b"30-bit")]
    for args, code, fragment in plan:
        rc = lib.sr_densify_plan(*args)
        assert rc == code and fragment in lib.sr_last_error(), (args, rc, lib.sr_last_error())
    counts[:] = [7, 7, 7, 7]
    assert lib.sr_densify_plan(0, None, None, None, None, 1.0, 0.0, 1.0, -1.0, None, None, 0, counts, None) == 0 and list(counts) == [0, 0, 0, 0]

    seg = lambda words=3, role=0, src=p, dst=p: _lib.SrDensifySegment(src, dst, words, role)
    table = lambda *segs: (_lib.SrDensifySegment * len(segs))(*segs)
    good = (ctypes.c_uint32 * 4)(3, 1, 2, 1)
    apply = [((-1, good, p, p, p, table(seg()), 1, p, big, None), INVALID, b"P < 0"),
             ((5, None, p, p, p, table(seg()), 1, p, big, None), INVALID, b"counts"),
             ((5, good, p, p, p, table(*[seg()] * 9), 9, p, big, None), INVALID, b"n_segments"),
             ((5, good, p, p, p, None, 1, p, big, None), INVALID, b"segments is NULL"),
             ((5, good, p, p, p, table(seg(role=4)), 1, p, big, None), INVALID, b"unknown role"),
             ((5, good, p, p, p, table(seg(role=-1)), 1, p, big, None), INVALID, b"unknown role"),
             ((5, good, p, p, p, table(seg(words=-1)), 1, p, big, None), INVALID, b"row_words"),
             ((5, good, p, p, p, table(seg(words=65536)), 1, p, big, None), INVALID, b"row_words"),
             ((5, good, p, p, p, table(seg(words=4, role=2)), 1, p, big, None), INVALID, b"xyz role"),
             ((5, good, p, p, p, table(seg(words=3, role=3)), 1, p, big, None), INVALID, b"scaling role"),
             ((5, good, p, p, p, table(seg(src=None)), 1, p, big, None), INVALID, b"src / dst"),
             ((5, good, p, p, p, table(seg(dst=None)), 1, p, big, None), INVALID, b"src / dst"),
             ((5, good, None, p, p, table(seg(role=2)), 1, p, big, None), INVALID, b"noise"),
             ((5, good, p, None, p, table(seg(role=2)), 1, p, big, None), INVALID, b"noise"),
             ((5, (ctypes.c_uint32 * 4)(5, 1, 2, 1), p, p, p, table(seg()), 1, p, big, None), INVALID, b"counts"),
             ((5, (ctypes.c_uint32 * 4)(3, 1, 1, 2), p, p, p, table(seg()), 1, p, big, None), INVALID, b"counts"),
             ((5, good, p, p, p, table(seg()), 1, None, big, None), INVALID, b"workspace"),
             ((5, good, p, p, p, table(seg()), 1, p, lib.sr_densify_workspace_bytes(5) - 1, None), TOO_SMALL, b"workspace")]
    for args, code, fragment in apply:
        rc = lib.sr_densify_apply(*args)
        assert rc == code and fragment in lib.sr_last_error(), (args[:2], rc, lib.sr_last_error())
    zero = (ctypes.c_uint32 * 4)()
    assert lib.sr_densify_apply(0, zero, None, None, None, None, 0, None, 0, None) == 0                    # no Gaussians: no error, no work
    assert lib.sr_densify_apply(5, zero, None, None, None, table(seg(src=None, dst=None)), 1, None, 0, None) == 0      # everything pruned: nothing to move
    assert lib.sr_densify_apply(5, good, None, None, None, table(seg(words=0, src=None, dst=None)), 1, p, big, None) == 0   # a row length of 0 launches nothing


def _cpu_model():
    c = dc.case("P65_rest45_state")
    return dc.Model(c, torch.optim.Adam, "cpu", torch.float32, foreach=False), c


def test_cpu_tensors_wrong_dtypes_and_shapes_are_refused():
    from streetunveiler_amd import densify_and_prune, densify_and_prune_tensors, prune_points
    from streetunveiler_amd._lib import SurfelRasterError
    model, c = _cpu_model()
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        densify_and_prune(model, 0.0002, 0.005, 5.0, 20)
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        prune_points(model, torch.zeros(65, dtype=torch.bool))
    args = (c.semantics, c.accum, c.denom, c.max_radii2D, 0.0002, 0.005, 5.0, 20, 0.01)
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        densify_and_prune_tensors(dict(c.params), dict(c.moments), *args)
    with pytest.raises(ValueError, match="lacks the group"):
        densify_and_prune_tensors({k: v for k, v in c.params.items() if k != "rotation"}, {}, *args)
    with pytest.raises(ValueError, match="max_grad"):
        densify_and_prune(model, 0.0, 0.005, 5.0, 20)


@pytest.mark.parametrize("what, change", [
    ("opacity is torch.float64", lambda p, m: p.update(opacity=p["opacity"].double())),
    ("scaling must be", lambda p, m: p.update(scaling=p["scaling"][:, :1].contiguous())),
    ("rotation must be", lambda p, m: p.update(rotation=p["rotation"][:-1].contiguous())),
    ("f_dc is not contiguous", lambda p, m: p.update(f_dc=p["f_dc"].permute(2, 1, 0).contiguous().permute(2, 1, 0))),
    ("exp_avg_sq of xyz must be", lambda p, m: m.update(xyz=(m["xyz"][0], m["xyz"][1][:, :2].contiguous()))),
    ("exp_avg of f_rest is torch.float16", lambda p, m: m.update(f_rest=(m["f_rest"][0].half(), m["f_rest"][1]))),
])
def test_wrong_tensors_are_named(what, change):
    """dtype, shape and contiguity are checked before the device, so the ValueErrors can be met here."""
    from streetunveiler_amd import densify_and_prune_tensors
    c = dc.case("P65_rest45_state")
    params, moments = dict(c.params), dict(c.moments)
    change(params, moments)
    with pytest.raises(ValueError, match=what):
        densify_and_prune_tensors(params, moments, c.semantics, c.accum, c.denom, c.max_radii2D, 0.0002, 0.005, 5.0, 20, 0.01)
    with pytest.raises(ValueError, match="semantics is torch.int16"):
        densify_and_prune_tensors(dict(c.params), {}, c.semantics.to(torch.int16), c.accum, c.denom, c.max_radii2D, 0.0002, 0.005, 5.0, 20, 0.01)
    with pytest.raises(ValueError, match="denom must be"):
        densify_and_prune_tensors(dict(c.params), {}, c.semantics, c.accum, c.denom[:-1], c.max_radii2D, 0.0002, 0.005, 5.0, 20, 0.01)

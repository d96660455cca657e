"""CPU: the radius-clustering oracle of tests/cluster_cases.py means what it should, its table rejects the wrong clusterings one can think
of, and the C-ABI of the op is declared, exported and refuses bad arguments before it touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import cluster_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(cc.CASES)


def _sequential_union_find(xyz, threshold, mask):
    """The reference's parallel=False loop: for i, for every later j in range, union(i, j); the smaller root wins."""
    adj = cc.adjacency(xyz, threshold, mask)
    father = list(range(len(xyz)))

    def find(x):
        while father[x] != x:
            father[x] = father[father[x]]
            x = father[x]
        return x
    for i in range(len(xyz)):
        for j in np.flatnonzero(adj[i, i + 1:]) + i + 1:
            a, b = find(i), find(int(j))
            father[max(a, b)] = min(a, b)
    out = np.array([find(i) for i in range(len(xyz))], np.int64).reshape(-1)
    if mask is not None:
        out[~mask] = -1
    return out


@pytest.mark.parametrize("name", ALL)
def test_oracle_equals_a_sequential_union_find(name):
    xyz, threshold, mask = cc.case(name)
    want = cc.oracle(name)
    assert want.dtype == np.int64 and want.shape == (len(xyz),)
    np.testing.assert_array_equal(want, _sequential_union_find(xyz, threshold, mask))
    part = cc.takes_part(xyz, mask)
    assert (want[part] <= np.flatnonzero(part)).all() and (want[part] >= 0).all()
    if mask is not None:
        assert (want[~mask] == -1).all()
    lone = np.flatnonzero(~np.isfinite(xyz).all(axis=1) & (np.ones(len(xyz), bool) if mask is None else mask))
    np.testing.assert_array_equal(want[lone], lone)


def test_what_the_named_cases_are_there_for():
    def components(name):
        return len(cc.partition(cc.oracle(name)))
    assert cc.oracle("size_0").shape == (0,) and cc.oracle("size_1").tolist() == [0]
    assert cc.oracle("pair_touching").tolist() == [0, 0] and cc.oracle("pair_apart").tolist() == [0, 1]
    assert len(cc.case("identical_600")[0]) > cc.BOX and not cc.oracle("identical_600").any()
    assert not cc.oracle("chain").any() and components("chain_gap") == 2
    assert components("lattice_at_spacing") == 729 and components("lattice_above_spacing") == 1
    assert cc.oracle("root_boundary_apart").tolist() == [0, 1] and cc.oracle("root_boundary_joined").tolist() == [0, 0]
    assert components("parallel_lines") == 4
    xyz, _, mask = cc.case("masked_bridge")
    left = xyz[:, 0] <= np.float32(0.1)
    assert components("masked_bridge") == 2 and len(set(cc.oracle("masked_bridge")[mask & left])) == 1
    assert len(cc.partition(cc.oracle_labels(xyz, cc.case("masked_bridge")[1], None))) == 1      # unmasked, the bridge joins them
    largest = {0.05: (40, 300), 0.0544: (300, 2000), 0.06: (2000, 4000)}      # below, at and above the radius where a giant component forms
    for r in cc.UNIFORM_RADII:      # singletons and mid-size components beside it
        sizes = np.array(sorted(len(g) for g in cc.partition(cc.oracle(f"uniform_{r}"))))
        assert (sizes == 1).sum() > 50 and ((sizes > 5) & (sizes < 100)).any() and largest[r][0] < sizes[-1] < largest[r][1], (r, sizes[-5:])
    # the non-finite points change nobody else's label
    for name in ("nonfinite", "nonfinite_masked"):
        xyz, threshold, mask = cc.case(name)
        bad = np.array(sorted(cc.NONFINITE_ROWS))
        keep = np.ones(len(xyz), bool)
        keep[bad] = False
        without = cc.oracle_labels(xyz[keep], threshold, None if mask is None else mask[keep])
        orig = np.flatnonzero(keep)
        mapped = {frozenset(orig[sorted(g)].tolist()) for g in cc.partition(without)}
        assert mapped == {g for g in cc.partition(cc.oracle(name)) if not (len(g) == 1 and next(iter(g)) in bad)}, name


def test_parallel_lines_alternate_along_the_morton_curve():
    xyz, _, _ = cc.case("parallel_lines")
    lo, ext = xyz.min(axis=0), np.maximum(xyz.max(axis=0) - xyz.min(axis=0), 1e-30)
    q = np.clip((xyz - lo) / ext * 1023, 0, 1023).astype(np.uint32)
    code = np.zeros(len(xyz), np.uint64)
    for bit in range(10):
        for c in range(3):
            code |= ((q[:, c] >> bit) & 1).astype(np.uint64) << np.uint64(3 * bit + c)
    on_upper = (xyz[np.argsort(code, kind="stable"), 1] > 0.005).astype(int)
    assert np.abs(np.diff(on_upper)).sum() > 100      # the two lines change places along the curve more than a hundred times


@pytest.mark.parametrize("name", cc.RANDOM_CASES)
def test_oracle_adjacency_is_the_reference_expression(name):
    """`(abs(a - b) ** 2).sum(-1) ** 0.5 < threshold` of the reference's loop, in torch on the CPU, row block by row block."""
    import torch
    xyz, threshold, mask = cc.case(name)
    if not len(xyz):
        return
    adj = cc.adjacency(xyz, threshold, mask)
    idx = np.flatnonzero(cc.takes_part(xyz, mask))       # the reference measures among the points it selected
    pts = torch.from_numpy(xyz[idx].copy())
    for lo in range(0, len(idx), 500):
        d = (torch.abs(pts[lo:lo + 500, None, :] - pts[None, :, :]) ** 2).sum(dim=-1) ** 0.5
        np.testing.assert_array_equal((d < threshold).numpy(), adj[np.ix_(idx[lo:lo + 500], idx)], err_msg=f"{name}, rows from {lo}")


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
def _morton_rank(xyz):
    if not len(xyz):
        return np.zeros(0, np.int64)
    fin = np.where(np.isfinite(xyz), xyz, 0)
    lo, ext = fin.min(axis=0), np.maximum(fin.max(axis=0) - fin.min(axis=0), 1e-30)
    q = np.clip((fin - lo) / ext * 1023, 0, 1023).astype(np.uint64)
    code = np.zeros(len(xyz), np.uint64)
    for bit in range(10):
        for c in range(3):
            code |= ((q[:, c] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + c)
    rank = np.empty(len(xyz), np.int64)
    rank[np.argsort(code, kind="stable")] = np.arange(len(xyz))
    return rank


def _mutant_not_strict(xyz, threshold, mask):
    return cc.labels_from_adjacency(cc.adjacency(xyz, threshold, mask, below=lambda d2, r: np.sqrt(d2) <= r), xyz, mask)


def _mutant_squared_threshold(xyz, threshold, mask):      # no root: the squared distance against the squared float32 threshold
    return cc.labels_from_adjacency(cc.adjacency(xyz, threshold, mask, below=lambda d2, r: d2 < r * r), xyz, mask)


def _mutant_no_root(xyz, threshold, mask):                # no root at all: the squared distance against the threshold
    return cc.labels_from_adjacency(cc.adjacency(xyz, threshold, mask, below=lambda d2, r: d2 < r), xyz, mask)


def _mutant_masked_bridges(xyz, threshold, mask):         # the mask is applied to the labels only
    return cc.labels_from_adjacency(cc.adjacency(xyz, threshold, None), xyz, mask)


def _mutant_named_by_morton_position(xyz, threshold, mask):
    want = cc.oracle_labels(xyz, threshold, mask)
    rank, out = _morton_rank(xyz), want.copy()
    for g in cc.partition(want):
        g = np.array(sorted(g))
        out[g] = g[np.argmin(rank[g])]
    return out


def _mutant_one_pointer_jump(xyz, threshold, mask):
    adj = cc.adjacency(xyz, threshold, mask)
    n = len(xyz)
    father = np.arange(n, dtype=np.int64)
    if n:
        father = np.where(adj.any(axis=1), np.argmax(adj, axis=1), father)     # the smallest index in range (the point itself included)
        father = np.minimum(father, np.arange(n))
        father = father[father]
    if mask is not None:
        father[~mask] = -1
    return father


MUTANTS = {"<= instead of <": _mutant_not_strict, "d2 < r * r without the root": _mutant_squared_threshold, "d2 < r": _mutant_no_root,
           "masked points as bridges": _mutant_masked_bridges, "named by the smallest Morton position": _mutant_named_by_morton_position,
           "a single pass of pointer jumping": _mutant_one_pointer_jump}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_table_rejects_wrong_clusterings(mutant):
    failed = [name for name in ALL if not np.array_equal(MUTANTS[mutant](*cc.case(name)), cc.oracle(name))]
    print(f"{mutant}: fails {len(failed)} of {len(ALL)} cases: {failed}")
    assert failed, f"no case of the table tells '{mutant}' from the oracle"


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
    for name in ("sr_cluster_workspace_bytes", "sr_cluster_radius"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.sr_abi_version() == 10      # an addition: nothing that existed changed
    for name in ("radius_components", "cluster_instance_with_mask", "cluster_semantic_instance"):
        assert name in streetunveiler_amd.__all__ and callable(getattr(streetunveiler_amd, name))
    from streetunveiler_amd.build import SOURCES
    assert ("cluster.hip", ["-ffp-contract=off"]) in [(s, list(f)) for s, f in SOURCES]


def test_workspace_size_grows_with_the_cloud(lib):
    sizes = [lib.sr_cluster_workspace_bytes(n) for n in (-5, 0, 1, 513, 100000, 3000000)]
    assert sizes[0] == sizes[1] > 0 and sizes == sorted(sizes)
    assert sizes[-1] >= 3000000 * (16 + 4 * 4)      # the sorted points, codes twice, order, parents


def test_argument_refusals_without_gpu(lib):
    """Every refusal comes before the first HIP call, or this test could not run here."""
    dummy = ctypes.create_string_buffer(64)
    p, big = ctypes.addressof(dummy), 1 << 40
    INVALID, TOO_SMALL = -1, -3
    table = [((-1, p, None, 0.07, p, p, big, None), INVALID, b"negative"),
             ((5, None, None, 0.07, p, p, big, None), INVALID, b"NULL"),
             ((5, p, None, 0.07, None, p, big, None), INVALID, b"NULL"),
             ((5, p, p, 0.07, p, None, big, None), INVALID, b"NULL"),
             ((5, p, None, float("nan"), p, p, big, None), INVALID, b"radius"),
             ((5, p, None, float("inf"), p, p, big, None), INVALID, b"radius"),
             ((5, p, None, -1e-3, p, p, big, None), INVALID, b"radius"),
             ((5, p, None, 1e300, p, p, big, None), INVALID, b"radius"),       # inf as a float32
             ((0, None, None, float("nan"), None, None, 0, None), INVALID, b"radius"),
             ((5, p, None, 0.07, p, p, lib.sr_cluster_workspace_bytes(5) - 1, None), TOO_SMALL, b"workspace")]
    for args, code, fragment in table:
        rc = lib.sr_cluster_radius(*args)
        assert rc == code and fragment in lib.sr_last_error(), (args, rc, lib.sr_last_error())
    assert lib.sr_cluster_radius(0, None, None, 0.07, None, None, 0, None) == 0      # an empty cloud is no error and no work


def test_cpu_tensors_and_wrong_shapes_are_refused():
    import torch
    from streetunveiler_amd import cluster_instance_with_mask, radius_components
    from streetunveiler_amd._lib import SurfelRasterError
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        radius_components(torch.zeros(5, 3), 0.07)
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        cluster_instance_with_mask(torch.zeros(5, 3), torch.ones(5, dtype=torch.bool))

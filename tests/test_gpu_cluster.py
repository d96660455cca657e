"""GPU (-m gpu): the radius clustering (csrc/cluster.hip through streetunveiler_amd.cluster) against the oracle of tests/cluster_cases.py,
label for label: no tolerance, no case left out.  tests/test_cluster_host.py shows that the table rejects the wrong clusterings one can
think of."""
import threading

import numpy as np
import pytest
import torch

from tests import cluster_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = sorted(cc.CASES)
BIT = 1 << 5      # the semantic bit of the mirror of cluster_semantic_instance


def _on_device(name):
    xyz, threshold, mask = cc.case(name)
    return torch.tensor(xyz, device=DEV).reshape(-1, 3), threshold, None if mask is None else torch.tensor(mask, device=DEV)


def _report(name, got, want):
    wrong = np.flatnonzero(got != want)
    print(f"{name}: {len(wrong)} of {len(want)} labels differ from the oracle" +
          (f"; first rows {wrong[:5].tolist()}: got {got[wrong[:5]].tolist()}, oracle {want[wrong[:5]].tolist()}" if len(wrong) else ""))


@pytest.mark.parametrize("name", ALL)
def test_radius_components_equal_the_oracle(name):
    from streetunveiler_amd import radius_components
    xyz, threshold, mask = _on_device(name)
    out = radius_components(xyz, threshold, mask)
    assert out.dtype == torch.int64 and out.shape == (len(xyz),) and out.device == xyz.device
    got, want = out.cpu().numpy(), cc.oracle(name)
    _report(name, got, want)
    np.testing.assert_array_equal(got, want, err_msg=f"{name}: {cc.CASES[name][0]}")


@pytest.mark.parametrize("name", ALL)
def test_the_two_mirrors_equal_the_oracle(name):
    """cluster_instance_with_mask takes the mask as it is (all true where the case has none); cluster_semantic_instance takes it as a bit
    of semantics_32bit among other bits."""
    from streetunveiler_amd import cluster_instance_with_mask, cluster_semantic_instance
    xyz, threshold, mask = _on_device(name)
    valid = torch.ones(len(xyz), dtype=torch.bool, device=DEV) if mask is None else mask
    want = cc.oracle(name)
    got = cluster_instance_with_mask(xyz, valid, threshold).cpu().numpy()
    _report(name + " (cluster_instance_with_mask)", got, want)
    np.testing.assert_array_equal(got, want, err_msg=name)
    other = torch.tensor(np.random.default_rng(7).integers(0, 1 << 20, size=len(xyz)) & ~BIT, dtype=torch.int32, device=DEV)
    semantics = other | (valid.to(torch.int32) * BIT)
    got = cluster_semantic_instance(xyz, semantics, BIT, threshold).cpu().numpy()
    _report(name + " (cluster_semantic_instance)", got, want)
    np.testing.assert_array_equal(got, want, err_msg=name)


def test_default_thresholds_are_the_references():
    import inspect
    from streetunveiler_amd import cluster_instance_with_mask, cluster_semantic_instance
    assert inspect.signature(cluster_instance_with_mask).parameters["threshold"].default == 7e-2
    assert inspect.signature(cluster_semantic_instance).parameters["threshold"].default == 3e-2
    xyz, _, mask = _on_device("uniform_0.06_half_masked")
    want = cc.oracle_labels(*cc.case("uniform_0.06_half_masked")[:1], 7e-2, cc.case("uniform_0.06_half_masked")[2])
    np.testing.assert_array_equal(cluster_instance_with_mask(xyz, mask).cpu().numpy(), want)


@pytest.mark.parametrize("name", ["uniform_0.0544", "uniform_0.06_half_masked", "chain", "identical_600"])
def test_two_runs_are_identical(name):
    """The unions race; the labels do not show it: the smaller root always wins, so a component's root is its smallest index."""
    from streetunveiler_amd import radius_components
    xyz, threshold, mask = _on_device(name)
    first = radius_components(xyz, threshold, mask)
    for _ in range(3):
        assert torch.equal(radius_components(xyz, threshold, mask), first)


@pytest.mark.parametrize("name", ["uniform_0.0544", "nonfinite_masked", "parallel_lines", "chain_gap"])
def test_permuting_the_points_keeps_the_partition(name):
    """The same points in another index order: other names, the same sets of points."""
    from streetunveiler_amd import radius_components
    xyz, threshold, mask = cc.case(name)
    perm = np.random.default_rng(5).permutation(len(xyz))
    got = radius_components(torch.tensor(xyz[perm], device=DEV), threshold, None if mask is None else torch.tensor(mask[perm], device=DEV)).cpu().numpy()
    moved = {frozenset(perm[sorted(g)].tolist()) for g in cc.partition(got)}      # back to the original points
    assert moved == cc.partition(cc.oracle(name))
    np.testing.assert_array_equal(got == -1, cc.oracle(name)[perm] == -1)


def test_side_stream_and_second_thread_give_the_same_labels():
    from streetunveiler_amd import radius_components
    name = "uniform_0.0544_half_masked"
    xyz, threshold, mask = _on_device(name)
    want = cc.oracle(name)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        on_side = radius_components(xyz, threshold, mask)
    side.synchronize()
    np.testing.assert_array_equal(on_side.cpu().numpy(), want, err_msg="side stream")
    result = {}

    def work():
        try:
            result["labels"] = radius_components(xyz, threshold, mask).cpu().numpy()
        except Exception as e:      # noqa: BLE001 -- handed to the asserting thread
            result["error"] = e
    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "error" not in result, result.get("error")
    np.testing.assert_array_equal(result["labels"], want, err_msg="second thread")


def test_input_forms():
    """float64, a non-contiguous view, a uint8 / int64 mask: the labels of the contiguous float32 / bool call; the inputs stay as they were."""
    from streetunveiler_amd import radius_components
    name = "uniform_0.06_half_masked"
    xyz, threshold, mask = _on_device(name)
    want = cc.oracle(name)
    wide = torch.zeros(len(xyz), 6, device=DEV)
    wide[:, ::2] = xyz
    before = wide.clone()
    for what, x, m in (("float64", xyz.double(), mask), ("non-contiguous", wide[:, ::2], mask), ("uint8 mask", xyz, mask.to(torch.uint8)),
                       ("int64 mask", xyz, mask.to(torch.int64) * 3)):
        np.testing.assert_array_equal(radius_components(x, threshold, m).cpu().numpy(), want, err_msg=what)
    assert torch.equal(wide, before)
    assert radius_components(torch.zeros(0, 3, device=DEV), 0.07).shape == (0,)
    assert radius_components(xyz, 0.0, mask).cpu().numpy().tolist() == np.where(cc.case(name)[2], np.arange(len(xyz)), -1).tolist()      # radius 0: nobody is in range


def test_cpu_tensors_wrong_shapes_and_bad_radii_are_refused():
    from streetunveiler_amd import cluster_instance_with_mask, cluster_semantic_instance, radius_components
    from streetunveiler_amd._lib import SurfelRasterError
    good = torch.zeros(5, 3, device=DEV)
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        radius_components(torch.zeros(5, 3), 0.07)
    with pytest.raises(SurfelRasterError, match="no CPU path"):
        radius_components(good, 0.07, torch.ones(5, dtype=torch.bool))
    for bad in (torch.zeros(5, 2, device=DEV), torch.zeros(15, device=DEV), torch.zeros(5, 3, 1, device=DEV)):
        with pytest.raises(SurfelRasterError, match="num_points, 3"):
            radius_components(bad, 0.07)
    for bad_mask in (torch.ones(4, dtype=torch.bool, device=DEV), torch.ones(5, 1, dtype=torch.bool, device=DEV)):
        with pytest.raises(SurfelRasterError, match="mask"):
            cluster_instance_with_mask(good, bad_mask)
    with pytest.raises(SurfelRasterError, match="mask"):
        cluster_semantic_instance(good, torch.ones(6, dtype=torch.int32, device=DEV), 1)
    for radius in (float("nan"), float("inf"), -0.01):
        with pytest.raises(SurfelRasterError, match="radius"):
            radius_components(good, radius)

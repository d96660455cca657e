"""CPU: the checker of the LiDAR voxel downsample against the reference's own class (tests/golden/voxel_init_golden.npz, written by
tools/make_voxel_init_golden.py), the integer purity rule against the reference's float32 expression, the bars of tests/voxel_cases.py
rejecting wrong implementations, and the CPU-computable parts of create_from_pcd against the reference's formulae."""
import os

import numpy as np
import pytest
import torch

from streetunveiler_amd import _lib as L
from streetunveiler_amd import voxel as V
from tests import voxel_cases as vc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxel_init_golden.npz")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


# ---- the checker against the reference's class ----------------------------------------------------------------------------------------------
def test_checker_reproduces_the_reference_class():
    """Indices, order, labels and m exact; the means within the ulp bar (the reference's torch.sort is not stable, so its own order of
    addition -- in the points' dtype -- is undefined: the means are not compared by bits)."""
    z = np.load(GOLDEN)
    names = [str(n) for n in z["names"]]
    assert len(names) >= 4
    dtypes, with_labels = set(), set()
    for name in names:
        get = lambda key: z[f"{name}/{key}"] if f"{name}/{key}" in z.files else None
        pts, col, nrm, sem = get("points"), get("colors"), get("normals"), get("semantics")
        dtypes.add(pts.dtype.name)
        with_labels.add(sem is not None)
        v = float(z[f"{name}/voxel_size"])
        p, c, n, s, counts, index = V.voxel_down_sample_torch(_t(pts), v, _t(col), _t(nrm), _t(sem), mean_dtype=torch.float64, return_counts=True,
                                                             return_index=True, round_means=False)
        assert np.array_equal(index.numpy(), get("out_index")), name            # m, the row order, the keep decisions
        if sem is None:
            assert s is None and get("out_semantics") is None
        else:
            assert s.dtype == torch.int32 and np.array_equal(s.numpy(), get("out_semantics")), name
        all_index = V.voxel_index_torch(_t(pts), v)[0].numpy()
        rows = np.searchsorted(index.numpy(), all_index)
        ok = rows < index.shape[0]
        ok[ok] = index.numpy()[rows[ok]] == all_index[ok]
        for key, src, truth in (("points", pts, p), ("colors", col, c), ("normals", nrm, n)):
            ref = get("out_" + key)
            if src is None:
                assert truth is None and ref is None
                continue
            assert ref.dtype == np.float32 and ref.shape == tuple(truth.shape), (name, key)
            largest = np.zeros(ref.shape, np.float64)
            np.maximum.at(largest, rows[ok], np.abs(src[ok].astype(np.float64)))
            err = np.abs(ref.astype(np.float64) - truth.numpy())
            ulp = np.spacing(largest.astype(np.float32))
            print(name, key, "worst error of the reference's own means: %.3f ulp of the largest member" % float((err / ulp).max()))
            # float64 clouds: the reference adds in float64 and its means are held to the bar of tests/voxel_cases.py, ONE float32 ulp of the
            # largest member.  float32 clouds: the reference adds a voxel's k members in float32, which the bar's derivation does not cover
            # -- k - 1 additions, each rounding a partial sum of at most k M to half an ulp(k M) <= k ulp(M), leave the sum off by less than
            # (k - 1) k ulp(M) and the mean by k - 1 ulps; the division and the store round once more: k ulps.  Measured on this fixture:
            # 1.33 ulps at k = 3 (f32_colors), 1.00 elsewhere.  That is the reference's own error; the checker's float64 means are the truth.
            k = counts.numpy().astype(np.float64)[:, None] if src.dtype == np.float32 else 1.0
            assert (err <= k * ulp).all(), (name, key, float((err / ulp).max()))
    assert dtypes == {"float32", "float64"} and with_labels == {True, False}


def test_integer_purity_rule_is_the_reference_float32_expression():
    """5 max >= 4 n against `1.0 * max / len < 0.8` with max an int64 tensor element (torch promotes the quotient to float32) for every
    (max, n), n <= 200."""
    n = torch.arange(1, 201, dtype=torch.int64)[None, :].expand(200, 200)
    most = torch.arange(1, 201, dtype=torch.int64)[:, None].expand(200, 200)
    valid = most <= n
    quotient = 1.0 * most / n                                       # what the reference's line forms per voxel
    assert quotient.dtype == torch.float32
    dropped = quotient < 0.8
    assert torch.equal(~dropped[valid], V.keep_rule(most, n)[valid])
    assert bool(V.keep_rule(4, 5)) and bool(V.keep_rule(8, 10)) and not V.keep_rule(3, 4) and not V.keep_rule(7, 9) and not V.keep_rule(1, 2)


# ---- the bars ------------------------------------------------------------------------------------------------------------------------------
SMALL = [n for n in vc.NAMES if not n.startswith(("own_voxel_4", "mix_"))]     # the numpy loop is slow: the large cases are the GPU test's


@pytest.mark.parametrize("name", SMALL)
def test_independent_numpy_statement_passes_the_bars(name):
    vc.compare(name, vc.numpy_down_sample(vc.case(name)), "numpy")


def test_case_list_is_what_the_issue_asks_for():
    names = set(vc.NAMES)
    assert {"n0", "n1", "identical", "one_voxel_5000", "faces", "negative", "far_10km_float32", "far_10km_float64", "two_clusters_300m", "label_shares",
            "heavy_threshold", "mix_20000_f32", "reciprocal_trap"} <= names
    for b in (vc.SORT_BLOCK, vc.SCAN_CHUNK):
        assert {f"own_voxel_{b - 1}", f"own_voxel_{b}", f"own_voxel_{b + 1}"} <= names
    assert {f"absent_{k}" for k in range(8)} <= names
    assert vc.case("one_voxel_5000")["points"].shape[0] == 5000 and vc.expected("one_voxel_5000")["counts"].tolist() == [5000]
    for b in (vc.SORT_BLOCK, vc.SCAN_CHUNK):                           # a voxel each
        assert vc.expected(f"own_voxel_{b + 1}")["index"].shape[0] == b + 1
    assert vc.expected("identical")["counts"].tolist() == [300]
    # offset^3 needs more than 32 bits at 300 m / 0.1 m
    offset = V.voxel_index_torch(_t(vc.case("two_clusters_300m")["points"]), 0.1)[1]
    assert offset ** 3 > 1 << 32
    # the faces: (p - lo) / v is an exact integer
    c = vc.case("faces")
    lo = c["points"].min(0) - np.float32(0.125)
    q = (c["points"] - lo) / np.float32(0.25)
    assert np.array_equal(q[1:], np.rint(q[1:])) and (q[0] == 0.5).all()       # (row 0 is the minimum itself, half a voxel inside)
    # the label shares: which voxels stay
    want = vc.expected("label_shares")
    assert want["index"].shape[0] == sum(vc.LABEL_SHARES_KEPT) and set(want["semantics"].tolist()) == {0, 255, 2}
    # the heavy threshold: members on both sides of it, kept and dropped
    counts = vc.expected("heavy_threshold")["counts"].tolist()
    assert counts == [1, vc.HEAVY - 1, vc.HEAVY, vc.HEAVY + 1, vc.HEAVY + 2]      # the anchor, then the four kept of the six
    assert max(vc.expected("mix_20000_f32")["counts"]) > vc.HEAVY
    assert {vc.case(f"absent_{k}")["semantics"].dtype.name for k in (4, 5, 6, 7)} >= {"int32", "int64"}


REJECTED_ON = {"reciprocal": "reciprocal_trap", "round": "negative", "lo_without_half": "negative", "offset_per_axis": "far_10km_float32",
               "strict_share": "label_shares", "float32_sum": "one_voxel_5000", "wrong_divisor": "label_shares", "descending": "negative"}


@pytest.mark.parametrize("variant", vc.VARIANTS)
def test_bars_reject_wrong_implementations(variant):
    name = REJECTED_ON[variant]
    vc.compare(name, vc.numpy_down_sample(vc.case(name)), "numpy")          # the right one passes on the same case
    with pytest.raises(AssertionError):
        vc.compare(name, vc.numpy_down_sample(vc.case(name), variant), variant)


def test_refusals_of_the_checker_and_of_cpu_tensors():
    for name, kw, fragment in vc.refusals():
        args = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        with pytest.raises(ValueError, match=fragment):
            V.voxel_down_sample_torch(**args)
    pts = torch.zeros((4, 3))
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        V.voxel_down_sample(pts, 0.1)
    with pytest.raises(ValueError, match="positive and finite"):
        V.voxel_down_sample(pts, 0.0)
    with pytest.raises(ValueError, match="rows"):
        V.voxel_down_sample(pts, 0.1, colors=torch.zeros((3, 3)))


def test_argument_refusals_of_the_c_abi_without_gpu():
    """Every refusal comes before the first HIP call, with the existing error codes."""
    import ctypes
    from streetunveiler_amd.build import build
    build()
    lib = L.load()
    dummy = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(dummy) + 15) // 16 * 16
    big = 1 << 40
    lo = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    nan_lo = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    INVALID, SMALL_BUFFER, UNSUPPORTED = -1, -3, -4

    def check(rc, code, fragment):
        assert rc == code and fragment.encode() in lib.sr_last_error(), (rc, lib.sr_last_error())
    assert lib.sr_voxel_workspace_bytes(-1) == 0 and lib.sr_voxel_workspace_bytes(0) > 0
    assert lib.sr_voxel_workspace_bytes(1 << 20) >= (1 << 20) * 40
    check(lib.sr_voxel_bounds(-1, p, 0, p, big, p, None), INVALID, "negative")
    check(lib.sr_voxel_bounds(10, None, 0, p, big, p, None), INVALID, "points is NULL")
    check(lib.sr_voxel_bounds(10, p + 4, 1, p, big, p, None), INVALID, "aligned")
    check(lib.sr_voxel_bounds(10, p, 2, p, big, p, None), INVALID, "points_f64")
    check(lib.sr_voxel_bounds(10, p, 0, p, 16, p, None), SMALL_BUFFER, "workspace")
    check(lib.sr_voxel_bounds(10, p, 0, p, big, None, None), INVALID, "bounds is NULL")
    check(lib.sr_voxel_bounds(0, p, 0, p, big, p, None), INVALID, "empty")
    for v in (0.0, -0.1, float("nan"), float("inf")):
        check(lib.sr_voxel_group(10, p, 0, None, 0, lo, v, 100, p, big, p, None), INVALID, "voxel_size")
    check(lib.sr_voxel_group(10, p, 0, None, 0, nan_lo, 0.1, 100, p, big, p, None), INVALID, "not finite")
    check(lib.sr_voxel_group(10, p, 0, None, 0, lo, 0.1, 0, p, big, p, None), INVALID, "offset")
    check(lib.sr_voxel_group(10, p, 0, None, 0, lo, 0.1, 1 << 21, p, big, p, None), UNSUPPORTED, "2^21")
    check(lib.sr_voxel_group(10, p, 0, p, 2, lo, 0.1, 100, p, big, p, None), INVALID, "semantics_bytes")
    check(lib.sr_voxel_group(10, p, 0, None, 0, lo, 0.1, 100, p, big, None, None), INVALID, "counts is NULL")
    check(lib.sr_voxel_group(10, p, 0, None, 0, lo, 0.1, 100, None, big, p, None), INVALID, "workspace is NULL")
    check(lib.sr_voxel_emit(10, p, 0, None, 0, None, 0, p, big, 11, 5, p, None, None, None, None, None, None), INVALID, "n_voxels")
    check(lib.sr_voxel_emit(10, p, 0, None, 0, None, 0, p, big, 5, 6, p, None, None, None, None, None, None), INVALID, "n_kept")
    check(lib.sr_voxel_emit(10, p, 0, None, 0, None, 0, p, big, 5, 5, None, None, None, None, None, None, None), INVALID, "out_points is NULL")
    check(lib.sr_voxel_emit(10, p, 0, p, 0, None, 0, p, big, 5, 5, p, None, None, None, None, None, None), INVALID, "out_colors is NULL")
    check(lib.sr_voxel_emit(10, p, 0, None, 0, p, 0, p, big, 5, 5, p, None, None, None, None, None, None), INVALID, "out_normals is NULL")
    check(lib.sr_voxel_emit(10, p, 0, None, 0, None, 0, p, big, 5, 5, p, None, None, None, None, p + 4, None), INVALID, "out_index")
    assert lib.sr_voxel_emit(10, p, 0, None, 0, None, 0, p, big, 5, 0, None, None, None, None, None, None, None) == 0      # no row: no work


# ---- create_from_pcd: the parts a CPU can compute ------------------------------------------------------------------------------------------
def test_initial_parameters_follow_the_reference_formulae():
    r = torch.Generator().manual_seed(4)
    colors = torch.rand((37, 3), generator=r, dtype=torch.float64)
    for degree in (0, 3):
        f = V.initial_features(colors, degree)
        assert f.dtype == torch.float32 and tuple(f.shape) == (37, (degree + 1) ** 2, 3)
        assert torch.equal(f[:, 0, :], (colors.float() - 0.5) / 0.28209479177387814) and not bool(f[:, 1:, :].any())      # RGB2SH, the rest zero
    o = V.initial_opacity(37, "cpu")
    assert o.dtype == torch.float32 and tuple(o.shape) == (37, 1)
    x = 0.1 * torch.ones((37, 1), dtype=torch.float)
    assert torch.equal(o, torch.log(x / (1 - x))) and abs(float(o[0]) - np.log(0.1 / 0.9)) < 1e-6                         # inverse_sigmoid(0.1)
    d2 = torch.tensor([0.0, 1e-9, 1e-7, 0.04, 9.0])
    s = V.initial_scaling(d2)
    assert tuple(s.shape) == (5, 2) and torch.equal(s[:, 0], s[:, 1])
    assert torch.equal(s[:, 0], torch.log(torch.sqrt(torch.clamp_min(d2, 0.0000001))))
    assert float(s[0, 0]) == float(s[1, 0]) == float(s[2, 0])                                                           # the clamp
    cloud = V.SemanticCloud(torch.zeros((4, 3)), torch.zeros((4, 3)), device="cpu")
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        V.create_from_pcd(cloud, 1.0)


def test_semantic_cloud_keeps_the_reference_attribute_names():
    cloud = V.SemanticCloud(np.zeros((5, 3)), np.ones((5, 3), np.float32), None, np.arange(5)[:, None], {"road": 0}, device="cpu")
    assert cloud.points.dtype == torch.float64 and cloud.colors.dtype == torch.float32 and cloud.normals is None
    assert tuple(cloud.semantics.shape) == (5,) and cloud.semantics_dict == {"road": 0} and len(cloud) == 5
    assert callable(cloud.voxel_down_sample) and callable(cloud.voxel_down_sample_with_no_grad)
    with pytest.raises(ValueError, match="rows"):
        V.SemanticCloud(np.zeros((5, 3)), np.ones((4, 3)), device="cpu")
    import streetunveiler_amd as S
    assert S.voxel_down_sample is V.voxel_down_sample and S.create_from_pcd is V.create_from_pcd and S.SemanticCloud is V.SemanticCloud

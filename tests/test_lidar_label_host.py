"""CPU: the checkers of the LiDAR colouring and labelling (streetunveiler_amd/lidar_label.py) against a fixture written from the reference's own
two helpers, the cases of tests/lidar_label_cases.py (no decision of a random row hangs on the last bit; the planted rows land where they
are meant to), the bars rejecting fourteen wrong implementations, the view record against the header's text, and the refusals."""
import os
import re

import numpy as np
import pytest
import torch

from streetunveiler_amd import _lib as L
from streetunveiler_amd import lidar_label as LL
from tests import lidar_label_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lidar_label_golden.npz")


def test_checkers_reproduce_the_reference_helpers_on_the_fixture():
    """mask, valid_pix and certain_mask of the reference's getCullMaskPointCloudInFrame / getCertainSemanticMask, exactly"""
    g = np.load(GOLDEN)
    pairs = sorted(k[:-len("mask")] for k in g.files if k.endswith("/mask"))
    assert len(pairs) >= 100
    inside = certain_total = uncertain_total = 0
    for key in pairs:
        case_name = key.split("/")[0]
        xyz = g[f"{case_name}/sweep{int(g[key + 'sweep'])}/xyz"]
        h, w = (int(x) for x in g[key + "hw"])
        mask, pix = LL.in_frame_numpy(h, w, xyz, g[key + "w2c"], g[key + "K"])
        assert np.array_equal(mask, g[key + "mask"]), key
        assert pix.dtype == np.int32 and np.array_equal(pix, g[key + "valid_pix"]), key
        certain = LL.certain_mask_numpy(g[key + "map"], pix, int(g[key + "check_range"]))
        assert np.array_equal(certain, g[key + "certain_mask"]), key
        inside += int(mask.sum())
        certain_total += int(certain.sum())
        uncertain_total += int((~certain).sum())
    assert inside > 5000 and certain_total > 1000 and uncertain_total > 1000      # the fixture exercises both answers


def test_fixture_is_what_the_cases_generate():
    """the stored inputs are the seeded cases' (the fixture and the GPU tests speak of the same clouds)"""
    g = np.load(GOLDEN)
    c = lc.case("merge_N65_S3_C3_r3")
    for s, (a, b, f0, f1) in enumerate(lc.groups(c)):
        assert g[f"{c.name}/sweep{s}/xyz"].tobytes() == c.points[a:b].tobytes()
        for f in range(f0, f1):
            assert np.array_equal(g[f"{c.name}/{f}/w2c"], c.views.w2c[f]) and np.array_equal(g[f"{c.name}/{f}/map"], c.views.map_numpy(f))


@pytest.mark.parametrize("name", lc.NAMES)
def test_no_random_decision_hangs_on_the_last_bit(name):
    assert lc.non_robust_pairs(lc.case(name)) == 0


@pytest.mark.parametrize("name", lc.NAMES)
def test_second_statement_equals_the_checker(name):
    c = lc.case(name)
    if c.raises:
        with pytest.raises(ValueError, match="n_classes"):
            LL.vote_semantics_numpy(c.points, c.views, lc.N_CLASSES)
        return
    lc.compare(name, lc.restated(name), "restated")


def test_cases_cover_what_they_claim():
    shapes = {(sp["op"], sp["N"]) for sp in lc.SPECS.values()}
    for N in (0, 1, 63, 64, 65, 4097):
        assert ("merge", N) in shapes and ("vote", N) in shapes
    assert {len(sp["views"]) for sp in lc.SPECS.values() if sp["op"] != "vote"} == {1, 3, 32}
    assert {len(sp["views"]) for sp in lc.SPECS.values() if sp["op"] == "vote"} >= {1, 3, 70}
    assert {sp["r"] for sp in lc.SPECS.values()} >= {1, 3, 10, 100}
    many = lc.case("merge_N4097_S1_C32_r3")
    assert {tuple(int(x) for x in hw) for hw in many.views.hw} == set(lc.SIZES)
    # the middle sweep of three is empty; a sweep's cameras see a point 0, 1 and 3 times, and their labels disagree somewhere
    c = lc.case("merge_N4097_S3_C3_r3_offset")
    assert c.sweep_offsets[1] == c.sweep_offsets[2]
    seen_by = np.zeros(len(c.points), dtype=np.int64)
    labels = np.full((len(c.points), 3), -1)
    for a, b, f0, f1 in lc.groups(c):
        for k, f in enumerate(range(f0, f1)):
            rows, u, v, certain = lc._hits(c, f, c.points[a:b], None)
            seen_by[a + rows[certain]] += 1
            labels[a + rows[certain], k] = c.views.map_numpy(f)[v[certain], u[certain]]
    assert {0, 1, 3} <= set(seen_by.tolist())
    both = (labels[:, 0] >= 0) & (labels[:, 1] >= 0)
    assert (labels[both, 0] != labels[both, 1]).any()
    # r = 100 is larger than every picture: every inside point is certain
    big = lc.case("merge_N4097_S1_C3_r100")
    for f in range(3):
        assert lc._hits(big, f, big.points, None)[3].all()
    # the unseen clouds are unseen, the tie case ties, the lut is not the identity
    assert len(lc.expected("merge_N65_S3_C3_unseen")["index"]) == 0 and not lc.expected("vote_N65_V3_unseen")["valid_mask"].any()
    ties = lc.expected("vote_N4097_V2_ties")
    assert ties["valid_mask"].sum() > 1000 and (ties["tag"] == 2).all()
    assert not np.array_equal(lc.LUT, np.arange(256))


def test_planted_rows_land_where_they_are_meant_to():
    """in the 48x64 A view: pix == 0, w, h are outside, the integer pixel and the .75 fraction truncate, the wrapped fourth corner decides"""
    c = lc.case("merge_N4097_S1_C1_r10")
    pix, z = LL.project_numpy(c.points, c.views.w2c[0], c.views.K[0])
    targets = lc.planted_pixels(48, 64, 10, True)
    assert np.array_equal(pix[:len(targets)], np.asarray(targets, dtype=np.float64)) and (z[:len(targets)] == 2.0).all()
    mask, valid = LL.in_frame_numpy(48, 64, c.points[:6], c.views.w2c[0], c.views.K[0])
    assert mask.tolist() == [True, False, False, False, False, True] and valid.tolist() == [[32, 24], [32, 24]]
    # u < r with v + r < h and u + r < w on a map in stripes: the reference's column w + u - r differs from l0, the mirrored one may not
    m = c.views.map_numpy(0)
    spot = np.array([[3, 5]])
    assert m[15, 64 + 3 - 10] != m[5, 3]
    assert not LL.certain_mask_numpy(m, spot, 10, "reference")[0]
    flat = np.full((48, 64), 2, dtype=np.uint8)
    flat[:, 57] = 4                                # only the wrapped column differs
    assert not LL.certain_mask_numpy(flat, spot, 10, "reference")[0] and LL.certain_mask_numpy(flat, spot, 10, "mirrored")[0]
    # row 0 and column 0 are never valid for the first three corners: u - r == 0 is not compared, u - r == 1 is (the reference's fourth
    # corner does read column u - r == 0: that is its line 94)
    edge = np.full((48, 64), 2, dtype=np.uint8)
    edge[:, 0] = 5
    edge[0, :] = 5
    assert LL.certain_mask_numpy(edge, np.array([[10, 10]]), 10, "mirrored")[0] and not LL.certain_mask_numpy(edge, np.array([[10, 10]]), 10, "reference")[0]
    edge[:, 1] = 5
    assert LL.certain_mask_numpy(edge, np.array([[10, 10]]), 10, "mirrored")[0] and not LL.certain_mask_numpy(edge, np.array([[11, 20]]), 10, "mirrored")[0]
    # u + r == w - 1 is compared, u + r == w is not
    right = np.full((48, 64), 2, dtype=np.uint8)
    right[:, 63] = 5
    assert not LL.certain_mask_numpy(right, np.array([[53, 20]]), 10)[0] and LL.certain_mask_numpy(right, np.array([[54, 20]]), 10)[0]


# which cases a flaw must fail on at least one of (all of the operation it touches are tried)
@pytest.mark.parametrize("flaw", lc.FLAWS)
def test_bars_reject_wrong_implementations(flaw):
    names = lc.VOTE_NAMES if flaw == "last_max" else lc.SWEEP_NAMES if flaw in ("first_camera", "uncertain_means", "point_major", "corner_ge0", "mirrored", "clamped") \
        else lc.NAMES
    rejected = []
    for name in names:
        if lc.case(name).raises:
            continue
        try:
            lc.compare(name, lc.restated(name, flaw), flaw)
        except AssertionError:
            rejected.append(name)
    assert rejected, f"no case rejects {flaw}"
    if flaw == "float32":
        assert "merge_N4097_S3_C3_r3_offset" in rejected and "vote_N4097_V3_offset_lut" in rejected


def test_view_record_matches_the_header():
    text = open(os.path.join(ROOT, "include", "surfel_raster.h")).read()
    body = re.search(r"^struct SrLabelView \{(.*?)\};", text, flags=re.S | re.M).group(1)
    fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert fields == ["double w2c[12]", "double K[9]", "int32_t h, w", "const uint8_t* image", "const uint8_t* map"]
    d = LL.VIEW_DTYPE
    assert d.names == ("w2c", "K", "h", "w", "image", "map") and d.itemsize == 192
    assert [d.fields[n][1] for n in d.names] == [0, 96, 168, 172, 176, 184]
    assert (LL.MAX_VIEWS, LL.MAX_CAMERAS, LL.MAX_CLASSES) == (65535, 32, 8)


def _views(**kw):
    args = dict(w2c=np.eye(4)[None], K=np.eye(3)[None], hw=[(4, 5)], images=[np.zeros((4, 5, 3), np.uint8)], maps=[np.zeros((4, 5), np.uint8)])
    args.update(kw)
    return LL.LabelViews(**args)


def test_refusals():
    with pytest.raises(ValueError, match="projective"):
        m = np.eye(4)[None].copy()
        m[0, 3, 0] = 0.5
        _views(w2c=m)
    with pytest.raises(ValueError, match="exactly"):
        _views(maps=[np.zeros((4, 6), np.uint8)])
    with pytest.raises(ValueError, match="exactly"):
        _views(images=[np.zeros((5, 5, 3), np.uint8)])
    with pytest.raises(ValueError, match="uint8"):
        _views(maps=[np.zeros((4, 5), np.int32)])
    with pytest.raises(ValueError, match="label_lut"):
        _views(label_lut=np.zeros(255, np.uint8))
    with pytest.raises(ValueError, match="at most"):
        LL.LabelViews(np.tile(np.eye(4), (65536, 1, 1)), np.tile(np.eye(3), (65536, 1, 1)), np.ones((65536, 2), np.int64), None, [])
    v = _views()
    p = torch.zeros((3, 3), dtype=torch.float64)
    for kw, fragment in ((dict(sweep_offsets=[0, 2]), "ascend"), (dict(sweep_offsets=[0, 3], cameras_per_sweep=2), "views"),
                         (dict(sweep_offsets=[0, 3], cameras_per_sweep=33), "cameras_per_sweep"), (dict(sweep_offsets=[0, 3], mode="both"), "mode"),
                         (dict(sweep_offsets=[0, 3], check_range=-1), "check_range"), (dict(sweep_offsets=[0, 3], fourth_corner="other"), "fourth_corner")):
        args = dict(points=p, views=v, cameras_per_sweep=1)
        args.update(kw)
        with pytest.raises(ValueError, match=fragment):
            LL.label_sweeps(**args)
    with pytest.raises(ValueError, match="float32 or float64"):
        LL.label_sweeps(p.half(), [0, 3], v, 1)
    with pytest.raises(ValueError, match="n_classes"):
        LL.vote_semantics(p, v, n_classes=9)
    # CPU tensors: loudly, there is no CPU path
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        LL.label_sweeps(p, [0, 3], v, 1)
    with pytest.raises(L.SurfelRasterError, match="no CPU path"):
        LL.vote_semantics(p, v)


def test_torch_twins_equal_the_checkers_on_the_cpu():
    for name in ("merge_N4097_S3_C3_r3_offset", "merge_N4097_S1_C3_r3_lut", "per_view_N4097_S3_C3_r3", "merge_N4097_S1_C1_r10_mirrored", "merge_N65_S3_C3_unseen"):
        c = lc.case(name)
        out = LL.label_sweeps_torch(lc.points_tensor(c), c.sweep_offsets, c.views, c.cameras, c.op, c.check_range, c.fourth_corner)
        lc.compare(name, {k: v.numpy() for k, v in out._asdict().items()}, "label_sweeps_torch")
    for name in ("vote_N4097_V70", "vote_N4097_V3_offset_lut", "vote_N4097_V2_ties"):
        c = lc.case(name)
        xyz, tag, valid = LL.vote_semantics_torch(lc.points_tensor(c), c.views, lc.N_CLASSES)
        lc.compare(name, {"xyz": xyz.numpy(), "tag": tag.numpy(), "valid_mask": valid.numpy()}, "vote_semantics_torch")
    with pytest.raises(ValueError, match="n_classes"):
        c = lc.case("vote_N65_V3_bad_label")
        LL.vote_semantics_torch(lc.points_tensor(c), c.views, lc.N_CLASSES)


def test_library_refuses_bad_arguments_without_a_gpu():
    lib = L.load()
    assert lib.sr_lidar_label_workspace_bytes(0, 1) > 0 and lib.sr_lidar_label_workspace_bytes(-1, 1) == 0 and lib.sr_lidar_label_workspace_bytes(1 << 30, 2) == 0
    assert lib.sr_lidar_label_workspace_bytes(4097, 3) >= 4097 * 3 * 12
    import ctypes as C
    buf8 = C.create_string_buffer(4096)
    at = C.c_void_p(C.addressof(buf8) + (-C.addressof(buf8)) % 16)
    for args, fragment in (((-1, at, 1, None, 1, 0, at, 1, 1, 10, 0, None, 0, at, 4000, at, None), b"negative"),
                           ((1, at, 1, None, 1, 1, at, 1, 33, 10, 0, None, 0, at, 4000, at, None), b"cameras_per_sweep"),
                           ((1, at, 1, None, 1, 1, at, 0, 1, 10, 0, None, 0, at, 4000, at, None), b"n_views"),
                           ((1, at, 1, None, 1, 1, at, 1, 1, -1, 0, None, 0, at, 4000, at, None), b"check_range"),
                           ((1, at, 1, None, 1, 1, at, 1, 1, 10, 2, None, 0, at, 4000, at, None), b"fourth_corner"),
                           ((1, at, 1, None, 2, 1, at, 2, 1, 10, 0, None, 0, at, 4000, at, None), b"sweep_offsets"),
                           ((1, at, 1, None, 1, 1, at, 1, 1, 10, 0, None, 0, at, 16, at, None), b"workspace"),
                           ((1, at, 1, None, 1, 1, at, 1, 1, 10, 0, None, 0, at, 4000, None, None), b"counts")):
        assert lib.sr_lidar_label_decide(*args) != 0 and fragment in lib.sr_last_error(), fragment
    assert lib.sr_lidar_vote(1, at, 1, at, 1, 9, None, at, 4000, at, at, None) != 0 and b"n_classes" in lib.sr_last_error()
    assert lib.sr_lidar_label_emit(1, at, 1, None, 1, 1, 1, at, 4000, 2, at, None, None, None, None, None) != 0 and b"n_rows" in lib.sr_last_error()

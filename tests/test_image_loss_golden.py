"""CPU: the photometric loss against tests/golden/image_loss_golden.npz, which tools/make_image_loss_golden.py wrote with the reference's
OWN utils/loss_utils.py (float32 run, autograd gradients, and the same code in float64 as the truth):
  * photometric_loss_torch -- the checker of the HIP kernels and their timing baseline -- reproduces the reference in float32 and in
    float64, under the bar of tests/image_loss_cases.py;
  * the C-ABI of the fused loss refuses bad arguments before any launch, without a GPU.
The -m gpu counterpart (tests/test_gpu_image_loss.py) runs the HIP kernels on the same fixture."""
import ctypes as C

import numpy as np
import pytest
import torch

from streetunveiler_amd import _lib
from streetunveiler_amd import image_loss  # noqa: F401  (the module under test: this file fails to import without it)
from streetunveiler_amd.build import build
from tests import image_loss_cases as ilc

CASES = ilc.fixture_cases()


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def test_fixture_covers_the_cases_it_promises():
    by = {c["name"]: c for c in CASES}
    shapes = {tuple(c["image"].shape) for c in CASES}
    assert (3, 7, 9) in shapes and (3, 37, 53) in shapes
    assert any(c["image"].shape[0] == 1 for c in CASES)
    assert len({c["lambda_dssim"] for c in CASES}) >= 2 and any(c["lambda_dssim"] == 0.2 for c in CASES)
    sky = [c for c in CASES if c["sky"] is not None]
    assert len(sky) >= 2 and all({"g_sky", "g_alpha"} <= set(c["truth"]) for c in sky)
    assert any(bool((c["alpha"] == 0).any()) and bool((c["alpha"] == 1).any()) for c in sky)
    flat = by["flat_step_c1_48x80"]     # sigma^2 out of a cancellation next to C2: the reference's own float32 deviation is largest here
    assert ilc.deviation(flat["ref"]["g_image"], flat["truth"]["g_image"], "g_image") > 1e-5
    for c in CASES:                      # the stored float32 run is the bar's unit: ratio 1 by construction
        assert all(v <= 1.0 for v in ilc.ratios(c["ref"], c).values())


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_torch_form_reproduces_the_reference(case):
    got64 = ilc.run_torch(case, torch.float64)
    ilc.assert_within_bar(got64, case, "photometric_loss_torch float64 vs truth")
    for k, truth in case["truth"].items():          # same window roundings, same formula: the float64 run IS the truth, to rounding
        assert ilc.deviation(got64[k], truth, k) <= 1e-12 * max(1.0, abs(float(np.abs(truth).max())))
    got32 = ilc.run_torch(case, torch.float32)
    ilc.assert_within_bar(got32, case, "photometric_loss_torch float32 vs truth")
    for k, truth in case["truth"].items():          # ... and the stored float32 values themselves, in the same unit
        scale = abs(float(truth)) if k in ilc.SCALARS else 1.0
        unit = max(ilc.deviation(case["ref"][k], truth, k), ilc.FLOOR * scale)
        d = ilc.deviation(got32[k], case["ref"][k], k)
        assert d <= ilc.BAR * unit, (case["name"], k, d / unit)


def test_torch_form_runs_in_any_float_dtype_and_refuses_half_a_composite():
    c = CASES[0]
    loss, l1, ssim = image_loss.photometric_loss_torch(c["image"].bfloat16(), c["gt"].bfloat16(), 0.2)
    assert loss.dtype == torch.bfloat16 and abs(float(loss) - float(c["truth"]["loss"])) < 2e-2
    with pytest.raises(ValueError, match="sky and alpha"):
        image_loss.photometric_loss_torch(c["image"], c["gt"], 0.2, sky=c["image"])


def test_cpu_tensors_are_refused():
    c = CASES[0]
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        image_loss.photometric_loss(c["image"], c["gt"])
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        image_loss.image_loss_forward(c["image"], c["gt"])


def test_package_exports_the_loss():
    import streetunveiler_amd
    assert streetunveiler_amd.photometric_loss is image_loss.photometric_loss
    assert streetunveiler_amd.photometric_loss_torch is image_loss.photometric_loss_torch
    assert streetunveiler_amd.image_loss_forward is image_loss.image_loss_forward and streetunveiler_amd.image_loss_backward is image_loss.image_loss_backward


def test_argument_errors_without_gpu(lib):
    """Refused before any launch: the pointers below are never dereferenced (no GPU is needed, and none is touched)."""
    p = C.c_void_p(4096)      # stands for a device pointer
    big = 1 << 30
    fwd = lambda W, H, Cn, image, gt, sky, alpha, ws, nbytes, out: lib.sr_image_loss_forward(W, H, Cn, 0.2, image, gt, sky, alpha, ws, nbytes, out, None)
    bwd = lambda W, H, Cn, image, gt, sky, alpha, ws, nbytes, g, gi, gs, ga: lib.sr_image_loss_backward(W, H, Cn, 0.2, image, gt, sky, alpha, ws, nbytes,
                                                                                                    g, gi, gs, ga, None)
    # 1. non-positive sizes
    for W, H, Cn in ((0, 8, 3), (8, -1, 3), (8, 8, 0)):
        assert fwd(W, H, Cn, p, p, None, None, p, big, p) == -1 and b"image size" in lib.sr_last_error()
        assert bwd(W, H, Cn, p, p, None, None, p, big, p, p, None, None) == -1 and b"image size" in lib.sr_last_error()
    # 2. a missing required pointer
    for args in ((None, p, None, None, p, big, p), (p, None, None, None, p, big, p), (p, p, None, None, None, big, p), (p, p, None, None, p, big, None)):
        assert fwd(8, 8, 3, *args) == -1 and b"NULL" in lib.sr_last_error()
    assert bwd(8, 8, 3, p, p, None, None, p, big, None, p, None, None) == -1 and b"NULL" in lib.sr_last_error()
    assert bwd(8, 8, 3, p, p, None, None, p, big, p, None, None, None) == -1 and b"NULL" in lib.sr_last_error()
    assert bwd(8, 8, 3, p, p, p, p, p, big, p, p, None, p) == -1 and b"g_sky" in lib.sr_last_error()
    # 3. only one of sky / alpha
    assert fwd(8, 8, 3, p, p, p, None, p, big, p) == -1 and b"sky and alpha" in lib.sr_last_error()
    assert fwd(8, 8, 3, p, p, None, p, p, big, p) == -1 and b"sky and alpha" in lib.sr_last_error()
    assert bwd(8, 8, 3, p, p, None, p, p, big, p, p, p, p) == -1 and b"sky and alpha" in lib.sr_last_error()
    # a workspace that is too small has a status of its own
    need = lib.sr_image_loss_workspace_bytes(8, 8, 3)
    assert fwd(8, 8, 3, p, p, None, None, p, need - 1, p) == -3 and b"workspace" in lib.sr_last_error()
    assert bwd(8, 8, 3, p, p, None, None, p, need - 1, p, p, None, None) == -3 and b"workspace" in lib.sr_last_error()


def test_workspace_bytes_are_monotone_in_the_element_count(lib):
    r = np.random.default_rng(3)
    shapes = [(1, 1, 1), (7, 9, 3), (1, 1600, 1), (41, 40, 1), (480, 320, 3), (1920, 1080, 3), (3840, 2160, 3), (1, 1, 4096), (4096, 1, 1)]
    shapes += [tuple(int(v) for v in (r.integers(1, 700), r.integers(1, 700), r.integers(1, 5))) for _ in range(200)]
    sized = sorted((W * H * Cn, lib.sr_image_loss_workspace_bytes(W, H, Cn)) for W, H, Cn in shapes)
    for (n0, b0), (n1, b1) in zip(sized, sized[1:]):
        assert (b0 == b1) if n0 == n1 else (b0 < b1), (n0, b0, n1, b1)
    assert all(b >= 12 * n for n, b in sized)          # three float planes per element (12 B per element kept for the backward)
    assert lib.sr_image_loss_workspace_bytes(0, 8, 3) == 0 and lib.sr_image_loss_workspace_bytes(8, 8, -1) == 0

"""GPU (-m gpu): the carried scan of csrc/scan.h at its chunk boundary.  One block walks an array 256 items at a time and carries the sum,
so item 257 is the first that depends on the carry.  The rest of the suite reaches that boundary in the sort's row scan (1,000,001 items =
489 blocks), in pass Y's (every full-size frame) and in the densify totals (tests/densify_cases.py P65536 / P65537 / P131073); here: the
emission scan's totals (blocks of 2048 Gaussians) and pass X's row scan (blocks of 1024 visible Gaussians), at 256 and 257 blocks, on a
64x64 frame of tiny Gaussians.  The list properties are those of tests/test_gpu_fullsize.py, by its own checker."""
import pytest
import torch

from streetunveiler_amd.synthetic import synthetic_camera, synthetic_gaussians
from tests.test_gpu_fullsize import _forward_properties

pytestmark = pytest.mark.gpu
W = H = 64


def _scene(P, seed):
    return synthetic_gaussians(P, W, H, seed=seed, scale_lo=1e-4, scale_hi=1e-3)


def _check(g, **forward_options):
    D, tiles_touched, frame_counts = _forward_properties(g, synthetic_camera(W, H), W, H, **forward_options)
    assert int(frame_counts[0]) == int(tiles_touched.sum()) == D
    assert int(frame_counts[1]) == int((tiles_touched != 0).sum())
    return int(frame_counts[1])


@pytest.mark.parametrize("P", [524_288, 524_289])
def test_emission_scan_totals_at_256_and_257_blocks(P):
    visible = _check(_scene(P, seed=3))
    assert 262_144 + 1024 < visible < P      # some Gaussians are culled; pass X's row scan is past its first chunk too


@pytest.fixture(scope="module")
def just_over_256_blocks_visible():
    """A scene with 262,145 visible Gaussians = 256 blocks of 1024 pass-X inputs and one more item, culled ones between them.  Whether a
    Gaussian is visible does not depend on the others, so the subset of a rendered scene keeps what the render counted."""
    from diff_surfel_rasterization import _C
    from tests.gpu_util import DEV, settings_for
    P0, want = 400_000, 262_145
    g = _scene(P0, seed=4)
    s = settings_for(synthetic_camera(W, H), [0, 0, 0], 3)
    e = torch.empty(0, device=DEV)
    d = {k: v.to(DEV) for k, v in g.items()}
    radii = _C.rasterize_gaussians(s.bg, d["means3D"], e, d["opacities"], d["scales"], d["rotations"], 1.0, e, s.viewmatrix, s.projmatrix,
                                   s.tanfovx, s.tanfovy, H, W, d["shs"], 3, s.campos, False, False, forward_only=True)[3]
    seen = (radii > 0).cpu()
    assert int(seen.sum()) > want and int((~seen).sum()) > 1000
    keep = ~seen | (torch.cumsum(seen, 0) <= want)      # every culled Gaussian and the first `want` visible ones, in place
    return {k: v[keep].contiguous() for k, v in g.items()}, want


@pytest.mark.parametrize("ballot_ranking", [False, True])
def test_pass_x_row_scan_at_257_blocks(just_over_256_blocks_visible, ballot_ranking):
    g, want = just_over_256_blocks_visible
    assert _check(g, ballot_ranking=ballot_ranking) == want

"""The two blend pairs of the 16x16 tile with three colour channels -- the one-wave-per-tile kernels of the large frames and the cooperative
four-waves-per-tile kernels the library picks below COOP_BELOW_TILES tiles -- held to each other on one scene.  Used by the parity tests
(tests/gpu_util.py re-exports it) and by tools/fuzz_parity.py.  A pair is forced the way SURFEL_EXTRA_FLAGS forces an A/B switch: its
SR_FLAG_* bit OR-ed into every operator call of the block (diff_surfel_rasterization._C._EXTRA_FLAGS, read at call time), so any
run_hip-style runner serves, forward and backward alike."""
import contextlib

import numpy as np

from tests.bars import bar

COOP_BELOW_TILES = 2600   # csrc/render_bwd.hip kCoopBelowTiles: the default picks the cooperative pair below this many 16x16 tiles, one wave per tile above


@contextlib.contextmanager
def forced_pair(kernel):
    """Inside the block every operator call (forward and backward) runs the blend pair `kernel`: None (the library's pick), "one_wave", "coop"."""
    from diff_surfel_rasterization import _C
    from streetunveiler_amd import _lib as L
    saved = _C._EXTRA_FLAGS
    _C._EXTRA_FLAGS = saved | {None: 0, "one_wave": L.SR_FLAG_ONE_WAVE_BACKWARD, "coop": L.SR_FLAG_COOP_BACKWARD}[kernel]
    try:
        yield
    finally:
        _C._EXTRA_FLAGS = saved


def _bits(a):
    """Bit pattern of an array (NaN / Inf included) for bit-identity checks."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
    return a is None and b is None or (a is not None and b is not None and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)))


def assert_blend_variants(run, n_tiles, raw=None, tag=""):
    """The HIP-vs-HIP contract of the blend kernels on one scene.  `run(backward_kernel=, row_mapped=)` -> run_hip-style dict (outputs and
    gradients); `raw(backward_kernel=, row_mapped=)` -> run_hip_raw-style dict (its final_T / n_contrib are compared too), or None.
      * color, allmap, radii (and final_T, n_contrib) bit-identical across the default, "one_wave", "coop" (the cooperative forward too),
        row_mapped=True and row_mapped=False;
      * the default's gradients bit-identical to those of the kernel the tile-count rule picks (coop below COOP_BELOW_TILES, one-wave above),
        and to the two forced forward mappings' (test_row_mapped_forward_is_bit_identical's contract);
      * one-wave twice and coop twice: the same bits;
      * one-wave vs coop: every finite gradient within bar("class_grads_vs_operator") of the tensor scale (summation order only), the same
        elements non-finite.
    -> (one-wave result, coop result): the caller holds BOTH to its oracle assertions."""
    configs = [dict(), dict(backward_kernel="one_wave"), dict(backward_kernel="coop"), dict(row_mapped=True), dict(row_mapped=False)]
    outs = [run(**c) for c in configs]
    one2, coop2 = run(backward_kernel="one_wave"), run(backward_kernel="coop")
    raws = [raw(**c) for c in configs] if raw is not None else None
    for c, o, r in zip(configs[1:], outs[1:], (raws or [None] * len(configs))[1:]):
        for k in ("color", "allmap", "radii"):
            assert _same_bits(o[k], outs[0][k]), f"{tag} {c}: {k} differs from the default forward's"
        if r is not None:
            for k in ("color", "allmap", "radii", "final_T", "n_contrib"):
                a, b = (r[k], raws[0][k]) if k in r else (r["img"][k], raws[0]["img"][k])
                assert _same_bits(a, b), f"{tag} {c}: {k} differs from the default forward's"
    default, one, coop, rows, quads = outs
    picked = coop if n_tiles < COOP_BELOW_TILES else one
    grads = [k for k in default if k.startswith("dL_") and default[k] is not None]
    assert grads, f"{tag}: no gradients (pass dc / da)"
    for k in grads:
        assert _same_bits(default[k], picked[k]), f"{tag} {k}: the default is not the {'cooperative' if picked is coop else 'one-wave'} kernel at {n_tiles} tiles"
        assert _same_bits(rows[k], default[k]) and _same_bits(quads[k], default[k]), f"{tag} {k}: a forced forward mapping changes the gradient"
        assert _same_bits(one2[k], one[k]), f"{tag} {k}: the one-wave backward is not deterministic"
        assert _same_bits(coop2[k], coop[k]), f"{tag} {k}: the cooperative backward is not deterministic"
        a, b = np.asarray(one[k], np.float64), np.asarray(coop[k], np.float64)
        fin = np.isfinite(a)
        assert np.array_equal(fin, np.isfinite(b)), f"{tag} {k}: one-wave and cooperative gradients are non-finite at different elements"
        scale = np.abs(a[fin]).max(initial=0.0) + 1e-30
        err = np.abs(a[fin] - b[fin]).max(initial=0.0)
        assert err <= bar("class_grads_vs_operator") * scale, f"{tag} {k}: cooperative vs one-wave differ by {err / scale:.2e} of the tensor scale"
    return one, coop


def blend_variants(g, cam, bg, deg, dc, da, **run_hip_kwargs):
    """assert_blend_variants on tests/gpu_util.py run_hip / run_hip_raw of one scene: 16x16 tiles, three colour channels, culling on only (the
    flags that force a blend pair are documented for that case alone).  `run_hip_kwargs`: colors / Tpre.  -> (one-wave result, coop result),
    run_hip dicts."""
    from tests.gpu_util import run_hip, run_hip_raw
    assert run_hip_kwargs.get("tile") in (None, (16, 16)) and run_hip_kwargs.get("quadrant_cull", True), "the blend pairs exist for 16x16, culling on"
    colors = run_hip_kwargs.get("colors")
    assert colors is None or np.shape(colors)[-1] == 3, "three colour channels"
    raw_kw = {k: v for k, v in run_hip_kwargs.items() if k in ("colors", "Tpre", "tile")}
    n_tiles = ((cam.image_width + 15) // 16) * ((cam.image_height + 15) // 16)

    def run(backward_kernel=None, row_mapped=None):
        with forced_pair(backward_kernel):
            return run_hip(g, cam, bg, deg, dc, da, row_mapped=row_mapped, **run_hip_kwargs)

    def raw(backward_kernel=None, row_mapped=None):
        with forced_pair(backward_kernel):
            return run_hip_raw(g, cam, bg, deg, row_mapped=row_mapped, **raw_kw)
    return assert_blend_variants(run, n_tiles, raw=raw, tag=f"{cam.image_width}x{cam.image_height}")

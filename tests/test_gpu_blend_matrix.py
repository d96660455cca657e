"""GPU (-m gpu): every blend-kernel instantiation against the CPU oracle on the edge scenes (tools/edge_scenes.py).

launch_render_forward / launch_render_backward dispatch to about twenty template instantiations (colour channels 3 / 6 / 9 x five tile
shapes, the banded walk of the 32x16 tile, kXG = false, the row-mapped pair); the edge-case tests of tests/test_gpu_parity.py reach the two
16x16 three-channel ones.  Here one parametrised test runs scene x configuration, a configuration being (NC, tile, colour gradients
wanted?, pair):

  NC = 3: tiles 8x8, 16x8, 32x8, 32x16, and 16x16 with backward_kernel="rows"
  NC = 6 (colors_precomp[P,6]): the five shapes with colour gradients, 16x16 also without (kXG = false)
  NC = 9 (shs + extra_colors[P,6]): the same six

Reference: the CPU oracle run with the same tile shape as the three-channel renders the reference program itself would run -- the SH render
(or, with six channels, the first precomputed-colour render) carrying the allmap gradient, the other precomputed-colour renders with a zero
allmap gradient -- images concatenated, geometry gradients summed, colour-side gradients from their own pass.  One reference per
(scene, tile, pass), shared by the configurations.  Assertions and bars per scene are those of the scene's 16x16 test in
tests/test_gpu_parity.py (tests/bars.py: nothing new, nothing wider); `ties` and `ragged_bands` also meet the free-running float64
reference.  Cross-checks: NC = 6 / 9 reproduce the NC = 3 forward bit for bit, kXG = false changes no other gradient's bits, every cell run
twice gives the same bits."""
import numpy as np
import pytest
import torch

from tests.bars import bar

pytestmark = pytest.mark.gpu

TILES = [(8, 8), (16, 8), (32, 8), (32, 16), (16, 16)]
CONFIGS = [(3, t, True, None) for t in TILES[:4]] + [(3, (16, 16), True, "rows")]
for _nc in (6, 9):
    CONFIGS += [(_nc, t, True, None) for t in TILES] + [(_nc, (16, 16), False, None)]
assert len(CONFIGS) == 17
GEOMETRY = ["dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D"]
PASSES = {3: [("sh", True)], 6: [("p0", True), ("p1", False)], 9: [("sh", True), ("p0", False), ("p1", False)]}   # (pass, carries the allmap gradient)
FREE_F64_SCENES = ("ties", "ragged_bands")   # the scenes the float64 reference is run on (ties: as at 16x16 today)


def _scene_names():
    from tools.edge_scenes import catalogue
    return list(catalogue())


def _config_id(c):
    nc, tile, want, pair = c
    return f"nc{nc}-{tile[0]}x{tile[1]}" + ("" if want else "-noxg") + (f"-{pair}" if pair else "")


CELLS = [pytest.param(s, c, id=f"{s}-{_config_id(c)}") for s in _scene_names() for c in CONFIGS]   # scene-major: the caches below hold one scene


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from streetunveiler_amd import _lib
    _lib.load()
    yield
    _CACHE.clear()


# ---- one scene at a time: the scene, its references per (tile, pass), its HIP results per configuration --------------------------------
_CACHE = {}


def _state(name):
    if _CACHE.get("name") != name:
        from tools.edge_scenes import catalogue
        _CACHE.clear()
        _CACHE.update(name=name, scene=catalogue()[name](), ref={}, hip={}, raw={})
    return _CACHE


def _pass_inputs(sc, p, with_da):
    """-> (bg[3], sh degree, colours or None, dc[3,H,W], da[7,H,W]) of one three-channel reference render."""
    k = {"sh": 0, "p0": 1, "p1": 2}[p]
    da = sc.da if with_da else torch.zeros_like(sc.da)
    return sc.bg9[3 * k:3 * k + 3], (sc.deg if p == "sh" else 0), (None if p == "sh" else sc.extra[:, 3 * k - 3:3 * k].copy()), sc.dc9[3 * k:3 * k + 3].contiguous(), da


def _ref_forward(name, tile, p):
    from tests.gpu_util import run_oracle
    st = _state(name)
    key = ("fwd", tile, p)
    if key not in st["ref"]:
        sc = st["scene"]
        bg, deg, colors, _, _ = _pass_inputs(sc, p, True)
        st["ref"][key] = run_oracle(sc.g, sc.cam, bg, deg, colors=colors, tile=tile)[0]
    return st["ref"][key]


def _ref_backward(name, tile, p, with_da):
    from oracle import surfel_oracle as so
    st = _state(name)
    key = ("bwd", tile, p, with_da)
    if key not in st["ref"]:
        _, _, _, dc, da = _pass_inputs(st["scene"], p, with_da)
        st["ref"][key] = so.rasterize_backward(_ref_forward(name, tile, p), dc.numpy(), da.numpy())
    return st["ref"][key]


def _ref_f64(name, tile, p, with_da, decisions):
    """Free-running float64 forward + margins of one pass (once), its float64 backward for this allmap gradient -> (fwd64, bwd64, margins)."""
    from oracle import surfel_oracle as so
    from tests.gpu_util import free_f64_reference
    st = _state(name)
    sc = st["scene"]
    key = ("f64", tile, p)
    if key not in st["ref"]:
        bg, deg, colors, _, _ = _pass_inputs(sc, p, True)
        fwd64, _, margins = free_f64_reference(sc.g, sc.cam, bg, deg, tile=tile, colors=colors, base=_ref_forward(name, tile, p), kernel_decisions=decisions)
        st["ref"][key] = (fwd64, margins)
    fwd64, margins = st["ref"][key]
    bkey = ("b64", tile, p, with_da)
    if bkey not in st["ref"]:
        _, _, _, dc, da = _pass_inputs(sc, p, with_da)
        st["ref"][bkey] = so.rasterize_backward(fwd64, dc.numpy(), da.numpy())
    return fwd64, st["ref"][bkey], margins


def _summed_reference(name, nc, tile):
    """The float32 oracle's passes of an NC-channel render put together -> (fwd: color [NC,H,W], allmap, radii; bwd: geometry summed, dL_dsh /
    dL_dcolors / dL_dextra from their own passes)."""
    fwds = [_ref_forward(name, tile, p) for p, _ in PASSES[nc]]
    bwds = [_ref_backward(name, tile, p, with_da) for p, with_da in PASSES[nc]]
    fwd = dict(color=np.concatenate([f["color"] for f in fwds], 0), allmap=fwds[0]["allmap"], radii=fwds[0]["radii"])
    bwd = {k: sum(np.asarray(b[k], np.float64) for b in bwds) for k in GEOMETRY}
    if nc != 6:
        bwd["dL_dsh"] = bwds[0]["dL_dsh"]
    if nc != 3:
        bwd["dL_dcolors" if nc == 6 else "dL_dextra"] = np.concatenate([b["dL_dcolors"] for b in bwds[-2:]], 1)
    return fwd, bwd


def _hip(name, config):
    """The cell's HIP result (run_hip-style dict), run TWICE: the same bits."""
    from tools.blend_pairs import _same_bits
    st = _state(name)
    if config not in st["hip"]:
        a, b = _run_hip_cell(st["scene"], config), _run_hip_cell(st["scene"], config)
        for k in a:
            assert _same_bits(a[k], b[k]), f"{name} {_config_id(config)}: {k} differs between two runs of the same cell"
        st["hip"][config] = a
    return st["hip"][config]


def _run_hip_cell(sc, config):
    from diff_surfel_rasterization import GaussianRasterizer
    from tests.gpu_util import DEV, settings_for
    nc, tile, want, pair = config
    cam, g = sc.cam, sc.g
    P = g["means3D"].shape[0]
    t = {k: g[k].to(DEV).clone().requires_grad_() for k in ("means3D", "opacities", "scales", "rotations")}
    m2d = torch.zeros(P, 3, device=DEV, requires_grad=True)
    kw = dict(means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    ex = shs = None
    if nc != 6:
        shs = g["shs"].to(DEV).clone().requires_grad_(); kw["shs"] = shs
    if nc != 3:
        ex = torch.as_tensor(sc.extra).to(DEV).clone().requires_grad_(want)
        kw["colors_precomp" if nc == 6 else "extra_colors"] = ex
    bg = {3: sc.bg9[:3], 6: sc.bg9[3:], 9: sc.bg9}[nc]
    dc = {3: sc.dc9[:3], 6: sc.dc9[3:], 9: sc.dc9}[nc].contiguous()
    color, radii, allmap = GaussianRasterizer(settings_for(cam, bg, 0 if nc == 6 else sc.deg), tile=None if tile == (16, 16) else tile, backward_kernel=pair)(**kw)
    ((color * dc.to(DEV)).sum() + (allmap * sc.da.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    z = lambda x: None if x is None or x.grad is None else x.grad.cpu().numpy()
    out = dict(color=color.detach().cpu().numpy(), allmap=allmap.detach().cpu().numpy(), radii=radii.cpu().numpy(), dL_dmeans3D=z(t["means3D"]),
               dL_dopacity=z(t["opacities"]), dL_dscales=z(t["scales"]), dL_drotations=z(t["rotations"]), dL_dmeans2D=z(m2d))
    if nc != 6:
        out["dL_dsh"] = z(shs)
    if nc != 3:
        out["dL_dcolors" if nc == 6 else "dL_dextra"] = z(ex)
    return out


def _raw(name, tile):
    """The three-channel forward's state buffers (binning, n_contrib) of this tile shape; with the pair decisions where the float64 reference
    or the band precondition needs them."""
    from tests.gpu_util import run_hip_raw
    st = _state(name)
    if tile not in st["raw"]:
        sc = st["scene"]
        st["raw"][tile] = run_hip_raw(sc.g, sc.cam, sc.bg9[:3], sc.deg, tile=None if tile == (16, 16) else tile,
                                      decisions=name in FREE_F64_SCENES and sc.g["means3D"].shape[0] > 0)
    return st["raw"][tile]


def _grad_names(config):
    nc, _, want, _ = config
    return GEOMETRY + (["dL_dsh"] if nc != 6 else []) + ([] if nc == 3 or not want else ["dL_dcolors" if nc == 6 else "dL_dextra"])


# ---- what a scene asserts: the assertions of its 16x16 test in tests/test_gpu_parity.py, same bars -------------------------------------
def _assert_oracle_bars(name, config, out, finite=False, invisible_zero=False):
    """_check_images + _check_grads against the (summed) float32 oracle: test_cloned_gaussians_and_depth_ties / _very_long_tile_lists / _degenerate_parameters."""
    from tests.test_gpu_parity import _check_grads, _check_images
    nc, tile, _, _ = config
    tag = f"{name} {_config_id(config)}"
    fwd, bwd = _summed_reference(name, nc, tile)
    names = _grad_names(config)
    np.testing.assert_array_equal(out["radii"], fwd["radii"], err_msg=tag)
    if finite:
        for a in [out["color"], out["allmap"], fwd["color"], fwd["allmap"]] + [out[n] for n in names] + [bwd[n] for n in names]:
            assert np.isfinite(np.asarray(a)).all(), tag
    _check_images(out, fwd, tag)
    _check_grads(out, bwd, names, tag)
    if invisible_zero:   # invisible Gaussians get exactly zero gradient
        inv = fwd["radii"] == 0
        for k in names:
            assert not np.asarray(out[k])[inv].any(), (tag, k)


def _assert_tiny(name, config, out):
    """test_very_long_tile_lists_and_tiny_images, the frames smaller than a tile."""
    nc, tile, _, _ = config
    fwd, bwd = _summed_reference(name, nc, tile)
    np.testing.assert_array_equal(out["radii"], fwd["radii"])
    np.testing.assert_allclose(out["color"], fwd["color"], atol=2e-4)
    np.testing.assert_allclose(out["allmap"][[0, 1, 2, 3, 4, 6]], fwd["allmap"][[0, 1, 2, 3, 4, 6]], atol=2e-3, rtol=2e-3)
    for k in [n for n in _grad_names(config) if n != "dL_dmeans2D"]:
        sc = np.abs(bwd[k]).max() + 1e-20
        assert np.abs(out[k].reshape(np.shape(bwd[k])) - bwd[k]).max() <= 2e-2 * sc, (name, _config_id(config), k)


def _assert_non_finite(name, config, out):
    """test_non_finite_parameters_do_not_spread."""
    sc = _state(name)["scene"]
    P = sc.g["means3D"].shape[0]
    idx = sc.poisoned
    healthy = np.ones(P, bool); healthy[idx] = False
    names = _grad_names(config)
    tag = f"{sc.field} = {sc.value} {_config_id(config)}"
    assert np.isfinite(out["color"]).all() and np.isfinite(out["allmap"]).all(), tag
    bad = {k: ~np.isfinite(np.asarray(out[k]).reshape(P, -1)).all(1) for k in names}
    assert not any(b[healthy].any() for b in bad.values()), f"{tag}: a healthy Gaussian has a non-finite gradient row"
    if sc.field in ("means3D", "scales", "rotations"):
        assert not out["radii"][idx].any() and not any(b.any() for b in bad.values()), f"{tag}: the poisoned Gaussians must be culled"
        for k in names:
            assert not np.asarray(out[k]).reshape(P, -1)[idx].any(), f"{tag}: {k} of a culled Gaussian is not zero"


def _assert_nothing_rendered(name, config, out):
    """test_empty_and_all_culled_inputs."""
    sc = _state(name)["scene"]
    nc = config[0]
    H, W = sc.cam.image_height, sc.cam.image_width
    bg = {3: sc.bg9[:3], 6: sc.bg9[3:], 9: sc.bg9}[nc]
    np.testing.assert_allclose(out["color"], np.broadcast_to(bg[:, None, None], (nc, H, W)))
    assert not out["allmap"].any() and not out["radii"].any() and out["radii"].shape == (sc.g["means3D"].shape[0],)
    if name == "all_culled":   # (P == 0: the images only, as in test_empty_and_all_culled_inputs -- there is no row to hold a gradient)
        for k in _grad_names(config):
            assert not out[k].any(), k


def _assert_free_f64(name, config, out):
    """The free-running float64 reference (its own decisions): _full_check's assert_free_parity for three channels; for 6 / 9 channels the
    per-pass images at the checker's robust pixels and the per-Gaussian sums of tests/test_gpu_class_pass_oracle.py."""
    from tests import gpu_util as gu
    nc, tile, want, _ = config
    sc = _state(name)["scene"]
    g, cam, budgets = sc.g, sc.cam, sc.budgets
    raw = _raw(name, tile)
    tag = f"{name} {_config_id(config)} "
    if nc == 3:
        xfwd, xbwd, margins = _ref_f64(name, tile, "sh", True, raw["decisions"])
        gu.assert_free_parity(out, raw["img"]["n_contrib"].view(np.uint32), xfwd, xbwd, margins, tag=tag, scene=(g, cam), **budgets)
        return
    total = gu._Sum(g)
    colour_rows = []
    for i, (p, with_da) in enumerate(PASSES[nc]):
        fwd64, bwd64, margins = _ref_f64(name, tile, p, with_da, raw["decisions"])
        total.add(None, fwd64, bwd64, margins, _ref_backward(name, tile, p, with_da))
        got = out["color"][3 * i:3 * i + 3]
        if i == 0:   # the pass that carries the allmap: every map, the non-robust share within the scene's budget
            gu.assert_free_parity(dict(color=got, allmap=out["allmap"]), None, fwd64, None, margins, tag=tag + p + " ", **{k: v for k, v in budgets.items() if k == "pixel_budget"})
            vis = fwd64["radii"] > 0
            share = 1.0 - (vis & (margins["gaussian"] > 1.0)).sum() / max(1, vis.sum())
            assert share <= budgets.get("gaussian_budget", gu.NONROBUST_GAUSSIAN_BUDGET), f"{tag}: {share:.2f} of the visible Gaussians are non-robust"
        else:
            err = np.abs(got.astype(np.float64) - fwd64["color"]) / (1.0 + np.abs(fwd64["color"])) - margins.get("value_noise", 0.0)
            rob = np.broadcast_to(margins["pixel"] > 1.0, err.shape)
            assert err[rob].max(initial=0.0) <= bar("robust_pixel") and err[~rob].max(initial=0.0) <= bar("nonrobust_pixel_cap"), f"{tag}: channels of pass {p}"
        if p == "sh":
            colour_rows.append(("dL_dsh", np.asarray(bwd64.get("dL_dsh64", bwd64["dL_dsh"]), np.float64)))
        elif want:
            colour_rows.append((p, np.asarray(bwd64.get("dL_dcolors64", bwd64["dL_dcolors"]), np.float64)))
    leaf = {v: k for k, v in gu.KEYS.items()}
    gu._check_rows({leaf[k]: out[k] for k in GEOMETRY}, total, g, cam, tag)
    rob = total.visible & total.robust
    P = total.P
    refs = [(n, r) for n, r in colour_rows if n == "dL_dsh"]
    if want:
        refs.append(("dL_dcolors" if nc == 6 else "dL_dextra", np.concatenate([r for n, r in colour_rows if n != "dL_dsh"], 1)))
    for k, ref in refs:   # colour-side gradients: each comes from one render only
        e = gu.row_errors(out[k], ref, np.ones(P, bool))
        assert gu.rows_within(e[rob], bar("row_p999"), bar("row_max")), f"{tag} {k}: robust rows p99.9 {np.quantile(e[rob], 0.999):.2e}, max {e[rob].max():.2e}"


def _assert_band_precondition(name):
    """ragged_bands must exercise both branches of the banded walk's flush (`add && written[slot]` and its else): list entries that blend
    into the upper 32x8 band of their 32x16 tile only, into the lower one only, into both -- in the frame and in its cut last tile row --
    counted from the kernels' own pair decisions."""
    from tools.edge_scenes import band_coverage
    st = _state(name)
    if "bands" not in st:
        sc = st["scene"]
        W, H = sc.cam.image_width, sc.cam.image_height
        assert all(W % t for t in (8, 16, 32)) and all(H % t for t in (8, 16)) and 9 <= H % 16 <= 15
        raw = _raw(name, (32, 16))
        st["bands"] = band_coverage(raw["decisions"]["valid"], raw["bin"]["ranges"], raw["img"]["n_contrib"].view(np.uint32).reshape(2, H, W)[0], W, H)
    cov = st["bands"]
    for last_row in (False, True):
        for which in ("upper", "lower", "both"):
            assert cov.get((last_row, which), 0) >= 20, f"ragged_bands: {cov.get((last_row, which), 0)} list entries reach the {which} band(s) {'in the last tile row' if last_row else 'above the last tile row'}: {cov}"


def _assert_cross_checks(name, config, out):
    from tests.gpu_util import run_hip
    from tools.blend_pairs import _bits, _same_bits
    nc, tile, want, pair = config
    tag = f"{name} {_config_id(config)}"
    sc = _state(name)["scene"]
    if nc != 3:   # the three-channel forward of this scene and tile, bit for bit (NaN-aware)
        three = _hip(name, (3, tile, True, None))
        assert np.array_equal(_bits(out["allmap"]), _bits(three["allmap"])) and np.array_equal(out["radii"], three["radii"]), f"{tag}: allmap / radii differ from the three-channel render's"
        if nc == 9:
            assert np.array_equal(_bits(out["color"][:3]), _bits(three["color"])), f"{tag}: channels 0..2 differ from the three-channel render's"
            six = _hip(name, (6, tile, True, None))
            assert np.array_equal(_bits(out["color"][3:]), _bits(six["color"])), f"{tag}: channels 3..8 differ from the six-channel render's"
        else:
            c3 = run_hip(sc.g, sc.cam, sc.bg9[3:6], 0, colors=sc.extra[:, :3].copy(), tile=None if tile == (16, 16) else tile)
            assert np.array_equal(_bits(out["color"][:3]), _bits(c3["color"])), f"{tag}: channels 0..2 differ from a three-channel render of the same colours"
    if not want:   # kXG = false: no colour gradient, every other gradient bit for bit that of the run which forms it
        k = "dL_dcolors" if nc == 6 else "dL_dextra"
        assert out[k] is None or not out[k].any(), f"{tag}: {k} formed although nobody wants it"
        full = _hip(name, (nc, tile, True, None))
        assert full[k] is not None or sc.g["means3D"].shape[0] == 0   # (P == 0: there is no row to hold a gradient)
        for n in _grad_names(config):
            assert _same_bits(out[n], full[n]), f"{tag}: {n} differs from the run that forms the colour gradients"


@pytest.mark.parametrize("scene,config", CELLS)
def test_blend_instantiation_on_edge_scene(scene, config):
    from tests.test_gpu_parity import _check_binning
    nc, tile, want, pair = config
    st = _state(scene)
    sc = st["scene"]
    P = sc.g["means3D"].shape[0]
    if scene == "ragged_bands":
        _assert_band_precondition(scene)
    # binning of this tile shape against the oracle's: lists, ranges, radii bit-exact
    raw = _raw(scene, tile)
    if P:
        _check_binning(raw, _ref_forward(scene, tile, "sh"))
    else:
        assert raw["D"] == 0
    out = _hip(scene, config)
    assert out["color"].shape[0] == nc
    if scene.startswith("tiny_"):
        _assert_tiny(scene, config, out)
    elif scene.startswith("non_finite_"):
        _assert_non_finite(scene, config, out)
    elif scene in ("no_gaussians", "all_culled"):
        _assert_nothing_rendered(scene, config, out)
    else:
        _assert_oracle_bars(scene, config, out, finite=scene == "degenerate", invisible_zero=scene in FREE_F64_SCENES)
    if scene in FREE_F64_SCENES:
        _assert_free_f64(scene, config, out)
    _assert_cross_checks(scene, config, out)


# ---- the 16x16 forward kernels that are not the band kernel: the same bits ---------------------------------------------------------------
# The cooperative forward (backward_kernel="coop", culling on) and the counting variant (blend_counters; three and six channels) share the
# band kernel's per-pixel step, initialisation, stores and hit-mask packing (csrc/blend_common.h).  On a frame that is a multiple of no tile
# and on one whose pixels saturate: images and per-pixel state bit for bit the band kernel's, and -- the hit masks -- the one-wave backward
# fed with the variant's state gives the band kernel's gradients bit for bit.
FORWARD_VARIANTS = {"coop": (3, dict(backward_kernel="coop")), "counting-nc3": (3, dict(blend_counters=True)), "counting-nc6": (6, dict(blend_counters=True))}
_BAND = {}


def _forward_then_one_wave_backward(sc, nc, **forward_kw):
    import diff_surfel_rasterization._C as _C
    from tests.gpu_util import DEV, settings_for
    g, cam = sc.g, sc.cam
    W, H, P = cam.image_width, cam.image_height, g["means3D"].shape[0]
    e = torch.empty(0, device=DEV)
    d = lambda k: g[k].to(DEV)
    bg, dc = (sc.bg9[:3], sc.dc9[:3]) if nc == 3 else (sc.bg9[3:], sc.dc9[3:])
    s = settings_for(cam, bg, sc.deg if nc == 3 else 0)
    sh, col = (d("shs"), e) if nc == 3 else (e, torch.as_tensor(sc.extra).to(DEV))
    deg = sc.deg if nc == 3 else 0
    if forward_kw.get("blend_counters"):
        forward_kw = dict(forward_kw, blend_counters=torch.zeros(16, dtype=torch.int64, device=DEV))
    D, color, allmap, radii, geom, binning, img = _C.rasterize_gaussians(s.bg, d("means3D"), col, d("opacities"), d("scales"), d("rotations"), 1.0, e, s.viewmatrix,
                                                                          s.projmatrix, s.tanfovx, s.tanfovy, H, W, sh, deg, s.campos, False, False, **forward_kw)
    if "blend_counters" in forward_kw:
        torch.cuda.synchronize()
        assert int(forward_kw["blend_counters"][0]) > 0, "the counting variant did not run"
    iv = _C.image_view(img, W, H)
    out = dict(color=color, allmap=allmap, radii=radii, final_T=iv["final_T"].clone(), n_contrib=iv["n_contrib"].clone())
    grads = _C.rasterize_gaussians_backward(s.bg, d("means3D"), radii, col, d("scales"), d("rotations"), 1.0, e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy,
                                            dc.contiguous().to(DEV), sc.da.to(DEV), sh, deg, s.campos, geom, D, binning, img, False, backward_kernel="one_wave")
    torch.cuda.synchronize()
    out.update({f"grad{i}": t for i, t in enumerate(grads) if torch.is_tensor(t)})
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("variant", list(FORWARD_VARIANTS))
@pytest.mark.parametrize("scene", ["ragged_bands", "opacity_extremes_2"])
def test_forward_variant_is_bit_identical_to_the_band_kernel(scene, variant):
    from tools.blend_pairs import _same_bits
    from tools.edge_scenes import catalogue
    nc, kw = FORWARD_VARIANTS[variant]
    if _BAND.get("scene") != scene:
        _BAND.clear()
        _BAND.update(scene=scene, sc=catalogue()[scene]())
    sc = _BAND["sc"]
    if nc not in _BAND:   # the band kernel (SR_FLAG_QUADRANT_MAPPED_FORWARD), once per scene and channel count
        _BAND[nc] = _forward_then_one_wave_backward(sc, nc, row_mapped=False)
    band = _BAND[nc]
    W, H = sc.cam.image_width, sc.cam.image_height
    if scene == "ragged_bands":
        assert W % 16 and H % 16
    else:   # pixels that stopped at the transmittance floor (kTStop = 1e-4 of common.h) with list entries left
        assert (band["final_T"][0] < 1e-3).mean() > 0.05, "the scene does not saturate"
    assert band["n_contrib"].any() and np.abs(band["grad3"]).max() > 0
    got = _forward_then_one_wave_backward(sc, nc, **kw)
    assert set(got) == set(band)
    for k in band:
        assert _same_bits(got[k], band[k]), f"{scene} {variant}: {k} differs from the band kernel's"

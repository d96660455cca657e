"""CPU: the sky model's torch restatement against an independent float64 numpy restatement of the same contract, its grid layout, its
state_dict, the bar's power to reject wrong models, and the new entry points' refusals.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sky_cases as sc
from streetunveiler_amd import _lib, sky
from streetunveiler_amd.build import build

U32 = 1 << 32


# ---- an independent restatement: scalar numpy, pixel by pixel, sharing no code with streetunveiler_amd/sky.py -------------------------
def np_levels():
    out, first = [], 0
    for l in range(16):
        res = 16 * 2 ** l
        rows = min(-(-res ** 3 // 8) * 8, 65536)
        out.append((res - 1.0, res, rows, first, res ** 3 > 65536))
        first += rows
    return out, first


def np_saturate(v):
    if not v >= 0:          # negative or NaN
        return 0
    return U32 - 1 if v >= U32 else int(v)


def np_row(level, corner):
    scale, res, rows, first, hashed = level
    if hashed:
        index = (corner[0] * 1 % U32) ^ (corner[1] * 2654435761 % U32) ^ (corner[2] * 805459861 % U32)
    else:
        index = (corner[0] + corner[1] * res + corner[2] * res * res) % U32
    return index % rows + first


def np_grid(params, x, plus_half=True):
    table, feats = params.reshape(-1, 2), []
    for level in np_levels()[0]:
        p = [x[d] * level[0] + (0.5 if plus_half else 0.0) for d in range(3)]
        cell = [np_saturate(math.floor(v) if math.isfinite(v) else v) for v in p]
        frac = [v - math.floor(v) if math.isfinite(v) else float("nan") for v in p]
        f = np.zeros(2)
        for bits in range(8):
            b = [(bits >> d) & 1 for d in range(3)]
            wgt = np.prod([frac[d] if b[d] else 1.0 - frac[d] for d in range(3)])
            f = f + wgt * table[np_row(level, [(cell[d] + b[d]) % U32 for d in range(3)])]
        feats += list(f)
    return np.array(feats)


def np_sh(d, flip=False, normalise=False):
    x, y, z = d / np.linalg.norm(d) if normalise else d
    s = -1.0 if flip else 1.0
    return np.array([0.28209479177387814, s * -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
                     1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.94617469575755997 * z * z - 0.31539156525251999,
                     -1.0925484305920792 * x * z, 0.54627421529603959 * (x * x - y * y), 0.59004358992664352 * y * (-3 * x * x + y * y),
                     2.8906114426405538 * x * y * z, 0.45704579946446572 * y * (1 - 5 * z * z), 0.3731763325901154 * z * (5 * z * z - 3),
                     0.45704579946446572 * x * (1 - 5 * z * z), 1.4453057213202769 * z * (x * x - y * y),
                     0.59004358992664352 * x * (-x * x + 3 * y * y)])


def np_embed(x, sin_first=True):
    out = list(x)
    for k in range(10):
        a, b = np.sin(x * 2.0 ** k), np.cos(x * 2.0 ** k)
        out += list(a) + list(b) if sin_first else list(b) + list(a)
    return np.array(out)


def np_image(case, flip=False, normalise=False, plus_half=True, sin_first=True, relu_last=False):
    s = {k: v.double().numpy() for k, v in case["state"].items()}
    K, c2w = case["K"].double().numpy(), case["c2w"].double().numpy()
    pos = c2w[:3, 3]
    tail = np.concatenate([np_grid(s["params"], pos, plus_half), np_embed(pos, sin_first)])
    out = np.zeros((3, case["H"], case["W"]))
    for j in range(case["H"]):
        for i in range(case["W"]):
            dirs = np.array([(i - K[0, 2]) / K[0, 0], -(j - K[1, 2]) / K[1, 1], -1.0])
            h = np.concatenate([np_sh(c2w[:3, :3] @ dirs, flip, normalise), tail])
            for k in range(3):
                h = np.maximum(s[f"w{k}"] @ h + s[f"b{k}"], 0.0)
            z = s["w3"] @ h + s["b3"]
            out[:, j, i] = 1.0 / (1.0 + np.exp(-(np.maximum(z, 0.0) if relu_last else z)))
    return out


def _case(name):
    return next(c for c in sc.CASES if c["name"] == name)


# ---- the grid's layout -----------------------------------------------------------------------------------------------------------------
def test_level_sizes_and_total():
    rows = [level[2] for level in sky.GRID_LEVELS]
    assert rows == [4096, 32768] + [65536] * 14 and sky.GRID_ROWS == 954368 and sky.GRID_PARAMS == 1908736
    assert [level[1] for level in sky.GRID_LEVELS] == [16 * 2 ** l for l in range(16)]
    assert [level[4] for level in sky.GRID_LEVELS] == [False, False] + [True] * 14
    assert sky.INPUT_CHANNELS == 111


def test_row_indices_by_hand():
    # level 0 (dense, 16^3): x = (0.31, 0.62, 0.17): p = x * 15 + 0.5 = (5.15, 9.8, 3.05) -> cell (5, 9, 3); corner 0: 5 + 9*16 + 3*256 = 917,
    # corner 7 = cell + (1, 1, 1): 6 + 10*16 + 4*256 = 1190.  level 1 (dense, 32^3, after 4096 rows): p = x * 31 + 0.5 = (10.11, 19.72, 5.77):
    # 10 + 19*32 + 5*1024 = 5738, + 4096.  level 2 (hashed, after 4096 + 32768): p = x * 63 + 0.5 = (20.03, 39.56, 11.21):
    # (20 ^ (39 * 2654435761 mod 2^32) ^ (11 * 805459861 mod 2^32)) mod 65536.
    rows, weights = sky.grid_rows_and_weights(torch.tensor([[0.31, 0.62, 0.17]], dtype=torch.float64))
    assert rows[0, 0, 0] == 917 and rows[0, 0, 7] == 1190 and rows[0, 1, 0] == 5738 + 4096
    hashed = (20 ^ (39 * 2654435761 % U32) ^ (11 * 805459861 % U32)) % 65536
    assert rows[0, 2, 0] == hashed + 4096 + 32768
    assert abs(float(weights[0, 0, 0]) - 0.85 * 0.2 * 0.95) < 1e-12 and abs(float(weights.sum(-1)[0, 5]) - 1.0) < 1e-12


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_saturating_cell_conversion(dtype):
    """In float64 and in float32, the dtype the model and the yardstick run in (2^32 - 1 is no float32 number: a limit applied to the
    float would let 2^32 through, which the uint32 mask turns into 0)."""
    x = torch.tensor([[-0.7, 1e3, float("nan")], [3e8, 0.0, -1e-9], [8192.5, 2e4, 4e9]], dtype=dtype)
    rows, weights = sky.grid_rows_and_weights(x)
    assert int(rows.min()) >= 0 and int(rows.max()) < sky.GRID_ROWS
    levels, _ = np_levels()
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    saturated = 0
    for n in range(3):
        for l in (0, 1, 2, 14, 15):
            # p in the arithmetic of `dtype`, as the contract's p = x * scale + 0.5
            p = [float(np_dtype(np_dtype(np_dtype(float(x[n, d])) * np_dtype(levels[l][0])) + np_dtype(0.5))) for d in range(3)]
            cell = [np_saturate(math.floor(v) if math.isfinite(v) else v) for v in p]
            saturated += sum(c == U32 - 1 for c in cell)
            for corner in (0, 1, 5, 7):
                want = np_row(levels[l], [(cell[d] + ((corner >> d) & 1)) % U32 for d in range(3)])
                assert int(rows[n, l, corner]) == want, (dtype, n, l, corner)
    assert saturated >= 4                                # 3e8 and 4e9 times the finest scales are beyond 2^32
    assert torch.isnan(weights[0]).all() and not torch.isnan(weights[1]).any()
    assert np_saturate(3e8 * (16 * 2 ** 15 - 1) + 0.5) == U32 - 1 and np_saturate(float(2 ** 32)) == U32 - 1


def test_vertex_position_has_one_corner_of_weight_one():
    for dtype in (torch.float32, torch.float64):
        _, weights = sky.grid_rows_and_weights(torch.tensor([sc.VERTEX], dtype=dtype))
        assert weights.shape == (1, 16, 8) and bool((weights[0, :, 0] == 1).all()) and bool((weights[0, :, 1:] == 0).all())


def test_position_cases_through_position_features():
    params = sc.make_state(1, grid_scale=1e4)["params"].double()
    for pos in ([0.31, 0.62, 0.17], sc.VERTEX, [-0.7, -2.5, -0.01], [1e3, -1e3, 1e3]):
        got = sky.position_features(params, torch.tensor(pos, dtype=torch.float64)).numpy()
        want = np.concatenate([np_grid(params.numpy(), np.array(pos)), np_embed(np.array(pos))])
        assert got.shape == (95,) and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), pos
    got = sky.position_features(params, torch.tensor([0.3, float("nan"), 0.2], dtype=torch.float64))
    assert torch.isnan(got[:32]).all()           # cell 0 on the NaN axis, NaN weights, every index in range (no exception above)


def test_grid_gradient_touches_at_most_256_parameters():
    params = sc.make_state(0)["params"].clone().requires_grad_()
    sky.position_features(params, torch.tensor([0.31, 0.62, 0.17])).sum().backward()
    assert 0 < int((params.grad != 0).sum()) <= 256


# ---- the twin against the independent restatement, and the bar -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shape_5x7_wg0", "fx_ne_fy", "principal_point_outside", "c2w_not_a_rotation", "position_negative", "position_1e3",
                                  "one_huge_bias", "weights_zero"])
def test_twin_matches_numpy_restatement(name):
    case = _case(name)
    if case["H"] * case["W"] > 35:
        case = dict(case, H=3, W=4)
    params, layers = sc.layers_of(case["state"], torch.float64, "cpu")
    got = sky.sky_forward_torch(params, layers, case["H"], case["W"], case["K"], case["c2w"]).numpy()
    assert np.abs(got - np_image(case)).max() <= 1e-12


def test_weights_zero_gives_sigmoid_of_b3():
    truth, _ = sc.reference(_case("weights_zero"))
    want = 1.0 / (1.0 + np.exp(-np.array([0.3, -1.2, 2.0], dtype=np.float32).astype(np.float64)))
    assert np.abs(truth["image"] - want[:, None, None]).max() < 1e-15


def test_references_are_usable_on_every_case():
    """What the references themselves must satisfy before a kernel is held to them.  (That the yardstick passes its own bar is true by
    the bar's construction and shows nothing; this checks what is not.)  The truth and the yardstick are finite wherever no NaN was put
    in, NaN in the same places where one was; every tensor has a non-zero truth unless the case is built to zero it (a bar relative to
    a zero scale would hold nothing).  How large the yardstick's own deviation is, is not bounded here: it is the reference's error, and
    in the cases whose grid values are of order 1 it reaches percents (at the finest level p = x * 524287 + 0.5 is about 3e5, where
    float32 numbers are 1/32 apart); test_bar_rejects_wrong_models shows the bar still rejects wrong models in such a case.  The two
    263x251 cases are left to the GPU tests, which compute their references anyway (seconds each)."""
    zero_by_design = {"weights_zero": {"g_params", "g_w0", "g_b0", "g_w1", "g_b1", "g_w2", "g_b2", "g_w3"},
                      "first_layer_dead": {"g_params", "g_w0", "g_b0", "g_w1", "g_w2"}, "weights_x50": set(sc.MODEL_GRADS)}
    for case in sc.CASES:
        if case["H"] * case["W"] > 67 * 129:
            continue
        truth, yard = sc.reference(case)
        for key, t in truth.items():
            y = yard[key]
            if case["name"] == "nan_in_c2w":
                assert np.array_equal(np.isnan(t), np.isnan(y)) and np.isnan(truth["image"]).all(), (case["name"], key)
                continue
            assert np.isfinite(t).all() and np.isfinite(y).all(), (case["name"], key)
            scale = np.abs(t).max()
            if key in zero_by_design.get(case["name"], ()) or (key == "g_params" and scale == 0):
                continue
            assert scale > 0, (case["name"], key)


@pytest.mark.parametrize("wrong", [dict(flip=True), dict(normalise=True), dict(plus_half=False), dict(sin_first=False), dict(relu_last=True)])
def test_bar_rejects_wrong_models(wrong):
    case = dict(_case("position_inside"), H=3, W=4)
    params, layers = sc.layers_of(case["state"], torch.float64, "cpu")
    truth = {"image": sky.sky_forward_torch(params, layers, 3, 4, case["K"], case["c2w"]).numpy()}
    params, layers = sc.layers_of(case["state"], torch.float32, "cpu")
    yard = {"image": sky.sky_forward_torch(params, layers, 3, 4, case["K"], case["c2w"]).double().numpy()}
    right = {"image": np_image(case).astype(np.float32)}
    assert sc.ratios(right, truth, yard)["image"] <= 1.0
    assert sc.ratios({"image": np_image(case, **wrong).astype(np.float32)}, truth, yard)["image"] > 10.0, wrong


# ---- the module's surface --------------------------------------------------------------------------------------------------------------
def test_state_dict_names_shapes_and_round_trip(tmp_path):
    model = sky.SkyModel(device="cpu")
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {"position_encoding.params": (1908736,)}
    for k, (o, i) in enumerate([(64, 111), (64, 64), (64, 64), (3, 64)]):
        want[f"blocks.layers.{k}.weight"], want[f"blocks.layers.{k}.bias"] = (o, i), (o,)
    assert shapes == want
    assert float(model.position_encoding.params.detach().abs().max()) <= 1e-4
    assert isinstance(model.optimizer, torch.optim.Adam) and model.optimizer.defaults["lr"] == 1e-4
    path = str(tmp_path / "sky_params.pt")
    model.save(path)
    other = sky.SkyModel(device="cpu")
    other.load(path)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), other.state_dict().values()))
    v, pos = torch.randn(2, 3, 3), torch.rand(2, 3, 3)
    assert model(v, pos).shape == (2, 3, 3)


def test_other_configurations_are_refused_by_name():
    for kwargs, name in ((dict(W=128), "W"), (dict(num_levels=8), "num_levels"), (dict(dir_embed_cfg={"degree": 3}), "dir_embed_cfg"),
                         (dict(weight_norm=True), "weight_norm")):
        with pytest.raises(ValueError, match=name):
            sky.SkyModel(device="cpu", **kwargs)


def test_fused_op_refuses_cpu_tensors():
    case = _case("shape_5x7_wg0")
    cam, weights = sc.fused_inputs(case, "cpu")
    with pytest.raises(_lib.SurfelRasterError, match="no CPU path"):
        sky.sky_rays_mlp(cam, 5, 7, *weights)


def test_exports():
    import streetunveiler_amd
    for name in ("SkyModel", "sky_rays_mlp", "sky_forward_torch", "position_features"):
        assert getattr(streetunveiler_amd, name) is getattr(sky, name) and name in streetunveiler_amd.__all__


# ---- the C-ABI without a GPU -----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_refuse_bad_arguments():
    build()
    lib = _lib.load()
    assert lib.sr_abi_version() == 10
    for name in ("sr_sky_workspace_bytes", "sr_sky_forward", "sr_sky_backward"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.sr_sky_workspace_bytes(3) >= 3 * 9603 * 8 and lib.sr_sky_workspace_bytes(0) >= lib.sr_sky_workspace_bytes(3)
    assert lib.sr_sky_workspace_bytes(1) < lib.sr_sky_workspace_bytes(2)
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    nine, eight = [p] * 9, [p] * 8
    assert lib.sr_sky_forward(-1, 4, p, *nine[1:], 0, p, None) == -1 and b"image size" in lib.sr_last_error()
    assert lib.sr_sky_forward(4, 4, None, *nine[1:], 0, p, None) == -1 and b"NULL" in lib.sr_last_error()
    assert lib.sr_sky_forward(4, 4, p, *nine[1:], -1, p, None) == -1 and b"max_workgroups" in lib.sr_last_error()
    assert lib.sr_sky_forward(4, 4, p, *nine[1:], 0, None, None) == -1 and b"out is NULL" in lib.sr_last_error()
    assert lib.sr_sky_forward(0, 4, p, *nine[1:], 0, None, None) == 0                       # H * W == 0: no error, no work
    assert lib.sr_sky_backward(4, -4, p, *nine[1:], p, 0, p, 1 << 40, *eight, None) == -1 and b"image size" in lib.sr_last_error()
    assert lib.sr_sky_backward(4, 4, p, *nine[1:], None, 0, p, 1 << 40, *eight, None) == -1 and b"g_out" in lib.sr_last_error()
    assert lib.sr_sky_backward(4, 4, p, *nine[1:], p, 0, None, 0, *eight, None) == -1 and b"workspace" in lib.sr_last_error()
    assert lib.sr_sky_backward(4, 4, p, *nine[1:], p, 2, p, 2 * 9603 * 8 - 1, *eight, None) == -3
    assert lib.sr_sky_backward(4, 4, p, *nine[1:], p, 0, None, 0, *([None] * 8), None) == 0   # nothing wanted: no work
    assert lib.sr_sky_backward(4, 0, p, *nine[1:], None, 0, None, 0, *eight, None) == 0

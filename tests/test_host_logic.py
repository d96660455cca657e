"""CPU: host-side logic around the operator -- SH python fallback, allmap post-processing, frame-sharded DP (gloo)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.postprocess_torch import postprocess_allmap
from streetunveiler_amd.sh import RGB2SH, SH2RGB, eval_sh
from streetunveiler_amd.synthetic import synthetic_camera


def test_python_sh_fallback_matches_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, "sh_golden.npz"))
    sh, dirs = torch.tensor(z["sh"]), torch.tensor(z["dirs"])
    for deg in range(4):
        np.testing.assert_allclose(eval_sh(deg, sh, dirs).numpy(), z[f"rgb_deg{deg}"], atol=1e-6)
    z4 = np.load(os.path.join(golden_dir, "sh4_golden.npz"))   # degree 4: 25 coefficients, reached by the reference's python function only
    np.testing.assert_allclose(eval_sh(4, torch.tensor(z4["sh"]), torch.tensor(z4["dirs"])).numpy(), z4["rgb_deg4"], atol=2e-6)
    rgb = torch.tensor(z["rgb2sh_in"])
    np.testing.assert_allclose(RGB2SH(rgb).numpy(), z["rgb2sh_out"], atol=1e-6)
    np.testing.assert_allclose(SH2RGB(RGB2SH(rgb)).numpy(), z["sh2rgb_out"], atol=1e-6)


def test_postprocess_allmap_against_direct_numpy():
    """oracle.postprocess_torch restates gaussian_renderer/__init__.py:148-186 + utils/point_utils.py:9-37
    (the checker of the fused HIP post-processing); here it is checked against an independent numpy transcription."""
    W, H = 40, 24
    cam = synthetic_camera(W, H, index=2)
    g = torch.Generator().manual_seed(0)
    allmap = torch.rand(7, H, W, generator=g)
    allmap[1, :3] = 0.0              # alpha == 0 rows -> 0/0 -> nan_to_num -> 0
    allmap[0] = allmap[0] * 10 + 1
    for ratio in (0.0, 1.0, 0.3):
        out = postprocess_allmap(cam, ratio, allmap.clone())
        a = allmap.numpy().astype(np.float64)
        alpha = a[1:2]
        with np.errstate(divide="ignore", invalid="ignore"):
            exp = np.nan_to_num(a[0:1] / alpha, nan=0.0, posinf=0.0, neginf=0.0)
        surf = exp * (1 - ratio) + ratio * a[5:6]
        np.testing.assert_allclose(out["surf_depth"].numpy(), surf, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(out["rend_alpha"].numpy(), alpha)
        R = cam.world_view_transform.numpy()[:3, :3].astype(np.float64)
        np.testing.assert_allclose(out["rend_normal"].numpy(), np.einsum("chw,dc->dhw", a[2:5], R), atol=1e-5)
        # pseudo-normals: back-project, central differences, normalise, zero border, times alpha
        fx = W / (2 * math.tan(cam.FoVx / 2)); fy = H / (2 * math.tan(cam.FoVy / 2))
        K = np.array([[fx, 0, W / 2], [0, fy, H / 2], [0, 0, 1]])
        c2w = np.linalg.inv(cam.world_view_transform.numpy().T.astype(np.float64))
        xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
        pix = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3).astype(np.float64)
        pts = (surf.reshape(-1, 1) * (pix @ np.linalg.inv(K).T @ c2w[:3, :3].T) + c2w[:3, 3]).reshape(H, W, 3)
        n = np.zeros_like(pts)
        dx = pts[2:, 1:-1] - pts[:-2, 1:-1]; dy = pts[1:-1, 2:] - pts[1:-1, :-2]
        cr = np.cross(dx, dy); n[1:-1, 1:-1] = cr / np.maximum(np.linalg.norm(cr, axis=-1, keepdims=True), 1e-12)
        np.testing.assert_allclose(out["surf_point"].numpy(), pts.transpose(2, 0, 1), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(out["surf_normal"].numpy(), n.transpose(2, 0, 1) * alpha, atol=2e-3)
        assert set(out) == {"rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal", "surf_point"}


def _dp_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from streetunveiler_amd.parallel import allreduce_gradients, frames_for_rank, init_distributed, reduce_densification_stats
    r, w, _ = init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    P = 1000
    g = torch.Generator().manual_seed(100 + rank)
    grads = [torch.randn(P, 3, generator=g), torch.randn(P, 16, 3, generator=g), torch.randn(P, 1, generator=g),
             torch.randn(P, 2, generator=g), torch.randn(P, 4, generator=g), None]
    local = [x.clone() if x is not None else None for x in grads]
    import streetunveiler_amd.parallel as par
    par._BUCKET_INPLACE_BYTES = 100_000   # exercise both the bucketed and the in-place path
    allreduce_gradients(grads)
    # gradients carved out of one flat buffer (what the rasterizer's backward returns) take the single-collective path
    flat = torch.randn(P * 10, generator=g)
    fviews = [flat[:P * 3].view(P, 3), flat[P * 3:P * 9].view(P, 2, 3), flat[P * 9:].view(P, 1)]
    flocal = flat.clone()
    allreduce_gradients(fviews + [None])
    # densification statistics of this rank's view
    vs_grad = torch.randn(P, 3, generator=g); radii = torch.randint(0, 5, (P,), generator=g, dtype=torch.int32)
    accum, denom, maxr = torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P)
    reduce_densification_stats(vs_grad, radii, accum, denom, maxr)
    torch.save(dict(local=local, reduced=grads, flocal=flocal, freduced=flat, vs_grad=vs_grad, radii=radii, accum=accum, denom=denom, maxr=maxr,
                    frames=frames_for_rank(8, rank, world)), os.path.join(tmp, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_frame_sharded_dp_gloo_world2(tmp_path):
    """all-reduced gradient == sum of the per-rank gradients; densification stats SUM/SUM/MAX."""
    world, port = 2, 29500 + (os.getpid() % 2000)
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    rs = [torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(world)]
    for k in range(5):
        expect = rs[0]["local"][k] + rs[1]["local"][k]
        for r in rs:
            torch.testing.assert_close(r["reduced"][k], expect, rtol=1e-6, atol=1e-6)
    for r in rs:
        torch.testing.assert_close(r["freduced"], rs[0]["flocal"] + rs[1]["flocal"], rtol=1e-6, atol=1e-6)
    acc = sum(torch.where((r["radii"] > 0)[:, None], r["vs_grad"].norm(dim=-1, keepdim=True), torch.zeros(1)) for r in rs)
    den = sum((r["radii"] > 0).float()[:, None] for r in rs)
    mx = torch.maximum(*[torch.where(r["radii"] > 0, r["radii"].float(), torch.zeros(1)) for r in rs])
    for r in rs:
        torch.testing.assert_close(r["accum"], acc); torch.testing.assert_close(r["denom"], den); torch.testing.assert_close(r["maxr"], mx)
    assert rs[0]["frames"] == [0, 2, 4, 6] and rs[1]["frames"] == [1, 3, 5, 7]


def _sh_adjoint_torch(means3D, cams, gathered, sh_coeffs, degree):
    """Test-side stand-in for the HIP expand kernel: autograd of the python SH evaluation (linear in sh)."""
    P = means3D.shape[0]
    sh = torch.zeros(P, sh_coeffs, 3, dtype=torch.float64, requires_grad=True)
    total = 0.0
    for v in range(cams.shape[0]):
        d = means3D.double() - cams[v].double()
        d = d / d.norm(dim=1, keepdim=True)
        total = total + (eval_sh(degree, sh.transpose(1, 2), d) * gathered[v].double()).sum()
    return torch.autograd.grad(total, sh)[0].float()


def _sh_exchange_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from streetunveiler_amd.parallel import active_sh_exchange, factored_sh_exchange, init_distributed
    init_distributed(backend="gloo")
    P = 500
    means3D = torch.randn(P, 3, generator=torch.Generator().manual_seed(7)) * 3      # same Gaussians on every rank
    g = torch.Generator().manual_seed(200 + rank)
    gc = torch.randn(P, 3, generator=g)
    gc[torch.rand(P, generator=g) < 0.3] = 0.0                                       # invisible in this rank's frame
    cam_of = lambda r: torch.randn(3, generator=torch.Generator().manual_seed(400 + r)) * 10
    campos = cam_of(rank)
    assert active_sh_exchange() is None
    with factored_sh_exchange(expand=_sh_adjoint_torch) as ex:
        assert active_sh_exchange() is ex
        summed = ex.run(gc, means3D, campos, 16, 3)
    with factored_sh_exchange(expand=_sh_adjoint_torch, all_campos=torch.stack([cam_of(r) for r in range(world)])) as ex2:
        ex2.run(gc, means3D, campos, 16, 2)
        assert ex2.calls == 1 and ex2.bytes_sent == P * 12
    assert active_sh_exchange() is None
    torch.save(dict(gc=gc, campos=campos, means3D=means3D, summed=summed), os.path.join(tmp, f"s{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_factored_sh_exchange_gloo_world2(tmp_path):
    """all-gather of 12-B colour gradients + local expansion == sum of the per-rank dL_dsh."""
    world, port = 2, 31500 + (os.getpid() % 2000)
    mp.spawn(_sh_exchange_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    rs = [torch.load(os.path.join(tmp_path, f"s{r}.pt")) for r in range(world)]
    expect = sum(_sh_adjoint_torch(r["means3D"], r["campos"][None], r["gc"][None], 16, 3) for r in rs)
    assert expect.abs().max() > 0.1
    for r in rs:
        torch.testing.assert_close(r["summed"], expect, rtol=1e-5, atol=1e-6)


def _accum_worker(rank, world, port, tmp, K):
    """Gradient accumulation: K frames per rank attach to ONE exchange; world 4 also checks the view <-> camera pairing for N > 2."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from streetunveiler_amd.parallel import active_sh_exchange, factored_sh_exchange, init_distributed
    init_distributed(backend="gloo")
    P = 300
    means3D = torch.randn(P, 3, generator=torch.Generator().manual_seed(7)) * 3      # same Gaussians on every rank
    cam_of = lambda r, j: torch.randn(3, generator=torch.Generator().manual_seed(1000 + 10 * r + j)) * 10
    g = torch.Generator().manual_seed(300 + rank)
    gcs = [torch.randn(P, 3, generator=g) for _ in range(K)]
    results = {}
    for known in (False, True):    # camera positions all-gathered by the exchange / known to every rank as [world, K, 3]
        all_campos = torch.stack([torch.stack([cam_of(r, j) for j in range(K)]) for r in range(world)]) if known else None
        rest = torch.full((P * 10,), float(rank + 1))          # the other gradients, accumulated locally over the K frames
        with factored_sh_exchange(expand=_sh_adjoint_torch, all_campos=all_campos, frames_per_rank=K) as ex:
            assert active_sh_exchange() is ex
            outs = [ex.run(gcs[j], means3D, cam_of(rank, j), 16, 3) for j in range(K)]
        assert all(o is None for o in outs[:-1]) and outs[-1] is not None and ex.calls == 1
        ex.finish([rest[:P * 3].view(P, 3), rest[P * 3:].view(P, 7)])
        assert ex.bytes_sent == K * P * 12 + P * 40
        results[known] = (outs[-1], rest)
    # ONE loss summed over the K frames: autograd runs the K backward nodes in REVERSE creation order.  The forward draws the frame
    # number (`attach`), the backward files its gradient under it -- the pairing with all_campos[r, j] must not depend on the order.
    all_campos = torch.stack([torch.stack([cam_of(r, j) for j in range(K)]) for r in range(world)])
    with factored_sh_exchange(expand=_sh_adjoint_torch, all_campos=all_campos, frames_per_rank=K) as ex:
        frames = [ex.attach() for _ in range(K)]
        assert frames == list(range(K))
        outs = [ex.run(gcs[j], means3D, cam_of(rank, j), 16, 3, frame=j) for j in reversed(frames)]
    assert all(o is None for o in outs[:-1]) and outs[-1] is not None
    with pytest.raises(RuntimeError, match="all_campos"):    # a camera list that does not match the frames' cameras is refused
        with factored_sh_exchange(expand=_sh_adjoint_torch, all_campos=all_campos + 1.0, frames_per_rank=K) as ex:
            for j in [ex.attach() for _ in range(K)]:
                ex.run(gcs[j], means3D, cam_of(rank, j), 16, 3, frame=j)
    # densification statistics: ONE all-gather up to three ranks, a SUM + MAX all-reduce pair from four ranks on (world 4 runs here)
    from streetunveiler_amd.parallel import reduce_densification_stats
    view = lambda r: (torch.randn(P, 3, generator=torch.Generator().manual_seed(900 + r)),
                      torch.randint(0, 5, (P,), generator=torch.Generator().manual_seed(950 + r), dtype=torch.int32))
    accum, denom, maxr = torch.ones(P, 1), torch.ones(P, 1), torch.full((P,), 2.0)
    reduce_densification_stats(*view(rank), accum, denom, maxr)
    e_acc = 1 + sum(torch.where((view(r)[1] > 0)[:, None], view(r)[0].norm(dim=-1, keepdim=True), torch.zeros(1)) for r in range(world))
    e_den = 1 + sum((view(r)[1] > 0).float()[:, None] for r in range(world))
    e_max = torch.stack([torch.full((P,), 2.0)] + [view(r)[1].float() for r in range(world)]).max(0).values
    torch.testing.assert_close(accum, e_acc); torch.testing.assert_close(denom, e_den); torch.testing.assert_close(maxr, e_max)
    torch.save(dict(gcs=gcs, cams=[cam_of(rank, j) for j in range(K)], means3D=means3D, free=results[False][0], known=results[True][0],
                    rest=results[True][1], reverse=outs[-1]), os.path.join(tmp, f"a{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,K", [(2, 3), (4, 1), (4, 2)])
def test_factored_exchange_accumulation_and_world4_ordering(tmp_path, world, K):
    """frames_per_rank = K: the first K - 1 backward calls return no SH gradient, the K-th returns the sum over all world * K views, each
    gradient paired with ITS camera (a wrong all-gather order for N > 2 would pair rank r's gradient with another rank's camera);
    finish() all-reduces the locally accumulated rest once."""
    port = 33500 + (os.getpid() % 2000) + 7 * world + K
    mp.spawn(_accum_worker, args=(world, port, str(tmp_path), K), nprocs=world, join=True)
    rs = [torch.load(os.path.join(tmp_path, f"a{r}.pt")) for r in range(world)]
    expect = sum(_sh_adjoint_torch(r["means3D"], r["cams"][j][None], r["gcs"][j][None], 16, 3) for r in rs for j in range(K))
    shuffled = sum(_sh_adjoint_torch(r["means3D"], rs[(i + 1) % world]["cams"][j][None], r["gcs"][j][None], 16, 3) for i, r in enumerate(rs) for j in range(K))
    assert (expect - shuffled).abs().max() > 1e-2          # the pairing matters: the check below would catch a permuted gather
    for r in rs:
        torch.testing.assert_close(r["free"], expect, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(r["known"], expect, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(r["reverse"], expect, rtol=1e-5, atol=1e-5)   # backward nodes in reverse creation order
        assert torch.equal(r["rest"], torch.full_like(r["rest"], float(sum(range(1, world + 1)))))


def test_exchange_rides_on_the_autograd_node_not_on_global_state():
    """factored_sh_exchange scopes a ContextVar on the calling thread; the operator's forward copies the exchange onto its autograd
    node, so a backward running later, outside the block and on another thread, still finds it -- and a thread that never entered
    the block sees none."""
    import threading
    import streetunveiler_amd.parallel as par
    seen = {}
    ex = par.ShExchange()
    token = par._ACTIVE_SH_EXCHANGE.set(ex)
    try:
        assert par.active_sh_exchange() is ex
        t = threading.Thread(target=lambda: seen.setdefault("other", par.active_sh_exchange()))
        t.start(); t.join()
    finally:
        par._ACTIVE_SH_EXCHANGE.reset(token)
    assert seen["other"] is None and par.active_sh_exchange() is None
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff_surfel_rasterization", "__init__.py")).read()
    fwd, bwd = src.split("def backward(ctx, grad_out_color", 1)
    assert "ctx.sh_exchange = active_sh_exchange()" in fwd and "active_sh_exchange" not in bwd.split("class _ClassDistortions")[0]


def test_ply_checkpoint_layout_and_round_trip(tmp_path):
    """Reference PLY layout [REF scene/gaussian_model.py:226-259, 338-382]: property names/order, channel-major SH
    features, int32 semantics; binary and ASCII, any property order."""
    from streetunveiler_amd.ply import attribute_names, load_ply, save_ply
    rng = np.random.default_rng(0)
    P = 37
    d = dict(xyz=rng.normal(size=(P, 3)), features_dc=rng.normal(size=(P, 1, 3)), features_rest=rng.normal(size=(P, 15, 3)),
             opacity=rng.normal(size=(P, 1)), scaling=rng.normal(size=(P, 2)), rotation=rng.normal(size=(P, 4)))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    sem = rng.integers(0, 6, size=(P, 1))
    path = os.path.join(tmp_path, "pc.ply")
    save_ply(path, d["xyz"], d["features_dc"], d["features_rest"], d["opacity"], d["scaling"], d["rotation"], sem)
    raw = open(path, "rb").read()
    names = attribute_names()
    assert names[:9] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] and names[9] == "f_rest_0" and names[53] == "f_rest_44"
    assert names[54:] == ["opacity", "scale_0", "scale_1", "rot_0", "rot_1", "rot_2", "rot_3"]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 37\n" + "".join(f"property float {n}\n" for n in names) + "property int semantics\nend_header\n"
    assert raw.startswith(header.encode()) and len(raw) == len(header) + P * (61 * 4 + 4)
    row0 = np.frombuffer(raw[len(header):len(header) + 62 * 4], "<f4")
    np.testing.assert_array_equal(row0[:3], d["xyz"][0]); np.testing.assert_array_equal(row0[3:6], 0)
    np.testing.assert_array_equal(row0[6:9], d["features_dc"][0, 0])                 # f_dc_c = channel c
    np.testing.assert_array_equal(row0[9:24], d["features_rest"][0, :, 0])            # f_rest_0..14 = channel 0, coefficients 1..15
    np.testing.assert_array_equal(row0[24:39], d["features_rest"][0, :, 1])
    back = load_ply(path)
    for k, v in d.items():
        np.testing.assert_array_equal(back[k], v)
    np.testing.assert_array_equal(back["semantics"], sem[:, 0])
    # ASCII, shuffled property order, an extra property: still loads by name
    order = list(rng.permutation(len(names)))
    cols = np.frombuffer(raw[len(header):], np.dtype([(n, "<f4") for n in names] + [("semantics", "<i4")]))
    with open(os.path.join(tmp_path, "a.ply"), "w") as fh:
        fh.write("ply\nformat ascii 1.0\ncomment shuffled\nelement vertex 37\nproperty int semantics\nproperty float extra\n")
        fh.write("".join(f"property float {names[k]}\n" for k in order) + "end_header\n")
        for r in cols:
            fh.write(" ".join([str(int(r["semantics"])), "1.5"] + [repr(float(r[names[k]])) for k in order]) + "\n")
    back2 = load_ply(os.path.join(tmp_path, "a.ply"))
    for k, v in d.items():
        np.testing.assert_array_equal(back2[k], v)
    with pytest.raises(ValueError):
        load_ply(path, max_sh_degree=2)


def test_fused_activations_only_for_models_with_plain_getters(tmp_path):
    """PipelineParams.fused_activations hands the RAW _opacity/_scaling/_rotation to the operator -- only valid when the model's
    getters are the plain activations.  A MaskGaussianModel-style model (getters activate `_x + _new_x * mask`
    [REF scene/mask_gaussian.py:140-176], `_x` frozen) must keep the getter path, or its trainable deltas would be dropped."""
    from streetunveiler_amd import gaussian_renderer as gr

    class MaskGaussianModel:   # same name and getter structure as the reference class
        def __init__(self, n):
            self._xyz = torch.zeros(n, 3)
            self._opacity, self._new_opacity = torch.zeros(n, 1), torch.full((n, 1), 0.7, requires_grad=True)
            self._scaling, self._new_scaling = torch.zeros(n, 2), torch.full((n, 2), -1.0, requires_grad=True)
            self._rotation, self._new_rotation = torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1), torch.full((n, 4), 0.3, requires_grad=True)
            self.mask = torch.ones(n)
        get_xyz = property(lambda s: s._xyz)
        get_opacity = property(lambda s: torch.sigmoid(s._opacity + s._new_opacity * s.mask[..., None]))
        get_scaling = property(lambda s: torch.exp(s._scaling + s._new_scaling * s.mask[..., None]))
        get_rotation = property(lambda s: torch.nn.functional.normalize(s._rotation + s._new_rotation * s.mask[..., None]))

    pipe = gr.PipelineParams(fused_activations=True)
    pc = MaskGaussianModel(5)
    assert not gr._fused_activations(pc, pipe)
    means3D, means2D, opacity, scales, rotations, cov = gr._geometry_inputs(pc, pipe, torch.zeros(5, 3), None, 1.0)
    assert torch.equal(opacity, pc.get_opacity) and torch.equal(scales, pc.get_scaling) and torch.equal(rotations, pc.get_rotation)
    opacity.sum().backward()
    assert pc._new_opacity.grad is not None and pc._new_opacity.grad.abs().sum() > 0    # the trainable delta receives the gradient

    class GaussianModel:       # the reference's plain model qualifies by name
        _opacity = _scaling = _rotation = torch.zeros(1)
    assert gr._fused_activations(GaussianModel(), pipe)
    raw = gr.SurfelModel(torch.zeros(2, 3), torch.zeros(2, 2), torch.ones(2, 4), torch.zeros(2, 1), torch.zeros(2, 16, 3), raw=True)
    act = gr.SurfelModel(torch.zeros(2, 3), torch.ones(2, 2), torch.ones(2, 4), torch.ones(2, 1), torch.zeros(2, 16, 3), raw=False)
    assert gr._fused_activations(raw, pipe) and not gr._fused_activations(act, pipe)
    assert not gr._fused_activations(raw, gr.PipelineParams(fused_activations=False))
    # a checkpoint's SH coefficients are ONE leaf: .grad exists after backward
    path = os.path.join(tmp_path, "pc.ply")
    g = torch.Generator().manual_seed(0)
    src = gr.SurfelModel(torch.randn(7, 3, generator=g), torch.randn(7, 2, generator=g), torch.randn(7, 4, generator=g),
                         torch.randn(7, 1, generator=g), torch.randn(7, 16, 3, generator=g), torch.arange(7, dtype=torch.int32), raw=True)
    src.save_ply(path)
    pc2 = gr.SurfelModel.from_ply(path, device="cpu")
    assert pc2._features.is_leaf and pc2._features.requires_grad and torch.equal(pc2._features.detach(), src._features)
    pc2.get_features.square().sum().backward()
    assert pc2._features.grad is not None


def test_bench_self_launches_its_ranks_without_a_launcher():
    """`python bench.py --gpus 2` outside torchrun must start two ranks itself (round-3 review: it died on an assert).  No GPU here: both
    workers get as far as `bench.py needs a GPU` -- i.e. past the launcher, the rendezvous-free start-up and the world-size check."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    env["SURFEL_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--gaussians", "1000",
                        "--no-cpu-baseline"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr[-2000:]
        return
    assert r.returncode != 0
    assert "without a torchrun environment: launching" in r.stderr
    assert r.stderr.count("bench.py needs a GPU") >= 2, r.stderr[-3000:]
    # a launcher environment that disagrees with --gpus is refused with a message, not an assert
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--steps", "1"], cwd=root,
                       env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gpus 4 but the launcher's WORLD_SIZE is 1" in r.stderr


def test_checkpoint_layout_and_activations_match_reference_gaussian_model(tmp_path, golden_dir):
    """G8: the reference's OWN GaussianModel (construct_list_of_attributes, save_ply, load_ply, the activation getters
    [REF scene/gaussian_model.py:31-39, 101-123, 226-259, 338-382]) was run on seeded raw parameters by tests/golden/make_golden.py
    with a capturing stand-in for plyfile; what it handed to PlyElement.describe and what its load_ply built are the fixture.
    ply.py must write those very bytes and read those very tensors; SurfelModel's getters must equal the reference's."""
    from streetunveiler_amd import gaussian_renderer as gr
    from streetunveiler_amd.ply import attribute_names, load_ply, save_ply
    z = np.load(os.path.join(golden_dir, "rotation_checkpoint_golden.npz"))
    raw = {k: z["g8_raw_" + k] for k in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")}
    P = raw["xyz"].shape[0]
    names = [str(n) for n in z["g8_attribute_names"]]
    assert attribute_names() == names
    assert [str(n) for n in z["g8_element_names"]] == names + ["semantics"]
    assert [str(f) for f in z["g8_element_formats"]] == ["<f4"] * len(names) + ["<i4"]
    path = os.path.join(tmp_path, "pc.ply")
    save_ply(path, raw["xyz"], raw["features_dc"], raw["features_rest"], raw["opacity"], raw["scaling"], raw["rotation"], z["g8_semantics"])
    body = open(path, "rb").read().split(b"end_header\n", 1)[1]
    assert body == z["g8_element_bytes"].tobytes(), "the vertex rows differ from what the reference hands to plyfile"
    assert len(body) == P * (len(names) * 4 + 4)
    back = load_ply(path)
    for k in raw:
        np.testing.assert_array_equal(back[k], z["g8_loaded_" + k]), k
        np.testing.assert_array_equal(back[k], raw[k])
    np.testing.assert_array_equal(back["semantics"], z["g8_loaded_semantics"][:, 0])
    assert int(z["g8_loaded_active_sh_degree"]) == 3
    # the activations: exp / sigmoid / normalize (eps 1e-12: row 0 is a quaternion of norm 1e-20) == SR_ACT_* of the C-ABI
    pc = gr.SurfelModel.from_ply(path, device="cpu")
    np.testing.assert_array_equal(pc.get_scaling.detach().numpy(), z["g8_get_scaling"])
    np.testing.assert_array_equal(pc.get_opacity.detach().numpy(), z["g8_get_opacity"])
    np.testing.assert_array_equal(pc.get_rotation.detach().numpy(), z["g8_get_rotation"])
    np.testing.assert_array_equal(pc.get_features.detach().numpy(), z["g8_get_features"])
    np.testing.assert_array_equal(pc.get_semantics_32bit.numpy().reshape(-1), z["g8_get_semantics_32bit"].reshape(-1))
    assert np.abs(z["g8_get_rotation"][0]).max() < 1e-6     # |q| = 1e-20 < eps: normalize() divides by eps, not by the norm


def test_densification_statistics_match_reference_gaussian_model(golden_dir):
    """G9: the reference's own `GaussianModel.add_densification_stats` [REF scene/gaussian_model.py:555-557] and train.py:168's
    max_radii2D update, run on two seeded views by tests/golden/make_golden.py.  `reduce_densification_stats` (one process: no
    exchange) must leave the same three arrays after every view -- the per-view semantics the multi-rank exchange then sums / maximises."""
    from streetunveiler_amd.parallel import reduce_densification_stats
    z = np.load(os.path.join(golden_dir, "rotation_checkpoint_golden.npz"))
    P = z["g9_view0_radii"].shape[0]
    accum, denom, maxr = torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P)
    for v in range(2):
        reduce_densification_stats(torch.tensor(z[f"g9_view{v}_grad"]), torch.tensor(z[f"g9_view{v}_radii"]), accum, denom, maxr)
        np.testing.assert_array_equal(accum.numpy(), z[f"g9_after{v}_accum"])
        np.testing.assert_array_equal(denom.numpy(), z[f"g9_after{v}_denom"])
        np.testing.assert_array_equal(maxr.numpy(), z[f"g9_after{v}_max_radii2D"])
    assert denom.max() == 2 and (denom == 0).any()


def test_bench_measurement_helpers(tmp_path, monkeypatch):
    """The parts of bench.py a first real multi-GPU run leans on, exercised without a GPU: RCCL's INIT log -> channel count (a single-channel
    ring must be recognisable), the predicted xGMI wire times, the exchange report, and the rule that a counter profile of OTHER kernel
    sources is not quoted."""
    import argparse, importlib, json, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    # --- RCCL log parsing (lines as RCCL 2.26 writes them with NCCL_DEBUG=INFO, NCCL_DEBUG_SUBSYS=INIT,GRAPH) ---
    log = tmp_path / "rccl.log"
    log.write_text("host:1:2 [0] NCCL INFO RCCL version : 2.26.6-HEAD:64f48b6\n"
                   "host:1:2 [0] NCCL INFO comm 0x1 rank 0 nranks 8 cudaDev 0 busId 1000 - Init START\n"
                   + "".join(f"host:1:2 [0] NCCL INFO Channel {c:02d}/32 : 0 1 2 3 4 5 6 7\n" for c in range(32))
                   + "host:1:2 [0] NCCL INFO Ring 00 : 7 -> 0 -> 1\nhost:1:2 [0] NCCL INFO 32 coll channels, 32 collnet channels\n")
    info = bench.rccl_topology(str(log), "nccl", 8)
    assert info["channels"] == 32 and info["coll_channels"] == 32 and info["nranks_in_log"] == 8 and info["version"].startswith("RCCL version")
    log.write_text("host:1:2 [0] NCCL INFO Channel 00/01 : 0 1\n")
    assert bench.rccl_topology(str(log), "nccl", 2)["channels"] == 1            # what bench.py flags in its JSON line (and refuses with SURFEL_REQUIRE_MULTI_CHANNEL=1)
    assert bench.rccl_topology(str(log), "gloo", 2)["channels"] is None          # nothing to read for another backend
    assert bench.rccl_topology(str(tmp_path / "missing.log"), "nccl", 2)["channels"] is None
    # --- predicted wire time: C3, 8 ranks, factored exchange ---
    P = 3_000_000
    px = bench.predicted_xgmi(P, 8, "factored")
    ag, ar = P * 12 * 8 * 7 / 8, P * 40 * 2 * 7 / 8
    assert abs(px["ring"]["all_gather_ms"] - ag / 76.8e9 * 1e3) < 2e-3 and abs(px["ring"]["all_reduce_ms"] - ar / 76.8e9 * 1e3) < 2e-3
    assert abs(px["direct_all_links"]["all_gather_ms"] * 7 - px["ring"]["all_gather_ms"]) < 1e-2
    assert bench.predicted_xgmi(P, 1, "factored")["all_gather_ms"] == 0.0
    assert bench.predicted_xgmi(P, 2, "allreduce")["ring"]["all_gather_ms"] == 0.0
    # --- exchange report: exposed vs alone ---
    detail = {"per_rank_ms_per_step": [4.0, 4.2], "exposed_ms_per_step_per_rank": [0.5, 0.7],
              "isolated_collectives": {"all_gather_colour_gradients": {"ms": 0.4}, "all_reduce_rest": {"ms": 1.0}}}
    rep = bench.exchange_report(detail, P, 2, 2, 4.2, "factored")
    assert rep["collectives_alone_ms_per_step"] == pytest.approx(0.4 * 2 + 1.0) and rep["exposed_ms_per_step_max_over_ranks"] == 0.7
    assert rep["hidden_fraction_of_the_collectives"] == pytest.approx(1 - 0.7 / 1.8, abs=1e-4) and rep["exposed_fraction_of_the_step"] == pytest.approx(0.7 / 4.2, abs=1e-4)
    assert bench.exchange_report(None, P, 2, 1, 4.0, "factored") is None
    # --- a profile is quoted only while its source digest is the current one ---
    from streetunveiler_amd.build import source_digest
    prof = tmp_path / "profiles"; prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    args = argparse.Namespace(tag="c3", sh_degree=3)
    kernels = {"sr::render_backward_kernel": {"traffic_bytes_per_launch": 123}}
    json.dump({"round": "r99", "head": "abc", "source_digest": source_digest(), "kernels": kernels}, open(prof / "r99_c3_hbm_traffic.json", "w"))
    t, src = bench.pmc_traffic("render_backward_kernel", args)
    assert t == 123 and src["round"] == "r99" and "stale" not in src
    json.dump({"round": "r99", "head": "abc", "source_digest": "0" * 16, "kernels": kernels}, open(prof / "r99_c3_hbm_traffic.json", "w"))
    t, src = bench.pmc_traffic("render_backward_kernel", args)
    assert t is None and "stale" in src and "re-run tools/profile_round.sh" in src["stale"]
    assert bench.pmc_traffic("render_backward_kernel", argparse.Namespace(tag="custom", sh_degree=3)) == (None, None)


def test_bench_dump_outputs_samples(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 files, maps cut to a seeded pixel sample and per-Gaussian arrays to a seeded row sample that are
    the same in every run, small arrays whole, and no more than DUMP_MAX_BYTES written."""
    import importlib, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    P, W, H = 70_000, 640, 480
    g = torch.Generator().manual_seed(3)
    maps = {"color": torch.randn(3, H, W, generator=g)}
    rows = {"radii": torch.randint(0, 40, (P,), generator=g, dtype=torch.int32), "grad_shs": torch.randn(P, 16, 3, generator=g)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), W * H, P, maps, rows, whole={"loss": torch.tensor(1.5, dtype=torch.float64)})
    pix, row = bench._dump_index(W * H, bench.DUMP_PIXELS, seed=0), bench._dump_index(P, bench.DUMP_ROWS, seed=1)
    assert len(set(pix.tolist())) == bench.DUMP_PIXELS and len(set(row.tolist())) == bench.DUMP_ROWS
    for run in ("a", "b"):
        got = {n: np.load(tmp_path / run / (n + ".npy")) for n in ("color", "radii", "grad_shs", "loss")}
        assert all(a.dtype == np.float32 for a in got.values())
        np.testing.assert_array_equal(got["color"], maps["color"].reshape(3, -1)[:, pix].numpy())
        np.testing.assert_array_equal(got["radii"], rows["radii"][row].float().numpy())
        np.testing.assert_array_equal(got["grad_shs"], rows["grad_shs"][row].numpy())
        assert got["loss"].tolist() == [1.5]
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)
    with pytest.raises(SystemExit, match="--dump-outputs would write"):
        bench.dump_outputs(str(tmp_path / "c"), W * H, P, maps, rows)
    assert not (tmp_path / "c").exists()


def test_posed_scene_and_rig_are_what_they_say():
    """The general-position scenes the parity tests rely on (streetunveiler_amd.synthetic.posed_scene / posed_rig): the camera has its own
    centre, a proper rotation and unrelated FoVs; the Gaussians sit in front of it in ITS frame with the benchmark scene's statistics;
    `behind_fraction` / `near_third` put exactly those Gaussians behind it / around the near plane; a rig's cameras share the Gaussians,
    not the centre."""
    import math
    from streetunveiler_amd.synthetic import posed_rig, posed_scene
    P, W, H = 4000, 320, 200
    cam, g = posed_scene(P, W, H, seed=11, spread=20.0)
    V = cam.world_view_transform.double()                      # W2C^T
    R = V[:3, :3]
    assert torch.allclose(R @ R.t(), torch.eye(3, dtype=torch.float64), atol=1e-6) and abs(float(torch.det(R)) - 1.0) < 1e-6
    assert float(cam.camera_center.abs().max()) > 1.0 and abs(cam.FoVx - cam.FoVy) > 1e-3
    assert torch.allclose(torch.cat([cam.camera_center.double(), torch.ones(1, dtype=torch.float64)]) @ V, torch.tensor([0, 0, 0, 1.0], dtype=torch.float64), atol=1e-5)
    local = torch.cat([g["means3D"].double(), torch.ones(P, 1, dtype=torch.float64)], 1) @ V
    z = local[:, 2]
    assert float(z.min()) > 0.99 and float(z.max()) < 50.01
    tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    assert float((local[:, 0].abs() / (z * tx)).max()) < 1.1001 and float((local[:, 1].abs() / (z * ty)).max()) < 1.1001
    inside = ((local[:, 0].abs() < z * tx) & (local[:, 1].abs() < z * ty)).double().mean()
    assert 0.78 < float(inside) < 0.88                         # ~17 % outside the frustum sides, as in the benchmark scene
    _, gb = posed_scene(P, W, H, seed=11, spread=20.0, behind_fraction=0.75)
    zb = (torch.cat([gb["means3D"].double(), torch.ones(P, 1, dtype=torch.float64)], 1) @ V)[:, 2]
    assert int((zb < 0).sum()) == 3000 and bool((zb[:1000] > 0).all())
    _, gn = posed_scene(P, W, H, seed=11, spread=20.0, near_third=True)
    zn = (torch.cat([gn["means3D"].double(), torch.ones(P, 1, dtype=torch.float64)], 1) @ V)[:, 2]
    assert float(zn[: P // 3].min()) > -0.1001 and float(zn[: P // 3].max()) < 0.4001 and float(zn[P // 3:].min()) > 0.99
    rig, gr = posed_rig(P, W, H, 4, seed=11, spread=20.0)
    assert torch.equal(rig[0].world_view_transform, cam.world_view_transform) and torch.equal(gr["means3D"], g["means3D"])
    centres = torch.stack([c.camera_center for c in rig])
    assert float(torch.pdist(centres).min()) > 0.05 and float((centres - centres[0]).norm(dim=1).max()) < 2.0 * math.sqrt(3) + 1e-3
    for c in rig[1:]:
        zc = (torch.cat([gr["means3D"].double(), torch.ones(P, 1, dtype=torch.float64)], 1) @ c.world_view_transform.double())[:, 2]
        assert float((zc > 0.2).double().mean()) > 0.98          # moved sideways / backwards, never into the scene


def test_per_semantics_cache_hits_across_the_views_the_upstream_getter_returns():
    """The upstream model's `get_semantics` is `self._semantics.squeeze(-1)`: a NEW view object per call [REF scene/gaussian_model.py:126].
    The cache of the derived class encodings must hit across such views, miss after an in-place change or a new parameter (densification),
    and never hold more than one entry per kind."""
    import torch
    from streetunveiler_amd import gaussian_renderer as gr

    class Model:
        def __init__(self, n):
            self._semantics = torch.randint(0, 6, (n, 1))

        @property
        def get_semantics(self):
            return self._semantics.squeeze(-1)

    gr._SEM_CACHE.clear()
    m = Model(500)
    a, b = m.get_semantics, m.get_semantics
    assert a is not b
    made = []
    make = lambda: made.append(1) or torch.zeros(1)
    v1 = gr._per_semantics(a, ("probe", 6), make)
    v2 = gr._per_semantics(b, ("probe", 6), make)
    assert v1 is v2 and len(made) == 1, "a second view of the same parameter must hit"
    del gr._SEM_CACHE["probe"]
    oh = gr._one_hot_classes(m.get_semantics, 6)
    assert oh.shape == (500, 6) and torch.equal(oh.argmax(1), m._semantics.squeeze(-1)) and gr._one_hot_classes(m.get_semantics, 6) is oh
    m._semantics[3, 0] = (m._semantics[3, 0] + 1) % 6                      # in-place edit: version bump
    oh2 = gr._one_hot_classes(m.get_semantics, 6)
    assert oh2 is not oh and torch.equal(oh2.argmax(1), m._semantics.squeeze(-1))
    m._semantics = torch.cat([m._semantics, torch.randint(0, 6, (40, 1))])   # densification: a new parameter
    assert gr._one_hot_classes(m.get_semantics, 6).shape == (540, 6)
    assert set(gr._SEM_CACHE) == {"one_hot"}, "one entry per kind: nothing stale stays alive"
    gr._SEM_CACHE.clear()


def test_resolve_tile_auto_by_frame_size(monkeypatch):
    """GaussianRasterizer(tile=...): None = the reference's 16x16 unless SURFEL_TILE says otherwise; "auto" = 8x8 for the reference's own
    `-r 4` frames (480x320: 600 tiles of 16x16 cannot fill 3 072 wave slots), 16x8 in between, 16x16 from ~1280x720 up."""
    from diff_surfel_rasterization import resolve_tile
    monkeypatch.delenv("SURFEL_TILE", raising=False)
    assert resolve_tile(None, 1920, 1080) is None and resolve_tile((16, 16), 480, 320) is None
    assert resolve_tile("auto", 480, 320) == (8, 8) and resolve_tile("auto", 640, 480) == (8, 8)
    assert resolve_tile("auto", 960, 640) == (16, 8)
    assert resolve_tile("auto", 1280, 720) is None and resolve_tile("auto", 1920, 1080) is None and resolve_tile("auto", 3840, 2160) is None
    assert resolve_tile("32x16", 100, 100) == (32, 16) and resolve_tile((8, 8), 4000, 4000) == (8, 8)
    monkeypatch.setenv("SURFEL_TILE", "auto")
    assert resolve_tile(None, 480, 320) == (8, 8) and resolve_tile(None, 1920, 1080) is None
    assert resolve_tile((32, 8), 480, 320) == (32, 8), "an explicit shape wins over the process default"


def _visible_rows_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from streetunveiler_amd.parallel import allreduce_gradients, allreduce_visible_rows, init_distributed, pack_visibility, unpack_visibility
    init_distributed(backend="gloo")
    P = 1003                                                    # (not a multiple of 8: the bitmap's last byte is partial)
    g = torch.Generator().manual_seed(500 + rank)
    out = {}
    for case, frac in (("street", 0.17), ("benchmark", 0.9), ("nothing", 0.0)):
        vis = torch.rand(P, generator=g) < frac                 # each rank sees its own subset
        assert torch.equal(unpack_visibility(pack_visibility(vis), P), vis)
        # the operator's gradients: one flat buffer carved into [P,3] | [P,16,3] | [P,1] | [P,2] | [P,4], exact zeros on rows the frame did not reach.
        # Integer-valued floats: every partial sum is exact, so the result does not depend on the order a ring adds the ranks in and
        # "the dense all-reduce's sums, bit for bit" is a meaningful statement for any number of ranks.
        flat = torch.randint(-50, 51, (P * 58,), generator=g).float()
        shapes = [(P, 3), (P, 16, 3), (P, 1), (P, 2), (P, 4)]
        views, off = [], 0
        for shp in shapes:
            n = int(torch.tensor(shp).prod()); views.append(flat[off:off + n].view(shp)); off += n
        for v in views:
            v[~vis] = 0
        dense = flat.clone()
        dviews, off = [], 0
        for shp in shapes:
            n = int(torch.tensor(shp).prod()); dviews.append(dense[off:off + n].view(shp)); off += n
        allreduce_gradients(dviews)
        info = allreduce_visible_rows(views, vis)
        out[case] = dict(compact=flat.clone(), dense=dense, info=info, vis=vis)
    # real-valued gradients, world 2: a + b is commutative -> bit-identical there too
    vis = torch.rand(P, generator=g) < 0.3
    a = torch.randn(P, 7, generator=g); a[~vis] = 0
    b = a.clone()
    allreduce_gradients([b]); allreduce_visible_rows([a], vis)
    out["real"] = dict(compact=a, dense=b)
    torch.save(out, os.path.join(tmp, f"v{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_visibility_compacted_gradient_exchange_equals_the_dense_allreduce(tmp_path, world):
    """allreduce_visible_rows: the ranks exchange only the rows reached on at least one rank (bitmaps all-gathered, union rows in ONE
    compacted buffer).  Same sums as the dense all-reduce, bit for bit; far fewer bytes when most Gaussians are behind the camera."""
    port = 33500 + (os.getpid() % 2000) + world
    mp.spawn(_visible_rows_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    rs = [torch.load(os.path.join(tmp_path, f"v{r}.pt")) for r in range(world)]
    P = 1003
    for case in ("street", "benchmark", "nothing"):
        for r in rs:
            assert torch.equal(r[case]["compact"], r[case]["dense"]), f"{case}: the compacted exchange differs from the dense all-reduce"
            assert torch.equal(r[case]["compact"], rs[0][case]["compact"]), "every rank holds the same sums"
        union = torch.stack([r[case]["vis"] for r in rs]).any(0)
        info = rs[0][case]["info"]
        assert info["rows_union"] == int(union.sum()) and info["rows_total"] == P
        dense_bytes = P * 58 * 4
        assert info["bytes_dense_equivalent"] == dense_bytes
        if case == "street":       # 17 % visible per rank: the union of 2 (4) ranks is ~31 % (~53 %) of the rows
            assert info["bytes_payload"] == info["rows_union"] * 58 * 4 + (P + 7) // 8 and info["bytes_payload"] < 0.62 * dense_bytes
        elif case == "benchmark":  # nearly everything visible: the dense path, plus the bitmap
            assert info["bytes_payload"] == dense_bytes + (P + 7) // 8
        else:
            assert info["bytes_payload"] == (P + 7) // 8
    if world == 2:
        for r in rs:
            assert torch.equal(r["real"]["compact"], r["real"]["dense"])
    else:
        for r in rs:
            torch.testing.assert_close(r["real"]["compact"], r["real"]["dense"], rtol=1e-6, atol=1e-6)

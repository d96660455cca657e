"""GPU (-m gpu): simple_knn drop-in against the brute-force CPU oracle (bit-exact) and scipy's KD-tree.

The cases are the table of tests/knn_cases.py: every instantiation of knn_search_kernel (K in {3, 10} x {self, reference}, with and without
the square root) at every size where the code takes another path, every cloud shape, and clouds with NaN / inf points, whose damage must
stay in their own rows.  tests/test_knn_host.py shows that this table rejects the wrong searches one can think of."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import knn_cases as kc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (3, 10)
FLT_MAX = np.float32(np.finfo(np.float32).max)

_cloud = kc.lidar_cloud


def _knn(query, reference, K, take_sqrt=False):
    """simple_knn._C._knn on host arrays -> host array (query None: self mode)."""
    from simple_knn._C import _knn as op
    q = None if query is None else torch.tensor(query, device=DEV)
    return op(q, torch.tensor(reference, device=DEV), K, take_sqrt).cpu().numpy()


def _same_bits(got, want, what):
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)    # bits: tells -0 from 0 and compares NaN


@pytest.mark.parametrize("n,seed", [(20000, 0), (777, 1), (513, 2), (64, 3), (11, 4)])
def test_dist3knn_dist10knn_bit_exact_vs_bruteforce(n, seed):
    from oracle.knn_oracle import knn_mean_dist2
    from simple_knn._C import dist10knn, dist3knn, distCUDA2
    pts = _cloud(n, seed)
    t = torch.tensor(pts, device=DEV)
    got3 = dist3knn(t).cpu().numpy()
    np.testing.assert_array_equal(got3, knn_mean_dist2(pts, 3))
    assert (got3 >= 0).all() and distCUDA2 is dist3knn
    np.testing.assert_array_equal(dist10knn(t).cpu().numpy(), knn_mean_dist2(pts, 10))


def test_knn_edge_cases():
    from oracle.knn_oracle import knn_mean_dist2
    from simple_knn._C import dist3knn, meanDistFromReferencePcd
    from streetunveiler_amd._lib import SurfelRasterError
    assert dist3knn(torch.zeros(0, 3, device=DEV)).shape == (0,)
    for n in (1, 2, 3, 4):   # fewer than K other points: the missing neighbours count as FLT_MAX, like the oracle
        pts = _cloud(n, 10 + n, clustered=False)
        np.testing.assert_array_equal(dist3knn(torch.tensor(pts, device=DEV)).cpu().numpy(), knn_mean_dist2(pts, 3))
    flat = _cloud(5000, 5, clustered=False); flat[:, 1] = 2.5            # degenerate extent along y
    np.testing.assert_array_equal(dist3knn(torch.tensor(flat, device=DEV)).cpu().numpy(), knn_mean_dist2(flat, 3))
    same = np.ones((300, 3), np.float32)                                  # all points identical
    assert not dist3knn(torch.tensor(same, device=DEV)).any()
    with pytest.raises(SurfelRasterError):
        dist3knn(torch.zeros(5, 3))
    with pytest.raises(SurfelRasterError):
        dist3knn(torch.zeros(5, 2, device=DEV))
    with pytest.raises(SurfelRasterError):
        meanDistFromReferencePcd(torch.zeros(5, 3, device=DEV), torch.zeros(0, 3, device=DEV))


def test_mean_dist_from_reference_cloud():
    from oracle.knn_oracle import knn_mean_dist2
    from simple_knn._C import meanDistFromReferencePcd
    ref = _cloud(30000, 6)
    qry = _cloud(4000, 7)
    qry[:100] = ref[:100]     # queries sitting on reference points: the point itself counts (distance 0)
    got = meanDistFromReferencePcd(torch.tensor(qry, device=DEV), torch.tensor(ref, device=DEV), False).cpu().numpy()
    np.testing.assert_array_equal(got, knn_mean_dist2(qry, 3, reference=ref))
    root = meanDistFromReferencePcd(torch.tensor(qry, device=DEV), torch.tensor(ref, device=DEV), True).cpu().numpy()
    np.testing.assert_array_equal(root, knn_mean_dist2(qry, 3, reference=ref, take_sqrt=True))
    # far-away queries (outside the reference's bounding box)
    far = qry + np.array([500, 0, -300], np.float32)
    got = meanDistFromReferencePcd(torch.tensor(far, device=DEV), torch.tensor(ref, device=DEV)).cpu().numpy()
    np.testing.assert_array_equal(got, knn_mean_dist2(far, 3, reference=ref))


# ---- the bit-exact matrix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", kc.SELF_SIZES)
def test_self_mode_sizes_bit_exact(n, K):
    """knn_search_kernel<K, true> with and without the square root, at every size of kc.SELF_SIZES."""
    pts = kc.self_cloud(n)
    for take_sqrt in (False, True):
        _same_bits(_knn(None, pts, K, take_sqrt), kc.oracle("self", n, K, take_sqrt), f"self n={n} K={K} sqrt={take_sqrt}")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("nq,nr", kc.REF_SIZES)
def test_reference_mode_sizes_bit_exact(nq, nr, K):
    """knn_search_kernel<K, false> with and without the square root, at every (nq, nr) of kc.REF_SIZES."""
    qry, ref = kc.ref_clouds(nq, nr)
    for take_sqrt in (False, True):
        _same_bits(_knn(qry, ref, K, take_sqrt), kc.oracle("ref", (nq, nr), K, take_sqrt), f"reference nq={nq} nr={nr} K={K} sqrt={take_sqrt}")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(kc.SHAPES))
def test_cloud_shapes_bit_exact(name, K):
    """Every cloud shape of kc.SHAPES, against itself and (its first 700 points as queries) in reference mode.

    denormal_blob: the squared distances are float32 denormals.  The kernels (gfx950, float32 denormals on) and the oracle (x86-64, no
    flush) agree bit for bit; neither side flushes."""
    pts = kc.shape_cloud(name)
    _same_bits(_knn(None, pts, K), kc.oracle("shape", name, K), f"{name} K={K}: {kc.SHAPES[name][0]}")
    from oracle.knn_oracle import knn_mean_dist2
    _same_bits(_knn(pts[:700], pts, K, True), knn_mean_dist2(pts[:700], K, reference=pts, take_sqrt=True), f"{name} K={K}, reference mode")


@pytest.mark.parametrize("K", KS)
def test_missing_neighbours_give_the_oracles_inf(K):
    """Fewer than K candidates: the missing ones are FLT_MAX, so two or more of them overflow the sum to inf, and exactly one leaves
    FLT_MAX / K (it absorbs the finite distances) -- in both, the oracle's bits."""
    from oracle.knn_oracle import knn_mean_dist2
    for others in (0, 1, K - 2, K - 1, K):
        pts = kc.lidar_cloud(others + 1, 40 + others, clustered=False)
        got = _knn(None, pts, K)
        _same_bits(got, knn_mean_dist2(pts, K), f"{others} others, K={K}")
        if others <= K - 2:
            assert np.isposinf(got).all()
        elif others == K - 1:
            assert (got == FLT_MAX / np.float32(K)).all()
        else:
            assert np.isfinite(got).all() and (got < 1e6).all()
        if others:      # the same through the reference-mode kernel: `others` reference points in all
            qry = kc.lidar_cloud(70, 50 + others, clustered=False)
            got = _knn(qry, pts[:others], K)
            _same_bits(got, knn_mean_dist2(qry, K, reference=pts[:others]), f"{others} reference points, K={K}")
            assert np.isposinf(got).all() if others <= K - 2 else (got == FLT_MAX / np.float32(K)).all() if others == K - 1 else np.isfinite(got).all()


# ---- containment of non-finite points ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(kc.NONFINITE))
def test_non_finite_points_do_not_spread(name, K):
    """A NaN or inf point is nobody's neighbour and has none: its own row is inf, every other row is what the cloud without it gives."""
    pts, bad = kc.nonfinite_self(name)
    want = kc.oracle("nonfinite_self", name, K)
    assert np.isposinf(want[bad]).all() and np.isfinite(np.delete(want, bad)).all()
    got = _knn(None, pts, K)
    wrong = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"{name} K={K}: {len(wrong)} of {len(got)} rows differ from the oracle" + (f"; first rows {wrong[:5].tolist()}: got {got[wrong[:5]].tolist()}, oracle {want[wrong[:5]].tolist()}" if len(wrong) else ""))
    _same_bits(got, want, f"{name} K={K}: {kc.NONFINITE[name][0]}")
    _same_bits(np.delete(got, bad), _knn(None, np.delete(pts, bad, axis=0), K), f"{name} K={K}: finite rows against the op on the cloud without the non-finite points")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("side", ("query", "reference"))
@pytest.mark.parametrize("name", sorted(kc.NONFINITE))
def test_non_finite_points_do_not_spread_in_reference_mode(name, side, K):
    """The same for meanDistFromReferencePcd's kernel: a non-finite reference point is ignored by every query; a non-finite query gets inf
    and leaves the other queries alone."""
    qry, ref, bad = kc.nonfinite_ref(name, side)
    want = kc.oracle("nonfinite_ref", (name, side), K)
    got = _knn(qry, ref, K)
    wrong = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"{name} in the {side} K={K}: {len(wrong)} of {len(got)} rows differ from the oracle")
    _same_bits(got, want, f"{name} in the {side}, K={K}")
    if side == "reference":
        assert np.isfinite(want).all()
        _same_bits(got, _knn(qry, np.delete(ref, bad, axis=0), K), f"{name} K={K}: against the op on the reference without the non-finite points")
    else:
        assert np.isposinf(want[bad]).all() and np.isfinite(np.delete(want, bad)).all()
        _same_bits(np.delete(got, bad), _knn(np.delete(qry, bad, axis=0), ref, K), f"{name} K={K}: finite queries against the op without the others")


# ---- contract ------------------------------------------------------------------------------------------------------------------
def test_side_stream_and_repeat_give_the_same_bits():
    from simple_knn._C import _knn as op
    qry, ref = kc.ref_clouds(4000, 32769)
    q, r = torch.tensor(qry, device=DEV), torch.tensor(ref, device=DEV)
    first = {(K, mode): op(q if mode else None, r, K).cpu().numpy() for K in KS for mode in (0, 1)}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        on_side = {key: op(q if key[1] else None, r, key[0]) for key in first}
    side.synchronize()
    for key, want in first.items():
        _same_bits(on_side[key].cpu().numpy(), want, f"side stream K={key[0]} reference-mode={key[1]}")
        _same_bits(op(q if key[1] else None, r, key[0]).cpu().numpy(), want, f"second call K={key[0]} reference-mode={key[1]}")


def test_input_forms_give_the_contiguous_float32_result():
    """float64, a non-contiguous view ([:, ::2] of an (n, 6) tensor) and requires_grad inputs; the input is left as it was."""
    from simple_knn._C import dist3knn, dist10knn, meanDistFromReferencePcd
    pts = kc.self_cloud(1025)
    t = torch.tensor(pts, device=DEV)
    want3, want10 = dist3knn(t).cpu().numpy(), dist10knn(t).cpu().numpy()
    _same_bits(want3, kc.oracle("self", 1025, 3), "contiguous float32")
    np.testing.assert_array_equal(t.cpu().numpy(), pts)                      # the input is unchanged
    wide = torch.zeros(len(pts), 6, device=DEV)
    wide[:, ::2] = t
    wide[:, 1::2] = 7.0
    before = wide.clone()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    forms = {"float64": t.double(), "non-contiguous": view, "requires_grad": t.clone().requires_grad_()}
    for what, x in forms.items():
        out = dist3knn(x)
        assert out.dtype == torch.float32 and not out.requires_grad and out.shape == (len(pts),)
        _same_bits(out.cpu().numpy(), want3, what)
        _same_bits(dist10knn(x).cpu().numpy(), want10, what + " K=10")
        _same_bits(meanDistFromReferencePcd(x[:300], x, True).cpu().numpy(), _knn(pts[:300], pts, 3, True), what + " reference mode")
    assert torch.equal(wide, before) and forms["float64"].dtype == torch.float64


def test_workspace_one_byte_short_is_refused():
    from streetunveiler_amd import _lib
    lib = _lib.load()
    for nq, nr in ((0, 1025), (700, 513), (513, 64)):
        ref = torch.tensor(kc.lidar_cloud(nr, 60), device=DEV)
        qry = torch.tensor(kc.lidar_cloud(nq, 61), device=DEV) if nq else None
        need = lib.sr_knn_workspace_bytes(nq, nr)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        out = torch.full((nq or nr,), -1.0, device=DEV)
        args = (nq, C.c_void_p(qry.data_ptr()) if nq else None, nr, C.c_void_p(ref.data_ptr()), 3, 0, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()))
        assert lib.sr_knn_mean_dist2(*args, need - 1, None) == -3 and b"workspace" in lib.sr_last_error()     # SR_ERR_BUFFER_TOO_SMALL
        torch.cuda.synchronize()
        assert (out == -1).all()                                                                               # and nothing ran
        assert lib.sr_knn_mean_dist2(*args, need, None) == 0
        torch.cuda.synchronize()
        assert (out >= 0).all()


# ---- 1 M points ----------------------------------------------------------------------------------------------------------------
# Candidates per point taken from the float64 KD-tree for the exact reference.  Verified once on the CPU (not part of the suite): with
# this c, kc.kdtree_exact_mean_dist2 equals oracle.knn_oracle.knn_mean_dist2 (brute force, 10^12 pairs) on all 1 000 000 rows of the
# cloud below.
C_1M = 8


def test_dist3knn_large_cloud_vs_kdtree():
    """1 M points (scene-initialisation scale, 1954 boxes = 31 passes of the box-group loop): checked against scipy's KD-tree in float64
    to rtol 2e-4, and EXACTLY against the float32 re-measurement of each point's C_1M nearest others from that tree
    (kc.kdtree_exact_mean_dist2), which equals the brute-force oracle on every row of this cloud.  No row is excluded."""
    from scipy.spatial import cKDTree
    from simple_knn._C import dist3knn
    from streetunveiler_amd.synthetic import synthetic_gaussians
    pts = synthetic_gaussians(1_000_000, 1920, 1080, seed=2)["means3D"].numpy()
    got = dist3knn(torch.tensor(pts, device=DEV)).cpu().numpy()
    d, idx = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=C_1M + 1, workers=-1)
    expect = (d[:, 1:4] ** 2).mean(axis=1)
    np.testing.assert_allclose(got, expect, rtol=2e-4, atol=1e-9)
    _same_bits(got, kc.kdtree_exact_mean_dist2(pts, 3, C_1M, idx=idx), "1 M points against the exact KD-tree reference")

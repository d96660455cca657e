"""CPU: what the kNN tests stand on.
  * The brute-force oracle (oracle/knn_oracle.c) is pinned: non-finite points are ignored, missing neighbours are FLT_MAX, and every variant
    agrees with a float64 evaluation.
  * The C-ABI of the kNN op refuses bad arguments before any launch, without a GPU.
  * The case table (tests/knn_cases.py) rejects wrong searches: numpy restatements of the search with one mistake each differ from the
    oracle on a named case, while the same restatements without the mistake reproduce it bit for bit.
The -m gpu counterpart (tests/test_gpu_knn.py) runs the HIP kernels on the same table."""
import ctypes as C

import numpy as np
import pytest

from oracle.knn_oracle import knn_mean_dist2
from streetunveiler_amd import _lib
from streetunveiler_amd.build import build
from tests import knn_cases as kc

FLT_MAX = np.float32(np.finfo(np.float32).max)
KS = (3, 10)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the oracle's semantics ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(kc.NONFINITE))
def test_oracle_ignores_non_finite_points(name, K):
    pts, bad = kc.nonfinite_self(name)
    got = kc.oracle("nonfinite_self", name, K)
    assert np.isposinf(got[bad]).all()
    np.testing.assert_array_equal(_bits(np.delete(got, bad)), _bits(knn_mean_dist2(np.delete(pts, bad, axis=0), K)))
    for side in ("query", "reference"):
        qry, ref, bad = kc.nonfinite_ref(name, side)
        got = kc.oracle("nonfinite_ref", (name, side), K)
        if side == "reference":
            np.testing.assert_array_equal(_bits(got), _bits(knn_mean_dist2(qry, K, reference=np.delete(ref, bad, axis=0))))
        else:
            assert np.isposinf(got[bad]).all()
            np.testing.assert_array_equal(_bits(np.delete(got, bad)), _bits(knn_mean_dist2(np.delete(qry, bad, axis=0), K, reference=ref)))


def test_non_finite_index_sets_cover_first_inside_and_last():
    for name in ("nan_points", "nan_y"):
        pts, bad = kc.nonfinite_self(name)
        assert bad[0] == 0 and bad[-1] == len(pts) - 1 and 0 < bad[1] < len(pts) - 1 and np.isnan(pts[bad]).any(axis=1).all()
        assert len(pts) <= 4096
    pts, bad = kc.nonfinite_self("inf_coords")
    assert np.isposinf(pts).sum() == 1 and np.isneginf(pts).sum() == 1 and not np.isnan(pts).any()
    assert np.isnan(kc.nonfinite_self("nan_y")[0][:, [0, 2]]).sum() == 0


@pytest.mark.parametrize("K", KS)
def test_oracle_counts_missing_neighbours_as_flt_max(K):
    """K > number of others: two or more missing neighbours overflow the float32 sum to inf; exactly one leaves FLT_MAX / K."""
    for others in range(0, K + 1):
        pts = kc.lidar_cloud(others + 1, 40 + others, clustered=False)
        got = knn_mean_dist2(pts, K)
        if others <= K - 2:
            assert np.isposinf(got).all(), (others, got)
        elif others == K - 1:
            assert (got == FLT_MAX / np.float32(K)).all(), (others, got)
        else:
            assert np.isfinite(got).all() and (got < 1e6).all()
        if others:
            ref = knn_mean_dist2(pts[:1], K, reference=pts[1:])     # the same count through the reference form
            assert _bits(ref)[0] == _bits(got)[0]


def test_oracle_variants_against_float64():
    """Self / reference, with and without the root, K = 3 and 10, on a 300-point cloud against numpy in float64.  The bar is one float32 ulp
    per squared distance, (sum of the K distances' ulps) / K, plus what the float32 reduction itself must round: half an ulp of the sum for
    each of its K-1 additions (/ K) and half an ulp of the mean for the division.  Through the root it becomes bar / (2 sqrt(mean)) plus
    the root's own half ulp."""
    pts = kc.lidar_cloud(300, 70).astype(np.float64)
    qry = kc.lidar_cloud(120, 71).astype(np.float64)
    for K in KS:
        for reference in (None, pts):
            q = pts if reference is None else qry
            d = ((q[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
            if reference is None:
                np.fill_diagonal(d, np.inf)
            best = np.sort(d, axis=1)[:, :K]
            exact = best.mean(axis=1)
            bar = np.spacing(best.astype(np.float32)).astype(np.float64).sum(axis=1) / K
            bar += (K - 1) * 0.5 * np.spacing(best.sum(axis=1).astype(np.float32)) / K + 0.5 * np.spacing(exact.astype(np.float32))
            got = knn_mean_dist2(q.astype(np.float32), K, reference=None if reference is None else pts.astype(np.float32))
            worst = (np.abs(got - exact) / np.maximum(bar, 1e-300)).max()
            assert (np.abs(got - exact) <= bar).all(), (K, reference is None, worst)
            root = knn_mean_dist2(q.astype(np.float32), K, reference=None if reference is None else pts.astype(np.float32), take_sqrt=True)
            np.testing.assert_array_equal(_bits(root), _bits(np.sqrt(got)))      # a correctly rounded float32 root of the same mean
            ok = exact > 0
            root_bar = bar[ok] / (2 * np.sqrt(exact[ok])) + 0.5 * np.spacing(root[ok]).astype(np.float64)
            assert (np.abs(root[ok] - np.sqrt(exact[ok])) <= root_bar).all(), (K, reference is None)


def test_numpy_restatement_is_the_oracle():
    """kc.dist2_f32 + kc.mean_of_k_smallest (what the mutants below and the 1 M-point reference are made of) reproduce the oracle's bits."""
    for kind, key in (("self", 257), ("shape", "identical_box"), ("nonfinite_self", "nan_points"), ("nonfinite_self", "inf_coords")):
        pts = {"self": kc.self_cloud, "shape": kc.shape_cloud, "nonfinite_self": lambda k: kc.nonfinite_self(k)[0]}[kind](key)
        for K in KS:
            np.testing.assert_array_equal(_bits(_brute(pts, K)), _bits(kc.oracle(kind, key, K)), err_msg=f"{kind} {key} K={K}")
    pts = kc.self_cloud(1025)
    for c in (3, 8):
        np.testing.assert_array_equal(_bits(kc.kdtree_exact_mean_dist2(pts, 3, c)), _bits(kc.oracle("self", 1025, 3)))


# ---- the C-ABI refuses before any launch ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def test_argument_errors_without_gpu(lib):
    """Refused before any launch: the pointers below are never dereferenced (no GPU is needed, and none is touched)."""
    p = C.c_void_p(4096)      # stands for a device pointer
    big = 1 << 40
    call = lambda nq, q, nr, r, K, out, ws, nbytes: lib.sr_knn_mean_dist2(nq, q, nr, r, K, 0, out, ws, nbytes, None)
    assert call(0, None, 100, p, 5, p, p, big) == -4 and b"K = 5" in lib.sr_last_error()              # SR_ERR_UNSUPPORTED
    assert call(7, p, 100, p, 0, p, p, big) == -4
    assert call(0, None, -1, p, 3, p, p, big) == -1 and b"negative" in lib.sr_last_error()
    assert call(-1, p, 100, p, 3, p, p, big) == -1 and b"negative" in lib.sr_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):                                              # reference, out, workspace
        r, out, ws = args
        assert call(0, None, 100, r, 10, out, ws, big) == -1 and b"NULL" in lib.sr_last_error()
        assert call(7, p, 100, r, 3, out, ws, big) == -1 and b"NULL" in lib.sr_last_error()
    assert call(5, p, 0, p, 3, p, p, big) == -1 and b"empty reference" in lib.sr_last_error()
    for nq, nr in ((0, 1), (0, 1025), (700, 513), (513, 64)):
        need = lib.sr_knn_workspace_bytes(nq, nr)
        assert need > 0
        for short in (need - 1, 0):
            assert call(nq, p if nq else None, nr, p, 3, p, p, short) == -3 and b"workspace" in lib.sr_last_error()   # SR_ERR_BUFFER_TOO_SMALL
    # nothing to do is no error, whatever else is passed
    assert call(0, None, 0, None, 3, None, None, 0) == 0
    assert call(0, p, 100, p, 10, None, None, 0) == 0
    assert call(0, p, 0, None, 3, None, None, 0) == 0


def test_workspace_bytes_are_monotone(lib):
    """Monotone in either count, and never short of what the layout holds: per point of either cloud two code arrays, the order and
    the sorted float4 (28 bytes), 32 bytes per box of 512 reference points, and the radix sort's temporary for the LARGER cloud.  With
    the counts swapped only the box table differs (a query cloud has none): apart from it, nq > nr asks for no less than nr > nq."""
    ws = lib.sr_knn_workspace_bytes
    boxes = lambda n: 32 * ((n + kc.BOX - 1) // kc.BOX)
    align = lambda b: (max(b, 1) + 255) // 256 * 256
    sizes = (0, 1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 32768, 32769, 65537, 1_000_000, 3_000_000)
    for fixed in sizes:
        row = [ws(n, max(fixed, 1)) for n in sizes]
        col = [ws(fixed, n) for n in sizes]
        assert row == sorted(row) and col == sorted(col), fixed
    for nq in sizes:
        for nr in sizes:
            assert ws(nq, nr) >= 28 * (nq + nr) + boxes(nr) + lib.sr_debug_radix_sort_temp_bytes(max(nq, nr)), (nq, nr)
            if nq > nr >= 1:
                assert ws(nq, nr) - align(boxes(nr)) >= ws(nr, nq) - align(boxes(nq)), (nq, nr)
    assert ws(-5, -5) == ws(0, 0)


# ---- the case table rejects wrong searches -------------------------------------------------------------------------------------
def _brute(pts, K, rows=None, keep_self=False, candidates=None, transform=None, count=None):
    """Self-mode brute force in numpy float32 (the oracle restated), with the hooks the mutants turn."""
    rows = np.arange(len(pts)) if rows is None else rows
    d = kc.dist2_f32(pts[rows], pts)
    if not keep_self:
        d[np.arange(len(rows)), rows] = FLT_MAX
    if candidates is not None:
        d[:, ~candidates] = FLT_MAX
    if transform is not None:
        with np.errstate(invalid="ignore"):
            d = transform(d)
    return kc.mean_of_k_smallest(d, K if count is None else count)


def _insertion(pts, K, poisoned):
    """Candidate after candidate into an ascending K-list, as the kernel does it: the branch-free fmin / fmax chain.  poisoned: a NaN distance
    goes into the chain as it is (both calls hand back best[k], so every entry is duplicated one slot down); else it is dropped first."""
    d = kc.dist2_f32(pts, pts)
    np.fill_diagonal(d, FLT_MAX)
    best = np.full((len(pts), K), FLT_MAX, np.float32)
    for j in range(len(pts)):
        c = d[:, j].copy()
        if not poisoned:
            c = np.fmin(c, FLT_MAX)
        for k in range(K):
            lo = np.fmin(best[:, k], c)
            c = np.fmax(best[:, k], c)
            best[:, k] = lo
    with np.errstate(over="ignore"):
        s = best[:, 0].copy()
        for k in range(1, K):
            s = s + best[:, k]
        return s / np.float32(K)


def _morton_order(pts):
    """The curve order of knn_morton_kernel (10 bits per axis over the cloud's bounds), ties in input order."""
    lo, hi = np.fmin.reduce(pts, axis=0), np.fmax.reduce(pts, axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        ext = np.fmax(hi - lo, np.float32(1e-30))
        t = (pts - lo) / ext * np.float32(1023)
        q = np.fmin(np.fmax(t, np.float32(0)), np.float32(1023))
    q = np.where(np.isnan(q), 0, q).astype(np.uint32)
    code = np.zeros(len(pts), np.uint32)
    for bit in range(10):
        for c in range(3):
            code |= ((q[:, c] >> bit) & 1) << (3 * bit + c)
    return np.argsort(code, kind="stable")


def _pruned_search(pts, K, centre_shift=0, drop_partial_box=False):
    """The search of knn_search_kernel<K, true> restated per query: the first bound `reject` from the K curve neighbours on either side
    of `centre`, then every box of 512 curve-consecutive points whose AABB is not farther than `reject`.  centre_shift = K takes the window
    from the wrong end (and the query itself into it); drop_partial_box loses the candidates of the last, partial box."""
    order = _morton_order(pts)
    P = pts[order]
    n = len(P)
    d = kc.dist2_f32(P, P)
    pos = np.arange(n)
    window = np.full((n, 2 * K), FLT_MAX, np.float32)
    col = 0
    for o in range(-K, K + 1):
        if o == 0:
            continue
        j = pos + centre_shift + o
        ok = (j >= 0) & (j < n)
        window[ok, col] = d[pos[ok], j[ok]]
        col += 1
    reject = np.sort(np.fmin(window, FLT_MAX), axis=1)[:, K - 1]
    np.fill_diagonal(d, FLT_MAX)
    n_boxes = (n + kc.BOX - 1) // kc.BOX
    for b in range(n_boxes):
        first, last = b * kc.BOX, min(n, (b + 1) * kc.BOX)
        bl, bh = P[first:last].min(axis=0), P[first:last].max(axis=0)
        gap = np.maximum(np.float32(0), np.maximum(bl - P, P - bh))
        pd = (gap[:, 0] * gap[:, 0] + gap[:, 1] * gap[:, 1]) + gap[:, 2] * gap[:, 2]
        skip = pd > reject
        if drop_partial_box and last - first < kc.BOX:
            skip[:] = True
        d[skip, first:last] = FLT_MAX
    out = np.empty(n, np.float32)
    out[order] = kc.mean_of_k_smallest(d, K)
    return out


_SPREAD_ROWS = np.arange(0, 65537, 257)

# mutant -> (what is wrong, (kind, key) of the case that must reject it, K, the search with the mistake, the rows it is run on)
MUTANTS = {
    "own_neighbour": ("the point counts as its own neighbour", ("self", 12), 3, lambda p, K: _brute(p, K, keep_self=True), None),
    "k_minus_1": ("K-1 neighbours are averaged", ("self", 64), 10, lambda p, K: _brute(p, K, count=K - 1), None),
    "unsquared": ("distances instead of squared distances", ("self", 65), 3, lambda p, K: _brute(p, K, transform=np.sqrt), None),
    "nan_poisoned_insertion": ("a NaN distance goes through the fmin / fmax chain", ("nonfinite_self", "nan_points"), 3,
                               lambda p, K: _insertion(p, K, poisoned=True), None),
    "nan_poisoned_insertion_nan_y": ("a NaN distance goes through the fmin / fmax chain", ("nonfinite_self", "nan_y"), 10,
                                     lambda p, K: _insertion(p, K, poisoned=True), None),
    "second_box_group_pass_lost": ("every candidate from index 32768 on is dropped", ("self", 65537), 3,
                                   lambda p, K: _brute(p, K, rows=_SPREAD_ROWS, candidates=np.arange(len(p)) < 32768), _SPREAD_ROWS),
    "second_box_group_pass_lost_by_one": ("every candidate from index 32768 on is dropped", ("self", 32769), 10,
                                          lambda p, K: _brute(p, K, rows=_near(p, 32768), candidates=np.arange(len(p)) < 32768), "near_32768"),
    "last_partial_box_lost": ("the last, partial box is not scanned", ("self", 513), 3, lambda p, K: _pruned_search(p, K, drop_partial_box=True), None),
    "first_bound_from_the_wrong_end": ("the first-bound window is centred K places off", ("shape", "offset_blob"), 3,
                                       lambda p, K: _pruned_search(p, K, centre_shift=K), None),
}


def _near(pts, i, count=64):
    """The rows nearest to point i (the only ones a lost candidate i can change)."""
    return np.sort(np.argsort(kc.dist2_f32(pts[i:i + 1], pts)[0], kind="stable")[:count])


def _case_cloud(kind, key):
    return {"self": kc.self_cloud, "shape": kc.shape_cloud, "nonfinite_self": lambda k: kc.nonfinite_self(k)[0]}[kind](key)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_case_table_rejects(name):
    what, (kind, key), K, search, rows = MUTANTS[name]
    pts = _case_cloud(kind, key)
    want = kc.oracle(kind, key, K)
    if isinstance(rows, str):
        rows = _near(pts, 32768)
    if rows is not None:
        want = want[rows]
    got = search(pts, K)
    differing = int((_bits(got) != _bits(want)).sum())
    assert differing > 0, f"case {kind} {key} (K={K}) does not reject the search in which {what}"


def test_the_restated_searches_are_exact_without_their_mistake():
    """The same restatements with the mistake taken out give the oracle's bits on the rejecting cases: what the mutants fail on is the
    mistake, not the restatement."""
    for n in (513, 1025):
        for K in KS:
            np.testing.assert_array_equal(_bits(_pruned_search(kc.self_cloud(n), K)), _bits(kc.oracle("self", n, K)), err_msg=f"pruned search n={n} K={K}")
    np.testing.assert_array_equal(_bits(_pruned_search(kc.shape_cloud("offset_blob"), 3)), _bits(kc.oracle("shape", "offset_blob", 3)))
    for name in ("nan_points", "nan_y"):
        pts = kc.nonfinite_self(name)[0]
        for K in KS:
            np.testing.assert_array_equal(_bits(_insertion(pts, K, poisoned=False)), _bits(kc.oracle("nonfinite_self", name, K)), err_msg=f"{name} K={K}")
    # on a finite cloud the poisoned chain IS exact: no finite case can see that mistake
    np.testing.assert_array_equal(_bits(_insertion(kc.self_cloud(513), 3, poisoned=True)), _bits(kc.oracle("self", 513, 3)))
    pts = kc.self_cloud(65537)
    np.testing.assert_array_equal(_bits(_brute(pts, 3, rows=_SPREAD_ROWS)), _bits(kc.oracle("self", 65537, 3)[_SPREAD_ROWS]))

"""Shared by tests/test_mesh_host.py, tests/test_gpu_mesh.py, tools/mesh_parity.py and tools/time_mesh.py: the cases of marching cubes
(streetunveiler_amd.mesh), their expectation (marching_cubes_numpy in float64 and in float32, computed once per case and left unchanged),
the topological measures the host tests hold the checker itself to, and THE BAR (`compare`):

  * faces equal the float64 checker's integer for integer, and so do Nv and Nf -- the decisions (inside, finite) are exact comparisons
    of float32 values, the order of vertices and faces is part of the contract and there are no atomics;
  * every vertex coordinate stays within BAR x max(dev32, FLOOR x scale) of the float64 checker's, dev32 = the largest |float32 checker -
    float64 checker| of the case and scale = its largest |coordinate| (the sky model's bar: a float32 evaluation of the same expression
    may round in another order than the twin, and where the twin happens to be exact one float32 ulp must still pass).

The shapes are the smallest at which the kernels can still go wrong: one cell; an odd cube; three different axis lengths; one row longer
than a wave and than a block along each axis; several 4096-point chunks through the scan; no cell at all."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np

from streetunveiler_amd import mesh as M

BAR, FLOOR = 4.0, 1e-6
SPHERE_R, TORUS_R, TORUS_r = 0.7031, 0.6, 0.2517
N_ANALYTIC = 33


def _case(volume, level=0.0, lo=None, hi=None, center=None, radius=None):
    return SimpleNamespace(volume=np.ascontiguousarray(volume, dtype=np.float32), level=level, lo=lo, hi=hi, center=center, radius=radius)


def _noise(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape)


def _axes(n, lo, hi):
    return np.meshgrid(*[np.linspace(lo[a], hi[a], n) for a in range(3)], indexing="ij")


def sphere_volume(n=N_ANALYTIC, r=SPHERE_R, c=(0.013, -0.021, 0.007), lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    X, Y, Z = _axes(n, lo, hi)
    return np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r


def torus_volume(n=N_ANALYTIC, R=TORUS_R, r=TORUS_r, c=(0.013, -0.021, 0.007)):
    X, Y, Z = _axes(n, (-1.0,) * 3, (1.0,) * 3)
    return np.sqrt((np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - R) ** 2 + (Z - c[2]) ** 2) - r


def _nonfinite():
    v = _noise((6, 6, 6), 11)
    v[2, 3, 1], v[4, 1, 4] = np.nan, np.inf
    return _case(v)


def _at_level():
    return _case(np.random.default_rng(12).integers(-1, 2, size=(7, 6, 5)).astype(np.float32))      # -1, 0, 1: a third of the corners at the level


BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
WIDE = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
CENTER, RADIUS = (0.1, -0.05, 0.15), 2.0

CASES = {
    "one_cell": lambda: _case(_noise((2, 2, 2), 1)),
    "cube_3": lambda: _case(_noise((3, 3, 3), 2)),
    "axes_5x4x3": lambda: _case(_noise((5, 4, 3), 3), lo=(-1.0, 0.5, 2.0), hi=(1.0, 1.25, 2.5)),
    "row_3x3x130": lambda: _case(_noise((3, 3, 130), 4)),
    "row_65x3x3": lambda: _case(_noise((65, 3, 3), 5)),
    "row_3x70x3": lambda: _case(_noise((3, 70, 3), 6)),
    "noise_40": lambda: _case(_noise((40, 40, 40), 7)),
    "flat_1x5x6": lambda: _case(_noise((1, 5, 6), 8)),
    "flat_5x6x1": lambda: _case(_noise((5, 6, 1), 9)),
    "all_above": lambda: _case(np.ones((4, 5, 6))),
    "all_at_level": lambda: _case(np.zeros((4, 5, 6))),
    "level_0.25": lambda: _case(_noise((6, 5, 7), 10), level=0.25),
    "corners_at_level": _at_level,
    "nan_and_inf": _nonfinite,
    "sphere": lambda: _case(sphere_volume(), lo=BOX[0], hi=BOX[1]),
    "sphere_index_space": lambda: _case(sphere_volume()),
    "sphere_uncontracted": lambda: _case(sphere_volume(), lo=BOX[0], hi=BOX[1], center=CENTER, radius=RADIUS),
    # the surface |y - (0.2, 0, 0)| = 1 runs from |y| = 0.8 to |y| = 1.2: both branches of the un-contraction
    "sphere_across_the_unit_ball": lambda: _case(sphere_volume(r=1.0, c=(0.2, 0.0, 0.0), lo=WIDE[0], hi=WIDE[1]), lo=WIDE[0], hi=WIDE[1], center=CENTER,
                                                 radius=RADIUS),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def run_checker(c, dtype=np.float64, volume=None, level=None):
    return M.marching_cubes_numpy(c.volume if volume is None else volume, c.level if level is None else level, c.lo, c.hi, c.center, c.radius, dtype)


def expectation(c):
    v64, f64 = run_checker(c)
    v32, f32 = run_checker(c, np.float32)
    assert np.array_equal(f64, f32) and v32.shape == v64.shape and v32.dtype == np.float32      # the twin takes the same decisions
    dev32 = float(np.abs(v32.astype(np.float64) - v64).max()) if len(v64) else 0.0
    scale = float(np.abs(v64).max()) if len(v64) else 1.0
    return SimpleNamespace(vertices=v64, faces=f64, dev32=dev32, scale=scale, bound=BAR * max(dev32, FLOOR * scale))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The expectation of a case, computed once and shared; left unchanged by everyone."""
    return expectation(case(name))


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def compare(vertices, faces, want, what=""):
    """THE BAR of the module docstring: a mesh (tensors or arrays) against `want` (`expected(name)`).  Prints every figure before it
    asserts.  -> (deviation, bound)."""
    vertices, faces = _host(vertices), _host(faces)
    print(f"{what}: Nv {vertices.shape[0]} (checker {want.vertices.shape[0]}), Nf {faces.shape[0]} (checker {want.faces.shape[0]})")
    assert vertices.ndim == 2 and vertices.shape[1] == 3 and faces.ndim == 2 and faces.shape[1] == 3, f"{what}: shapes"
    assert vertices.shape[0] == want.vertices.shape[0], f"{what}: {vertices.shape[0]} vertices, the checker has {want.vertices.shape[0]}"
    assert faces.shape[0] == want.faces.shape[0], f"{what}: {faces.shape[0]} faces, the checker has {want.faces.shape[0]}"
    assert faces.dtype == np.int32 and np.array_equal(faces, want.faces), f"{what}: faces differ from the float64 checker's"
    assert np.isfinite(vertices).all() == np.isfinite(want.vertices).all() and np.array_equal(np.isfinite(vertices), np.isfinite(want.vertices)), \
        f"{what}: non-finite at other vertices than the float64 checker"
    ok = np.isfinite(want.vertices)
    dev = float(np.abs(vertices.astype(np.float64) - want.vertices)[ok].max()) if ok.any() else 0.0
    print(f"{what}: vertices off by {dev:.3e}; float32 checker {want.dev32:.3e}, scale {want.scale:.3e}, bound {want.bound:.3e}")
    assert dev <= want.bound, f"{what}: vertices off by {dev:.3e}, beyond {want.bound:.3e}"
    return dev, want.bound


# ---- measures of a mesh ----------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_counts(faces):
    """-> (undirected edges [E,2], how often each occurs, the largest |count(u -> v) - count(v -> u)|)."""
    d = directed_edges(faces)
    if not len(d):
        return np.zeros((0, 2), dtype=np.int64), np.zeros((0,), dtype=np.int64), 0
    und, inverse, counts = np.unique(np.sort(d, axis=1), axis=0, return_inverse=True, return_counts=True)
    signed = np.bincount(inverse.reshape(-1), weights=np.where(d[:, 0] < d[:, 1], 1.0, -1.0), minlength=len(und))
    return und, counts, int(np.abs(signed).max())


def euler(vertices, faces):
    return len(vertices) - len(edge_counts(faces)[0]) + len(faces)


def signed_volume(vertices, faces):
    """Positive when the normals (right-hand rule) point out of the enclosed region."""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def trilinear(volume, points):
    """The trilinear interpolant of `volume` (index space) at `points` [n,3], float64."""
    vol = np.asarray(volume, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)
    i0 = np.clip(np.floor(p).astype(np.int64), 0, np.array(vol.shape) - 2)
    f = p - i0
    out = np.zeros(len(p))
    for c in range(8):
        o = np.array([c & 1, (c >> 1) & 1, c >> 2])
        w = np.prod(np.where(o, f, 1 - f), axis=1)
        out += w * vol[i0[:, 0] + o[0], i0[:, 1] + o[1], i0[:, 2] + o[2]]
    return out


# ---- wrong implementations the bar must reject -----------------------------------------------------------------------------------------
MUTANTS = {"two axes swapped": "sphere", "flipped winding": "sphere", "<= instead of <": "corners_at_level", "un-welded vertices": "sphere"}


def mutant(name):
    """-> (vertices, faces) of a plausible but wrong implementation on case MUTANTS[name]."""
    c = case(MUTANTS[name])
    if name == "two axes swapped":      # the same surface, marched with ix and iy exchanged: another order of vertices and faces
        v, f = run_checker(c, np.float32, volume=c.volume.transpose(1, 0, 2))
        return v[:, [1, 0, 2]], f
    if name == "<= instead of <":      # for float32 values v <= level iff v < the next float32 above level
        return run_checker(c, np.float32, level=np.nextafter(np.float32(c.level), np.float32(np.inf)))
    v, f = run_checker(c, np.float32)
    if name == "flipped winding":
        return v, np.ascontiguousarray(f[:, ::-1])
    if name == "un-welded vertices":
        return v[f.reshape(-1)], np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)
    raise KeyError(name)


# ---- the C-ABI's refusals --------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    """Every refusal of sr_mesh_count / sr_mesh_emit comes before the first HIP call: made here on dummy host pointers, no GPU needed."""
    from streetunveiler_amd import _lib
    INVALID, UNSUPPORTED = -1, -4
    dummy = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(dummy) + 255) & ~255
    dims = lambda *d: (ctypes.c_int32 * 3)(*d)
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    big, nan = 1 << 40, float("nan")
    need = lib.sr_mesh_workspace_bytes(dims(5, 4, 3))
    assert need >= 5 * 60 and lib.sr_mesh_workspace_bytes(dims(1024, 1024, 1024)) >= 5 << 30
    assert lib.sr_mesh_workspace_bytes(None) == 0 and lib.sr_mesh_workspace_bytes(dims(0, 4, 3)) == 0
    assert lib.sr_mesh_workspace_bytes(dims(2048, 1024, 1024)) == 0 and lib.sr_mesh_workspace_bytes(dims(65536, 65536, 65536)) == 0
    count = [((None, dims(5, 4, 3), 0.0, p, big, p, None), INVALID, b"volume is NULL"),
             ((p, None, 0.0, p, big, p, None), INVALID, b"dims is NULL"),
             ((p, dims(5, 0, 3), 0.0, p, big, p, None), INVALID, b"at least one sample"),
             ((p, dims(5, 4, -3), 0.0, p, big, p, None), INVALID, b"at least one sample"),
             ((p, dims(5, 4, 3), nan, p, big, p, None), INVALID, b"level is NaN"),
             ((p, dims(2048, 1024, 1024), 0.0, p, big, p, None), UNSUPPORTED, b"2^31"),
             ((p, dims(65536, 65536, 65536), 0.0, p, big, p, None), UNSUPPORTED, b"2^31"),
             ((p, dims(5, 4, 3), 0.0, None, big, p, None), INVALID, b"workspace is NULL"),
             ((p, dims(5, 4, 3), 0.0, p, need - 1, p, None), INVALID, b"workspace"),
             ((p, dims(5, 4, 3), 0.0, p + 4, big, p, None), INVALID, b"16-B aligned"),
             ((p, dims(5, 4, 3), 0.0, p, big, None, None), INVALID, b"counts is NULL")]
    for args, code, fragment in count:
        rc = lib.sr_mesh_count(*args)
        assert rc == code and fragment in lib.sr_last_error(), (rc, fragment, lib.sr_last_error())
    space = ctypes.byref(_lib.SrTsdfSpace(1.0, 1, f3, 1.0))
    emit = [((None, dims(5, 4, 3), 0.0, f3, f3, None, p, big, 3, 1, p, p, None), INVALID, b"volume is NULL"),
            ((p, dims(5, 4, 3), nan, f3, f3, None, p, big, 3, 1, p, p, None), INVALID, b"level is NaN"),
            ((p, dims(5, 4, 3), 0.0, None, f3, None, p, big, 3, 1, p, p, None), INVALID, b"lo / step"),
            ((p, dims(5, 4, 3), 0.0, f3, None, space, p, big, 3, 1, p, p, None), INVALID, b"lo / step"),
            ((p, dims(5, 4, 3), 0.0, f3, f3, None, p, need - 1, 3, 1, p, p, None), INVALID, b"workspace"),
            ((p, dims(5, 4, 3), 0.0, f3, f3, None, p, big, -1, 1, p, p, None), INVALID, b"negative"),
            ((p, dims(5, 4, 3), 0.0, f3, f3, None, p, big, 3, -1, p, p, None), INVALID, b"negative"),
            ((p, dims(5, 4, 3), 0.0, f3, f3, None, p, big, 3, (1 << 31) // 3 + 1, p, p, None), UNSUPPORTED, b"int32"),
            ((p, dims(5, 4, 3), 0.0, f3, f3, None, p, big, 0, 1, p, p, None), INVALID, b"without vertices"),
            ((p, dims(5, 4, 3), 0.0, f3, f3, None, p, big, 3, 1, None, p, None), INVALID, b"vertices is NULL"),
            ((p, dims(5, 4, 3), 0.0, f3, f3, space, p, big, 3, 1, p, None, None), INVALID, b"faces is NULL"),
            ((p, dims(2048, 2048, 512), 0.0, f3, f3, None, p, big, 3, 1, p, p, None), UNSUPPORTED, b"2^31")]
    for args, code, fragment in emit:
        rc = lib.sr_mesh_emit(*args)
        assert rc == code and fragment in lib.sr_last_error(), (rc, fragment, lib.sr_last_error())
    # nothing to emit is no error and no work: an empty mesh, and a grid without cells
    assert lib.sr_mesh_emit(p, dims(5, 4, 3), 0.0, f3, f3, None, p, big, 0, 0, None, None, None) == 0
    assert lib.sr_mesh_emit(p, dims(5, 1, 3), 0.0, f3, f3, None, p, big, 0, 0, None, None, None) == 0

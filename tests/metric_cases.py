"""The cases of the Euclidean distance transform and of the surface metrics, and what they must give, stated in plain
NumPy / SciPy: brute force over the seeds with exactly the association the library promises, erosion from scipy.ndimage.  Shared by
the CPU tier (test_metric_cases_host.py), the GPU tier (test_gpu_metrics.py) and tools/gen_metric_golden.py."""
import functools

import numpy as np
from scipy import ndimage

LONG_LINE = 512   # MGC_EDT_PANEL_LINE (medpy_amd/csrc/mgc_edt.h): longer lines along the first two axes leave the panel path

# the smallest shapes at which each mechanism can go wrong: one tile; partial tiles on every axis; many tiles and segments over 64
# along the first and the last axis; axes of extent 1 that exist; 2-D; 1-D
SHAPES = [(8, 8, 8), (9, 17, 20), (70, 9, 17), (17, 9, 70), (1, 13, 31), (7, 1, 9), (33, 70), (100,)]
# one long axis each: the first two take the long-line path (out4 says so), the last axis never does -- its rows go by segments
LONG_SHAPES = [(LONG_LINE + 1, 1, 3), (1, LONG_LINE + 1, 3), (1, 3, LONG_LINE + 1)]
SPACINGS = [None, (2.5, 0.7, 0.7), (1.0, 0.4296875, 0.4296875), (3.3, 1.1, 0.9)]
EDT_RTOL = 8 * 2.0 ** -52      # two evaluation orders of a candidate: five roundings each, 10 * 2^-53, the next power of two
METRIC_RTOL = 32 * 2.0 ** -52  # 5 from the inputs and the root, 2 * log2(n) * 2^-53 per mean with n <= 4096: under 18, the next power of two


def spacing_for(spacing, ndim):
    return None if spacing is None else tuple(spacing[:ndim])


# ---- patterns: uint8 planes, not zero = seed / object ------------------------------------------------------------------------------
def corner(shape):
    m = np.zeros(shape, np.uint8)
    m[(0,) * len(shape)] = 1
    return m


def far_tile(shape):
    """seeds only in the last tile of the volume"""
    m = np.zeros(shape, np.uint8)
    m[tuple(slice(((n - 1) // 8) * 8, n) for n in shape)] = 1
    return m


def tie(shape):
    """two seeds at the ends of the longest axis: the voxels between them have two nearest seeds"""
    m = np.zeros(shape, np.uint8)
    ax = int(np.argmax(shape))
    lo, hi = [0] * len(shape), [0] * len(shape)
    hi[ax] = shape[ax] - 1
    m[tuple(lo)] = m[tuple(hi)] = 1
    return m


def ones(shape):
    return np.ones(shape, np.uint8)


def zeros(shape):
    return np.zeros(shape, np.uint8)


def checkerboard(shape):
    return (np.indices(shape).sum(axis=0) % 2).astype(np.uint8)


def shell(shape):
    """a hollow box one voxel inside the volume (where the volume has the room)"""
    m = np.zeros(shape, np.uint8)
    outer = tuple(slice(1, n - 1) if n > 2 else slice(0, n) for n in shape)
    inner = tuple(slice(2, n - 2) if n > 4 else slice(0, 0) for n in shape)
    m[outer] = 1
    m[inner] = 0
    return m


def box(shape):
    """a solid box that touches the border of the volume at index 0 of every axis"""
    m = np.zeros(shape, np.uint8)
    m[tuple(slice(0, n // 2 + 1) for n in shape)] = 1
    return m


def bernoulli(p, seed, value=1):
    def f(shape):
        return ((np.random.default_rng(seed).random(shape) < p) * value).astype(np.uint8)
    f.__name__ = "bernoulli_%g" % p
    return f


PATTERNS = {"corner": (corner, 0), "far_tile": (far_tile, 0), "tie": (tie, 0), "ones": (ones, 0), "zeros": (zeros, 0), "checkerboard": (checkerboard, 0),
            "shell": (shell, 0), "box": (box, 0), "bernoulli_0.002": (bernoulli(0.002, 5), 5), "bernoulli_0.3": (bernoulli(0.3, 7, 201), 7)}
CASES = [(name, shape) for shape in SHAPES for name in PATTERNS]
LONG_CASES = [(name, shape) for shape in LONG_SHAPES for name in ("corner", "bernoulli_0.002", "bernoulli_0.3")]


def case_id(case):
    return "%s-%s" % (case[0], "x".join(map(str, case[1])))


def plane_of(case):
    return PATTERNS[case[0]][0](case[1])


def partner(shape):
    """the second object of the surface cases: a box in the far half of the volume and a few specks"""
    m = np.zeros(shape, np.uint8)
    m[tuple(slice(n // 3, n) for n in shape)] = 1
    m |= (np.random.default_rng(23).random(shape) < 0.05).astype(np.uint8)
    m[(0,) * len(shape)] = 0
    return m


# ---- what the library must give -------------------------------------------------------------------------------------------------------
def _table(n, s):
    """T[v, j] = fl(fl(s * (v - j))^2)"""
    a = np.float64(s) * (np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.float64)
    return a * a


def _key(a):
    a = np.ascontiguousarray(a)
    return a.shape, a.dtype.str, a.tobytes()


@functools.lru_cache(maxsize=None)
def _edt_sq(key, side, spacing):
    shape, dtype, raw = key
    nd = len(shape)
    shape3 = (1,) * (3 - nd) + shape
    sp = (1.0,) * (3 - nd) + (tuple(spacing) if spacing is not None else (1.0,) * nd)
    seeds = (np.frombuffer(raw, dtype=dtype).reshape(shape3) != 0) == bool(side)
    out = np.full(shape3, np.inf)
    tz, ty, tx = (_table(n, s) for n, s in zip(shape3, sp))
    # every seed is a candidate of every voxel; the seeds of a row go together
    for sz, sy in zip(*np.nonzero(seeds.any(axis=2))):
        xs = np.flatnonzero(seeds[sz, sy])
        c = tx[:, xs][None, :, :] + ty[:, sy][:, None, None]      # fl(fl(a_x^2) + fl(a_y^2)): (dy, dx, seeds of the row)
        c = c[None] + tz[:, sz][:, None, None, None]              # fl(. + fl(a_z^2)): (dz, dy, dx, seeds of the row)
        np.minimum(out, c.min(axis=3), out=out)
    out = out.reshape(shape)
    out.setflags(write=False)
    return out


def expected_edt_sq(plane, side, spacing=None):
    """min over the seeds s (the voxels of plane whose being non-zero equals side) of fl(fl(fl(a_x^2) + fl(a_y^2)) + fl(a_z^2)),
    a_k = fl(spacing_k * (v_k - s_k)), x the last axis: every candidate of every voxel is evaluated.  +inf without a seed.
    Read-only and cached: one array serves every test that asks for it."""
    plane = np.asarray(plane)
    return _edt_sq(_key(plane), int(bool(side)), None if spacing is None else tuple(float(s) for s in spacing))


def border(obj, connectivity):
    obj = np.asarray(obj) != 0
    return obj ^ ndimage.binary_erosion(obj, structure=ndimage.generate_binary_structure(obj.ndim, connectivity), iterations=1)


def expected_surface_sq(a, b, connectivity, spacing=None):
    """the squared distances from the border voxels of a to the nearest border voxel of b, in ascending voxel id; the arrays have the
    handle's dimensions: (1, Y, X) is a 3-D volume whose voxels all have neighbours outside, along the first axis"""
    ra, rb = border(a, connectivity), border(b, connectivity)
    if not ra.any() or not rb.any():
        return np.empty(0), int(ra.sum()), int(rb.sum())
    return expected_edt_sq(rb.astype(np.uint8), 1, spacing)[ra], int(ra.sum()), int(rb.sum())


def expected_counts(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return [int(np.count_nonzero(a & b)), int(np.count_nonzero(a & ~b)), int(np.count_nonzero(~a & b)), int(np.count_nonzero(~a & ~b))]


# ---- the metrics on the host, as the reference computes them from the surface lists and the counts ---------------------------------------
def host_surface(a, b, spacing, connectivity):
    return np.sqrt(expected_surface_sq(a, b, connectivity, spacing)[0])


def host_metrics(a, b, spacing, connectivity):
    s1, s2 = host_surface(a, b, spacing, connectivity), host_surface(b, a, spacing, connectivity)
    return {"hd": float(max(s1.max(), s2.max())), "hd95": float(np.percentile(np.hstack((s1, s2)), 95)), "asd": float(s1.mean()),
            "assd": float(np.concatenate([s1, s2]).mean())}


COUNT_METRICS = ("dc", "jc", "precision", "recall", "sensitivity", "specificity", "true_negative_rate", "true_positive_rate", "positive_predictive_value", "ravd")
SURFACE_METRICS = ("hd", "hd95", "asd", "assd")


def golden_cases():
    """(pattern name, shape) of the golden file: every case whose first object is not empty, against partner(shape)"""
    return [c for c in CASES if plane_of(c).any()]


def connectivities(shape):
    return list(range(1, len(shape) + 1))


def golden_key(case, spacing, connectivity):
    return "%s|%s|%d" % (case_id(case), "none" if spacing is None else ",".join(repr(float(s)) for s in spacing), connectivity)

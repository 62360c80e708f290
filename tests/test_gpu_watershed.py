"""GPU tier of the seeded watershed: every case of watershed_cases.py through mgc_watershed_image, == the statement;
every minimum-filter case through mgc_local_minima_image, == the reference's recorded mask; every refusal; the pool's accounting;
the Python layer; and the label pipeline end to end: image -> diffusion -> gradient-like map -> minima -> watershed -> region cut."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import watershed_cases as wc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "watershed.npz")
INVALID, UNSUPPORTED = 1, 6


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _shape(shape):
    return (C.c_int64 * len(shape))(*shape)


def c_watershed(image, markers, mask, ndim=None, shape=None, dtype=None, device=0):
    """(rc, labels, out8) of mgc_watershed_image on host arrays"""
    from medpy_amd import _lib
    shape = tuple(image.shape if shape is None else shape)
    labels = np.full(image.shape, -7, np.int32)
    out8 = np.full(8, -7, np.int64)
    rc = _lib.load().mgc_watershed_image(device, len(shape) if ndim is None else ndim, _shape(shape), _lib.ptr(image), wc.DTYPE_ID[image.dtype.name] if dtype is None else dtype,
                                         None if markers is None else _lib.ptr(markers), None if mask is None else _lib.ptr(mask), _lib.ptr(labels), _lib.ptr(out8))
    return rc, labels, out8


def c_minima(image, size, ndim=None, shape=None, dtype=None):
    from medpy_amd import _lib
    shape = tuple(image.shape if shape is None else shape)
    out = np.full(image.shape, 9, np.uint8)
    out4 = np.full(4, -7, np.int64)
    rc = _lib.load().mgc_local_minima_image(0, len(shape) if ndim is None else ndim, _shape(shape), _lib.ptr(image), wc.DTYPE_ID[image.dtype.name] if dtype is None else dtype, size,
                                            _lib.ptr(out), _lib.ptr(out4))
    return rc, out, out4


@pytest.mark.parametrize("name", wc.NAMES)
def test_every_case_equals_the_statement(name):
    from medpy_amd import _lib
    c = wc.BY_NAME[name]
    want = wc.solved(name)[2]
    gc.collect()
    idle = _lib.pool_info()["idle_bytes"]
    rc, labels, out8 = c_watershed(c.image, c.markers, c.mask)
    assert rc == 0, _lib.load().mgc_last_error(None)
    assert np.array_equal(labels, want), "%d voxels differ" % int((labels != want).sum())
    seeds = int(((c.markers > 0) & (True if c.mask is None else c.mask != 0)).sum())
    print(name, "out8", out8.tolist())
    assert out8[0] == seeds and out8[5] == int((want != 0).sum()) and out8[7] == 0
    assert (out8[1] == 0) == (seeds == 0) and out8[2] >= out8[1] and out8[3] >= out8[2] and 1 <= out8[6] <= 33
    if name in wc.SELF_WAKE_FAILS:
        assert out8[4] > 0
    assert _lib.pool_info()["idle_bytes"] == idle                         # every block came from the pool and went back
    note = _lib.load().mgc_last_error(None).decode()
    for word in ("upload_ms=", "flood_ms=", "resolve_ms=", "download_ms="):
        assert word in note, note


def test_a_volume_whose_blocks_the_pool_keeps_gives_all_of_them_back():
    """the blocks of the small cases are below the pool's smallest block; here the planes are pool blocks"""
    from medpy_amd import _lib
    shape = (40, 64, 128)                                                  # 327 680 voxels: the plane of T is 2.5 MiB
    rng = np.random.default_rng(5)
    image = rng.integers(0, 3, shape).astype(np.uint8)
    markers = np.zeros(shape, np.int32)
    markers[3, 5, 7], markers[30, 60, 100] = 1, 2
    gc.collect()
    rc, first, _ = c_watershed(image, markers, None)
    assert rc == 0
    p0 = _lib.pool_info()
    rc, again, out8 = c_watershed(image, markers, None)
    p1 = _lib.pool_info()
    assert rc == 0 and np.array_equal(first, again) and out8[5] == image.size
    assert p1["idle_bytes"] == p0["idle_bytes"] and p1["hits"] > p0["hits"]
    assert set(np.unique(first)) == {1, 2}


@pytest.mark.parametrize("name", [c.name for c in wc.MIN_CASES if c.image.dtype.name in wc.DTYPES])
def test_every_minimum_filter_case_equals_the_reference(golden, name):
    from medpy_amd import _lib
    c = wc.MIN_BY_NAME[name]
    want = wc.golden_mask(golden, name)
    gc.collect()
    idle = _lib.pool_info()["idle_bytes"]
    rc, mask, out4 = c_minima(c.image, c.size)
    assert rc == 0, _lib.load().mgc_last_error(None)
    assert set(np.unique(mask)) <= {0, 1} and np.array_equal(mask != 0, want)
    assert out4.tolist() == [int(want.sum()), 0, 0, 0]
    assert _lib.pool_info()["idle_bytes"] == idle


def test_refusals():
    from medpy_amd import _lib
    last = lambda: _lib.load().mgc_last_error(None).decode()
    img = np.zeros((3, 4, 5), np.uint8)
    mk = np.zeros((3, 4, 5), np.int32)
    gc.collect()
    pool = _lib.pool_info()
    for nd in (0, 4, -1):
        assert c_watershed(img, mk, None, ndim=nd)[0] == INVALID and "ndim" in last()
        assert c_minima(img, 2, ndim=nd)[0] == INVALID and "ndim" in last()
    for shape in ((3, 0, 5), (3, 4, -1)):
        assert c_watershed(img, mk, None, shape=shape)[0] == INVALID and "extent" in last()
        assert c_minima(img, 2, shape=shape)[0] == INVALID
    lib = _lib.load()
    out = np.zeros(img.shape, np.int32)
    m8 = np.zeros(img.shape, np.uint8)
    assert lib.mgc_watershed_image(0, 3, _shape(img.shape), None, 0, _lib.ptr(mk), None, _lib.ptr(out), None) == INVALID and "image NULL" in last()
    assert lib.mgc_watershed_image(0, 3, None, _lib.ptr(img), 0, _lib.ptr(mk), None, _lib.ptr(out), None) == INVALID and "shape NULL" in last()
    assert lib.mgc_watershed_image(0, 3, _shape(img.shape), _lib.ptr(img), 0, None, None, _lib.ptr(out), None) == INVALID and "markers NULL" in last()
    assert lib.mgc_watershed_image(0, 3, _shape(img.shape), _lib.ptr(img), 0, _lib.ptr(mk), None, None, None) == INVALID and "labels_out NULL" in last()
    assert lib.mgc_local_minima_image(0, 3, _shape(img.shape), None, 0, 2, _lib.ptr(m8), None) == INVALID
    assert lib.mgc_local_minima_image(0, 3, _shape(img.shape), _lib.ptr(img), 0, 2, None, None) == INVALID and "mask_out NULL" in last()
    assert c_watershed(img, mk, None, dtype=10)[0] == INVALID and c_watershed(img, mk, None, dtype=-1)[0] == INVALID
    bad = mk.copy()
    bad[2, 3, 4] = -1
    assert c_watershed(img, bad, None)[0] == INVALID and "markers[59]" in last()
    for size in (0, -3):
        assert c_minima(img, size)[0] == INVALID and "size" in last()
    for v in (np.nan, np.inf, -np.inf):
        f = np.zeros((3, 4, 5), np.float32)
        f[1, 0, 2] = v
        assert c_watershed(f, mk, None)[0] == INVALID and "image[22] is not finite" in last()
        assert c_minima(f, 2)[0] == INVALID and "not finite" in last()
    for dt in (6, 7, 9):
        assert c_watershed(np.zeros((3, 4, 5), np.float64), mk, None, dtype=dt)[0] == UNSUPPORTED and "64-bit" in last()
        assert c_minima(np.zeros((3, 4, 5), np.float64), 2, dtype=dt)[0] == UNSUPPORTED
    # 2^32 - 1 voxels or more: refused from the shape alone, before anything is read or allocated
    for shape in ((2 ** 32 - 1,), (2 ** 16, 2 ** 16), (1625, 1625, 1627), (2 ** 40, 2 ** 40, 2 ** 40)):
        assert c_watershed(img, mk, None, shape=shape)[0] == UNSUPPORTED and "2^32 - 1" in last()
        assert c_minima(img, 2, shape=shape)[0] == UNSUPPORTED
    assert c_watershed(img, mk, None, device=99)[0] == INVALID and "device" in last()
    assert _lib.pool_info() == pool                                          # nothing was allocated


def test_python_layer(golden):
    from medpy_amd import filter as flt
    from medpy_amd.filter import image as fi
    for name in ("tiles_ties_masked", "extremes_int8", "float32_zeros_denormals", "dim2_13x18_perm", "dim1_20_ties", "markers_above_255"):
        c = wc.BY_NAME[name]
        want = wc.solved(name)[2]
        got = flt.watershed(c.image, c.markers, None if c.mask is None else c.mask.astype(bool))
        assert got.dtype == np.int32 and np.array_equal(got, want), name
        assert flt.watershed_info()["reached"] == int((want != 0).sum())
        # other marker types; a transposed (non-contiguous) image
        assert np.array_equal(flt.watershed(c.image, c.markers.astype(np.uint16 if c.markers.max() < 2 ** 16 else np.int64), c.mask), want)
    c = wc.BY_NAME["tiles_perm"]
    assert np.array_equal(flt.watershed(c.image.T, c.markers.T), wc.statement(np.ascontiguousarray(c.image.T), np.ascontiguousarray(c.markers.T))[2])
    # float64 and 64-bit integers go through the ranking path: the same regions, because only the order matters
    c = wc.BY_NAME["tiles_ties_masked"]
    want = wc.solved(c.name)[2]
    assert np.array_equal(flt.watershed(c.image.astype(np.float64) * 1e-300 - 1e-299, c.markers, c.mask), want)
    assert np.array_equal(flt.watershed(c.image.astype(np.int64) * 2 ** 40 - 2 ** 62, c.markers, c.mask), want)
    assert np.array_equal(flt.watershed(c.image.astype(np.float16), c.markers, c.mask), want)
    assert np.array_equal(flt.watershed(c.image > 1, c.markers, c.mask), wc.statement((c.image > 1).astype(np.uint8), c.markers, c.mask)[2])
    # local_minima: the reference's pair, every dtype, the 64-bit ones ranked
    for mc in wc.MIN_CASES:
        idx, val = flt.local_minima(mc.image, mc.size)
        gi, gv = golden[mc.name + "/indices"], golden[mc.name + "/values"]
        assert np.array_equal(val, gv) and val.dtype == gv.dtype and idx.shape == gi.shape, mc.name
        for v in np.unique(val):
            assert set(map(tuple, idx[val == v])) == set(map(tuple, gi[gv == v])), mc.name
        si, sv = wc.local_minima_statement(mc.image, mc.size)
        assert np.array_equal(idx, si) and np.array_equal(val, sv)             # ours is the stable order
    assert flt.local_minima(np.zeros((4, 4)))[0].shape == (16, 2)             # the reference's default, min_distance = 4
    # minima_markers: the script's steps between the two calls, numbered like scipy.ndimage.label
    import scipy.ndimage as ndi
    rng = np.random.default_rng(11)
    img = rng.integers(0, 5, (9, 17, 20)).astype(np.int16)
    mask = rng.random(img.shape) < 0.8
    for m in (None, mask):
        plane = wc.minima_statement(img, 3)
        if m is not None:
            plane = plane & m
        want, k = ndi.label(plane)
        got = fi.minima_markers(img, 3, m)
        assert got.dtype == np.int32 and np.array_equal(got, want) and got.max() == k


def test_image_to_region_cut_end_to_end():
    """image -> diffusion -> a gradient-like map made in NumPy -> minima_markers -> watershed -> graph_from_labels(...).maxflow(): the
    region image equals the statement's, hence the cut on it is the cut on the statement's regions"""
    from medpy_amd import filter as flt, graphcut
    from medpy_amd.graphcut import energy_label as el
    n = 48
    rng = np.random.default_rng(3)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing="ij")
    ball = ((z - 24) ** 2 + (y - 22) ** 2 + (x - 26) ** 2) < 14 ** 2
    image = (ball * 100.0 + rng.normal(0, 8, (n, n, n))).astype(np.float32)
    smooth = flt.anisotropic_diffusion(image, niter=3, kappa=30, gamma=0.1, option=2)
    g = np.zeros_like(smooth)
    for a in range(3):
        d = np.abs(np.diff(smooth, axis=a))
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, n - 1), slice(1, n)
        g[tuple(lo)] += d
        g[tuple(hi)] += d
    gradient = np.round(g).astype(np.uint16)                                  # whole numbers: plateaus and ties in plenty
    markers = flt.minima_markers(gradient, 4)
    import scipy.ndimage as ndi
    assert np.array_equal(markers, ndi.label(wc.minima_statement(gradient, 4))[0])
    regions = flt.watershed(gradient, markers)
    want = wc.statement(gradient, markers)[2]
    assert np.array_equal(regions, want)
    k = int(markers.max())
    assert k > 50 and regions.min() == 1 and np.array_equal(np.unique(regions), np.arange(1, k + 1))
    fg = np.zeros((n, n, n), bool)
    bg = np.zeros((n, n, n), bool)
    fg[22:27, 20:25, 24:29] = True
    bg[:2] = True
    cut = graphcut.graph_from_labels(regions, fg, bg, boundary_term=el.boundary_difference_of_means, boundary_term_args=smooth)
    ref = graphcut.graph_from_labels(want, fg, bg, boundary_term=el.boundary_difference_of_means, boundary_term_args=smooth)
    flow = cut.maxflow()
    assert flow == ref.maxflow() and flow > 0
    ids = [int(r) - 1 for r in np.unique(regions[fg])] + [int(r) - 1 for r in np.unique(regions[bg])[:20]]
    sides = [cut.what_segment(i) for i in ids]
    assert sides == [ref.what_segment(i) for i in ids] and sides[0] != sides[-1]      # the markers' regions lie on their sides

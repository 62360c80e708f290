"""-m gpu: anisotropic diffusion on the device -- every case of diffusion_cases.py through mgc_diffuse_image and through
mgc_diffuse (the boundary image, then a feature image that takes precedence) against the reference's recorded output: ``==`` for
options 2 and 3, the measured bound for option 1; the result kept on the device as the feature image and read there by the
histogram calls; what a call may not touch; a volume of several bricks with partial ones on every face; every refusal.  The golden
file is read once per module and shared (diffusion_cases.golden)."""
import ctypes as C

import numpy as np
import pytest

import diffusion_cases as dc
import test_gpu_histogram_term as fam

pytestmark = pytest.mark.gpu

SHAPE = (9, 17, 70)   # several bricks along every axis, none of them whole
KAPPA, GAMMA = 20.5, 0.25


def _graph(shape, boundary=None, feature=None):
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph(shape)
    if boundary is not None:
        g._set_boundary("difference_linear", boundary, None, False)
    if feature is not None:
        g._set_feature_image(feature)
    return g


def _noise(shape, dtype=np.uint8, seed=3):
    return np.random.default_rng(seed).integers(0, 200, shape).astype(dtype)


def _bricks(shape):
    s3 = (1,) * (3 - len(shape)) + tuple(shape)
    return -(-s3[0] // dc.BZ) * -(-s3[1] // dc.BY) * -(-s3[2] // dc.BX)


# ---- 1. every case, through both entries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.NAMES)
def test_image_of_the_callers(name):
    from medpy_amd import filter as flt
    case = dc.BY_NAME[name]
    got = flt.anisotropic_diffusion(dc.image(case), case.niter, case.kappa, case.gamma, case.spacing, case.option)
    dc.check(got, case, "mgc_diffuse_image")


@pytest.mark.parametrize("name", dc.NAMES)
def test_image_of_the_handle(name):
    case = dc.BY_NAME[name]
    img = dc.image(case)
    g = _graph(case.shape, boundary=img)   # the boundary image, in the case's dtype
    got = g.anisotropic_diffusion(case.niter, case.kappa, case.gamma, case.spacing, case.option)
    dc.check(got, case, "mgc_diffuse, boundary image")
    assert g.diffusion_info() == {"iterations": case.niter, "bricks": _bricks(case.shape)}
    g.close()
    other = np.full(case.shape, 5, dtype=np.uint16)
    g = _graph(case.shape, boundary=other, feature=img)   # a feature image takes precedence
    dc.check(g.anisotropic_diffusion(case.niter, case.kappa, case.gamma, case.spacing, case.option), case, "mgc_diffuse, feature image")
    g.close()


@pytest.mark.parametrize("option", [2, 3])
def test_a_volume_of_many_bricks_equals_the_statement(option):
    shape = (37, 45, 150)
    img = np.random.default_rng(41).normal(100.0, 40.0, shape).astype(np.float32)
    from medpy_amd import filter as flt
    got = flt.anisotropic_diffusion(img, 4, 30.0, 0.15, (1.0, 0.8, 1.3), option)
    want = dc.statement(img, 4, 30.0, 0.15, (1.0, 0.8, 1.3), option)
    assert got.dtype == np.float32 and np.array_equal(got, want), int((got != want).sum())
    img16 = np.random.default_rng(42).integers(0, 4096, shape).astype(np.uint16)   # x extent no multiple of 4 away: the scalar rows of the first launch
    got = flt.anisotropic_diffusion(img16[:, :, :149], 4, 300.0, 0.15, None, option)
    assert np.array_equal(got, dc.statement(img16[:, :, :149], 4, 300.0, 0.15, None, option))


# ---- 2. keep = 1: the result stays on the device as the feature image -----------------------------------------------------------
@pytest.mark.parametrize("option", [2, 3])
@pytest.mark.parametrize("had_feature", [False, True], ids=["boundary_image", "replaces_a_feature_image"])
def test_keep_makes_the_result_the_feature_image(option, had_feature):
    from medpy_amd.graphcut import histogram as h
    img = _noise(SHAPE, np.uint8)
    fg, bg = fam._markers(SHAPE)
    n = int(np.prod(SHAPE))
    g = _graph(SHAPE, boundary=np.zeros(SHAPE, np.int16) if had_feature else img, feature=img.astype(np.float64) if had_feature else None)
    g._set_markers(fg, bg)
    before = g.stats()["device_bytes"]
    want = dc.statement(img, 3, KAPPA, GAMMA, None, option)
    got = g.anisotropic_diffusion(3, KAPPA, GAMMA, None, option, keep=True)
    assert np.array_equal(got, want)
    assert g.stats()["device_bytes"] - before == 4 * n - (8 * n if had_feature else 0)
    # the histogram calls read the smoothed image where it lies: exact integers
    nbins, lo, width = 32, float(want.min()), float(np.ptp(want)) / 32 + 1e-3
    bins = h.histogram_bins(want, nbins, lo, width)
    for got_h, mask in zip(g.marker_histograms(nbins, lo, width), (fg, bg)):
        assert np.array_equal(got_h, np.bincount(bins[mask], minlength=nbins))
    labels = np.random.default_rng(5).random(SHAPE) < 0.4
    for got_h, mask in zip(g.label_histograms(labels, nbins, lo, width), (labels, ~labels)):
        assert np.array_equal(got_h, np.bincount(bins[mask], minlength=nbins))
    # a later keep = 0 call reads the kept image (two more iterations of it) and leaves it alone
    kept = g.stats()["device_bytes"]
    again = g.anisotropic_diffusion(2, KAPPA, GAMMA, None, option)
    assert np.array_equal(again, dc.statement(want, 2, KAPPA, GAMMA, None, option))
    assert g.stats()["device_bytes"] == kept
    assert np.array_equal(g.marker_histograms(nbins, lo, width)[0], np.bincount(bins[fg], minlength=nbins))
    # keep again without a download: the feature image is replaced by one of the same size
    assert g.anisotropic_diffusion(2, KAPPA, GAMMA, None, option, keep=True, download=False) is None
    assert g.stats()["device_bytes"] == kept
    bins2 = h.histogram_bins(again, nbins, lo, width)
    assert np.array_equal(g.marker_histograms(nbins, lo, width)[1], np.bincount(bins2[bg], minlength=nbins))
    # niter = 0 with keep: the float32 copy of what is there
    assert np.array_equal(g.anisotropic_diffusion(0, KAPPA, GAMMA, None, option, keep=True), again)
    g.close()


def test_a_solved_handle_keeps_its_cut():
    shape = (9, 17, 20)
    img = fam._image(shape, "u8")
    fg, bg = fam._markers(shape)
    g = fam._built(fam._handle(shape, None, fam._nweights(shape, None), fg, bg, feature=img), "as_shipped")
    flow = g.maxflow()
    labels = g.labels().copy()
    stats, launches = g.stats(), g.launch_counts()
    for option in (1, 2, 3):
        got = g.anisotropic_diffusion(2, KAPPA, GAMMA, None, option)   # keep = 0: nothing on the handle changes
        if option != 1:
            assert np.array_equal(got, dc.statement(img, 2, KAPPA, GAMMA, None, option))
    after = g.stats()
    for key in ("device_bytes", "discharge_launches", "relabel_launches", "discharge_tiles", "global_relabels", "phases", "solve_ms", "build_ms"):
        assert after[key] == stats[key], key
    assert g.launch_counts() == launches
    assert np.array_equal(g.labels(), labels) and g.maxflow() == flow
    # keep = 1 on the solved handle: flow and labels stay; the feature image is the smoothed one
    want = dc.statement(img, 2, KAPPA, GAMMA, None, 2)
    g.anisotropic_diffusion(2, KAPPA, GAMMA, None, 2, keep=True, download=False)
    assert np.array_equal(g.labels(), labels) and g.maxflow() == flow
    assert np.array_equal(g.anisotropic_diffusion(0, KAPPA, GAMMA), want)
    g.close()


# ---- 2b. the pool gets every block back -------------------------------------------------------------------------------------------
POOL_SHAPE = (64, 64, 80)   # a float32 image of 1.25 MiB: above the pool's threshold of 1 MiB (MGC_POOL_MIN), so its buffers are pool blocks


def _pool():
    from medpy_amd import _lib
    p = _lib.pool_info()
    return p["idle_bytes"], p["hits"], p["misses"]


def test_keep_0_takes_two_blocks_from_the_pool_and_gives_both_back():
    import gc
    gc.collect()   # no handle some earlier test left to the collector may move the pool between the looks below
    n4 = 4 * int(np.prod(POOL_SHAPE))
    img = _noise(POOL_SHAPE, np.uint8)
    g = _graph(POOL_SHAPE, boundary=img)
    out = g.anisotropic_diffusion(2, KAPPA, GAMMA, None, 2)   # the first call: its two buffers reach the pool when it ends
    idle0, hits0, misses0 = _pool()
    assert idle0 >= 2 * n4
    held = g.stats()["device_bytes"]
    for niter, buffers in ((2, 2), (5, 2), (1, 1), (0, 1)):   # one buffer is enough for at most one iteration
        got = g.anisotropic_diffusion(niter, KAPPA, GAMMA, None, 2)
        idle1, hits1, misses1 = _pool()
        assert idle1 == idle0, (niter, idle1 - idle0)                      # every block is back
        assert hits1 - hits0 == buffers and misses1 == misses0, (niter, hits1 - hits0, misses1 - misses0)   # ... and each came from the pool
        assert g.stats()["device_bytes"] == held
        hits0 = hits1
        if niter == 2:
            assert np.array_equal(got, out)
    g.close()


def test_keep_1_leaves_the_pool_one_block_short_and_a_replaced_image_goes_back():
    import gc
    gc.collect()
    n4 = 4 * int(np.prod(POOL_SHAPE))
    img = _noise(POOL_SHAPE, np.uint8)
    g = _graph(POOL_SHAPE, boundary=img)
    from medpy_amd import filter as flt
    flt.anisotropic_diffusion(_noise(POOL_SHAPE, np.float32), 2, KAPPA, GAMMA, None, 3)   # (three blocks of the size are idle from here on)
    idle0, hits0, misses0 = _pool()
    held = g.stats()["device_bytes"]
    g.anisotropic_diffusion(2, KAPPA, GAMMA, None, 3, keep=True, download=False)
    idle1, hits1, misses1 = _pool()
    assert idle0 - idle1 == n4 and hits1 - hits0 == 2 and misses1 == misses0   # two taken, one back: exactly the result stays out
    assert g.stats()["device_bytes"] - held == n4
    g.anisotropic_diffusion(3, KAPPA, GAMMA, None, 3, keep=True, download=False)   # the kept image is replaced: the old one goes back
    idle2, hits2, misses2 = _pool()
    assert idle2 == idle1 and hits2 - hits1 == 2 and misses2 == misses1
    assert g.stats()["device_bytes"] - held == n4
    g.close()
    assert _pool()[0] >= idle0   # with the handle gone the kept block is idle again (the handle's other blocks of 1 MiB and more too)


def test_the_handle_free_call_gives_all_three_blocks_back():
    import gc
    from medpy_amd import filter as flt
    gc.collect()
    n4 = 4 * int(np.prod(POOL_SHAPE))
    img = _noise(POOL_SHAPE, np.float32)   # float32 input: the input block has the size of the two buffers
    first = flt.anisotropic_diffusion(img, 2, KAPPA, GAMMA, None, 2)
    idle0, hits0, misses0 = _pool()
    assert idle0 >= 3 * n4
    for niter, blocks in ((2, 3), (8, 3), (1, 2), (0, 2)):
        got = flt.anisotropic_diffusion(img, niter, KAPPA, GAMMA, None, 2)
        idle1, hits1, misses1 = _pool()
        assert idle1 == idle0, (niter, idle1 - idle0)
        assert hits1 - hits0 == blocks and misses1 == misses0, (niter, hits1 - hits0, misses1 - misses0)
        hits0 = hits1
        if niter == 2:
            assert np.array_equal(got, first)
    # a refused call takes nothing
    with pytest.raises(ValueError):
        flt.anisotropic_diffusion(img, 2, -1.0, GAMMA)
    assert _pool() == (idle0, hits0, misses0)


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_handle_free_call():
    from medpy_amd import _lib
    lib = _lib.load()
    img = _noise((3, 4, 5), np.uint8)
    out = np.full(img.shape, -7.0, np.float32)
    shp = (C.c_int64 * 3)(3, 4, 5)
    sp = np.array([1.0, 1.0, 1.0])

    def call(ndim=3, shape=shp, image=_lib.ptr(img), dtype=0, niter=1, kappa=50.0, gamma=0.1, spacing=None, option=1, o=_lib.ptr(out)):
        return lib.mgc_diffuse_image(0, ndim, shape, image, dtype, niter, kappa, gamma, spacing, option, o, None)

    bad_shape = (C.c_int64 * 3)(3, 0, 5)
    for kw in ({"ndim": 0}, {"ndim": 4}, {"shape": bad_shape}, {"shape": None}, {"image": None}, {"dtype": 10}, {"dtype": -1}, {"niter": -1}, {"option": 0}, {"option": 4},
               {"kappa": 0.0}, {"kappa": -1.0}, {"kappa": np.inf}, {"kappa": np.nan}, {"gamma": np.nan}, {"gamma": np.inf}, {"o": None},
               {"spacing": _lib.ptr(np.array([1.0, 0.0, 1.0]))}, {"spacing": _lib.ptr(np.array([1.0, np.inf, 1.0]))}, {"spacing": _lib.ptr(np.array([np.nan, 1.0, 1.0]))},
               {"spacing": _lib.ptr(np.array([1.0, 1.0, -2.0]))}):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert lib.mgc_last_error(None), kw
        assert (out == -7.0).all(), kw   # before anything is written
    assert call(spacing=_lib.ptr(sp)) == _lib.OK
    assert np.array_equal(out, dc.statement(img, 1, 50.0, 0.1, None, 1)) or dc.error_measure(out, dc.statement(img, 1, 50.0, 0.1, None, 1)) <= dc.E1_BOUND
    note = lib.mgc_last_error(None).decode()
    assert "upload_ms=" in note and "iterate_ms=" in note and "download_ms=" in note
    out4 = np.zeros(4, np.int64)
    assert lib.mgc_diffuse_image(0, 3, shp, _lib.ptr(img), 0, 5, 50.0, 0.1, None, 2, _lib.ptr(out), _lib.ptr(out4)) == _lib.OK
    assert out4.tolist() == [5, 1, 0, 0]


def test_refusals_on_a_handle_leave_it_as_it_was():
    from medpy_amd import _lib
    lib = _lib.load()
    shape = (5, 6, 7)
    img = _noise(shape, np.int16)
    g = _graph(shape)
    out = np.full(shape, -7.0, np.float32)
    o = _lib.ptr(out)
    assert lib.mgc_diffuse(g._h, 1, 50.0, 0.1, None, 1, 0, o, None) == _lib.ERR_STATE   # no image at all
    assert b"no feature image" in lib.mgc_last_error(g._h)
    assert lib.mgc_diffuse(None, 1, 50.0, 0.1, None, 1, 0, o, None) == _lib.ERR_INVALID
    g._set_boundary("difference_linear", img, None, False)
    fg, bg = fam._markers(shape)
    g._set_markers(fg, bg)
    before = g.stats()
    bad_sp = [_lib.ptr(np.array(v)) for v in ([1.0, 0.0, 1.0], [np.inf, 1.0, 1.0], [1.0, 1.0, np.nan], [-1.0, 1.0, 1.0])]
    calls = [(-1, 50.0, 0.1, None, 1, 0, o), (1, 0.0, 0.1, None, 1, 0, o), (1, -2.0, 0.1, None, 1, 0, o), (1, np.nan, 0.1, None, 1, 0, o), (1, np.inf, 0.1, None, 1, 0, o),
             (1, 50.0, np.nan, None, 1, 0, o), (1, 50.0, -np.inf, None, 1, 0, o), (1, 50.0, 0.1, None, 0, 0, o), (1, 50.0, 0.1, None, 4, 0, o), (1, 50.0, 0.1, None, 1, 2, o),
             (1, 50.0, 0.1, None, 1, -1, o), (1, 50.0, 0.1, None, 1, 0, None)] + [(1, 50.0, 0.1, s, 1, 1, o) for s in bad_sp]
    for args in calls:
        assert lib.mgc_diffuse(g._h, *args, None) == _lib.ERR_INVALID, args
        assert lib.mgc_last_error(g._h), args
    assert (out == -7.0).all() and g.stats()["device_bytes"] == before["device_bytes"]
    # the handle is as it was: the histograms still read the boundary image (a refused keep = 1 installed nothing)
    from medpy_amd.graphcut import histogram as h
    bins = h.histogram_bins(img, 16, -130.0, 20.0)
    assert np.array_equal(g.marker_histograms(16, -130.0, 20.0)[0], np.bincount(bins[fg], minlength=16))
    assert lib.mgc_diffuse(g._h, 1, 50.0, 0.1, None, 2, 1, None, None) == _lib.OK   # out may be NULL with keep = 1
    note = lib.mgc_last_error(g._h).decode()
    assert "upload_ms=" in note and "iterate_ms=" in note and "download_ms=" in note
    g.close()


def test_a_slab_handle_is_refused():
    from medpy_amd import _lib
    lib = _lib.load()
    shp = (C.c_int64 * 3)(32, 8, 8)
    h = C.c_void_p()
    assert lib.mgc_create_slab(3, shp, 6, 0, 0, 2, C.byref(h)) == _lib.OK
    out = np.zeros((32, 8, 8), np.float32)
    try:
        assert lib.mgc_diffuse(h, 1, 50.0, 0.1, None, 1, 0, _lib.ptr(out), None) == _lib.ERR_UNSUPPORTED
        assert b"slab" in lib.mgc_last_error(h)
    finally:
        lib.mgc_destroy(h)


# ---- 4. the Python layer --------------------------------------------------------------------------------------------------------
def test_filter_with_and_without_a_graph():
    from medpy_amd import filter as flt
    from medpy_amd import graphcut
    shape = (6, 9, 70)
    img = _noise(shape, np.uint16, 9)
    want = dc.statement(img, 3, 60.0, 0.2, (1.0, 2.0, 0.5), 3)
    assert np.array_equal(flt.anisotropic_diffusion(img, 3, 60.0, 0.2, (1.0, 2.0, 0.5), 3), want)
    assert np.array_equal(flt.anisotropic_diffusion(img.tolist(), niter=3, kappa=60, gamma=0.2, voxelspacing=[1, 2, 0.5], option=3), dc.statement(
        np.asarray(img.tolist()), 3, 60.0, 0.2, (1.0, 2.0, 0.5), 3))   # anything array-like; int64 goes up as it is
    g = _graph(shape, boundary=img)
    assert np.array_equal(flt.anisotropic_diffusion(None, 3, 60.0, 0.2, (1.0, 2.0, 0.5), 3, graph=g), want)        # the graph's image, where it lies
    assert np.array_equal(flt.anisotropic_diffusion(img[::-1].copy(), 3, 60.0, 0.2, (1.0, 2.0, 0.5), 3, graph=g),
                          dc.statement(img[::-1], 3, 60.0, 0.2, (1.0, 2.0, 0.5), 3))                                  # an image of the caller's, of the graph's shape
    assert g.diffusion_info() == {"iterations": 3, "bricks": 1 * 2 * 2}
    with pytest.raises(ValueError, match="shape"):
        flt.anisotropic_diffusion(img[1:], graph=g)
    g.close()
    # the defaults are the reference's: niter 1, kappa 50, gamma 0.1, option 1
    one = flt.anisotropic_diffusion(img)
    assert dc.error_measure(one, dc.statement(img, 1, 50, 0.1, None, 1)) <= dc.E1_BOUND
    for bad in (np.zeros((2, 2, 2, 2)), np.zeros((1, 2, 2, 2, 2), np.uint8)):
        with pytest.raises(NotImplementedError):
            flt.anisotropic_diffusion(bad)
    # the other graph classes have no lattice image to diffuse
    sg = graphcut.GraphDouble(4, 3)
    for name in ("anisotropic_diffusion", "diffusion_info"):
        with pytest.raises(NotImplementedError, match="voxel lattice"):
            getattr(sg, name)()

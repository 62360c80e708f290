"""-m gpu: the geodesic distance transform and the regional term on top of it -- mgc_geodesic_distance against the
Dijkstra statement of geodesic_cases.py on every case with ``==``, the markers read where they lie, every image dtype, the term
against the dense calls of its two arrays expanded on the host (t-links bit for bit, labels equal, flow to 1e-9), the warm refit
after a stroke against a cold build, and the states, refusals and side effects of the three calls.  Every reference is computed
once per case and module (geodesic_cases caches it) and shared."""
import numpy as np
import pytest

import geodesic_cases as gc
import test_gpu_histogram_term as fam

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in gc.CASES]
TERM_CASES = [((9, 17, 20), None), ((9, 17, 20), 26), ((33, 70), None), ((33, 70), 8)]
TERM_IDS = ["x".join(map(str, s)) + "_n%d" % (c or 2 * len(s)) for s, c in TERM_CASES]
GAMMA, LAM, STEP = 0.37, 3.0, 0.5


def _graph(shape, image=None, conn=None):
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph(shape, connectivity=conn)
    if image is not None:
        g._set_feature_image(image)
    return g


def _spacing(shape):
    return gc.cut_spacing(gc.SPACINGS[1], len(shape))


# ---- 1. the transform ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_distance_on_a_plane_of_the_callers(name):
    case = gc.BY_NAME[name]
    img, seeds = case.inputs()
    want = case.expected()
    g = _graph(case.shape, img if case.gamma != 0 else None)   # (gamma == 0: no image is needed)
    got = g.geodesic_distance(seeds, case.gamma, case.step, case.spacing, case.connectivity)
    info = g.geodesic_info()
    print(name, info)
    assert got.dtype == np.float64 and got.shape == case.shape
    assert np.array_equal(got, want), int((got != want).sum())
    assert info["seeds"] == int(seeds.sum()) and info["finite"] == int(np.isfinite(want).sum())
    assert (info["rounds"] == 0) == (info["seeds"] == 0) and (info["tile_visits"] == 0) == (info["seeds"] == 0)
    assert info["sweeps"] <= gc.SWEEP_CAP * info["tile_visits"]
    if name.startswith("wall_serpentine"):   # longer than the sweep cap: the visit ends there and wakes its own tile
        assert info["capped_visits"] > 0 and info["rounds"] > 1, info
    g.close()


def test_markers_where_they_lie_before_and_after_an_edit():
    shape = (9, 17, 20)
    img = gc.make_image("u8_ties", shape)
    fg, bg = fam._markers(shape)
    sp = _spacing(shape)
    g = fam._built(fam._handle(shape, None, fam._nweights(shape, None), fg, bg, feature=img), "as_shipped")
    for full, conn in ((0, 1), (1, 3)):
        for name, plane in (("fg", fg), ("bg", bg)):
            there = g.geodesic_distance(name, GAMMA, STEP, sp, conn)
            assert there.tobytes() == g.geodesic_distance(plane, GAMMA, STEP, sp, conn).tobytes()
            assert np.array_equal(there, gc.expected_geodesic(img, plane, GAMMA, STEP, sp, full))
    g.maxflow()
    g.edit_markers(fg=np.array([5, 1700, 3059]), bg=np.array([40, 41]), erase=np.flatnonzero(fg.ravel())[:2])
    fg1, bg1 = g.markers()
    assert (fg1 != fg).any() and (bg1 != bg).any()
    for name, plane in (("fg", fg1), ("bg", bg1)):
        there = g.geodesic_distance(name, GAMMA, STEP, sp, 3)
        assert there.tobytes() == g.geodesic_distance(plane, GAMMA, STEP, sp, 3).tobytes()
        assert np.array_equal(there, gc.expected_geodesic(img, plane, GAMMA, STEP, sp, 1))
    g.close()
    # a handle that was never given markers has no seeds
    g = _graph(shape, img)
    for name in ("fg", "bg"):
        assert np.isinf(g.geodesic_distance(name)).all() and g.geodesic_info()["seeds"] == 0 and g.geodesic_info()["rounds"] == 0
    g.close()


@pytest.mark.parametrize("dtype", fam.ALL_DTYPES, ids=[np.dtype(d).name for d in fam.ALL_DTYPES])
def test_every_image_dtype(dtype):
    shape = (9, 17, 20)
    rng = np.random.default_rng(77)
    base = rng.integers(0, 100, shape)
    if np.dtype(dtype).kind == "i":
        base = base - 50
    img = (base * 0.75).astype(dtype) if np.dtype(dtype).kind == "f" else base.astype(dtype)
    seeds = gc.make_seeds("bernoulli_002", shape)
    g = _graph(shape, img)
    for full, conn in ((0, 1), (1, 3)):
        assert np.array_equal(g.geodesic_distance(seeds, 0.37, 1.0, None, conn), gc.expected_geodesic(img, seeds, 0.37, 1.0, None, full))
    g.close()


def test_one_voxel_and_one_row():
    for shape in ((1,), (1, 1, 1), (1, 1, 9), (5, 1, 1), (1, 12)):
        img = gc.make_image("ramp", shape)
        g = _graph(shape, img)
        for kind in ("first", "last", "none", "all"):
            seeds = gc.make_seeds(kind, shape)
            for full, conn in ((0, 1), (1, len(shape))):
                got = g.geodesic_distance(seeds, 1.0, 1.0, None, conn)
                assert np.array_equal(got, gc.expected_geodesic(img, seeds, 1.0, 1.0, None, full)), (shape, kind, full)
        g.close()


# ---- 2. the term ---------------------------------------------------------------------------------------------------------------
def _term_arrays(img, fg, bg, gamma, lam, step, sp, full):
    d_f = gc.expected_geodesic(img, fg, gamma, step, sp, full)
    d_b = gc.expected_geodesic(img, bg, gamma, step, sp, full)
    return gc.expected_term(d_f, d_b, lam)


def _boundary(shape, conn, img):
    """(boundary term, its arguments, the image argument of the geodesic term).  Face neighbourhood: n-link weights of the caller's
    and the image handed to the term (it becomes the feature image); full neighbourhood: a built-in boundary term, whose image the
    geodesic term reads where it lies."""
    from medpy_amd.graphcut import energy_voxel
    if conn in (None, 2 * len(shape)):
        nw = fam._nweights(shape, conn)
        return energy_voxel.boundary_precomputed, ([nw[o] for o in fam._offsets(len(shape), conn)],), img
    return energy_voxel.boundary_difference_linear, (img, False), None


@pytest.mark.parametrize("shape,conn", TERM_CASES, ids=TERM_IDS)
def test_term_equals_the_dense_call_of_its_arrays(shape, conn):
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel
    nd = len(shape)
    full = int(conn not in (None, 2 * nd))
    fg, bg = fam._markers(shape)
    img = fam._image(shape, "u8")
    sp = _spacing(shape)
    bterm, bargs, gimg = _boundary(shape, conn, img)
    s, k = _term_arrays(img, fg, bg, GAMMA, LAM, STEP, sp, full)
    assert (s > 0).any() and (k > 0).any() and (s != k).any()
    a = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_geodesic, regional_term_args=(GAMMA, LAM, STEP, sp, None, gimg),
                                   boundary_term=bterm, boundary_term_args=bargs, connectivity=conn)
    b = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_precomputed, regional_term_args=(s, k),
                                   boundary_term=bterm, boundary_term_args=bargs, connectivity=conn)
    assert a.tweights().tobytes() == b.tweights().tobytes()
    assert a.tweight_edit_info() == b.tweight_edit_info() and a.tweight_edit_info()["dense_calls"] == 1
    flow_b = b.maxflow()
    fam._assert_cut(a, flow_b, b.labels())
    # the explicit connectivity of the term: the other neighbourhood than the graph's own
    other, oconn = 1 - full, (nd if not full else 1)
    s2, k2 = _term_arrays(img, fg, bg, GAMMA, LAM, STEP, sp, other)
    c = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_geodesic, regional_term_args=(GAMMA, LAM, STEP, sp, oconn, gimg),
                                   boundary_term=bterm, boundary_term_args=bargs, connectivity=conn)
    d = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_precomputed, regional_term_args=(s2, k2),
                                   boundary_term=bterm, boundary_term_args=bargs, connectivity=conn)
    assert c.tweights().tobytes() == d.tweights().tobytes()
    for g in (a, b, c, d):
        g.close()


def test_the_store_accumulates_in_call_order():
    shape = (9, 17, 20)
    rng = np.random.default_rng(5)
    nw = fam._nweights(shape, None)
    fg, bg = fam._markers(shape)
    img = fam._image(shape, "i16")
    prob = rng.random(shape)
    before = (rng.normal(0, 1, shape), rng.normal(0, 1, shape))   # negative weights are allowed: the order of the calls shows
    after = (rng.normal(0, 1, shape), rng.normal(0, 1, shape))
    s, k = _term_arrays(img, fg, bg, 1.0, LAM, 1.0, None, 0)
    graphs = []
    for device in (True, False):
        g = fam._handle(shape, None, nw, fg, bg, feature=img)
        g._set_regional(prob, 0.7)
        g._add_tweights(*before)
        if device:
            g._add_tweights_geodesic(1.0, LAM)
        else:
            g._add_tweights(s, k)
        g._add_tweights(*after)
        fam._built(g, "as_shipped")
        graphs.append(g)
    a, b = graphs
    assert a.tweights().tobytes() == b.tweights().tobytes()
    assert a.tweight_edit_info() == b.tweight_edit_info() and a.tweight_edit_info()["dense_calls"] == 3
    flow_b = b.maxflow()
    fam._assert_cut(a, flow_b, b.labels())
    # the warm form is mgc_update_tweights of the arrays: whatever the store held, one dense call is left
    s2, k2 = _term_arrays(img, fg, bg, 0.37, 2.0, 1.0, None, 1)
    a.update_tweights_geodesic(0.37, 2.0, connectivity=3)
    b.update_tweights_dense(s2, k2)
    assert a.tweights().tobytes() == b.tweights().tobytes()
    assert a.tweight_edit_info() == b.tweight_edit_info() and a.tweight_edit_info()["dense_calls"] == 1
    flow_b = b.maxflow()
    fam._assert_cut(a, flow_b, b.labels())
    a.close()
    b.close()


@pytest.mark.parametrize("shape,conn", TERM_CASES[:2], ids=TERM_IDS[:2])
def test_refit_after_a_stroke_equals_a_cold_build(shape, conn):
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel
    nd = len(shape)
    fg, bg = fam._markers(shape)
    img = fam._image(shape, "u8")
    bterm, bargs, gimg = _boundary(shape, conn, img)

    def build(fg_now):
        return graphcut.graph_from_voxels(fg_now, bg, regional_term=energy_voxel.regional_geodesic, regional_term_args=(GAMMA, LAM, STEP, None, None, gimg),
                                          boundary_term=bterm, boundary_term_args=bargs, connectivity=conn)
    g = build(fg)
    g.maxflow()
    labels0 = g.labels().copy()
    stroke = fam._stroke(shape, labels0, fg, bg)
    g.edit_markers(fg=stroke)
    g.refit_regional_geodesic()
    fg1 = fg.copy()
    fg1.ravel()[stroke] = True
    cold = build(fg1)
    assert g.tweights().tobytes() == cold.tweights().tobytes()
    flow_cold = cold.maxflow()
    fam._assert_cut(g, flow_cold, cold.labels())
    labels1 = g.labels()
    assert (labels1 != labels0).any()
    np.testing.assert_array_equal(np.sort(g.changed_labels()), np.flatnonzero((labels1 != labels0).ravel()))
    g.close()
    cold.close()


# ---- 3. states, refusals, side effects -----------------------------------------------------------------------------------------
def _raises(code, call, *names):
    from medpy_amd import _lib
    with pytest.raises(_lib.MedpyHipError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    assert all(n in str(ei.value) for n in names), str(ei.value)


def test_states_refusals_and_no_side_effects():
    from medpy_amd import _lib
    shape = (9, 8, 7)
    nw = fam._nweights(shape, None)
    fg, bg = fam._markers(shape)
    img = fam._image(shape, "f32")
    seeds = gc.make_seeds("bernoulli_30", shape)
    want = gc.expected_geodesic(img, seeds, 1.0, 1.0, None, 1)
    lib = _lib.load()
    out = np.full(seeds.size, -3.0)
    out8 = np.full(8, -3, np.int64)
    P = _lib.ptr(seeds.view(np.uint8))

    def msg(h):
        return lib.mgc_last_error(h).decode()
    # a handle without an image: gamma > 0 is a state error, gamma == 0 runs
    bare = _graph(shape)
    _raises(_lib.ERR_STATE, lambda: bare.geodesic_distance(seeds, gamma=1.0), "mgc_geodesic_distance", "gamma", "no feature image")
    _raises(_lib.ERR_STATE, lambda: bare._add_tweights_geodesic(1.0, 1.0), "mgc_add_tweights_geodesic", "no feature image")
    assert np.array_equal(bare.geodesic_distance(seeds, gamma=0.0, connectivity=3), gc.expected_geodesic(None, seeds, 0.0, 1.0, None, 1))
    bare.close()
    g = fam._handle(shape, None, nw, fg, bg, feature=img)
    # an unbuilt handle will do for the transform; the warm form needs a built one
    assert np.array_equal(g.geodesic_distance(seeds, connectivity=3), want)
    _raises(_lib.ERR_STATE, lambda: g.update_tweights_geodesic(1.0, 1.0), "mgc_update_tweights_geodesic", "before mgc_build")
    g._add_tweights_geodesic(1.0, 2.0)
    fam._built(g, "as_shipped")
    flow0 = g.maxflow()
    labels0 = g.labels().copy()
    tw0 = g.tweights().copy()
    stats0, counts0, info0 = g.stats(), g.launch_counts(), g.tweight_edit_info()
    assert np.array_equal(g.geodesic_distance(seeds, connectivity=3), want)
    assert np.array_equal(g.geodesic_distance("fg", connectivity=1), gc.expected_geodesic(img, fg, 1.0, 1.0, None, 0))
    # refusals of the C calls, each with a sentence, each before anything is written
    H = g._h
    assert lib.mgc_geodesic_distance(None, P, 0, 0, 1.0, 1.0, None, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID
    assert lib.mgc_add_tweights_geodesic(None, 0, 1.0, 1.0, None, 1.0) == _lib.ERR_INVALID
    assert lib.mgc_update_tweights_geodesic(None, 0, 1.0, 1.0, None, 1.0) == _lib.ERR_INVALID
    for source in (-1, 3):
        assert lib.mgc_geodesic_distance(H, P, source, 0, 1.0, 1.0, None, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID
        assert "mgc_geodesic_distance" in msg(H) and "source" in msg(H)
    assert lib.mgc_geodesic_distance(H, None, 0, 0, 1.0, 1.0, None, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID and "seeds NULL" in msg(H)
    for source in (1, 2):
        assert lib.mgc_geodesic_distance(H, P, source, 0, 1.0, 1.0, None, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID and "seeds given" in msg(H)
    calls = (("mgc_geodesic_distance", lambda full, gamma, step, sp, lam: lib.mgc_geodesic_distance(H, P, 0, full, gamma, step, sp, _lib.ptr(out), _lib.ptr(out8))),
             ("mgc_add_tweights_geodesic", lambda full, gamma, step, sp, lam: lib.mgc_add_tweights_geodesic(H, full, gamma, step, sp, lam)),
             ("mgc_update_tweights_geodesic", lambda full, gamma, step, sp, lam: lib.mgc_update_tweights_geodesic(H, full, gamma, step, sp, lam)))
    for name, call in calls:
        for full in (2, -1):
            assert call(full, 1.0, 1.0, None, 1.0) == _lib.ERR_INVALID and name in msg(H) and "full" in msg(H)
        for bad in (-1.0, np.inf, np.nan):
            assert call(0, bad, 1.0, None, 1.0) == _lib.ERR_INVALID and name in msg(H) and "gamma" in msg(H)
            assert call(0, 1.0, bad, None, 1.0) == _lib.ERR_INVALID and name in msg(H) and "step" in msg(H)
            if name != "mgc_geodesic_distance":
                assert call(0, 1.0, 1.0, None, bad) == _lib.ERR_INVALID and name in msg(H) and "lam" in msg(H)
        for at, bad in ((1, (1.0, 0.0, 1.0)), (2, (1.0, 1.0, -1.0)), (0, (np.inf, 1.0, 1.0)), (1, (1.0, np.nan, 1.0))):
            sp = np.asarray(bad, np.float64)
            assert call(0, 1.0, 1.0, _lib.ptr(sp), 1.0) == _lib.ERR_INVALID and name in msg(H) and "spacing[%d]" % at in msg(H)
    assert (out == -3.0).all() and (out8 == -3).all()
    # every output of the transform is optional
    assert lib.mgc_geodesic_distance(H, P, 0, 1, 1.0, 1.0, None, None, None) == _lib.OK
    assert lib.mgc_geodesic_distance(H, P, 0, 1, 1.0, 1.0, None, None, _lib.ptr(out8)) == _lib.OK
    assert out8.tolist()[:1] == [int(seeds.sum())] and out8[5] == seeds.size and out8[6] == 0 and out8[7] == 0
    # nothing on the handle has changed: statistics with device_bytes, launch counts, the store, labels, flow
    assert g.stats() == stats0 and g.launch_counts() == counts0 and g.tweight_edit_info() == info0
    assert g.tweights().tobytes() == tw0.tobytes()
    assert np.array_equal(g.labels(), labels0) and g.maxflow() == flow0
    # a pending edit: the transform reads the edited markers; the snapshot of the edit survives it
    stroke = fam._stroke(shape, labels0, fg, bg)
    g.edit_markers(fg=stroke)
    fg1 = g.markers()[0]
    assert np.array_equal(g.geodesic_distance("fg", connectivity=3), gc.expected_geodesic(img, fg1, 1.0, 1.0, None, 1))
    flow1 = g.maxflow()
    labels1 = g.labels().copy()
    stats1, counts1 = g.stats(), g.launch_counts()
    g.geodesic_distance("bg")
    g.geodesic_distance(seeds, gamma=0.0)
    assert g.stats() == stats1 and g.launch_counts() == counts1
    np.testing.assert_array_equal(np.sort(g.changed_labels()), np.flatnonzero((labels1 != labels0).ravel()))
    assert g.maxflow() == flow1
    np.testing.assert_array_equal(g.labels(), labels1)
    g.close()
    # a float image must be finite: the lowest flat index and the value are named, and nothing is written
    bad_img = img.copy()
    bad_img.ravel()[9] = np.inf
    bad_img.ravel()[5] = np.nan
    g = fam._handle(shape, None, nw, fg, bg, feature=bad_img)
    _raises(_lib.ERR_INVALID, lambda: g.geodesic_distance(seeds), "mgc_geodesic_distance", "image[5] = nan")
    _raises(_lib.ERR_INVALID, lambda: g._add_tweights_geodesic(1.0, 1.0), "mgc_add_tweights_geodesic", "image[5] = nan")
    assert g.tweight_edit_info()["store_held"] == 0
    assert np.array_equal(g.geodesic_distance(seeds, gamma=0.0), gc.expected_geodesic(None, seeds, 0.0, 1.0, None, 0))   # (the image is not read)
    g.close()
    # t-links merged on the host leave no store to add to
    g = fam._handle(shape, None, nw, fg, bg, feature=img)
    g._set_tweights_merged(np.zeros(seeds.size), 0.0)
    _raises(_lib.ERR_STATE, lambda: g._add_tweights_geodesic(1.0, 1.0), "mgc_add_tweights_geodesic", "mgc_set_tweights_merged")
    g.close()


def test_slab_handles_are_refused():
    from medpy_amd import _lib, synthetic
    from medpy_amd.slab import HipSlab
    sph = synthetic.sphere((32, 24, 24))
    lib = _lib.load()
    for rank in range(2):
        sl = HipSlab(sph["image"].shape, rank, 2)
        plane = np.ascontiguousarray(sph["fg"][sl.plane0:sl.plane1]).view(np.uint8)
        assert lib.mgc_geodesic_distance(sl._h, _lib.ptr(plane), 0, 0, 0.0, 1.0, None, None, None) == _lib.ERR_UNSUPPORTED
        assert b"slab" in lib.mgc_last_error(sl._h)
        assert lib.mgc_geodesic_distance(sl._h, None, 1, 0, 0.0, 1.0, None, None, None) == _lib.ERR_UNSUPPORTED
        assert lib.mgc_add_tweights_geodesic(sl._h, 0, 0.0, 1.0, None, 1.0) == _lib.ERR_UNSUPPORTED
        assert b"slab" in lib.mgc_last_error(sl._h)
        assert lib.mgc_update_tweights_geodesic(sl._h, 0, 0.0, 1.0, None, 1.0) == _lib.ERR_UNSUPPORTED
        assert b"slab" in lib.mgc_last_error(sl._h)

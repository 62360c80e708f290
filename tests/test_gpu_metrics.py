"""GPU tier of the Euclidean distance transform and the surface metrics: mgc_distance_transform, mgc_surface_distances and
mgc_overlap_counts against the brute-force statement of metric_cases.py on callers' planes, on the resident cut of small solved graphs
of both neighbourhoods, the long-line path, medpy_amd.metric.binary against numbers recorded from the reference, and the states and
side effects.  == at unit spacing, 8 * 2^-52 relative on squares at the others, 32 * 2^-52 on the metrics (metric_cases.py derives both)."""
import json
import os

import numpy as np
import pytest

import metric_cases as mc
import test_gpu_histogram_term as fam

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_binary.json")


@pytest.fixture(scope="module")
def handles():
    """one unbuilt graph per shape: a caller's plane needs no more than a handle"""
    from medpy_amd.graphcut import VoxelGraph
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = VoxelGraph(shape)
        return made[shape]
    yield get
    for g in made.values():
        g.close()


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


def _same_squares(got, want, spacing, what):
    assert got.shape == want.shape and got.dtype == np.float64, what
    if spacing is None:
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=what)
        fin = np.isfinite(want)
        err = np.abs(got[fin] - want[fin])
        assert (err <= mc.EDT_RTOL * want[fin]).all(), (what, float(np.max(err / np.where(want[fin] > 0, want[fin], 1))))


# ---- 1. the transform of a caller's plane ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES + mc.LONG_CASES, ids=mc.case_id)
def test_distance_transform_of_a_plane(handles, case):
    g = handles(case[1])
    plane = mc.plane_of(case)
    long_lines = sum(plane.size // n for n in plane.shape[:-1] if n > mc.LONG_LINE)
    if case in mc.LONG_CASES[:-3]:
        assert long_lines == 3                       # (L + 1, 1, 3) and (1, L + 1, 3): three lines of L + 1 voxels
    for spacing in mc.SPACINGS:
        sp = mc.spacing_for(spacing, plane.ndim)
        for side, to in ((1, "foreground"), (0, "background")):
            what = "%s to %s spacing %r" % (mc.case_id(case), to, sp)
            want = mc.expected_edt_sq(plane, side, sp)
            got = g.distance_transform(plane, to=to, spacing=sp, squared=True)
            _same_squares(got, want, sp, what)
            nseeds = int(((plane != 0) == bool(side)).sum())
            assert g.edt_info() == {"seeds": nseeds, "long_lines": long_lines if nseeds else 0}, what
            if nseeds == 0:
                assert np.isposinf(got).all(), what
            else:
                assert (got[(plane != 0) == bool(side)] == 0).all(), what
    # the root is NumPy's; bool planes are the same planes; a scalar spacing counts for every axis
    np.testing.assert_array_equal(g.distance_transform(plane != 0), np.sqrt(mc.expected_edt_sq(plane, 1)))
    _same_squares(g.distance_transform(plane, spacing=0.7, squared=True), mc.expected_edt_sq(plane, 1, (0.7,) * plane.ndim), (0.7,), "scalar spacing")


def test_the_long_line_path_ran(handles):
    """out4 of the C call on the shapes with one long axis: the first two axes leave the panel, the last never does"""
    from medpy_amd import _lib
    lib = _lib.load()
    for shape, want in zip(mc.LONG_SHAPES, (3, 3, 0)):
        g = handles(shape)
        plane = mc.bernoulli(0.3, 7)(shape)
        out = np.empty(plane.size)
        out4 = np.full(4, -1, np.int64)
        assert lib.mgc_distance_transform(g._h, _lib.ptr(plane), 1, None, _lib.ptr(out), _lib.ptr(out4)) == _lib.OK
        assert out4.tolist() == [int((plane != 0).sum()), want, 0, 0]
        np.testing.assert_array_equal(out.reshape(shape), mc.expected_edt_sq(plane, 1))
    # at the threshold itself the panel still takes the line
    shape = (mc.LONG_LINE, 1, 3)
    g = handles(shape)
    plane = mc.corner(shape)
    np.testing.assert_array_equal(g.distance_transform(plane, squared=True), mc.expected_edt_sq(plane, 1))
    assert g.edt_info()["long_lines"] == 0


# ---- 2. the resident cut ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_graph", [False, True], ids=["face_graph", "full_graph"])
@pytest.mark.parametrize("shape", [(9, 17, 20), (8, 8, 8), (33, 70), (1, 13, 31)], ids=lambda s: "x".join(map(str, s)))
def test_resident_cut_equals_the_downloaded_labels(shape, full_graph):
    """t-links of +-1 over n-links of 0: the label is the sign of the t-link, whatever the pattern.  The calls on the labels where they
    lie must give bit for bit what the same calls give on the labels read back."""
    nd = len(shape)
    conn = 3 ** nd - 1 if full_graph else None
    zero = np.zeros(shape)
    g = fam._handle(shape, conn, {o: (zero, zero) for o in fam._offsets(nd, conn)})
    truth = mc.partner(shape)
    built = False
    for name in ("bernoulli_0.3", "shell", "corner"):
        mask = mc.plane_of((name, shape)) != 0
        src, snk = mask.astype(np.float64), (~mask).astype(np.float64)
        if built:
            g.update_tweights_dense(src, snk)
        else:
            g._add_tweights(src, snk)
            g._build()
            built = True
        g.maxflow()
        labels = g.labels().copy()
        np.testing.assert_array_equal(labels, mask)
        sp = mc.spacing_for(mc.SPACINGS[3], nd)
        for to in ("foreground", "background"):
            for s in (None, sp):
                res = g.distance_transform(to=to, spacing=s, squared=True)
                assert res.tobytes() == g.distance_transform(labels, to=to, spacing=s, squared=True).tobytes()
                _same_squares(res, mc.expected_edt_sq(mask.astype(np.uint8), int(to == "foreground"), s), s, name)
        for c in mc.connectivities(shape):
            assert g.surface_distances(truth, voxelspacing=sp, connectivity=c).tobytes() == g.surface_distances(truth, labels, sp, c).tobytes()
        assert g.overlap_counts(truth) == g.overlap_counts(truth, labels) == tuple(mc.expected_counts(mask, truth))
    g.close()


# ---- 3. surface distances and counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_surface_distances_and_counts(handles, case):
    from medpy_amd import _lib
    g = handles(case[1])
    lib = _lib.load()
    a, b = mc.plane_of(case), mc.partner(case[1])
    assert g.overlap_counts(b, a) == tuple(mc.expected_counts(a, b))
    assert g.overlap_counts(a != 0, b != 0) == tuple(mc.expected_counts(b, a))
    for conn in mc.connectivities(case[1]):
        for spacing in mc.SPACINGS:
            sp = mc.spacing_for(spacing, a.ndim)
            spa = None if sp is None else np.asarray(sp, np.float64)
            for p, q in ((a, b), (b, a)):
                want, na, nb = mc.expected_surface_sq(p, q, conn, sp)
                n = want.size
                for cap in sorted({n + 3, max(n // 2, 1), 0}, reverse=True):   # room for all; cap smaller than n; nothing at all
                    sds = np.full(cap + 2, -7.0)
                    out8 = np.full(8, -1, np.int64)
                    rc = lib.mgc_surface_distances(g._h, _lib.ptr(p), _lib.ptr(q), conn, None if spa is None else _lib.ptr(spa), cap, _lib.ptr(sds) if cap else None,
                                                   _lib.ptr(out8))
                    assert rc == _lib.OK, lib.mgc_last_error(g._h)
                    assert out8.tolist() == [na, nb, int((p != 0).sum()), int((q != 0).sum()), 0, 0, 0, 0]
                    k = min(n, cap)
                    _same_squares(sds[:k], want[:k], sp, "%s conn %d spacing %r cap %d" % (mc.case_id(case), conn, sp, cap))
                    assert (sds[k:] == -7.0).all()                              # nothing behind the list or the capacity
                if n:   # the method: the list, already square-rooted, past a first capacity that was too small
                    g.SURFACE_LIST = max(n // 2, 1)
                    try:
                        got = g.surface_distances(q, p, sp, conn)
                    finally:
                        del g.SURFACE_LIST
                    assert got.size == n
                    if sp is None:
                        np.testing.assert_array_equal(got, np.sqrt(want))
                    else:
                        assert (np.abs(got - np.sqrt(want)) <= mc.EDT_RTOL * np.sqrt(want)).all()


def test_a_flat_volume_is_not_a_plane(handles):
    """(1, Y, X) on a 3-D handle: every voxel has neighbours outside along the first axis and is border; on a 2-D handle it has an interior"""
    a2, b2 = mc.box((13, 31)), mc.partner((13, 31))
    g2, g3 = handles((13, 31)), handles((1, 13, 31))
    for conn in (1, 2):
        s2, s3 = g2.surface_distances(b2, a2, None, conn), g3.surface_distances(b2[None], a2[None], None, conn)
        assert s3.size == int(a2.sum()) and s2.size < s3.size
        np.testing.assert_array_equal(s2, np.sqrt(mc.expected_surface_sq(a2, b2, conn)[0]))
        np.testing.assert_array_equal(s3, np.sqrt(mc.expected_surface_sq(a2[None], b2[None], conn)[0]))


# ---- 4. medpy_amd.metric.binary ----------------------------------------------------------------------------------------------------------------
def _close(got, want, exact):
    return got == want if exact else abs(got - want) <= mc.METRIC_RTOL * abs(want)


@pytest.mark.parametrize("case", mc.golden_cases(), ids=mc.case_id)
def test_metric_functions_against_the_reference(handles, gold, case):
    from medpy_amd.metric import binary
    g = handles(case[1])
    a, b = mc.plane_of(case), mc.partner(case[1])
    for name in mc.COUNT_METRICS:
        assert getattr(binary, name)(a, b, graph=g) == gold["counts"][mc.case_id(case)][name], name
    for conn in mc.connectivities(case[1]):
        for spacing in mc.SPACINGS:
            sp = mc.spacing_for(spacing, a.ndim)
            want = gold["surface"][mc.golden_key(case, sp, conn)]
            for name in mc.SURFACE_METRICS:
                got = getattr(binary, name)(a, b, sp, conn, graph=g)
                assert _close(float(got), want[name], sp is None), (name, conn, sp, float(got), want[name])


@pytest.mark.parametrize("shape", [(9, 17, 20), (33, 70), (100,)], ids=lambda s: "x".join(map(str, s)))
def test_with_and_without_a_graph_agree_bit_for_bit(handles, gold, shape):
    from medpy_amd.metric import binary
    g = handles(shape)
    a, b = mc.plane_of(("shell", shape)), mc.partner(shape)
    sp = mc.spacing_for(mc.SPACINGS[1], len(shape))
    for name in mc.COUNT_METRICS:
        assert getattr(binary, name)(a, b) == getattr(binary, name)(a, b, graph=g) == gold["counts"][mc.case_id(("shell", shape))][name]
    for name in mc.SURFACE_METRICS:
        for kw in ({}, {"voxelspacing": sp, "connectivity": len(shape)}, {"voxelspacing": 0.7}):
            assert np.float64(getattr(binary, name)(a, b, **kw)).tobytes() == np.float64(getattr(binary, name)(a, b, graph=g, **kw)).tobytes()
    # anything that is not zero is object, whatever the dtype
    assert binary.hd(a.astype(np.float32) * 3.5, b.astype(np.int16) * -2) == binary.hd(a, b, graph=g)


def test_empty_objects_and_bad_arguments(handles):
    from medpy_amd.metric import binary
    shape = (9, 17, 20)
    g = handles(shape)
    a, empty = mc.box(shape), mc.zeros(shape)
    for f in (binary.hd, binary.hd95, binary.asd, binary.assd):
        for kw in ({}, {"graph": g}):
            with pytest.raises(RuntimeError, match="first supplied array does not contain any binary object"):
                f(empty, a, **kw)
            with pytest.raises(RuntimeError, match="second supplied array does not contain any binary object"):
                f(a, empty, **kw)
    with pytest.raises(RuntimeError, match="second supplied array"):
        binary.ravd(a, empty, graph=g)
    assert binary.dc(empty, empty, graph=g) == 1.0 and binary.precision(empty, a, graph=g) == 0.0 and binary.recall(a, empty, graph=g) == 0.0
    with pytest.raises(RuntimeError, match="length"):
        binary.hd(a, a, voxelspacing=(1.0, 2.0), graph=g)
    with pytest.raises(ValueError, match="spacing"):
        binary.hd(a, a, voxelspacing=(1.0, 0.0, 1.0), graph=g)
    with pytest.raises(ValueError, match="shape"):
        binary.hd(a[1:], a[1:], graph=g)
    with pytest.raises(ValueError, match="no graph"):
        binary.dc(None, a)


def test_scoring_the_cut_just_made():
    """hd(None, truth, graph=g): the first object is the graph's current cut, read where it lies"""
    from medpy_amd.metric import binary
    shape = (9, 17, 20)
    zero = np.zeros(shape)
    g = fam._handle(shape, None, {o: (zero, zero) for o in fam._offsets(3, None)})
    mask = mc.shell(shape) != 0
    g._add_tweights(mask.astype(np.float64), (~mask).astype(np.float64))
    g._build()
    g.maxflow()
    truth = mc.partner(shape)
    sp = (3.3, 1.1, 0.9)
    for name in mc.SURFACE_METRICS:
        assert np.float64(getattr(binary, name)(None, truth, sp, 2, graph=g)).tobytes() == np.float64(getattr(binary, name)(mask, truth, sp, 2, graph=g)).tobytes()
    for name in mc.COUNT_METRICS:
        assert getattr(binary, name)(None, truth, graph=g) == getattr(binary, name)(mask, truth)
    g.close()


# ---- 5. states and side effects ---------------------------------------------------------------------------------------------------------------
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
    t = fam._term(img, fg, bg, fam.BINS["f32"])
    plane, truth = mc.bernoulli(0.5, 3)(shape), mc.partner(shape)
    g = fam._handle(shape, None, nw, fg, bg, feature=img)
    g._add_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"])
    calls = ((lambda: g.distance_transform(), "mgc_distance_transform"), (lambda: g.surface_distances(truth), "mgc_surface_distances"),
             (lambda: g.overlap_counts(truth), "mgc_overlap_counts"))

    def on_planes():
        np.testing.assert_array_equal(g.distance_transform(plane, squared=True), mc.expected_edt_sq(plane, 1))
        np.testing.assert_array_equal(g.surface_distances(truth, plane), np.sqrt(mc.expected_surface_sq(plane, truth, 1)[0]))
        assert g.overlap_counts(truth, plane) == tuple(mc.expected_counts(plane, truth))
    # a NULL plane needs a cut; a caller's plane does not
    for call, name in calls:
        _raises(_lib.ERR_STATE, call, name, "before mgc_build")
    on_planes()
    fam._built(g, "as_shipped")
    for call, name in calls:
        _raises(_lib.ERR_STATE, call, name, "before mgc_maxflow")
    on_planes()
    flow0 = g.maxflow()
    labels0 = g.labels().copy()
    stats0, counts0 = g.stats(), g.launch_counts()
    np.testing.assert_array_equal(g.distance_transform(squared=True), mc.expected_edt_sq(labels0.astype(np.uint8), 1))
    np.testing.assert_array_equal(g.surface_distances(truth), np.sqrt(mc.expected_surface_sq(labels0, truth, 1)[0]))
    assert g.overlap_counts(truth) == tuple(mc.expected_counts(labels0, truth))
    on_planes()
    # refusals of the C calls, each with a sentence, each before anything is written
    lib = _lib.load()
    out = np.full(plane.size, -3.0)
    out8 = np.full(8, -3, np.int64)
    P, T = _lib.ptr(plane), _lib.ptr(truth)
    assert lib.mgc_distance_transform(None, P, 1, None, _lib.ptr(out), None) == _lib.ERR_INVALID
    assert lib.mgc_surface_distances(None, P, T, 1, None, 0, None, None) == _lib.ERR_INVALID
    assert lib.mgc_overlap_counts(None, P, T, _lib.ptr(out8)) == _lib.ERR_INVALID
    for side in (2, -1):
        assert lib.mgc_distance_transform(g._h, P, side, None, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID
        assert "mgc_distance_transform" in lib.mgc_last_error(g._h).decode() and "side" in lib.mgc_last_error(g._h).decode()
    for bad in ((1.0, 0.0, 1.0), (1.0, 1.0, -1.0), (np.inf, 1.0, 1.0), (1.0, np.nan, 1.0)):
        sp = np.asarray(bad, np.float64)
        assert lib.mgc_distance_transform(g._h, P, 1, _lib.ptr(sp), _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID
        assert "spacing" in lib.mgc_last_error(g._h).decode()
        assert lib.mgc_surface_distances(g._h, P, T, 1, _lib.ptr(sp), out.size, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID
        assert "mgc_surface_distances" in lib.mgc_last_error(g._h).decode() and "spacing" in lib.mgc_last_error(g._h).decode()
    for conn in (0, 4, -1):
        assert lib.mgc_surface_distances(g._h, P, T, conn, None, out.size, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID
        assert "connectivity" in lib.mgc_last_error(g._h).decode()
    assert lib.mgc_surface_distances(g._h, P, T, 1, None, -1, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID and "capacity" in lib.mgc_last_error(g._h).decode()
    assert lib.mgc_surface_distances(g._h, P, T, 1, None, 5, None, _lib.ptr(out8)) == _lib.ERR_INVALID and "NULL" in lib.mgc_last_error(g._h).decode()
    assert lib.mgc_surface_distances(g._h, P, None, 1, None, 5, _lib.ptr(out), _lib.ptr(out8)) == _lib.ERR_INVALID and "b NULL" in lib.mgc_last_error(g._h).decode()
    assert lib.mgc_overlap_counts(g._h, P, None, _lib.ptr(out8)) == _lib.ERR_INVALID and "b NULL" in lib.mgc_last_error(g._h).decode()
    assert lib.mgc_overlap_counts(g._h, P, T, None) == _lib.ERR_INVALID and "out4" in lib.mgc_last_error(g._h).decode()
    assert (out == -3.0).all() and (out8 == -3).all()
    # every output of the transform is optional; an empty object is no error of the C call
    assert lib.mgc_distance_transform(g._h, P, 1, None, None, None) == _lib.OK
    empty = mc.zeros(shape)
    assert lib.mgc_surface_distances(g._h, _lib.ptr(empty), T, 1, None, out.size, _lib.ptr(out), _lib.ptr(out8)) == _lib.OK
    assert out8.tolist() == [0, int(mc.border(truth, 1).sum()), 0, int(truth.sum()), 0, 0, 0, 0] and (out == -3.0).all()
    assert lib.mgc_surface_distances(g._h, T, _lib.ptr(empty), 1, None, out.size, _lib.ptr(out), _lib.ptr(out8)) == _lib.OK
    assert out8.tolist() == [int(mc.border(truth, 1).sum()), 0, int(truth.sum()), 0, 0, 0, 0, 0] and (out == -3.0).all()
    # nothing on the handle has changed: statistics with device_bytes, launch counts, labels, flow
    assert g.stats() == stats0 and g.launch_counts() == counts0
    assert np.array_equal(g.labels(), labels0) and g.maxflow() == flow0
    # a pending edit: no current cut in between, a caller's plane all the same
    stroke = fam._stroke(shape, labels0, fg, bg)
    g.edit_markers(fg=stroke)
    for call, name in calls:
        _raises(_lib.ERR_STATE, call, name, "before mgc_maxflow")
    on_planes()
    flow1 = g.maxflow()
    labels1 = g.labels().copy()
    assert (labels1 != labels0).any()
    stats1, counts1 = g.stats(), g.launch_counts()
    np.testing.assert_array_equal(g.distance_transform(to="background", squared=True), mc.expected_edt_sq(labels1.astype(np.uint8), 0))
    g.surface_distances(truth, connectivity=3)
    g.overlap_counts(truth)
    # everything is as it was, and the label snapshot of the edit is still there
    assert g.stats() == stats1 and g.launch_counts() == counts1
    np.testing.assert_array_equal(np.sort(g.changed_labels()), np.flatnonzero((labels1 != labels0).ravel()))
    assert g.maxflow() == flow1
    np.testing.assert_array_equal(g.labels(), labels1)
    g.close()


def test_slab_handles_are_refused():
    from medpy_amd import _lib, synthetic
    from medpy_amd.slab import HipSlab
    sph = synthetic.sphere((32, 24, 24))
    lib = _lib.load()
    out4 = np.zeros(4, np.int64)
    for rank in range(2):
        sl = HipSlab(sph["image"].shape, rank, 2)
        plane = np.ascontiguousarray(sph["fg"][sl.plane0:sl.plane1]).view(np.uint8)
        for lab in (None, _lib.ptr(plane)):
            assert lib.mgc_distance_transform(sl._h, lab, 1, None, None, None) == _lib.ERR_UNSUPPORTED
            assert b"slab" in lib.mgc_last_error(sl._h)
            assert lib.mgc_surface_distances(sl._h, lab, _lib.ptr(plane), 1, None, 0, None, None) == _lib.ERR_UNSUPPORTED
            assert b"slab" in lib.mgc_last_error(sl._h)
            assert lib.mgc_overlap_counts(sl._h, lab, _lib.ptr(plane), _lib.ptr(out4)) == _lib.ERR_UNSUPPORTED
            assert b"slab" in lib.mgc_last_error(sl._h)

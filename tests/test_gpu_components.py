"""GPU tier of the connected components and the cleaning rule: mgc_components and mgc_clean_labels through the public
methods against the plain NumPy / SciPy statement of cc_cases.py -- on a caller's plane, on the current cut of graphs whose labels
are known by construction and of ordinary solved graphs, the rule field by field, the states and side effects, 2-D and 1-D graphs,
and the command line.  Exact equality everywhere: there is no tolerance in this feature."""
import os

import numpy as np
import pytest

import cc_cases as cc
import test_gpu_histogram_term as fam

pytestmark = pytest.mark.gpu

FACE_FULL = ("face", "full")


@pytest.fixture(scope="module")
def handles():
    """one unbuilt graph per shape and marker set: a caller's plane needs no more than a handle"""
    from medpy_amd.graphcut import VoxelGraph
    made = {}

    def get(shape, markers):
        key = (shape, markers)
        if key not in made:
            g = VoxelGraph(shape)
            fg, bg = cc.sparse_markers(shape) if markers else (None, None)
            if markers:
                g._set_markers(fg, bg)
            made[key] = (g, fg, bg)
        return made[key]
    yield get
    for g, _, _ in made.values():
        g.close()


def _assert_components(got, mask, side, full, fg, bg, ids=True):
    want_ids, first, size, flags = cc.expected_components(mask, side, full, fg, bg)
    if ids:
        assert got.ids.dtype == np.int32 and got.ids.shape == mask.shape
        np.testing.assert_array_equal(got.ids, want_ids)
    else:
        assert got.ids is None
    for name, want in (("first", first), ("size", size), ("flags", flags)):
        assert getattr(got, name).dtype == want.dtype, name
        np.testing.assert_array_equal(getattr(got, name), want, err_msg=name)
    info = got.info
    assert list(info) == list(cc.INFO_KEYS)
    assert info["components"] == first.size and info["voxels"] == int(size.sum())
    assert info["largest_size"] == (int(size.max()) if size.size else 0)
    assert info["largest_id"] == (int(np.argmax(size)) + 1 if size.size else 0)   # ties: the smaller id
    return info


# ---- 1. a caller's plane --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_components_of_a_plane_equal_scipy(handles, case):
    pattern, shape = case
    mask = pattern(shape)
    ntiles = int(np.prod([(n + 7) // 8 for n in shape]))
    for markers in (False, True):
        g, fg, bg = handles(shape, markers)
        for side in (1, 0):
            for full, name in enumerate(FACE_FULL):
                info = _assert_components(g.components(mask, foreground=bool(side), connectivity=name), mask, side, full, fg, bg)
                assert info["tiles_skipped"] == 0 and info["tiles_processed"] == ntiles   # no label summaries for a caller's plane
    # bool planes are the same planes
    g, fg, bg = handles(shape, True)
    _assert_components(g.components(mask != 0), mask, 1, 0, fg, bg)


@pytest.mark.parametrize("shape", [(17, 16, 31), (40, 33), (70,)], ids=["17x16x31", "40x33", "70"])
def test_counts_only_and_short_tables(handles, shape):
    from medpy_amd import _lib
    g, fg, bg = handles(shape, True)
    mask = cc.bernoulli(0.31)(shape)
    _assert_components(g.components(mask, ids=False), mask, 1, 0, fg, bg, ids=False)
    _assert_components(g.components(mask, foreground=False, connectivity="full", ids=False), mask, 0, 1, fg, bg, ids=False)
    # the first table of components() is too short: it calls once more
    want = cc.expected_components(mask, 1, 0, fg, bg)
    K = want[1].size
    assert K > 5
    g.COMPONENTS_TABLE = 3
    try:
        _assert_components(g.components(mask), mask, 1, 0, fg, bg)
    finally:
        del g.COMPONENTS_TABLE
    # the C call: a capacity below K fills the first rows and reports K; a capacity of 0 takes NULL tables
    lib = _lib.load()
    plane = np.ascontiguousarray(mask)
    for cap in (5, 1, 0):
        first, size = np.full(cap + 2, -7, np.int64), np.full(cap + 2, -7, np.int64)
        flags = np.full(cap + 2, 0xee, np.uint8)
        ids = np.zeros(mask.size, np.int32)
        out8 = np.zeros(8, np.int64)
        rc = lib.mgc_components(g._h, _lib.ptr(plane), 1, 0, _lib.ptr(ids), cap, _lib.ptr(first) if cap else None, _lib.ptr(size) if cap else None,
                                _lib.ptr(flags) if cap else None, _lib.ptr(out8))
        assert rc == _lib.OK and out8[0] == K
        np.testing.assert_array_equal(ids.reshape(shape), want[0])
        np.testing.assert_array_equal(first[:cap], want[1][:cap])
        np.testing.assert_array_equal(size[:cap], want[2][:cap])
        np.testing.assert_array_equal(flags[:cap], want[3][:cap])
        assert (first[cap:] == -7).all() and (size[cap:] == -7).all() and (flags[cap:] == 0xee).all()   # nothing behind the capacity
    assert lib.mgc_components(g._h, _lib.ptr(plane), 1, 0, None, 0, None, None, None, None) == _lib.OK   # every output is optional


# ---- 2. the current cut ---------------------------------------------------------------------------------------------------------------
CUT_SHAPES = cc.SHAPES   # rows of whole runs of eight (label summaries: 8x8x8, 16x8x8, 24x24x24) and rows that are not
CUT_PATTERNS = [p for p in cc.PATTERNS if p is not cc.bytes_plane]   # (a cut's labels are 0 / 1)


@pytest.mark.parametrize("full_graph", [False, True], ids=["face_graph", "full_graph"])
@pytest.mark.parametrize("shape", CUT_SHAPES, ids=["x".join(map(str, s)) for s in CUT_SHAPES])
def test_components_of_a_cut_known_by_construction(shape, full_graph):
    """t-links of +-1 over n-links of 0: the label is the sign of the t-link, whatever the pattern"""
    nd = len(shape)
    conn = 3 ** nd - 1 if full_graph else None
    zero = np.zeros(shape)
    g = fam._handle(shape, conn, {o: (zero, zero) for o in fam._offsets(nd, conn)})
    built = False
    rows8 = shape[-1] % 8 == 0
    for pattern in CUT_PATTERNS:
        mask = pattern(shape)
        if mask is None:
            continue
        src, snk = (mask != 0).astype(np.float64), (mask == 0).astype(np.float64)
        if built:
            g.update_tweights_dense(src, snk)
        else:
            g._add_tweights(src, snk)
            g._build()
            built = True
        g.maxflow()
        np.testing.assert_array_equal(g.labels(), mask != 0)
        for side in (1, 0):
            info = _assert_components(g.components(foreground=bool(side)), mask, side, int(full_graph), None, None)   # the graph's own neighbourhood
            other = _assert_components(g.components(foreground=bool(side), connectivity=FACE_FULL[1 - full_graph]), mask, side, 1 - int(full_graph), None, None)
            for i in (info, other):
                ntiles = int(np.prod([(n + 7) // 8 for n in shape]))
                assert i["tiles_skipped"] + i["tiles_processed"] == ntiles
                if not rows8:
                    assert i["tiles_skipped"] == 0
                elif pattern in (cc.zeros, cc.ones):
                    assert i["tiles_skipped"] == ntiles   # every tile is decided by its label summary
        assert g.clean_labels().tolist() == (mask != 0).tolist()
        assert g.clean_labels(changed_only=True).size == 0
    g.close()


@pytest.mark.parametrize("shape,conn", [((17, 16, 31), None), ((16, 9, 16), None), ((9, 10, 11), 26), ((8, 9, 16), 26)],
                         ids=["17x16x31_n6", "16x9x16_n6_rows8", "9x10x11_n26", "8x9x16_n26_rows8"])
def test_components_of_an_ordinary_cut(shape, conn):
    nw = fam._nweights(shape, conn)
    fg, bg = fam._markers(shape)
    img = fam._image(shape, "f32")
    t = fam._term(img, fg, bg, fam.BINS["f32"], lam=fam._lam(conn))
    g = fam._handle(shape, conn, nw, fg, bg, feature=img)
    g._add_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"])
    fam._built(g, "as_shipped")
    g.maxflow()
    labels = g.labels().copy()
    assert fg.sum() < labels.sum() < labels.size
    for side in (1, 0):
        for full, name in enumerate(FACE_FULL):
            _assert_components(g.components(foreground=bool(side), connectivity=name), labels, side, full, fg, bg)
    _assert_components(g.components(), labels, 1, int(conn == 26), fg, bg)
    for r in (cc.rule(fg_full=int(conn == 26), seeded=1, fill_holes=1), cc.rule(fg_full=int(conn == 26), min_size=3, largest=2)):
        want, changed, info = cc.expected_clean(labels, r, fg, bg)
        kw = dict(min_size=r["min_size"], largest=r["largest"] or None, seeded=bool(r["seeded"]), fill_holes=bool(r["fill_holes"]))
        np.testing.assert_array_equal(g.clean_labels(**kw), want)
        np.testing.assert_array_equal(g.clean_labels(changed_only=True, **kw), changed)
        assert {k: v for k, v in g.clean_info().items() if k != "list_written"} == info
        if changed.size > 1:   # a list capacity of 1 on the current cut: the volume and the cut's labels come down instead, the ids are the same
            g.CLEAN_LIST = 1
            try:
                np.testing.assert_array_equal(g.clean_labels(changed_only=True, **kw), changed)
                assert g.clean_info()["list_written"] == 0
            finally:
                del g.CLEAN_LIST
    np.testing.assert_array_equal(g.labels(), labels)
    g.close()


# ---- 3. the cleaning rule ---------------------------------------------------------------------------------------------------------------
def _clean_cases():
    shape = (24, 24, 24)
    specks = (cc.shells(shape) | cc.bernoulli(0.2)(shape)).astype(np.uint8)
    fg, bg = cc.sparse_markers(shape, p=0.004)
    cavity = np.zeros(shape, np.uint8)
    cavity[10, 12, 12] = 1   # a background marker in the innermost cavity of the shells (distance 10 from the border)
    flat = (cc.shells((40, 33)) | cc.bernoulli(0.2)((40, 33))).astype(np.uint8)
    return [("shells", cc.shells(shape), None, None), ("shells_bg_in_cavity", cc.shells(shape), fg, cavity), ("specks", specks, fg, bg),
            ("specks_bytes", specks * 201, fg, bg), ("specks_2d", flat) + cc.sparse_markers((40, 33), p=0.01), ("line", cc.bernoulli(0.5)((70,)), None, None)]


RULES = [cc.rule(), cc.rule(min_size=4), cc.rule(largest=1), cc.rule(largest=3), cc.rule(largest=10 ** 6), cc.rule(seeded=1), cc.rule(fill_holes=1),
         cc.rule(fill_holes=1, hole_full=1), cc.rule(fg_full=1), cc.rule(fg_full=1, min_size=2, largest=4, seeded=1, fill_holes=1, hole_full=1),
         cc.rule(min_size=3, largest=2, seeded=1, fill_holes=1)]


@pytest.mark.parametrize("case", _clean_cases(), ids=lambda c: c[0])
def test_clean_labels_equals_the_rule_on_the_host(case):
    from medpy_amd.graphcut import VoxelGraph
    _, mask, fg, bg = case
    g = VoxelGraph(mask.shape)
    if fg is not None or bg is not None:
        g._set_markers(fg, bg)
    for r in RULES:
        want, changed, info = cc.expected_clean(mask, r, fg, bg)
        kw = dict(min_size=r["min_size"], largest=r["largest"] or None, seeded=bool(r["seeded"]), fill_holes=bool(r["fill_holes"]),
                  connectivity=FACE_FULL[r["fg_full"]], hole_connectivity=FACE_FULL[r["hole_full"]])
        got = g.clean_labels(mask, **kw)
        assert got.dtype == np.bool_ and got.shape == mask.shape
        np.testing.assert_array_equal(got, want, err_msg=str(r))
        assert g.clean_info() == dict(info, list_written=0), r
        ids = g.clean_labels(mask, changed_only=True, **kw)
        assert ids.dtype == np.int64
        np.testing.assert_array_equal(ids, changed, err_msg=str(r))
        assert g.clean_info() == dict(info, list_written=1), r
        if r == cc.rule():
            assert changed.size == 0 and info["voxels_changed"] == 0   # the identity rule
        # into the caller's array
        out = np.ones(mask.shape, bool)
        assert g.clean_labels(mask, out=out, **kw) is out
        np.testing.assert_array_equal(out, want)
        # a list capacity of 1: the volume comes down instead, the ids are the same
        if changed.size > 1:
            g.CLEAN_LIST = 1
            try:
                np.testing.assert_array_equal(g.clean_labels(mask, changed_only=True, **kw), changed)
                assert g.clean_info() == dict(info, list_written=0)
            finally:
                del g.CLEAN_LIST
    # the defaults: the graph's own neighbourhood for the foreground (face here), face for the holes
    want, _, _ = cc.expected_clean(mask, cc.rule(fill_holes=1), fg, bg)
    np.testing.assert_array_equal(g.clean_labels(mask, fill_holes=True), want)
    g.close()


def test_marker_in_a_cavity_keeps_it_open():
    from medpy_amd.graphcut import VoxelGraph
    shape = (24, 24, 24)
    mask = cc.shells(shape)
    bg = np.zeros(shape, np.uint8)
    bg[10, 12, 12] = 1   # in the innermost cavity: distance 10 from the border
    g = VoxelGraph(shape)
    closed = g.clean_labels(mask, fill_holes=True)
    assert closed[1:-1, 1:-1, 1:-1].all() and not closed[0].any()
    filled = g.clean_info()["cavities_filled"]
    g._set_markers(None, bg)
    kept = g.clean_labels(mask, fill_holes=True)
    assert not kept[10, 12, 12] and g.clean_info()["cavities_filled"] == filled - 1
    g.close()


# ---- 4. states and side effects -------------------------------------------------------------------------------------------------------
def _raises(code, call, *names):
    from medpy_amd import _lib
    with pytest.raises(_lib.MedpyHipError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    assert all(n in str(ei.value) for n in names), str(ei.value)


def test_states_refusals_and_no_side_effects():
    import ctypes
    from medpy_amd import _lib
    shape = (9, 8, 7)
    nw = fam._nweights(shape, None)
    fg, bg = fam._markers(shape)
    img = fam._image(shape, "f32")
    t = fam._term(img, fg, bg, fam.BINS["f32"])
    plane = cc.bernoulli(0.5)(shape)

    def solved_graph():
        g = fam._handle(shape, None, nw, fg, bg, feature=img)
        g._add_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"])
        return g
    g = solved_graph()
    # labels=None needs a cut; a caller's plane does not
    for call, name in ((lambda: g.components(), "mgc_components"), (lambda: g.clean_labels(min_size=2), "mgc_clean_labels")):
        _raises(_lib.ERR_STATE, call, name, "before mgc_build")
    _assert_components(g.components(plane), plane, 1, 0, fg, bg)
    fam._built(g, "as_shipped")
    _raises(_lib.ERR_STATE, lambda: g.components(), "mgc_components", "before mgc_maxflow")
    _raises(_lib.ERR_STATE, lambda: g.clean_labels(), "mgc_clean_labels", "before mgc_maxflow")
    _assert_components(g.components(plane), plane, 1, 0, fg, bg)
    flow0 = g.maxflow()
    labels0 = g.labels().copy()
    stats0, counts0 = g.stats(), g.launch_counts()
    _assert_components(g.components(), labels0, 1, 0, fg, bg)
    _assert_components(g.components(plane, foreground=False, connectivity="full"), plane, 0, 1, fg, bg)
    np.testing.assert_array_equal(g.clean_labels(seeded=True, fill_holes=True), cc.expected_clean(labels0, cc.rule(seeded=1, fill_holes=1), fg, bg)[0])
    g.clean_labels(plane, largest=1, changed_only=True)
    # refusals of the C calls, each with a sentence, each before anything is written
    lib = _lib.load()
    out8 = np.full(8, -3, np.int64)
    table = [np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(4, np.uint8)]
    ptrs = [_lib.ptr(a) for a in table]
    assert lib.mgc_components(None, None, 1, 0, None, 0, None, None, None, None) == _lib.ERR_INVALID
    for side, full, cap, what in ((2, 0, 4, "side"), (-1, 0, 4, "side"), (1, 2, 4, "full"), (1, 0, -1, "capacity")):
        assert lib.mgc_components(g._h, None, side, full, None, cap, *ptrs, _lib.ptr(out8)) == _lib.ERR_INVALID
        msg = lib.mgc_last_error(g._h).decode()
        assert "mgc_components" in msg and what in msg, msg
    assert lib.mgc_components(g._h, None, 1, 0, None, 4, None, ptrs[1], ptrs[2], _lib.ptr(out8)) == _lib.ERR_INVALID
    assert "NULL" in lib.mgc_last_error(g._h).decode()
    assert lib.mgc_clean_labels(None, None, None, None, 0, None, None) == _lib.ERR_INVALID
    assert lib.mgc_clean_labels(g._h, None, None, None, 0, None, _lib.ptr(out8)) == _lib.ERR_INVALID and "rule" in lib.mgc_last_error(g._h).decode()
    for kw, what in (({"min_size": 0}, "min_size"), ({"largest": -1}, "largest"), ({"seeded": 2}, "seeded")):
        r = _lib.CleanRule(0, 0, 0, 0, 1, 0)
        for k, v in kw.items():
            setattr(r, k, v)
        assert lib.mgc_clean_labels(g._h, None, ctypes.byref(r), None, 0, None, _lib.ptr(out8)) == _lib.ERR_INVALID
        msg = lib.mgc_last_error(g._h).decode()
        assert "mgc_clean_labels" in msg and what in msg, msg
    r = _lib.CleanRule(0, 0, 0, 0, 1, 0)
    assert lib.mgc_clean_labels(g._h, None, ctypes.byref(r), None, -1, None, _lib.ptr(out8)) == _lib.ERR_INVALID and "capacity" in lib.mgc_last_error(g._h).decode()
    assert (out8 == -3).all()
    # nothing on the handle has changed: statistics with device_bytes, launch counts, labels, flow
    assert g.stats() == stats0 and g.launch_counts() == counts0
    assert np.array_equal(g.labels(), labels0) and g.maxflow() == flow0
    # a pending edit: no current cut in between, a caller's plane all the same
    stroke = fam._stroke(shape, labels0, fg, bg)
    g.edit_markers(fg=stroke)
    _raises(_lib.ERR_STATE, lambda: g.components(), "mgc_components", "before mgc_maxflow")
    _raises(_lib.ERR_STATE, lambda: g.clean_labels(changed_only=True), "mgc_clean_labels", "before mgc_maxflow")
    fg1 = np.asarray(g.markers()[0]).astype(bool)
    _assert_components(g.components(plane), plane, 1, 0, fg1, bg)
    flow1 = g.maxflow()
    labels1 = g.labels().copy()
    assert (labels1 != labels0).any()
    stats1, counts1 = g.stats(), g.launch_counts()
    _assert_components(g.components(), labels1, 1, 0, fg1, bg)
    g.clean_labels(fill_holes=True, min_size=2)
    # everything is as it was, and the label snapshot of the edit is still there
    assert g.stats() == stats1 and g.launch_counts() == counts1
    np.testing.assert_array_equal(np.sort(g.changed_labels()), np.flatnonzero((labels1 != labels0).ravel()))
    assert g.maxflow() == flow1
    # the same edit on a graph that never heard of components: the same labels, the same flow
    h = solved_graph()
    fam._built(h, "as_shipped")
    assert h.maxflow() == flow0
    h.edit_markers(fg=stroke)
    assert h.maxflow() == flow1
    np.testing.assert_array_equal(h.labels(), labels1)
    # ... and a second edit after the calls goes the same way on both
    stroke2 = fam._stroke(shape, labels1, fg1, bg)
    for graph in (g, h):
        graph.edit_markers(fg=stroke2)
    assert g.maxflow() == h.maxflow()
    np.testing.assert_array_equal(g.labels(), h.labels())
    g.close()
    h.close()


def test_slab_handles_are_refused():
    import ctypes
    from medpy_amd import _lib, synthetic
    from medpy_amd.slab import HipSlab
    sph = synthetic.sphere((32, 24, 24))
    lib = _lib.load()
    r = _lib.CleanRule(0, 0, 0, 0, 1, 0)
    for rank in range(2):
        sl = HipSlab(sph["image"].shape, rank, 2)
        plane = np.ascontiguousarray(sph["fg"][sl.plane0:sl.plane1]).view(np.uint8)
        for lab in (None, _lib.ptr(plane)):
            assert lib.mgc_components(sl._h, lab, 1, 0, None, 0, None, None, None, None) == _lib.ERR_UNSUPPORTED
            assert b"slab" in lib.mgc_last_error(sl._h)
            assert lib.mgc_clean_labels(sl._h, lab, ctypes.byref(r), None, 0, None, None) == _lib.ERR_UNSUPPORTED
            assert b"slab" in lib.mgc_last_error(sl._h)


# ---- 5. 2-D and 1-D graphs end to end -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,conn", [((9, 10), 4), ((9, 10), 8), ((40, 33), 8), ((1, 1, 17), None), ((70,), None)], ids=["9x10_n4", "9x10_n8", "40x33_n8", "1x1x17", "70"])
def test_low_dimensional_graphs_end_to_end(shape, conn):
    nw = fam._nweights(shape, conn)
    fg, bg = fam._markers(shape)
    img = fam._image(shape, "i16")
    t = fam._term(img, fg, bg, fam.BINS["i16"], lam=fam._lam(conn))
    g = fam._handle(shape, conn, nw, fg, bg, feature=img)
    g._add_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"])
    fam._built(g, "as_shipped")
    g.maxflow()
    labels = g.labels().copy()
    full = int(conn == 3 ** len(shape) - 1 and len(shape) > 1)
    _assert_components(g.components(), labels, 1, full, fg, bg)
    for side in (1, 0):
        for f, name in enumerate(FACE_FULL):
            _assert_components(g.components(foreground=bool(side), connectivity=name), labels, side, f, fg, bg)
    want, changed, info = cc.expected_clean(labels, cc.rule(fg_full=full, seeded=1, fill_holes=1), fg, bg)
    np.testing.assert_array_equal(g.clean_labels(seeded=True, fill_holes=True), want)
    np.testing.assert_array_equal(g.clean_labels(seeded=True, fill_holes=True, changed_only=True), changed)
    g.close()


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------
def test_cli_flags_on_the_real_fixture(tmp_path):
    from conftest import GOLDEN
    from medpy_amd import io
    from medpy_amd.cli.graphcut_voxel import main
    z = np.load(os.path.join(GOLDEN, "reference_b0.npz"))
    img, markers = z["image"].astype(np.dtype(str(z["image_dtype"]))), z["markers"]
    hdr = io.Header((1.0, 1.0))
    io.save(img, str(tmp_path / "b0.nii.gz"), hdr, True)
    io.save(markers, str(tmp_path / "m.nii.gz"), hdr, True)
    base = [str(float(z["difference_exponential/sigma"])), str(tmp_path / "b0.nii.gz"), str(tmp_path / "m.nii.gz")]
    assert main(base + [str(tmp_path / "raw.nii.gz")]) == 0
    raw = io.load(str(tmp_path / "raw.nii.gz"))[0].astype(bool)
    fg, bg = markers == 1, markers == 2
    for flags, r in ((["--keep-seeded", "--fill-holes"], cc.rule(seeded=1, fill_holes=1)), (["--keep-largest", "1"], cc.rule(largest=1)),
                     (["--min-size", "50", "--fill-holes"], cc.rule(min_size=50, fill_holes=1))):
        assert main(base + [str(tmp_path / "clean.nii.gz"), "-f"] + flags) == 0
        got = io.load(str(tmp_path / "clean.nii.gz"))[0].astype(bool)
        want, changed, info = cc.expected_clean(raw, r, fg, bg)
        print(flags, info)
        np.testing.assert_array_equal(got, want)

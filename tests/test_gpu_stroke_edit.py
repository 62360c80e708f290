"""-m gpu: markers edited by voxel lists and labels read back as the list of voxels that changed (VoxelGraph.edit_markers /
markers / changed_labels / labels(out=...), C ABI mgc_edit_markers / mgc_get_markers / mgc_labels_delta; DESIGN 10, "Edits by
list").  Every cut after a list edit is held against (i) a COLD graph_from_voxels of the equivalent masks -- labels identical, flow
== -- and (ii) the BK oracle, and the preflow it leaves must pass mgc_validate; the resident masks are read back and compared with
the mask formula, and the list of changed labels with the difference of two full reads."""
import ctypes

import numpy as np
import pytest

from oracle import pipeline

pytestmark = pytest.mark.gpu


def _kwargs(s, reg=None, conn=None):
    from medpy_amd import graphcut
    kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
              boundary_term_args=(s["image"], s["sigma"], False))
    if reg is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    if conn:
        kw["connectivity"] = conn
    return kw


def _graph(fg, bg, s, reg=None, conn=None):
    from medpy_amd import graphcut
    return graphcut.graph_from_voxels(fg, bg, **_kwargs(s, reg, conn))


def _check(g, fg, bg, s, reg=None, conn=None, oracle=True):
    """the warm cut of g (inputs fg / bg / reg now) against a cold build and the BK oracle; returns (flow, labels)"""
    from medpy_amd import _lib
    flow = g.maxflow()
    labels = g.labels().copy()
    cold = _graph(fg, bg, s, reg, conn)
    cflow = cold.maxflow()
    assert np.array_equal(labels, cold.labels()), "warm and cold labels differ in %d voxels" % int((labels != cold.labels()).sum())
    assert flow == cflow, (flow, cflow)
    cold.close()
    if oracle:
        ref = pipeline.graphcut_voxel(fg, bg, term=s["term"], image=s["image"], sigma=s["sigma"],
                                      prob=None if reg is None else reg["prob"], alpha=None if reg is None else reg["alpha"],
                                      connectivity=conn)
        assert np.array_equal(labels, ref.labels), "labels differ from the BK oracle in %d voxels" % int((labels != ref.labels).sum())
        assert flow == pytest.approx(ref.flow, rel=1e-9)
    v = g.validate()
    _lib.assert_valid(v)
    assert v["max_pair_error"] <= 1e-9 and v["max_node_error"] <= 1e-9
    assert flow == pytest.approx(v["cut_capacity"] + v["flow_constant"], rel=1e-12)
    flat = labels.ravel()
    for i in (int(np.argmin(flat)), int(np.argmax(flat))):
        assert g.what_segment(i) == (g.termtype.SOURCE if flat[i] else g.termtype.SINK)
    return flow, labels


def _apply(fg, bg, fg_ids=None, bg_ids=None, erase=None):
    """the edit in mask terms: fg' = (fg & ~erase) | fg_ids, bg' = (bg & ~erase) | bg_ids"""
    shape = fg.shape
    e, f, b = (np.zeros(fg.size, dtype=bool) for _ in range(3))
    for m, ids in ((e, erase), (f, fg_ids), (b, bg_ids)):
        if ids is not None:
            m[np.asarray(ids, dtype=np.int64)] = True
    return ((fg.ravel() & ~e) | f).reshape(shape), ((bg.ravel() & ~e) | b).reshape(shape)


def _lists(fg0, bg0, fg1, bg1):
    """lists (fg, bg, erase) that turn the masks (fg0, bg0) into (fg1, bg1): what left is erased, and a voxel that keeps its
    other marker gets it set again"""
    erase = (fg0 & ~fg1) | (bg0 & ~bg1)
    kw = dict(fg=np.flatnonzero((fg1 & ~fg0) | (erase & fg1)), bg=np.flatnonzero((bg1 & ~bg0) | (erase & bg1)), erase=np.flatnonzero(erase))
    a, b = _apply(fg0, bg0, kw["fg"], kw["bg"], kw["erase"])
    assert np.array_equal(a, fg1) and np.array_equal(b, bg1)
    return kw


def _stroke(shape, lo, hi):
    """voxels on the ray from the centre along the last axis at distances [lo * n, hi * n), two or three voxels wide across it"""
    n = min(shape)
    grids = np.ogrid[tuple(slice(0, s) for s in shape)]
    m = np.ones(shape, dtype=bool)
    for k, (g, s) in enumerate(zip(grids, shape)):
        c = (s - 1) / 2.0
        m = m & (((g - c) >= lo * n) & ((g - c) < hi * n) if k == len(shape) - 1 else np.abs(g - c) <= 1)
    return m


def _edits(s):
    """the edits of an interactive session on synthetic.sphere as lists: {name: keyword arguments of edit_markers}"""
    shape = s["fg"].shape
    face = np.zeros(shape, dtype=bool)
    face[0] = s["bg"][0]
    return {"leak_fix": dict(bg=np.flatnonzero(_stroke(shape, 0.15, 0.25))),     # background stroke inside the bright ball
            "fg_outside": dict(fg=np.flatnonzero(_stroke(shape, 0.35, 0.45))),   # foreground stroke outside it
            "face_removed": dict(erase=np.flatnonzero(face))}                    # part of the face markers taken away


def _edit_and_check(g, fg, bg, kw, s, reg=None, conn=None, oracle=True):
    """one list edit on a SOLVED graph g whose markers are (fg, bg): everything the edit owes; returns the new (fg, bg, labels)"""
    old = g.labels().copy()
    g.edit_markers(**kw)
    fg1, bg1 = _apply(fg, bg, kw.get("fg"), kw.get("bg"), kw.get("erase"))
    _, new = _check(g, fg1, bg1, s, reg, conn, oracle)
    mf, mb = g.markers()
    assert mf.dtype == np.bool_ and mf.shape == fg.shape
    assert np.array_equal(mf, fg1) and np.array_equal(mb, bg1)
    changed = g.changed_labels()
    assert changed.dtype == np.int64 and changed.ndim == 1
    assert np.array_equal(changed, np.flatnonzero(new.ravel() != old.ravel()))
    assert np.array_equal(g.changed_labels(), changed)  # (the call changes no state)
    for dtype in (np.bool_, np.uint8):
        prev = old.astype(dtype)
        got = g.labels(out=prev)
        assert got is prev and np.array_equal(prev.astype(bool), new)
    assert np.array_equal(g.labels(), new)  # the plain read is a full read still
    return fg1, bg1, new


# the flipped labels the BK oracle gives for (n, edit): they pin the non-empty and the empty list
FLIPPED = {(32, "leak_fix"): 13, (32, "fg_outside"): 13, (32, "face_removed"): 0,
           (64, "leak_fix"): 24, (64, "fg_outside"): 28, (64, "face_removed"): 0}


@pytest.mark.parametrize("n", [32, 64, 96])
@pytest.mark.parametrize("edit", ["leak_fix", "fg_outside", "face_removed"])
def test_strokes_6(n, edit):
    from medpy_amd import synthetic
    s = synthetic.sphere((n, n, n))
    g = _graph(s["fg"], s["bg"], s)
    g.maxflow()
    old = g.labels().copy()
    _, _, new = _edit_and_check(g, s["fg"], s["bg"], _edits(s)[edit], s)
    if (n, edit) in FLIPPED:
        assert int((new != old).sum()) == FLIPPED[(n, edit)]
        assert g.changed_labels().size == FLIPPED[(n, edit)]


def test_every_op_in_one_call():
    """sets fg on fresh voxels, sets bg on voxels that carry fg (both markers on one voxel: the flow constant changes), erases
    some of each kind, sets a marker that is set already"""
    from medpy_amd import synthetic
    from medpy_amd.graphcut.graph import merge_marker_edits
    s = synthetic.sphere((40, 40, 40))
    shape = s["fg"].shape
    fg_ids, bg_ids = np.flatnonzero(s["fg"]), np.flatnonzero(s["bg"])
    kw = dict(fg=np.concatenate([np.flatnonzero(_stroke(shape, 0.35, 0.45)), fg_ids[-3:]]),  # fresh voxels; three that are set already
              bg=fg_ids[:5],                                                                # both markers on five voxels
              erase=np.concatenate([fg_ids[5:12], bg_ids[:40]]))
    ops = set(merge_marker_edits(shape, **kw)[1].tolist())
    assert ops == {1, 2, 12}
    g = _graph(s["fg"], s["bg"], s)
    g.maxflow()
    fg1, bg1, _ = _edit_and_check(g, s["fg"], s["bg"], kw, s)
    assert int((fg1 & bg1).sum()) == 5
    # ... and the merged entries: erase + set of the other kind, set of both kinds on one voxel
    both = np.flatnonzero(fg1 & bg1)
    kw2 = dict(fg=np.concatenate([bg_ids[100:104], bg_ids[200:203]]), bg=bg_ids[200:203], erase=np.concatenate([both[:2], bg_ids[100:104]]))
    assert {9, 3, 12} <= set(merge_marker_edits(shape, **kw2)[1].tolist())
    _edit_and_check(g, fg1, bg1, kw2, s)


def test_chain_of_five_list_edits_and_two_edits_before_one_solve():
    from medpy_amd import synthetic
    s = synthetic.sphere((48, 48, 48))
    shape = s["fg"].shape
    g = _graph(s["fg"], s["bg"], s)
    g.maxflow()
    fg, bg = s["fg"], s["bg"]
    no_face = bg.copy()
    no_face[-1] = False
    chain = [(fg, bg | _stroke(shape, 0.15, 0.25)),
             (fg | _stroke(shape, 0.35, 0.45), bg | _stroke(shape, 0.15, 0.25)),
             (fg | _stroke(shape, 0.35, 0.45), no_face),
             (fg, no_face | _stroke(shape, -0.25, -0.15)),
             (fg, bg)]
    fg_now, bg_now = fg, bg
    for fg_k, bg_k in chain:
        fg_now, bg_now, _ = _edit_and_check(g, fg_now, bg_now, _lists(fg_now, bg_now, fg_k, bg_k), s)
        assert np.array_equal(fg_now, fg_k) and np.array_equal(bg_now, bg_k)
    # two edits, no solve between them: the list refers to the last solve BEFORE THE FIRST of the two
    before = g.labels().copy()
    g.edit_markers(bg=np.flatnonzero(_stroke(shape, 0.15, 0.25)))
    g.edit_markers(fg=np.flatnonzero(_stroke(shape, 0.35, 0.45)))
    fg2, bg2 = fg | _stroke(shape, 0.35, 0.45), bg | _stroke(shape, 0.15, 0.25)
    _, after = _check(g, fg2, bg2, s)
    changed = g.changed_labels()
    assert changed.size > 0 and np.array_equal(changed, np.flatnonzero(after.ravel() != before.ravel()))
    assert np.array_equal(g.labels(out=before.copy()), after)


@pytest.mark.parametrize("edit", ["leak_fix", "fg_outside", "face_removed"])
def test_same_state_as_the_mask_path(edit):
    from medpy_amd import synthetic
    s = synthetic.sphere((48, 48, 48))
    a, b = _graph(s["fg"], s["bg"], s), _graph(s["fg"], s["bg"], s)
    assert a.maxflow() == b.maxflow()
    kw = _edits(s)[edit]
    fg1, bg1 = _apply(s["fg"], s["bg"], kw.get("fg"), kw.get("bg"), kw.get("erase"))
    a.update_markers(fg1, bg1)
    b.edit_markers(**kw)
    assert a.maxflow() == b.maxflow()
    assert np.array_equal(a.labels(), b.labels())
    va, vb = a.validate(), b.validate()
    for k, x in va.items():
        if isinstance(x, int):
            assert vb[k] == x, k
    assert va["cut_capacity"] == vb["cut_capacity"] and va["flow_constant"] == vb["flow_constant"]


def test_more_changed_labels_than_the_buffer_holds():
    """32^3, every fg marker erased: the oracle puts all 3 648 voxels of the former foreground on the sink side"""
    from medpy_amd import _lib, synthetic
    s = synthetic.sphere((32, 32, 32))
    g = _graph(s["fg"], s["bg"], s)
    g.maxflow()
    old = g.labels().copy()
    assert int(old.sum()) == 3648
    fg_ids = np.flatnonzero(s["fg"])
    assert fg_ids.size == 136
    g.edit_markers(erase=fg_ids)
    _, new = _check(g, np.zeros_like(s["fg"]), s["bg"], s)
    assert not new.any()
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    ids = np.full(100, -7, dtype=np.int64)
    assert lib.mgc_labels_delta(g._h, 100, _lib.ptr(ids), ctypes.byref(n)) == _lib.OK
    assert n.value == 3648 and (ids == -7).all()
    n = ctypes.c_int64(-1)
    assert lib.mgc_labels_delta(g._h, 0, None, ctypes.byref(n)) == _lib.OK and n.value == 3648
    ids = np.full(3648 + 8, -7, dtype=np.int64)
    assert lib.mgc_labels_delta(g._h, 3648, _lib.ptr(ids), ctypes.byref(n)) == _lib.OK
    assert n.value == 3648 and (ids[3648:] == -7).all()
    assert np.array_equal(ids[:3648], np.flatnonzero(old.ravel()))
    assert np.array_equal(g.changed_labels(), ids[:3648])  # (more than the Python layer's first buffer: it asks twice)
    assert g.stats()["delta_ms"] > 0.0


@pytest.mark.parametrize("shape,conn,regional", [((48, 48, 48), 26, False), ((48, 48, 48), 26, True), ((96, 80), None, False),
                                                 ((96, 80), 8, False), ((600,), None, False), ((33, 41, 29), None, False)])
def test_shapes_and_neighbourhoods(shape, conn, regional):
    """(33, 41, 29): rows that are no multiple of 8 (k_labels is the read-out) and a volume whose last 16-byte vector is partial"""
    from medpy_amd import synthetic
    s = synthetic.sphere(shape)
    reg = synthetic.regional(shape) if regional else None
    g = _graph(s["fg"], s["bg"], s, reg, conn)
    g.maxflow()
    fg, bg = s["fg"], s["bg"]
    for name, kw in _edits(s).items():
        fg, bg, _ = _edit_and_check(g, fg, bg, kw, s, reg, conn)
    last = int(np.prod(shape)) - 1  # the volume's last voxel: in the tail of the comparison when the size is no multiple of 16
    _edit_and_check(g, fg, bg, dict(fg=np.array([last]), erase=np.array([last])), s, reg, conn)


def test_handle_built_without_a_marker_kind():
    from medpy_amd import synthetic
    shape = (40, 40, 40)
    s = synthetic.sphere(shape)
    reg = synthetic.regional(shape)
    none = np.zeros(shape, dtype=bool)
    g = _graph(s["fg"], none, s, reg)  # (GCGraph.record_markers skips an empty mask: the handle holds no bg plane)
    g.maxflow()
    bytes_before = g.stats()["device_bytes"]
    mf, mb = g.markers()
    assert np.array_equal(mf, s["fg"]) and not mb.any()
    kw = dict(bg=np.flatnonzero(_stroke(shape, 0.15, 0.25)))
    fg1, bg1, _ = _edit_and_check(g, s["fg"], none, kw, s, reg)
    assert g.stats()["device_bytes"] - bytes_before == 2 * s["fg"].size  # the plane the edit created + the kept labels
    bg2 = bg1 | _stroke(shape, -0.25, -0.15)
    g.update_markers(fg1, bg2)  # the plane is reused
    _check(g, fg1, bg2, s, reg)
    assert g.stats()["device_bytes"] - bytes_before == 2 * s["fg"].size
    mf, mb = g.markers()
    assert np.array_equal(mf, fg1) and np.array_equal(mb, bg2)


def test_cold_rebuild_after_list_edits():
    from medpy_amd import _lib, synthetic
    s = synthetic.sphere((40, 40, 40))
    g = _graph(s["fg"], s["bg"], s)
    g.maxflow()
    old = g.labels().copy()
    kw = _edits(s)["leak_fix"]
    g.edit_markers(**kw)
    fg1, bg1 = _apply(s["fg"], s["bg"], kw.get("fg"), kw.get("bg"), kw.get("erase"))
    g._build()
    _, new = _check(g, fg1, bg1, s)
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.changed_labels()
    assert ei.value.code == _lib.ERR_STATE
    stale = old.copy()
    assert np.array_equal(g.labels(out=stale), new) and (new != old).any()
    # the mask update drops the kept labels too
    g.edit_markers(fg=np.flatnonzero(_stroke(s["fg"].shape, 0.35, 0.45)))
    g.maxflow()
    g.changed_labels()
    g.update_markers(fg1, bg1)
    g.maxflow()
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.changed_labels()
    assert ei.value.code == _lib.ERR_STATE


def test_refused_calls_change_nothing():
    from medpy_amd import _lib, synthetic
    s = synthetic.sphere((24, 24, 24))
    nvox = s["fg"].size
    g = _graph(s["fg"], s["bg"], s)
    flow = g.maxflow()
    labels = g.labels().copy()
    with pytest.raises(_lib.MedpyHipError) as ei:  # never edited by list: no earlier cut is kept
        g.changed_labels()
    assert ei.value.code == _lib.ERR_STATE
    lib = _lib.load()
    free = np.flatnonzero(~(s["fg"] | s["bg"]))[:4]
    bad = [([free[0], nvox], [1, 1], "outside"), ([free[0], -1], [1, 1], "outside"), ([free[0], free[1]], [1, 0], "ops 0"),
           ([free[0], free[1]], [1, 16], "ops 16"), ([free[0], free[1]], [2, 5], "same marker"), ([free[0], free[1]], [1, 10], "same marker"),
           ([free[0], free[1], free[2], free[1]], [1, 2, 1, 2], "twice")]
    for ids, ops, word in bad:
        ids, ops = np.array(ids, dtype=np.int64), np.array(ops, dtype=np.uint8)
        rc = lib.mgc_edit_markers(g._h, ids.size, _lib.ptr(ids), _lib.ptr(ops))
        assert rc == _lib.ERR_INVALID, (ids, ops)
        msg = lib.mgc_last_error(g._h).decode()
        assert word in msg and "entry %d" % (3 if word == "twice" else 1) in msg, msg
        mf, mb = g.markers()
        assert np.array_equal(mf, s["fg"]) and np.array_equal(mb, s["bg"])
        assert g.maxflow() == flow and np.array_equal(g.labels(), labels)
        g._labels = None  # (a full read from the device, not the Python layer's copy)
        assert np.array_equal(g.labels(), labels)
        with pytest.raises(_lib.MedpyHipError):
            g.changed_labels()
    # n == 0: MGC_OK, and a solved handle stays solved
    g.edit_markers()
    g.edit_markers(fg=np.empty(0, dtype=np.int64), erase=[])
    g._labels = None
    assert np.array_equal(g.labels(), labels)
    # the Python layer's own refusals
    for kw in (dict(fg=[nvox]), dict(bg=[-1]), dict(erase=np.array([1.0])), dict(fg=([1], [1])), dict(fg=([1], [1], [24]))):
        with pytest.raises(ValueError):
            g.edit_markers(**kw)
    with pytest.raises(ValueError):
        g.labels(out=np.zeros((24, 24, 23), dtype=bool))
    g.edit_markers(fg=(np.array([3]), np.array([4]), np.array([5])))  # an index tuple
    assert g.markers()[0][3, 4, 5] and g.markers()[0].sum() == s["fg"].sum() + 1
    g.close()


def test_state_errors():
    from medpy_amd import _lib, graphcut, synthetic
    from medpy_amd.graphcut.graph import EmbeddedLatticeGraph, VoxelGraph
    s = synthetic.sphere((24, 24, 24))
    g = VoxelGraph(s["fg"].shape)  # before mgc_build
    g._set_boundary("difference_exponential", s["image"], s["sigma"], False)
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.edit_markers(fg=[5])
    assert ei.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.changed_labels()
    assert ei.value.code == _lib.ERR_STATE
    assert not g.markers()[0].any() and not g.markers()[1].any()
    g.close()
    # an edit before the first solve: nothing to keep, the cut is right
    g = _graph(s["fg"], s["bg"], s)
    kw = _edits(s)["leak_fix"]
    g.edit_markers(**kw)
    fg1, bg1 = _apply(s["fg"], s["bg"], kw.get("fg"), kw.get("bg"), kw.get("erase"))
    _check(g, fg1, bg1, s)
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.changed_labels()
    assert ei.value.code == _lib.ERR_STATE
    g.close()
    # graphs that went elsewhere
    s4 = synthetic.sphere((6, 6, 6, 6))
    g4 = _graph(s4["fg"], s4["bg"], s4)
    assert not isinstance(g4, VoxelGraph)
    fg2, bg2 = np.zeros((4, 4), bool), np.zeros((4, 4), bool)
    fg2[0, 0], bg2[3, 3] = True, True
    ge = graphcut.graph_from_voxels(fg2, bg2, boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                    boundary_term_args=(np.arange(9, dtype=np.float64).reshape(3, 3), 1.0, False))
    assert isinstance(ge, EmbeddedLatticeGraph)
    for other in (g4, ge):
        with pytest.raises(NotImplementedError):
            other.edit_markers(fg=[1])
        with pytest.raises(NotImplementedError):
            other.changed_labels()
        with pytest.raises(NotImplementedError):
            other.markers()


def test_no_list_edit_after_a_solve_that_did_not_converge():
    from medpy_amd import _lib, synthetic
    s = synthetic.sphere((96, 96, 96))
    g = _graph(s["fg"], s["bg"], s)
    g.set_param("max_outer", 1)
    with pytest.raises(_lib.MedpyHipError):
        g.maxflow()
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.edit_markers(**_edits(s)["leak_fix"])
    assert ei.value.code == _lib.ERR_STATE
    mf, mb = g.markers()
    assert np.array_equal(mf, s["fg"]) and np.array_equal(mb, s["bg"])
    g.set_param("max_outer", 100000)
    g._build()
    g.maxflow()
    _edit_and_check(g, s["fg"], s["bg"], _edits(s)["leak_fix"], s)


def test_memory_of_the_kept_labels():
    from medpy_amd import synthetic
    s = synthetic.sphere((64, 64, 64))
    nvox = s["fg"].size
    a, b = _graph(s["fg"], s["bg"], s), _graph(s["fg"], s["bg"], s)
    a.maxflow()
    b.maxflow()
    assert a.stats()["device_bytes"] == b.stats()["device_bytes"]
    b.edit_markers(**_edits(s)["leak_fix"])
    assert b.stats()["device_bytes"] - a.stats()["device_bytes"] == nvox  # both kinds of marker exist: the kept labels alone
    b.maxflow()
    b.changed_labels()
    b.edit_markers(**_edits(s)["fg_outside"])
    b.maxflow()
    b.changed_labels()
    assert b.stats()["device_bytes"] - a.stats()["device_bytes"] == nvox

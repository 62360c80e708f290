"""-m gpu: what the six calls that fill the t-link store share and where they differ, in one table --
mgc_add_tweights / mgc_update_tweights, their _binned and their _geodesic forms, each from every state a handle can be in.  After
a call: the counts of tweight_edit_info(), whether the label snapshot of changed_labels() survives, the keys of the note, what the
handle holds of device memory, what went back to the pool -- and that a refused call changes none of it.  The expectations are
stated here, from the calls' contracts; every input is made once per case and shared."""
import re

import numpy as np
import pytest

import geodesic_cases as gc
import test_gpu_histogram_term as fam

pytestmark = pytest.mark.gpu

# a partial tile on every axis, and more than one tile on one axis; each at both neighbourhoods, each image kind at both
CASES = [((9, 8, 7), None, "u8"), ((9, 8, 7), 26, "f32"), ((17, 9, 10), None, "f32"), ((17, 9, 10), 26, "u8")]
CASE_IDS = ["x".join(map(str, s)) + "_n%d_%s" % (c or 6, k) for s, c, k in CASES]
GAMMA, LAM = 0.37, 3.0
TW_SEG = 4096   # voxels per segment of the store's partial sums (mgc_tweight_edit.h)

# the table: call -> (warm form?, keeps the label snapshot?, keys of its note in order; the warm forms of two add fold_ms)
GEO_COUNTS = ["rounds_fg", "rounds_bg", "visits_fg", "visits_bg"]
CALLS = {
    "add": (False, False, ["upload_ms", "check_ms", "accumulate_ms"]),
    "update": (True, False, None),   # leaves no note
    "add_binned": (False, False, ["check_ms", "expand_ms", "flow_const_ms"]),
    "update_binned": (True, False, ["check_ms", "expand_ms", "flow_const_ms", "fold_ms"]),
    "add_geodesic": (False, False, ["transform_ms", "expand_ms", "flow_const_ms"] + GEO_COUNTS),
    "update_geodesic": (True, True, ["transform_ms", "expand_ms", "flow_const_ms", "fold_ms"] + GEO_COUNTS),
}
COLD = [c for c in CALLS if not CALLS[c][0]]
WARM = [c for c in CALLS if CALLS[c][0]]
BUILT_STATES = ["built", "solved", "edited"]   # built but unsolved; solved; solved, then one edit_markers not yet re-solved
_IN = {}


def _inputs(shape, conn, kind):
    key = (shape, conn, kind)
    if key not in _IN:
        rng = np.random.default_rng(31)
        fg, bg = fam._markers(shape)
        img = fam._image(shape, kind)
        _IN[key] = {"nw": fam._nweights(shape, conn), "fg": fg, "bg": bg, "img": img, "term": fam._term(img, fg, bg, fam.BINS[kind], lam=fam._lam(conn)),
                    "held": (rng.uniform(0.0, 2.0, shape), rng.uniform(0.0, 2.0, shape)),   # what a handle "that holds a store" was given
                    "dense": (rng.normal(0.5, 1.0, shape), rng.normal(0.5, 1.0, shape).astype(np.float32))}
        for a in _IN[key]["held"] + _IN[key]["dense"] + (img, fg, bg):
            a.setflags(write=False)
    return _IN[key]


def _geo_arrays(key, fg, bg):
    """(S, K) of the geodesic term of the markers fg / bg at the graph's own neighbourhood, on the host"""
    shape, conn, kind = key
    ck = ("geo", key, fg.tobytes(), bg.tobytes())
    if ck not in _IN:
        img, full = _inputs(*key)["img"], int(conn == 26)
        _IN[ck] = gc.expected_term(gc.expected_geodesic(img, fg, GAMMA, 1.0, None, full), gc.expected_geodesic(img, bg, GAMMA, 1.0, None, full), LAM)
    return _IN[ck]


def _arrays(key, call, g):
    """the two arrays a call stands for: its own, or the tables / the transforms expanded on the host"""
    p = _inputs(*key)
    if call in ("add", "update"):
        return p["dense"]
    if call.endswith("binned"):
        return p["term"]["S"], p["term"]["K"]
    return _geo_arrays(key, *g.markers())


def _issue(key, call, g):
    p = _inputs(*key)
    t = p["term"]
    {"add": lambda: g._add_tweights(*p["dense"]),
     "update": lambda: g.update_tweights_dense(*p["dense"]),
     "add_binned": lambda: g._add_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"]),
     "update_binned": lambda: g.update_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"]),
     "add_geodesic": lambda: g._add_tweights_geodesic(GAMMA, LAM),
     "update_geodesic": lambda: g.update_tweights_geodesic(GAMMA, LAM)}[call]()


def _handle(key, store, image=None):
    p = _inputs(*key)
    g = fam._handle(key[0], key[1], p["nw"], p["fg"], p["bg"], feature=p["img"] if image is None else image)
    if store:
        g._add_tweights(*p["held"])
    return g


def _store_bytes(shape):
    """the store (the plane of t-links, the plane of shares behind a 16-byte border) and its segment partials with their sum"""
    n = int(np.prod(shape))
    return 8 * (((n + 1) & ~1) + n) + 8 * ((n + TW_SEG - 1) // TW_SEG + 1)


def _keys(note):
    return re.findall(r"(\w+)=", note)


def _info(store_held, dense_calls, list_entries, voxels_changed):
    return {"store_held": store_held, "dense_calls": dense_calls, "list_entries": list_entries, "voxels_changed": voxels_changed}


def _snapshot_served(g):
    """the next maxflow(), then: the ids changed_labels() serves, or None where it refuses (no earlier cut is kept)"""
    from medpy_amd import _lib
    g.maxflow()
    try:
        return np.sort(g.changed_labels())
    except _lib.MedpyHipError as e:
        assert e.code == _lib.ERR_STATE and "mgc_labels_delta" in str(e), str(e)
        return None


def _observe(g):
    from medpy_amd import _lib
    return g.tweight_edit_info(), g.stats()["device_bytes"], _lib.pool_info()["idle_bytes"], g.last_note()


def _changed(key, old_calls, new_calls):
    """voxels whose merged t-link differs bit for bit between two histories of dense calls"""
    tr0, _ = fam._merged(key[0], old_calls)
    tr1, _ = fam._merged(key[0], new_calls)
    return int((tr0.view(np.int64) != tr1.view(np.int64)).sum())


@pytest.mark.parametrize("store", [False, True], ids=["fresh", "holds_a_store"])
@pytest.mark.parametrize("shape,conn,kind", CASES, ids=CASE_IDS)
def test_cold_forms(shape, conn, kind, store):
    key = (shape, conn, kind)
    deltas = []
    for call in COLD:
        g = _handle(key, store)
        info0, bytes0, idle0, _ = _observe(g)
        assert info0 == _info(int(store), int(store), 0, 0)
        _issue(key, call, g)
        info, bytes1, idle1, note = _observe(g)
        print(call, info, bytes1 - bytes0, note)
        assert info == _info(1, int(store) + 1, 0, 0)                                    # (a)
        assert _keys(note) == CALLS[call][2] and note.startswith("mgc_" + ("add_tweights" + call[3:]) + ":")   # (c)
        deltas.append(bytes1 - bytes0)                                                   # (d)
        assert idle1 >= idle0                                                            # (e)
        g._build()
        assert _snapshot_served(g) is None                                               # (b): a build keeps no earlier cut
        g.close()
    assert deltas == [0 if store else _store_bytes(shape)] * 3, deltas


@pytest.mark.parametrize("store", [False, True], ids=["fresh", "holds_a_store"])
@pytest.mark.parametrize("shape,conn,kind", CASES, ids=CASE_IDS)
def test_warm_forms_need_a_built_handle(shape, conn, kind, store):
    from medpy_amd import _lib
    key = (shape, conn, kind)
    g = _handle(key, store)
    before = _observe(g)
    for call in WARM:
        with pytest.raises(_lib.MedpyHipError) as ei:
            _issue(key, call, g)
        assert ei.value.code == _lib.ERR_STATE and "before mgc_build" in str(ei.value), str(ei.value)
        assert _observe(g)[:3] == before[:3]
    g.close()


@pytest.mark.parametrize("state", BUILT_STATES)
@pytest.mark.parametrize("store", [False, True], ids=["no_store", "holds_a_store"])
@pytest.mark.parametrize("shape,conn,kind", CASES, ids=CASE_IDS)
def test_warm_forms(shape, conn, kind, store, state):
    key = (shape, conn, kind)
    p = _inputs(*key)
    nvox = int(np.prod(shape))
    for call in WARM:
        keeps = CALLS[call][1]
        g = fam._built(_handle(key, store), "as_shipped")
        labels0 = None
        if state != "built":
            g.maxflow()
            labels0 = g.labels().copy()
        if state == "edited":
            g.edit_markers(fg=fam._stroke(shape, labels0, p["fg"], p["bg"]))
        info0, bytes0, idle0, note0 = _observe(g)
        s, k = _arrays(key, call, g)
        _issue(key, call, g)
        info, bytes1, idle1, note = _observe(g)
        print(call, state, info, bytes1 - bytes0, note)
        changed = _changed(key, [p["held"]] if store else [], [(s, k)])
        assert changed > 0
        assert info == _info(1, 1, 0, changed)                                           # (a): what clear + one dense call leave
        if CALLS[call][2] is None:                                                       # (c)
            assert note == note0
        else:
            assert _keys(note) == CALLS[call][2] and note.startswith("mgc_update_tweights" + call[6:] + ":")
        # (d): the store of a handle that had none; the geodesic form also reserves the plane of the kept labels after a finished solve
        # (the edit before it has done so already)
        assert bytes1 - bytes0 == (0 if store else _store_bytes(shape)) + (nvox if keeps and state == "solved" else 0)
        assert idle1 >= idle0                                                            # (e)
        served = _snapshot_served(g)                                                     # (b)
        if keeps and state != "built":
            np.testing.assert_array_equal(served, np.flatnonzero((g.labels() != labels0).ravel()))
        else:
            assert served is None
        g.close()


@pytest.mark.parametrize("shape,conn,kind", CASES, ids=CASE_IDS)
def test_refused_calls_change_nothing(shape, conn, kind):
    from medpy_amd import _lib
    lib = _lib.load()
    key = (shape, conn, kind)
    p = _inputs(*key)
    t = p["term"]
    last = int(np.prod(shape)) - 1
    bad_sink = np.array(p["dense"][1], dtype=np.float64)
    bad_sink.flat[last] = np.nan
    bad_img = fam._image(shape, "f32").copy()
    bad_term = fam._term(bad_img, p["fg"], p["bg"], fam.BINS["f32"])   # (tables and a binning that pass their own checks)
    bad_img.flat[last] = np.inf

    def refused(g, warm):
        up = "update" if warm else "add"
        yield "sink[%d] = nan" % last, "t-link weights must be finite", (lambda: g.update_tweights_dense(p["dense"][0], bad_sink)) if warm else (lambda: g._add_tweights(p["dense"][0], bad_sink))
        yield "image[%d] = inf" % last, "the feature image must be finite", (
            lambda: g.update_tweights_binned(bad_term["tables"][0], bad_term["tables"][1], *bad_term["binning"])) if warm else (
            lambda: g._add_tweights_binned(bad_term["tables"][0], bad_term["tables"][1], *bad_term["binning"]))
        yield "image[%d] = inf" % last, "the image must be finite", (lambda: g.update_tweights_geodesic(GAMMA, LAM)) if warm else (lambda: g._add_tweights_geodesic(GAMMA, LAM))
        yield "lam = inf", "lam must be finite", lambda: _lib.check(g._h, getattr(lib, "mgc_%s_tweights_geodesic" % up)(g._h, int(conn == 26), GAMMA, 1.0, None, np.inf))

    states = [("fresh", False, lambda: _handle(key, False, bad_img)), ("holds_a_store", False, lambda: _handle(key, True, bad_img))]
    for store in (False, True):
        def solved(store=store):
            g = fam._built(_handle(key, store, bad_img), "as_shipped")
            g.maxflow()
            return g
        states.append(("solved" + "_holds_a_store" * store, True, solved))
    for name, warm, make in states:
        g = make()
        before = _observe(g)
        labels0 = g.labels().copy() if warm else None
        for offender, wording, call in refused(g, warm):
            with pytest.raises(_lib.MedpyHipError) as ei:
                call()
            print(name, str(ei.value))
            assert ei.value.code == _lib.ERR_INVALID and offender in str(ei.value) and wording in str(ei.value), str(ei.value)
            info, nbytes, idle, _ = _observe(g)
            assert info == before[0] and nbytes == before[1] and idle >= before[2]       # (d), (e)
        if warm:   # the cut the handle held is still its cut
            np.testing.assert_array_equal(g.labels(), labels0)
        g.close()


def test_binned_and_geodesic_leave_what_the_arrays_leave():
    """(f), at one shape: with equivalent inputs the store is bit for bit that of the arrays pair -- cold, and warm on top of a store"""
    key = CASES[2]
    p = _inputs(*key)
    for pair in ("binned", "geodesic"):
        a, b = _handle(key, True), _handle(key, True)
        s, k = _arrays(key, "add_" + pair, a)
        _issue(key, "add_" + pair, a)
        b._add_tweights(s, k)
        for g in (a, b):
            fam._built(g, "as_shipped")
        assert fam._bits(a.tweights()) == fam._bits(b.tweights()) and a.tweight_edit_info() == b.tweight_edit_info()
        assert a.maxflow() == b.maxflow()
        _issue(key, "update_" + pair, a)
        b.update_tweights_dense(s, k)
        assert fam._bits(a.tweights()) == fam._bits(b.tweights()) and a.tweight_edit_info() == b.tweight_edit_info()
        assert a.maxflow() == b.maxflow()
        np.testing.assert_array_equal(a.labels(), b.labels())
        a.close()
        b.close()

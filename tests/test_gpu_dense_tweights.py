"""-m gpu: whole t-link weight arrays (mgc_add_tweights / GCGraph.set_tweights_dense), their warm update and their edits by voxel
list against the BK oracle.

n-link weights are drawn from uniform(0.1, 10) and go in through _add_nweights; source and sink weights from uniform(0, 5), a
tenth of the source entries negated.  Continuous weights: the minimum cut is unique and the labels must equal BK's voxel for
voxel, without the tie relaxation of oracle/cutcheck.py.  The oracle is fed in the library's merge order: explicit t-links first,
the regional probability map, the markers last.  Every reference cut is computed once per input and module and shared."""
import itertools

import numpy as np
import pytest

from oracle import bk

pytestmark = pytest.mark.gpu

MAX = 65535.0  # GCGraph.MAX
CASES = [((9, 8, 7), None), ((1, 1, 17), None), ((3, 1, 5), None), ((17, 9, 10), None), ((9, 10), 4), ((9, 10), 8), ((9, 10, 11), 26)]
CASE_IDS = ["x".join(map(str, s)) + "_n%d" % (c or 2 * len(s)) for s, c in CASES]
FORMS = ["as_shipped", "large_volume_forms"]
_REF = {}


def _offsets(ndim, conn):
    if conn in (None, 2 * ndim):
        return [tuple(1 if k == a else 0 for k in range(ndim)) for a in range(ndim)]
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if o > (0,) * ndim]


def _arcs(shape, off):
    ids = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, shape))
    dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, shape))
    mask = np.zeros(shape, bool)
    mask[src] = True
    return mask, ids[src].ravel(), ids[dst].ravel()


def _nweights(shape, conn, seed=23):
    rng = np.random.default_rng(seed)
    return {o: (rng.uniform(0.1, 10.0, shape), rng.uniform(0.1, 10.0, shape)) for o in _offsets(len(shape), conn)}


def _tweights(shape, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 5.0, shape)
    s[rng.random(shape) < 0.1] *= -1.0
    return s.astype(dtype), rng.uniform(0.0, 5.0, shape).astype(dtype)


def _markers(shape):
    """a small box of fg near the low corner, the far face along the last axis as bg"""
    fg = np.zeros(shape, bool)
    bg = np.zeros(shape, bool)
    fg[tuple(slice(n // 3, n // 3 + 2) for n in shape[:-1]) + (slice(1, 3),)] = True
    bg[..., -1] = True
    return fg, bg


def _bk(key, shape, nw, calls=(), fg=None, bg=None, prob=None):
    """(flow, labels) of BK: explicit t-links call by call, the probability map (p, alpha), the markers last"""
    if key in _REF:
        return _REF[key]
    n = int(np.prod(shape))
    g = bk.BKGraph(n, n * 13 + 16)
    for s, k in calls:
        g.add_tweights(None, np.asarray(s, np.float64).ravel(), np.asarray(k, np.float64).ravel())
    if prob is not None:
        p, alpha = prob
        g.add_tweights(None, (p * alpha).astype(np.float64).ravel(), ((1 - p) * alpha).astype(np.float64).ravel())
    for o, (there, back) in nw.items():
        mask, i, j = _arcs(shape, o)
        g.sum_edges(i, j, there[mask], back[mask])
    for m, (s, t) in ((fg, (MAX, 0.0)), (bg, (0.0, MAX))):
        idx = np.flatnonzero(m.ravel()) if m is not None else np.empty(0, np.int64)
        if idx.size:
            g.add_tweights(idx, np.full(idx.size, s), np.full(idx.size, t))
    flow = g.maxflow()
    _REF[key] = (flow, g.labels().astype(bool).reshape(shape))
    return _REF[key]


def _handle(shape, conn, nw, calls=(), fg=None, bg=None, prob=None, forms="as_shipped", build=True):
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph(shape, connectivity=conn)
    if prob is not None:
        g._set_regional(*prob)
    if fg is not None or bg is not None:
        g._set_markers(fg, bg)
    for o, (there, back) in nw.items():
        g._add_nweights(o, there, back)
    for s, k in calls:
        g._add_tweights(s, k)
    if build:
        g._build()
        if forms == "large_volume_forms":
            from conftest import LARGE_VOLUME_FORMS
            for kv in LARGE_VOLUME_FORMS.split(","):
                name, v = kv.split("=")
                g.set_param(name, int(v))
    return g


def _assert_cut(g, flow_ref, labels_ref):
    from medpy_amd import _lib
    flow = g.maxflow()
    v = g.validate()
    print("flow %r (BK %r), %d voxels differ, pair error %g, node error %g" % (flow, flow_ref, int((g.labels() != labels_ref).sum()),
                                                                                 v["max_pair_error"], v["max_node_error"]))
    np.testing.assert_array_equal(g.labels(), labels_ref)
    assert flow == pytest.approx(flow_ref, rel=1e-9, abs=1e-300)
    assert not any(v[k] for k in _lib.VIOLATION_KEYS), v
    assert v["max_pair_error"] <= 1e-9 and v["max_node_error"] <= 1e-9, v
    return flow


def _merged(shape, calls):
    from medpy_amd.graphcut.graph import merge_tweights_into
    n = int(np.prod(shape))
    tr, fc = np.zeros(n), 0.0
    for s, k in calls:
        fc = merge_tweights_into(tr, fc, np.arange(n), np.asarray(s, np.float64).ravel(), np.asarray(k, np.float64).ravel())
    return tr, fc


def _replaced(calls, ids, s, k):
    """the one call that leaves what the store holds after edit_tweights(ids, s, k) on a store of ONE call"""
    (s0, k0), = calls
    s1, k1 = s0.astype(np.float64).copy(), k0.astype(np.float64).copy()
    s1.ravel()[ids] = s
    k1.ravel()[ids] = k
    return [(s1, k1)]


# ---- 1. cold ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_cold_store_and_cut(shape, conn, forms):
    nw = _nweights(shape, conn)
    fg, bg = _markers(shape)
    one64, one32 = [_tweights(shape, 5)], [_tweights(shape, 5, np.float32)]
    two = [_tweights(shape, 5, np.float32), _tweights(shape, 6)]
    for name, calls in (("one64", one64), ("one32", one32), ("two", two)):
        g = _handle(shape, conn, nw, calls, forms=forms)
        info = g.tweight_edit_info()
        assert info["store_held"] == 1 and info["dense_calls"] == len(calls)
        tr, _ = _merged(shape, calls)
        assert g.tweights().ravel().view(np.int64).tolist() == tr.view(np.int64).tolist()   # bit for bit the host merge
        _assert_cut(g, *_bk(("cold", shape, conn, name), shape, nw, calls))
        g.close()
    # markers, and a regional probability map, on top: the merge order
    g = _handle(shape, conn, nw, two, fg, bg, forms=forms)
    _assert_cut(g, *_bk(("cold", shape, conn, "two+markers"), shape, nw, two, fg, bg))
    g.close()
    prob = (np.random.default_rng(7).random(shape).astype(np.float32), 3.0)
    g = _handle(shape, conn, nw, one64, fg, bg, prob=prob, forms=forms)
    _assert_cut(g, *_bk(("cold", shape, conn, "one+prob+markers"), shape, nw, one64, fg, bg, prob=prob))
    g.close()


# ---- 2. through the public interface ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,conn", [((17, 9, 10), None), ((9, 10), 8), ((9, 10, 11), 26)], ids=["17x9x10_n6", "9x10_n8", "9x10x11_n26"])
def test_regional_precomputed_takes_the_device_path(shape, conn):
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel
    nw = _nweights(shape, conn)
    fg, bg = _markers(shape)
    calls = [_tweights(shape, 5)]

    def boundary(graph, args):
        for o, (there, back) in args.items():
            graph.set_nweights_dense(o, there, back)
    g = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_precomputed, regional_term_args=calls[0],
                                   boundary_term=boundary, boundary_term_args=nw, connectivity=conn)
    info = g.tweight_edit_info()
    assert info["store_held"] == 1 and info["dense_calls"] == 1   # the store, not the host merge
    _assert_cut(g, *_bk(("public", shape, conn), shape, nw, calls, fg, bg))
    g.edit_tweights(0, 1.0, 2.0)   # (a graph of the device path can be edited)
    g.close()
    # per-node t-weights in the mix: merged on the host, the same cut, and no edits
    def regional(graph, args):
        graph.set_tweights_dense(*args)
        graph.set_tweight(0, 0.0, 0.0)
    g = graphcut.graph_from_voxels(fg, bg, regional_term=regional, regional_term_args=calls[0], boundary_term=boundary, boundary_term_args=nw,
                                   connectivity=conn)
    assert g.tweight_edit_info()["store_held"] == 0
    _assert_cut(g, *_bk(("public", shape, conn), shape, nw, calls, fg, bg))
    with pytest.raises(NotImplementedError):
        g.edit_tweights(0, 1.0, 2.0)
    with pytest.raises(NotImplementedError):
        g.update_tweights_dense(*calls[0])
    g.close()


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(1, 1, 17), (9, 8, 7)], ids=["1x1x17", "9x8x7"])
def test_array_checks_name_the_first_offender_and_change_nothing(shape, dtype):
    from medpy_amd import _lib
    nw = _nweights(shape, None)
    calls = [_tweights(shape, 5, dtype)]
    g = _handle(shape, None, nw, calls)
    n = int(np.prod(shape))
    t0, info0, bytes0 = g.tweights(), g.tweight_edit_info(), g.stats()["device_bytes"]
    last = n - 1   # (odd n: the entry behind the last whole vector)
    for which, idx, value in (("source", last, np.nan), ("sink", last, np.inf), ("source", 3, -np.inf), ("sink", n // 2, np.nan)):
        for call in (g._add_tweights, g.update_tweights_dense):
            s, k = (a.copy() for a in _tweights(shape, 9, dtype))
            (s if which == "source" else k).ravel()[idx] = value
            if idx != last:
                (k if which == "source" else s).ravel()[last] = np.nan   # a later offender, in the other array: not the one named
            with pytest.raises(_lib.MedpyHipError) as ei:
                call(s, k)
            assert ei.value.code == _lib.ERR_INVALID and "%s[%d]" % (which, idx) in str(ei.value), str(ei.value)
            assert g.tweight_edit_info() == info0 and g.stats()["device_bytes"] == bytes0
            assert np.array_equal(g.tweights(), t0)   # (still built: the refused call left the handle as it was)
    # both arrays bad at one index: the source entry is the first
    s, k = (a.copy() for a in _tweights(shape, 9, dtype))
    s.ravel()[2] = k.ravel()[2] = np.nan
    with pytest.raises(_lib.MedpyHipError) as ei:
        g._add_tweights(s, k)
    assert "source[2]" in str(ei.value)
    _assert_cut(g, *_bk(("refuse", shape, str(np.dtype(dtype))), shape, nw, calls))
    g.close()


def test_list_errors_are_refused_before_the_first_write():
    from medpy_amd import _lib
    shape = (17, 9, 10)
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    calls = [_tweights(shape, 5)]
    ref = _bk(("list_refuse", shape), shape, nw, calls, fg, bg)
    g = _handle(shape, None, nw, calls, fg, bg)
    n = int(np.prod(shape))
    flow0 = _assert_cut(g, *ref)
    t0, info0 = g.tweights(), g.tweight_edit_info()
    for ids, s, k, names in (([5, n, 7], 1.0, 1.0, "entry 1"), ([5, -1], 1.0, 1.0, "entry 1"), ([9, 4, 9], 1.0, 1.0, "entry 2"),
                             ([4, 9, 11], [1.0, np.nan, 1.0], 1.0, "entry 1"), ([4, 9, 11], 1.0, [1.0, 1.0, np.inf], "entry 2")):
        with pytest.raises(_lib.MedpyHipError) as ei:
            g.edit_tweights(np.array(ids), s, k)
        assert ei.value.code == _lib.ERR_INVALID and names in str(ei.value), str(ei.value)
        assert g.tweight_edit_info() == info0 and np.array_equal(g.tweights(), t0)
        assert g.maxflow() == flow0 and np.array_equal(g.labels(), ref[1])   # the finished solve is still there
    # n == 0 keeps a finished solve
    g.edit_tweights(np.empty(0, np.int64), 1.0, 1.0)
    assert g.maxflow() == flow0 and np.array_equal(g.labels(), ref[1]) and g.tweight_edit_info() == info0
    # an unsorted list is taken (sorted in a copy)
    ids = np.array([700, 3, 250])
    g.edit_tweights(ids, [9.0, 8.0, 7.0], [0.0, 0.5, 0.25])
    assert g.tweight_edit_info()["list_entries"] == 3
    _assert_cut(g, *_bk(("list_refuse", shape, "unsorted"), shape, nw, _replaced(calls, ids, [9.0, 8.0, 7.0], [0.0, 0.5, 0.25]), fg, bg))
    g.close()


def test_states():
    from medpy_amd import _lib
    lib = _lib.load()
    shape = (9, 8, 7)
    n = int(np.prod(shape))
    nw = _nweights(shape, None)
    s, k = _tweights(shape, 5)
    one = (np.array([3], np.int64), np.array([1.0]), np.array([2.0]))

    def edit(g):
        return lib.mgc_edit_tweights(g._h, 1, *[_lib.ptr(a) for a in one])
    g = _handle(shape, None, nw, [(s, k)], build=False)   # before mgc_build
    assert edit(g) == _lib.ERR_STATE
    assert lib.mgc_update_tweights(g._h, _lib.ptr(s), _lib.ptr(k), _lib.DTYPE_IDS[s.dtype]) == _lib.ERR_STATE
    # the store and mgc_set_tweights_merged are exclusive, both ways
    tr = np.ascontiguousarray((s - k).ravel())
    assert lib.mgc_set_tweights_merged(g._h, _lib.ptr(tr), 0.0) == _lib.ERR_STATE
    g._clear_tweights()
    assert g.tweight_edit_info()["store_held"] == 0
    g._set_tweights_merged(tr, 1.5)
    assert lib.mgc_add_tweights(g._h, _lib.ptr(s), _lib.ptr(k), _lib.DTYPE_IDS[s.dtype]) == _lib.ERR_STATE
    g._build()
    assert edit(g) == _lib.ERR_STATE and lib.mgc_update_tweights(g._h, _lib.ptr(s), _lib.ptr(k), _lib.DTYPE_IDS[s.dtype]) == _lib.ERR_STATE
    assert b"mgc_set_tweights_merged" in lib.mgc_last_error(g._h)
    assert g.tweight_edit_info()["store_held"] == 0
    g._clear_tweights()
    g._add_tweights(s, k)
    g._build()
    assert edit(g) == _lib.OK and g.tweight_edit_info()["store_held"] == 1
    assert lib.mgc_add_tweights(g._h, _lib.ptr(s), None, _lib.DTYPE_IDS[s.dtype]) == _lib.ERR_INVALID
    assert lib.mgc_add_tweights(g._h, _lib.ptr(s), _lib.ptr(k), _lib.DTYPE_IDS[np.dtype(np.int32)]) == _lib.ERR_INVALID
    g.close()
    assert n == s.size


def test_no_edit_after_a_solve_that_did_not_converge():
    from medpy_amd import _lib, graphcut, synthetic
    sph = synthetic.sphere((96, 96, 96))   # (the volume test_gpu_warm_resolve.py stops after one outer round)
    g = graphcut.graph_from_voxels(sph["fg"], sph["bg"], boundary_term=getattr(graphcut.energy_voxel, "boundary_" + sph["term"]),
                                   boundary_term_args=(sph["image"], sph["sigma"], False))
    g.set_param("max_outer", 1)
    with pytest.raises(_lib.MedpyHipError):
        g.maxflow()
    bytes0 = g.stats()["device_bytes"]
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.edit_tweights(5, 1.0, 0.0)
    assert ei.value.code == _lib.ERR_STATE and g.tweight_edit_info()["store_held"] == 0 and g.stats()["device_bytes"] == bytes0
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.update_tweights_dense(np.ones(sph["fg"].shape, np.float32), np.ones(sph["fg"].shape, np.float32))
    assert ei.value.code == _lib.ERR_STATE and g.stats()["device_bytes"] == bytes0
    g.close()


def test_slab_handles_are_rebuilt_not_edited():
    from medpy_amd import _lib, synthetic
    from medpy_amd.slab import HipSlab, LoopbackExchange, sync_boundary_table
    sph = synthetic.sphere((32, 24, 24))
    slabs = [HipSlab(sph["image"].shape, r, 2) for r in range(2)]
    for sl in slabs:
        planes = slice(sl.plane0, sl.plane1)
        sl.set_boundary(sph["term"], sph["image"][planes], sph["sigma"], False)
        sl.set_markers(sph["fg"][planes], sph["bg"][planes])
    sync_boundary_table(slabs, LoopbackExchange(slabs))
    lib = _lib.load()
    ids, s, k = np.array([0], np.int64), np.array([1.0]), np.array([0.0])
    out = np.zeros(4, np.int64)
    for sl in slabs:
        sl.build()
        assert lib.mgc_edit_tweights(sl._h, 1, _lib.ptr(ids), _lib.ptr(s), _lib.ptr(k)) == _lib.ERR_STATE
        assert b"slab" in lib.mgc_last_error(sl._h)
        assert lib.mgc_get_tweight_edit_info(sl._h, _lib.ptr(out)) == _lib.OK and not out.any()


# ---- 4. warm whole-array update --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_warm_update_equals_cold_and_bk(shape, conn, forms):
    nw = _nweights(shape, conn)
    fg, bg = _markers(shape)
    arrays = [_tweights(shape, 5), _tweights(shape, 6, np.float32), _tweights(shape, 7)]
    g = _handle(shape, conn, nw, [arrays[0], arrays[1]], fg, bg, forms=forms)   # (two calls: the update replaces both)
    _assert_cut(g, *_bk(("warm", shape, conn, "01"), shape, nw, [arrays[0], arrays[1]], fg, bg))
    first = None
    for step in (2, 1, 0, 2):   # a chain; the last update goes back to arrays seen before
        g.update_tweights_dense(*arrays[step])
        info = g.tweight_edit_info()
        assert info["store_held"] == 1 and info["dense_calls"] == 1 and info["voxels_changed"] > 0
        ref = _bk(("warm", shape, conn, step), shape, nw, [arrays[step]], fg, bg)
        flow = _assert_cut(g, *ref)
        cold = _handle(shape, conn, nw, [arrays[step]], fg, bg, forms=forms)
        assert cold.maxflow() == pytest.approx(flow, rel=1e-9) and np.array_equal(cold.labels(), g.labels())
        assert g.tweights().ravel().view(np.int64).tolist() == cold.tweights().ravel().view(np.int64).tolist()
        cold.close()
        if step == 2 and first is None:
            first = g.labels().copy()
    assert np.array_equal(g.labels(), first)   # back to the first arrays of the chain: the first cut
    g.update_tweights_dense(*arrays[2])        # the same arrays again: nothing changes bitwise
    assert g.tweight_edit_info()["voxels_changed"] == 0
    _assert_cut(g, *_bk(("warm", shape, conn, 2), shape, nw, [arrays[2]], fg, bg))
    g.close()


def test_warm_update_gives_a_handle_its_first_store():
    shape = (17, 9, 10)
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    g = _handle(shape, None, nw, (), fg, bg)
    _assert_cut(g, *_bk(("first_store", shape, "none"), shape, nw, (), fg, bg))
    assert g.tweight_edit_info()["store_held"] == 0
    calls = [_tweights(shape, 5)]
    g.update_tweights_dense(*calls[0])
    assert g.tweight_edit_info()["store_held"] == 1
    _assert_cut(g, *_bk(("first_store", shape, "one"), shape, nw, calls, fg, bg))
    g.close()


# ---- 5. warm list edits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("shape", [(17, 9, 10), (16, 16, 16)], ids=["17x9x10", "16x16x16"])
def test_list_edits(shape, forms):
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    calls = [_tweights(shape, 5)]
    rng = np.random.default_rng(31)
    flow0, lab0 = _bk(("edit", shape, 0), shape, nw, calls, fg, bg)
    g = _handle(shape, None, nw, calls, fg, bg, forms=forms)
    _assert_cut(g, flow0, lab0)
    free = ~fg.ravel() & ~bg.ravel()
    # (a) voxels of the sink side get strong source links: they flip
    ids_a = rng.choice(np.flatnonzero(~lab0.ravel() & free), 20, replace=False)
    s_a, k_a = rng.uniform(60.0, 90.0, 20), rng.uniform(0.0, 1.0, 20)
    g.edit_tweights(ids_a, s_a, k_a)
    info = g.tweight_edit_info()
    assert info["list_entries"] == 20 and info["voxels_changed"] == 20
    calls_a = _replaced(calls, ids_a, s_a, k_a)
    flow1, lab1 = _bk(("edit", shape, "a"), shape, nw, calls_a, fg, bg)
    _assert_cut(g, flow1, lab1)
    changed = g.changed_labels()
    assert changed.size > 0 and changed.tolist() == np.flatnonzero(lab0.ravel() != lab1.ravel()).tolist()
    # (b) inside the source region: voxels whose label said "cannot reach the sink" get sink links and flip
    ids_b = rng.choice(np.flatnonzero(lab1.ravel() & free), 20, replace=False)
    s_b, k_b = rng.uniform(0.0, 1.0, 20), rng.uniform(60.0, 90.0, 20)
    g.edit_tweights(np.unravel_index(ids_b, shape), s_b, k_b)   # (index tuples)
    calls_b = _replaced(calls_a, ids_b, s_b, k_b)
    flow2, lab2 = _bk(("edit", shape, "b"), shape, nw, calls_b, fg, bg)
    _assert_cut(g, flow2, lab2)
    changed = g.changed_labels()
    assert changed.size > 0 and changed.tolist() == np.flatnonzero(lab1.ravel() != lab2.ravel()).tolist()
    assert not lab2.ravel()[ids_b].any()
    # (c) two edits before one solve: the delta spans both -- and they lead back to the first store, so to the first cut
    g.edit_tweights(ids_b, calls[0][0].ravel()[ids_b], calls[0][1].ravel()[ids_b])
    g.edit_tweights(ids_a, calls[0][0].ravel()[ids_a], calls[0][1].ravel()[ids_a])
    _assert_cut(g, flow0, lab0)
    assert g.changed_labels().tolist() == np.flatnonzero(lab2.ravel() != lab0.ravel()).tolist()
    cold = _handle(shape, None, nw, calls, forms=forms)
    assert g.tweights().ravel()[free].view(np.int64).tolist() == cold.tweights().ravel()[free].view(np.int64).tolist()   # the old values, bit for bit
    cold.close()
    # (d) a rebuild after edits is the graph of the edited store
    g.edit_tweights(ids_a, s_a, k_a)
    g._build()
    _assert_cut(g, flow1, lab1)
    g.close()


@pytest.mark.parametrize("side", ["source", "sink"])
def test_an_edit_gives_a_markers_only_graph_its_store_and_a_tile_its_first_tlink(side):
    """The flag invariant: the tile of voxel (12, 2, 3) of the (17, 9, 10) volume holds no marker and, the store being created by
    the edit itself, no t-link at all; the edit gives it its first source link in one run and its first sink link in the other."""
    shape = (17, 9, 10)
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    if side == "sink":   # a bg box in the far corner instead of the face: the cut hugs it, the edited voxel starts on the source side
        bg = np.zeros(shape, bool)
        bg[-2:, -2:, -2:] = True
    vox = (12, 2, 3)
    assert not fg[8:16, 0:8, 0:8].any() and not bg[8:16, 0:8, 0:8].any()
    flow0, lab0 = _bk(("flags", side, 0), shape, nw, (), fg, bg)
    assert lab0[vox] == (side == "sink")
    g = _handle(shape, None, nw, (), fg, bg)
    _assert_cut(g, flow0, lab0)
    assert g.tweight_edit_info()["store_held"] == 0
    s, k = (100.0, 0.0) if side == "source" else (0.0, 100.0)
    g.edit_tweights((np.array([vox[0]]), np.array([vox[1]]), np.array([vox[2]])), s, k)
    assert g.tweight_edit_info() == {"store_held": 1, "dense_calls": 0, "list_entries": 1, "voxels_changed": 1}
    sa, ka = np.zeros(shape), np.zeros(shape)
    sa[vox], ka[vox] = s, k
    flow1, lab1 = _bk(("flags", side, 1), shape, nw, [(sa, ka)], fg, bg)
    _assert_cut(g, flow1, lab1)
    changed = g.changed_labels()
    assert changed.size > 0 and changed.tolist() == np.flatnonzero(lab0.ravel() != lab1.ravel()).tolist()
    assert g.tweights()[vox] == s - k
    # and back: the zero t-link again, the first cut
    g.edit_tweights(int(np.ravel_multi_index(vox, shape)), 0.0, 0.0)
    _assert_cut(g, flow0, lab0)
    g.close()


# ---- 6. clear --------------------------------------------------------------------------------------------------------------------
def test_clear_forgets_the_store():
    from medpy_amd import _lib
    shape = (17, 9, 10)
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    g = _handle(shape, None, nw, [_tweights(shape, 5), _tweights(shape, 6)], fg, bg)
    g.maxflow()
    bytes1 = g.stats()["device_bytes"]
    g._clear_tweights()
    assert g.tweight_edit_info() == {"store_held": 0, "dense_calls": 0, "list_entries": 0, "voxels_changed": 0}
    n = int(np.prod(shape))
    assert bytes1 - g.stats()["device_bytes"] == 8 * (2 * n + (n + 4095) // 4096 + 1)   # the store was counted, and is given back
    with pytest.raises(_lib.MedpyHipError) as ei:   # unbuilt
        g.maxflow()
    assert ei.value.code == _lib.ERR_STATE
    g._build()
    _assert_cut(g, *_bk(("clear", shape), shape, nw, (), fg, bg))
    g.close()


# ---- 7. the schedule of a regional term -------------------------------------------------------------------------------------------
def test_a_store_filled_by_dense_calls_is_scheduled_like_a_probability_map():
    """mgc_maxflow picks the 26-neighbourhood schedule of a pre-pushed graph for a probability map; a store that dense calls filled
    is the same kind of graph and launches the same kernel forms, a store that only a list edit filled those of its markers graph"""
    shape, conn = (9, 10, 11), 26
    nw = _nweights(shape, conn)
    fg, bg = _markers(shape)
    p = np.random.default_rng(7).random(shape).astype(np.float32)

    def kinds(g):
        g.maxflow()
        out = {k for k, v in g.launch_counts().items() if v}
        g.close()
        return out
    with_map = kinds(_handle(shape, conn, nw, (), fg, bg, prob=(p, 3.0)))
    dense = kinds(_handle(shape, conn, nw, [(p * np.float32(3.0), (1 - p) * np.float32(3.0))], fg, bg))
    plain = kinds(_handle(shape, conn, nw, (), fg, bg))
    edited = _handle(shape, conn, nw, (), fg, bg)
    edited.edit_tweights(0, 0.0, 0.0)
    assert edited.tweight_edit_info()["store_held"] == 1 and edited.tweight_edit_info()["dense_calls"] == 0
    print("map", sorted(with_map), "dense", sorted(dense), "markers", sorted(plain))
    assert dense == with_map
    assert kinds(edited) == plain

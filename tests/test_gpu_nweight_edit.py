"""-m gpu: edits of n-links by arc list (VoxelGraph.edit_nweights / clear_nweight_edits / nweight_edit_info, C ABI
mgc_edit_nweights / mgc_clear_nweight_edits / mgc_get_nweight_edit_info; DESIGN 10, "Edits of n-links by list") against the BK oracle.

As in test_gpu_dense_nweights.py the weights are drawn from uniform(0.1, 10) -- continuous, so the minimum cut is unique and the
labels must equal BK's voxel for voxel -- the oracle is oracle.bk.BKGraph fed with index lists built in NumPy, the flow is held to
rel 1e-9 and every violation count of mgc_validate to zero; the two conservation errors are held to 1e-9, the bound of the
boundary-update tests.  The edit is applied to the weight arrays in NumPy (`_apply`) and BK cuts the edited arrays."""
import itertools

import numpy as np
import pytest

from oracle import bk

pytestmark = pytest.mark.gpu

MAX = 65535.0  # GCGraph.MAX
CASES = [((17, 9, 10), None), ((9, 10), 4), ((9, 10), 8), ((9, 10, 11), 26), ((1, 1, 17), None), ((3, 1, 5), None), ((20, 18, 19), None)]
CASE_IDS = ["x".join(map(str, s)) + "_n%d" % (c or 2 * len(s)) for s, c in CASES]
_REF = {}


# ---- the lattice in NumPy (the helpers of test_gpu_dense_nweights.py) ---------------------------------------------------------------
def _offsets(ndim, conn):
    """the forward half of the neighbourhood: every arc pair once"""
    if conn in (None, 2 * ndim):
        return [tuple(1 if k == a else 0 for k in range(ndim)) for a in range(ndim)]
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if o > (0,) * ndim]


def _neg(off):
    return tuple(-o for o in off)


def _arcs(shape, off):
    """(mask of the voxels p with p + off inside, ids of those p, ids of p + off)"""
    ids = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, shape))
    dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, shape))
    mask = np.zeros(shape, bool)
    mask[src] = True
    return mask, ids[src].ravel(), ids[dst].ravel()


def _markers(shape):
    """a small box of fg near the low corner, the far face along the last axis as bg"""
    fg = np.zeros(shape, bool)
    bg = np.zeros(shape, bool)
    fg[_fg_box(shape)] = True
    bg[..., -1] = True
    return fg, bg


def _fg_box(shape):
    return tuple(slice(n // 3, n // 3 + 2) for n in shape[:-1]) + (slice(1, 3),)


def _weights(shape, conn, seed):
    """{offset: (there, back)} for the forward offsets, float64"""
    rng = np.random.default_rng(seed)
    return {o: (rng.uniform(0.1, 10.0, shape), rng.uniform(0.1, 10.0, shape)) for o in _offsets(len(shape), conn)}


def _bk_cut(shape, weights, fg, bg, tweights=None):
    """(flow, labels) of BK on the lattice arcs of `weights`, t-links `tweights` (src, snk) first, the markers last (generate.py:159-172)"""
    n = int(np.prod(shape))
    g = bk.BKGraph(n, n * 13 + 16)
    if tweights is not None:
        g.add_tweights(None, tweights[0].ravel(), tweights[1].ravel())
    for o, (there, back) in weights.items():
        mask, i, j = _arcs(shape, o)
        g.sum_edges(i, j, np.asarray(there, dtype=np.float64)[mask], np.asarray(back, dtype=np.float64)[mask])
    for m, (s, t) in ((fg, (MAX, 0.0)), (bg, (0.0, MAX))):
        idx = np.flatnonzero(m.ravel())
        if idx.size:
            g.add_tweights(idx, np.full(idx.size, s), np.full(idx.size, t))
    flow = g.maxflow()
    return flow, g.labels().astype(bool).reshape(shape)


def _ref(key, shape, weights, fg, bg, tweights=None):
    """a reference cut, computed once per module and key"""
    if key not in _REF:
        _REF[key] = _bk_cut(shape, weights, fg, bg, tweights)
    return _REF[key]


def _handle(shape, conn, weights, fg, bg, build=True):
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph(shape, connectivity=conn)
    g._set_markers(fg, bg)
    for o, (there, back) in weights.items():
        g._add_nweights(o, there, back)
    if build:
        g._build()
    return g


def _assert_cut(g, flow_ref, labels_ref):
    from medpy_amd import _lib
    flow = g.maxflow()
    labels = g.labels()
    v = g.validate()
    print("flow %r (BK %r), %d voxels differ, pair error %.3g, node error %.3g"
          % (flow, flow_ref, int((labels != labels_ref).sum()), v["max_pair_error"], v["max_node_error"]))
    np.testing.assert_array_equal(labels, labels_ref)
    assert flow == pytest.approx(flow_ref, rel=1e-9, abs=1e-300)
    assert not any(v[k] for k in _lib.VIOLATION_KEYS), v
    assert v["max_pair_error"] <= 1e-9 and v["max_node_error"] <= 1e-9, v
    return flow


# ---- edits in NumPy -----------------------------------------------------------------------------------------------------------------
def _apply(shape, weights, i, j, cap, rev):
    """the edit on copies of the weight arrays: the arc i[k] -> j[k] gets cap[k], the arc j[k] -> i[k] gets rev[k]"""
    out = {o: (t.astype(np.float64).copy(), b.astype(np.float64).copy()) for o, (t, b) in weights.items()}
    i, j = np.atleast_1d(i), np.atleast_1d(j)
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), i.shape)
    rev = np.broadcast_to(np.asarray(rev, dtype=np.float64), i.shape)
    ci, cj = np.stack(np.unravel_index(i, shape), 1), np.stack(np.unravel_index(j, shape), 1)
    for k in range(i.size):
        o = tuple(int(v) for v in cj[k] - ci[k])
        if o in out:
            out[o][0][tuple(ci[k])], out[o][1][tuple(ci[k])] = cap[k], rev[k]
        else:
            out[_neg(o)][0][tuple(cj[k])], out[_neg(o)][1][tuple(cj[k])] = rev[k], cap[k]
    return out


def _capacity(shape, weights, i, j):
    """capacities of the arcs i[k] -> j[k] in the arrays"""
    ci, cj = np.stack(np.unravel_index(i, shape), 1), np.stack(np.unravel_index(j, shape), 1)
    out = np.empty(len(i))
    for k in range(len(i)):
        o = tuple(int(v) for v in cj[k] - ci[k])
        out[k] = weights[o][0][tuple(ci[k])] if o in weights else weights[_neg(o)][1][tuple(cj[k])]
    return out


def _leaving(shape, conn, inside, open_axis=None):
    """(i, j): the arcs from a voxel of the mask `inside` to a neighbour outside it; with `open_axis`, all but those whose head lies
    beyond the mask's low end on that axis (the face that stays open)"""
    flat = inside.ravel()
    low = None if open_axis is None else int(np.argwhere(inside)[:, open_axis].min())
    ii, jj = [], []
    for o in _offsets(len(shape), conn):
        for off in (o, _neg(o)):
            _, i, j = _arcs(shape, off)
            sel = flat[i] & ~flat[j]
            if low is not None:
                sel &= np.unravel_index(j, shape)[open_axis] >= low
            ii.append(i[sel])
            jj.append(j[sel])
    return np.concatenate(ii), np.concatenate(jj)


def _dilated_fg_box(shape):
    """the fg box with one voxel around it, clipped to the volume, but tight on the side of the bg face (so that the smallest volumes
    keep a voxel between the box and that face); the axis whose low face stays open (the first of extent > 1)"""
    inside = np.zeros(shape, bool)
    inside[tuple(slice(max(0, n // 3 - 1), n // 3 + 3) for n in shape[:-1]) + (slice(0, 3),)] = True
    return inside, next(k for k, n in enumerate(shape) if n > 1)


def _edit_for(kind, shape, conn, w, labels0):
    """the three edits of test 1 as (i, j, cap, rev)"""
    inside, open_axis = _dilated_fg_box(shape)
    if kind == "barrier":     # both ways 0 on every arc that leaves the box, but for one face
        i, j = _leaving(shape, conn, inside, open_axis)
        return i, j, np.zeros(i.size), np.zeros(i.size)
    if kind == "one_way":     # the same arcs given from outside: the way in keeps its capacity, the way out (rev) is 0
        j, i = _leaving(shape, conn, inside, open_axis)
        return i, j, _capacity(shape, w, i, j), np.zeros(i.size)
    # glue: the arcs the first cut crosses, both ways x 100
    i, j = _leaving(shape, conn, labels0)
    return i, j, 100.0 * _capacity(shape, w, i, j), 100.0 * _capacity(shape, w, j, i)


# ---- 1. a barrier, one-way arcs and glue on a dense-store handle ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["barrier", "one_way", "glue"])
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_edit_on_a_dense_store_handle(shape, conn, kind):
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    flow0, labels0 = _ref(("cut", shape, conn), shape, w, fg, bg)
    i, j, cap, rev = _edit_for(kind, shape, conn, w, labels0)
    w1 = _apply(shape, w, i, j, cap, rev)
    flow1, labels1 = _ref(("cut", shape, conn, kind), shape, w1, fg, bg)
    flipped = np.flatnonzero(labels0.ravel() != labels1.ravel())
    assert i.size > 0 and flipped.size > 0   # (BK alone: the edit moves the cut)
    g = _handle(shape, conn, w, fg, bg)
    _assert_cut(g, flow0, labels0)
    before = g.labels().copy()
    g.edit_nweights(i, j, cap, rev)
    info = g.nweight_edit_info()
    print(kind, "arcs", i.size, info)
    assert info["pairs_kept"] == i.size and info["pairs_changed"] == i.size
    _assert_cut(g, flow1, labels1)
    assert np.array_equal(g.changed_labels(), flipped)
    assert np.array_equal(g.labels(out=before), labels1)
    g.close()


# ---- 2. a handle whose capacities the image determines --------------------------------------------------------------------------------
def _image_graph(shape, conn, regional):
    from medpy_amd import graphcut
    rng = np.random.default_rng(61)
    image = rng.normal(0.0, 10.0, shape).astype(np.float32)
    fg, bg = _markers(shape)
    kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(image, 20.0, False))
    tw = None
    if regional:
        prob = rng.uniform(0.0, 1.0, shape)   # float64: the t-links are prob * alpha and (1 - prob) * alpha in double
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(prob, 2.0))
        tw = (prob * 2.0, (1.0 - prob) * 2.0)
    if conn:
        kw["connectivity"] = conn
    return graphcut.graph_from_voxels(fg, bg, **kw), image, fg, bg, tw


def _read_weights(g, shape, conn):
    """{offset: (there, back)} as the graph returns them; NaN outside the volume is replaced by 0 (BK never reads those entries)"""
    out = {}
    for o in _offsets(len(shape), conn):
        there = g.nweights_offset(o)
        back_at_head = g.nweights_offset(_neg(o))   # [q] = arc q -> q - o
        back = np.full(shape, np.nan)
        src = tuple(slice(max(0, -v), n - max(0, v)) for v, n in zip(o, shape))
        dst = tuple(slice(max(0, v), n - max(0, -v)) for v, n in zip(o, shape))
        back[src] = back_at_head[dst]
        mask = _arcs(shape, o)[0]
        assert np.array_equal(np.isnan(there), ~mask) and np.array_equal(np.isnan(back), ~mask)
        out[o] = (np.nan_to_num(there), np.nan_to_num(back))
    return out


@pytest.mark.parametrize("regional", [False, True], ids=["markers", "regional"])
@pytest.mark.parametrize("shape,conn", [((17, 9, 10), None), ((9, 10, 11), 26)], ids=["17x9x10_n6", "9x10x11_n26"])
def test_edit_on_an_image_term_handle(shape, conn, regional):
    from medpy_amd import _lib, graphcut
    g, image, fg, bg, tw = _image_graph(shape, conn, regional)
    ndir = 26 if conn == 26 else 2 * len(shape)
    ntiles = int(np.prod([(n + 7) // 8 for n in shape]))
    w = _read_weights(g, shape, conn)
    _assert_cut(g, *_bk_cut(shape, w, fg, bg, tw))
    bytes0 = g.stats()["device_bytes"]
    # a barrier around the fg box but for one face, and three arcs of the voxel in the far corner raised
    inside, open_axis = _dilated_fg_box(shape)
    i, j = _leaving(shape, conn, inside, open_axis)
    far = int(np.prod(shape)) - 1
    i2 = np.array([far, far, far])
    j2 = np.array([far - 1, far - shape[-1], far - shape[-1] * shape[-2]])
    cap = np.concatenate([np.zeros(i.size), [3.5, 0.25, 7.0]])
    rev = np.concatenate([np.zeros(i.size), [0.0, 0.25, 1e-3]])
    i, j = np.concatenate([i, i2]), np.concatenate([j, j2])
    w1 = _apply(shape, w, i, j, cap, rev)
    edited = {(int(a), int(b)) for a, b in zip(i, j)} | {(int(b), int(a)) for a, b in zip(i, j)}
    # untouched arcs, as get_edge (the residual) saw them before the edit: a handful around the edit and across the volume
    rng = np.random.default_rng(3)
    picks = []
    for o in _offsets(len(shape), conn):
        _, a, b = _arcs(shape, o)
        for k in rng.choice(a.size, 6, replace=False):
            if (int(a[k]), int(b[k])) not in edited:
                picks += [(int(a[k]), int(b[k])), (int(b[k]), int(a[k]))]
    seen = {p: g.get_edge(*p) for p in picks}
    g.edit_nweights(i, j, cap, rev)
    snapshot = int(np.prod(shape))   # the handle held a finished solve: its labels are put aside as well, one byte per voxel (the snapshot rule)
    assert g.stats()["device_bytes"] - bytes0 - snapshot == 8 * ndir * ntiles * 512
    # the capacities as built: the edited values bit for bit, every other arc bit for bit what it was (the fill against mgc_built_capacity)
    got = _read_weights(g, shape, conn)
    for o in w1:
        assert np.array_equal(got[o][0], w1[o][0]) and np.array_equal(got[o][1], w1[o][1]), o
    for p in picks:
        assert g.get_edge(*p) == seen[p], p
    for a, b, c, r in zip(i, j, cap, rev):   # residuals of the edited pairs: inside the new pair of capacities, 0 on a barrier
        rab, rba = g.get_edge(int(a), int(b)), g.get_edge(int(b), int(a))
        assert 0.0 <= rab <= c + r and 0.0 <= rba <= c + r and rab + rba == pytest.approx(c + r, rel=1e-9, abs=0.0)
    flow1 = _assert_cut(g, *_bk_cut(shape, w1, fg, bg, tw))
    labels1 = g.labels().copy()
    # the handle holds its capacities now: update_boundary_term is refused and leaves everything as it was
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.update_boundary_term(graphcut.energy_voxel.boundary_difference_exponential, (None, 10.0, False))
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    assert g.maxflow() == flow1 and np.array_equal(g.labels(), labels1)
    g.close()


@pytest.mark.parametrize("shape,conn,ndir,ntiles", [((17, 9, 10), None, 6, 12), ((9, 10, 11), 26, 26, 8)], ids=["17x9x10_n6", "9x10x11_n26"])
def test_what_the_first_edit_allocates(shape, conn, ndir, ntiles):
    """never solved: the capacities as built, 8 * ndir * ntiles * 512 bytes, and nothing else; the first edit that finds a finished
    solve adds the label snapshot, one byte per voxel; later edits allocate nothing"""
    g, image, fg, bg, tw = _image_graph(shape, conn, False)
    bytes0 = g.stats()["device_bytes"]
    g.edit_nweights(0, 1, 0.0)
    assert g.stats()["device_bytes"] - bytes0 == 8 * ndir * ntiles * 512
    g.maxflow()
    g.edit_nweights(0, 1, 1.0)
    assert g.stats()["device_bytes"] - bytes0 == 8 * ndir * ntiles * 512 + int(np.prod(shape))
    g.maxflow()
    g.edit_nweights(0, 1, 2.0, 0.0)
    assert g.stats()["device_bytes"] - bytes0 == 8 * ndir * ntiles * 512 + int(np.prod(shape))
    g.close()


# ---- 3. where the kernel can go wrong -------------------------------------------------------------------------------------------------
def test_three_arcs_of_one_voxel_in_one_call():
    shape, conn = (17, 9, 10), None
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    g = _handle(shape, conn, w, fg, bg)
    g.maxflow()
    v = int(np.ravel_multi_index((7, 4, 3), shape))   # beside the fg box, in the corner layer of its tile: the +z arc crosses a tile face
    i = np.array([v, v, v])
    j = np.array([v + 1, v + shape[2], v + shape[1] * shape[2]])
    cap, rev = np.array([0.0, 0.0, 0.0]), np.array([0.0, 12.5, 0.0])
    g.edit_nweights(i, j, cap, rev)
    assert g.nweight_edit_info()["pairs_changed"] == 3
    _assert_cut(g, *_bk_cut(shape, _apply(shape, w, i, j, cap, rev), fg, bg))
    g.close()


def test_a_pair_across_a_tile_corner():
    shape, conn = (9, 10, 11), 26
    w = _weights(shape, conn, 23)
    fg = np.zeros(shape, bool)
    bg = np.zeros(shape, bool)
    fg[5:8, 5:8, 5:8] = True     # the source fills the corner of the first tile ...
    bg[8, 8:, 8:] = True         # ... the sink sits in the tile diagonally across: (7, 7, 7) -> (8, 8, 8) is the shortest way
    a, b = int(np.ravel_multi_index((7, 7, 7), shape)), int(np.ravel_multi_index((8, 8, 8), shape))
    g = _handle(shape, conn, w, fg, bg)
    flow0 = g.maxflow()
    labels0 = g.labels().copy()
    assert g.get_edge(a, b) == 0.0   # (saturated: the arc from a marked voxel to a marked voxel carries all it can)
    g.edit_nweights(a, b, 0.0, 0.0)
    info = g.nweight_edit_info()
    assert info["pairs_changed"] == 1 and info["arcs_clamped"] == 2 and info["voxels_changed"] == 2, info
    flow1 = _assert_cut(g, *_bk_cut(shape, _apply(shape, w, [a], [b], 0.0, 0.0), fg, bg))
    assert flow1 == pytest.approx(flow0 - w[(1, 1, 1)][0][7, 7, 7], rel=1e-9)
    g.edit_nweights(b, a, 2.0, 400.0)   # the other way round: b -> a gets 2, a -> b gets 400
    flow2 = _assert_cut(g, *_bk_cut(shape, _apply(shape, w, [a], [b], 400.0, 2.0), fg, bg))
    assert flow2 == pytest.approx(flow1 + 400.0, rel=1e-9)
    assert np.array_equal(g.labels(), labels0)   # both ends are markers: the labels never move
    g.close()


def test_a_tile_without_flags_gains_a_sink_link():
    shape, conn = (20, 18, 19), None
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    g = _handle(shape, conn, w, fg, bg)
    g.maxflow()
    labels = g.labels()
    tile = (slice(0, 8), slice(0, 8), slice(8, 16))   # the tile between the fg box (x 1..2) and the bg face (x 18), on their straight line: no marker, no t-link, so no flag
    mfg, mbg = g.markers()
    assert not mfg[tile].any() and not mbg[tile].any() and not g.tweights()[tile].any()
    # the arc inside the tile, between two voxels on the sink side, that carries the most flow (get_edge: the residual)
    best = (0.0, None)
    ids = np.arange(int(np.prod(shape))).reshape(shape)
    for z, y in itertools.product(range(0, 8), range(0, 8)):
        for x in range(8, 15):
            a, b = int(ids[z, y, x]), int(ids[z, y, x + 1])
            if labels[z, y, x] or labels[z, y, x + 1]:
                continue
            f = w[(0, 0, 1)][0][z, y, x] - g.get_edge(a, b)
            if f > best[0]:
                best = (f, (a, b))
    f, (a, b) = best
    assert f > 1e-3   # the flow of the fg box crosses this tile on its way to the bg face
    g.edit_nweights(a, b, 0.0, 0.0)
    info = g.nweight_edit_info()
    # the tail takes the flow back as excess, the head owes it: sink > 0 on a voxel of a tile that had neither plane valid
    assert info["arcs_clamped"] == 2 and info["voxels_changed"] == 2, info
    _assert_cut(g, *_bk_cut(shape, _apply(shape, w, [a], [b], 0.0, 0.0), fg, bg))
    g.close()


@pytest.mark.parametrize("shape,conn", [((17, 9, 10), None), ((9, 10, 11), 26), ((1, 1, 17), None)], ids=["17x9x10_n6", "9x10x11_n26", "1x1x17_n6"])
def test_edit_on_a_built_never_solved_handle(shape, conn):
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    flow0, labels0 = _ref(("cut", shape, conn), shape, w, fg, bg)
    i, j, cap, rev = _edit_for("barrier", shape, conn, w, labels0)
    g = _handle(shape, conn, w, fg, bg)
    g.edit_nweights(i, j, cap, rev)
    info = g.nweight_edit_info()
    assert info["pairs_changed"] == i.size and info["arcs_clamped"] == 0 and info["voxels_changed"] == 0, info   # no flow yet: nothing to clamp
    for a, b in list(zip(i, j))[:4]:
        assert g.get_edge(int(a), int(b)) == 0.0 and g.get_edge(int(b), int(a)) == 0.0   # before maxflow() the residual IS the capacity
    _assert_cut(g, *_ref(("cut", shape, conn, "barrier"), shape, _apply(shape, w, i, j, cap, rev), fg, bg))
    from medpy_amd import _lib
    with pytest.raises(_lib.MedpyHipError) as ei:   # no solve was held when the edit came: no snapshot
        g.changed_labels()
    assert ei.value.code == _lib.ERR_STATE
    g.close()


def test_an_edit_that_changes_nothing_bitwise():
    shape, conn = (17, 9, 10), None
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    flow0, labels0 = _ref(("cut", shape, conn), shape, w, fg, bg)
    g = _handle(shape, conn, w, fg, bg)
    flow = _assert_cut(g, flow0, labels0)
    i, j = _leaving(shape, conn, _dilated_fg_box(shape)[0])
    g.edit_nweights(i, j, _capacity(shape, w, i, j), _capacity(shape, w, j, i))
    info = g.nweight_edit_info()
    assert info["pairs_kept"] == i.size and info["pairs_changed"] == 0 and info["arcs_clamped"] == 0 and info["voxels_changed"] == 0, info
    assert g.maxflow() == flow and np.array_equal(g.labels(), labels0)
    assert g.changed_labels().size == 0
    g.edit_nweights(np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0))   # n == 0: not even the solve is dropped
    assert g.nweight_edit_info() == info and g.changed_labels().size == 0
    g.close()


@pytest.mark.parametrize("shape,conn", [((20, 18, 19), None), ((9, 10, 11), 26)], ids=["20x18x19_n6", "9x10x11_n26"])
def test_chain_of_five_edits(shape, conn):
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    g = _handle(shape, conn, w, fg, bg)
    _assert_cut(g, *_ref(("cut", shape, conn), shape, w, fg, bg))
    rng = np.random.default_rng(7)
    pairs = np.concatenate([np.stack(_arcs(shape, o)[1:], 1) for o in _offsets(len(shape), conn)])
    for step in range(5):
        labels_before = g.labels().copy()
        # 40 random pairs of the whole volume: a third barriers, a third one-way, a third raised; later steps hit earlier pairs again
        sel = pairs[rng.choice(len(pairs), 40, replace=False)]
        kinds = rng.integers(0, 3, 40)
        cap = np.where(kinds == 0, 0.0, np.where(kinds == 1, rng.uniform(0.1, 10.0, 40), rng.uniform(10.0, 50.0, 40)))
        rev = np.where(kinds == 2, rng.uniform(10.0, 50.0, 40), 0.0)
        w = _apply(shape, w, sel[:, 0], sel[:, 1], cap, rev)
        g.edit_nweights(sel[:, 0], sel[:, 1], cap, rev)
        if step == 3:   # two edits without a solve between them: the snapshot spans both
            more = pairs[rng.choice(len(pairs), 40, replace=False)]
            w = _apply(shape, w, more[:, 0], more[:, 1], 0.0, 0.0)
            g.edit_nweights(more[:, 0], more[:, 1], 0.0)
        flow, labels = _bk_cut(shape, w, fg, bg)
        _assert_cut(g, flow, labels)
        assert np.array_equal(g.changed_labels(), np.flatnonzero(labels_before.ravel() != labels.ravel()))
    g.close()


# ---- 4. refusals leave the handle as it was -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,conn", [((17, 9, 10), None), ((9, 10), 8)], ids=["17x9x10_n6", "9x10_n8"])
def test_refusals_leave_the_handle_as_it_was(shape, conn):
    from medpy_amd import _lib
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    g = _handle(shape, conn, w, fg, bg)
    flow = g.maxflow()
    g.edit_nweights(0, 1, 3.0, 4.0)   # (so that the list and the info hold something)
    flow = g.maxflow()
    labels = g.labels().copy()
    info = g.nweight_edit_info()
    last = _offsets(len(shape), conn)[-1]
    caps, residual = g.nweights_offset(last).copy(), g.get_edge(2, 3)
    n = int(np.prod(shape))
    step = shape[-1]
    good_i, good_j = [2, 3], [3, 4]
    bad = [("id == nvox", (n, 0), (1.0, 1.0), _lib.ERR_INVALID),
           ("negative id", (5, -1), (1.0, 1.0), _lib.ERR_INVALID),
           ("not neighbours", (5, 7), (1.0, 1.0), _lib.ERR_UNSUPPORTED),
           ("i == j", (5, 5), (1.0, 1.0), _lib.ERR_UNSUPPORTED),
           ("negative capacity", (5, 6), (-1.0, 1.0), _lib.ERR_INVALID),
           ("infinite capacity", (5, 6), (1.0, np.inf), _lib.ERR_INVALID),
           ("NaN capacity", (5, 6), (np.nan, 1.0), _lib.ERR_INVALID),
           ("pair twice", (3, 2), (1.0, 1.0), _lib.ERR_INVALID)]
    if conn is None:
        bad.append(("a diagonal in the 6-neighbourhood", (5, 6 + step), (1.0, 1.0), _lib.ERR_UNSUPPORTED))
    for what, (a, b), (c, r), code in bad:
        with pytest.raises(_lib.MedpyHipError) as ei:
            g.edit_nweights(good_i + [a], good_j + [b], [0.0, 0.0, c], [0.0, 0.0, r])
        assert ei.value.code == code, what
        assert "entry 2" in str(ei.value), (what, str(ei.value))
        assert g.nweight_edit_info() == info, what
        assert g.maxflow() == flow and np.array_equal(g.labels(), labels), what
        assert g.get_edge(2, 3) == residual and np.array_equal(g.nweights_offset(last), caps, equal_nan=True), what
    with pytest.raises(ValueError):
        g.edit_nweights([0, 1], [1, 2, 3], 1.0)
    g.close()


def test_state_errors():
    from medpy_amd import _lib
    from medpy_amd.graphcut import VoxelGraph
    shape = (17, 9, 10)
    w = _weights(shape, None, 23)
    fg, bg = _markers(shape)
    g = _handle(shape, None, w, fg, bg, build=False)
    with pytest.raises(_lib.MedpyHipError) as ei:   # before mgc_build
        g.edit_nweights(0, 1, 0.0)
    assert ei.value.code == _lib.ERR_STATE
    assert g.nweight_edit_info()["pairs_kept"] == 0
    g._build()
    _assert_cut(g, *_ref(("cut", shape, None), shape, w, fg, bg))
    g.close()


def _sphere_graph(s):
    from medpy_amd import graphcut
    return graphcut.graph_from_voxels(s["fg"], s["bg"], boundary_term=getattr(graphcut.energy_voxel, "boundary_" + s["term"]),
                                      boundary_term_args=(s["image"], s["sigma"], False))


def test_no_edit_after_a_solve_that_did_not_converge():
    from medpy_amd import _lib, synthetic
    s = synthetic.sphere((96, 96, 96))   # (the volume test_gpu_warm_resolve.py stops after one outer round)
    g = _sphere_graph(s)
    g.set_param("max_outer", 1)
    with pytest.raises(_lib.MedpyHipError):
        g.maxflow()
    bytes0 = g.stats()["device_bytes"]
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.edit_nweights(0, 1, 0.0)
    assert ei.value.code == _lib.ERR_STATE and g.nweight_edit_info()["pairs_kept"] == 0 and g.stats()["device_bytes"] == bytes0
    g.set_param("max_outer", 100000)
    g._build()   # (the refused call left the inputs alone: the rebuild is the graph of the image)
    cold = _sphere_graph(s)
    assert g.maxflow() == cold.maxflow() and np.array_equal(g.labels(), cold.labels())
    g.close()
    cold.close()


def test_slab_handles_are_rebuilt_not_edited():
    from medpy_amd import _lib, synthetic
    from medpy_amd.slab import HipSlab, LoopbackExchange, solve_slabs, sync_boundary_table
    s = synthetic.sphere((32, 24, 24))
    slabs = [HipSlab(s["image"].shape, r, 2) for r in range(2)]
    for sl in slabs:
        planes = slice(sl.plane0, sl.plane1)
        sl.set_boundary(s["term"], s["image"][planes], s["sigma"], False)
        sl.set_markers(s["fg"][planes], s["bg"][planes])
    ex = LoopbackExchange(slabs)
    sync_boundary_table(slabs, ex)
    lib = _lib.load()
    i, j, cap = (np.array([0], np.int64), np.array([1], np.int64), np.array([0.0]))
    out = np.zeros(4, np.int64)
    for sl in slabs:
        sl.build()
        assert lib.mgc_edit_nweights(sl._h, 1, _lib.ptr(i), _lib.ptr(j), _lib.ptr(cap), None) == _lib.ERR_STATE
        assert b"slab" in lib.mgc_last_error(sl._h)
        assert lib.mgc_get_nweight_edit_info(sl._h, _lib.ptr(out)) == _lib.OK and not out.any()
    solve_slabs(slabs, ex)
    parts = [sl.finish() for sl in slabs]
    g = _sphere_graph(s)
    assert float(sum(p[1] for p in parts)) == pytest.approx(g.maxflow(), rel=1e-12)
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=0).astype(bool), g.labels())
    for sl in slabs:
        sl.close()


# ---- 5. persistence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,conn", [((17, 9, 10), None), ((9, 10, 11), 26)], ids=["17x9x10_n6", "9x10x11_n26"])
def test_edits_stay_with_the_handle(shape, conn):
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    flow0, labels0 = _ref(("cut", shape, conn), shape, w, fg, bg)
    i, j, cap, rev = _edit_for("barrier", shape, conn, w, labels0)
    w1 = _apply(shape, w, i, j, cap, rev)
    g = _handle(shape, conn, w, fg, bg)
    g.maxflow()
    g.edit_nweights(i, j, cap, rev)
    g.edit_nweights(i[:3], j[:3], 5.0, 0.5)   # a later edit of a pair replaces the earlier one
    w1 = _apply(shape, w1, i[:3], j[:3], 5.0, 0.5)
    assert g.nweight_edit_info()["pairs_kept"] == i.size
    _assert_cut(g, *_bk_cut(shape, w1, fg, bg))
    # new markers, warm: the barriers are part of the residual graph
    fg2 = fg.copy()
    fg2[tuple(n // 2 for n in shape[:-1]) + (shape[-1] // 2,)] = True
    ref2 = _bk_cut(shape, w1, fg2, bg)
    g.update_markers(fg2, bg)
    _assert_cut(g, *ref2)
    # a cold rebuild applies the list again, behind the dense store
    g._build()
    _assert_cut(g, *ref2)
    for o in w1:
        assert np.array_equal(np.nan_to_num(g.nweights_offset(o)), np.where(_arcs(shape, o)[0], w1[o][0], 0.0)), o
    # forgotten: the graph of the arrays as they were given
    g.clear_nweight_edits()
    assert g.nweight_edit_info()["pairs_kept"] == 0
    from medpy_amd import _lib
    with pytest.raises(_lib.MedpyHipError) as ei:   # unbuilt, as after mgc_clear_nweights
        g.maxflow()
    assert ei.value.code == _lib.ERR_STATE
    g._build()
    _assert_cut(g, *_bk_cut(shape, w, fg2, bg))
    g.close()


# ---- 6. the same state from the list and from scratch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_same_state_from_list_and_from_scratch(shape, conn):
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    flow0, labels0 = _ref(("cut", shape, conn), shape, w, fg, bg)
    i, j, cap, rev = _edit_for("one_way", shape, conn, w, labels0)
    w1 = _apply(shape, w, i, j, cap, rev)
    warm = _handle(shape, conn, w, fg, bg)
    warm.maxflow()
    warm.edit_nweights(i, j, cap, rev)
    cold = _handle(shape, conn, w1, fg, bg)
    flow = _assert_cut(warm, *_ref(("cut", shape, conn, "one_way"), shape, w1, fg, bg))
    assert cold.maxflow() == pytest.approx(flow, rel=1e-12, abs=1e-300)
    assert np.array_equal(warm.labels(), cold.labels())
    for o in _offsets(len(shape), conn):
        for off in (o, _neg(o)):
            assert np.array_equal(warm.nweights_offset(off), cold.nweights_offset(off), equal_nan=True), off
    warm.close()
    cold.close()

"""-m gpu: whole n-link weight arrays (mgc_add_nweights / GCGraph.set_nweights_dense) against the BK oracle.

Weights are drawn from uniform(0.1, 10): continuous, so the minimum cut is unique and the labels must equal BK's voxel for voxel,
without the tie relaxation of oracle/cutcheck.py.  The oracle is oracle.bk.BKGraph fed by sum_edges with index lists built in
NumPy; every reference cut is computed once per input and module and shared."""
import itertools

import numpy as np
import pytest

from oracle import bk, energy_numpy

pytestmark = pytest.mark.gpu

MAX = 65535.0  # GCGraph.MAX
CASES = [((9, 8, 7), None), ((1, 1, 17), None), ((3, 1, 5), None), ((17, 9, 10), None), ((9, 10), 4), ((9, 10), 8), ((9, 10, 11), 26)]
CASE_IDS = ["x".join(map(str, s)) + "_n%d" % (c or 2 * len(s)) for s, c in CASES]
_REF = {}


def _offsets(ndim, conn):
    """the forward half of the neighbourhood: every arc pair once"""
    if conn in (None, 2 * ndim):
        return [tuple(1 if k == a else 0 for k in range(ndim)) for a in range(ndim)]
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if o > (0,) * ndim]


def _arcs(shape, off):
    """(mask of the voxels p with p + off inside, ids of those p, ids of p + off)"""
    ids = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, shape))
    dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, shape))
    mask = np.zeros(shape, bool)
    mask[src] = True
    return mask, ids[src].ravel(), ids[dst].ravel()


def _shifted(shape, off, a):
    """out[p + off] = a[p] where both are inside, NaN elsewhere: what the read-back of the reverse offset must show"""
    out = np.full(shape, np.nan)
    src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, shape))
    dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, shape))
    out[dst] = np.asarray(a, dtype=np.float64)[src]
    return out


def _neg(off):
    return tuple(-o for o in off)


def _markers(shape):
    """a small box of fg near the low corner, the far face along the last axis as bg"""
    fg = np.zeros(shape, bool)
    bg = np.zeros(shape, bool)
    box = tuple(slice(n // 3, n // 3 + 2) for n in shape[:-1]) + (slice(1, 3),)
    fg[box] = True
    bg[..., -1] = True
    return fg, bg


def _weights(shape, conn, seed, dtype=np.float64, directed_half=False):
    """{offset: (there, back)} for the forward offsets"""
    rng = np.random.default_rng(seed)
    out = {}
    for o in _offsets(len(shape), conn):
        there = rng.uniform(0.1, 10.0, shape).astype(dtype)
        back = rng.uniform(0.1, 10.0, shape).astype(dtype)
        if directed_half:
            back[rng.random(shape) < 0.5] = 0.0
        out[o] = (there, back)
    return out


def _bk_cut(shape, weights, fg, bg, tweights=None, extra=None):
    """(flow, labels) of BK on the lattice arcs of `weights` ({offset: (there, back or None)}), t-links `tweights` (src, snk)
    first, the markers last (generate.py:159-172)"""
    n = int(np.prod(shape))
    g = bk.BKGraph(n, n * 13 + 16)
    if tweights is not None:
        g.add_tweights(None, tweights[0].ravel(), tweights[1].ravel())
    for o, (there, back) in weights.items():
        mask, i, j = _arcs(shape, o)
        cap = np.asarray(there, dtype=np.float64)[mask]
        rev = cap if back is None else np.asarray(back, dtype=np.float64)[mask]
        g.sum_edges(i, j, cap, rev)
    for i, j, cap, rev in extra or ():
        g.sum_edges(i, j, cap, rev)
    for m, (s, t) in ((fg, (MAX, 0.0)), (bg, (0.0, MAX))):
        idx = np.flatnonzero(m.ravel())
        if idx.size:
            g.add_tweights(idx, np.full(idx.size, s), np.full(idx.size, t))
    flow = g.maxflow()
    return flow, g.labels().astype(bool).reshape(shape)


def _handle(shape, conn, weights, fg=None, bg=None, symmetric=False):
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph(shape, connectivity=conn)
    if fg is not None:
        g._set_markers(fg, bg)
    for o, (there, back) in weights.items():
        g._add_nweights(o, there, None if symmetric else back)
    return g


def _large_volume_forms(g):
    from conftest import LARGE_VOLUME_FORMS
    for kv in LARGE_VOLUME_FORMS.split(","):
        k, v = kv.split("=")
        g.set_param(k, int(v))


def _assert_cut(g, flow_ref, labels_ref, rel=1e-9):
    flow = g.maxflow()
    print("flow %r (BK %r), %d voxels differ" % (flow, flow_ref, int((g.labels() != labels_ref).sum())))
    np.testing.assert_array_equal(g.labels(), labels_ref)
    assert flow == pytest.approx(flow_ref, rel=rel, abs=1e-300)
    v = g.validate()
    from medpy_amd import _lib
    assert not any(v[k] for k in _lib.VIOLATION_KEYS), v
    return flow


# ---- 1. round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_back", [True, False], ids=["back", "symmetric"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_round_trip_is_bit_identical(shape, conn, dtype, with_back):
    w = _weights(shape, conn, 11, dtype)
    g = _handle(shape, conn, w, symmetric=not with_back)
    g._build()
    crossed = 0
    for o, (there, back) in w.items():
        if not with_back:
            back = there
        mask, i, j = _arcs(shape, o)
        got = g.nweights_offset(o)
        assert np.array_equal(np.isnan(got), ~mask)
        assert np.array_equal(got[mask], there.astype(np.float64)[mask])
        got = g.nweights_offset(_neg(o))
        want = _shifted(shape, o, back)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
        # single arcs, those across a tile border (coordinate 7 -> 8) among them; before maxflow() the residual IS the capacity
        border = [k for k in range(i.size) if any(c == 7 and d == 1 for c, d in zip(np.unravel_index(i[k], shape), o))][:3]
        crossed += len(border)
        picks = border + ([0, i.size - 1] if i.size else [])   # (an offset along an axis of extent 1 has no arcs)
        for k in picks:
            assert g.get_edge(int(i[k]), int(j[k])) == float(there.ravel()[i[k]])
            assert g.get_edge(int(j[k]), int(i[k])) == float(back.ravel()[i[k]])
    assert crossed > 0 or max(shape) <= 8   # every shape beyond one tile had arcs across a tile border looked at


# ---- 2. the cut -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", ["as_shipped", "large_volume_forms"])
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_cut_equals_bk(shape, conn, forms):
    w = _weights(shape, conn, 23)
    fg, bg = _markers(shape)
    key = ("cut", shape, conn)
    if key not in _REF:
        _REF[key] = _bk_cut(shape, w, fg, bg)
    g = _handle(shape, conn, w, fg, bg)
    g._build()
    if forms == "large_volume_forms":
        _large_volume_forms(g)
    _assert_cut(g, *_REF[key])


# ---- 3. directed weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,conn", [((17, 9, 10), None), ((9, 10, 11), 26)], ids=["17x9x10_n6", "9x10x11_n26"])
def test_directed_weights(shape, conn):
    w = _weights(shape, conn, 37, directed_half=True)
    fg, bg = _markers(shape)
    g = _handle(shape, conn, w, fg, bg)
    g._build()
    _assert_cut(g, *_bk_cut(shape, w, fg, bg))
    assert g.launch_counts()["k_dt_axis"] == 0   # an arc of capacity 0 inside the volume: the relabel runs as passes


# ---- 4. every arc residual: the first relabel is the distance transform ------------------------------------------------------------
def test_all_positive_symmetric_graph_starts_with_the_distance_transform():
    shape = (17, 9, 10)
    w = _weights(shape, None, 41)
    fg, bg = _markers(shape)
    g = _handle(shape, None, w, fg, bg, symmetric=True)
    g._build()
    _assert_cut(g, *_bk_cut(shape, {o: (t, None) for o, (t, _) in w.items()}, fg, bg))
    assert g.launch_counts()["k_dt_axis"] > 0


# ---- 5. accumulation ---------------------------------------------------------------------------------------------------------------
def test_calls_accumulate_in_order_on_top_of_the_built_in_term():
    from medpy_amd.graphcut import VoxelGraph
    shape, off = (9, 8, 7), (1, 0, 0)
    rng = np.random.default_rng(53)
    image = rng.normal(0, 10, shape).astype(np.float32)

    def with_term():
        g = VoxelGraph(shape)
        g._set_boundary("difference_exponential", image, 15.0, False)
        return g

    g0 = with_term()
    g0._build()
    built, built_back = g0.nweights_offset(off), g0.nweights_offset(_neg(off))
    scales = (1e-8, 1e8, 1.0)   # sixteen orders of magnitude: (b + w1) + w2 + w3 differs from b + (w1 + w2 + w3) in the last bits
    there = [rng.uniform(0.1, 10.0, shape) * s for s in scales]
    back = [rng.uniform(0.1, 10.0, shape) * s for s in scales]
    g = with_term()
    for t, b in zip(there, back):
        g._add_nweights(off, t, b)
    g._build()
    mask, i, j = _arcs(shape, off)
    want = ((built + there[0]) + there[1]) + there[2]
    want_back = ((built_back + _shifted(shape, off, back[0])) + _shifted(shape, off, back[1])) + _shifted(shape, off, back[2])
    regrouped = built + ((there[0] + there[1]) + there[2])
    print("arcs where the order of the adds shows: %d of %d" % (int((want[mask] != regrouped[mask]).sum()), int(mask.sum())))
    got, got_back = g.nweights_offset(off), g.nweights_offset(_neg(off))
    assert np.array_equal(got[mask], want[mask]) and np.array_equal(np.isnan(got), ~mask)
    ok = ~np.isnan(want_back)
    assert np.array_equal(got_back[ok], want_back[ok]) and np.array_equal(np.isnan(got_back), ~ok)
    # an explicit batch on the same arcs, some of them twice: term, dense, list
    pick = rng.choice(i.size, 60, replace=False)
    ei, ej = np.concatenate([i[pick], i[pick[:20]]]), np.concatenate([j[pick], j[pick[:20]]])
    cap, rev = rng.uniform(0.1, 10.0, ei.size) * 1e-4, rng.uniform(0.1, 10.0, ei.size) * 1e4
    g._add_edges(ei, ej, cap, rev)
    g._build()
    want, want_back = want.ravel().copy(), want_back.ravel().copy()
    for k in range(ei.size):     # sum_edge, call by call
        want[ei[k]] += cap[k]
        want_back[ej[k]] += rev[k]
    got, got_back = g.nweights_offset(off).ravel(), g.nweights_offset(_neg(off)).ravel()
    assert np.array_equal(got[mask.ravel()], want[mask.ravel()])
    assert np.array_equal(got_back[ok.ravel()], want_back[ok.ravel()])


# ---- 6. with a regional term: the pre-push has moved flow before the store is applied --------------------------------------------------
@pytest.mark.parametrize("shape,conn", [((16, 16, 16), None), ((9, 10, 11), 26)], ids=["16x16x16_n6", "9x10x11_n26"])
def test_dense_weights_with_regional_term(shape, conn):
    from medpy_amd.graphcut import VoxelGraph
    rng = np.random.default_rng(61)
    image = rng.normal(0, 10, shape)
    prob, alpha, sigma = rng.uniform(0.0, 1.0, shape), 3.0, 7.0
    w = _weights(shape, conn, 67)
    fg, bg = _markers(shape)
    # the oracle: an arc's capacity is (weight of the division term) + (dense weight), the two adds of the device in the same order
    offs = _offsets(len(shape), conn)
    if conn is None:
        term_w = {o: (np.pad(a, [(0, 1) if k == ax else (0, 0) for k in range(len(shape))]), None)
                  for ax, (o, a) in enumerate(zip(offs, energy_numpy.boundary_weights("difference_division", image, sigma)))}
    else:
        tw = energy_numpy.boundary_weights_offsets("difference_division", image, offs, sigma)
        term_w = {o: (np.nan_to_num(np.asarray(tw[o])), None) for o in offs}
    summed = {o: (term_w[o][0] + w[o][0], term_w[o][0] + w[o][1]) for o in offs}
    ref = _bk_cut(shape, summed, fg, bg, tweights=energy_numpy.regional_probability_tweights(prob, alpha))
    g = VoxelGraph(shape, connectivity=conn)
    g._set_boundary("difference_division", image, sigma, False)
    g._set_regional(prob, alpha)
    g._set_markers(fg, bg)
    for o, (there, back) in w.items():
        g._add_nweights(o, there, back)
    g._build()
    for o in offs[:2]:   # the capacities as built are term + dense although the residuals already carry the pre-push
        mask = _arcs(shape, o)[0]
        assert np.array_equal(g.nweights_offset(o)[mask], summed[o][0][mask])
    _assert_cut(g, *ref)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_arrays_leave_the_handle_as_it_was():
    from medpy_amd import _lib
    from medpy_amd.graphcut import VoxelGraph
    shape = (9, 8, 7)
    rng = np.random.default_rng(71)
    image = rng.normal(0, 10, shape)
    w = _weights(shape, None, 73)
    fg, bg = _markers(shape)

    def with_term():
        g = VoxelGraph(shape)
        g._set_boundary("difference_division", image, 7.0, False)
        g._set_markers(fg, bg)
        return g

    g = with_term()
    for o, (there, back) in w.items():
        there, back = there.copy(), back.copy()
        there[~_arcs(shape, o)[0]] = np.nan   # ignored entries may hold anything
        back[~_arcs(shape, o)[0]] = np.nan
        g._add_nweights(o, there, back)
    g._build()
    before = {o: g.nweights_offset(o) for o in w}
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        for o in w:
            for into_back in (False, True):
                there, back = w[o][0].copy(), w[o][1].copy()
                pos = (4, 3, 2)   # not ignored for any forward axis offset
                (back if into_back else there)[pos] = bad
                flat = int(np.ravel_multi_index(pos, shape))
                with pytest.raises(_lib.MedpyHipError) as ei:
                    g._add_nweights(o, there, back)
                assert ei.value.code == _lib.ERR_INVALID
                assert "%s[%d]" % ("back" if into_back else "there", flat) in str(ei.value), str(ei.value)
    # two offenders: the first one in C order is named
    there = w[(1, 0, 0)][0].copy()
    there[5, 0, 0] = -2.0
    there[2, 7, 6] = np.nan
    with pytest.raises(_lib.MedpyHipError) as ei:
        g._add_nweights((1, 0, 0), there)
    assert "there[%d]" % int(np.ravel_multi_index((2, 7, 6), shape)) in str(ei.value), str(ei.value)
    # the handle is as it was: built, and the next build + solve are those of the accepted calls
    for o in w:
        assert np.array_equal(g.nweights_offset(o), before[o], equal_nan=True)
    g._build()
    term_w = {o: np.pad(a, [(0, 1) if k == ax else (0, 0) for k in range(3)])
              for ax, (o, a) in enumerate(zip(w, energy_numpy.boundary_weights("difference_division", image, 7.0)))}
    summed = {o: (term_w[o] + w[o][0], term_w[o] + w[o][1]) for o in w}
    _assert_cut(g, *_bk_cut(shape, summed, fg, bg))
    # without the store: the graph of the built-in term alone
    g._clear_nweights()
    g._build()
    g1 = with_term()
    g1._build()
    for o in w:
        assert np.array_equal(g.nweights_offset(o), g1.nweights_offset(o), equal_nan=True)
    assert g.maxflow() == pytest.approx(g1.maxflow(), rel=1e-12) and np.array_equal(g.labels(), g1.labels())


# ---- 8. rebuild and warm edit -------------------------------------------------------------------------------------------------------
def test_rebuild_and_warm_marker_edit():
    from medpy_amd import _lib
    shape = (17, 9, 10)
    w = _weights(shape, None, 83)
    fg, bg = _markers(shape)
    g = _handle(shape, None, w, fg, bg)
    g._build()
    f1 = g.maxflow()
    l1 = g.labels().copy()
    g._build()
    assert g.maxflow() == f1 and np.array_equal(g.labels(), l1)
    # a stroke: more foreground next to the far face, some background in the middle
    fg2, bg2 = fg.copy(), bg.copy()
    fg2[10:13, 4:6, 6:8] = True
    bg2[3:5, 1:3, 4:6] = True
    g.edit_markers(fg=np.flatnonzero((fg2 & ~fg).ravel()), bg=np.flatnonzero((bg2 & ~bg).ravel()))
    f2 = g.maxflow()
    cold = _handle(shape, None, w, fg2, bg2)
    cold._build()
    fc = cold.maxflow()
    assert np.array_equal(g.labels(), cold.labels())
    assert f2 == pytest.approx(fc, rel=1e-9)
    for h in (g, cold):
        v = h.validate()
        assert not any(v[k] for k in _lib.VIOLATION_KEYS), v
    assert np.array_equal(g.changed_labels(), np.flatnonzero((g.labels() != l1).ravel()))
    assert (g.labels() != l1).any()
    _assert_cut(cold, *_bk_cut(shape, w, fg2, bg2))


# ---- 9. the ready plug-in --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["skeleton", "full_shape_pairs"])
def test_boundary_precomputed_equals_the_built_in_term(layout):
    from medpy_amd import graphcut
    shape, sigma = (17, 9, 10), 7.0
    image = np.random.default_rng(97).normal(0, 10, shape)
    fg, bg = _markers(shape)
    ws = energy_numpy.boundary_weights("difference_division", image, sigma)   # the division term is bit-exact on the device
    if layout == "full_shape_pairs":
        ws = [(p, p.astype(np.float64).copy()) for p in
              (np.pad(a, [(0, 1) if k == ax else (0, 0) for k in range(3)], constant_values=np.nan) for ax, a in enumerate(ws))]
    g = graphcut.graph_from_voxels(fg, bg, boundary_term=graphcut.energy_voxel.boundary_precomputed, boundary_term_args=(ws,))
    ref = graphcut.graph_from_voxels(fg, bg, boundary_term=graphcut.energy_voxel.boundary_difference_division,
                                     boundary_term_args=(image, sigma, False))
    flow, flow_ref = g.maxflow(), ref.maxflow()
    assert np.array_equal(g.labels(), ref.labels())
    assert flow == pytest.approx(flow_ref, rel=1e-12)
    for axis in range(3):
        assert np.array_equal(g.nweights(axis), ref.nweights(axis))

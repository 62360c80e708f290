"""-m gpu: the source side of the minimum cut and the ambiguity set of a solved voxel graph (mgc_cut_sets; VoxelGraph.source_side /
ambiguous / cut_is_unique / cut_sets_info) against the BK oracle.

Every graph of sections 1 - 4 has small whole numbers (or dyadic fractions) for capacities, so all f64 arithmetic of either solver is
exact, and the sets R_s (reachable from the source) and R_t (can reach the sink) of the residual graph are the same for EVERY maximum
flow: the device's sets must equal ``oracle.cutcheck.ambiguity(bk_graph, tol=0.0)`` bit for bit, the cut around R_s must have exactly
the capacity maxflow() returned.  The generators make the two sets differ by a third of the volume (two walls of equal capacity: the
block between them is ambiguous) and plant directed pockets -- voxels that arcs only enter, or only leave -- which a flood that tests
the wrong end's mask bit gets wrong.  Section 5: floating-point graphs, solver-independent invariants only.  Every oracle cut is
computed once per input and shared."""
import ctypes
import itertools

import numpy as np
import pytest

from oracle import bk, cutcheck, pipeline

pytestmark = pytest.mark.gpu

_REF = {}


# ---- graphs ------------------------------------------------------------------------------------------------------------------------
def _offsets(ndim, conn):
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


def _shifted(m, off):
    """s[p] = m[p + off] (False where p + off is outside)"""
    s = np.zeros_like(m)
    src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, m.shape))
    dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, m.shape))
    s[src] = m[dst]
    return s


def walls_graph(shape, walls, seed, conn=None):
    """Two (or three) walls of EQUAL capacity across the last axis, directed pockets on both sides.  Returns (nw, source, sink):
    nw[offset] = (there, back), arrays of the volume's shape: there[p] the capacity of p -> p + offset, back[p] of p + offset -> p.
      interior axis arcs 4..8, both directions drawn on their own; diagonal arcs (full neighbourhood) 0..8
      the arcs crossing the planes between w and w + 1 of the last axis, w in walls: ONE array of 0..2 over the other axes, rolled by
        the wall's number along axis 0 -- every wall has the same capacity; diagonal arcs that cross such a plane: 0
      source weight 1000 on the first plane of the last axis, sink weight 1000 on the last
      3 % in-only voxels (every arc leaving them 0), 3 % out-only voxels (every arc entering them 0), none next to a wall or on an
        end plane
      2 % voxels with a source or a sink weight 1..3, outside the walls only"""
    rng = np.random.default_rng(seed)
    shape = tuple(shape)
    nd, last = len(shape), shape[-1]
    wall_cap = rng.integers(0, 3, shape[:-1]).astype(np.float64)
    nw = {}
    for o in _offsets(nd, conn):
        axis_arc = sum(1 for v in o if v) == 1
        lo, hi = (4, 9) if axis_arc else (0, 9)
        there = rng.integers(lo, hi, shape).astype(np.float64)
        back = rng.integers(lo, hi, shape).astype(np.float64)
        if o[-1]:
            for k, w in enumerate(walls):
                at = w if o[-1] > 0 else w + 1   # the arc p -> p + o crosses the plane between w and w + 1
                cap = (np.roll(wall_cap, k, axis=0) if nd > 1 else wall_cap) if axis_arc else 0.0
                there[..., at] = cap
                back[..., at] = cap
        nw[o] = (there, back)
    x = np.arange(last)
    free = (x > 0) & (x < last - 1)
    for w in walls:
        free &= (x != w) & (x != w + 1)
    free = np.broadcast_to(free, shape)
    kind = rng.random(shape)
    in_only, out_only = free & (kind < 0.03), free & (kind >= 0.03) & (kind < 0.06)
    for o, (there, back) in nw.items():
        there[in_only] = 0.0                      # p -> p + o leaves p
        back[_shifted(in_only, o)] = 0.0          # p + o -> p leaves p + o
        back[out_only] = 0.0                      # p + o -> p enters p
        there[_shifted(out_only, o)] = 0.0        # p -> p + o enters p + o
    source, sink = np.zeros(shape), np.zeros(shape)
    source[..., 0] = 1000.0
    sink[..., -1] = 1000.0
    outside = np.broadcast_to((x <= walls[0]) | (x > walls[-1]), shape)
    pick = outside & (rng.random(shape) < 0.02)
    pick[..., 0] = pick[..., -1] = False
    which = rng.random(shape) < 0.5
    weight = rng.integers(1, 4, shape).astype(np.float64)
    source[pick & which] = weight[pick & which]
    sink[pick & ~which] = weight[pick & ~which]
    return nw, source, sink


def snake_graph(shape, c, perm=(0, 1, 2), source=5.0, sink=3.0):
    """All arcs 0 except a directed snake (there = c, back = 0) that runs boustrophedon through every row of every layer of a volume of
    ``shape`` -- then the axes are permuted by ``perm``, so that between the two layouts used the path crosses tile faces in all six
    directions.  Source weight at the head, sink weight at the tail.  Returns (shape, nw, source, sink, path)."""
    a, b, n = shape
    path = []
    for z in range(a):
        rows = range(b) if z % 2 == 0 else range(b - 1, -1, -1)
        for r, y in enumerate(rows):
            fwd = (z * b + r) % 2 == 0
            for x in (range(n) if fwd else range(n - 1, -1, -1)):
                path.append((z, y, x))
    path = np.array(path)[:, list(perm)]      # axis k of the volume is axis perm[k] of the snake's own frame
    vshape = tuple(shape[k] for k in perm)
    nw = {o: (np.zeros(vshape), np.zeros(vshape)) for o in _offsets(3, None)}
    for p, q in zip(path[:-1], path[1:]):
        d = tuple(int(v) for v in (q - p))
        assert sum(abs(v) for v in d) == 1
        if sum(d) > 0:
            nw[d][0][tuple(p)] = c               # p -> p + e
        else:
            nw[tuple(-v for v in d)][1][tuple(q)] = c   # (q + e = p) -> q
    src, snk = np.zeros(vshape), np.zeros(vshape)
    src[tuple(path[0])] = source
    snk[tuple(path[-1])] = sink
    return vshape, nw, src, snk, path


def _bk(key, shape, nw, source, sink):
    """(flow, from_source, to_sink, ambiguous) of BK on the same arcs, each once per key"""
    if key not in _REF:
        n = int(np.prod(shape))
        g = bk.BKGraph(n, n * 13 + 16)
        g.add_tweights(None, np.asarray(source, np.float64).ravel(), np.asarray(sink, np.float64).ravel())
        for o, (there, back) in nw.items():
            mask, i, j = _arcs(shape, o)
            g.sum_edges(i, j, there[mask], back[mask])
        flow = g.maxflow()
        fs, ts, amb = cutcheck.ambiguity(g, tol=0.0)
        _REF[key] = (flow, fs.reshape(shape), ts.reshape(shape), amb.reshape(shape))
    return _REF[key]


def _handle(shape, conn, nw, source, sink):
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph(shape, connectivity=conn)
    for o, (there, back) in nw.items():
        g._add_nweights(o, there, back)
    g._add_tweights(source, sink)
    g._build()
    return g


def _assert_sets(g, ref, unique=None):
    """the device's sets against the oracle's, bit for bit; the counts, the capacity of the cut around R_s, cut_is_unique"""
    flow_ref, fs, ts, amb = ref
    flow = g.maxflow()
    got_fs, got_amb, labels, info = g.source_side(), g.ambiguous(), g.labels(), g.cut_sets_info()
    print("flow %r (BK %r) source_cut %r | from_source %d (BK %d) to_sink %d (BK %d) ambiguous %d (BK %d) | passes %d visits %d seeded %d skipped %d"
          % (flow, flow_ref, info["source_cut"], int(got_fs.sum()), int(fs.sum()), int((~labels).sum()), int(ts.sum()), int(got_amb.sum()), int(amb.sum()),
             info["flood_passes"], info["tile_visits"], info["tiles_seeded"], info["tiles_skipped"]))
    assert got_fs.dtype == np.bool_ and got_fs.shape == fs.shape and got_amb.dtype == np.bool_ and got_amb.shape == amb.shape
    assert flow == flow_ref
    np.testing.assert_array_equal(labels, ~ts)
    np.testing.assert_array_equal(got_fs, fs)
    np.testing.assert_array_equal(got_amb, amb)
    assert info["source_cut"] == flow
    assert (info["from_source"], info["to_sink"], info["ambiguous"]) == (int(got_fs.sum()), int((~labels).sum()), int(got_amb.sum()))
    assert g.cut_is_unique() == (int(amb.sum()) == 0)
    if unique is not None:
        assert g.cut_is_unique() is unique
    return info


# ---- 1. two equal walls with directed pockets ---------------------------------------------------------------------------------------
WALLS = [((20, 13, 27), (8, 17)), ((9, 10, 33), (7, 15, 24)), ((17, 17, 17), (5, 10)), ((8, 8, 8), (2, 4)), ((19, 26), (8, 16)), ((41,), (9, 20, 30))]
WALL_IDS = ["x".join(map(str, s)) for s, _ in WALLS]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape,walls", WALLS, ids=WALL_IDS)
def test_walls_and_pockets(shape, walls, seed):
    nw, source, sink = walls_graph(shape, walls, seed)
    ref = _bk(("walls", shape, seed), shape, nw, source, sink)
    g = _handle(shape, None, nw, source, sink)
    _assert_sets(g, ref, unique=False)
    if len(shape) > 1:   # (what makes the case a test: each of the three sets is a good part of the volume)
        n = float(np.prod(shape))
        assert min(ref[1].sum(), ref[2].sum(), ref[3].sum()) > 0.15 * n, [int(r.sum()) for r in ref[1:]]
    g.close()


# ---- 2. serpentine -----------------------------------------------------------------------------------------------------------------
SNAKE = (3, 34, 37)
LAYOUTS = {"rows_along_x": (0, 1, 2), "rows_along_z": (2, 1, 0)}


@pytest.mark.parametrize("c", [1, 2, 3, 7])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_serpentine(layout, c):
    """Source weight 5 at the head, sink weight 3 at the tail, every arc of the path c one way and 0 back.  c = 1, 2: the path is
    saturated, R_s is the head, R_t the tail, all between ambiguous; c = 3: the sink link is saturated too, R_t is empty.  In these
    three the source reaches nothing beyond the head, so the flood has nowhere to go; c = 7 is the variant in which it has: the
    sink link alone is saturated, R_s is the whole path, and the flood must follow it across some two hundred tile faces, through the
    reverse arcs as well (excess is stranded somewhere along the path).  Expected sets: the oracle's, always."""
    shape, nw, source, sink, path = snake_graph(SNAKE, float(c), LAYOUTS[layout])
    ref = _bk(("snake", layout, c), shape, nw, source, sink)
    flow_ref, fs, ts, amb = ref
    assert flow_ref == min(5.0, c, 3.0)
    head, tail = tuple(path[0]), tuple(path[-1])
    if c < 5:
        assert fs.sum() == 1 and fs[head] and int(ts.sum()) == (1 if c < 3 else 0) and (c == 3 or ts[tail])
    else:
        assert fs.all() and not ts.any()
    g = _handle(shape, None, nw, source, sink)
    info = _assert_sets(g, ref)
    if c >= 5:
        assert info["flood_passes"] > 1 and info["tile_visits"] > info["tiles_seeded"]
    g.close()


def test_no_source_weight_anywhere():
    shape, nw, source, sink, _ = snake_graph(SNAKE, 2.0)
    source[...] = 0.0
    ref = _bk(("snake", "no_source"), shape, nw, source, sink)
    g = _handle(shape, None, nw, source, sink)
    info = _assert_sets(g, ref)
    assert not g.source_side().any() and info["tile_visits"] == 0 and info["flood_passes"] == 0 and info["tiles_seeded"] == 0
    g.close()


# ---- 3. the full neighbourhood -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape,walls,conn", [((17, 17, 17), (5, 10), 26), ((19, 26), (8, 16), 8)], ids=["17x17x17_n26", "19x26_n8"])
def test_walls_full_neighbourhood(shape, walls, conn, seed):
    nw, source, sink = walls_graph(shape, walls, seed, conn)
    ref = _bk(("walls", shape, seed, conn), shape, nw, source, sink)
    g = _handle(shape, conn, nw, source, sink)
    _assert_sets(g, ref, unique=False)
    g.close()


# ---- 4. after warm edits -----------------------------------------------------------------------------------------------------------
def _changed(g):
    """changed_labels(), or the error code where the graph keeps no snapshot (update_markers by masks drops it)"""
    from medpy_amd import _lib
    try:
        return g.changed_labels().tolist()
    except _lib.MedpyHipError as e:
        return e.code


def _unchanged_by_the_call(g, labels_before, snapshot=True):
    """changed_labels() after the call is what it was before it, and what the two label volumes say"""
    from medpy_amd import _lib
    before = _changed(g)
    g.__dict__["_cut_sets_cache"] = {}   # (a fresh call, not the cached answer)
    g.source_side()
    g.ambiguous()
    assert _changed(g) == before
    if snapshot:
        assert before == np.flatnonzero((g.labels() != labels_before).ravel()).tolist()
    else:
        assert before == _lib.ERR_STATE


def test_after_tweight_and_nweight_edits():
    shape, walls = WALLS[0]
    nw, source, sink = walls_graph(shape, walls, 0)
    g = _handle(shape, None, nw, source, sink)
    _assert_sets(g, _bk(("walls", shape, 0), shape, nw, source, sink), unique=False)
    labels0 = g.labels().copy()
    # a sink weight on one voxel between the walls: the block around it can reach the sink now
    at = (10, 6, 12)
    sink = sink.copy()
    sink[at] = 7.0
    g.edit_tweights(int(np.ravel_multi_index(at, shape)), 0.0, 7.0)
    with pytest.raises(Exception) as e:
        g.source_side()
    from medpy_amd import _lib
    assert isinstance(e.value, _lib.MedpyHipError) and e.value.code == _lib.ERR_STATE
    _assert_sets(g, _bk(("walls", shape, 0, "sink_at"), shape, nw, source, sink))
    _unchanged_by_the_call(g, labels0)
    labels1 = g.labels().copy()
    # one arc of the first wall closed: the walls are no longer equal
    there, back = (a.copy() for a in nw[(0, 0, 1)])
    open_arcs = np.argwhere(there[..., walls[0]] > 0)
    p = tuple(int(v) for v in open_arcs[len(open_arcs) // 2]) + (walls[0],)
    there[p] = back[p] = 0.0
    nw = dict(nw)
    nw[(0, 0, 1)] = (there, back)
    i = int(np.ravel_multi_index(p, shape))
    g.edit_nweights([i], [i + 1], [0.0], [0.0])
    _assert_sets(g, _bk(("walls", shape, 0, "sink_at", "arc_closed"), shape, nw, source, sink))
    _unchanged_by_the_call(g, labels1)
    g.close()


def test_after_update_markers_on_a_built_in_term():
    """difference_division with sigma 1 on an image of 0s and 3s: every n-link is 1 or 1/4, the markers weigh 65535 -- exact
    arithmetic.  Two planes of weak arcs of equal capacity; then a background stroke inside the block between them."""
    from medpy_amd import graphcut
    shape = (20, 13, 27)
    image = np.zeros(shape, np.float32)
    image[..., 9:18] = 3.0
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    fg[..., 0] = True
    bg[..., -1] = True
    g = graphcut.graph_from_voxels(fg, bg, boundary_term=graphcut.energy_voxel.boundary_difference_division, boundary_term_args=(image, 1.0, False))

    def ref(fg, bg):
        cut = pipeline.graphcut_voxel(fg, bg, term="difference_division", image=image, sigma=1.0)
        fs, ts, amb = cutcheck.ambiguity(cut.graph, tol=0.0)
        return cut.flow, fs.reshape(shape), ts.reshape(shape), amb.reshape(shape)
    r0 = ref(fg, bg)
    assert r0[3][..., 9:18].all() and not r0[3][..., :9].any()   # the block between the planes, and nothing before it
    _assert_sets(g, r0, unique=False)
    labels0 = g.labels().copy()
    bg2 = bg.copy()
    bg2[8:11, 5:8, 13] = True
    g.update_markers(fg, bg2)
    _assert_sets(g, ref(fg, bg2))
    _unchanged_by_the_call(g, labels0, snapshot=False)   # (an update by masks keeps no snapshot, with or without the call)
    g.close()


# ---- 5. floating-point graphs: what holds for every solver ---------------------------------------------------------------------------
@pytest.mark.parametrize("forms", ["as_shipped", "large_volume_forms"])
@pytest.mark.parametrize("volume,n", [("sphere", 48), ("hard", 40)])
def test_floating_point_invariants(volume, n, forms, monkeypatch):
    from conftest import LARGE_VOLUME_FORMS
    from medpy_amd import _lib, graphcut, synthetic
    if forms == "large_volume_forms":
        monkeypatch.setenv("MEDPY_HIP_PARAMS", LARGE_VOLUME_FORMS)
    s = getattr(synthetic, volume)((n, n, n))
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                   boundary_term_args=(s["image"], s["sigma"], False))
    flow = g.maxflow()
    fs, amb, labels, info = g.source_side(), g.ambiguous(), g.labels(), g.cut_sets_info()
    key = ("float", volume, n)
    if key not in _REF:
        cut = pipeline.graphcut_voxel(s["fg"], s["bg"], term=s["term"], image=s["image"], sigma=s["sigma"])
        _REF[key] = [int(a.sum()) for a in cutcheck.ambiguity(cut.graph, tol=0.0)]
    print("%s %d^3 %s: flow %r source_cut %r | from_source %d to_sink %d ambiguous %d | BK at tol 0: %r | passes %d visits %d skipped %d"
          % (volume, n, forms, flow, info["source_cut"], info["from_source"], info["to_sink"], info["ambiguous"], _REF[key],
             info["flood_passes"], info["tile_visits"], info["tiles_skipped"]))
    assert not (fs & ~labels).any()
    assert fs[s["fg"]].all()
    assert not (amb & fs).any() and not (amb & ~labels).any()
    assert info["source_cut"] == pytest.approx(flow, rel=1e-9)
    _lib.assert_valid(g.validate())
    g.close()


# ---- 6. contract -------------------------------------------------------------------------------------------------------------------
def _raw(g, want_fs=True, want_amb=True):
    from medpy_amd import _lib
    n = int(np.prod(g._shape))
    fs = np.full(n, 7, np.uint8) if want_fs else None
    amb = np.full(n, 7, np.uint8) if want_amb else None
    rc = _lib.load().mgc_cut_sets(g._h, None if fs is None else _lib.ptr(fs), None if amb is None else _lib.ptr(amb))
    out, cut = np.zeros(8, np.int64), ctypes.c_double(0.0)
    if rc == _lib.OK:
        assert _lib.load().mgc_get_cut_sets_info(g._h, _lib.ptr(out), ctypes.byref(cut)) == _lib.OK
    return rc, fs, amb, out.tolist(), cut.value


def test_states_and_what_a_call_leaves():
    from medpy_amd import _lib
    from medpy_amd.graphcut import VoxelGraph
    shape, walls = WALLS[0]
    nw, source, sink = walls_graph(shape, walls, 1)
    g = VoxelGraph(shape)
    for o, (there, back) in nw.items():
        g._add_nweights(o, there, back)
    g._add_tweights(source, sink)
    assert _raw(g)[0] == _lib.ERR_STATE                      # before the build
    g._build()
    rc, fs, amb, _, _ = _raw(g)
    assert rc == _lib.ERR_STATE and (fs == 7).all() and (amb == 7).all()   # before the solve; nothing written
    flow = g.maxflow()
    labels = g.labels().copy()
    before = (g.stats(), g.launch_counts(), g.validate())
    rc, fs, amb, out, cut = _raw(g)
    assert rc == _lib.OK and set(np.unique(fs)) <= {0, 1} and set(np.unique(amb)) <= {0, 1}
    assert out[:3] == [int(fs.sum()), int((~labels).sum()), int(amb.sum())] and out[7] == 0 and cut == flow
    # either pointer NULL, both NULL, and twice: the same answer every time
    for want_fs, want_amb in ((True, False), (False, True), (False, False), (True, True)):
        rc2, fs2, amb2, out2, cut2 = _raw(g, want_fs, want_amb)
        assert rc2 == _lib.OK and out2 == out and cut2 == cut
        assert fs2 is None or np.array_equal(fs2, fs)
        assert amb2 is None or np.array_equal(amb2, amb)
    after = (g.stats(), g.launch_counts(), g.validate())
    assert before[0] == after[0], "mgc_get_stats (device_bytes among them) changed"
    assert before[1] == after[1] and before[2] == after[2]
    assert g.maxflow() == flow and np.array_equal(g.labels(), labels)
    np.testing.assert_array_equal(fs.astype(bool).reshape(shape), g.source_side())
    # an edit that has not been solved
    g.edit_tweights(5, 1.0, 0.0)
    rc, fs3, amb3, _, _ = _raw(g)
    assert rc == _lib.ERR_STATE and (fs3 == 7).all() and (amb3 == 7).all()
    with pytest.raises(_lib.MedpyHipError) as e:
        g.cut_is_unique()
    assert e.value.code == _lib.ERR_STATE
    g.maxflow()
    assert _raw(g)[0] == _lib.OK
    g.close()


def test_slab_handle_is_refused():
    from medpy_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    gshape = (ctypes.c_int64 * 3)(32, 8, 8)
    assert lib.mgc_create_slab(3, gshape, 6, 0, 0, 2, ctypes.byref(h)) == _lib.OK
    try:
        out = np.full(32 * 8 * 8, 7, np.uint8)
        assert lib.mgc_cut_sets(h, _lib.ptr(out), None) == _lib.ERR_UNSUPPORTED
        assert (out == 7).all()
    finally:
        lib.mgc_destroy(h)


def test_sparse_graph_refuses():
    from medpy_amd.graphcut import graph
    g = graph.SparseGraph(4)
    for name in ("source_side", "ambiguous", "cut_is_unique", "cut_sets_info"):
        with pytest.raises(NotImplementedError, match="sparse-graph solver"):
            getattr(g, name)()
    g.close()

"""-m gpu: ``msg_cut_sets`` / ``msg_cut_sets_tol`` and ``cut_sets()`` / ``cut_sets_unique()`` of every graph kind.

The fifteen graphs of tests/sparse_cases.py and the three dusty ones have passed the host simulator against exact arithmetic in
test_sparse_cut_sets_host.py; what only this file tests is the flood with every node of a kernel running at once, the C entry points
and their contract, and the graphs the library assembles itself (region graphs, 4-D lattices, parallel arcs of GraphInt / GraphFloat).
Expected sets come from two solves of oracle/exact_maxflow.py (tests/sparse_cut_sets_cases.py), never from a solver of this project."""
import ctypes as C

import numpy as np
import pytest

import sparse_cases as sc
import sparse_cut_sets_cases as cs
from test_gpu_sparse_warm import Handle, _ptr

pytestmark = pytest.mark.gpu
ULP64 = cs.ULP64


def _double(n, i, j, cap, rev, tr, fc=0.0):
    from medpy_amd.graphcut import GraphDouble
    g = GraphDouble(n, max(int(np.size(i)), 1))
    g.set_param("max_rounds", 100 * max(int(n), 64))
    if np.size(i):
        g._add_edges(i, j, cap, rev)
    g._set_tweights_merged(tr, fc)
    return g


def _case_graph(name):
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    return _double(n, i, j, cap, rev, tr, fc)


def _check_info(got, n):
    f, t, a, info = got
    assert all(x.dtype == np.bool_ and x.shape == (n,) for x in (f, t, a))
    assert (info["from_source"], info["to_sink"], info["ambiguous"]) == (int(f.sum()), int(t.sum()), int(a.sum()))
    assert info["from_source"] + info["to_sink"] + info["ambiguous"] == n and not (f & t).any()


# ---- 1. the fifteen cases

@pytest.mark.parametrize("name", sc.SOLVE_NAMES)
def test_case_against_exact_arithmetic_and_the_host_simulator(name):
    """whole-number cases: the exact sets bit for bit at tol None, 0 and ULP64, both cuts == the flow; float cases: the exact sets at
    ULP64 (all five: none is held to the invariants alone), cuts within rel 1e-12.  At every tolerance: the simulator's sets, and the
    invariants."""
    g = _case_graph(name)
    n = sc.case(name)[0]
    want, sim = cs.exact_sets(name), cs.host_sim_case(name)
    flow = g.maxflow()
    sc.assert_flow(flow, sc.cut_of(name)[1], name, "cold solve")
    prev = None
    for tol in cs.TOLS:
        got = g.cut_sets(tol)
        _check_info(got, n)
        info = got.info
        print(name, tol, {k: info[k] for k in ("from_source", "to_sink", "ambiguous", "forward_passes", "backward_passes", "arcs_closed", "tlinks_closed", "source_cut", "sink_cut")})
        if name in sc.INTEGER_CASES and tol in (None, 0.0, ULP64):
            cs.assert_sets(got[:3], want, "%s tol %r" % (name, tol))
            assert info["source_cut"] == info["sink_cut"] == flow, (name, tol, info, flow)
        if name not in sc.INTEGER_CASES and tol == ULP64:
            cs.assert_sets(got[:3], want, "%s tol ULP64" % name)
            for key in ("source_cut", "sink_cut"):
                assert abs(info[key] - flow) <= 1e-12 * abs(flow), (name, key, info[key], flow)
        cs.assert_sets(got[:3], sim["sets"][tol], "%s tol %r against the host simulator" % (name, tol))
        if name in sc.INTEGER_CASES:   # (on float inputs the residuals, and with them what the threshold closes, depend on the order in which
            assert (info["arcs_closed"], info["tlinks_closed"]) == (0, 0)   # concurrent relabels are seen: wide_range closes 1 arc here, 0 in the simulator)
        assert g.cut_sets_unique(tol) == (info["ambiguous"] == 0)
        if tol is None:
            assert np.array_equal(got.to_sink, ~g.labels()) and info["tol"] is None and not info["tol_path"] and info["sink_cut"] == flow
        else:
            assert info["tol"] == tol and info["tol_path"]
        if prev is not None:
            assert not (got.from_source & ~prev[0]).any() and not (got.to_sink & ~prev[1]).any() and not (prev[2] & ~got.ambiguous).any(), (name, tol)
        prev = got[:3]
    g.close()


@pytest.mark.parametrize("name", cs.DUSTY_CASES)
def test_dusty_case_gives_the_clean_sets_at_ulp64(name):
    n, i, j, cap, rev, tr, fc = cs.dusty(name)
    g = _double(n, i, j, cap, rev, tr, fc)
    g.maxflow()
    got, sim = g.cut_sets(ULP64), cs.host_sim_dusty(name)
    print(name, got.info)
    cs.assert_sets(got[:3], cs.exact_sets(name), "dusty %s at ULP64 against the clean graph" % name)
    cs.assert_sets(got[:3], sim["sets"][ULP64], "dusty %s at ULP64 against the host simulator" % name)
    assert got.info["arcs_closed"] > 0 and got.info["tlinks_closed"] > 0
    assert g.cut_sets_unique(ULP64) == (cs.SIZES[name][2] == 0)
    g.close()


# ---- 2. graphs the library assembles itself

def _exact_of_graph(g):
    """the exact sets of the graph AS BUILT: its own arcs and merged t-links read back"""
    tail, head, cap = g.arcs()
    n = g._nodes
    fwd = tail < head
    back = {(int(a), int(b)): float(w) for a, b, w in zip(tail[~fwd], head[~fwd], cap[~fwd])}
    i, j, c = tail[fwd].astype(np.int64), head[fwd].astype(np.int64), cap[fwd]
    r = np.array([back[(int(b), int(a))] for a, b in zip(i, j)], np.float64)
    return cs.exact_sets_of(n, i, j, c, r, g.tweights())


@pytest.mark.parametrize("term", ["stawiaski", "difference_of_means"])
def test_region_graph(term):
    """24 x 20 x 16 voxels in 240 regions of 4 x 4 x 2, whole-number image, object markers on the first slab of regions, background markers
    on the last, and two planes of region borders of the same capacity (20) in between: the two slabs between them are ambiguous"""
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_label as el
    shape = (24, 20, 16)
    z, y, x = np.indices(shape)
    lab = ((z // 4) * 40 + (y // 4) * 8 + (x // 2) + 1).astype(np.int32)
    fg, bg = z < 4, z >= 20
    if term == "stawiaski":   # 1 / (1 + 3)**2 per voxel pair across the planes z = 7 | 8 and 15 | 16, 1 across every other border
        img = np.where((z == 7) | (z == 15), 3, 0).astype(np.int32)
        g = graphcut.graph_from_labels(lab, fg, bg, boundary_term=el.boundary_stawiaski, boundary_term_args=img)
    else:   # region means 0, 0, 8, 8, 16, 16 by slab: 1 - 8 / 16 per region pair across the same two planes
        img = (8 * (z // 8)).astype(np.int32)
        g = graphcut.graph_from_labels(lab, fg, bg, boundary_term=el.boundary_difference_of_means, boundary_term_args=img)
    assert isinstance(g, graphcut.RegionGraph) and g._nodes == 240
    flow = g.maxflow()
    want = _exact_of_graph(g)
    slab = np.arange(240) // 40
    assert np.array_equal(want[0], slab < 2) and np.array_equal(want[1], slab >= 4)   # (the oracle says what the construction intends)
    for tol in (None, 0.0, ULP64):
        got = g.cut_sets(tol)
        _check_info(got, 240)
        cs.assert_sets(got[:3], want, "region graph, %s, tol %r" % (term, tol))
        assert got.info["source_cut"] == got.info["sink_cut"] == flow == 20.0   # dyadic weights: exact
        assert g.cut_sets_unique(tol) is False
    g.close()


def test_four_dimensional_voxel_graph():
    """6 x 5 x 4 x 3, whole-number image that steps by half its range between planes 1 | 2 and 3 | 4 of axis 0: both steps cost the same"""
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel as ev
    shape = (6, 5, 4, 3)
    img = np.broadcast_to(np.array([0, 0, 4, 4, 8, 8], np.int32).reshape(6, 1, 1, 1), shape).copy()
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    fg[0], bg[-1] = True, True
    g = graphcut.graph_from_voxels(fg, bg, boundary_term=ev.boundary_difference_linear, boundary_term_args=(img, False))
    assert isinstance(g, graphcut.SparseGraph) and not isinstance(g, graphcut.RegionGraph)
    flow = g.maxflow()
    want = _exact_of_graph(g)
    plane = np.arange(360) // 60
    assert np.array_equal(want[0], plane < 2) and np.array_equal(want[1], plane >= 4)
    for tol in (None, ULP64):
        got = g.cut_sets(tol)
        _check_info(got, 360)
        cs.assert_sets(got[:3], want, "4-D lattice, tol %r" % (tol,))
        assert got.info["source_cut"] == got.info["sink_cut"] == flow == 30.0
    assert g.cut_sets_unique() is False
    g.close()


def parallel_arc_calls(kind, seed=77, n=60, calls=150):
    """(n, add_edge calls, add_tweights calls, exact sets): ``calls`` add_edge calls over fewer node pairs, so many pairs carry parallel
    arcs; whole-number capacities 0..3 (int) or quarters of them (float), t-links on a third of the nodes: ties, and nodes without arcs"""
    rng = np.random.default_rng(seed)
    num = int if kind == "int" else (lambda v: float(np.float32(v) / 4))
    edges, arcs = [], {}
    pool = rng.integers(0, n - 4, (calls // 2, 2))   # the last four nodes get no arc; half as many node pairs as calls
    for _ in range(calls):
        a, b = (int(v) for v in pool[rng.integers(0, len(pool))])
        if a == b:
            continue
        c, r = num(rng.integers(0, 4)), num(rng.integers(0, 4))
        edges.append((a, b, c, r))
        arcs[(a, b)] = arcs.get((a, b), 0.0) + float(c)
        arcs[(b, a)] = arcs.get((b, a), 0.0) + float(r)
    tlinks, tr = [], np.zeros(n)
    for u in np.flatnonzero(rng.random(n) < 0.3):
        s, k = num(rng.integers(0, 6)), num(rng.integers(0, 6))
        tlinks.append((int(u), s, k))
        tr[u] = float(s) - float(k)
    pairs = sorted(k for k in arcs if k[0] < k[1])
    i, j = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    cap, rev = np.array([arcs[p] for p in pairs]), np.array([arcs[(p[1], p[0])] for p in pairs])
    assert len(edges) > len(pairs) + 20, "hardly any parallel arcs"
    return n, edges, tlinks, cs.exact_sets_of(n, i, j, cap, rev, tr)


@pytest.mark.parametrize("kind", ["int", "float"])
def test_graph_int_and_float_with_parallel_arcs(kind):
    from medpy_amd import _lib
    from medpy_amd.graphcut import GraphFloat, GraphInt
    n, edges, tlinks, want = parallel_arc_calls(kind)
    assert min(int(w.sum()) for w in want) > 0, [int(w.sum()) for w in want]   # (what makes the case a test: none of the three sets is empty)
    g = (GraphInt if kind == "int" else GraphFloat)(n, len(edges))
    g.add_node(n)
    for a, b, c, r in edges:
        g.add_edge(a, b, c, r)
    for u, s, k in tlinks:
        g.add_tweights(u, s, k)
    flow = g.maxflow()
    for tol in (None, 0.0, ULP64):
        got = g.cut_sets(tol)
        _check_info(got, n)
        cs.assert_sets(got[:3], want, "Graph%s, tol %r" % (kind, tol))
        assert got.info["source_cut"] == got.info["sink_cut"] == float(flow)
        assert g.cut_sets_unique(tol) is False
    g.add_edge(0, 1, edges[0][2], edges[0][3])   # an arc the device has not seen: refused from the Python layer, nothing is sent
    with pytest.raises(_lib.MedpyHipError) as e:
        g.cut_sets()
    assert e.value.code == _lib.ERR_STATE
    g.close()


# ---- 3. warm

def test_after_a_warm_solve():
    from medpy_amd import _lib
    name = "ring_chords_ties"
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    g = _double(n, i, j, cap, rev, tr, fc)
    g.maxflow()
    cs.assert_sets(g.cut_sets()[:3], cs.exact_sets(name), name)
    rng = np.random.default_rng(20)
    ids = np.sort(rng.choice(n, 20, replace=False))
    tr2 = tr.copy()
    tr2[ids] = rng.integers(-5, 6, 20).astype(float)
    g.update_tweights(ids, tr2[ids])
    for call in (lambda: g.cut_sets(), lambda: g.cut_sets(ULP64), lambda: g.cut_sets_unique()):
        with pytest.raises(_lib.MedpyHipError) as e:
            call()
        assert e.value.code == _lib.ERR_STATE
    flow = g.maxflow()
    assert g.warm_info()["skipped_build"]
    cold = _double(n, i, j, cap, rev, tr2, fc)
    assert cold.maxflow() == flow
    want = cs.exact_sets_of(n, i, j, cap, rev, tr2)
    assert not all(np.array_equal(a, b) for a, b in zip(want, cs.exact_sets(name))), "the edit moved nothing: the case shows nothing"
    for tol in (None, ULP64):
        got = g.cut_sets(tol)
        cs.assert_sets(got[:3], want, "warm, tol %r" % (tol,))
        cs.assert_sets(got[:3], cold.cut_sets(tol)[:3], "warm against cold, tol %r" % (tol,))
        assert got.info["source_cut"] == got.info["sink_cut"] == flow
    g.close()
    cold.close()


# ---- 4. the contract of the C entry points

class H(Handle):
    def cut_sets(self, tol, want=(True, True, True), canary=0xAB):
        """(rc, [from_source, to_sink, ambiguous]) -- arrays pre-filled with the canary, None where the pointer was NULL"""
        planes = [np.full(self.n, canary, np.uint8) if w else None for w in want]
        p = [None if a is None else _ptr(a) for a in planes]
        if tol is None:
            rc = self.lib.msg_cut_sets(self.h, p[0], p[2])
        else:
            rc = self.lib.msg_cut_sets_tol(self.h, C.c_double(tol), p[0], p[1], p[2])
        return rc, planes

    def cut_info(self):
        out, vals = np.zeros(16, np.int64), np.zeros(4)
        rc = self.lib.msg_get_cut_sets_info(self.h, _ptr(out), _ptr(vals))
        return rc, out.tolist(), vals.tolist()

    def stats(self):
        st = self.L.SparseStats()
        assert self.lib.msg_get_stats(self.h, C.byref(st)) == self.L.OK
        return st.as_dict()


def _loaded(name):
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    h = H(n)
    h.add_edges(i, j, cap, rev)
    h.set_tweights(tr, fc)
    return h


def test_null_pointers_refusals_and_what_a_call_leaves():
    name = "ring_chords_ties"
    n, tr = sc.case(name)[0], sc.case(name)[6]
    want = cs.exact_sets(name)
    h = _loaded(name)
    L = h.L
    try:
        def refused(code, tol, what):
            rc, planes = h.cut_sets(tol)
            assert rc == code, (what, tol, rc)
            assert all(p is None or (p == 0xAB).all() for p in planes), "%s: a refused call wrote to its outputs" % what

        assert h.cut_info()[0] == L.ERR_STATE   # no call yet
        for tol in (None, 0.0, ULP64):
            refused(L.ERR_STATE, tol, "before msg_maxflow")
        rc, flow = h.maxflow()
        assert rc == L.OK
        for tol in (-0.1, 1.0, 2.0, float("nan"), float("inf"), -float("inf")):
            refused(L.ERR_INVALID, tol, "bad tol")
        assert h.lib.msg_cut_sets(None, None, None) == L.ERR_INVALID and h.lib.msg_cut_sets_tol(None, C.c_double(0.0), None, None, None) == L.ERR_INVALID
        assert h.lib.msg_get_cut_sets_info(None, None, None) == L.ERR_INVALID
        # a warm state to look at: solve, update, solve -- labels of the earlier solve are held
        ids = np.arange(0, 200, 10)
        assert h.update(ids, -tr[ids], sc.case(name)[7]) == L.OK
        refused(L.ERR_STATE, None, "after msg_update_tweights")
        refused(L.ERR_STATE, ULP64, "after msg_update_tweights")
        assert h.maxflow()[0] == L.OK
        assert h.update(ids, tr[ids], sc.case(name)[7]) == L.OK
        rc, flow2 = h.maxflow()
        assert rc == L.OK and flow2 == flow
        before = (h.labels()[1].tobytes(), h.stats(), h.info(), h.delta(n)[1:2], h.delta(n)[2].tobytes())
        # all eight combinations of NULL (four for the call without a tolerance, which has no to_sink)
        infos = []
        for tol in (None, ULP64):
            for mask in range(8):
                sel = (bool(mask & 1), bool(mask & 2) and tol is not None, bool(mask & 4))
                rc, planes = h.cut_sets(tol, sel)
                assert rc == L.OK, (tol, sel)
                for k, p in enumerate(planes):
                    if p is not None:
                        assert np.array_equal(p.astype(bool), want[k]) and p.max() <= 1, (tol, sel, k)
                rc, out16, out4 = h.cut_info()
                assert rc == L.OK
                infos.append((tol, out16, out4))
                assert (h.labels()[1].tobytes(), h.stats(), h.info(), h.delta(n)[1:2], h.delta(n)[2].tobytes()) == before, "a call changed what the solve left"
        for tol, out16, out4 in infos:   # the counts do not depend on which planes come down
            assert out16[:3] == [int(w.sum()) for w in want] and out16[10:] == [0] * 6
            assert out16[9] == (0 if tol is None else 1) and out4[0] == (-1.0 if tol is None else tol)
            assert out4[1] == out4[2] == flow
            assert (out16[5], out16[6]) == (0, 0) if tol is None else (out16[5] >= 8 and out16[6] > 0)
        assert h.lib.msg_get_cut_sets_info(h.h, None, None) == L.OK
        rc, again = h.maxflow()
        assert rc == L.OK and again == flow and np.array_equal(h.labels()[1].astype(bool), ~want[1])
    finally:
        h.close()


def test_a_warm_solve_after_cut_sets_equals_one_without():
    name = "hub5000"
    n, tr, fc = sc.case(name)[0], sc.case(name)[6], sc.case(name)[7]
    a, b = _loaded(name), _loaded(name)
    try:
        assert a.maxflow() == b.maxflow()
        for tol in (None, 0.0, ULP64, 1e-6):
            assert a.cut_sets(tol)[0] == a.L.OK
        rng = np.random.default_rng(5)
        ids = np.sort(rng.choice(n, 400, replace=False))
        vals = rng.integers(-3, 4, 400).astype(float)
        for h in (a, b):
            assert h.update(ids, vals, fc) == h.L.OK
        fa, fb = a.maxflow(), b.maxflow()
        assert fa == fb and fa[0] == a.L.OK and a.info() == b.info() and a.info()[0] == 1
        assert a.labels()[1].tobytes() == b.labels()[1].tobytes()
        sa, sb = a.stats(), b.stats()
        assert all(sa[k] == sb[k] for k in ("rounds", "global_relabels", "relabel_passes", "nodes", "arcs")), (sa, sb)
        for tol in (None, ULP64):
            pa, pb = a.cut_sets(tol)[1], b.cut_sets(tol)[1]
            assert all(x is None or x.tobytes() == y.tobytes() for x, y in zip(pa, pb))
        tr2 = tr.copy()
        tr2[ids] = vals
        n_, i, j, cap, rev = sc.case(name)[:5]
        cs.assert_sets(a.cut_sets(ULP64)[1], cs.exact_sets_of(n, i, j, cap, rev, tr2), "hub5000 after the update")
    finally:
        a.close()
        b.close()


# ---- 5. one name on every graph kind

def test_voxel_graph_cut_sets_is_its_four_calls():
    from medpy_amd.graphcut import CutSets
    from test_gpu_cut_sets import _handle, walls_graph
    shape = (8, 8, 8)
    nw, source, sink = walls_graph(shape, (2, 4), 0)
    g = _handle(shape, None, nw, source, sink)
    g.maxflow()
    for tol in (None, ULP64):
        got = g.cut_sets(tol)
        assert isinstance(got, CutSets) and all(a.shape == shape for a in got[:3])
        assert np.array_equal(got.from_source, g.source_side(tol)) and np.array_equal(got.to_sink, g.sink_side(tol))
        assert np.array_equal(got.ambiguous, g.ambiguous(tol)) and got.info == g.cut_sets_info(tol)
        assert g.cut_sets_unique(tol) == g.cut_is_unique(tol) and g.cut_sets_unique(tol) is False
        assert int(got.ambiguous.sum()) > 0
    g.close()

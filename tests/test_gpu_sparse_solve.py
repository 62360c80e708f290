"""-m gpu: the cold path of the sparse-graph solver (msg_sparse.hip, msg_node_ops.inl) on graphs that stress its schedule -- depth far
beyond rounds_per_relabel, rows of thousands of arcs, exact ties, one-way arcs, graphs without arcs / sinks / excess -- against the
exact cut of tests/sparse_cases.py (Dinic in Python integers).  Every case has passed the host simulator against the same values in
test_sparse_cases_host.py; what only this file tests is the solver with every node of a kernel running at once.

Labels must equal the exact ones; the flow bit for bit on the whole-number cases, within rel 1e-12 (include/medpy_hip.h) otherwise.
Nothing here compares rounds or relabel passes with the host simulator: both depend on the order in which concurrent relabels are
seen."""
import ctypes as C
import time

import numpy as np
import pytest

import sparse_cases as sc
from test_gpu_sparse_warm import Handle

pytestmark = pytest.mark.gpu


class H(Handle):
    """the ctypes handle of test_gpu_sparse_warm.py with the read-backs this file needs"""

    def stats(self):
        st = self.L.SparseStats()
        assert self.lib.msg_get_stats(self.h, C.byref(st)) == self.L.OK
        return st.as_dict()

    def segment(self, i):
        seg = C.c_int(-1)
        assert self.lib.msg_what_segment(self.h, int(i), C.byref(seg)) == self.L.OK
        return seg.value

    def error(self):
        return (self.lib.msg_last_error(self.h) or b"").decode()


def max_rounds(n):
    """The guard every solve here runs under: 100 rounds per node.  The host simulator needs at most one round per node on these
    cases (path2000: 2 000); a solver that has stopped making progress -- a reverse-arc index that points at the wrong arc hands every
    push back to its sender -- ends as MGC_ERR_NOT_CONVERGED with the case's name, not as a hang."""
    return 100 * max(int(n), 64)


def _load(name, h=None):
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    h = h or H(n)
    assert h.param("max_rounds", max_rounds(n)) == h.L.OK
    if i.size:
        h.add_edges(i, j, cap, rev)
    h.set_tweights(tr, fc)
    return h


def _solve_and_check(h, name, what):
    want_labels, want_flow = sc.cut_of(name)
    rc, flow = h.maxflow()
    assert rc == h.L.OK, "%s %s: msg_maxflow returned %d: %s" % (name, what, rc, h.error())
    rc, labels = h.labels()
    assert rc == h.L.OK
    sc.assert_labels(labels, want_labels, name, what)
    sc.assert_flow(flow, want_flow, name, what)
    return flow, labels


@pytest.mark.parametrize("name", sc.SOLVE_NAMES)
def test_solve_case_through_the_c_abi(name):
    """path2000, measured on MI355X with this test: 0.37 s in msg_maxflow (2 000 rounds, 33 global relabels, 38 640 relabel passes),
    0.48 s for the whole case -- the chain keeps its 2 000 nodes.  The other cases take 0.1 s or less."""
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    h = _load(name)
    try:
        assert h.segment(0) == 0 and h.segment(n - 1) == 0   # before maxflow every node reads SOURCE (graph.h:561-571)
        t0 = time.perf_counter()
        flow, labels = _solve_and_check(h, name, "cold solve")
        seconds = time.perf_counter() - t0
        want_labels = sc.cut_of(name)[0]
        for u in (0, n - 1, sc.HUB.get(name, n // 2)):
            assert h.segment(u) == (0 if want_labels[u] else 1), "%s: msg_what_segment(%d) disagrees with the labels" % (name, u)
        st = h.stats()
        assert st["nodes"] == n and st["edges_added"] == i.size, st
        assert st["arcs"] == sc.arcs_of(name)[0].size, (st["arcs"], sc.arcs_of(name)[0].size)
        assert st["global_relabels"] >= 1 and st["relabel_passes"] >= 8
        info = h.info()
        assert info[0] == 0 and info[3] == 1, info   # a cold build, the only one
        print("%s: %d nodes, %d arcs, %.3f s in msg_maxflow, rounds %d, global relabels %d, relabel passes %d"
              % (name, n, st["arcs"], seconds, st["rounds"], st["global_relabels"], st["relabel_passes"]))
        if name == "path2000":
            assert st["rounds"] > 64 * 8 and st["global_relabels"] > 8   # deeper than many batches of rounds
        if name in ("no_sink", "isolated_tlinks", "one_way_away"):
            assert st["rounds"] == 0 and st["global_relabels"] == 1, st   # nothing active at the first count
    finally:
        h.close()


@pytest.mark.parametrize("name", ["random3000", "hub5000"])
def test_solve_case_through_graph_double_in_bulk(name):
    from medpy_amd.graphcut import GraphDouble
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    want_labels, want_flow = sc.cut_of(name)
    g = GraphDouble(n, i.size)
    g.set_param("max_rounds", max_rounds(n))
    g._add_edges(i, j, cap, rev)
    g._set_tweights_merged(tr, fc)
    flow = g.maxflow()
    sc.assert_labels(g.labels(), want_labels, name, "GraphDouble")
    sc.assert_flow(flow, want_flow, name, "GraphDouble")
    assert g.get_arc_num() == sc.arcs_of(name)[0].size
    for u in (0, n - 1, sc.HUB.get(name, n // 2)):
        assert g.what_segment(u) == (g.termtype.SOURCE if want_labels[u] else g.termtype.SINK)
    g.close()


def test_k40_40_ties_through_graph_int_call_by_call():
    """Graph<int,int,int>: sum_edge / add_tweights one call each; the flow is an ``int`` with the exact value"""
    from medpy_amd.graphcut import GraphInt
    name = "k40_40_ties"
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    want_labels, want_flow = sc.cut_of(name)
    g = GraphInt(n, i.size)
    assert g.add_node(n) == 0
    g.set_param("max_rounds", max_rounds(n))
    for a, b, c, r in zip(i.tolist(), j.tolist(), cap.tolist(), rev.tolist()):
        g.sum_edge(a, b, int(c), int(r))
    for u in range(n):
        g.add_tweights(u, int(max(tr[u], 0.0)), int(max(-tr[u], 0.0)))
    flow = g.maxflow()
    assert isinstance(flow, int) and fc == 0.0 and flow == want_flow, (flow, want_flow)
    sc.assert_labels(g.labels(), want_labels, name, "GraphInt")
    g.close()


def test_eighths_through_graph_float_call_by_call():
    """Graph<float,float,float> on ring_chords_ties with every capacity and t-link divided by 8: float32 holds them and their sums
    exactly, so the cut is the same and the flow an eighth, exactly"""
    from medpy_amd.graphcut import GraphFloat
    name = "ring_chords_ties"
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    want_labels, want_flow = sc.cut_of(name)
    g = GraphFloat(n, i.size)
    assert g.add_node(n) == 0
    g.set_param("max_rounds", max_rounds(n))
    for a, b, c, r in zip(i.tolist(), j.tolist(), (cap / 8).tolist(), (rev / 8).tolist()):
        g.sum_edge(a, b, c, r)
    for u in np.flatnonzero(tr).tolist():
        g.add_tweights(u, max(tr[u], 0.0) / 8, max(-tr[u], 0.0) / 8)
    flow = g.maxflow()
    assert fc == 0.0 and flow == want_flow / 8, (flow, want_flow / 8)
    sc.assert_labels(g.labels(), want_labels, name, "GraphFloat")
    g.close()


KNOB_VALUES = (1, 2, 17, 64, 100000)


@pytest.mark.parametrize("name", sc.SWEEP_CASES)
def test_rounds_per_relabel_sweep(name):
    """labels identical and equal to the exact ones at every value; the flow bit-identical across values (it is computed from the
    labels and the capacities as built, in a fixed order); more global relabels at 1 than at 64"""
    flows, relabels = {}, {}
    for v in KNOB_VALUES:
        h = _load(name)
        try:
            assert h.param("rounds_per_relabel", v) == h.L.OK
            flows[v], _ = _solve_and_check(h, name, "rounds_per_relabel %d" % v)
            st = h.stats()
            relabels[v] = st["global_relabels"]
            print("%s rounds_per_relabel %d: rounds %d, global relabels %d, relabel passes %d, %.1f ms" % (name, v, st["rounds"], st["global_relabels"], st["relabel_passes"], st["solve_ms"]))
        finally:
            h.close()
    assert len({np.float64(f).tobytes() for f in flows.values()}) == 1, flows
    assert relabels[1] > relabels[64], relabels


@pytest.mark.parametrize("pname, value", [("rounds_per_relabel", 0), ("rounds_per_relabel", -1), ("max_rounds", 0), ("warm", 2), ("no_such_knob", 1)])
def test_refused_parameters_change_nothing(pname, value):
    name = "k40_40_ties"
    h = _load(name)
    try:
        flow0, labels0 = _solve_and_check(h, name, "before the refused call")
        assert h.param(pname, value) == h.L.ERR_INVALID
        assert pname in h.error(), h.error()
        flow1, labels1 = _solve_and_check(h, name, "after msg_set_param(%s, %d) was refused" % (pname, value))
        assert flow1 == flow0 and np.array_equal(labels0, labels1)
        assert h.info()[0] == 0   # msg_maxflow again without an update in between: a cold build
    finally:
        h.close()


def test_solve_add_edges_solve():
    """edges added after a solve: the next solve is a cold build of all edges and equals the exact cut of the joined graph"""
    n, i, j, cap, rev, once, tr, fc = sc.case("components_joined")
    m = sc.case("components")[1].size
    h = _load("components")
    try:
        flow0, _ = _solve_and_check(h, "components", "first solve")
        assert h.info()[3] == 1
        h.add_edges(i[m:], j[m:], cap[m:], rev[m:])
        flow1, _ = _solve_and_check(h, "components_joined", "solve after msg_add_edges")
        info = h.info()
        assert info[0] == 0 and info[3] == 2, info   # not skipped: built again from the whole edge list
        st = h.stats()
        assert st["edges_added"] == i.size and st["arcs"] == sc.arcs_of("components_joined")[0].size
        assert flow1 > flow0
    finally:
        h.close()

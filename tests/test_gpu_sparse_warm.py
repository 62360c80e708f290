"""-m gpu: warm re-solves, edits by node list and the label delta on the sparse-graph solver ("The sparse-graph
solver"; msg_update_tweights / msg_labels_delta / msg_get_warm_info, SparseGraph.update_tweights / changed_nodes, RegionGraph).

Every warm solve is held against a COLD solve of the same inputs in the same library (labels array_equal, flow ==) and against
the BK oracle (labels equal, flow to rel=1e-9), and warm_info() must say the build was skipped.  No tie relaxation in this file:
the inputs carry float (or whole-number) capacities whose maximal source set -- what both solvers read out -- is unique."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import bk, energy_label_numpy as eln
from test_sparse_warm_host import component_of, random_graph

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "reference_labels.npz"))


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


class Handle(object):
    """a msg_* handle driven through medpy_amd._lib directly"""

    def __init__(self, nodes):
        from medpy_amd import _lib
        self.L, self.lib, self.n = _lib, _lib.load(), int(nodes)
        self.h = C.c_void_p()
        assert self.lib.msg_create(self.n, 0, C.byref(self.h)) == _lib.OK

    def close(self):
        if self.h:
            self.lib.msg_destroy(self.h)
            self.h = None

    def add_edges(self, i, j, cap, rev):
        i, j = np.ascontiguousarray(i, np.int64), np.ascontiguousarray(j, np.int64)
        cap, rev = np.ascontiguousarray(cap, np.float64), np.ascontiguousarray(rev, np.float64)
        assert self.lib.msg_add_edges(self.h, i.size, _ptr(i), _ptr(j), _ptr(cap), _ptr(rev)) == self.L.OK

    def set_tweights(self, tr, fc=0.0):
        tr = np.ascontiguousarray(tr, np.float64)
        assert self.lib.msg_set_tweights_merged(self.h, _ptr(tr), float(fc)) == self.L.OK

    def update(self, ids, tr, fc=0.0):
        tr = np.ascontiguousarray(tr, np.float64)
        if ids is None:
            return self.lib.msg_update_tweights(self.h, tr.size, None, _ptr(tr), float(fc))
        ids = np.ascontiguousarray(ids, np.int64)
        return self.lib.msg_update_tweights(self.h, ids.size, _ptr(ids), _ptr(tr), float(fc))

    def maxflow(self):
        flow = C.c_double(0.0)
        rc = self.lib.msg_maxflow(self.h, C.byref(flow))
        return rc, flow.value

    def labels(self):
        out = np.empty(self.n, np.uint8)
        rc = self.lib.msg_labels(self.h, _ptr(out))
        return rc, out

    def delta(self, cap):
        ids, n = np.full(max(cap, 1), -1, np.int64), C.c_int64(-1)
        rc = self.lib.msg_labels_delta(self.h, cap, _ptr(ids), C.byref(n))
        return rc, n.value, ids

    def info(self):
        out = np.zeros(4, np.int64)
        assert self.lib.msg_get_warm_info(self.h, _ptr(out)) == self.L.OK
        return out.tolist()

    def param(self, name, value):
        return self.lib.msg_set_param(self.h, name.encode(), int(value))


def _bk(n, i, j, cap, rev, tr):
    o = bk.BKGraph(n, max(16, i.size))
    if i.size:
        o.sum_edges(i, j, cap, rev)
    o.add_tweights(None, np.maximum(tr, 0.0), np.maximum(-tr, 0.0))
    return o.maxflow(), o.labels()


# ---- 1. the raw classes: add_tweights -> maxflow -> add_tweights -> maxflow

def _edit_calls(rng, n, kind):
    """the (node, cap_source, cap_sink) calls of one edit on ~5 % of the nodes; whole numbers for GraphInt"""
    draw = (lambda: float(rng.integers(0, 40))) if kind == "int" else (lambda: float(rng.random() * 3))
    return [(int(u), draw(), draw()) for u in np.flatnonzero(rng.random(n) < 0.05)]


@pytest.mark.parametrize("kind", ["double", "int"])
def test_raw_classes_resolve_warm_after_add_tweights(kind):
    from medpy_amd.graphcut import GraphDouble, GraphInt
    cls = {"double": GraphDouble, "int": GraphInt}[kind]
    num = (lambda v: int(v)) if kind == "int" else float
    rng = np.random.default_rng(11)
    for trial in range(6):
        n, i, j, cap, rev, src, snk = random_graph(rng)
        if kind == "int":   # whole-number capacities: exact arithmetic
            cap, rev = np.floor(cap * 40) + 1, np.floor(rev * 40) + 1
            src, snk = np.floor(src * 40), np.floor(snk * 40)
        calls = [(int(u), src[u], snk[u]) for u in range(n) if src[u] or snk[u]]

        def build(all_calls):
            g = cls(n, i.size)
            assert g.add_node(n) == 0
            for a, b, c, r in zip(i.tolist(), j.tolist(), cap.tolist(), rev.tolist()):
                g.sum_edge(a, b, num(c), num(r))
            for u, s, k in all_calls:
                g.add_tweights(u, num(s), num(k))
            return g

        def oracle(all_calls):
            o = bk.BKGraph(n, max(16, i.size))
            if i.size:
                o.sum_edges(i, j, cap, rev)
            for u, s, k in all_calls:   # t-links accumulate call by call, as in the graph under test (graph.h:416-425)
                o.add_tweights(np.array([u]), np.array([float(s)]), np.array([float(k)]))
            return o.maxflow(), o.labels()

        g = build(calls)
        g.maxflow()
        assert not g.warm_info()["skipped_build"]
        for step in range(3):
            tr = g.tweights()
            edit = _edit_calls(rng, n, kind)
            if step == 1:   # a node that feeds the graph becomes one that drains it
                u = int(np.argmax(tr))
                edit.append((u, 0, float(np.ceil(abs(tr[u])) + 2)))
            if step == 2:   # every sink link of one component goes (cancelled by as much source capacity): no label of it stays finite
                comp = component_of(n, i, j, int(np.argmin(tr)))
                edit = [(int(u), float(-tr[u]), 0) for u in np.flatnonzero(comp & (tr < 0))] + [c for c in edit if not comp[c[0]]]
            calls = calls + edit
            for u, s, k in edit:
                g.add_tweights(u, num(s), num(k))
            flow = g.maxflow()
            info = g.warm_info()
            assert info["skipped_build"] and info["cold_builds"] == 1, info
            cold = build(calls)
            cflow = cold.maxflow()
            assert not cold.warm_info()["skipped_build"]
            np.testing.assert_array_equal(g.labels(), cold.labels())
            assert flow == cflow
            oflow, olabels = oracle(calls)
            np.testing.assert_array_equal(g.labels().astype(np.uint8), olabels)
            assert flow == pytest.approx(oflow, rel=1e-9, abs=1e-12)
            if step == 2:
                assert g.labels()[comp].all()
            assert g.what_segment(0) == (g.termtype.SOURCE if olabels[0] else g.termtype.SINK)


# ---- 2. region graphs

def _region_inputs(case, term):
    from medpy_amd.graphcut import energy_label as el
    g = lambda k: GOLD["%s/%s" % (case, k)]
    kw = dict(boundary_term=el.boundary_stawiaski, boundary_term_args=g("gradient"))
    if term == "stawiaski_atlas":
        kw.update(regional_term=el.regional_atlas, regional_term_args=(g("prob"), 0.5))
    return g("labels"), g("fg").astype(bool), g("bg").astype(bool), kw


def _region_oracle(case, term, lab, fg, bg):
    """BK on the graph graph_from_labels describes.  With the atlas term the regional t-links are the library's own region sums
    (a float32 accumulation whose order differs from numpy.sum's -- tests/test_gpu_labels.py allows rel=1e-6 for it); edges,
    markers and the solve are the oracle's."""
    grad = GOLD[case + "/gradient"]
    if term == "stawiaski":
        flow, seg, _ = eln.graphcut_labels(lab, fg, bg, "stawiaski", grad)
        return flow, seg
    from medpy_amd.graphcut.graph import region_sums
    n = int(lab.max())
    sums, _ = region_sums(lab, GOLD[case + "/prob"], n)
    src = (np.float32(0.5) * sums.astype(np.float32)).astype(np.float64)   # (energy_label.regional_atlas on a float32 map)
    o = bk.BKGraph(n, 10 * n)
    o.add_tweights(None, src, -src)
    i, j, cap, rev, _ = eln.BOUNDARY["stawiaski"](lab, grad)
    o.sum_edges(i, j, cap, rev)
    s, t = np.unique(lab[fg] - 1), np.unique(lab[bg] - 1)
    o.add_tweights(s, np.full(s.size, 65535.0), np.zeros(s.size))
    o.add_tweights(t, np.zeros(t.size), np.full(t.size, 65535.0))
    return o.maxflow(), o.labels().astype(bool)


@pytest.mark.parametrize("term", ["stawiaski", "stawiaski_atlas"])
@pytest.mark.parametrize("case", ["l2d_f32", "l3d_f32"])
def test_region_graph_marker_edits_resolve_warm(case, term):
    from medpy_amd import graphcut
    lab, fg0, bg0, kw = _region_inputs(case, term)
    flat = lab.reshape(-1)
    a = graphcut.graph_from_labels(lab, fg0, bg0, **kw)   # edited by masks
    b = graphcut.graph_from_labels(lab, fg0, bg0, **kw)   # edited by voxel lists
    assert isinstance(a, graphcut.RegionGraph) and isinstance(a, graphcut.SparseGraph)
    flow0 = a.maxflow()
    assert b.maxflow() == flow0
    labels0 = a.labels().copy()
    oflow, oseg = _region_oracle(case, term, lab, fg0, bg0)
    np.testing.assert_array_equal(labels0, oseg)
    assert flow0 == pytest.approx(oflow, rel=1e-9)
    for m, want in zip(a.markers(), (fg0, bg0)):   # markers() round-trips
        assert m.dtype == np.bool_ and np.array_equal(m, want)
    marked_fg, marked_bg = np.unique(lab[fg0]) - 1, np.unique(lab[bg0]) - 1
    # the strokes: a background stroke in a region the first cut gave to the object, next to the fg markers' regions ...
    inside = [r for r in np.flatnonzero(labels0) if r not in marked_fg][0]
    bg_stroke = np.flatnonzero(flat == inside + 1)[:3]
    # ... a foreground stroke of two voxels elsewhere: in a region it gave to the background (with the atlas term every such region is
    # under the bg markers of these cases: then in another unmarked region of the object, where the hard link replaces the atlas') ...
    free = [r for r in range(labels0.size) if r not in marked_bg and r not in marked_fg and r != inside]
    outside = ([r for r in free if not labels0[r]] or free)[-1]
    fg_stroke = np.flatnonzero(flat == outside + 1)[:2]
    assert fg_stroke.size == 2
    # ... and the fg marker of one region taken away
    removed = np.flatnonzero(fg0.reshape(-1) & (flat == marked_fg[0] + 1))
    fg, bg = fg0.copy().reshape(-1), bg0.copy().reshape(-1)
    prev = labels0
    for name, (f, k, e) in (("bg stroke", (None, bg_stroke, None)), ("fg stroke", (fg_stroke, None, None)), ("marker removed", (None, None, removed)),
                            ("erase one of two", (None, None, fg_stroke[:1])), ("identical", (None, None, None))):
        if e is not None:
            fg[e], bg[e] = False, False
        if f is not None:
            fg[f] = True
        if k is not None:
            bg[k] = True
        tr_before = b.tweights()
        a.update_markers(fg.reshape(lab.shape), bg.reshape(lab.shape))
        b.edit_markers(fg=f, bg=k, erase=e)
        if name == "erase one of two":   # the region keeps its other marked voxel: still marked, nothing to send
            assert np.array_equal(b.tweights(), tr_before) and b.markers()[0].reshape(-1)[fg_stroke[1]]
        assert a.tweights().tobytes() == b.tweights().tobytes()   # the voxel lists give the state the masks give
        for m_a, m_b, want in zip(a.markers(), b.markers(), (fg, bg)):
            assert np.array_equal(m_a.reshape(-1), want) and np.array_equal(m_b.reshape(-1), want)
        flow, flow_b = a.maxflow(), b.maxflow()
        for g in (a, b):
            info = g.warm_info()
            assert info["skipped_build"] and info["snapshot"] and info["cold_builds"] == 1, (name, info)
        cold = graphcut.graph_from_labels(lab, fg.reshape(lab.shape), bg.reshape(lab.shape), **kw)
        cflow = cold.maxflow()
        assert not cold.warm_info()["skipped_build"]
        np.testing.assert_array_equal(a.labels(), cold.labels(), err_msg=name)
        np.testing.assert_array_equal(b.labels(), cold.labels(), err_msg=name)
        assert flow == cflow and flow_b == cflow, name
        oflow, oseg = _region_oracle(case, term, lab, fg.reshape(lab.shape), bg.reshape(lab.shape))
        np.testing.assert_array_equal(a.labels(), oseg, err_msg=name)
        assert flow == pytest.approx(oflow, rel=1e-9), name
        changed = a.changed_labels()   # region ids, 0-based
        assert changed.dtype == np.int64 and np.array_equal(changed, np.flatnonzero(prev != a.labels())), name
        assert np.array_equal(b.changed_labels(), changed)
        if name in ("erase one of two", "identical"):
            assert changed.size == 0 and a.warm_info()["folded"] == 0
        prev = a.labels().copy()
    # back to the markers of the first solve: its flow and labels
    a.update_markers(fg0, bg0)
    assert a.maxflow() == flow0 and a.warm_info()["skipped_build"]
    np.testing.assert_array_equal(a.labels(), labels0)
    with pytest.raises(ValueError):
        a.update_markers(fg0[1:], bg0)
    with pytest.raises(ValueError):
        a.edit_markers(fg=np.array([lab.size]))
    with pytest.raises(NotImplementedError):
        a.update_regional_term(GOLD[case + "/prob"], 0.5)


# ---- 3. the label delta

@pytest.mark.parametrize("n", [7, 16, 17, 4097])
def test_changed_nodes_is_the_label_difference(n):
    from medpy_amd import _lib
    from medpy_amd.graphcut import GraphDouble
    rng = np.random.default_rng(n)
    m = 3 * n
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = i != j
    i, j = i[keep], j[keep]
    cap, rev = rng.random(i.size) * 0.3 + 1e-3, rng.random(i.size) * 0.3 + 1e-3
    tr = rng.normal(0, 1, n)
    g = GraphDouble(n, i.size)
    g._add_edges(i, j, cap, rev)
    g.update_tweights(np.arange(n), tr)   # before any solve: stored, the solve is cold
    g.maxflow()
    assert not g.warm_info()["skipped_build"] and not g.warm_info()["snapshot"]
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.changed_nodes()   # no labels of an earlier solve
    assert ei.value.code == _lib.ERR_STATE
    before = g.labels().copy()
    # two edits before one solve: the delta spans both
    ids1 = np.unique(np.concatenate([rng.integers(0, n, max(2, n // 8)), [0, n - 1]]))
    tr[ids1] = -tr[ids1] - np.sign(tr[ids1])
    g.update_tweights(ids1, tr[ids1])
    assert g.warm_info()["folded"] == ids1.size and g.warm_info()["snapshot"]
    ids2 = np.unique(rng.integers(0, n, max(2, n // 8)))[::-1]   # descending: sorted in a copy by the library
    tr[ids2] = rng.normal(0, 2, ids2.size)
    g.update_tweights(ids2, tr[ids2])
    flow = g.maxflow()
    assert g.warm_info()["skipped_build"]
    oflow, olabels = _bk(n, i, j, cap, rev, tr)
    np.testing.assert_array_equal(g.labels().astype(np.uint8), olabels)
    assert flow == pytest.approx(oflow, rel=1e-9, abs=1e-12)
    want = np.flatnonzero(before != g.labels())
    assert want.size > 0   # (the edits flip the sign of t-links: labels move)
    got = g.changed_nodes()
    assert got.dtype == np.int64 and np.array_equal(got, want)
    patched = g.labels(out=before.copy())
    assert np.array_equal(patched, g.labels())
    as_bytes = before.astype(np.uint8)
    assert g.labels(out=as_bytes) is as_bytes and np.array_equal(as_bytes, g.labels().astype(np.uint8))
    # a cap too small: the count comes back, nothing is written
    out, cnt = np.full(want.size, -1, np.int64), C.c_int64(0)
    g._call("msg_labels_delta", want.size - 1, _lib.ptr(out), C.byref(cnt))
    assert cnt.value == want.size and (out == -1).all()
    g._call("msg_labels_delta", want.size, _lib.ptr(out), C.byref(cnt))
    assert cnt.value == want.size and np.array_equal(out, want)


# ---- 4. grid-stride and size, through the library directly

def test_whole_vector_and_long_list_updates_on_a_million_nodes():
    n = 1100003   # more than the 4096 x 256 threads of a launch
    rng = np.random.default_rng(4)
    base = np.arange(0, n - 3, 4)
    i = np.concatenate([base, base + 1, base + 2])   # disjoint 4-node paths: the solve is a few rounds deep
    j = i + 1
    cap, rev = rng.random(i.size) + 1e-3, rng.random(i.size) + 1e-3
    tr = rng.normal(0, 1, n)
    warm, cold = Handle(n), Handle(n)
    try:
        for h in (warm, cold):
            h.add_edges(i, j, cap, rev)
            h.set_tweights(tr, 0.25)
        rc, flow = warm.maxflow()
        assert rc == 0 and warm.info() == [0, 0, 0, 1]
        rc, before = warm.labels()
        oflow, olabels = _bk(n, i, j, cap, rev, tr)
        np.testing.assert_array_equal(before, olabels)
        assert flow == pytest.approx(0.25 + oflow, rel=1e-9)
        steps = []
        tr1 = np.where(rng.random(n) < 0.5, tr, rng.normal(0, 1, n))
        steps.append((None, tr1, tr1, -1.5))   # the whole vector, ids NULL
        ids = np.concatenate([[n - 1, 0], rng.choice(np.arange(1, n - 1), 69998, replace=False)])   # a list of 70 000, not in order
        tr2 = tr1.copy()
        tr2[ids] = rng.normal(0, 1, ids.size)
        steps.append((ids, tr2[ids], tr2, 2.0))
        for ids, vals, full, fc in steps:
            assert warm.update(ids, vals, fc) == 0
            assert warm.info()[1:3] == [n if ids is None else ids.size, 1]
            rc, flow = warm.maxflow()
            assert rc == 0 and warm.info() == [1, n if ids is None else ids.size, 1, 1]
            cold.set_tweights(full, fc)
            rc, cflow = cold.maxflow()
            assert rc == 0 and cold.info()[0] == 0
            rc, labels = warm.labels()
            np.testing.assert_array_equal(labels, cold.labels()[1])
            assert flow == cflow
            oflow, olabels = _bk(n, i, j, cap, rev, full)
            np.testing.assert_array_equal(labels, olabels)
            assert flow == pytest.approx(fc + oflow, rel=1e-9)
            want = np.flatnonzero(labels != before)
            rc, cnt, got = warm.delta(want.size)
            assert rc == 0 and cnt == want.size and np.array_equal(got[:cnt], want)
            before = labels
    finally:
        warm.close()
        cold.close()


# ---- 5. state rules

def _small(rng, n=300):
    m = 4 * n
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = i != j
    i, j = i[keep], j[keep]
    return n, i, j, rng.random(i.size) + 1e-3, rng.random(i.size) + 1e-3, rng.normal(0, 1, n)


def test_a_refused_list_changes_nothing():
    from medpy_amd import _lib
    from medpy_amd.graphcut import GraphDouble
    n, i, j, cap, rev, tr = _small(np.random.default_rng(21))
    g = GraphDouble(n, i.size)
    g._add_edges(i, j, cap, rev)
    g.update_tweights(np.arange(n), tr)
    g.maxflow()
    g.update_tweights(np.array([3, 5]), np.array([-tr[3], -tr[5]]))
    g.maxflow()
    tweights, labels, info, changed = g.tweights(), g.labels().copy(), g.warm_info(), g.changed_nodes()
    for ids, vals in (([1, n], [0.5, 0.5]), ([-1, 2], [0.5, 0.5]), ([4, 9, 4], [0.5, 0.5, 0.5]), ([4, 9], [0.5, float("nan")]), ([4, 9], [float("inf"), 0.5])):
        with pytest.raises(_lib.MedpyHipError) as ei:
            g.update_tweights(np.array(ids), np.array(vals))
        assert ei.value.code == _lib.ERR_INVALID
        assert np.array_equal(g.tweights(), tweights) and g.warm_info() == info
        assert np.array_equal(g.labels(), labels) and np.array_equal(g.changed_nodes(), changed)
    again = g.maxflow()   # nothing changed: the same cut, reached from the resident state
    np.testing.assert_array_equal(g.labels(), labels)
    assert again == pytest.approx(_bk(n, i, j, cap, rev, tweights)[0], rel=1e-9)


def test_updates_that_cannot_be_warm_give_a_correct_cold_solve():
    from medpy_amd.graphcut import GraphDouble
    rng = np.random.default_rng(22)
    n, i, j, cap, rev, tr = _small(rng)

    def check(g, edges, tr, cold_builds, warm):
        flow = g.maxflow()
        info = g.warm_info()
        assert info["skipped_build"] == warm and info["cold_builds"] == cold_builds, info
        oflow, olabels = _bk(n, *edges, tr)
        np.testing.assert_array_equal(g.labels().astype(np.uint8), olabels)
        assert flow == pytest.approx(oflow, rel=1e-9, abs=1e-12)

    g = GraphDouble(n, i.size)
    g.add_node(n)
    g._add_edges(i, j, cap, rev)
    g.update_tweights(np.arange(n), tr)   # before any solve
    check(g, (i, j, cap, rev), tr, 1, False)
    ids = np.array([0, 7, 19])
    tr = tr.copy()
    tr[ids] = -2 * tr[ids]
    g.update_tweights(ids, tr[ids])
    check(g, (i, j, cap, rev), tr, 1, True)
    # sum_edge after the solve: the arcs changed, the next solve builds again
    g.sum_edge(0, n - 1, 0.75, 0.5)
    tr[ids] = 0.5 * tr[ids]
    g.update_tweights(ids, tr[ids])
    e2 = (np.append(i, 0), np.append(j, n - 1), np.append(cap, 0.75), np.append(rev, 0.5))
    check(g, e2, tr, 2, False)
    # warm = 0: every update is stored only, every solve cold; warm = 1 again: warm from the next finished solve on
    g.set_param("warm", 0)
    tr[ids] = tr[ids] - 1.0
    g.update_tweights(ids, tr[ids])
    assert g.warm_info()["folded"] == 0
    check(g, e2, tr, 3, False)
    g.set_param("warm", 1)
    tr[ids] = tr[ids] + 3.0
    g.update_tweights(ids, tr[ids])
    check(g, e2, tr, 3, True)
    from medpy_amd import _lib
    for bad in (2, -1):
        with pytest.raises(_lib.MedpyHipError):
            g.set_param("warm", bad)
    # reset(): an empty graph again
    g.reset()
    g.add_node(n)
    g._add_edges(i, j, cap, rev)
    g.update_tweights(ids, tr[ids])
    only = np.zeros(n)
    only[ids] = tr[ids]
    check(g, (i, j, cap, rev), only, 1, False)


def test_not_converged_then_update_then_cold():
    from medpy_amd import _lib
    rng = np.random.default_rng(23)
    n = 64   # a chain from the source link at one end to the sink link at the other: one round of pushes cannot finish it
    i, j = np.arange(n - 1), np.arange(1, n)
    cap, rev = rng.random(n - 1) + 1.0, rng.random(n - 1) + 1.0
    tr = np.where(rng.random(n) < 0.2, rng.normal(0, 0.1, n), 0.0)
    tr[0], tr[n - 1] = 5.0, -5.0
    h = Handle(n)
    try:
        h.add_edges(i, j, cap, rev)
        h.set_tweights(tr)
        rc, cnt, _ = h.delta(8)
        assert rc == _lib.ERR_STATE   # before any solve
        assert h.param("max_rounds", 1) == 0 and h.param("rounds_per_relabel", 1) == 0
        rc, _ = h.maxflow()
        assert rc == _lib.ERR_NOT_CONVERGED
        ids = np.array([2, 11, 40])
        tr = tr.copy()
        tr[ids] = -tr[ids]
        assert h.update(ids, tr[ids]) == 0   # no finished solve to fold into: stored, no error
        assert h.info()[:3] == [0, 0, 0]
        assert h.param("max_rounds", 1 << 40) == 0 and h.param("rounds_per_relabel", 64) == 0
        rc, flow = h.maxflow()
        assert rc == 0 and h.info() == [0, 0, 0, 2]   # cold: built again
        oflow, olabels = _bk(n, i, j, cap, rev, tr)
        np.testing.assert_array_equal(h.labels()[1], olabels)
        assert flow == pytest.approx(oflow, rel=1e-9)
        rc, cnt, _ = h.delta(8)
        assert rc == _lib.ERR_STATE   # solved, but no labels of an earlier solve are held
        assert h.update(np.zeros(0, np.int64), np.zeros(0)) == 0   # an empty list on a finished solve: warm, nothing folded
        rc, flow2 = h.maxflow()
        assert rc == 0 and flow2 == flow and h.info() == [1, 0, 1, 2]
        rc, cnt, _ = h.delta(8)
        assert rc == 0 and cnt == 0
    finally:
        h.close()


def test_four_dimensional_voxel_graphs_still_refuse_the_lattice_calls():
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel as ev
    shape = (3, 4, 3, 2)
    rng = np.random.default_rng(1)
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    fg[1, 1, 1, 0], bg[0], bg[-1] = True, True, True
    g = graphcut.graph_from_voxels(fg, bg, boundary_term=ev.boundary_difference_exponential,
                                   boundary_term_args=(rng.random(shape).astype(np.float32), 1.0, False))
    assert isinstance(g, graphcut.SparseGraph) and not isinstance(g, graphcut.RegionGraph)
    g.maxflow()
    for call in (lambda: g.update_markers(fg, bg), lambda: g.update_regional_term(fg, 1.0), lambda: g.edit_markers(fg=[0]),
                 lambda: g.changed_labels(), lambda: g.markers()):
        with pytest.raises(NotImplementedError):
            call()

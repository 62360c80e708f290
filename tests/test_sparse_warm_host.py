"""CPU tier of the warm re-solve on the sparse-graph solver ("The sparse-graph solver"):

* the marker re-merge ``RegionGraph`` runs (``merge_region_markers``) against the merge ``GCGraph`` does call by call, bit for bit,
  and the host bookkeeping of ``RegionGraph`` (voxel masks -> marked regions) without a device;
* the t-link fold and the schedule of medpy_amd/csrc/msg_node_ops.inl, run on the host by tests/hostsim/hostsim_sparse_warm.cpp,
  against the BK oracle: solve, fold a list, solve again from the resident state;
* the host-side check of an update list (medpy_amd/csrc/msg_list_check.h), compiled into a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import bk

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "medpy_amd", "csrc")


def random_graph(rng):
    """the generator of tests/test_gpu_labels.py:test_raw_graphdouble_calls_random_graphs"""
    n = int(rng.integers(2, 400))
    m = int(rng.integers(1, 6 * n))
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = i != j
    i, j = i[keep], j[keep]
    cap, rev = rng.random(i.size) + 1e-3, rng.random(i.size) * (rng.random(i.size) < 0.7) + 1e-3
    src = np.where(rng.random(n) < 0.2, rng.random(n) * 3, 0.0)
    snk = np.where(rng.random(n) < 0.2, rng.random(n) * 3, 0.0)
    return n, i, j, cap, rev, src, snk


def component_of(n, i, j, start):
    """the nodes joined to ``start`` by edges, as a bool mask"""
    seen = np.zeros(n, bool)
    seen[start] = True
    while True:
        grow = seen.copy()
        grow[j[seen[i]]] = True
        grow[i[seen[j]]] = True
        if grow.sum() == seen.sum():
            return seen
        seen = grow


def bk_cut(n, i, j, cap, rev, tr):
    o = bk.BKGraph(n, max(16, i.size))
    if i.size:
        o.sum_edges(i, j, cap, rev)
    o.add_tweights(None, np.maximum(tr, 0.0), np.maximum(-tr, 0.0))
    return o.maxflow(), o.labels()


# ---- the marker re-merge

def _gcgraph_call_by_call(n, regional, fg_nodes, bg_nodes):
    """GCGraph's own merge, one set_tweight call per node as the reference makes them (graph.py:334-380, 536-552)"""
    from medpy_amd.graphcut import GCGraph
    g = GCGraph(n, 4 * n)
    if regional is not None:
        for u in range(n):
            g.set_tweight(u, float(regional[0][u]), float(regional[1][u]))
    for u in fg_nodes:
        g.set_tweight(int(u), GCGraph.MAX, 0)
    for u in bg_nodes:
        g.set_tweight(int(u), 0, GCGraph.MAX)
    return g._GCGraph__tr, g._GCGraph__flow_const


@pytest.mark.parametrize("with_regional", [False, True])
def test_marker_remerge_is_gcgraphs_merge_bit_for_bit(with_regional):
    from medpy_amd.graphcut import GCGraph
    from medpy_amd.graphcut.graph import merge_region_markers, merge_tweights_into
    rng = np.random.default_rng(5 + with_regional)
    for trial in range(20):
        n = int(rng.integers(3, 60))
        regional = None
        tr0, flow0 = np.zeros(n), 0.0
        if with_regional:   # regional_atlas: (alpha * w, -alpha * w), w of either sign; a few plain (source, sink) pairs among them
            w = rng.normal(0, 40, n)
            regional = (0.5 * w, -0.5 * w)
            if trial % 2:
                regional = (np.abs(w), rng.random(n) * 30)
            flow0 = merge_tweights_into(tr0, 0.0, np.arange(n), regional[0], regional[1])
        fg_nodes = np.flatnonzero(rng.random(n) < 0.25)
        bg_nodes = np.flatnonzero(rng.random(n) < 0.25)
        if trial % 3 == 0:   # a region under both kinds of marker
            both = int(rng.integers(0, n))
            fg_nodes, bg_nodes = np.union1d(fg_nodes, [both]), np.union1d(bg_nodes, [both])
        want_tr, want_flow = _gcgraph_call_by_call(n, regional, fg_nodes, bg_nodes)
        before = tr0.copy()
        got_tr, got_flow = merge_region_markers(tr0, flow0, fg_nodes, bg_nodes, GCGraph.MAX)
        assert np.array_equal(tr0, before)   # the t-links of the terms are kept for the next edit
        if want_tr is None:
            want_tr = np.zeros(n)
        assert got_tr.tobytes() == np.asarray(want_tr, dtype=np.float64).tobytes()
        assert got_flow == want_flow and isinstance(got_flow, float)
        if trial % 3 == 0 and not with_regional:
            assert got_tr[both] == 0.0 and got_flow >= GCGraph.MAX   # (MAX, 0) then (0, MAX): both links, MAX flows straight through


def _hostless_region_graph(label_image, fg, bg, tr0=None, flow0=0.0):
    """RegionGraph's marker bookkeeping without a device: the object as GCGraph leaves it, minus the library handle"""
    from medpy_amd.graphcut import RegionGraph
    g = object.__new__(RegionGraph)
    g._h, g._nodes, g._labels = None, int(label_image.max()), None
    g._set_regions(label_image, fg, bg, tr0, flow0)
    g._remerge()
    return g


def test_region_graph_voxel_edits_match_the_mask_path():
    from medpy_amd.graphcut import GCGraph
    from medpy_amd.graphcut.graph import merge_region_markers
    rng = np.random.default_rng(9)
    shape = (9, 11)
    lab = (np.arange(99).reshape(shape) // 7 + 1).astype(np.int32)   # 15 regions of 7 voxels (the last of 1)
    n = int(lab.max())
    tr0 = rng.normal(0, 5, n)
    fg, bg = rng.random(shape) < 0.05, rng.random(shape) < 0.05
    a = _hostless_region_graph(lab, fg, bg, tr0, 1.25)
    b = _hostless_region_graph(lab, fg, bg, tr0, 1.25)
    for step in range(12):
        f, k, e = (rng.integers(0, lab.size, rng.integers(0, 4)) for _ in range(3))
        b.edit_markers(fg=f, bg=k, erase=e)
        mf, mk, me = (np.isin(np.arange(lab.size), x).reshape(shape) for x in (f, k, e))
        fg, bg = (fg & ~me) | mf, (bg & ~me) | mk
        a.update_markers(fg, bg)
        for g in (a, b):
            assert np.array_equal(g.markers()[0], fg) and np.array_equal(g.markers()[1], bg)
        assert a.tweights().tobytes() == b.tweights().tobytes() and a._flow_const == b._flow_const
        want = merge_region_markers(tr0, 1.25, np.unique(lab[fg]) - 1, np.unique(lab[bg]) - 1, GCGraph.MAX)
        assert a.tweights().tobytes() == want[0].tobytes() and a._flow_const == want[1]
    # a region is marked while any marked voxel lies in it
    c = _hostless_region_graph(lab, np.zeros(shape, bool), np.zeros(shape, bool), tr0, 0.0)
    c.edit_markers(fg=np.array([14, 15]))   # two voxels of region 3
    marked = c.tweights().copy()
    assert marked[2] != tr0[2]
    c.edit_markers(erase=np.array([14]))
    assert np.array_equal(c.tweights(), marked) and c.markers()[0].sum() == 1
    c.edit_markers(erase=np.array([15]))
    assert np.array_equal(c.tweights(), tr0) and not c.markers()[0].any()
    with pytest.raises(ValueError):
        c.update_markers(np.zeros((9, 10), bool), None)
    with pytest.raises(ValueError):
        c.edit_markers(fg=np.array([99]))


# ---- the fold and the warm schedule on the host

@pytest.fixture(scope="module")
def warm_sim():
    so = os.path.join(HERE, "hostsim", "libhostsim_sparse_warm.so")
    src = os.path.join(HERE, "hostsim", "hostsim_sparse_warm.cpp")
    dep = os.path.join(CSRC, "msg_node_ops.inl")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    pi, pf, pu = (np.ctypeslib.ndpointer(t, flags="C_CONTIGUOUS") for t in (np.int64, np.float64, np.uint8))
    lib.hostsim_sparse_warm.argtypes = [C.c_int64, C.c_int64, pi, pi, pf, pf, pf, C.c_int64, pi, pf, C.c_int, pu, pf, pi, pf, pf, pf, pi]
    return lib


def _run_warm(lib, n, i, j, cap, rev, tr, ids, tr_new):
    i, j = np.ascontiguousarray(i, np.int64), np.ascontiguousarray(j, np.int64)
    tr_io = np.array(tr, dtype=np.float64)
    labels, cuts = np.zeros(2 * n, np.uint8), np.zeros(2)
    row, cap0, rcap = np.zeros(n + 1, np.int64), np.zeros(2 * i.size + 1), np.zeros(2 * i.size + 1)
    state, stats = np.zeros(4 * n), np.zeros(3, np.int64)
    rc = lib.hostsim_sparse_warm(n, i.size, i, j, np.ascontiguousarray(cap), np.ascontiguousarray(rev), tr_io, ids.size,
                                 np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(tr_new, np.float64), 64, labels, cuts, row, cap0,
                                 rcap, state, stats)
    assert rc == 0
    return tr_io, labels.reshape(2, n), cuts, row, cap0[:stats[0]], rcap[:stats[0]], state.reshape(4, n), stats


@pytest.mark.parametrize("edit", ["random", "source_to_sink", "no_sink_left"])
def test_fold_then_resolve_on_the_host_matches_bk(warm_sim, edit):
    rng = np.random.default_rng(11)
    for trial in range(6):
        n, i, j, cap, rev, src, snk = random_graph(rng)
        tr = src - snk
        ids = np.flatnonzero(rng.random(n) < 0.05)
        tr_new = rng.normal(0, 2, ids.size)
        if edit == "source_to_sink":   # a node that feeds the graph becomes one that drains it
            u = int(np.argmax(tr)) if (tr > 0).any() else 0
            ids = np.union1d(ids, [u])
            tr_new = rng.normal(0, 2, ids.size)
            tr_new[np.searchsorted(ids, u)] = -(abs(tr[u]) + 1.5)
        if edit == "no_sink_left":   # every sink link of one component goes: no label of it stays finite
            start = int(np.argmin(tr))
            comp = component_of(n, i, j, start)
            ids = np.flatnonzero(comp & (tr < 0))
            tr_new = np.where(rng.random(ids.size) < 0.5, 0.0, rng.random(ids.size))
        if trial % 2:   # (the node function takes the entries in any order)
            p = rng.permutation(ids.size)
            ids, tr_new = ids[p], tr_new[p]
        tr_after, labels, cuts, row, cap0, rcap, state, stats = _run_warm(warm_sim, n, i, j, cap, rev, tr, ids, tr_new)
        want = tr.copy()
        want[ids] = tr_new
        assert np.array_equal(tr_after, want)
        for k, t in enumerate((tr, want)):
            oflow, olabels = bk_cut(n, i, j, cap, rev, t)
            np.testing.assert_array_equal(labels[k], olabels)
            assert cuts[k] == pytest.approx(oflow, rel=1e-9, abs=1e-12)
        if edit == "no_sink_left" and ids.size:
            assert labels[1][comp].all()
        # the fold keeps the preflow: what a node holds minus what it may still send to the sink = its t-link + what flowed in
        inflow = np.array([np.sum(rcap[row[u]:row[u + 1]] - cap0[row[u]:row[u + 1]]) for u in range(n)])
        scale = max(float(np.abs(cap0).max()) if cap0.size else 0.0, float(np.abs(want).max()), float(np.abs(tr).max()), 1e-300)
        assert np.abs((state[0] - state[1]) - (tr + inflow)).max() <= 1e-12 * scale     # (the finished solve, before the fold)
        assert np.abs((state[2] - state[3]) - (want + inflow)).max() <= 1e-12 * scale   # after it
        assert (state[2] >= 0).all() and (state[3] >= 0).all() and not ((state[2] > 0) & (state[3] > 0)).any()
        # nodes not in the list keep their state bit for bit
        others = np.ones(n, bool)
        others[ids] = False
        assert state[2][others].tobytes() == state[0][others].tobytes() and state[3][others].tobytes() == state[1][others].tobytes()


# ---- the list check of msg_update_tweights

def test_update_list_check_stand_alone(tmp_path):
    """range / finite / sort / duplicate, before any write: the stand-alone program runs the cases and says which failed"""
    exe = str(tmp_path / "msg_list_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", exe, os.path.join(HERE, "hostsim", "msg_list_check_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr

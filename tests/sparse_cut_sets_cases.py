"""What tests/test_sparse_cut_sets_host.py (CPU tier) and tests/test_gpu_sparse_cut_sets.py (-m gpu) share for ``msg_cut_sets`` /
``msg_cut_sets_tol``.  Not a test module, no GPU, no library.

* ``exact_sets``: from_source / to_sink / ambiguous of a graph in exact arithmetic, by two solves of oracle/exact_maxflow.py: the nodes
  that reach the sink, and -- the same solve on the transposed graph (every arc turned round, sources and sinks swapped) -- the nodes
  the source reaches.
* ``rule_sets``: the rule of medpy_amd/csrc/msg_reach_ops.inl restated in NumPy over a residual graph given as arrays.
* ``dusty``: a case with capacities and t-links of 2**-80 where the clean graph has zeros; ``scaled`` and ``side_by_side`` to move a
  graph through the exponent range and to put two of different magnitude into one.
* ``host_sim`` / ``run_host_sim``: tests/hostsim/hostsim_sparse_reach.cpp, compiled on first use.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import sparse_cases as sc
from oracle import exact_maxflow

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "medpy_amd", "csrc")
ULP64 = 64 * 2.0 ** -52
DUST = 2.0 ** -80
TOLS = (None, 0.0, ULP64, 1e-12, 1e-6)
FLOAT_CASES = tuple(n for n in sc.SOLVE_NAMES if n not in sc.INTEGER_CASES)
DUSTY_CASES = ("hub5000", "ring_chords_ties", "one_way_away")
# the sizes the sets must have (from_source, to_sink, ambiguous): pinned, so that an oracle that drifts is noticed too
SIZES = {
    "path2000": (1201, 799, 0), "path300_two_bottlenecks": (3, 3, 294), "hub5000": (853, 3544, 604), "two_hubs": (1501, 1501, 0),
    "k40_40_ties": (10, 70, 0), "ring_chords_ties": (446, 331, 723), "random3000": (2869, 131, 0), "wide_range": (403, 97, 0),
    "one_way_away": (1, 1, 298), "duplicates3000": (24, 26, 0), "components": (297, 495, 208), "isolated_tlinks": (16, 32, 16),
    "no_sink": (2995, 0, 5), "no_source": (0, 2996, 4), "end_nodes": (2, 9, 29),
}
_CACHE = {}


# ---- exact sets ----------------------------------------------------------------------------------------------------------------------

def exact_sets_of(n, i, j, cap, rev, tr):
    """(from_source, to_sink, ambiguous) as bool arrays, of the graph AS BUILT (repeated pairs summed first, ``merged_edges``)"""
    mi, mj, mc, mr = sc.merged_edges(n, i, j, cap, rev)
    tr = np.asarray(tr, np.float64)
    to_sink = exact_maxflow.canonical_sink_side(n, mi, mj, mc, mr, tr)
    from_source = exact_maxflow.canonical_sink_side(n, mi, mj, mr, mc, -tr)
    assert to_sink is not None and from_source is not None, "%d nodes: beyond the exact oracle" % n
    assert not (to_sink & from_source).any(), "the oracle's own sets overlap"
    return from_source, to_sink, ~(from_source | to_sink)


def exact_sets(name):
    """``exact_sets_of`` a case of sparse_cases, solved once per process (the sink side is the one ``sparse_cases.cut_of`` solved)"""
    if name not in _CACHE:
        n, i, j, cap, rev, once, tr, fc = sc.case(name)
        mi, mj, mc, mr = sc.merged_edges(n, i, j, cap, rev)
        to_sink = ~sc.cut_of(name)[0].astype(bool)
        from_source = exact_maxflow.canonical_sink_side(n, mi, mj, mr, mc, -np.asarray(tr, np.float64))
        assert not (to_sink & from_source).any(), "%s: the oracle's own sets overlap" % name
        _CACHE[name] = (from_source, to_sink, ~(from_source | to_sink))
    return _CACHE[name]


# ---- the rule, in NumPy --------------------------------------------------------------------------------------------------------------

def _flood(n, src, dst, seeds):
    """the nodes reachable from ``seeds`` along the arcs src[k] -> dst[k]"""
    mark = seeds.copy()
    frontier = seeds.copy()
    while frontier.any():
        new = np.zeros(n, bool)
        new[dst[frontier[src]]] = True
        frontier = new & ~mark
        mark |= frontier
    return mark


def rule_sets(n, tail, head, rcap, cap0, excess, sink, tr, tol, labels=None):
    """the rule of msg_reach_ops.inl over arrays: arcs (tail, head) sorted by (tail, head), every arc with its reverse.  Returns
    (from_source, to_sink, ambiguous, arcs_closed, tlinks_closed).  ``tol`` None: open iff rcap > 0 and to_sink = ``~labels``."""
    tail, head = np.asarray(tail, np.int64), np.asarray(head, np.int64)
    key = tail * n + head
    assert (np.diff(key) > 0).all()
    rev = np.searchsorted(key, head * n + tail)
    assert not tail.size or (key[rev] == head * n + tail).all()
    tr = np.zeros(n) if tr is None else np.asarray(tr, np.float64)
    if tol is None:
        open_ = rcap > 0
        seed_s = excess > 0
        from_source = _flood(n, tail[open_], head[open_], seed_s)
        to_sink = ~np.asarray(labels).astype(bool)
        return from_source, to_sink, ~(from_source | to_sink), 0, 0
    scale = np.zeros(n)
    np.maximum.at(scale, tail, cap0 + cap0[rev])
    with np.errstate(invalid="ignore"):
        thr = tol * np.maximum(scale[tail], scale[head]) if tol > 0 else np.zeros(tail.size)
        nthr = tol * np.maximum(np.abs(tr), scale) if tol > 0 else np.zeros(n)
    open_ = (rcap > 0) & (rcap > thr)
    seed_s, seed_t = (excess > 0) & (excess > nthr), (sink > 0) & (sink > nthr)
    from_source = _flood(n, tail[open_], head[open_], seed_s)
    to_sink = _flood(n, head[open_], tail[open_], seed_t)
    closed_t = int(((excess > 0) & ~seed_s).sum() + ((sink > 0) & ~seed_t).sum())
    return from_source, to_sink, ~(from_source | to_sink), int(((rcap > 0) & ~open_).sum()), closed_t


# ---- dust ----------------------------------------------------------------------------------------------------------------------------

def dusty(name, seed=80):
    """the case as one edge per node pair, with DUST in place of every zero capacity whose other direction carries >= 1, and +-DUST
    t-links on a twentieth of the nodes that have none and whose arcs carry >= 1.  Returns (n, i, j, cap, rev, tr, flow_const)."""
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    mi, mj, mc, mr = sc.merged_edges(n, i, j, cap, rev)
    mc, mr, tr = mc.copy(), mr.copy(), np.array(tr, np.float64)
    dc, dr = (mc == 0) & (mr >= 1), (mr == 0) & (mc >= 1)
    assert dc.sum() + dr.sum() > 0, "%s: no zero capacity next to one >= 1" % name
    scale = np.zeros(n)
    np.maximum.at(scale, mi, mc + mr)
    np.maximum.at(scale, mj, mc + mr)
    mc[dc], mr[dr] = DUST, DUST
    rng = np.random.default_rng(seed)
    free = np.flatnonzero((tr == 0) & (scale >= 1))
    pick = rng.choice(free, max(1, free.size // 20), replace=False)
    assert (tr[pick] == 0).all() and (scale[pick] >= 1).all()
    tr[pick] = DUST * rng.choice([-1.0, 1.0], pick.size)
    return n, mi, mj, mc, mr, tr, fc


def scaled(graph, factor):
    """every capacity, t-link and the flow constant times ``factor`` (a power of two: nothing rounds)"""
    n, i, j, cap, rev, tr, fc = graph
    return n, i, j, cap * factor, rev * factor, tr * factor, fc * factor


def side_by_side(a, b):
    """two graphs in one, the nodes of ``b`` behind those of ``a``, no arc between them"""
    return (a[0] + b[0], np.concatenate([a[1], b[1] + a[0]]), np.concatenate([a[2], b[2] + a[0]]), np.concatenate([a[3], b[3]]),
            np.concatenate([a[4], b[4]]), np.concatenate([a[5], b[5]]), a[6] + b[6])


# ---- the host simulator --------------------------------------------------------------------------------------------------------------

def host_sim():
    if "lib" not in _CACHE:
        so = os.path.join(HERE, "hostsim", "libhostsim_sparse_reach.so")
        src = os.path.join(HERE, "hostsim", "hostsim_sparse_reach.cpp")
        deps = [src, os.path.join(CSRC, "msg_node_ops.inl"), os.path.join(CSRC, "msg_reach_ops.inl")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
        lib = C.CDLL(so)
        pi, pf, pu, p32 = (np.ctypeslib.ndpointer(t, flags="C_CONTIGUOUS") for t in (np.int64, np.float64, np.uint8, np.int32))
        lib.hostsim_sparse_reach.argtypes = [C.c_int64, C.c_int64, pi, pi, pf, pf, pf, C.c_double, C.c_int, C.c_int, pf, pu, pf, pu, pi, pf, pi, p32, p32,
                                             pf, pf, pf, pf]
        _CACHE["lib"] = lib
    return _CACHE["lib"]


INFO_KEYS = ("from_source", "to_sink", "ambiguous", "forward_passes", "forward_seeds", "backward_passes", "backward_seeds", "arcs_closed",
             "tlinks_closed", "tol_path")


def run_host_sim(n, i, j, cap, rev, tr, flow_const=0.0, tols=TOLS):
    """dict: ``labels``, ``flow``, the residual graph (``tail``, ``head``, ``rcap``, ``cap0``, ``excess``, ``sink``) and per tol of
    ``tols`` an entry ``sets[tol]`` = (from_source, to_sink, ambiguous) and ``info[tol]`` = what msg_get_cut_sets_info reports"""
    lib = host_sim()
    i, j = np.ascontiguousarray(i, np.int64), np.ascontiguousarray(j, np.int64)
    cap, rev, tr = (np.ascontiguousarray(a, np.float64) for a in (cap, rev, tr))
    m = max(2 * i.size, 1)
    tv = np.array([-1.0 if t is None else float(t) for t in tols], np.float64)
    labels, flow = np.zeros(n, np.uint8), np.zeros(1)
    sets, info, vals = np.zeros((len(tols), 3, n), np.uint8), np.zeros((len(tols), 16), np.int64), np.zeros((len(tols), 4))
    arcs, tail, head = np.zeros(1, np.int64), np.zeros(m, np.int32), np.zeros(m, np.int32)
    rcap, cap0, excess, sink = np.zeros(m), np.zeros(m), np.zeros(n), np.zeros(n)
    rc = lib.hostsim_sparse_reach(n, i.size, i, j, cap, rev, tr, float(flow_const), 64, len(tols), tv, labels, flow, sets, info, vals, arcs, tail, head,
                                  rcap, cap0, excess, sink)
    assert rc == 0, "host simulator: %s" % {1: "the solve did not converge", 2: "a flood changed the residual graph", 3: "flow in flight after the solve"}.get(rc, rc)
    a = int(arcs[0])
    out = {"labels": labels, "flow": float(flow[0]), "tail": tail[:a], "head": head[:a], "rcap": rcap[:a], "cap0": cap0[:a], "excess": excess, "sink": sink,
           "sets": {}, "info": {}}
    for k, t in enumerate(tols):
        out["sets"][t] = tuple(sets[k, p].astype(bool) for p in range(3))
        d = dict(zip(INFO_KEYS, info[k].tolist()))
        d.update(tol=float(vals[k, 0]), source_cut=float(vals[k, 1]), sink_cut=float(vals[k, 2]), scale_max=float(vals[k, 3]))
        out["info"][t] = d
    return out


def host_sim_case(name):
    """``run_host_sim`` of a case of sparse_cases, once per process"""
    if ("sim", name) not in _CACHE:
        n, i, j, cap, rev, once, tr, fc = sc.case(name)
        _CACHE[("sim", name)] = run_host_sim(n, i, j, cap, rev, tr, fc)
    return _CACHE[("sim", name)]


def host_sim_dusty(name):
    if ("dusty", name) not in _CACHE:
        n, i, j, cap, rev, tr, fc = dusty(name)
        _CACHE[("dusty", name)] = run_host_sim(n, i, j, cap, rev, tr, fc, tols=(0.0, ULP64))
    return _CACHE[("dusty", name)]


def assert_sets(got, want, what):
    for k, kind in enumerate(("from_source", "to_sink", "ambiguous")):
        g, w = np.asarray(got[k]).astype(bool).ravel(), np.asarray(want[k]).astype(bool).ravel()
        bad = np.flatnonzero(g != w)
        assert not bad.size, "%s: %s differs on %d of %d nodes (%d set, %d expected), first at node %d" % (what, kind, bad.size, w.size, int(g.sum()), int(w.sum()), int(bad[0]))

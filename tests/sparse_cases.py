"""What tests/test_sparse_cases_host.py (CPU tier) and the -m gpu files of the sparse-graph solver (test_gpu_sparse_build.py,
test_gpu_sparse_solve.py) share: graphs that stress the build and the schedule of msg_sparse.hip, with expected values that come from
no solver of this project.  Not a test module, no GPU, no library.

Every generator has a fixed seed and returns ``(n, i, j, cap, rev, once, tr, flow_const)``: edge k joins i[k] and j[k] with capacity
cap[k] there and rev[k] back, ``once`` is the flag of msg_add_label_edges (0 on every solve case), tr the merged t-links (> 0 from
the source, < 0 to the sink), flow_const what ``maxflow()`` adds to the capacity of the cut.

* ``expected_arcs``: Graph::sum_edge as k_msg_arc_sums promises it, in plain Python.
* ``expected_cut``: the labels every maximum flow has (oracle/exact_maxflow.py: Dinic in Python integers) and the capacity of that cut
  as a rational.  Every solve case has at most 6 000 nodes, so the exact oracle applies.
* ``check_arcs``: the comparison of a read-back with ``expected_arcs``; it takes arrays, so that the CPU tier can hand it doctored
  ones and require each to be rejected with a named arc.
"""
from fractions import Fraction

import numpy as np

from oracle import exact_maxflow

_CACHE = {}


# ---- expected values -----------------------------------------------------------------------------------------------------------------

def expected_arcs(n, i, j, cap, rev, once=None):
    """(tail, head, cap) of every distinct directed arc, sorted by (tail, head): for each edge in insertion order
    ``arc[(i, j)] += cap`` and ``arc[(j, i)] += rev``, sequential float64 additions starting from 0.0.  An edge flagged ``once``
    counts only at its first appearance per directed arc.  Both directions exist even where a capacity is 0."""
    i, j = np.asarray(i, np.int64).tolist(), np.asarray(j, np.int64).tolist()
    cap, rev = np.asarray(cap, np.float64).tolist(), np.asarray(rev, np.float64).tolist()
    once = [0] * len(i) if once is None else np.asarray(once).tolist()
    arc, seen_once = {}, set()
    for a, b, c, r, o in zip(i, j, cap, rev, once):
        assert 0 <= a < n and 0 <= b < n and a != b, (a, b, n)
        for key, w in (((a, b), c), ((b, a), r)):
            if o:
                if key in seen_once:
                    continue
                seen_once.add(key)
            arc[key] = arc.get(key, 0.0) + w
    keys = sorted(arc)
    tail = np.array([k[0] for k in keys], np.int32)
    head = np.array([k[1] for k in keys], np.int32)
    return tail, head, np.array([arc[k] for k in keys], np.float64)


def merged_edges(n, i, j, cap, rev, once=None):
    """the graph AS BUILT as an edge list without repeated pairs: (i, j, cap, rev) with i < j, capacities those of ``expected_arcs``"""
    tail, head, c = expected_arcs(n, i, j, cap, rev, once)
    fwd = tail < head
    back = {(int(a), int(b)): float(w) for a, b, w in zip(tail[~fwd], head[~fwd], c[~fwd])}
    mi, mj, mc = tail[fwd].astype(np.int64), head[fwd].astype(np.int64), c[fwd]
    mr = np.array([back[(int(b), int(a))] for a, b in zip(mi, mj)], np.float64)
    return mi, mj, mc, mr


def expected_cut(n, i, j, cap, rev, tr, flow_const=0.0):
    """(labels, flow) of the graph as built.  Labels: uint8, 1 where the node cannot reach the sink in the residual graph of a maximum
    flow -- the complement of ``canonical_sink_side``, the one label set every maximum flow has.  Flow: the capacity of that cut as a
    rational plus ``flow_const``, rounded once.  Repeated pairs are summed first, as the library sums them (``merged_edges``): the
    cut is that of the float64 capacities the solver sees."""
    mi, mj, mc, mr = merged_edges(n, i, j, cap, rev)
    tr = np.asarray(tr, np.float64)
    sink_side = exact_maxflow.canonical_sink_side(n, mi, mj, mc, mr, tr)
    assert sink_side is not None, "%d nodes: beyond the exact oracle" % n
    src = ~sink_side
    total = Fraction(float(flow_const))
    for c in mc[src[mi] & ~src[mj]].tolist():
        total += Fraction(c)
    for c in mr[src[mj] & ~src[mi]].tolist():
        total += Fraction(c)
    for c in tr[(tr > 0) & ~src].tolist():
        total += Fraction(c)
    for c in tr[(tr < 0) & src].tolist():
        total += Fraction(-c)
    return src.astype(np.uint8), float(total)


def check_arcs(got, want, what, rel=None):
    """``got`` = (tail, head, cap) as read back, ``want`` that of ``expected_arcs``.  The arc lists must be the same; the capacities
    bit for bit (``rel`` None) or within ``rel`` of the expected one.  The message names the first arc that is lost, made up,
    misplaced or carries another capacity."""
    gt, gh, gc = (np.asarray(a) for a in got)
    wt, wh, wc = (np.asarray(a) for a in want)
    gkeys = list(zip(gt.tolist(), gh.tolist()))
    wkeys = list(zip(wt.tolist(), wh.tolist()))
    if gkeys != wkeys:
        gs, ws = set(gkeys), set(wkeys)
        lost, extra = sorted(ws - gs), sorted(gs - ws)
        assert not lost, "%s: arc %s is missing (%d missing, %d arcs read, %d expected)" % (what, lost[0], len(lost), len(gkeys), len(wkeys))
        assert not extra, "%s: arc %s does not belong to the graph (%d such)" % (what, extra[0], len(extra))
        assert len(gkeys) == len(gs), "%s: an arc appears twice (%d arcs read, %d distinct)" % (what, len(gkeys), len(gs))
        k = next(k for k, (a, b) in enumerate(zip(gkeys, wkeys)) if a != b)
        raise AssertionError("%s: arcs are not sorted by (tail, head): entry %d is %s, expected %s" % (what, k, gkeys[k], wkeys[k]))
    assert gt.dtype == np.int32 and gh.dtype == np.int32 and gc.dtype == np.float64, (gt.dtype, gh.dtype, gc.dtype)
    if rel is None:
        if gc.tobytes() != wc.tobytes():
            bad = np.flatnonzero(gc.view(np.uint64) != wc.view(np.uint64))
            k = int(bad[0])
            raise AssertionError("%s: arc %s carries %r, expected %r (%d arcs differ)" % (what, wkeys[k], float(gc[k]), float(wc[k]), bad.size))
    else:
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero(~(np.abs(gc - wc) <= rel * np.abs(wc)) & ~((gc == wc) | (np.isnan(gc) & np.isnan(wc))))
        if bad.size:
            k = int(bad[0])
            raise AssertionError("%s: arc %s carries %r, expected %r within rel %g (%d arcs differ)" % (what, wkeys[k], float(gc[k]), float(wc[k]), rel, bad.size))


def rows_of(n, tail):
    """CSR row starts of a sorted tail array (what k_msg_rows finds by binary search)"""
    return np.searchsorted(np.asarray(tail), np.arange(n + 1), side="left")


# ---- generators ----------------------------------------------------------------------------------------------------------------------

def _pack(n, i, j, cap, rev, tr, flow_const=0.0):
    i, j = np.asarray(i, np.int64).reshape(-1), np.asarray(j, np.int64).reshape(-1)
    cap, rev = np.asarray(cap, np.float64).reshape(-1), np.asarray(rev, np.float64).reshape(-1)
    assert i.size == j.size == cap.size == rev.size and not (i == j).any()
    tr = np.asarray(tr, np.float64)
    assert tr.shape == (n,) and n <= 6000
    return int(n), i, j, cap, rev, np.zeros(i.size, np.uint8), tr, float(flow_const)


def _chain(n, rng, lo=2, hi=8):
    k = np.arange(n - 1)
    return k, k + 1, rng.integers(lo, hi + 1, n - 1).astype(float), rng.integers(lo, hi + 1, n - 1).astype(float)


def path2000():
    """chain of 2 000 nodes, whole-number capacities 2..8, the arc 1200 -> 1201 of capacity 1; 10 units enter at node 0, node n - 1
    drains 10.  One unit gets through; nine stay sealed behind the bottleneck and nodes 0..1200 must end at MSG_HINF.  Deeper than
    rounds_per_relabel (64) and than the 8 relabel passes between two looks at the counter, many times over."""
    n = 2000
    rng = np.random.default_rng(2000)
    i, j, cap, rev = _chain(n, rng)
    cap[1200] = 1.0
    tr = np.zeros(n)
    tr[0], tr[-1] = 10.0, -10.0
    return _pack(n, i, j, cap, rev, tr, 3.0)


def path300_two_bottlenecks():
    """chain of 300: arcs of capacity 1 next to both ends (2 -> 3 and 296 -> 297), an exact tie between two minimum cuts"""
    n = 300
    rng = np.random.default_rng(300)
    i, j, cap, rev = _chain(n, rng)
    cap[2], cap[296] = 1.0, 1.0
    tr = np.zeros(n)
    tr[0], tr[-1] = 7.0, -7.0
    return _pack(n, i, j, cap, rev, tr)


def hub5000():
    """star: node 0 joined to 5 000 leaves, 1..4 from the hub to the leaf, 0..4 back (a fifth of the back arcs carry 0), leaf t-links
    in -3..3.  One thread walks a 5 000-arc row; k_msg_reverse searches it for every leaf."""
    m = 5000
    rng = np.random.default_rng(5000)
    leaves = np.arange(1, m + 1)
    tr = np.concatenate([[0.0], rng.integers(-3, 4, m).astype(float)])
    return _pack(m + 1, np.zeros(m, np.int64), leaves, rng.integers(1, 5, m), rng.integers(0, 5, m), tr)


def two_hubs():
    """two stars of 1 500 leaves; sources under hub 0, sinks under hub 1, and ONE arc hub 0 -> hub 1 (capacity 1 000, nothing back)
    that all flow has to take: it is the minimum cut unless the leaves' own arcs are"""
    m = 1500
    rng = np.random.default_rng(1500)
    a_leaves, b_leaves = np.arange(2, 2 + m), np.arange(2 + m, 2 + 2 * m)
    i = np.concatenate([a_leaves, np.full(m, 1), [0]])
    j = np.concatenate([np.full(m, 0), b_leaves, [1]])
    cap = np.concatenate([rng.integers(1, 5, m), rng.integers(1, 5, m), [1000]])
    rev = np.concatenate([rng.integers(0, 3, m), rng.integers(0, 3, m), [0]])
    tr = np.zeros(2 + 2 * m)
    tr[a_leaves] = rng.integers(1, 4, m)
    tr[b_leaves] = -rng.integers(1, 4, m)
    return _pack(2 + 2 * m, i, j, cap, rev, tr, 0.5)


def k40_40_ties():
    """complete bipartite 40 + 40, one-way whole-number capacities 0..2 from left to right, sources left, sinks right: dense, exact
    ties, many admissible arcs side by side"""
    rng = np.random.default_rng(4040)
    left, right = np.meshgrid(np.arange(40), np.arange(40, 80), indexing="ij")
    tr = np.concatenate([rng.integers(1, 41, 40), -rng.integers(1, 41, 40)]).astype(float)
    return _pack(80, left.ravel(), right.ravel(), rng.integers(0, 3, 1600), np.zeros(1600), tr)


def ring_chords_ties():
    """ring of 1 500 plus a chord from every 7th node to the node opposite, whole-number capacities 0..3 both ways, a tenth of the
    nodes with t-links in -5..5: cycles, arcs of capacity 0, ties"""
    n = 1500
    rng = np.random.default_rng(1507)
    k = np.arange(n)
    chords = np.arange(0, n // 2, 7)
    i = np.concatenate([k, chords])
    j = np.concatenate([(k + 1) % n, chords + n // 2])
    tr = np.where(rng.random(n) < 0.1, rng.integers(-5, 6, n), 0).astype(float)
    return _pack(n, i, j, rng.integers(0, 4, i.size), rng.integers(0, 4, i.size), tr)


def _random_edges(rng, n, m):
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = i != j
    return i[keep], j[keep]


def random3000():
    """3 000 nodes, about 9 000 random edges (a few pairs repeat), float capacities in (0, 1), t-links N(0, 1): a unique cut"""
    n = 3000
    rng = np.random.default_rng(3000)
    i, j = _random_edges(rng, n, 9000)
    return _pack(n, i, j, rng.uniform(1e-9, 1.0, i.size), rng.uniform(1e-9, 1.0, i.size), rng.normal(0.0, 1.0, n), 0.25)


def wide_range():
    """500 nodes, 2 000 random edges, capacities and t-links 10**uniform(-6, 6): the rounding of ``e -= d`` at twelve decades"""
    n = 500
    rng = np.random.default_rng(500)
    i, j = _random_edges(rng, n, 2000)
    tr = np.where(rng.random(n) < 0.4, 10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1.0, 1.0], n), 0.0)
    return _pack(n, i, j, 10.0 ** rng.uniform(-6, 6, i.size), 10.0 ** rng.uniform(-6, 6, i.size), tr)


def one_way_away():
    """chain of 300 whose arcs all point away from the sink (node 0 drains, every arc k -> k + 1, nothing back), 9 units enter at the
    far end: the source cannot reach the sink, the flow is the constant alone"""
    n = 300
    rng = np.random.default_rng(301)
    k = np.arange(n - 1)
    tr = np.zeros(n)
    tr[0], tr[-1] = -9.0, 9.0
    return _pack(n, k, k + 1, rng.integers(1, 6, n - 1), np.zeros(n - 1), tr, 2.5)


def duplicates3000():
    """50 nodes; the pair (3, 7) given 3 000 times with float capacities, as (3, 7) and as (7, 3) mixed, among 200 random edges: one
    long run in k_msg_arc_sums, whose sum depends on the order of the additions"""
    n = 50
    rng = np.random.default_rng(3007)
    oi, oj = _random_edges(rng, n, 200)
    flip = rng.random(3000) < 0.5
    di, dj = np.where(flip, 7, 3), np.where(flip, 3, 7)
    i, j = np.concatenate([oi, di]), np.concatenate([oj, dj])
    order = rng.permutation(i.size)
    cap, rev = 10.0 ** rng.uniform(-3, 0, i.size), 10.0 ** rng.uniform(-3, 0, i.size)
    return _pack(n, i[order], j[order], cap, rev, rng.normal(0.0, 40.0, n))


def _component_edges(rng, size, m, offset):
    i, j = _random_edges(rng, size, m)
    return i + offset, j + offset, rng.integers(1, 6, i.size).astype(float), rng.integers(1, 6, i.size).astype(float)


COMPONENT_SIZE = 200


def components():
    """five disjoint random graphs of 200 nodes, whole-number capacities: (0) sources and sinks, (1) sources only, (2) sinks only,
    (3) neither, (4) sources in its first half and sinks in its second with capacity 0 on every arc between the halves -- sealed-in
    excess, trees that never meet"""
    s = COMPONENT_SIZE
    rng = np.random.default_rng(5200)
    parts = [_component_edges(rng, s, 600, c * s) for c in range(5)]
    i, j, cap, rev = (np.concatenate([p[k] for p in parts]) for k in range(4))
    half = 4 * s + s // 2
    across = (i >= 4 * s) & ((i < half) != (j < half))
    cap[across], rev[across] = 0.0, 0.0
    tr = np.zeros(5 * s)
    kind = rng.integers(-4, 5, 5 * s).astype(float) * (rng.random(5 * s) < 0.3)
    node = np.arange(5 * s)
    tr[node < s] = kind[node < s]
    tr[(node >= s) & (node < 2 * s)] = np.abs(kind[(node >= s) & (node < 2 * s)])
    tr[(node >= 2 * s) & (node < 3 * s)] = -np.abs(kind[(node >= 2 * s) & (node < 3 * s)])
    tr[(node >= 4 * s) & (node < half)] = np.abs(kind[(node >= 4 * s) & (node < half)])
    tr[node >= half] = -np.abs(kind[node >= half])
    return _pack(5 * s, i, j, cap, rev, tr, 1.0)


def components_joined():
    """``components`` and four edges added after a first solve: component 1 (sources only) gets arcs into component 2 (sinks only)"""
    n, i, j, cap, rev, once, tr, fc = components()
    s = COMPONENT_SIZE
    ni = np.array([s + 3, s + 50, s + 120, 2 * s + 9])
    nj = np.array([2 * s + 7, 2 * s + 90, 2 * s + 150, s + 77])
    ncap, nrev = np.array([3.0, 2.0, 4.0, 0.0]), np.array([0.0, 1.0, 0.0, 5.0])
    return _pack(n, np.concatenate([i, ni]), np.concatenate([j, nj]), np.concatenate([cap, ncap]), np.concatenate([rev, nrev]), tr, fc)


def isolated_tlinks():
    """64 nodes and NO edges (the n2 == 0 branch of msg_build): labels by the sign of the t-link, 0 -> source side"""
    n = 64
    tr = np.tile([2.5, -1.5, 0.0, -0.25], n // 4)
    e = np.zeros(0)
    return _pack(n, e, e, e, e, tr, 0.75)


def no_sink():
    """random3000's arcs, every negative t-link 0: nothing drains, all labels 1 at the first count"""
    n, i, j, cap, rev, once, tr, fc = random3000()
    return _pack(n, i, j, cap, rev, np.maximum(tr, 0.0), fc)


def no_source():
    """random3000's arcs, every positive t-link 0: no excess, the labels are the sink tree alone"""
    n, i, j, cap, rev, once, tr, fc = random3000()
    return _pack(n, i, j, cap, rev, np.minimum(tr, 0.0), fc)


def end_nodes():
    """40 nodes, edges only among nodes 10..19, t-links on nodes 0 and 39 (and on 12 and 17, so that flow moves): empty CSR rows at
    the front, in the middle and at the end"""
    n = 40
    rng = np.random.default_rng(40)
    i, j = _random_edges(rng, 10, 30)
    i, j = i + 10, j + 10
    keep = ~(((i == 14) | (j == 14)))   # node 14: an empty row between two filled ones
    i, j = i[keep], j[keep]
    tr = np.zeros(n)
    tr[0], tr[39], tr[12], tr[17] = 4.0, -4.0, 6.0, -6.0
    return _pack(n, i, j, rng.integers(1, 4, i.size), rng.integers(0, 4, i.size), tr)


SOLVE_CASES = {f.__name__: f for f in (path2000, path300_two_bottlenecks, hub5000, two_hubs, k40_40_ties, ring_chords_ties, random3000, wide_range,
                                       one_way_away, duplicates3000, components, isolated_tlinks, no_sink, no_source, end_nodes)}
SOLVE_NAMES = list(SOLVE_CASES)
# whole-number capacities and t-links (flow constants in halves and quarters): every sum any solver forms is exact, the flow is compared bit for bit
INTEGER_CASES = ("path2000", "path300_two_bottlenecks", "hub5000", "two_hubs", "k40_40_ties", "ring_chords_ties", "one_way_away", "components",
                 "isolated_tlinks", "end_nodes")
# shallow enough that rounds_per_relabel = 1 stays cheap (path2000 takes 2.3 M relabel passes there in the host simulator)
SWEEP_CASES = ("path300_two_bottlenecks", "k40_40_ties", "ring_chords_ties", "components")
BUILD_CASES = ("duplicates3000", "hub5000", "end_nodes", "k40_40_ties")
# a node that many arcs meet in, per case (msg_what_segment is asked about the first node, the last and this one)
HUB = {"hub5000": 0, "two_hubs": 1, "duplicates3000": 3, "k40_40_ties": 40}
EXTRA_CASES = {"components_joined": components_joined}


def case(name):
    """the arrays of a case, generated once per process"""
    if ("case", name) not in _CACHE:
        _CACHE[("case", name)] = (SOLVE_CASES.get(name) or EXTRA_CASES[name])()
    return _CACHE[("case", name)]


def arcs_of(name):
    """``expected_arcs`` of a case, computed once per process"""
    if ("arcs", name) not in _CACHE:
        n, i, j, cap, rev, once, tr, fc = case(name)
        _CACHE[("arcs", name)] = expected_arcs(n, i, j, cap, rev, once)
    return _CACHE[("arcs", name)]


def cut_of(name):
    """``expected_cut`` of a case, solved once per process"""
    if ("cut", name) not in _CACHE:
        n, i, j, cap, rev, once, tr, fc = case(name)
        _CACHE[("cut", name)] = expected_cut(n, i, j, cap, rev, tr, fc)
    return _CACHE[("cut", name)]


def is_integer_case(name):
    return name in INTEGER_CASES or name == "components_joined"


def assert_flow(flow, want, name, what):
    """bit-equal on the whole-number cases, within rel 1e-12 otherwise (the figure include/medpy_hip.h gives for msg_maxflow)"""
    if is_integer_case(name):
        assert flow == want, "%s %s: flow %r, expected exactly %r" % (name, what, flow, want)
    else:
        assert abs(flow - want) <= 1e-12 * abs(want), "%s %s: flow %r, expected %r within rel 1e-12" % (name, what, flow, want)


def assert_labels(labels, want, name, what):
    labels, want = np.asarray(labels).astype(np.uint8).ravel(), np.asarray(want).astype(np.uint8).ravel()
    bad = np.flatnonzero(labels != want)
    assert not bad.size, "%s %s: %d of %d labels differ from the exact cut, first at node %d (got %d)" % (name, what, bad.size, want.size, int(bad[0]), int(labels[bad[0]]))

"""CPU tier of the sparse-graph cases (tests/sparse_cases.py): before a case goes to the GPU (test_gpu_sparse_solve.py,
test_gpu_sparse_build.py) its expected values are pinned here against two independent programs -- the compiled BK oracle
(oracle/bk.py) and the host simulator, which runs the node operations and the schedule of msg_node_ops.inl one node after the other
(tests/hostsim/hostsim_sparse.cpp, through ``sim_solve`` of test_label_oracle.py).  A case whose answer hinges on rounding fails here
and is changed, not relaxed.  The comparison the GPU build tests use (``check_arcs``) is fed doctored arrays and must reject each."""
import numpy as np
import pytest

import sparse_cases as sc
from oracle import bk
from test_label_oracle import sim_solve


def _bk_graph(name):
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    g = bk.BKGraph(n, max(16, i.size))
    if i.size:
        g.sum_edges(i, j, cap, rev)
    g.add_tweights(None, np.maximum(tr, 0.0), np.maximum(-tr, 0.0))
    return g


def test_every_case_is_small_enough_for_the_exact_oracle_and_named_once():
    assert len(sc.SOLVE_NAMES) == 15 and set(sc.SWEEP_CASES) <= set(sc.SOLVE_NAMES) and set(sc.BUILD_CASES) <= set(sc.SOLVE_NAMES)
    for name in sc.SOLVE_NAMES + list(sc.EXTRA_CASES):
        n, i, j, cap, rev, once, tr, fc = sc.case(name)
        assert n <= 6000 and not once.any()
        assert np.isfinite(cap).all() and np.isfinite(rev).all() and (cap >= 0).all() and (rev >= 0).all() and np.isfinite(tr).all()
        if sc.is_integer_case(name):
            for a in (cap, rev, tr):   # whole numbers (quarters on the t-links of isolated_tlinks): every sum is exact
                assert np.array_equal(4 * a, np.floor(4 * a)) and np.abs(a).max(initial=0.0) <= 1000


def test_the_cases_reach_what_they_are_for():
    """the properties the table of cases promises, read off the arrays and the exact cut"""
    lab, flow = sc.cut_of("path2000")
    assert lab[:1201].all() and not lab[1201:].any() and flow == 3.0 + 1.0   # nine units sealed behind the bottleneck
    lab, flow = sc.cut_of("path300_two_bottlenecks")
    assert lab[:297].all() and not lab[297:].any() and flow == 1.0   # of the two tied cuts the one next to the sink
    tail, head, cap = sc.arcs_of("hub5000")
    rows = sc.rows_of(5001, tail)
    assert rows[1] - rows[0] == 5000 and (cap[tail != 0] == 0).sum() > 500   # one row of 5 000 arcs, many zero back arcs
    lab, flow = sc.cut_of("two_hubs")
    assert flow == 0.5 + 1000.0 and lab[0] == 1 and lab[1] == 0   # the one arc between the hubs is the cut
    lab, flow = sc.cut_of("one_way_away")
    assert flow == 2.5 and lab[0] == 0 and lab[1:].all()
    lab, flow = sc.cut_of("isolated_tlinks")
    tr = sc.case("isolated_tlinks")[6]
    assert np.array_equal(lab, (tr >= 0).astype(np.uint8)) and flow == 0.75
    lab, flow = sc.cut_of("no_sink")
    assert lab.all() and flow == 0.25
    lab, flow = sc.cut_of("no_source")
    assert flow == 0.25 and 0 < lab.sum() < lab.size   # nodes outside the sink tree stay at the source
    tail, head, cap = sc.arcs_of("end_nodes")
    deg = np.diff(sc.rows_of(40, tail))
    assert not deg[:10].any() and not deg[20:].any() and deg[14] == 0 and deg[13] and deg[15]
    tail, head, cap = sc.arcs_of("duplicates3000")
    n, i, j = sc.case("duplicates3000")[:3]
    assert ((i == 3) & (j == 7)).sum() > 1000 and ((i == 7) & (j == 3)).sum() > 1000
    lab, flow = sc.cut_of("components")
    s = sc.COMPONENT_SIZE
    assert lab[s:2 * s].all() and lab[3 * s:4 * s].all() and lab[4 * s:4 * s + s // 2].all() and not lab[2 * s:3 * s].all()
    lab2, flow2 = sc.cut_of("components_joined")
    assert flow2 > flow   # the new edges let component 1 drain into component 2


@pytest.mark.parametrize("name", sc.SOLVE_NAMES + ["components_joined"])
def test_expected_cut_agrees_with_bk(name):
    want_labels, want_flow = sc.cut_of(name)
    g = _bk_graph(name)
    flow = g.maxflow() + sc.case(name)[7]
    sc.assert_labels(g.labels(), want_labels, name, "BK")
    assert abs(flow - want_flow) <= 1e-12 * abs(want_flow), (name, flow, want_flow)


@pytest.mark.parametrize("name", sc.SOLVE_NAMES + ["components_joined"])
def test_host_simulator_reproduces_the_exact_cut(name):
    """rounds_per_relabel 0 (= 64), 1 and 7; 0 only for path2000 (2.3 M relabel passes at 1)"""
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    want_labels, want_flow = sc.cut_of(name)
    arcs = sc.arcs_of(name)[0].size
    for rounds in ((0,) if name == "path2000" else (0, 1, 7)):
        labels, cut, stats = sim_solve(n, i, j, cap, rev, once, tr, rounds=rounds)
        assert stats[4] == arcs
        sc.assert_labels(labels, want_labels, name, "host simulator, rounds_per_relabel %d" % rounds)
        sc.assert_flow(cut + fc, want_flow, name, "host simulator, rounds_per_relabel %d" % rounds)
    if name == "path2000":
        assert stats[0] > 64 * 8 and stats[2] > 8 * 100   # deeper than one batch of rounds and than many looks at the relabel counter


@pytest.mark.parametrize("name", ["duplicates3000", "random3000"])
def test_expected_arcs_against_bk_get_edge(name):
    """Graph::sum_edge of the compiled oracle, arc by arc; absent pairs read 0"""
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    tail, head, c = sc.arcs_of(name)
    g = _bk_graph(name)
    pick = np.arange(tail.size) if tail.size < 2000 else np.random.default_rng(1).choice(tail.size, 1500, replace=False)
    for k in pick.tolist():
        assert g.get_edge(int(tail[k]), int(head[k])) == c[k], (name, int(tail[k]), int(head[k]))
    have = set(zip(tail.tolist(), head.tolist()))
    rng = np.random.default_rng(2)
    absent = [(a, b) for a, b in rng.integers(0, n, (200, 2)).tolist() if a != b and (a, b) not in have][:20]
    assert len(absent) >= 5
    for a, b in absent:
        assert g.get_edge(a, b) == 0.0
    assert tail.size == 2 * len({(min(a, b), max(a, b)) for a, b in zip(i.tolist(), j.tolist())})


def test_expected_arcs_once_flag_and_order():
    """the ``once`` flag counts a repeated pair once per directed arc; unflagged repeats add up in insertion order"""
    big, small = 1e16, 1.0
    t, h, c = sc.expected_arcs(3, [0, 0, 0, 1], [1, 1, 1, 0], [big, small, -big, 5.0], [0.0, 0.0, 0.0, 0.0])
    assert t.tolist() == [0, 1] and h.tolist() == [1, 0]
    assert c[0] == (big + small) - big and c[1] == 5.0   # (1e16 + 1) - 1e16 = 0 in float64: the order is visible
    t, h, c = sc.expected_arcs(3, [0, 1, 0, 2], [1, 0, 1, 1], [2.0, 7.0, 2.0, 1.0], [3.0, 9.0, 3.0, 4.0], [1, 1, 1, 0])
    assert list(zip(t.tolist(), h.tolist(), c.tolist())) == [(0, 1, 2.0), (1, 0, 3.0), (1, 2, 4.0), (2, 1, 1.0)]
    t, h, c = sc.expected_arcs(4, [], [], [], [])
    assert t.size == 0 and t.dtype == np.int32 and c.dtype == np.float64


def _doctored(name):
    """read-backs a broken build would give, each with the word its rejection must carry"""
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    tail, head, c = sc.arcs_of(name)
    odd = np.arange(i.size) % 2 == 1
    yield "carries", sc.expected_arcs(n, i, j, np.where(odd, rev, cap), np.where(odd, cap, rev))   # ecap / erev swapped for odd entries
    yield "missing", (tail[:-1], head[:-1], c[:-1])
    yield "missing", (np.delete(tail, 5), np.delete(head, 5), np.delete(c, 5))
    yield "twice", (np.insert(tail, 5, tail[5]), np.insert(head, 5, head[5]), np.insert(c, 5, c[5]))
    swapped = np.arange(tail.size)
    swapped[[3, 4]] = [4, 3]
    yield "sorted", (tail[swapped], head[swapped], c[swapped])
    bumped = c.copy()
    bumped[11] = np.nextafter(bumped[11], np.inf)   # one ulp on one arc
    yield "carries", (tail, head, bumped)
    if name == "duplicates3000":   # the run of 3 000 added up back to front
        yield "carries", sc.expected_arcs(n, i[::-1], j[::-1], cap[::-1], rev[::-1])


@pytest.mark.parametrize("name", ["duplicates3000", "hub5000"])
def test_check_arcs_rejects_doctored_read_backs(name):
    want = sc.arcs_of(name)
    sc.check_arcs(want, want, name)
    for word, got in _doctored(name):
        with pytest.raises(AssertionError, match=word):
            sc.check_arcs(got, want, name)
    close = (want[0], want[1], want[2] * (1 + 1e-13))
    sc.check_arcs(close, want, name, rel=1e-12)
    with pytest.raises(AssertionError, match="carries"):
        sc.check_arcs((want[0], want[1], want[2] * (1 + 1e-11)), want, name, rel=1e-12)

"""What tests/test_cut_sets_tol_host.py (CPU tier) and tests/test_gpu_cut_sets_tol.py (-m gpu) share: the walls graphs with dust, the
BK oracle on them, and a NumPy restatement of the device's rule of mgc_cut_sets_tol over the oracle's residual graph.  Not a
test module.

The dusty graph: the walls graph of tests/test_gpu_cut_sets.py with every zero arc inside the volume replaced by 2^-80 and with a 2^-80
source or sink weight on 5 % of the voxels that hold no t-link.  In exact arithmetic its cut is unique (the dust decides every tie); what
a user means by it is the clean graph, and at 64 ulp the sets of the dusty graph must be the tol-0 sets of the clean one.
Generator condition (asserted): every voxel's scale -- its largest arc-pair capacity -- is at least 4, so that next to dust always
stands a weight of order 1; SEEDS lists, per case, the first generator seeds for which that holds."""
import numpy as np

from oracle import bk, cutcheck
from test_gpu_cut_sets import _arcs, walls_graph

ULP64 = 64 * 2.0 ** -52
DUST = 2.0 ** -80

# (shape, walls, neighbourhood or None for 2 * ndim)
CASES = [((20, 13, 27), (8, 17), None), ((9, 10, 33), (7, 15, 24), None), ((17, 17, 17), (5, 10), None), ((8, 8, 8), (2, 4), None),
         ((9, 9, 17), (3, 7, 11), None), ((19, 26), (8, 16), None), ((41,), (9, 20, 30), None),
         ((8, 8, 8), (2, 4), 26), ((9, 9, 17), (3, 7, 11), 26), ((19, 26), (8, 16), 8)]
CASE_IDS = ["x".join(map(str, s)) + ("_n%d" % c if c else "") for s, _, c in CASES]
N_SEEDS = 2
_CACHE = {}


def scale_as_built(shape, nw):
    """per voxel, the largest there + back over the arc pairs at it"""
    s = np.zeros(int(np.prod(shape)))
    for o, (there, back) in nw.items():
        mask, i, j = _arcs(shape, o)
        pair = there[mask] + back[mask]
        np.maximum.at(s, i, pair)
        np.maximum.at(s, j, pair)
    return s.reshape(shape)


def dusty(shape, nw, source, sink, seed):
    """the same graph with dust: (nw, source, sink), new arrays"""
    rng = np.random.default_rng(1000 + seed)
    out = {}
    for o, (there, back) in nw.items():
        mask, _, _ = _arcs(shape, o)
        t, b = there.copy(), back.copy()
        t[mask & (t == 0)] = DUST
        b[mask & (b == 0)] = DUST
        out[o] = (t, b)
    free = (source == 0) & (sink == 0)
    pick = free & (rng.random(shape) < 0.05)
    which = rng.random(shape) < 0.5
    source, sink = source.copy(), sink.copy()
    source[pick & which] = DUST
    sink[pick & ~which] = DUST
    return out, source, sink


def seeds_of(case):
    """the first N_SEEDS generator seeds of a case whose every voxel has scale >= 4 (1-D volumes can produce all-dust voxels)"""
    key = ("seeds", case)
    if key not in _CACHE:
        shape, walls, conn = CASES[case]
        good = []
        for seed in range(64):
            nw, _, _ = walls_graph(shape, walls, seed, conn)
            if scale_as_built(shape, nw).min() >= 4.0:
                good.append(seed)
            if len(good) == N_SEEDS:
                break
        assert len(good) == N_SEEDS, (CASE_IDS[case], good)
        _CACHE[key] = good
    return _CACHE[key]


def graphs(case, seed):
    """{"clean": (nw, source, sink), "dusty": (...)} of one case, each generated once"""
    key = ("graphs", case, seed)
    if key not in _CACHE:
        shape, walls, conn = CASES[case]
        clean = walls_graph(shape, walls, seed, conn)
        assert scale_as_built(shape, clean[0]).min() >= 4.0    # the generator condition
        _CACHE[key] = {"clean": clean, "dusty": dusty(shape, *clean, seed)}
    return _CACHE[key]


def scaled(graph, factor):
    nw, source, sink = graph
    return {o: (t * factor, b * factor) for o, (t, b) in nw.items()}, source * factor, sink * factor


def side_by_side(shape, first, second):
    """two graphs of one shape next to each other along axis 0, every arc between them 0: (shape, nw, source, sink)"""
    n0 = shape[0]
    big = (2 * n0,) + tuple(shape[1:])
    nw = {}
    for o in first[0]:
        pair = []
        for a, b in zip(first[0][o], second[0][o]):
            a = a.copy()
            if o[0] > 0:
                a[n0 - 1] = 0.0      # p -> p + o (and back) across the seam
            elif o[0] < 0:
                b = b.copy()
                b[0] = 0.0
            pair.append(np.concatenate([a, b], axis=0))
        nw[o] = tuple(pair)
    return big, nw, np.concatenate([first[1], second[1]], axis=0), np.concatenate([first[2], second[2]], axis=0)


def bk_solve(shape, nw, source, sink):
    """the solved BK graph and its flow"""
    n = int(np.prod(shape))
    g = bk.BKGraph(n, n * 13 + 16)
    g.add_tweights(None, np.asarray(source, np.float64).ravel(), np.asarray(sink, np.float64).ravel())
    for o, (there, back) in nw.items():
        mask, i, j = _arcs(shape, o)
        g.sum_edges(i, j, there[mask], back[mask])
    return g, g.maxflow()


def bk_tol0(key, shape, nw, source, sink):
    """(flow, from_source, to_sink, ambiguous) of BK at tol 0, once per key"""
    if key not in _CACHE:
        g, flow = bk_solve(shape, nw, source, sink)
        _CACHE[key] = (flow,) + tuple(a.reshape(shape) for a in cutcheck.ambiguity(g, tol=0.0))
    return _CACHE[key]


def clean_sets(case, seed):
    shape = CASES[case][0]
    return bk_tol0(("clean", case, seed), shape, *graphs(case, seed)["clean"])


def _closure(n, frm, to, seeds):
    """the nodes reachable from ``seeds`` along the arcs frm[k] -> to[k]"""
    order = np.argsort(frm, kind="stable")
    frm, to = frm[order], to[order]
    start = np.searchsorted(frm, np.arange(n + 1))
    mark = seeds.copy()
    frontier = np.flatnonzero(seeds)
    while frontier.size:
        cnt = start[frontier + 1] - start[frontier]
        first = np.repeat(start[frontier], cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        nb = np.unique(to[first + within])
        frontier = nb[~mark[nb]]
        mark[frontier] = True
    return mark


def device_rule(g, tr0, tol):
    """(from_source, to_sink, ambiguous) by the DEVICE's rule (medpy_amd/csrc/mgc_reach_tol.h) on the residual graph of a solved
    BKGraph.  tr0: the merged t-links as built (source weight - sink weight).  BK's residual t-link stands in for what the device holds
    of it: > 0 for the excess, < 0 for the residual sink link."""
    tail, head, rcap, trcap = g.export()
    tail, head = tail.astype(np.int64), head.astype(np.int64)
    n = trcap.size
    pair = rcap + rcap[np.arange(rcap.size) ^ 1]
    scale = np.zeros(n)
    np.maximum.at(scale, tail, pair)
    np.maximum.at(scale, head, pair)
    is_open = (rcap > 0) & (rcap > tol * np.maximum(scale[tail], scale[head]))
    t_scale = tol * np.maximum(np.abs(np.asarray(tr0, np.float64).ravel()), scale)
    src_seed = (trcap > 0) & (trcap > t_scale)
    snk_seed = (-trcap > 0) & (-trcap > t_scale)
    fs = _closure(n, tail[is_open], head[is_open], src_seed)
    ts = _closure(n, head[is_open], tail[is_open], snk_seed)
    return fs, ts, ~(fs | ts)

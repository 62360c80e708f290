"""CPU tier: every schedule knob of MgcSolveParams against the BK oracle, on the host simulator.

The simulator runs the same ``mgc_solve`` text (medpy_amd/csrc/mgc_driver.inl) as the library, on simulator slabs (the Z-slab schedule
with its border exchanges) and on the single simulator handle.  The contract: whatever schedule a caller picks, the labels are the
reference BK's voxel for voxel and the solve says it converged.  The slab knobs are swept as a covering design (every pair of values
of every two knobs in at least one row) instead of their full product; the single handle takes one knob at a time at its edges."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hostsim"))

_CACHE = {}


def _volume(name):
    """(connectivity, shape, simulator weights, t-links, BK labels): sphere (32,16,24) seed 1, sphere (40,24,16), hard 24^3 and a
    26-neighbourhood sphere 24^3 with a regional term"""
    if name in _CACHE:
        return _CACHE[name]
    import sim
    from medpy_amd import synthetic
    from oracle import energy_numpy, pipeline
    gen, shape, conn, kw = {"sphere32x16x24s1": ("sphere", (32, 16, 24), 6, {"seed": 1}), "sphere40x24x16": ("sphere", (40, 24, 16), 6, {}),
                            "hard24": ("hard", (24, 24, 24), 6, {}), "sphere24_n26_regional": ("sphere", (24, 24, 24), 26, {})}[name]
    s = getattr(synthetic, gen)(shape, **kw)
    if conn == 6:
        w = energy_numpy.boundary_weights(s["term"], s["image"], s["sigma"])
        g = pipeline.build_graph(s["fg"], s["bg"], weights=w)
    else:
        r = synthetic.regional(shape)
        w = energy_numpy.boundary_weights_offsets(s["term"], s["image"], energy_numpy.forward_offsets(3, 26), s["sigma"])
        g = pipeline.build_graph(s["fg"], s["bg"], weights=w, connectivity=26, prob=r["prob"], alpha=r["alpha"])
    tr = np.array([g.get_trcap(i) for i in range(s["fg"].size)])
    g.maxflow()
    ref = g.labels().reshape(shape).astype(bool)
    _CACHE[name] = (conn, shape, w if conn == 6 else sim.weights26(shape, w), w, tr, ref)
    return _CACHE[name]


def _solve_slabs(name, nslabs, **knobs):
    import sim
    from medpy_amd.slab import LoopbackExchange, solve_slabs
    conn, shape, wsim, _, tr, ref = _volume(name)
    cls = sim.SimSlab if conn == 6 else sim.SimSlab26
    slabs = [cls(shape, r, nslabs) for r in range(nslabs)]
    for s in slabs:
        s.load(wsim, tr)
    st = solve_slabs(slabs, LoopbackExchange(slabs), **knobs)
    labels = np.concatenate([s.finish()[0] for s in slabs], axis=0)
    for s in slabs:
        s.close()
    return labels, ref, st


def _assert_cut(labels, ref, st, what):
    assert st["converged"] == 1, (what, st)
    bad = int((labels != ref).sum())
    assert bad == 0, "%s: %d voxels differ from BK (%d foreground instead of %d)" % (what, bad, int(labels.sum()), int(ref.sum()))


# ---- the Z-slab schedule ------------------------------------------------------------------------------------------------------------
SLAB_KNOBS = {  # solve_slabs keyword -> values (exchange_every is MgcSolveParams::exchange_passes)
    "exchange_rounds": (1, 2, 3, 4, 5, 6, 7, 8),
    "check_rounds": (1, 2, 3, 5, 8),
    "stop_below": (0, 1, 10 ** 6),
    "rounds_per_relabel": (1, 3, 64),
    "exchange_every": (1, 3, 8),
    "relabel_batch": (1, 3),
}
SLAB_VOLUMES = {"sphere32x16x24s1": (2, 3, 4), "sphere40x24x16": (2, 3, 4), "hard24": (2, 3), "sphere24_n26_regional": (2, 3)}


def covering_design(factors, seed=0, candidates=40):
    """rows (dicts) in which every pair of values of every two factors appears at least once: greedy, each row the best of
    ``candidates`` random ones that start from an uncovered pair (deterministic for a seed)"""
    names = list(factors)
    todo = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in factors[a] for vb in factors[b]}
    rng = np.random.default_rng(seed)
    rows = []
    while todo:
        first = sorted(todo, key=repr)[0]
        best, gain = None, -1
        for _ in range(candidates):
            row = {n: factors[n][rng.integers(len(factors[n]))] for n in names}
            row[first[0]], row[first[2]] = first[1], first[3]
            g = sum((a, row[a], b, row[b]) in todo for a, b in itertools.combinations(names, 2))
            if g > gain:
                best, gain = row, g
        rows.append(best)
        todo -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(names, 2)}
    return rows


def _slab_cases():
    out = []
    for vi, (name, nslabs) in enumerate(SLAB_VOLUMES.items()):
        factors = dict(SLAB_KNOBS, nslabs=nslabs)
        for row in covering_design(factors, seed=vi):
            kw = dict(row)
            n = kw.pop("nslabs")
            tag = "%s-%dslabs-" % (name, n) + "-".join("%s%d" % (k, v) for k, v in kw.items())
            out.append(pytest.param(name, n, kw, id=tag))
    return out


def test_covering_design_covers_every_pair():
    factors = dict(SLAB_KNOBS, nslabs=(2, 3, 4))
    rows = covering_design(factors)
    for a, b in itertools.combinations(factors, 2):
        seen = {(r[a], r[b]) for r in rows}
        assert seen == set(itertools.product(factors[a], factors[b])), (a, b)
    assert len(rows) < 60  # (the full product is 8640 rows)


@pytest.mark.parametrize("name,nslabs,kw", _slab_cases())
def test_slab_schedule_knobs_reach_the_oracle_cut(name, nslabs, kw):
    labels, ref, st = _solve_slabs(name, nslabs, **kw)
    _assert_cut(labels, ref, st, kw)


@pytest.mark.parametrize("exchange_rounds", [1, 2, 3, 5, 7])
def test_border_flow_is_delivered_before_an_early_end_of_the_rounds(exchange_rounds):
    """Regression: with exchange_rounds 3 or 5 the colour rounds of a cycle broke at the check after round 8 -- no exchange in that
    round -- with flow still in the outboxes that face a ghost tile.  The next activation found no work, and the solve reported
    converged with 8 foreground voxels where BK has 480 (mgc_driver.inl: a round that may end the cycle always exchanges)."""
    labels, ref, st = _solve_slabs("sphere32x16x24s1", 4, rounds_per_relabel=64, exchange_rounds=exchange_rounds)
    assert int(ref.sum()) == 480  # (True: the source side)
    _assert_cut(labels, ref, st, exchange_rounds)


@pytest.mark.parametrize("gen,shape,nslabs,counts", [
    ("sphere", (32, 24, 24), 2, (14, 18, 32, 3)), ("sphere", (40, 24, 16), 3, (13, 18, 24, 3)), ("hard", (32, 32, 32), 4, (27, 34, 63, 4)),
    ("sphere", (21, 16, 24), 2, (8, 16, 14, 2)), ("sphere", (64, 16, 16), 8, (14, 18, 32, 3))])
def test_default_schedule_is_launch_for_launch_unchanged(gen, shape, nslabs, counts):
    """At the defaults (check_rounds 8, a multiple of exchange_rounds 2) the exchange in a round that may end the cycle is one the
    schedule made anyway: exchanges, colour phases, relabel passes and global relabels of the volumes of
    test_slab_hostsim.py::test_loopback_slabs_match_oracle are the ones recorded before that rule."""
    import sim
    from medpy_amd import synthetic
    from medpy_amd.slab import LoopbackExchange, solve_slabs
    from oracle import energy_numpy, pipeline
    s = getattr(synthetic, gen)(shape)
    w = energy_numpy.boundary_weights(s["term"], s["image"], s["sigma"])
    g = pipeline.build_graph(s["fg"], s["bg"], weights=w)
    tr = np.array([g.get_trcap(i) for i in range(s["fg"].size)])
    g.maxflow()
    slabs = [sim.SimSlab(shape, r, nslabs) for r in range(nslabs)]
    for sl in slabs:
        sl.load(w, tr)
    st = solve_slabs(slabs, LoopbackExchange(slabs))
    _assert_cut(np.concatenate([sl.finish()[0] for sl in slabs], axis=0), g.labels().reshape(shape).astype(bool), st, "defaults")
    assert (st["exchanges"], st["phases"], st["relabel_passes"], st["outer"]) == counts, st


def test_unknown_or_refused_knobs_raise():
    import sim
    from medpy_amd.slab import LoopbackExchange, solve_slabs
    conn, shape, wsim, _, tr, _ = _volume("sphere32x16x24s1")
    slabs = [sim.SimSlab(shape, r, 2) for r in range(2)]
    for s in slabs:
        s.load(wsim, tr)
    with pytest.raises(TypeError):
        solve_slabs(slabs, LoopbackExchange(slabs), stop_bellow=3)
    with pytest.raises(TypeError):
        sim.SimSlab.solve_group(slabs, None, {"grid_cap": 3})  # a kernel-form knob: the simulator has no such thing
    for knob, value in (("check_rounds", 0), ("relabel_batch", 0), ("exchange_rounds", 0), ("stop_below", -1), ("radial", 3),
                        ("radial_min_c", 0), ("radial_budget_x16", 0), ("max_cycles", 0), ("rounds_per_relabel", -1)):
        with pytest.raises(ValueError, match=knob):
            solve_slabs(slabs, LoopbackExchange(slabs), **{knob: value})
        with pytest.raises(ValueError, match=knob):
            sim.solve(shape, wsim, tr, **{knob: value})
    with pytest.raises(TypeError):
        sim.solve(shape, wsim, tr, exchange_round=2)
    assert len(sim.SCHEDULE_KNOBS) == sim.lib().hostsim_param_count()  # (sim._knob_vector checks it too)


# ---- the single simulator handle --------------------------------------------------------------------------------------------------
SINGLE_KNOBS = [("rounds_per_relabel", 1), ("rounds_per_relabel", 3), ("rounds_per_relabel", 64), ("max_cycles", 1), ("max_cycles", 3),
                ("max_sweeps", 1), ("max_sweeps", 3), ("relabel_batch", 1), ("relabel_batch", 3), ("check_rounds", 1), ("check_rounds", 3),
                ("check_rounds", 5), ("stop_below", 1), ("stop_below", 10 ** 6), ("adaptive_rounds", 0), ("adaptive_rounds", 1),
                ("adaptive_rounds", 100), ("radial_min_c", 1), ("radial_rounds0", 1), ("radial_rounds0", 2), ("radial_budget_x16", 1),
                ("radial_budget_x16", 64)]


def _solve_single(name, **knobs):
    import sim
    conn, shape, wsim, w, tr, ref = _volume(name)
    if conn == 6:
        labels, st = sim.solve(shape, wsim, tr, **knobs)
    else:
        labels, st = sim.solve26(shape, w, tr, **knobs)
    return labels.astype(bool), ref, st


@pytest.mark.parametrize("knob,value", SINGLE_KNOBS, ids=["%s=%d" % kv for kv in SINGLE_KNOBS])
@pytest.mark.parametrize("name", ["sphere32x16x24s1", "hard24"])
def test_single_handle_knob_edges_reach_the_oracle_cut(name, knob, value):
    for incremental, radial in itertools.product((0, 1), (0, 1, 2)):
        labels, ref, st = _solve_single(name, incremental_relabel=incremental, radial=radial, **{knob: value})
        assert st["rc"] == 0, st
        _assert_cut(labels, ref, st, (knob, value, incremental, radial))
        if radial and knob == "radial_min_c" and incremental:
            assert st["radial_cycles"] >= 1, st  # (the flood phase did run: radial_min_c 1 lets every graph in)


N26_KNOBS = SINGLE_KNOBS + [("max_cycles", -1)]


@pytest.mark.parametrize("knob,value", N26_KNOBS, ids=["%s=%d" % kv for kv in N26_KNOBS])
def test_single_handle_knob_edges_full_neighbourhood(knob, value):
    for incremental, radial in itertools.product((0, 1), (0, 1)):
        labels, ref, st = _solve_single("sphere24_n26_regional", incremental_relabel=incremental, radial=radial, **{knob: value})
        assert st["rc"] == 0, st
        _assert_cut(labels, ref, st, (knob, value, incremental, radial))


# ---- the table of the GPU tier ------------------------------------------------------------------------------------------------------
def test_every_set_param_knob_is_in_the_gpu_table():
    """the names of the strcmp chain of mgc_set_param against tests/test_gpu_schedule_knobs.py: a knob cannot land without test values
    there (or a stated reason in its EXCLUDED), and the table names no knob the library does not accept"""
    import re
    import test_gpu_schedule_knobs as T
    from medpy_amd import _lib
    src = open(os.path.join(ROOT, "medpy_amd", "csrc", "mgc_kernels.hip")).read()
    body = src[src.index("int mgc_set_param("):]
    body = body[:body.index("\n}\n")]
    names = set(re.findall(r'strcmp\(name, "([a-z0-9_]+)"\)', body))
    assert len(names) >= 40, sorted(names)
    tabled = set(T.KNOBS) | set(T.GRID_KNOBS)
    missing = sorted(names - tabled - set(T.EXCLUDED))
    assert not missing, "mgc_set_param accepts knobs the GPU tier does not test: %s" % missing
    assert not (tabled - names), "the GPU table names knobs mgc_set_param does not accept: %s" % sorted(tabled - names)
    assert not (tabled & set(T.EXCLUDED))
    assert set(T.REFUSED) - {"no_such_knob"} <= names
    for table in (T.KNOBS, T.GRID_KNOBS):
        for values, scope, along, expect in table.values():
            assert values and set(scope) <= {6, 26} and set(along) <= names and set(expect) <= set(scope)
            assert set(expect.values()) <= set(_lib.LAUNCH_KINDS), expect


def test_launch_kinds_follow_the_header():
    """medpy_amd._lib.LAUNCH_KINDS names the MGC_LAUNCH_* kinds of include/medpy_hip.h, in their order"""
    import re
    from medpy_amd import _lib
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    kinds = dict((int(v), k) for k, v in re.findall(r"\bMGC_LAUNCH_([A-Z0-9_]+) = (\d+)", header))
    assert sorted(kinds) == list(range(len(_lib.LAUNCH_KINDS)))
    assert int(re.search(r"\bMGC_NLAUNCH = (\d+)", header).group(1)) == len(_lib.LAUNCH_KINDS)
    for i, name in enumerate(_lib.LAUNCH_KINDS):
        want = name.upper().replace("K26_DISCHARGE", "DISCHARGE26").replace("K_", "")
        assert kinds[i] == want, (i, kinds[i], name)

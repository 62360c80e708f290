"""CPU tier of ``msg_cut_sets`` / ``msg_cut_sets_tol``: the source side of the smallest minimum cut and the ambiguity set
of a graph on the sparse-graph solver.

* the node operations and the schedule of medpy_amd/csrc/msg_reach_ops.inl, run on the host behind the solve of msg_node_ops.inl by
  tests/hostsim/hostsim_sparse_reach.cpp, on the fifteen graphs of tests/sparse_cases.py against the sets of exact arithmetic
  (two solves of oracle/exact_maxflow.py), and against the rule restated in NumPy on the simulator's own residual graph;
* the same graphs with dust (2**-80) where they have zeros: the rounding tolerance gives the clean graph's sets back, tol 0 does not;
* tests/hostsim/sparse_reach_main.cpp, a stand-alone program: the flood in any order of the nodes against a breadth-first search;
* the refusals the Python layer makes on its own, the names every graph kind has, header / table / build list."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sparse_cases as sc
import sparse_cut_sets_cases as cs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
MAIN = os.path.join(HERE, "hostsim", "sparse_reach_main.cpp")
ULP64 = cs.ULP64


# ---- the oracle itself

@pytest.mark.parametrize("name", sc.SOLVE_NAMES)
def test_exact_sets_have_the_pinned_sizes(name):
    f, t, a = cs.exact_sets(name)
    assert (int(f.sum()), int(t.sum()), int(a.sum())) == cs.SIZES[name]
    assert not (f & t).any() and (f | t | a).all()
    assert np.array_equal(t, ~sc.cut_of(name)[0].astype(bool))


# ---- the simulator against exact arithmetic

@pytest.mark.parametrize("name", sc.INTEGER_CASES)
def test_integer_cases_bit_for_bit(name):
    """whole-number capacities: no sum rounds, so the sets are the exact ones without and with a tolerance, and both cuts ARE the flow"""
    sim, want = cs.host_sim_case(name), cs.exact_sets(name)
    for tol in (None, 0.0, ULP64):
        cs.assert_sets(sim["sets"][tol], want, "%s tol %r" % (name, tol))
        info = sim["info"][tol]
        assert info["source_cut"] == info["sink_cut"] == sim["flow"] == sc.cut_of(name)[1], (name, tol, info, sim["flow"])
        assert (info["from_source"], info["to_sink"], info["ambiguous"]) == cs.SIZES[name]
        assert info["arcs_closed"] == 0 and info["tlinks_closed"] == 0


@pytest.mark.parametrize("name", cs.FLOAT_CASES)
def test_float_cases_exact_at_ulp64(name):
    """float capacities: the device's own preflow residuals, judged at the parity statement's granularity, give the exact sets -- on all
    five (none is held to the invariants alone); the cuts within rel 1e-12 of the exact one, the figure medpy_hip.h gives for the flow"""
    sim, want = cs.host_sim_case(name), cs.exact_sets(name)
    cs.assert_sets(sim["sets"][ULP64], want, "%s tol ULP64" % name)
    info, flow = sim["info"][ULP64], sc.cut_of(name)[1]
    print(name, info, sim["flow"], flow)
    for key in ("source_cut", "sink_cut"):
        assert abs(info[key] - flow) <= 1e-12 * abs(flow), (name, key, info[key], flow)
    assert info["tol"] == ULP64 and info["tol_path"] == 1


@pytest.mark.parametrize("name", sc.SOLVE_NAMES)
def test_invariants_and_the_rule_in_numpy(name):
    sim = cs.host_sim_case(name)
    n = sim["labels"].size
    tr = sc.case(name)[6]
    prev = None
    for tol in cs.TOLS:
        f, t, a = sim["sets"][tol]
        info = sim["info"][tol]
        assert not (f & t).any() and not (f & a).any() and not (t & a).any(), (name, tol)
        assert int(f.sum()) + int(t.sum()) + int(a.sum()) == n and (info["from_source"], info["to_sink"], info["ambiguous"]) == (f.sum(), t.sum(), a.sum())
        rf, rt, ra, arcs_closed, tlinks_closed = cs.rule_sets(n, sim["tail"], sim["head"], sim["rcap"], sim["cap0"], sim["excess"], sim["sink"], tr, tol, sim["labels"])
        cs.assert_sets((f, t, a), (rf, rt, ra), "%s tol %r against the rule in NumPy" % (name, tol))
        assert (info["arcs_closed"], info["tlinks_closed"]) == (arcs_closed, tlinks_closed), (name, tol)
        assert info["forward_seeds"] == int((sim["excess"] > 0).sum() if tol is None else _seeds(sim, tr, tol, "excess").sum()), (name, tol)
        assert info["backward_seeds"] == (0 if tol is None else int(_seeds(sim, tr, tol, "sink").sum())), (name, tol)
        if tol is None:
            assert np.array_equal(t, ~sim["labels"].astype(bool)) and info["tol"] == -1.0 and info["tol_path"] == 0 and info["backward_passes"] == 0
            assert info["sink_cut"] == sim["flow"]
        else:
            assert info["forward_passes"] % 8 == 0 and info["backward_passes"] % 8 == 0 and info["backward_passes"] > 0
        if prev is not None:   # nested as the tolerance rises: a larger threshold opens nothing
            assert not (f & ~prev[0]).any() and not (t & ~prev[1]).any() and not (prev[2] & ~a).any(), (name, tol)
        prev = (f, t, a)
    # None and 0.0: the same sets, one by the labels, one by a backward flood of its own
    cs.assert_sets(sim["sets"][0.0], sim["sets"][None], "%s tol 0.0 against the plain call" % name)


def _seeds(sim, tr, tol, what):
    n = sim["labels"].size
    key = sim["tail"].astype(np.int64) * n + sim["head"]
    rev = np.searchsorted(key, sim["head"].astype(np.int64) * n + sim["tail"])
    scale = np.zeros(n)
    np.maximum.at(scale, sim["tail"], sim["cap0"] + sim["cap0"][rev])
    thr = tol * np.maximum(np.abs(tr), scale) if tol > 0 else np.zeros(n)
    return (sim[what] > 0) & (sim[what] > thr)


# ---- dust

@pytest.mark.parametrize("name", cs.DUSTY_CASES)
def test_dust_decides_nothing_at_ulp64(name):
    """2**-80 where the clean graph has zeros: in exact arithmetic, and at tol 0, the dust decides ties; at ULP64 the sets are the clean
    graph's, arc for arc closed by the threshold"""
    sim, clean = cs.host_sim_dusty(name), cs.exact_sets(name)
    cs.assert_sets(sim["sets"][ULP64], clean, "dusty %s at ULP64 against the clean graph" % name)
    info = sim["info"][ULP64]
    print(name, info)
    assert info["arcs_closed"] > 0 and info["tlinks_closed"] > 0
    assert not all(np.array_equal(g, w) for g, w in zip(sim["sets"][0.0], clean)), "%s: the dust changes nothing at tol 0: the case shows nothing" % name


def test_dust_in_exact_arithmetic():
    """what the generator is for: in exact arithmetic the dust decides ties, so the dusty graphs' OWN ambiguity sets are a small part of
    the clean ones (with this seed: 4 nodes against 298, 148 against 723)"""
    for name in ("one_way_away", "ring_chords_ties"):
        n, i, j, cap, rev, tr, fc = cs.dusty(name)
        f, t, a = cs.exact_sets_of(n, i, j, cap, rev, tr)
        clean = cs.exact_sets(name)[2]
        print(name, int(a.sum()), int(clean.sum()))
        assert 4 * int(a.sum()) < int(clean.sum()), (name, int(a.sum()), int(clean.sum()))


@pytest.mark.parametrize("exponent", [-200, 100])
def test_dusty_ring_at_other_magnitudes(exponent):
    """every weight times a power of two: the rule is relative, the sets stay"""
    g = cs.scaled(cs.dusty("ring_chords_ties"), 2.0 ** exponent)
    sim = cs.run_host_sim(*g, tols=(ULP64,))
    cs.assert_sets(sim["sets"][ULP64], cs.exact_sets("ring_chords_ties"), "dusty ring_chords_ties x 2**%d" % exponent)
    ref = cs.host_sim_dusty("ring_chords_ties")["info"][ULP64]
    assert (sim["info"][ULP64]["arcs_closed"], sim["info"][ULP64]["tlinks_closed"]) == (ref["arcs_closed"], ref["tlinks_closed"])
    assert sim["info"][ULP64]["scale_max"] == ref["scale_max"] * 2.0 ** exponent


@pytest.mark.parametrize("name", ["ring_chords_ties", "one_way_away"])
def test_two_magnitudes_side_by_side(name):
    """two dusty copies in one graph, the second 2**-60 of the first: the rule is local (the scale of a node's own arcs), so the small
    copy is not judged by the large one's numbers and both give their clean sets"""
    d = cs.dusty(name)
    sim = cs.run_host_sim(*cs.side_by_side(d, cs.scaled(d, 2.0 ** -60)), tols=(ULP64,))
    want = tuple(np.concatenate([w, w]) for w in cs.exact_sets(name))
    cs.assert_sets(sim["sets"][ULP64], want, "two dusty %s side by side" % name)


# ---- the flood, stand-alone

def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + flags + ["-o", exe, MAIN])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-400:])
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"(\d+) cases, (\d+) floods of more than one pass, 0 failed", out.stdout)
    assert m and int(m.group(1)) >= 1000 and int(m.group(2)) >= 100


def test_flood_stand_alone(tmp_path):
    """random directed residual graphs, nodes visited ascending, descending and in random permutations to the fixpoint: the marks are
    those of a breadth-first search both ways, the backward flood is the forward flood on the transposed bits (the program has its own
    main and says which case failed)"""
    _build_and_run(tmp_path, "sparse_reach", [])


def test_flood_stand_alone_sanitized(tmp_path):
    flags = _sanitizer_flags(tmp_path)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    _build_and_run(tmp_path, "sparse_reach_san", flags)


# ---- the Python layer without a library

def _hostless(cls, n=4):
    from medpy_amd.graphcut import graph
    g = object.__new__(cls)
    g._h, g._nodes = None, n
    g._pending = ([], [], [], [])
    g._host_arcs, g._host_sent = {}, {}
    g._tr, g._sent_tr = None, None
    g._flow_const, g._sent_flow_const = 0.0, None
    g._dev_solved, g._dev_updated = True, False
    g._labels = None
    calls = []
    g._call = lambda name, *a: calls.append(name)
    return g, calls, graph


@pytest.mark.parametrize("kind", ["SparseGraph", "RegionGraph", "GraphFloat", "GraphInt"])
def test_python_layer_refuses_what_maxflow_has_not_seen(kind):
    from medpy_amd import _lib
    from medpy_amd.graphcut import graph

    def pending(g):
        g._pending[0].append(0)

    def host_arcs(g):
        g._host_arcs = {(0, 1): [2.0, 0.0], (1, 0): [1.0, 0.0]}

    def host_arcs_grown(g):
        g._host_arcs = {(0, 1): [2.0, 1.0], (1, 0): [1.0, 0.0]}
        g._host_sent = {(0, 1): (2.0, 1.0)}

    def tr_never_sent(g):
        g._tr = np.zeros(4)

    def tr_differs(g):
        g._tr, g._sent_tr = np.array([0.0, 1.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0, -2.0])

    def dev_updated(g):
        g._tr = g._sent_tr = np.zeros(4)
        g._dev_updated = True

    for edit in (pending, host_arcs, host_arcs_grown, tr_never_sent, tr_differs, dev_updated):
        for method in ("cut_sets", "cut_sets_unique"):
            for kw in ({}, {"tol": ULP64}):
                g, calls, _ = _hostless(getattr(graph, kind))
                edit(g)
                with pytest.raises(_lib.MedpyHipError) as e:
                    getattr(g, method)(**kw)
                assert e.value.code == _lib.ERR_STATE and calls == [], (edit.__name__, method, calls)
                assert g._pending[0] == ([0] if edit is pending else []), "the refusal flushed the pending edges"
    # nothing held back: the call goes to the library (here: a recorder), the host arcs that WERE sent do not count
    g, calls, _ = _hostless(getattr(graph, kind))
    g._host_arcs, g._host_sent = {(0, 1): [2.0, 1.0], (1, 0): [1.0, 0.0]}, {(0, 1): (3.0, 1.0)}
    g._tr = g._sent_tr = np.array([1.0, 0.0, 0.0, -1.0])
    assert g.cut_sets_unique(ULP64) is True and calls == ["msg_cut_sets_tol", "msg_get_cut_sets_info"]   # (the recorder writes nothing: 0 ambiguous)
    assert g.cut_sets_unique(ULP64) is True and len(calls) == 2   # cached
    g._labels = None   # what every edit does
    assert g.cut_sets_unique(ULP64) is True and len(calls) == 4
    assert g.cut_sets_unique() is True and calls[4:] == ["msg_cut_sets", "msg_get_cut_sets_info"]


def test_cut_sets_is_one_call_and_cached():
    from medpy_amd.graphcut import graph
    g, calls, _ = _hostless(graph.SparseGraph)
    g._labels = np.array([True, False, True, False])
    got = g.cut_sets(ULP64)
    assert isinstance(got, graph.CutSets) and got._fields == ("from_source", "to_sink", "ambiguous", "info")
    assert calls == ["msg_cut_sets_tol", "msg_get_cut_sets_info"]
    assert all(a.shape == (4,) and a.dtype == np.bool_ for a in got[:3])
    assert got.info["tol"] == 0.0 and got.info["tol_path"] is False and set(graph.SparseGraph.CUT_SETS_INFO_KEYS) <= set(got.info)
    assert g.cut_sets(ULP64) is got and g.cut_sets_unique(ULP64) is True and len(calls) == 2   # the counts of the same call
    plain = g.cut_sets()
    assert calls[2:] == ["msg_cut_sets", "msg_get_cut_sets_info"] and plain.info["tol"] is None
    assert plain.to_sink.tolist() == [False, True, False, True]   # ~labels(): no plane of its own comes down


def test_the_pinned_methods_still_refuse_and_name_the_new_call():
    from medpy_amd.graphcut import graph
    for cls in (graph.SparseGraph, graph.RegionGraph, graph.GraphFloat, graph.GraphInt):
        g = object.__new__(cls)
        for name in ("source_side", "sink_side", "ambiguous", "cut_is_unique", "cut_sets_info"):
            with pytest.raises(NotImplementedError, match="sparse-graph solver") as e:
                getattr(cls, name)(g)
            assert "cut_sets()" in str(e.value)
        assert callable(cls.cut_sets) and callable(cls.cut_sets_unique)


def test_voxel_kinds_compose_the_same_name():
    """VoxelGraph / EmbeddedLatticeGraph: cut_sets() is their four existing calls, no call of its own"""
    from medpy_amd.graphcut import CutSets, graph
    v = object.__new__(graph.VoxelGraph)
    v._shape, v._nodes = (2, 3), 6
    planes = {"source_side": np.array([[1, 0, 0], [0, 0, 0]], bool), "sink_side": np.array([[0, 0, 0], [0, 0, 1]], bool),
              "ambiguous": np.array([[0, 1, 1], [1, 1, 0]], bool), "info": {"ambiguous": 4}}
    v.__dict__["_cut_sets_cache"] = {("tol", ULP64): planes}
    got = v.cut_sets(ULP64)
    assert isinstance(got, CutSets) and got.from_source is planes["source_side"] and got.to_sink is planes["sink_side"] and got.ambiguous is planes["ambiguous"]
    assert got.info == {"ambiguous": 4} and v.cut_sets_unique(ULP64) is False
    e = object.__new__(graph.EmbeddedLatticeGraph)
    e._inner, e._n, e._nodes = v, 6, 8
    e._tail_tr = np.array([65535.0, 0.0])
    got = e.cut_sets(ULP64)
    assert got.from_source.tolist() == [True, False, False, False, False, False, True, False]
    assert got.to_sink.tolist() == [False] * 5 + [True, False, False] and got.ambiguous.tolist() == [False, True, True, True, True, False, False, True]
    assert e.cut_sets_unique(ULP64) is False


def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    want = {"msg_cut_sets": r"int msg_cut_sets\(msg_handle h, uint8_t\* from_source, uint8_t\* ambiguous\);",
            "msg_cut_sets_tol": r"int msg_cut_sets_tol\(msg_handle h, double tol, uint8_t\* from_source, uint8_t\* to_sink, uint8_t\* ambiguous\);",
            "msg_get_cut_sets_info": r"int msg_get_cut_sets_info\(msg_handle h, int64_t\* out16, double\* out4\);"}
    for name, decl in want.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    assert "msg_reach_ops.inl" in build.DEPS

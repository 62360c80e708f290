"""CPU tier of the cut sets at a rounding tolerance (mgc_cut_sets_tol): the scale and open steps of
mgc_reach_tol_ops.inl and both directions of the tile step of mgc_reach_ops.inl as a stand-alone host program against a per-voxel restatement and a voxel BFS; the pin that makes the GPU tier's
expectations legitimate -- the device's RULE, restated in NumPy over BK's residual graph of the dusty graph, gives at 64 ulp the tol-0 sets
of the clean graph, for every case and seed the GPU tier uses; header, symbol table and library agree on the two new calls; the Python
surface that needs no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cut_sets_tol_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAIN = os.path.join(HERE, "hostsim", "reach_tol_main.cpp")


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
    assert re.search(r"\d+ cases, \d+ forward and \d+ backward floods of more than one pass, \d+ arcs closed by the threshold, 0 failed", out.stdout)


def test_steps_stand_alone(tmp_path):
    """directed residuals with dust, garbage on padding voxels and on directions that leave the volume, partial tiles, tiles in random
    order, 6 and 26 directions: scales and thresholded masks equal the per-voxel restatement, both closures equal a voxel BFS"""
    _build_and_run(tmp_path, "reach_tol", [])


def test_steps_stand_alone_sanitized(tmp_path):
    flags = _sanitizer_flags(tmp_path)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    _build_and_run(tmp_path, "reach_tol_san", flags)


@pytest.mark.parametrize("case", range(len(cases.CASES)), ids=cases.CASE_IDS)
def test_rule_on_the_dusty_graph_gives_the_clean_sets(case):
    """The pin.  BK solves the dusty graph; the device's rule over that residual graph at 64 ulp must give, bit for bit, what
    cutcheck.ambiguity gives on the clean graph at tol 0 -- and at tol 0 the dusty graph's own sets, which differ (the dust decides every
    tie).  Also with every weight x 2^-200 and x 2^100: the rule is relative."""
    shape = cases.CASES[case][0]
    for seed in cases.seeds_of(case):
        gr = cases.graphs(case, seed)
        _, fs, ts, amb = cases.clean_sets(case, seed)
        assert amb.any()
        for factor in (1.0, 2.0 ** -200, 2.0 ** 100):
            nw, source, sink = cases.scaled(gr["dusty"], factor)
            g, _ = cases.bk_solve(shape, nw, source, sink)
            got = [a.reshape(shape) for a in cases.device_rule(g, source - sink, cases.ULP64)]
            print(cases.CASE_IDS[case], "seed", seed, "x", factor, "clean", int(fs.sum()), int(ts.sum()), int(amb.sum()), "rule on dusty at 64 ulp", [int(a.sum()) for a in got])
            np.testing.assert_array_equal(got[0], fs)
            np.testing.assert_array_equal(got[1], ts)
            np.testing.assert_array_equal(got[2], amb)
            if factor == 1.0:
                at0 = cases.device_rule(g, source - sink, 0.0)
                ref0 = cutcheck_sets(g)
                for a, b in zip(at0, ref0):                      # at tol 0 the restatement is cutcheck's BFS
                    np.testing.assert_array_equal(a, b)
                if len(shape) > 1:                               # the dust did decide ties: tol 0 is not the answer here
                    assert int(at0[2].sum()) < int(amb.sum())    # (a 1-D wall is one arc: nothing to tie with)


def cutcheck_sets(g):
    from oracle import cutcheck
    return cutcheck.ambiguity(g, tol=0.0)


def test_side_by_side_needs_a_local_scale():
    """two graphs side by side, the second x 2^-60: the rule with per-voxel scales gives BK's tol-0 sets of the clean whole; one global
    scale (cutcheck.py's t-link rule, applied to arcs as well) closes every arc of the small half"""
    case, seed = 3, cases.seeds_of(3)[0]
    shape = cases.CASES[case][0]
    gr = cases.graphs(case, seed)
    big, nw, source, sink = cases.side_by_side(shape, gr["dusty"], cases.scaled(gr["dusty"], 2.0 ** -60))
    _, fs, ts, amb = cases.bk_tol0(("side", case, seed), *cases.side_by_side(shape, gr["clean"], cases.scaled(gr["clean"], 2.0 ** -60)))
    g, _ = cases.bk_solve(big, nw, source, sink)
    got = [a.reshape(big) for a in cases.device_rule(g, source - sink, cases.ULP64)]
    for a, b in zip(got, (fs, ts, amb)):
        np.testing.assert_array_equal(a, b)
    assert fs[shape[0]:].any() and ts[shape[0]:].any() and amb[shape[0]:].any()
    tail, head, rcap, _ = g.export()
    small = (tail >= int(np.prod(shape))) & (rcap > 0)
    assert small.any() and not (rcap[small] > cases.ULP64 * (rcap + rcap[np.arange(rcap.size) ^ 1]).max()).any()


def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    want = {"mgc_cut_sets_tol": r"int mgc_cut_sets_tol\(mgc_handle h, double tol, uint8_t\* from_source, uint8_t\* to_sink, uint8_t\* ambiguous\);",
            "mgc_get_cut_sets_tol_info": r"int mgc_get_cut_sets_tol_info\(mgc_handle h, int64_t\* out16, double\* out4\);"}
    for name, decl in want.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    assert _lib.SIGNATURES["mgc_cut_sets_tol"][1][1] is ctypes.c_double
    for d in ("mgc_reach_ops.inl", "mgc_reach_tol_ops.inl", "mgc_reach_tol.h", "mgc_reach_driver.inl"):
        assert d in build.DEPS and os.path.exists(os.path.join(build.CSRC, d)), d
    # the rule is stated once, in the header that host code compiles; the steps are what the host program compiles
    rule = open(os.path.join(build.CSRC, "mgc_reach_tol.h")).read()
    assert "mgc_tol_arc_open" in rule and "mgc_tol_tlink_open" in rule and "__global__" not in rule and "hip_runtime" not in rule
    text = open(os.path.join(build.CSRC, "mgc_reach_tol_ops.inl")).read()
    host_part = text[:text.index("#if defined(__HIPCC__)")]
    assert "mgc_reach_open_tile" in host_part and "__global__" not in host_part and "hip_runtime" not in text
    # one tile step and one flood kernel serve both directions; they live in mgc_reach_ops.inl, the back forms are gone
    step = open(os.path.join(build.CSRC, "mgc_reach_ops.inl")).read()
    step_host = step[:step.index("#if defined(__HIPCC__)")]
    assert "template <int NDIR, bool BACK = false, class Mask, class Sync>" in step_host and "__global__" not in step_host and "hip_runtime" not in step
    assert step.count("uint32_t mgc_reach_tile_step(") == 1 and step.count("void k_reach_flood(") == 1
    for gone in ("mgc_reach_tile_step_back", "k_reach_flood_back"):
        assert gone not in step and gone not in text, gone
    # the backward path consults neither labels nor summaries: the code of the step and of the flood kernel (header comment apart),
    # the host part of the tol file, the backward seeding's arguments
    back = step_host[step_host.index("MGC_HD bool mgc_reach_pull("):] + step[step.index("void k_reach_flood("):step.index("void k_reach_readout(")] + host_part
    assert "height" not in back and "tsum" not in back and "d_labels" not in back
    # ... and one include behind the last function of the kernel file, the first of the drivers there, brings the reach code in: nothing
    # of the solve moved in the code object
    import driver_chain
    driver_chain.assert_behind_everything_before_it("mgc_reach_driver.inl", "mgc_reach")
    kernels = open(os.path.join(build.CSRC, "mgc_kernels.hip")).read()
    assert "mgc_reach" not in kernels.replace('#include "mgc_reach_driver.inl"', "")
    driver = open(os.path.join(build.CSRC, "mgc_reach_driver.inl")).read()
    assert driver.count('#include "mgc_reach_ops.inl"') == 1 and driver.count('#include "mgc_reach_tol_ops.inl"') == 1


class _Recorder(object):
    """stands in for the library: records the calls of a VoxelGraph that owns no handle"""

    def __init__(self, n):
        self.calls = []
        self.tols = []
        self.n = n

    def __call__(self, name, *args):
        self.calls.append(name)
        if name == "mgc_get_cut_sets_info":
            out = np.frombuffer((ctypes.c_int64 * 8).from_address(args[0].value), dtype=np.int64)
            out[:] = [3, 4, self.n - 7, 2, 5, 1, 6, 0]
            args[1]._obj.value = 12.5
        if name == "mgc_cut_sets_tol":
            self.tols.append(args[0])
        if name == "mgc_get_cut_sets_tol_info":
            out = np.frombuffer((ctypes.c_int64 * 16).from_address(args[0].value), dtype=np.int64)
            out[:] = [3, 4, self.n - 7, 2, 5, 1, 7, 8, 9, 10, 11, 6, 0, 0, 0, 0]
            vals = np.frombuffer((ctypes.c_double * 4).from_address(args[1].value), dtype=np.float64)
            vals[:] = [self.tols[-1], 12.5, 12.75, 8.0]


def _voxel_graph(shape):
    from medpy_amd.graphcut import graph
    g = object.__new__(graph.VoxelGraph)
    g._h = None
    g._shape = shape
    g._nodes = int(np.prod(shape))
    g._labels = None
    rec = _Recorder(g._nodes)
    g._call = rec
    return g, rec


def test_tol_none_is_todays_path_and_a_number_the_new_one():
    from medpy_amd import graphcut
    from medpy_amd.graphcut import graph
    assert graph.ULP64 == 64 * 2.0 ** -52 == graphcut.ULP64
    g, rec = _voxel_graph((3, 4, 5))
    assert g.cut_is_unique(tol=None) is False
    assert rec.calls == ["mgc_cut_sets", "mgc_get_cut_sets_info"]
    assert g.cut_sets_info() == {"from_source": 3, "to_sink": 4, "ambiguous": 53, "flood_passes": 2, "tile_visits": 5, "tiles_seeded": 1,
                                 "tiles_skipped": 6, "source_cut": 12.5}
    assert len(rec.calls) == 2
    # a number: the new pair, once per tol and kind of answer
    assert g.cut_is_unique(graph.ULP64) is False
    assert rec.calls[2:] == ["mgc_cut_sets_tol", "mgc_get_cut_sets_tol_info"] and rec.tols == [graph.ULP64]
    info = g.cut_sets_info(tol=graph.ULP64)
    assert len(rec.calls) == 4                        # the counts came with the first call
    assert info == {"from_source": 3, "to_sink": 4, "ambiguous": 53, "forward_passes": 2, "forward_visits": 5, "forward_seeded": 1,
                    "backward_passes": 7, "backward_visits": 8, "backward_seeded": 9, "arcs_closed": 10, "tlinks_closed": 11, "tiles_skipped": 6,
                    "tol": graph.ULP64, "source_cut": 12.5, "sink_cut": 12.75, "scale_max": 8.0}
    a = g.source_side(graph.ULP64)
    assert a.shape == (3, 4, 5) and a.dtype == np.bool_ and g.source_side(tol=graph.ULP64) is a and len(rec.calls) == 6
    b = g.sink_side(graph.ULP64)
    assert b.shape == (3, 4, 5) and b.dtype == np.bool_ and g.sink_side(graph.ULP64) is b and len(rec.calls) == 8
    c = g.ambiguous(graph.ULP64)
    assert c.dtype == np.bool_ and g.ambiguous(graph.ULP64) is c and len(rec.calls) == 10
    # another tol: its own calls, its own cache; 0.0 is a number, not None
    assert g.cut_sets_info(0.0)["tol"] == 0.0 and rec.calls[10:] == ["mgc_cut_sets_tol", "mgc_get_cut_sets_tol_info"] and rec.tols[-1] == 0.0
    assert g.cut_sets_info(graph.ULP64)["tol"] == graph.ULP64 and len(rec.calls) == 12
    assert g.source_side(graph.ULP64) is a and g.cut_sets_info() == {"from_source": 3, "to_sink": 4, "ambiguous": 53, "flood_passes": 2, "tile_visits": 5,
                                                                     "tiles_seeded": 1, "tiles_skipped": 6, "source_cut": 12.5}
    assert len(rec.calls) == 12
    g._labels = np.zeros((3, 4, 5), bool)             # reading the labels keeps the sets; sink_side() without a tol is their complement
    assert g.source_side(graph.ULP64) is a and g.sink_side().all() and len(rec.calls) == 12
    g._labels = None                                  # what every build, update and edit does drops them, for every tol
    assert g.source_side(graph.ULP64) is not a and len(rec.calls) == 14
    assert g.cut_is_unique(0.0) is False and len(rec.calls) == 16


def test_other_graph_kinds():
    from medpy_amd.graphcut import graph
    for cls in (graph.SparseGraph, graph.RegionGraph, graph.GraphFloat, graph.GraphInt):
        g = object.__new__(cls)
        for name in ("source_side", "sink_side", "ambiguous", "cut_is_unique", "cut_sets_info"):
            for kw in ({}, {"tol": None}, {"tol": graph.ULP64}):
                with pytest.raises(NotImplementedError, match="sparse-graph solver"):
                    getattr(cls, name)(g, **kw)
    # a lattice with isolated nodes behind it forwards the tol; an isolated node is on the side its t-link points to, ambiguous at 0
    inner, rec = _voxel_graph((2, 3))
    tol = graph.ULP64
    inner.__dict__["_cut_sets_cache"] = {("tol", tol): {"source_side": np.array([[1, 0, 0], [0, 0, 0]], bool), "sink_side": np.array([[0, 0, 0], [0, 0, 1]], bool),
                                                        "ambiguous": np.array([[0, 1, 1], [1, 1, 0]], bool), "info": {"ambiguous": 4}}}
    e = object.__new__(graph.EmbeddedLatticeGraph)
    e._inner, e._n, e._nodes = inner, 6, 9
    e._tail_tr = np.array([65535.0, -65535.0, 0.0])
    assert e.source_side(tol).tolist() == [True, False, False, False, False, False, True, False, False]
    assert e.sink_side(tol).tolist() == [False, False, False, False, False, True, False, True, False]
    assert e.ambiguous(tol=tol).tolist() == [False, True, True, True, True, False, False, False, True]
    assert e.cut_is_unique(tol) is False and e.cut_sets_info(tol) == {"ambiguous": 4} and rec.calls == []

"""CPU tier of the source-side cut and the ambiguity set: the tile step of mgc_reach_ops.inl as a stand-alone host
program against a plain voxel BFS, the agreement of header, symbol table and library on the two new calls, and the Python surface
that needs no device (result cache, the graph kinds that refuse)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAIN = os.path.join(HERE, "hostsim", "reach_main.cpp")


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
    assert re.search(r"\d+ cases, \d+ floods of more than one pass, 0 failed", out.stdout)


def test_flood_stand_alone(tmp_path):
    """randomly masked lattices, 6 and 26 directions, partial tiles, tiles visited in random order to a fixpoint: the marks are those
    of a voxel BFS, no padding voxel is ever marked (the program has its own main and says which case failed)"""
    _build_and_run(tmp_path, "reach", [])


def test_flood_stand_alone_sanitized(tmp_path):
    flags = _sanitizer_flags(tmp_path)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    _build_and_run(tmp_path, "reach_san", flags)


def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    want = {"mgc_cut_sets": r"int mgc_cut_sets\(mgc_handle h, uint8_t\* from_source, uint8_t\* ambiguous\);",
            "mgc_get_cut_sets_info": r"int mgc_get_cut_sets_info\(mgc_handle h, int64_t\* out8, double\* source_cut\);"}
    for name, decl in want.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    assert "mgc_reach_ops.inl" in build.DEPS
    for d in build.DEPS:
        assert os.path.exists(os.path.join(build.CSRC, d)), d
    # the tile step is what the host program compiles: nothing of the HIP runtime outside the device-only part of the file
    text = open(os.path.join(build.CSRC, "mgc_reach_ops.inl")).read()
    host_part = text[:text.index("#if defined(__HIPCC__)")]
    assert "mgc_reach_tile_step" in host_part and "__global__" not in host_part and "hip_runtime" not in text


class _Recorder(object):
    """stands in for the library: counts the calls of a VoxelGraph that owns no handle"""

    def __init__(self, n):
        self.calls = []
        self.n = n

    def __call__(self, name, *args):
        self.calls.append(name)
        if name == "mgc_get_cut_sets_info":
            out = np.frombuffer((ctypes.c_int64 * 8).from_address(args[0].value), dtype=np.int64)
            out[:] = [3, 4, self.n - 7, 2, 5, 1, 6, 0]
            args[1]._obj.value = 12.5


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


def test_results_are_cached_until_the_next_edit():
    g, rec = _voxel_graph((3, 4, 5))
    assert g.cut_is_unique() is False
    assert rec.calls == ["mgc_cut_sets", "mgc_get_cut_sets_info"]
    info = g.cut_sets_info()
    assert info == {"from_source": 3, "to_sink": 4, "ambiguous": 53, "flood_passes": 2, "tile_visits": 5, "tiles_seeded": 1,
                    "tiles_skipped": 6, "source_cut": 12.5}
    assert len(rec.calls) == 2                        # the counts came with the first call
    a = g.source_side()
    assert a.shape == (3, 4, 5) and a.dtype == np.bool_ and g.source_side() is a and len(rec.calls) == 4
    b = g.ambiguous()
    assert b.shape == (3, 4, 5) and b.dtype == np.bool_ and g.ambiguous() is b and len(rec.calls) == 6
    g._labels = np.zeros((3, 4, 5), bool)             # reading the labels keeps the sets ...
    assert g.source_side() is a and len(rec.calls) == 6
    g._labels = None                                  # ... what every build, update and edit does drops them
    assert g.source_side() is not a and len(rec.calls) == 8


def test_other_graph_kinds():
    from medpy_amd.graphcut import graph
    for cls in (graph.SparseGraph, graph.RegionGraph, graph.GraphFloat, graph.GraphInt):
        g = object.__new__(cls)
        for name in ("source_side", "ambiguous", "cut_is_unique", "cut_sets_info"):
            with pytest.raises(NotImplementedError, match="sparse-graph solver"):
                getattr(cls, name)(g)
    # a lattice with isolated nodes behind it forwards to its voxel graph; an isolated node follows the sign of its t-link
    inner, _ = _voxel_graph((2, 3))
    inner.__dict__["_cut_sets_cache"] = {"source_side": np.array([[1, 0, 0], [0, 0, 0]], bool), "ambiguous": np.array([[0, 1, 0], [0, 0, 0]], bool),
                                         "info": {"ambiguous": 1}}
    e = object.__new__(graph.EmbeddedLatticeGraph)
    e._inner, e._n, e._nodes = inner, 6, 9
    e._tail_tr = np.array([65535.0, -65535.0, 0.0])
    assert e.source_side().tolist() == [True, False, False, False, False, False, True, False, False]
    assert e.ambiguous().tolist() == [False, True, False, False, False, False, False, False, True]
    assert e.cut_is_unique() is False and e.cut_sets_info() == {"ambiguous": 1}

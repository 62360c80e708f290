"""CPU tier of the edits of n-links by arc list ("Edits of n-links by list"): the directed per-arc rule of
mgc_nlink_fold.h and the host preparation of mgc_nlink_edit.h run as a stand-alone host program, the pure argument normalisation
of VoxelGraph.edit_nweights, and the agreement of header, symbol table and library on the three new calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


def test_directed_rule_and_host_preparation_stand_alone(tmp_path):
    """The rule: unchanged capacities touch nothing; 0 <= r' <= c_out' + c_in'; a flow inside the new bounds gives back exactly 0;
    symmetric inputs give mgc_nlink_fold bit for bit; on dyadic inputs the two ends hand back opposite amounts and
    r'_ab + r'_ba == c'_ab + c'_ba.  The preparation, on (17, 9, 10) / 6, (9, 10, 11) / 26, (9, 10) / 4 and 8, (1, 1, 17): every
    refusal with the entry it names, direction indices against the encoding of mgc_add_nweights, two tiles for a pair across a
    face / edge / corner, the arcs of one voxel adjacent, tile ranges that cover the half-arcs once.  The program has its own
    main, runs the cases and says which failed."""
    exe = str(tmp_path / "nlink_edit")
    flags = _sanitizer_flags(tmp_path)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + flags + ["-o", exe, os.path.join(HERE, "hostsim", "nlink_edit_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def _normalise(*args):
    from medpy_amd.graphcut.graph import normalise_nweight_edit
    return normalise_nweight_edit(*args)


def test_normalisation_broadcasts_and_converts():
    i, j, cap, rev = _normalise(3, 4, 2)
    assert (i.tolist(), j.tolist(), cap.tolist(), rev) == ([3], [4], [2.0], None)
    assert i.dtype == np.int64 and j.dtype == np.int64 and cap.dtype == np.float64
    i, j, cap, rev = _normalise(np.arange(5, dtype=np.int32), np.arange(1, 6, dtype=np.uint16), 0.0, np.float32(1.5))
    assert i.tolist() == [0, 1, 2, 3, 4] and j.tolist() == [1, 2, 3, 4, 5] and cap.tolist() == [0.0] * 5 and rev.tolist() == [1.5] * 5
    for a in (i, j, cap, rev):
        assert a.flags.c_contiguous and a.flags.writeable is not None and a.ndim == 1
        assert a.dtype in (np.int64, np.float64)
    # strided and non-native inputs come out C-contiguous in the library's dtypes
    ids = np.arange(12, dtype=np.int64)[::2]
    w = np.linspace(0, 1, 12, dtype=np.float32)[::2]
    i, j, cap, rev = _normalise(ids, ids + 1, w, w[::-1])
    assert i.flags.c_contiguous and cap.flags.c_contiguous and rev.flags.c_contiguous
    assert cap.tolist() == w.astype(np.float64).tolist() and rev.tolist() == w[::-1].astype(np.float64).tolist()
    # lists, and a scalar node against an array of nodes (a star around one voxel)
    i, j, cap, rev = _normalise(7, [6, 8, 17], [1, 2, 3])
    assert i.tolist() == [7, 7, 7] and j.tolist() == [6, 8, 17] and cap.tolist() == [1.0, 2.0, 3.0] and rev is None
    # empty lists stay empty
    i, j, cap, rev = _normalise(np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0))
    assert i.size == j.size == cap.size == 0 and rev is None


def test_normalisation_refuses():
    with pytest.raises(ValueError):
        _normalise([0, 1], [1, 2, 3], 1.0)            # different lengths
    with pytest.raises(ValueError):
        _normalise([0, 1], [1, 2], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        _normalise([0.0, 1.0], [1, 2], 1.0)            # ids that are not whole numbers
    with pytest.raises(ValueError):
        _normalise([[0, 1]], [[1, 2]], 1.0)            # more than one axis
    with pytest.raises(ValueError):
        _normalise([0], [1], ["a"])                    # weights that are not numbers
    with pytest.raises(ValueError):
        _normalise([0, 1], [1, 2], 1.0, [1.0, 2.0, 3.0])


def test_other_graph_kinds_refuse():
    from medpy_amd.graphcut import graph
    for cls in (graph.SparseGraph, graph.RegionGraph, graph.EmbeddedLatticeGraph):
        g = object.__new__(cls)
        with pytest.raises(NotImplementedError):
            cls.edit_nweights(g, 0, 1, 1.0)
        with pytest.raises(NotImplementedError):
            cls.clear_nweight_edits(g)
        with pytest.raises(NotImplementedError):
            cls.nweight_edit_info(g)


def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    want = {"mgc_edit_nweights": r"int mgc_edit_nweights\(mgc_handle h, int64_t n, const int64_t\* i, const int64_t\* j, const double\* cap, const double\* rev\);",
            "mgc_clear_nweight_edits": r"int mgc_clear_nweight_edits\(mgc_handle h\);",
            "mgc_get_nweight_edit_info": r"int mgc_get_nweight_edit_info\(mgc_handle h, int64_t\* out4\);"}
    for name, decl in want.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    assert _lib.SIGNATURES["mgc_edit_nweights"] == _lib.SIGNATURES["mgc_add_edges"]   # "takes its argument list from mgc_add_edges"
    deps = build.DEPS
    assert "mgc_nlink_edit_ops.inl" in deps and "mgc_nlink_edit.h" in deps and "mgc_nlink_fold.h" in deps
    for d in deps:
        assert os.path.exists(os.path.join(build.CSRC, d)), d
    # the host preparation stays plain C++: a stand-alone program includes it
    text = open(os.path.join(build.CSRC, "mgc_nlink_edit.h")).read()
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text

"""CPU tier of the warm update of the boundary term ("The boundary term"): the per-arc rule of mgc_nlink_fold.h run
as a stand-alone host program, the pure argument normalisation of VoxelGraph.update_boundary_term, and the agreement of header,
symbol table and library on the three new calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_fold_rule_stand_alone(tmp_path):
    """unchanged capacity -> nothing touched; 0 <= r' <= 2c'; a flow inside the new bounds gives back exactly 0; on dyadic inputs
    the two ends of a pair hand back opposite amounts and r'_ab + r'_ba == 2c': the program runs the cases and says which failed"""
    exe = str(tmp_path / "nlink_fold")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", exe, os.path.join(HERE, "hostsim", "nlink_fold_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def _normalise(shape, facts, term, args):
    from medpy_amd.graphcut.graph import normalise_boundary_update
    return normalise_boundary_update(shape, facts, term, args)


def test_kept_image_sends_nothing_but_the_arguments():
    from medpy_amd.graphcut import energy_voxel as ev
    from medpy_amd.graphcut.graph import FACTS_UNKNOWN
    u = _normalise((4, 5, 6), (False, 0.0, 0.0), ev.boundary_difference_exponential, (None, 10.0, False))
    assert u["term"] == "difference_exponential" and u["image"] is None and u["sigma"] == 10.0
    assert u["spacing"] is None and u["table"] is None and u["facts"] == (False, 0.0, 0.0)
    u = _normalise((4, 5, 6), FACTS_UNKNOWN, ev.boundary_difference_division, (None, 3.0, (2, 1, 0.5)))
    assert u["term"] == "difference_division" and u["image"] is None and u["spacing"] == (2, 1, 0.5) and u["table"] is None
    assert u["facts"] == FACTS_UNKNOWN   # (what the graph knows of its image does not change)
    u = _normalise((4, 5, 6), FACTS_UNKNOWN, ev.boundary_difference_linear, (None, False))
    assert u["term"] == "difference_linear" and u["sigma"] is None and u["image"] is None


def test_table_decision():
    """by table exactly where graph_from_voxels of the same arguments goes by table: exponential / power terms on whole numbers"""
    from medpy_amd.graphcut import energy_voxel as ev
    from medpy_amd.graphcut.graph import FACTS_UNKNOWN, boundary_table
    rng = np.random.default_rng(5)
    ct = rng.integers(0, 900, (4, 5, 6)).astype(np.uint16)
    noise = rng.random((4, 5, 6)).astype(np.float32)
    # a kept image: from the facts remembered at build time
    held = (True, float(ct.min()), float(ct.max()))
    u = _normalise(ct.shape, held, ev.boundary_difference_exponential, (None, 50.0, False))
    assert u["table"] is not None and u["table"].tobytes() == boundary_table("difference_exponential", ct, 50.0).tobytes()
    u = _normalise(ct.shape, held, ev.boundary_maximum_power, (None, 2.0, False))
    assert u["table"].tobytes() == boundary_table("maximum_power", ct, 2.0).tobytes()
    assert _normalise(ct.shape, held, ev.boundary_difference_division, (None, 50.0, False))["table"] is None
    assert _normalise(ct.shape, (False, 0.0, 0.0), ev.boundary_difference_exponential, (None, 50.0, False))["table"] is None
    assert _normalise(ct.shape, None, ev.boundary_difference_exponential, (None, 50.0, False))["table"] is None
    # a new image: from the image
    u = _normalise(ct.shape, (False, 0.0, 0.0), ev.boundary_difference_exponential, (ct, 25.0, False))
    assert u["image"].dtype == np.uint16 and u["image"].flags.c_contiguous and u["facts"] == held
    assert u["table"].tobytes() == boundary_table("difference_exponential", ct, 25.0).tobytes()
    u = _normalise(ct.shape, held, ev.boundary_difference_exponential, (noise, 25.0, False))
    assert u["table"] is None and u["facts"] == (False, 0.0, 0.0)
    u = _normalise(ct.shape, held, ev.boundary_difference_division, (ct, 25.0, False))
    assert u["table"] is None and u["facts"] == FACTS_UNKNOWN   # (nobody looked at the new image)
    # dtypes the library does not take go up as graph_from_voxels sends them
    assert _normalise(ct.shape, held, ev.boundary_difference_division, (ct.astype(np.float16), 25.0, False))["image"].dtype == np.float32
    assert _normalise(ct.shape, held, ev.boundary_difference_division, (ct > 400, 25.0, False))["image"].dtype == np.uint8


def test_refused_forms():
    from medpy_amd.graphcut import energy_voxel as ev
    from medpy_amd.graphcut.graph import FACTS_UNKNOWN
    img = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(NotImplementedError):
        _normalise(img.shape, FACTS_UNKNOWN, ev.boundary_precomputed, ([img, img, img],))
    with pytest.raises(NotImplementedError):
        _normalise(img.shape, FACTS_UNKNOWN, ev.boundary_difference_exponential, (img[1:], 5.0, False))
    with pytest.raises(NotImplementedError):
        _normalise(img.shape, FACTS_UNKNOWN, ev.boundary_difference_exponential, (img.reshape(4, 30), 5.0, False))
    # an exponential term on a kept image nobody ever looked at: the table decision cannot be made
    with pytest.raises(NotImplementedError):
        _normalise(img.shape, FACTS_UNKNOWN, ev.boundary_difference_exponential, (None, 5.0, False))
    with pytest.raises(ValueError):
        _normalise(img.shape, FACTS_UNKNOWN, lambda graph, args: None, (img, 5.0, False))
    with pytest.raises(NotImplementedError):   # two terms in one call
        def twice(graph, args):
            ev.boundary_difference_exponential(graph, args)
            ev.boundary_difference_exponential(graph, args)
        _normalise(img.shape, FACTS_UNKNOWN, twice, (img, 5.0, False))
    with pytest.raises(NotImplementedError):   # edges set one by one
        _normalise(img.shape, FACTS_UNKNOWN, lambda graph, args: graph.set_nweight(0, 1, 1.0, 1.0), (img, 5.0, False))


def test_other_graph_kinds_refuse():
    from medpy_amd.graphcut import graph
    for cls in (graph.SparseGraph, graph.RegionGraph, graph.EmbeddedLatticeGraph):
        with pytest.raises(NotImplementedError):
            cls.update_boundary_term(object.__new__(cls), None, None)


def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    want = {"mgc_update_boundary": r"int mgc_update_boundary\(mgc_handle h, int term, const void\* image, int dtype, double sigma, const double\* spacing\);",
            "mgc_update_boundary_lut": r"int mgc_update_boundary_lut\(mgc_handle h, const double\* table, int64_t n\);",
            "mgc_get_boundary_update_info": r"int mgc_get_boundary_update_info\(mgc_handle h, int64_t\* out4\);"}
    for name, decl in want.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    assert _lib.SIGNATURES["mgc_update_boundary"] == _lib.SIGNATURES["mgc_set_boundary"]
    deps = build.DEPS
    assert "mgc_nlink_ops.inl" in deps and "mgc_nlink_fold.h" in deps

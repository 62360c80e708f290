"""CPU tier of the histograms over every voxel and of the iterated refit: the run merging of mgc_label_hist.h as a
stand-alone host program against a plain per-voxel count, the loop of iterate_regional_histogram on a scripted stand-in, and the
agreement of header, symbol table and library on the new call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GROUP = 16   # MGC_LH_GROUP


# ---- the run merging as a stand-alone program -----------------------------------------------------------------------------------
def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """label_hist_main.cpp compiled plainly and once more under the sanitizers: both run every case"""
    tmp = tmp_path_factory.mktemp("label_hist")
    src = os.path.join(HERE, "hostsim", "label_hist_main.cpp")
    exes = [str(tmp / "label_hist_plain")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exes[0], src])
    flags = _sanitizer_flags(tmp)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    if flags:
        exes.append(str(tmp / "label_hist_san"))
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + flags + ["-o", exes[1], src])
    return tmp, exes


def _expected_adds(labels, bins, nbins):
    """maximal runs of equal (label, bin) inside every group of 16 consecutive voxels"""
    key = np.where(labels != 0, 0, nbins) + bins
    adds = 0
    for base in range(0, key.size, GROUP):
        k = key[base:base + GROUP]
        adds += 1 + int((k[1:] != k[:-1]).sum())
    return adds


def _run(programs, labels, bins, nbins):
    tmp, exes = programs
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    bins = np.ascontiguousarray(bins, dtype=np.int64)
    labels.tofile(str(tmp / "labels.bin"))
    bins.tofile(str(tmp / "bins.bin"))
    want_fg = np.bincount(bins[labels != 0], minlength=nbins)
    want_bg = np.bincount(bins[labels == 0], minlength=nbins)
    for exe in exes:
        out = subprocess.run([exe, str(nbins), str(tmp / "labels.bin"), str(tmp / "bins.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        res = np.fromfile(str(tmp / "out.bin"), dtype=np.int64)
        assert res.size == 4 * nbins + 2
        merged, plain, adds, bad_groups = res[:2 * nbins], res[2 * nbins:4 * nbins], int(res[-2]), int(res[-1])
        np.testing.assert_array_equal(merged, plain)                       # the merged path counts what the per-voxel loop counts
        np.testing.assert_array_equal(merged[:nbins], want_fg)             # ... which is numpy.bincount under the labels
        np.testing.assert_array_equal(merged[nbins:], want_bg)             # ... and under their complement
        assert bad_groups == 0 and merged.sum() == labels.size
        assert adds == _expected_adds(labels, bins, nbins)                 # one add per maximal run, no more and no fewer
    return adds


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 5 * GROUP, 5 * GROUP + 9, 1000])
def test_merged_runs_count_what_a_plain_loop_counts(programs, n):
    """random, all one bin, alternating, a run over the whole group, and -- where n is no multiple of 16 -- a group cut short by
    the end of the volume, for every pattern"""
    rng = np.random.default_rng(5 + n)
    nbins = 7
    groups = (n + GROUP - 1) // GROUP
    # random labels and bins: few bins, so runs of every length up to a few voxels occur
    _run(programs, rng.integers(0, 2, n), rng.integers(0, nbins, n), nbins)
    _run(programs, rng.integers(0, 2, n) * 255, rng.integers(0, 2, n), 2)   # label bytes other than 1
    # all one bin and one label: one add per group
    for lab in (0, 1):
        assert _run(programs, np.full(n, lab), np.full(n, 3), nbins) == groups
    # all one bin, the label flips once in the middle of a group
    lab = np.zeros(n, np.uint8)
    lab[n // 2:] = 1
    assert _run(programs, lab, np.full(n, nbins - 1), nbins) == groups + (1 if n > 1 and (n // 2) % GROUP else 0)
    # alternating bins (no run longer than 1), alternating labels over one bin, and both alternating at different periods
    assert _run(programs, np.ones(n), np.arange(n) % 2, nbins) == n
    assert _run(programs, np.arange(n) % 2, np.zeros(n, np.int64), nbins) == n
    _run(programs, (np.arange(n) // 3) % 2, (np.arange(n) // 2) % nbins, nbins)
    # runs that span whole groups and end on a group border; a run that crosses a border is two adds
    _run(programs, np.ones(n), (np.arange(n) // GROUP) % nbins, nbins)
    _run(programs, np.ones(n), ((np.arange(n) + 5) // GROUP) % nbins, nbins)


def test_merged_runs_at_the_largest_bin_count(programs):
    rng = np.random.default_rng(2)
    n = 4 * GROUP + 3
    bins = rng.integers(0, 65536, n)
    bins[:4] = 65535
    bins[-3:] = 0
    _run(programs, rng.integers(0, 2, n), bins, 65536)
    _run(programs, np.ones(n), np.zeros(n, np.int64), 1)   # one bin: fg and bg are the two counters


# ---- the loop on a scripted stand-in --------------------------------------------------------------------------------------------
def _stand_in(script, lam=1.0, eps=0.5, binning=(4, 0.0, 1.0)):
    """a VoxelGraph without a library whose label_histograms / update_tweights_binned / maxflow are scripted: ``script`` is the list
    of fg histograms its cuts show, one per look"""
    from medpy_amd.graphcut import graph
    g = object.__new__(graph.VoxelGraph)
    g._h = None
    g._shape = (2, 2)
    g._binning = binning
    g._hist_params = (lam, eps)
    g._tweights_merged = False
    total = np.array([9, 9, 9, 9], np.int64)
    log = []

    def label_histograms(labels=None, nbins=None, lo=None, width=None):
        assert labels is None and nbins is None and lo is None and width is None
        fg = np.asarray(script[sum(1 for e in log if e[0] == "hist")], np.int64)
        log.append(("hist", fg.tolist()))
        return fg, total - fg

    def update_tweights_binned(source_table, sink_table, nbins=None, lo=None, width=None):
        log.append(("update", np.asarray(source_table).tolist(), np.asarray(sink_table).tolist()))

    def maxflow():
        log.append(("maxflow",))
        return 100.0 + sum(1 for e in log if e[0] == "maxflow")
    g.label_histograms, g.update_tweights_binned, g.maxflow = label_histograms, update_tweights_binned, maxflow
    return g, log, total


def _kinds(log):
    return [e[0] for e in log]


def test_loop_stops_at_the_fixed_point():
    from medpy_amd.graphcut import histogram_tables
    script = [[1, 2, 3, 4], [2, 2, 2, 4], [2, 3, 1, 4], [2, 3, 1, 4], [9, 9, 9, 9]]
    g, log, total = _stand_in(script, lam=2.0, eps=0.25)
    res = g.iterate_regional_histogram()
    assert res["converged"] is True and len(res["rounds"]) == 3
    assert [r["moved"] for r in res["rounds"]] == [None, 2, 2]
    assert [r["fg_voxels"] for r in res["rounds"]] == [10, 10, 10] and [r["bg_voxels"] for r in res["rounds"]] == [26, 26, 26]
    assert [r["flow"] for r in res["rounds"]] == [101.0, 102.0, 103.0]
    assert res["fg_hist"].tolist() == script[3] and res["bg_hist"].tolist() == (total - script[3]).tolist()
    assert _kinds(log) == ["hist", "update", "maxflow"] * 3 + ["hist"]   # the last look finds nothing moved: no update, no solve
    # every refit is fed histogram_tables of the histograms of the look before it, with the graph's lam and eps
    updates = [e for e in log if e[0] == "update"]
    for k, e in enumerate(updates):
        s, t = histogram_tables(np.array(script[k]), total - np.array(script[k]), 2.0, 0.25)
        assert e[1] == s.tolist() and e[2] == t.tolist()
    assert g._hist_params == (2.0, 0.25)


def test_loop_stop_below_max_refits_and_the_first_refit():
    script = [[1, 2, 3, 4], [3, 2, 1, 4], [3, 1, 2, 4], [3, 1, 2, 4]]   # moved: 4, 2, 0
    # stop_below = 2 stops one look earlier than the fixed point
    g, log, _ = _stand_in(script)
    res = g.iterate_regional_histogram(stop_below=2)
    assert res["converged"] is True and [r["moved"] for r in res["rounds"]] == [None, 4] and res["fg_hist"].tolist() == script[2]
    assert _kinds(log) == ["hist", "update", "maxflow"] * 2 + ["hist"]
    # stop_below above everything: the first refit is done all the same, the second look then stops the loop
    g, log, _ = _stand_in(script)
    res = g.iterate_regional_histogram(stop_below=10 ** 9)
    assert res["converged"] is True and len(res["rounds"]) == 1 and res["rounds"][0]["moved"] is None
    assert _kinds(log) == ["hist", "update", "maxflow", "hist"]
    # an already fitted term: one refit, then nothing moves
    g, log, _ = _stand_in([[1, 2, 3, 4]] * 3)
    res = g.iterate_regional_histogram()
    assert res["converged"] is True and len(res["rounds"]) == 1 and _kinds(log) == ["hist", "update", "maxflow", "hist"]
    # the cap: max_refits refits, one look behind the last, converged False while the histograms still move
    for cap in (1, 2):
        g, log, _ = _stand_in(script)
        res = g.iterate_regional_histogram(max_refits=cap)
        assert res["converged"] is False and len(res["rounds"]) == cap and res["fg_hist"].tolist() == script[cap]
        assert _kinds(log) == ["hist", "update", "maxflow"] * cap + ["hist"]
    g, log, _ = _stand_in(script)
    res = g.iterate_regional_histogram(max_refits=3)   # the cap is reached in the look that finds the fixed point
    assert res["converged"] is True and len(res["rounds"]) == 3
    g, log, _ = _stand_in(script)
    res = g.iterate_regional_histogram(max_refits=0)   # no refit allowed: one look, nothing else
    assert res["converged"] is False and res["rounds"] == [] and _kinds(log) == ["hist"] and res["fg_hist"].tolist() == script[0]
    # lam and eps given: used, and remembered
    from medpy_amd.graphcut import histogram_tables
    g, log, total = _stand_in(script)
    g.iterate_regional_histogram(max_refits=1, lam=3.0, eps=0.125)
    s, t = histogram_tables(np.array(script[0]), total - np.array(script[0]), 3.0, 0.125)
    assert log[1] == ("update", s.tolist(), t.tolist()) and g._hist_params == (3.0, 0.125)


def test_value_errors_come_before_the_library():
    from medpy_amd.graphcut import graph
    g, log, _ = _stand_in([[1, 2, 3, 4]] * 3)
    for kw in ({"max_refits": -1}, {"max_refits": 2.5}, {"max_refits": True}, {"stop_below": -1}, {"stop_below": 0.5}, {"eps": 0.0}, {"eps": float("nan")},
               {"lam": -1.0}, {"lam": float("inf")}):
        with pytest.raises(ValueError):
            g.iterate_regional_histogram(**kw)
    assert log == [] and g._hist_params == (1.0, 0.5)
    g._tweights_merged = True   # t-links merged on the host: refused as refit_regional_histogram refuses them
    with pytest.raises(NotImplementedError):
        g.iterate_regional_histogram()
    g._tweights_merged = False
    g._binning = g._hist_params = None   # a graph built without the term: the ValueError of refit_regional_histogram
    with pytest.raises(ValueError, match="built without a histogram term"):
        g.iterate_regional_histogram()
    with pytest.raises(ValueError, match="built without a histogram term"):
        g.refit_regional_histogram()
    assert log == []
    # label_histograms: the labels and the binning are checked before the library is asked (_h is None: a call would fail loudly)
    g = object.__new__(graph.VoxelGraph)
    g._h = None
    g._shape = (2, 3)
    ok = np.zeros((2, 3), bool)
    for bad in (np.zeros((3, 2), bool), np.zeros(6, bool), np.zeros((2, 3), np.int32), np.zeros((2, 3), np.float32), [[0, 1, 0], [1, 0, 0]], 1):
        with pytest.raises(ValueError, match="labels must be"):
            g.label_histograms(bad, 4, 0.0, 1.0)
    with pytest.raises(ValueError):   # no binning to fall back on
        g.label_histograms(ok)
    with pytest.raises(ValueError):   # nbins, lo and width come together
        g.label_histograms(ok, nbins=4)
    with pytest.raises(ValueError):
        g.label_histograms(ok, 0, 0.0, 1.0)
    assert g.label_histogram_info() == {"fg_voxels": 0, "bg_voxels": 0, "below": 0, "above": 0}
    for cls in (graph.SparseGraph, graph.RegionGraph, graph.EmbeddedLatticeGraph):   # the other graph classes get no new methods
        for name in ("label_histograms", "label_histogram_info", "iterate_regional_histogram"):
            assert not hasattr(cls, name)


# ---- symbols ----------------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree_on_the_new_call():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decl = (r"int mgc_label_histograms\(mgc_handle h, const uint8_t\* labels, int64_t nbins, double lo, double width, int64_t\* fg_hist, int64_t\* bg_hist, "
            r"int64_t\* out4\);")
    assert re.search(decl, header)
    assert "mgc_label_histograms" in _lib.SIGNATURES and hasattr(lib, "mgc_label_histograms")
    res, args = _lib.SIGNATURES["mgc_label_histograms"]
    assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    for d in ("mgc_label_hist.h", "mgc_label_hist_ops.inl", "mgc_label_hist_driver.inl"):
        assert d in build.DEPS and os.path.exists(os.path.join(build.CSRC, d)), d
    text = open(os.path.join(build.CSRC, "mgc_label_hist.h")).read()
    # the run merging stays plain C++: a stand-alone program includes it
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text
    assert int(re.search(r"#define MGC_LH_GROUP (\d+)", text).group(1)) == GROUP
    # behind every kernel that was there before it: at the end of the kernel file behind the binned driver, and nothing else includes it
    import driver_chain
    driver_chain.assert_behind_everything_before_it("mgc_label_hist_driver.inl", "mgc_label_hist")
    assert '#include "mgc_label_hist' not in open(os.path.join(build.CSRC, "mgc_binned_ops.inl")).read()

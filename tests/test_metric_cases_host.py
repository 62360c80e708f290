"""CPU tier of the Euclidean distance transform and the surface metrics: the steps of mgc_edt.h as a stand-alone host
program (plain, and under the sanitizers where this machine has the runtimes) against the brute-force statement of metric_cases.py
on every case, a doctored build that a named case must reject, the statement itself against SciPy, the host restatement of the
metrics against numbers recorded from the reference, and the agreement of header, symbol table and library."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import metric_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "metric_binary.json")
CXX = ["g++", "-std=c++17", "-ffp-contract=off"]


def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """edt_main.cpp compiled plainly, once more under the sanitizers (both run every case), and doctored"""
    tmp = tmp_path_factory.mktemp("edt")
    src = os.path.join(HERE, "hostsim", "edt_main.cpp")
    exes = [str(tmp / "edt_plain")]
    subprocess.check_call(CXX + ["-O2", "-o", exes[0], src])
    flags = _sanitizer_flags(tmp)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    if flags:
        exes.append(str(tmp / "edt_san"))
        subprocess.check_call(CXX + ["-O1", "-g"] + flags + ["-o", exes[1], src])
    doctored = str(tmp / "edt_doctored")
    subprocess.check_call(CXX + ["-O2", "-DEDT_SHORT=1", "-o", doctored, src])
    return tmp, exes, doctored


def _shape3(shape):
    return (1,) * (3 - len(shape)) + tuple(shape)


def _sp3(spacing, ndim):
    return [repr(1.0)] * (3 - ndim) + [repr(float(s)) for s in (spacing if spacing is not None else (1.0,) * ndim)]


def _edt(tmp, exe, plane, spacing):
    """{side: (squared transform, seeds, long lines)} of the host program"""
    np.ascontiguousarray(plane, dtype=np.uint8).tofile(str(tmp / "plane.bin"))
    out = subprocess.run([exe, "edt"] + [str(n) for n in _shape3(plane.shape)] + _sp3(spacing, plane.ndim) + [str(tmp / "plane.bin"), str(tmp / "out.bin")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    res = np.fromfile(str(tmp / "out.bin"), dtype=np.float64)
    assert res.size == 2 * (plane.size + 2)
    got = {}
    for side in (0, 1):
        part = res[side * (plane.size + 2):(side + 1) * (plane.size + 2)]
        got[side] = (part[:plane.size].reshape(plane.shape), int(part[-2]), int(part[-1]))
    return got


def _surf(tmp, exe, a, b, connectivity, spacing):
    np.ascontiguousarray(a, dtype=np.uint8).tofile(str(tmp / "a.bin"))
    np.ascontiguousarray(b, dtype=np.uint8).tofile(str(tmp / "b.bin"))
    out = subprocess.run([exe, "surf"] + [str(n) for n in _shape3(a.shape)] + [str(a.ndim), str(connectivity)] + _sp3(spacing, a.ndim)
                         + [str(tmp / "a.bin"), str(tmp / "b.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    res = np.fromfile(str(tmp / "out.bin"), dtype=np.float64)
    return res[2:], int(res[0]), int(res[1])


def _same_squares(got, want, spacing, what):
    """== at unit spacing (and wherever a value is infinite), within EDT_RTOL relative at the others"""
    assert got.shape == want.shape, what
    if spacing is None:
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=what)
        fin = np.isfinite(want)
        assert (np.abs(got[fin] - want[fin]) <= mc.EDT_RTOL * want[fin]).all(), what


@pytest.mark.parametrize("case", mc.CASES + mc.LONG_CASES, ids=mc.case_id)
def test_host_program_matches_brute_force(programs, case):
    """every pattern x shape x spacing, both sides, plain and under the sanitizers.  The host program promises the definition bit for
    bit, so it is held to == at every spacing, which is no less than the tolerance asks."""
    tmp, exes, _ = programs
    plane = mc.plane_of(case)
    long_lines = {s: (plane.size // s if s > mc.LONG_LINE else 0) for s in plane.shape[:-1]}
    for spacing in mc.SPACINGS:
        sp = mc.spacing_for(spacing, plane.ndim)
        for exe in exes:
            got = _edt(tmp, exe, plane, sp)
            for side in (0, 1):
                want = mc.expected_edt_sq(plane, side, sp)
                what = "%s side %d spacing %r" % (mc.case_id(case), side, sp)
                _same_squares(got[side][0], want, sp, what)
                np.testing.assert_array_equal(got[side][0], want, err_msg=what)
                nseeds = int(((plane != 0) == bool(side)).sum())
                assert got[side][1] == nseeds, what
                assert got[side][2] == (sum(long_lines.values()) if nseeds else 0), what
                if nseeds == 0:
                    assert np.isposinf(got[side][0]).all()
                else:
                    assert (got[side][0][(plane != 0) == bool(side)] == 0).all()


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_host_surface_lists_match(programs, case):
    """every case against partner(shape), both ways round, at every connectivity and spacing: length, order, values"""
    tmp, exes, _ = programs
    a, b = mc.plane_of(case), mc.partner(case[1])
    for conn in mc.connectivities(case[1]):
        for spacing in mc.SPACINGS:
            sp = mc.spacing_for(spacing, a.ndim)
            for exe in exes:
                for p, q in ((a, b), (b, a)):
                    want, na, nb = mc.expected_surface_sq(p, q, conn, sp)
                    got, ga, gb = _surf(tmp, exe, p, q, conn, sp)
                    assert (ga, gb) == (na, nb)
                    np.testing.assert_array_equal(got, want)


def test_a_flat_volume_is_not_a_plane(programs):
    """(1, Y, X) on a 3-D handle: every voxel has neighbours outside along the first axis and is border; the same plane on a 2-D
    handle has an interior"""
    tmp, exes, _ = programs
    a2, b2 = mc.box((13, 31)), mc.partner((13, 31))
    a3, b3 = a2[None], b2[None]
    for conn in (1, 2):
        got2 = _surf(tmp, exes[0], a2, b2, conn, None)
        got3 = _surf(tmp, exes[0], a3, b3, conn, None)
        assert got3[1] == int(a2.sum()) and got3[2] == int(b2.sum())       # all of the object
        assert got2[1] < got3[1]
        for got, (p, q) in ((got2, (a2, b2)), (got3, (a3, b3))):
            want, na, nb = mc.expected_surface_sq(p, q, conn, None)
            assert (got[1], got[2]) == (na, nb)
            np.testing.assert_array_equal(got[0], want)


def test_overlap_classes(programs):
    tmp, exes, _ = programs
    for case in mc.CASES[::7]:
        a, b = mc.plane_of(case), mc.partner(case[1])
        a.tofile(str(tmp / "a.bin"))
        b.tofile(str(tmp / "b.bin"))
        for exe in exes:
            assert subprocess.run([exe, "counts", str(a.size), str(tmp / "a.bin"), str(tmp / "b.bin"), str(tmp / "out.bin")]).returncode == 0
            assert np.fromfile(str(tmp / "out.bin")).astype(np.int64).tolist() == mc.expected_counts(a, b)


def test_doctored_window_is_rejected_by_the_corner_seed(programs):
    """the same program with every window one candidate short: the voxels at the far end of a line from the only seed lose it"""
    tmp, _, doctored = programs
    for shape in [(9, 17, 20), (70, 9, 17), (33, 70), (mc.LONG_LINE + 1, 1, 3)]:
        plane = mc.corner(shape)
        got = _edt(tmp, doctored, plane, None)[1][0]
        want = mc.expected_edt_sq(plane, 1)
        assert not np.array_equal(got, want)
        far = tuple(n - 1 for n in shape)
        assert got[far] != want[far]
        # the last axis has no window: its rows are right
        np.testing.assert_array_equal(got[(0,) * (len(shape) - 1)], want[(0,) * (len(shape) - 1)])


# ---- the definition is held to something --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_the_definition_against_scipy(case):
    plane = mc.plane_of(case)
    for side in (0, 1):
        seeds = (plane != 0) == bool(side)
        if not seeds.any():
            assert np.isposinf(mc.expected_edt_sq(plane, side)).all()
            continue
        for spacing in mc.SPACINGS:
            sp = mc.spacing_for(spacing, plane.ndim)
            want = mc.expected_edt_sq(plane, side, sp)
            ref = ndimage.distance_transform_edt(~seeds, sampling=sp)
            if sp is None:
                np.testing.assert_array_equal(np.sqrt(want), ref)
            else:
                sq = ref * ref
                # the reference's own square root and this squaring add a rounding each to its 2.0 * 2^-52: still inside the bound
                assert (np.abs(sq - want) <= mc.EDT_RTOL * want).all(), (mc.case_id(case), side, sp, float(np.max(np.abs(sq - want) / np.where(want > 0, want, 1))))


# ---- the metrics on the host against the numbers recorded from the reference ------------------------------------------------------------------
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _close(got, want, exact):
    return got == want if exact else abs(got - want) <= mc.METRIC_RTOL * abs(want)


@pytest.mark.parametrize("case", mc.golden_cases(), ids=mc.case_id)
def test_host_metrics_reproduce_the_reference(case):
    gold = _golden()
    a, b = mc.plane_of(case), mc.partner(case[1])
    for conn in mc.connectivities(case[1]):
        for spacing in mc.SPACINGS:
            sp = mc.spacing_for(spacing, a.ndim)
            want = gold["surface"][mc.golden_key(case, sp, conn)]
            got = mc.host_metrics(a, b, sp, conn)
            for name in mc.SURFACE_METRICS:
                assert _close(got[name], want[name], sp is None), (name, conn, sp, got[name], want[name])


def test_golden_file_covers_the_cases():
    gold = _golden()
    keys = {mc.golden_key(c, mc.spacing_for(s, len(c[1])), k) for c in mc.golden_cases() for s in mc.SPACINGS for k in mc.connectivities(c[1])}
    assert set(gold["surface"]) == keys
    assert set(gold["counts"]) == {mc.case_id(c) for c in mc.golden_cases()}
    for v in gold["counts"].values():
        assert set(v) == set(mc.COUNT_METRICS)
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_count_metrics_from_four_counts():
    from medpy_amd.metric import binary
    gold = _golden()
    for case in mc.golden_cases():
        tp, fp, fn, tn = mc.expected_counts(mc.plane_of(case), mc.partner(case[1]))
        for name in mc.COUNT_METRICS:
            assert binary._from_counts(name, tp, fp, fn, tn) == gold["counts"][mc.case_id(case)][name], (name, mc.case_id(case))
    # the rule of the reference where a ratio divides by zero: two empty objects overlap fully (1.0), the rates are 0.0; ravd raises
    # on an empty reference
    for name, want in (("dc", 1.0), ("jc", 1.0), ("precision", 0.0), ("recall", 0.0), ("specificity", 0.0)):
        assert binary._from_counts(name, 0, 0, 0, 0) == want
    with pytest.raises(RuntimeError, match="second supplied array"):
        binary._from_counts("ravd", 0, 3, 0, 5)


# ---- symbols, classes, argument checks ----------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decls = {
        "mgc_distance_transform": r"int mgc_distance_transform\(mgc_handle h, const uint8_t\* plane, int side, const double\* spacing, double\* out_sq, int64_t\* out4\);",
        "mgc_surface_distances": r"int mgc_surface_distances\(mgc_handle h, const uint8_t\* a, const uint8_t\* b, int connectivity, const double\* spacing, int64_t cap, "
                                 r"double\* sds_sq, int64_t\* out8\);",
        "mgc_overlap_counts": r"int mgc_overlap_counts\(mgc_handle h, const uint8_t\* a, const uint8_t\* b, int64_t\* out4\);",
    }
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    for d in ("mgc_edt.h", "mgc_edt_ops.inl", "mgc_edt_driver.inl"):
        assert d in build.DEPS and os.path.exists(os.path.join(build.CSRC, d)), d
    text = open(os.path.join(build.CSRC, "mgc_edt.h")).read()
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text   # plain C++: a stand-alone program includes it
    assert int(re.search(r"#define MGC_EDT_PANEL_LINE (\d+)", text).group(1)) == mc.LONG_LINE
    assert "-ffp-contract=off" in build.FLAGS
    # behind every kernel that was there before it: at the end of the kernel file behind the driver of the components, and nothing in
    # front includes it
    import driver_chain
    driver_chain.assert_behind_everything_before_it("mgc_edt_driver.inl", "mgc_edt")


def test_classes_and_value_errors_without_a_library():
    from medpy_amd.graphcut import graph
    from medpy_amd.metric import binary
    import medpy_amd.metric
    for cls in (graph.SparseGraph, graph.RegionGraph):
        g = object.__new__(cls)
        for name in ("distance_transform", "surface_distances", "overlap_counts"):
            with pytest.raises(NotImplementedError, match="voxel lattice"):
                getattr(g, name)(None)
    for name in ("distance_transform", "surface_distances", "overlap_counts"):
        assert hasattr(graph.EmbeddedLatticeGraph, name) and hasattr(graph.VoxelGraph, name)
    for name in mc.COUNT_METRICS + mc.SURFACE_METRICS:
        assert callable(getattr(binary, name)) and getattr(medpy_amd.metric, name) is getattr(binary, name)
    # the arguments are checked before the library is asked (_h is None: a call would fail loudly)
    g = object.__new__(graph.VoxelGraph)
    g._h = None
    g._shape = (2, 3)
    ok = np.zeros((2, 3), bool)
    for bad in (np.zeros((3, 2), bool), np.zeros((2, 3), np.float32), [[0, 1, 0], [1, 0, 0]]):
        with pytest.raises(ValueError, match="labels must be"):
            g.distance_transform(bad)
        with pytest.raises(ValueError, match="reference must be"):
            g.overlap_counts(bad, ok)
    with pytest.raises(ValueError, match="to must be"):
        g.distance_transform(ok, to="inside")
    for sp in ((1.0, 0.0), (1.0, -2.0), (np.inf, 1.0), (np.nan, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            g.distance_transform(ok, spacing=sp)
        with pytest.raises(ValueError, match="spacing"):
            binary.hd(ok, ok, voxelspacing=sp)
    with pytest.raises(RuntimeError, match="length"):
        binary.hd(ok, ok, voxelspacing=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="connectivity"):
        g.surface_distances(ok, ok, connectivity=3)
    with pytest.raises(NotImplementedError):
        binary.hd(np.ones((2, 2, 2, 2)), np.ones((2, 2, 2, 2)))
    with pytest.raises(NotImplementedError):
        binary.dc(np.ones((2, 2, 2, 2)), np.ones((2, 2, 2, 2)))

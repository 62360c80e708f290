"""CPU tier of the geodesic distance transform: the steps of mgc_geo.h as a stand-alone host program (plain, and under
the sanitizers where this machine has the runtimes) against the Dijkstra statement of geodesic_cases.py on every case with ``==``,
two doctored builds that named cases must reject and no other case may, the statement itself against SciPy and against two answers
spelled out by hand, the rule of the regional term, and the agreement of header, symbol table and library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import geodesic_cases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = ["g++", "-std=c++17", "-ffp-contract=off"]
NAMES = [c.name for c in gc.CASES]


def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """geo_main.cpp compiled plainly, once more under the sanitizers (both run every case), and the two doctored builds"""
    tmp = tmp_path_factory.mktemp("geo")
    src = os.path.join(HERE, "hostsim", "geo_main.cpp")
    exes = [str(tmp / "geo_plain")]
    subprocess.check_call(CXX + ["-O2", "-o", exes[0], src])
    flags = _sanitizer_flags(tmp)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    if flags:
        exes.append(str(tmp / "geo_san"))
        subprocess.check_call(CXX + ["-O1", "-g"] + flags + ["-o", exes[1], src])
    doctored = {}
    for name, bit in (("GEO_NO_DIAGONAL_WAKE", 1), ("GEO_NO_SELF_WAKE", 2)):
        doctored[name] = str(tmp / name.lower())
        subprocess.check_call(CXX + ["-O2", "-D%s" % name, "-o", doctored[name], src])
    return tmp, exes, doctored


def _run(tmp, exe, case, order=1):
    """(D, info) of the host program: the tiles of a round in the random order of seed ``order``"""
    img, seeds = case.inputs()
    nd = len(case.shape)
    shape3 = (1,) * (3 - nd) + case.shape
    sp3 = [repr(1.0)] * (3 - nd) + [repr(float(s)) for s in (case.spacing or (1.0,) * nd)]
    image = "-"
    if case.gamma != 0:
        image = str(tmp / "image.bin")
        img.astype(np.float64).tofile(image)
    np.ascontiguousarray(seeds, dtype=np.uint8).tofile(str(tmp / "seeds.bin"))
    out = subprocess.run([exe] + [str(n) for n in shape3] + [str(case.full), repr(case.gamma), repr(case.step)] + sp3 + [str(order), image, str(tmp / "seeds.bin"),
                                                                                                                           str(tmp / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    res = np.fromfile(str(tmp / "out.bin"), dtype=np.float64)
    assert res.size == seeds.size + 6
    return res[:-6].reshape(case.shape), dict(zip(("seeds", "rounds", "tile_visits", "sweeps", "capped_visits", "finite"), res[-6:].astype(np.int64).tolist()))


# ---- the host program on every case --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_program_equals_the_statement(programs, name):
    tmp, exes, _ = programs
    case = gc.BY_NAME[name]
    want = case.expected()
    _, seeds = case.inputs()
    for exe in exes:
        got, info = _run(tmp, exe, case)
        assert np.array_equal(got, want), (os.path.basename(exe), int((got != want).sum()))
        assert info["seeds"] == int(seeds.sum()) and info["finite"] == int(np.isfinite(want).sum())
        assert (info["rounds"] == 0) == (info["seeds"] == 0)
        assert info["sweeps"] <= gc.SWEEP_CAP * info["tile_visits"]


def test_another_order_of_the_tiles_gives_the_same_numbers(programs):
    tmp, exes, _ = programs
    for name in NAMES:
        if name.startswith("wall_") or name.startswith("9x17x20"):
            case = gc.BY_NAME[name]
            for order in (2, 3):
                assert np.array_equal(_run(tmp, exes[0], case, order)[0], case.expected()), (name, order)


def test_the_wall_cases_make_the_schedule_work(programs):
    tmp, exes, _ = programs
    for full in ("face", "full"):
        _, info = _run(tmp, exes[0], gc.BY_NAME["wall_serpentine-g1000-%s" % full])
        assert info["capped_visits"] > 0 and info["rounds"] > 1, info   # longer than the sweep cap: the tile wakes itself
        _, info = _run(tmp, exes[0], gc.BY_NAME["wall_corridor_2d-g1000-%s" % full])
        tiles = 5 * 9
        assert info["tile_visits"] > 2 * tiles, info                       # settled tiles are woken again, more than once
    want = gc.BY_NAME["wall_diagonal-g1000-full"].expected()
    assert want[8, 8, 8] == want[7, 7, 7] + np.sqrt(3.0)                    # at the full neighbourhood the chamber opens through the corner
    assert gc.BY_NAME["wall_diagonal-g1000-face"].expected()[8, 8, 8] > 1000.0   # at the face neighbourhood only through the wall


# ---- the doctored builds -------------------------------------------------------------------------------------------------------
def _rejected(tmp, exe):
    return {name for name in NAMES if not np.array_equal(_run(tmp, exe, gc.BY_NAME[name])[0], gc.BY_NAME[name].expected())}


def test_no_diagonal_wake_is_rejected_by_the_diagonal_opening_at_the_full_neighbourhood_only(programs):
    tmp, _, doctored = programs
    bad = _rejected(tmp, doctored["GEO_NO_DIAGONAL_WAKE"])
    assert "wall_diagonal-g1000-full" in bad and "wall_diagonal-g1-full" in bad
    assert not {n for n in bad if n.endswith("-face")}, bad            # accepted at the face neighbourhood: no tile reads across an edge there
    assert {n for n in bad if not n.startswith("wall_diagonal")} == set(), bad


def test_no_self_wake_is_rejected_by_the_serpentine(programs):
    tmp, _, doctored = programs
    bad = _rejected(tmp, doctored["GEO_NO_SELF_WAKE"])
    for full in ("face", "full"):
        assert "wall_serpentine-g1000-%s" % full in bad
    # nothing that fits the sweep cap is affected: only cases with a visit that ended at the cap may differ
    for name in bad:
        assert _run(tmp, programs[1][0], gc.BY_NAME[name])[1]["capped_visits"] > 0, name


# ---- the statement itself ------------------------------------------------------------------------------------------------------
def _scipy_dijkstra(case):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    img, seeds = case.inputs()
    shape, nd = case.shape, len(case.shape)
    val = img.astype(np.float64)
    sp = case.spacing or (1.0,) * nd
    ids = np.arange(seeds.size).reshape(shape)
    rows, cols, w = [], [], []
    for d in gc.offsets(nd, case.full):
        e = gc.step_length(d, sp, case.step)
        src = tuple(slice(max(0, -o), m - max(0, o)) for o, m in zip(d, shape))
        dst = tuple(slice(max(0, o), m - max(0, -o)) for o, m in zip(d, shape))
        rows.append(ids[src].ravel())
        cols.append(ids[dst].ravel())
        w.append(np.full(ids[src].size, e) if case.gamma == 0 else e + case.gamma * np.abs(val[src] - val[dst]).ravel())
    m = csr_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(seeds.size, seeds.size))
    return dijkstra(m, indices=np.flatnonzero(seeds.ravel()), min_only=True).reshape(shape)


def test_statement_equals_scipy_where_every_arc_is_positive():
    pytest.importorskip("scipy")
    n = 0
    for case in gc.CASES:
        _, seeds = case.inputs()
        if case.step > 0 and seeds.any():   # (SciPy's sparse graph has no arcs of length 0, and wants a seed)
            assert np.array_equal(_scipy_dijkstra(case), case.expected()), case.name
            n += 1
    assert n > 60


def test_statement_by_hand():
    ramp = np.arange(5, dtype=np.uint8)
    seeds = np.zeros(5, bool)
    seeds[0] = True
    assert gc.expected_geodesic(ramp, seeds, 2.0, 1.0, None, 0).tolist() == [0.0, 3.0, 6.0, 9.0, 12.0]
    seeds[:] = [False, False, True, False, False]
    assert gc.expected_geodesic(ramp, seeds, 2.0, 1.0, (0.5,), 1).tolist() == [5.0, 2.5, 0.0, 2.5, 5.0]
    wall = np.array([[0, 9, 0], [0, 9, 0], [0, 0, 0]], dtype=np.int16)
    seeds = np.zeros((3, 3), bool)
    seeds[0, 0] = True
    # round the wall: down, along the bottom, up; into the wall costs 1 + 9, along it 1
    assert gc.expected_geodesic(wall, seeds, 1.0, 1.0, None, 0).tolist() == [[0.0, 10.0, 6.0], [1.0, 11.0, 5.0], [2.0, 3.0, 4.0]]
    r2 = np.sqrt(2.0)
    full = gc.expected_geodesic(wall, seeds, 1.0, 1.0, None, 1)
    assert full[2, 1] == 1.0 + r2 and full[1, 2] == (1.0 + r2) + r2 and full[0, 2] == ((1.0 + r2) + r2) + 1.0 and full[1, 1] == r2 + 9.0
    assert np.isinf(gc.expected_geodesic(wall, np.zeros((3, 3), bool), 1.0, 1.0, None, 1)).all()
    assert (gc.expected_geodesic(None, seeds, 0.0, 0.0, None, 0) == 0).all()
    assert gc.step_length((1, 1, 1), (3.3, 1.1, 0.9), 0.5) == 0.5 * np.sqrt((0.9 * 0.9 + 1.1 * 1.1) + 3.3 * 3.3)


def test_expected_term_on_its_five_branches():
    inf = np.inf
    d_f = np.array([inf, inf, 2.0, 0.0, 1.0, 3.0])
    d_b = np.array([inf, 5.0, inf, 0.0, 3.0, 0.0])
    s, k = gc.expected_term(d_f, d_b, 0.8)
    assert s.tolist() == [0.0, 0.0, 0.8, 0.4, 0.8 * (3.0 / 4.0), 0.0]
    assert k.tolist() == [0.0, 0.8, 0.0, 0.4, 0.8 * (1.0 / 4.0), 0.8 * (3.0 / 3.0)]
    s, k = gc.expected_term(d_f, d_b, 0.0)
    assert not s.any() and not k.any()


# ---- symbols, classes, argument checks -----------------------------------------------------------------------------------------
def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decls = {
        "mgc_geodesic_distance": r"int mgc_geodesic_distance\(mgc_handle h, const uint8_t\* seeds, int source, int full, double gamma, double step, const double\* spacing, "
                                 r"double\* out, int64_t\* out8\);",
        "mgc_add_tweights_geodesic": r"int mgc_add_tweights_geodesic\(mgc_handle h, int full, double gamma, double step, const double\* spacing, double lam\);",
        "mgc_update_tweights_geodesic": r"int mgc_update_tweights_geodesic\(mgc_handle h, int full, double gamma, double step, const double\* spacing, double lam\);",
    }
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    for d in ("mgc_geo.h", "mgc_geo_ops.inl", "mgc_geo_driver.inl"):
        assert d in build.DEPS and os.path.exists(os.path.join(build.CSRC, d)), d
    text = open(os.path.join(build.CSRC, "mgc_geo.h")).read()
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text   # plain C++: a stand-alone program includes it
    assert int(re.search(r"#define MGC_GEO_SWEEP_CAP (\d+)", text).group(1)) == gc.SWEEP_CAP
    assert text.count("#pragma clang fp contract(off)") >= 2 and "-ffp-contract=off" in build.FLAGS
    assert "sqrt" not in open(os.path.join(build.CSRC, "mgc_geo_ops.inl")).read()   # the device takes no square root
    # behind every other kernel of the library: the last of the drivers at the end of the kernel file, and nothing in front includes it
    import driver_chain
    driver_chain.assert_behind_everything_before_it("mgc_geo_driver.inl", "mgc_geo")


def test_classes_and_value_errors_without_a_library():
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel, graph
    for cls in (graph.SparseGraph, graph.RegionGraph):
        g = object.__new__(cls)
        for name in ("geodesic_distance", "geodesic_info", "refit_regional_geodesic"):
            with pytest.raises(NotImplementedError, match="voxel lattice"):
                getattr(g, name)()
    for name in ("geodesic_distance", "geodesic_info", "refit_regional_geodesic"):
        assert hasattr(graph.EmbeddedLatticeGraph, name) and hasattr(graph.VoxelGraph, name)
    assert "regional_geodesic" in energy_voxel.__all__ and graphcut.regional_geodesic is energy_voxel.regional_geodesic
    # the arguments are checked before the library is asked (_h is None: a call would fail loudly)
    g = object.__new__(graph.VoxelGraph)
    g._h = None
    g._shape = (2, 3)
    g._full_neighbourhood = False
    ok = np.zeros((2, 3), bool)
    for bad in (np.zeros((3, 2), bool), np.zeros((2, 3), np.float32), [[0, 1, 0], [1, 0, 0]]):
        with pytest.raises(ValueError, match="seeds must be"):
            g.geodesic_distance(bad)
    with pytest.raises(ValueError, match="seeds must be"):
        g.geodesic_distance("foreground")
    for kw in ({"gamma": -1.0}, {"gamma": np.inf}, {"step": -0.5}, {"step": np.nan}):
        with pytest.raises(ValueError, match="finite and not negative"):
            g.geodesic_distance(ok, **kw)
    for sp in ((1.0, 0.0), (1.0, -2.0), (np.inf, 1.0), (np.nan, 1.0), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            g.geodesic_distance(ok, spacing=sp)
    for conn in (0, 3, 26):
        with pytest.raises(ValueError, match="connectivity"):
            g.geodesic_distance(ok, connectivity=conn)
    with pytest.raises(ValueError, match="built without a geodesic term"):
        g.refit_regional_geodesic()
    assert g.geodesic_info() == dict.fromkeys(graph.VoxelGraph.GEODESIC_INFO_KEYS, 0)
    # the facade checks before it records, and a graph that goes to the sparse-graph solver refuses the term
    f = graphcut.GCGraph(6, 7, shape=(2, 3))
    for args in ((-1.0, 1.0), (1.0, np.inf), (1.0, 1.0, -1.0), (1.0, 1.0, 1.0, (1.0, 0.0)), (1.0, 1.0, 1.0, None, 3), (1.0, 1.0, 1.0, None, None, np.zeros(5)), (1.0,)):
        with pytest.raises(ValueError):
            energy_voxel.regional_geodesic(f, args)
    energy_voxel.regional_geodesic(f, (1.0, 2.0))
    f.set_nweight(0, 5, 1.0, 1.0)   # not neighbours of the lattice: the sparse-graph solver
    with pytest.raises(NotImplementedError, match="geodesic regional term"):
        f.get_graph()

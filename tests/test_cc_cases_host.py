"""CPU tier of the connected components and the cleaning rule: the steps of mgc_cc.h as a stand-alone host program against
scipy.ndimage.label on every case of cc_cases.py, a doctored stand-in that the corner and edge cases must reject, the rule of the
cleaning step, the host statement of the cleaning on hand-written cases, and the agreement of header, symbol table and library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cc_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]   # (side, full) in the order cc_main labels


def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """cc_main.cpp compiled plainly, once more under the sanitizers (both run every case), and doctored"""
    tmp = tmp_path_factory.mktemp("cc")
    src = os.path.join(HERE, "hostsim", "cc_main.cpp")
    exes = [str(tmp / "cc_plain")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exes[0], src])
    flags = _sanitizer_flags(tmp)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    if flags:
        exes.append(str(tmp / "cc_san"))
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + flags + ["-o", exes[1], src])
    doctored = str(tmp / "cc_doctored")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCC_SKIP_DIAGONAL", "-o", doctored, src])
    return tmp, exes, doctored


def _label(tmp, exe, mask, fg, bg, seed):
    """the four labellings of cc_main as {(side, full): (ids, first, size, flags, unions, walk)}"""
    shape3 = (1,) * (3 - mask.ndim) + mask.shape
    paths = {}
    for name, arr in (("plane", mask), ("fg", fg), ("bg", bg)):
        paths[name] = "-"
        if arr is not None:
            paths[name] = str(tmp / (name + ".bin"))
            np.ascontiguousarray(arr, dtype=np.uint8).tofile(paths[name])
    out = subprocess.run([exe, "run"] + [str(n) for n in shape3] + [str(seed), paths["plane"], paths["fg"], paths["bg"], str(tmp / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    res = np.fromfile(str(tmp / "out.bin"), dtype=np.int64)
    got, at = {}, 0
    for combo in COMBOS:
        K, unions, walk = (int(x) for x in res[at:at + 3])
        at += 3
        ids = res[at:at + mask.size].astype(np.int32).reshape(mask.shape)
        at += mask.size
        first, size, flags = res[at:at + K], res[at + K:at + 2 * K], res[at + 2 * K:at + 3 * K].astype(np.uint8)
        at += 3 * K
        got[combo] = (ids, first, size, flags, unions, walk)
    assert at == res.size
    return got


def _check(got, mask, fg, bg, combos=COMBOS):
    for side, full in combos:
        ids, first, size, flags = cc.expected_components(mask, side, full, fg, bg)
        g = got[(side, full)]
        np.testing.assert_array_equal(g[0], ids)
        np.testing.assert_array_equal(g[1], first)
        np.testing.assert_array_equal(g[2], size)
        np.testing.assert_array_equal(g[3], flags)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_host_program_matches_scipy(programs, case):
    """every pattern x shape, both sides, both neighbourhoods, without markers and with sparse ones, plain and under the sanitizers"""
    tmp, exes, _ = programs
    pattern, shape = case
    mask = pattern(shape)
    for k, (fg, bg) in enumerate([(None, None), cc.sparse_markers(shape)]):
        for exe in exes:
            _check(_label(tmp, exe, mask, fg, bg, seed=11 + k), mask, fg, bg)


def test_the_order_of_the_visits_does_not_matter(programs):
    tmp, exes, _ = programs
    mask = cc.bernoulli(0.31)((17, 16, 31))
    fg, bg = cc.sparse_markers(mask.shape)
    for seed in range(5):
        _check(_label(tmp, exes[0], mask, fg, bg, seed), mask, fg, bg)


def test_checkerboard_counts(programs):
    tmp, exes, _ = programs
    for shape in cc.SHAPES:
        mask = cc.checkerboard(shape)
        got = _label(tmp, exes[0], mask, None, None, 1)
        assert got[(1, 0)][1].size == (mask.size + 1) // 2           # face: every voxel alone
        if sum(n > 1 for n in shape) >= 2:
            assert got[(1, 1)][1].size == 1 and got[(0, 1)][1].size == 1   # full: one component per colour


def test_a_solid_face_costs_a_handful_of_unions(programs):
    tmp, exes, _ = programs
    got = _label(tmp, exes[0], cc.ones((24, 24, 24)), None, None, 1)
    faces = 3 * 2 * 9   # 27 tiles: 54 faces between two of them, 64 pairs across each
    # One union per face for the first pair of the run, and at most two more: the first pair's upper voxel is its tile's local root,
    # whose parent word moves when the tile is linked, so the two pairs that would lean on that pair may not recognise it.  None for
    # the edges and corners: a voxel of this side lies between the two of every diagonal pair.
    for full in (0, 1):
        assert faces <= got[(1, full)][4] <= 3 * faces
    assert got[(1, 0)][1].size == 1 and got[(1, 0)][2][0] == 24 ** 3


def test_doctored_merge_is_rejected_by_the_corner_and_edge_cases(programs):
    """the same program with the corner / edge pairs of the merge left out: right at face, wrong at full exactly where voxels meet
    only across a tile corner or a tile edge"""
    tmp, _, doctored = programs
    for pattern, shape in [(cc.corner_touch, (9, 10, 11)), (cc.corner_touch, (24, 24, 24)), (cc.corner_touch, (40, 33)), (cc.edge_touch, (17, 16, 31)),
                           (cc.edge_touch, (24, 24, 24))]:
        mask = pattern(shape)
        got = _label(tmp, doctored, mask, None, None, 3)
        _check(got, mask, None, None, combos=[(0, 0), (1, 0)])   # the face neighbourhood has no such pairs
        want = cc.expected_components(mask, 1, 1)
        assert got[(1, 1)][1].size > want[1].size                # the two voxels did not join
        with pytest.raises(AssertionError):
            _check(got, mask, None, None, combos=[(1, 1)])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def _rule(programs, size, flags, min_size, largest, seeded):
    tmp, exes, _ = programs
    np.concatenate([np.asarray(size, np.int64), np.asarray(flags, np.int64)]).tofile(str(tmp / "table.bin"))
    res = None
    for exe in exes:
        out = subprocess.run([exe, "rule", str(min_size), str(largest), str(seeded), str(tmp / "table.bin"), str(tmp / "rule.bin")], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        res = np.fromfile(str(tmp / "rule.bin"), dtype=np.int64)
        assert res.size == len(size) + 2
    return res[:-2].astype(bool).tolist(), int(res[-2]), int(res[-1])


def test_rule_of_step_one(programs):
    size = [5, 9, 9, 1, 9, 3]
    flags = [1, 0, 5, 1, 4, 0]
    T, F = True, False
    assert _rule(programs, size, flags, 1, 0, 0) == ([T] * 6, 6, 0)                          # the identity
    assert _rule(programs, size, flags, 4, 0, 0) == ([T, T, T, F, T, F], 4, 4)
    assert _rule(programs, size, flags, 1, 1, 0) == ([F, T, F, F, F, F], 1, 27)              # ties on size: the smaller id
    assert _rule(programs, size, flags, 1, 2, 0) == ([F, T, T, F, F, F], 2, 18)
    assert _rule(programs, size, flags, 1, 4, 0) == ([T, T, T, F, T, F], 4, 4)
    assert _rule(programs, size, flags, 1, 60, 0) == ([T] * 6, 6, 0)                         # more than there are
    assert _rule(programs, size, flags, 1, 0, 1) == ([T, F, T, T, F, F], 3, 21)              # seeded
    assert _rule(programs, size, flags, 2, 1, 1) == ([F, F, T, F, F, F], 1, 27)              # all together
    assert _rule(programs, size, [f & ~1 for f in flags], 1, 0, 1) == ([F] * 6, 0, 36)       # seeded without markers leaves nothing
    assert _rule(programs, [], [], 1, 3, 1) == ([], 0, 0)
    rng = np.random.default_rng(4)
    for _ in range(20):
        n = int(rng.integers(1, 40))
        size, flags = rng.integers(1, 6, n), rng.integers(0, 8, n)
        m, lg, sd = int(rng.integers(1, 4)), int(rng.integers(0, 6)), int(rng.integers(0, 2))
        keep = cc.rule_keep(size, flags, m, lg, sd)
        assert _rule(programs, size, flags, m, lg, sd) == (keep.tolist(), int(keep.sum()), int(size[~keep].sum()))


def test_expected_clean_on_hand_written_cases():
    F = np.array([[1, 1, 0, 0, 0, 0, 1],
                  [1, 0, 0, 1, 1, 0, 0],
                  [0, 0, 0, 1, 1, 0, 0],
                  [0, 1, 0, 0, 0, 1, 0],
                  [0, 0, 0, 0, 0, 0, 0]], np.uint8)
    same = lambda got, want: np.array_equal(got, np.array(want, bool))
    out, changed, info = cc.expected_clean(F, cc.rule())
    assert same(out, F) and changed.size == 0 and info == dict(fg_components=5, survivors=5, voxels_removed=0, cavities_filled=0, voxels_filled=0, voxels_changed=0)
    out, changed, info = cc.expected_clean(F, cc.rule(min_size=2))
    assert same(out, [[1, 1, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 0, 0], [0, 0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0] * 7])
    assert changed.tolist() == [6, 22, 26] and info["survivors"] == 2 and info["voxels_removed"] == 3
    out, changed, info = cc.expected_clean(F, cc.rule(largest=1))
    assert same(out, [[0] * 7, [0, 0, 0, 1, 1, 0, 0], [0, 0, 0, 1, 1, 0, 0], [0] * 7, [0] * 7]) and changed.tolist() == [0, 1, 6, 7, 22, 26]
    # at the full neighbourhood the square and the voxel at (3, 5) are one component of five
    out, changed, info = cc.expected_clean(F, cc.rule(fg_full=1, largest=1))
    assert same(out, [[0] * 7, [0, 0, 0, 1, 1, 0, 0], [0, 0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 1, 0], [0] * 7]) and info["fg_components"] == 4
    fg = np.zeros_like(F)
    fg[0, 1] = fg[3, 1] = 1
    out, changed, info = cc.expected_clean(F, cc.rule(seeded=1), fg)
    assert same(out, [[1, 1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0], [0] * 7, [0, 1, 0, 0, 0, 0, 0], [0] * 7]) and info["survivors"] == 2
    out, changed, info = cc.expected_clean(F, cc.rule(seeded=1))   # no markers: nothing is seeded
    assert not out.any() and info["survivors"] == 0 and info["voxels_removed"] == 10
    # holes: a ring with a cavity of two, a ring whose cavity holds a background marker, a ring open to the border
    R = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1],
                  [1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 0],
                  [1, 0, 0, 1, 0, 1, 0, 1, 0, 1, 1],
                  [1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0],
                  [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    bg = np.zeros_like(R)
    bg[2, 6] = 1
    out, changed, info = cc.expected_clean(R, cc.rule(fill_holes=1), None, bg)
    want = R.copy()
    want[2, 1] = want[2, 2] = 1
    assert same(out, want) and changed.tolist() == [23, 24] and info["cavities_filled"] == 1 and info["voxels_filled"] == 2
    out, changed, info = cc.expected_clean(R, cc.rule(fill_holes=1))   # without the marker the second cavity closes too
    want[2, 6] = 1
    assert same(out, want) and info["cavities_filled"] == 2 and info["voxels_filled"] == 3 and info["voxels_changed"] == 3
    # a cavity that leaks through a corner: closed at the face neighbourhood of the background, open at the full one
    C = np.array([[0, 0, 0, 0, 0],
                  [0, 1, 1, 0, 0],
                  [0, 1, 0, 1, 0],
                  [0, 1, 1, 1, 0],
                  [0, 0, 0, 0, 0]], np.uint8)
    assert cc.expected_clean(C, cc.rule(fill_holes=1, hole_full=0))[2]["voxels_filled"] == 1
    assert cc.expected_clean(C, cc.rule(fill_holes=1, hole_full=1))[2]["voxels_filled"] == 0
    # step 2 works on the result of step 1: a speck inside a cavity is removed, then the whole cavity fills
    S = cc.shells((9, 9))
    out, changed, info = cc.expected_clean(S, cc.rule(min_size=9, fill_holes=1))
    assert info["fg_components"] == 2 and info["survivors"] == 1 and info["voxels_removed"] == 8   # the inner ring of eight goes
    assert info["cavities_filled"] == 1 and info["voxels_filled"] == 25 and out[1:-1, 1:-1].all() and not out[0].any()
    assert info["voxels_changed"] == 25 - 8


def test_shells_hold_a_cavity_in_a_cavity():
    ids, first, size, flags = cc.expected_components(cc.shells((24, 24, 24)), 0, 0)
    assert (flags & cc.FLAG_BORDER).tolist() == [4] + [0] * (size.size - 1) and size.size >= 3


# ---- symbols, classes, command line -------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decls = {
        "mgc_components": r"int mgc_components\(mgc_handle h, const uint8_t\* labels, int side, int full, int32_t\* ids, int64_t cap, int64_t\* first, int64_t\* size, "
                          r"uint8_t\* flags, int64_t\* out8\);",
        "mgc_clean_labels": r"int mgc_clean_labels\(mgc_handle h, const uint8_t\* labels, const mgc_clean_rule\* rule, uint8_t\* out, int64_t cap, int64_t\* changed_ids, "
                            r"int64_t\* out8\);",
    }
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    assert re.search(r"typedef struct \{ int32_t fg_full, seeded, fill_holes, hole_full; int64_t min_size, largest; \} mgc_clean_rule;", header)
    assert [f[0] for f in _lib.CleanRule._fields_] == ["fg_full", "seeded", "fill_holes", "hole_full", "min_size", "largest"]
    assert ctypes.sizeof(_lib.CleanRule) == 32
    for d in ("mgc_cc.h", "mgc_cc_ops.inl", "mgc_cc_driver.inl"):
        assert d in build.DEPS and os.path.exists(os.path.join(build.CSRC, d)), d
    text = open(os.path.join(build.CSRC, "mgc_cc.h")).read()
    # the steps stay plain C++: a stand-alone program includes them
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text
    # behind every kernel that was there before it: at the end of the kernel file behind the driver of the label histograms, and nothing
    # in front includes it
    import driver_chain
    driver_chain.assert_behind_everything_before_it("mgc_cc_driver.inl", "mgc_cc")


def test_classes_and_value_errors_without_a_library():
    from medpy_amd.graphcut import Components, graph
    assert Components._fields == ("ids", "first", "size", "flags", "info")
    for cls in (graph.SparseGraph, graph.RegionGraph):
        g = object.__new__(cls)
        for name in ("components", "clean_labels", "clean_info"):
            with pytest.raises(NotImplementedError, match="voxel lattice"):
                getattr(g, name)()
    for name in ("components", "clean_labels", "clean_info"):
        assert hasattr(graph.EmbeddedLatticeGraph, name) and hasattr(graph.VoxelGraph, name)
    # the arguments are checked before the library is asked (_h is None: a call would fail loudly)
    g = object.__new__(graph.VoxelGraph)
    g._h = None
    g._shape = (2, 3)
    g._clean_info = None
    g._full_neighbourhood = False
    ok = np.zeros((2, 3), bool)
    for bad in (np.zeros((3, 2), bool), np.zeros((2, 3), np.float32), [[0, 1, 0], [1, 0, 0]]):
        with pytest.raises(ValueError, match="labels must be"):
            g.components(bad)
        with pytest.raises(ValueError, match="labels must be"):
            g.clean_labels(bad)
    for kw in ({"connectivity": "edge"}, {"connectivity": 6}):
        with pytest.raises(ValueError, match="connectivity"):
            g.components(ok, **kw)
        with pytest.raises(ValueError, match="connectivity"):
            g.clean_labels(ok, **kw)
    for kw in ({"min_size": 0}, {"min_size": 1.5}, {"largest": -1}, {"largest": True}, {"hole_connectivity": "all"}, {"out": np.zeros((2, 3), np.uint8)},
               {"out": np.zeros((3, 2), bool)}):
        with pytest.raises(ValueError):
            g.clean_labels(ok, **kw)
    assert g.clean_info() == {k: 0 for k in cc.CLEAN_KEYS}


def test_cli_flags_parse():
    from medpy_amd.cli import graphcut_voxel
    p = graphcut_voxel.getParser()
    base = ["1.0", "img.nii", "markers.nii", "out.nii"]
    a = p.parse_args(base)
    assert (a.keep_seeded, a.keep_largest, a.min_size, a.fill_holes) == (False, None, None, False)
    assert graphcut_voxel.clean_rule(a) is None                       # without the flags the script does what it always did
    a = p.parse_args(base + ["--keep-seeded", "--keep-largest", "2", "--min-size", "30", "--fill-holes"])
    assert (a.keep_seeded, a.keep_largest, a.min_size, a.fill_holes) == (True, 2, 30, True)
    assert graphcut_voxel.clean_rule(a) == dict(seeded=True, largest=2, min_size=30, fill_holes=True)
    assert graphcut_voxel.clean_rule(p.parse_args(base + ["--min-size", "4"])) == dict(seeded=False, largest=None, min_size=4, fill_holes=False)
    for bad in (["--keep-largest", "0"], ["--min-size", "0"], ["--keep-largest", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)

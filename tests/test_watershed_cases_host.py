"""CPU tier of the seeded watershed: the NumPy / heap statement of the definition against Meyer's flood and against what
must hold of any watershed; the lines the kernels compile (medpy_amd/csrc/mgc_ws.h) as a stand-alone host program
(tests/hostsim/ws_main.cpp), plain and under ASan / UBSan, against the statement with ==; two doctored builds of that program
rejected where named; the minimum filter against the reference's recorded output (tests/golden/watershed.npz)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

import watershed_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "watershed.npz")
REFERENCE_ROOT = "/root/reference"
CXX = ["g++", "-std=c++17"]


def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """ws_main.cpp compiled plainly, once more under the sanitizers (both run every case), and the two doctored builds"""
    tmp = tmp_path_factory.mktemp("ws")
    src = os.path.join(HERE, "hostsim", "ws_main.cpp")
    exes = [str(tmp / "ws_main")]
    subprocess.check_call(CXX + ["-O2", "-o", exes[0], src])
    flags = _sanitizer_flags(tmp)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    if flags:
        exes.append(str(tmp / "ws_main_san"))
        subprocess.check_call(CXX + ["-O1", "-g"] + flags + ["-o", exes[1], src])
    doctored = {}
    for name in ("WS_NO_RISE_RESET", "WS_NO_SELF_WAKE"):
        doctored[name] = str(tmp / name.lower())
        subprocess.check_call(CXX + ["-O2", "-D%s" % name, "-o", doctored[name], src])
    return tmp, exes, doctored


def _shape3(shape):
    return (1,) * (3 - len(shape)) + tuple(shape)


def run_program(exe, tmp, case, order=1):
    """(T, parents, labels, info) of the host program for one case"""
    c = case
    c.image.tofile(str(tmp / "image.bin"))
    c.markers.tofile(str(tmp / "markers.bin"))
    mask = "-"
    if c.mask is not None:
        mask = str(tmp / "mask.bin")
        c.mask.tofile(mask)
    out = subprocess.run([exe] + [str(n) for n in _shape3(c.image.shape)] + [str(wc.DTYPE_ID[c.image.dtype.name]), str(order), str(tmp / "image.bin"), str(tmp / "markers.bin"), mask,
                                                                            str(tmp / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    raw = open(str(tmp / "out.bin"), "rb").read()
    n = c.image.size
    assert len(raw) == n * 16 + 64
    T = np.frombuffer(raw, np.uint64, n, 0).reshape(c.image.shape)
    parent = np.frombuffer(raw, np.uint32, n, 8 * n).reshape(c.image.shape)
    labels = np.frombuffer(raw, np.int32, n, 12 * n).reshape(c.image.shape)
    info = np.frombuffer(raw, np.int64, 8, 16 * n)
    return T, parent, labels, info


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    names = set(wc.NAMES)
    for axis in range(3):
        for e in (1, 2, 7, 8, 9, 17):
            assert wc.BY_NAME["extent_a%d_%d" % (axis, e)].image.shape[axis] == e
    assert {len(c.image.shape) for c in wc.CASES} == {1, 2, 3}
    assert {c.image.dtype.name for c in wc.CASES} == set(wc.DTYPES)
    assert wc.CORRIDOR[0] > 2 * wc.SWEEP_CAP
    assert wc.BY_NAME["markers_above_255"].markers.max() == 300 and wc.BY_NAME["markers_above_255_perm"].markers.max() == 2 ** 31 - 1
    assert wc.BY_NAME["uint32_above_2_31"].image.min() < 2 ** 31 < wc.BY_NAME["uint32_above_2_31"].image.max()
    z = wc.BY_NAME["float32_signed_zeros"].image
    assert np.signbit(z).any() and not np.signbit(z).all() and (z == 0).all()
    for dt in ("int8", "int16", "int32"):
        im = wc.BY_NAME["extremes_" + dt].image
        assert im.min() == np.iinfo(dt).min and im.max() == np.iinfo(dt).max
    assert any(c.distinct for c in wc.CASES) and any(not c.distinct for c in wc.CASES)
    for c in wc.CASES:
        if c.distinct:
            assert np.unique(c.image).size == c.image.size, c.name
    assert max(c.image.size for c in wc.CASES) == 40 * 40 * 72
    assert set(wc.RISE_RESET_FAILS + wc.RISE_RESET_PASSES + wc.SELF_WAKE_FAILS + wc.SELF_WAKE_PASSES) <= names
    text = open(os.path.join(ROOT, "medpy_amd", "csrc", "mgc_ws.h")).read()
    assert int(re.search(r"#define MGC_WS_SWEEP_CAP (\d+)", text).group(1)) == wc.SWEEP_CAP
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text   # plain C++: a stand-alone program includes it


def test_keys_keep_the_order_of_the_values():
    for dt in wc.DTYPES[:-1]:
        info = np.iinfo(dt)
        v = np.array(sorted({info.min, info.min + 1, -1 if info.min < 0 else 0, 0, 1, info.max - 1, info.max}), dtype=dt)
        k = wc.keys_of(v)
        assert (np.diff(k.astype(np.int64)) > 0).all() and k.max() < 2 ** 32, dt
    v = np.array([-3e38, -1.5, -1.17549435e-38, -1e-40, -1e-45, 0.0, 1e-45, 1e-40, 1.17549435e-38, 1.5, 3e38], np.float32)
    k = wc.keys_of(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert wc.keys_of(np.array([-0.0], np.float32))[0] == wc.keys_of(np.array([0.0], np.float32))[0]


@pytest.mark.parametrize("name", [c.name for c in wc.CASES if c.distinct])
def test_statement_is_meyers_flood_where_no_two_values_are_equal(name):
    c = wc.BY_NAME[name]
    assert np.array_equal(wc.solved(name)[2], wc.meyer_flood(c.image, c.markers, c.mask))


@pytest.mark.parametrize("name", wc.NAMES)
def test_statement_regions_are_connected_and_everything_a_seed_reaches_is_labelled(name):
    c = wc.BY_NAME[name]
    T, parent, labels = wc.solved(name)
    inside = np.ones(c.image.shape, bool) if c.mask is None else c.mask != 0
    seeds = inside & (c.markers > 0)
    assert np.array_equal(labels[seeds], c.markers[seeds])
    assert (labels[~inside] == 0).all()
    # every voxel of a component of the mask that holds a seed is labelled, no other is
    comp, n = ndi.label(inside)
    seeded = np.zeros(n + 1, bool)
    seeded[np.unique(comp[seeds])] = True
    seeded[0] = False
    assert np.array_equal(labels != 0, seeded[comp])
    assert np.array_equal(T != wc.INF, labels != 0) and np.array_equal(parent != wc.NONE, labels != 0)
    # a region is connected to one of its seeds: every component of a label holds a seed of that label
    for lab in np.unique(labels[labels != 0]):
        regions, k = ndi.label(labels == lab)
        assert set(np.unique(regions[seeds & (c.markers == lab)])) == set(range(1, k + 1)), lab
    # H is the minimax height: never below the voxel's own key
    keys = wc.keys_of(c.image)
    reached = T != wc.INF
    assert ((T[reached] >> np.uint64(32)) >= keys[reached]).all()


def test_hand_answers():
    assert wc.solved("ridge_left_lower")[2].tolist() == [1, 1, 1, 2, 2]
    assert wc.solved("ridge_right_lower")[2].tolist() == [1, 1, 2, 2, 2]
    assert wc.solved("ridge_level")[2].tolist() == [1, 1, 1, 2, 2]          # a tie: the lower index
    assert wc.solved("meet_on_face_16")[2].ravel().tolist() == [1] * 8 + [2] * 8
    assert wc.solved("meet_on_face_17")[2].ravel().tolist() == [1] * 9 + [2] * 8
    T = wc.solved("plateau_one_seed")[0]
    z, y, x = np.indices(T.shape)
    k = int(wc.keys_of(np.array([9], np.int16))[0])
    assert np.array_equal(T, (np.uint64(k) << np.uint64(32)) + (abs(z - 1) + abs(y - 2) + x).astype(np.uint64))
    lab = wc.solved("mask_cuts_a_region_off")[2]
    assert (lab[:, :, :6] == 1).all() and (lab[:, :, 6:] == 0).all()
    assert np.array_equal(wc.solved("seed_outside_the_mask")[2], lab)
    assert not wc.solved("no_seeds")[2].any() and not wc.solved("mask_all_zero")[2].any()
    assert (wc.solved("one_seed")[2] == 1).all()
    c = wc.BY_NAME["every_voxel_a_seed"]
    assert np.array_equal(wc.solved(c.name)[2], c.markers)
    T = wc.solved("corridor_winds_in_one_tile")[0]
    assert int((T[T != wc.INF] & np.uint64(0xFFFFFFFF)).max()) == wc.CORRIDOR[0] - 1


@pytest.mark.parametrize("name", wc.NAMES)
def test_host_program_equals_the_statement(programs, name):
    tmp, exes, _ = programs
    c = wc.BY_NAME[name]
    T, parent, labels = wc.solved(name)
    for exe in exes:
        for order in ((1, 2) if c.image.size < 20000 else (1,)):
            got = run_program(exe, tmp, c, order)
            assert np.array_equal(got[0], T) and np.array_equal(got[1], parent) and np.array_equal(got[2], labels), (exe, order)
            info = got[3]
            assert info[0] == int(((c.markers > 0) & (True if c.mask is None else c.mask != 0)).sum())
            assert info[5] == int((labels != 0).sum()) and info[6] <= 33 and info[7] == 0
            assert (info[1] == 0) == (info[0] == 0) and info[2] >= info[1] and info[3] >= info[2]
    if name in wc.SELF_WAKE_FAILS:
        assert info[4] > 0       # the visit did end at the cap
    if name in wc.SELF_WAKE_PASSES:
        assert info[4] == 0


@pytest.mark.parametrize("doctor,fails,passes", [("WS_NO_RISE_RESET", wc.RISE_RESET_FAILS, wc.RISE_RESET_PASSES), ("WS_NO_SELF_WAKE", wc.SELF_WAKE_FAILS, wc.SELF_WAKE_PASSES)])
def test_doctored_builds_are_rejected_where_named(programs, doctor, fails, passes):
    tmp, _, doctored = programs
    for name in fails:
        got = run_program(doctored[doctor], tmp, wc.BY_NAME[name])
        assert not np.array_equal(got[0], wc.solved(name)[0]), name
    for name in passes:
        got = run_program(doctored[doctor], tmp, wc.BY_NAME[name])
        assert np.array_equal(got[0], wc.solved(name)[0]) and np.array_equal(got[2], wc.solved(name)[2]), name


# ---- the minimum filter ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_file_holds_every_case_and_nothing_else(golden):
    assert set(golden.files) == {n + s for n in wc.MIN_NAMES for s in ("/indices", "/values")}
    assert os.path.getsize(GOLDEN) < (1 << 20)
    sizes = {c.size for c in wc.MIN_CASES}
    assert sizes == {1, 2, 3, 4, 5}
    assert any(c.size > min(c.image.shape) for c in wc.MIN_CASES) and any(c.size >= 2 * max(c.image.shape) for c in wc.MIN_CASES)
    assert {c.image.dtype.name for c in wc.MIN_CASES} == set(wc.DTYPE_ID)


@pytest.mark.parametrize("name", wc.MIN_NAMES)
def test_minimum_filter_statement_equals_the_reference(golden, name):
    c = wc.MIN_BY_NAME[name]
    want = wc.golden_mask(golden, name)
    assert np.array_equal(wc.minima_statement(c.image, c.size), want)
    assert np.array_equal(c.image == ndi.minimum_filter(c.image, size=c.size), want)
    idx, val = wc.local_minima_statement(c.image, c.size)
    gi, gv = golden[name + "/indices"], golden[name + "/values"]
    assert np.array_equal(val, gv) and val.dtype == gv.dtype and idx.shape == gi.shape
    # the reference's argsort is not stable: per value the index SETS are equal
    for v in np.unique(val):
        assert set(map(tuple, idx[val == v])) == set(map(tuple, gi[gv == v]))


@pytest.mark.parametrize("name", [c.name for c in wc.MIN_CASES if c.image.dtype.name in wc.DTYPES])
def test_host_program_minima_equal_the_reference(programs, golden, name):
    tmp, exes, _ = programs
    c = wc.MIN_BY_NAME[name]
    c.image.tofile(str(tmp / "image.bin"))
    for exe in exes:
        out = subprocess.run([exe, "minima"] + [str(n) for n in _shape3(c.image.shape)] + [str(wc.DTYPE_ID[c.image.dtype.name]), str(c.size), str(tmp / "image.bin"),
                                                                                           str(tmp / "out.bin")], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
        got = np.fromfile(str(tmp / "out.bin"), np.uint8).reshape(c.image.shape)
        assert np.array_equal(got != 0, wc.golden_mask(golden, name)), exe


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE_ROOT, "medpy", "filter")), reason="needs a checkout of the reference")
def test_golden_file_is_what_the_generator_writes(tmp_path, golden):
    out = tmp_path / "watershed.npz"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_watershed_golden.py"), "--reference", REFERENCE_ROOT, "--out", str(out)])
    z = np.load(str(out))
    assert set(z.files) == set(golden.files)
    for k in z.files:
        if k.endswith("/values"):
            assert np.array_equal(z[k], golden[k]) and z[k].dtype == golden[k].dtype, k


# ---- the library's side, without a device ---------------------------------------------------------------------------------------
def test_entry_points_are_declared_loaded_and_in_their_place():
    from medpy_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    decls = {
        "mgc_watershed_image": r"int mgc_watershed_image\(int device, int ndim, const int64_t\* shape, const void\* image, int dtype, const int32_t\* markers, const uint8_t\* mask, "
                               r"int32_t\* labels_out, int64_t\* out8\);",
        "mgc_local_minima_image": r"int mgc_local_minima_image\(int device, int ndim, const int64_t\* shape, const void\* image, int dtype, int size, uint8_t\* mask_out, int64_t\* out4\);",
    }
    lib = _lib.load()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    for d in ("mgc_ws.h", "mgc_ws_ops.inl", "mgc_ws_driver.inl"):
        assert d in build.DEPS and os.path.exists(os.path.join(build.CSRC, d)), d
    # the kernels come in behind the diffusion's and in front of the six drivers that end the kernel file, once
    kernels = open(os.path.join(build.CSRC, "mgc_kernels.hip")).read()
    inc = '#include "mgc_ws_driver.inl"'
    assert kernels.count(inc) == 1 and kernels.count('"mgc_ws_') == 1
    assert kernels.index('#include "mgc_diffuse_driver.inl"') < kernels.index(inc) < kernels.index('#include "mgc_reach_driver.inl"')
    from driver_chain import DRIVERS
    for d in DRIVERS + ["mgc_diffuse_driver.inl"]:
        assert "mgc_ws" not in open(os.path.join(build.CSRC, d)).read(), d


def test_python_layer_refuses_before_the_library_is_asked():
    from medpy_amd import filter as flt
    from medpy_amd.filter import image as ws
    assert flt.watershed is ws.watershed and flt.local_minima is ws.local_minima and flt.minima_markers is ws.minima_markers
    img = np.zeros((3, 4), np.uint8)
    mk = np.zeros((3, 4), np.int32)
    with pytest.raises(NotImplementedError, match="4-D"):
        ws.watershed(np.zeros((2, 2, 2, 2)), np.zeros((2, 2, 2, 2), np.int32))
    with pytest.raises(ValueError, match="shape"):
        ws.watershed(img, np.zeros((4, 3), np.int32))
    with pytest.raises(ValueError, match="shape"):
        ws.watershed(img, mk, mask=np.ones((4, 3), bool))
    with pytest.raises(ValueError, match="negative"):
        ws.watershed(img, mk - 1)
    with pytest.raises(ValueError, match="integer"):
        ws.watershed(img, mk.astype(np.float32))
    with pytest.raises(ValueError, match="int32"):
        ws.watershed(img, mk.astype(np.int64) + 2 ** 31)
    with pytest.raises(ValueError, match="finite"):
        ws.watershed(np.full((3, 4), np.nan, np.float32), mk)
    with pytest.raises(ValueError, match="finite"):
        ws.local_minima(np.full((3, 4), np.inf), 2)
    with pytest.raises(ValueError, match="empty"):
        ws.watershed(np.zeros((0, 4)), np.zeros((0, 4), np.int32))
    for bad in (0, -1, 1.5, "two"):
        with pytest.raises(ValueError, match="min_distance"):
            ws.local_minima(img, bad)
    # the ranks of a 64-bit image keep its order and its ties
    a = np.array([[2 ** 40, -5, 7], [7, 2 ** 40, -(2 ** 62)]], np.int64)
    r = ws.orderable(a)
    assert r.dtype == np.uint32 and np.array_equal(r, [[3, 1, 2], [2, 3, 0]])
    f = np.array([-0.0, 0.0, -1e-300, 1e-300], np.float64)
    assert ws.orderable(f).tolist() == [1, 1, 0, 2]
    assert ws.orderable(img) is img

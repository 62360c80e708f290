"""CPU tier of the anisotropic diffusion: the statement of diffusion_cases.py against the reference's recorded output
(tests/golden/diffusion.npz) with ``==`` for options 2 and 3 and inside the measured bound for option 1, the lines of mgc_diffuse.h
as a stand-alone host program that walks the volume brick by brick (plain, and under the sanitizers where this machine has the
runtimes) against the same file, two doctored builds that named cases must reject and no case that cannot see the fault may, and
the agreement of header, symbol table, library and Python layer."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import diffusion_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = ["g++", "-std=c++17", "-ffp-contract=off"]
DTYPE_ID = {"uint8": 0, "int8": 1, "uint16": 2, "int16": 3, "uint32": 4, "int32": 5, "uint64": 6, "int64": 7, "float32": 8, "float64": 9}


def _bricks(shape):
    s3 = (1,) * (3 - len(shape)) + tuple(shape)
    return -(-s3[0] // dc.BZ) * -(-s3[1] // dc.BY) * -(-s3[2] // dc.BX)


# ---- the statement and the golden file -----------------------------------------------------------------------------------------
def test_the_cases_cover_what_they_must():
    shapes = {c.shape for c in dc.CASES}
    for s in ((1, 1, 1), (1, 1, 5), (3, 1, 4)):
        assert s in shapes
    for axis, b in ((0, dc.BZ), (1, dc.BY), (2, dc.BX)):
        for n in (1, 2, b - 1, b, b + 1):
            assert any(len(s) == 3 and s[axis] == n for s in shapes), (axis, n)
    assert any(len(s) == 3 and s[2] == 2 * dc.BX + 3 for s in shapes)
    assert {len(s) for s in shapes} == {1, 2, 3}
    assert any(s[-1] % 4 for s in shapes) and any(s[-1] % 4 == 0 and s[-1] > dc.BX for s in shapes)
    for option in (1, 2, 3):
        mine = [c for c in dc.CASES if c.option == option]
        assert {c.niter for c in mine} == set(dc.NITERS) and {c.dtype for c in mine} == set(dc.DTYPES)
        assert {c.pattern for c in mine} >= {"noise", "constant"}
        for axis in range(3):   # non-unit spacing on each axis in turn
            assert any(c.spacing and len(c.spacing) == 3 and c.spacing[axis] != 1 and all(v == 1 for k, v in enumerate(c.spacing) if k != axis) for c in mine)
    assert {c.pattern for c in dc.CASES if c.option == 3} >= {"step0", "step1", "step2", "noisy_step0", "noisy_step1", "noisy_step2", "ramp"}
    small = [c for c in dc.CASES if int(np.prod(c.shape)) <= 1500]
    assert len(small) > 0.8 * len(dc.CASES)
    assert os.path.getsize(dc.GOLDEN) < 400 * 1024
    assert set(np.load(dc.GOLDEN).files) == set(dc.NAMES)
    f64 = dc.image(next(c for c in dc.CASES if c.dtype == "float64"))
    assert (f64.astype(np.float32).astype(np.float64) != f64).any()   # values float32 cannot hold


@pytest.mark.parametrize("name", dc.NAMES)
def test_statement_equals_the_reference(name):
    case = dc.BY_NAME[name]
    got = dc.statement(dc.image(case), case.niter, case.kappa, case.gamma, case.spacing, case.option)
    gold = dc.golden(name)
    assert got.dtype == np.float32 and got.shape == gold.shape
    if case.option == 1:   # the statement's own exp against NumPy's float32 exp: what E1_MEASURED measures
        assert dc.error_measure(got, gold) <= dc.E1_MEASURED, dc.error_measure(got, gold)
    else:
        assert np.array_equal(got, gold), int((got != gold).sum())


def test_patterns_behave_as_they_should():
    for c in dc.CASES:
        gold, img = dc.golden(c.name), dc.image(c)
        if c.pattern == "constant" or c.pattern.startswith("step") or c.pattern == "ramp" or c.niter == 0:
            assert np.array_equal(gold, np.array(img, dtype=np.float32)), c.name   # unchanged: no flux anywhere
        if c.pattern.startswith("noisy_step"):
            axis = int(c.pattern[-1])
            low = np.indices(c.shape)[axis] < c.shape[axis] // 2
            assert gold[low].max() < 20 and gold[~low].min() > 190, c.name   # the two sides did not mix
            assert not np.array_equal(gold, img.astype(np.float32))          # ... and each side did diffuse
    ks = np.float32(dc.KAPPA_RAMP * 2 ** 0.5)
    ramp = dc.image(next(c for c in dc.CASES if c.pattern == "ramp" and len(c.shape) == 3))
    for axis in range(3):
        assert (np.abs(np.diff(ramp.astype(np.float32), axis=axis)) == ks).all()   # |d| equals kappa_s exactly


def test_e1_measured_is_the_committed_measurement():
    rows = [json.loads(ln) for ln in open(os.path.join(ROOT, "profiles", "diffusion.jsonl")) if ln.strip()]
    mine = {r["case"]: r["e"] for r in rows if r.get("kind") == "e1_statement_vs_golden"}
    assert set(mine) == {c.name for c in dc.CASES if c.option == 1}
    assert dc.E1_MEASURED == max(mine.values()) and 0 < dc.E1_MEASURED < 1e-6
    assert dc.E1_BOUND == 8 * dc.E1_MEASURED
    top = [r for r in rows if r.get("kind") == "e1_statement_vs_golden_max"]
    assert len(top) == 1 and top[0]["E1_MEASURED"] == dc.E1_MEASURED


@pytest.mark.needs_reference
def test_the_generator_reproduces_the_committed_file(tmp_path):
    from oracle.overlay import REF as REFERENCE_ROOT
    out = tmp_path / "diffusion.npz"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_diffusion_golden.py"), "--reference", REFERENCE_ROOT, "--out", str(out)])
    z = np.load(str(out))
    assert set(z.files) == set(dc.NAMES)
    for name in dc.NAMES:
        assert z[name].tobytes() == dc.golden(name).tobytes() and z[name].dtype == np.float32, name


# ---- the host program ----------------------------------------------------------------------------------------------------------
def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """diffusion_main.cpp compiled plainly, once more under the sanitizers (both run every case), and the two doctored builds"""
    tmp = tmp_path_factory.mktemp("diffusion")
    src = os.path.join(HERE, "hostsim", "diffusion_main.cpp")
    exes = [str(tmp / "ad_plain")]
    subprocess.check_call(CXX + ["-O2", "-o", exes[0], src])
    flags = _sanitizer_flags(tmp)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    if flags:
        exes.append(str(tmp / "ad_san"))
        subprocess.check_call(CXX + ["-O1", "-g"] + flags + ["-o", exes[1], src])
    doctored = {}
    for name in ("AD_CLAMP_AT_BRICK_BORDER", "AD_SUM_X_FIRST"):
        doctored[name] = str(tmp / name.lower())
        subprocess.check_call(CXX + ["-O2", "-D%s" % name, "-o", doctored[name], src])
    return tmp, exes, doctored


def _run(tmp, exe, case):
    img = np.ascontiguousarray(dc.image(case))
    nd = len(case.shape)
    img.tofile(str(tmp / "in.bin"))
    args = [str(n) for n in (1,) * (3 - nd) + case.shape] + [str(nd), str(DTYPE_ID[case.dtype]), str(case.niter), repr(case.kappa), repr(case.gamma)]
    args += [repr(float(s)) for s in (case.spacing or (1.0,) * nd)] + [str(case.option), str(tmp / "in.bin"), str(tmp / "out.bin")]
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    return np.fromfile(str(tmp / "out.bin"), dtype=np.float32).reshape(case.shape)


@pytest.mark.parametrize("name", dc.NAMES)
def test_host_program_equals_the_reference(programs, name):
    tmp, exes, _ = programs
    case = dc.BY_NAME[name]
    for exe in exes:
        dc.check(_run(tmp, exe, case), case, os.path.basename(exe))


def _accepted(got, case):
    try:
        dc.check(got, case)
        return True
    except AssertionError:
        return False


def _rejected(tmp, exe):
    return {c.name for c in dc.CASES if not _accepted(_run(tmp, exe, c), c)}


# a border between two bricks along z, along y, along x, in 3-D, 2-D and 1-D, every option
CLAMP_NAMED = ["9x9x65-int16-noise-n2-k50-g0.1-o1", "9x9x65-uint16-noise-n8-k20.5-g0.25-o2", "9x9x65-float32-noise-n1-k7.25-g0.05-o3"]
CLAMP_NAMED += ["9x65-uint16-noise-n1-k20.5-g0.25-o%d" % o for o in (1, 2, 3)] + ["2x9x68-float32-noise-n2-k50-g0.1-o%d" % o for o in (1, 2, 3)]
CLAMP_NAMED += ["9x3x5-uint8-noise-n2-k50-g0.1-o%d" % o for o in (1, 2, 3)]
CLAMP_NAMED += ["2x9x5-uint16-noise-n5-k7.25-g0.05-o1", "2x3x65-uint16-noise-n8-k50-g0.1-o2", "131-int16-noise-n5-k50-g0.1-o2", "131-uint8-noise-n1-k7.25-g0.05-o1"]
# three terms that are all non-zero, options 2 and 3 (a fault of the last bit: inside any bound option 1 could be given, see below)
SUM_NAMED = ["9x9x65-uint16-noise-n8-k20.5-g0.25-o2", "3x9x70-uint8-noise-n5-k20.5-g0.25-o3"]
SUM_NAMED += ["2x9x68-float32-noise-n%d-k50-g0.1-o%d" % (n, o) for n in (1, 2, 5, 8) for o in (2, 3)] + ["9x3x5-float32-noise-n2-k50-g0.1-o%d" % o for o in (2, 3)]


def test_a_halo_clamped_at_the_brick_border_is_rejected(programs):
    tmp, _, doctored = programs
    bad = _rejected(tmp, doctored["AD_CLAMP_AT_BRICK_BORDER"])
    assert {dc.BY_NAME[n].option for n in CLAMP_NAMED} == {1, 2, 3}
    assert set(CLAMP_NAMED) <= bad, sorted(set(CLAMP_NAMED) - bad)
    # one brick, or no iteration: the halo lies outside the volume or is never read; such a case cannot see the fault and passes
    for name in bad:
        assert _bricks(dc.BY_NAME[name].shape) > 1 and dc.BY_NAME[name].niter >= 1, name
    assert any(_bricks(c.shape) == 1 and c.niter >= 1 and c.pattern == "noise" for c in dc.CASES)
    # the bound of option 1 discriminates: the named option-1 cases are beyond it by orders of magnitude, not merely unequal
    for name in CLAMP_NAMED:
        case = dc.BY_NAME[name]
        if case.option == 1:
            e = dc.error_measure(_run(tmp, doctored["AD_CLAMP_AT_BRICK_BORDER"], case), dc.golden(name))
            print(name, e, dc.E1_BOUND)
            assert e > 100 * dc.E1_BOUND, (name, e)


def test_axes_added_last_to_first_are_rejected_in_three_dimensions_only(programs):
    tmp, _, doctored = programs
    bad = _rejected(tmp, doctored["AD_SUM_X_FIRST"])
    assert {dc.BY_NAME[n].option for n in SUM_NAMED} == {2, 3}
    assert set(SUM_NAMED) <= bad, sorted(set(SUM_NAMED) - bad)
    # float32 addition commutes: with two terms or one the order cannot matter, nor where an axis of extent 1 adds zero.  And the
    # order of a sum is a fault of the last bit: only == sees it, so no option-1 case can be named for this build (its bound is there
    # because option 1's exp is not the reference's to the last bit)
    for name in bad:
        case = dc.BY_NAME[name]
        assert len(case.shape) == 3 and min(case.shape) >= 2 and case.niter >= 1 and case.option != 1, name


# ---- symbols, classes, argument checks -----------------------------------------------------------------------------------------
def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decls = {
        "mgc_diffuse_image": r"int mgc_diffuse_image\(int device, int ndim, const int64_t\* shape, const void\* image, int dtype, int niter, double kappa, double gamma, "
                             r"const double\* spacing, int option,\s+float\* out, int64_t\* out4\);",
        "mgc_diffuse": r"int mgc_diffuse\(mgc_handle h, int niter, double kappa, double gamma, const double\* spacing, int option, int keep, float\* out, int64_t\* out4\);",
    }
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    for d in ("mgc_diffuse.h", "mgc_diffuse_ops.inl", "mgc_diffuse_driver.inl"):
        assert d in build.DEPS and os.path.exists(os.path.join(build.CSRC, d)), d
    text = open(os.path.join(build.CSRC, "mgc_diffuse.h")).read()
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text   # plain C++: a stand-alone program includes it
    for name, want in (("BZ", dc.BZ), ("BY", dc.BY), ("BX", dc.BX)):
        assert int(re.search(r"#define MGC_AD_%s (\d+)" % name, text).group(1)) == want
    assert dc.BX % 64 == 0 and "-ffp-contract=off" in build.FLAGS and "-ffast-math" not in build.FLAGS
    code = text + open(os.path.join(build.CSRC, "mgc_diffuse_ops.inl")).read()
    for word in ("__fdividef", "__frcp", "__expf", "__frsqrt"):
        assert word not in code, word
    # the kernels come in behind the last function of the kernel file, once
    kernels = open(os.path.join(build.CSRC, "mgc_kernels.hip")).read()
    assert kernels.count('#include "mgc_diffuse_driver.inl"') == 1 and kernels.index('#include "mgc_diffuse_driver.inl"') > kernels.index("int mgc_get_stats(")


def test_classes_and_value_errors_without_a_library():
    from medpy_amd import filter as flt
    from medpy_amd.filter import smoothing
    from medpy_amd.graphcut import graph
    assert flt.anisotropic_diffusion is smoothing.anisotropic_diffusion
    for cls in (graph.SparseGraph, graph.RegionGraph):
        g = object.__new__(cls)
        for name in ("anisotropic_diffusion", "diffusion_info"):
            with pytest.raises(NotImplementedError, match="voxel lattice"):
                getattr(g, name)()
    for name in ("anisotropic_diffusion", "diffusion_info"):
        assert hasattr(graph.EmbeddedLatticeGraph, name) and hasattr(graph.VoxelGraph, name)
    img = np.zeros((2, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="4-D"):
        smoothing.anisotropic_diffusion(np.zeros((2, 2, 2, 2)))
    # the arguments are checked before the library is asked (_h is None: a call would fail loudly)
    g = object.__new__(graph.VoxelGraph)
    g._h = None
    g._shape = (2, 3)
    bad = ({"niter": -1}, {"niter": 1.5}, {"niter": "two"}, {"option": 0}, {"option": 4}, {"option": 2.5}, {"kappa": 0}, {"kappa": -3.0}, {"kappa": np.inf}, {"kappa": np.nan},
           {"kappa": "k"}, {"gamma": np.nan}, {"gamma": np.inf}, {"voxelspacing": (1.0,)}, {"voxelspacing": (1.0, 0.0)}, {"voxelspacing": (1.0, -1.0)},
           {"voxelspacing": (np.inf, 1.0)}, {"voxelspacing": (np.nan, 1.0)}, {"voxelspacing": (1.0, 1.0, 1.0)}, {"voxelspacing": 2.0})
    for kw in bad:
        with pytest.raises(ValueError):
            smoothing.anisotropic_diffusion(img, **kw)
        args = dict(niter=1, kappa=50, gamma=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            g.anisotropic_diffusion(**args)
    with pytest.raises(ValueError, match="download=False needs keep=True"):
        g.anisotropic_diffusion(1, 50, 0.1, download=False)
    with pytest.raises(ValueError, match="no graph was given"):
        smoothing.anisotropic_diffusion(None)
    with pytest.raises(ValueError, match="shape"):
        smoothing.anisotropic_diffusion(np.zeros((3, 2)), graph=g)
    with pytest.raises(ValueError, match="empty"):
        smoothing.anisotropic_diffusion(np.zeros((0, 3)))
    assert g.diffusion_info() == {"iterations": 0, "bricks": 0}

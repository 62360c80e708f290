"""CPU tier of the histogram regional term: the NumPy definition (histogram_binning / histogram_bins /
histogram_tables), the rule of mgc_binned.h as a stand-alone host program against that definition, the plug-in on a facade that
merges on the host, and the agreement of header, symbol table and library on the new calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DTYPES = {"u8": np.uint8, "i8": np.int8, "u16": np.uint16, "i16": np.int16, "u32": np.uint32, "i32": np.int32, "u64": np.uint64, "i64": np.int64,
          "f32": np.float32, "f64": np.float64}


def _hist():
    from medpy_amd.graphcut import histogram
    return histogram


# ---- the NumPy definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_binning_and_bins_of_every_dtype(name):
    h = _hist()
    dtype = np.dtype(DTYPES[name])
    rng = np.random.default_rng(3)
    if dtype.kind == "f":
        img = rng.uniform(-3.0, 9.0, (5, 6, 7)).astype(dtype)
        with pytest.raises(ValueError):
            h.histogram_binning(img)   # bins=None needs an integer image
    else:
        lo_v = -40 if dtype.kind == "i" else 3
        img = rng.integers(lo_v, lo_v + 100, (5, 6, 7)).astype(dtype)
        nbins, lo, width = h.histogram_binning(img)
        assert (nbins, lo, width) == (int(img.max()) - int(img.min()) + 1, float(img.min()), 1.0)
        b = h.histogram_bins(img, nbins, lo, width)
        assert b.dtype == np.int64 and b.shape == img.shape
        np.testing.assert_array_equal(b, img.astype(np.int64) - int(img.min()))   # one bin per value
    for bins in (1, 7, 16, 65536):
        nbins, lo, width = h.histogram_binning(img, bins)
        assert nbins == bins and lo == float(img.min()) and width == (float(img.max()) - float(img.min())) / bins
        b = h.histogram_bins(img, nbins, lo, width)
        assert b.min() == 0 and b.max() == bins - 1                      # the maximum lands in the last bin (by the clamp)
        assert b[np.unravel_index(np.argmax(img), img.shape)] == bins - 1
        x = np.floor((img.astype(np.float64) - lo) / width)
        np.testing.assert_array_equal(b, np.clip(x, 0, bins - 1).astype(np.int64))


def test_values_on_bin_borders_and_outside_the_range():
    h = _hist()
    v = np.array([0.0, 0.25, 0.5, 0.75, 1.0, np.nextafter(0.5, 0), np.nextafter(0.5, 1), -0.0, -1e-300, -5.0, 1.25, 1e300])
    b = h.histogram_bins(v, 4, 0.0, 0.25)
    assert b.tolist() == [0, 1, 2, 3, 3, 1, 2, 0, 0, 0, 3, 3]   # a border belongs to the bin above it; outside: clamped
    # an integer image binned coarsely: borders at multiples of the width
    img = np.arange(0, 21, dtype=np.uint8)
    nbins, lo, width = h.histogram_binning(img, 4)
    assert (nbins, lo, width) == (4, 0.0, 5.0)
    assert h.histogram_bins(img, nbins, lo, width).tolist() == [0] * 5 + [1] * 5 + [2] * 5 + [3] * 6


def test_constant_image_and_extreme_bin_counts():
    h = _hist()
    for img in (np.full((3, 4), 7, np.int16), np.full((3, 4), 2.5, np.float32)):
        for bins in ((None, 5) if img.dtype.kind == "i" else (5,)):
            nbins, lo, width = h.histogram_binning(img, bins)
            assert width == 1.0 and lo == float(img.flat[0]) and nbins == (1 if bins is None else bins)
            assert not h.histogram_bins(img, nbins, lo, width).any()
    wide = np.array([0, 65535], np.uint16)
    assert h.histogram_binning(wide) == (65536, 0.0, 1.0)
    assert h.histogram_bins(wide, 65536, 0.0, 1.0).tolist() == [0, 65535]
    assert h.histogram_bins(wide, 1, 0.0, 1.0).tolist() == [0, 0]
    big = np.array([-2 ** 62, 2 ** 62], np.int64)   # beyond 2^53: float64 of the range, no overflow of the dtype
    assert h.histogram_binning(big, 2) == (2, float(-2 ** 62), float(2 ** 62))
    assert h.histogram_bins(big, 2, float(-2 ** 62), float(2 ** 62)).tolist() == [0, 1]


def test_every_value_error():
    h = _hist()
    img = np.arange(12, dtype=np.int32).reshape(3, 4)
    with pytest.raises(ValueError, match="pass bins"):
        h.histogram_binning(np.array([0, 65536], np.int32))
    assert h.histogram_binning(np.array([0, 65535], np.int32))[0] == 65536
    for bins in (0, -1, 65537, 2.5, True, "7"):
        with pytest.raises(ValueError):
            h.histogram_binning(img, bins)
    for bad in (np.nan, np.inf, -np.inf):
        f = img.astype(np.float64)
        f[1, 2] = bad
        with pytest.raises(ValueError):
            h.histogram_binning(f, 8)
    with pytest.raises(ValueError):
        h.histogram_binning(np.empty((0, 3), np.uint8), 4)
    with pytest.raises(ValueError):
        h.histogram_binning(np.array(["a"]), 4)
    with pytest.raises(ValueError):   # a range that has no finite width
        h.histogram_binning(np.array([-1.7e308, 1.7e308]), 4)
    for args in ((0, 0.0, 1.0), (65537, 0.0, 1.0), (2.0, 0.0, 1.0), (4, np.nan, 1.0), (4, np.inf, 1.0), (4, 0.0, 0.0), (4, 0.0, -1.0), (4, 0.0, np.inf),
                 (4, 0.0, np.nan)):
        with pytest.raises(ValueError):
            h.histogram_bins(img, *args)
    ones = np.ones(4)
    for lam, eps in ((1.0, 0.0), (1.0, -0.5), (1.0, np.nan), (1.0, np.inf), (-1.0, 0.5), (np.nan, 0.5), (np.inf, 0.5)):
        with pytest.raises(ValueError):
            h.histogram_tables(ones, ones, lam, eps)
    for fg, bg in ((ones, np.ones(5)), (np.empty(0), np.empty(0)), (-ones, ones), (ones, ones * np.nan)):
        with pytest.raises(ValueError):
            h.histogram_tables(fg, bg)


def test_tables():
    h = _hist()
    fg, bg = np.array([0, 3, 1, 0]), np.array([5, 0, 0, 1])
    s, k = h.histogram_tables(fg, bg, lam=2.0, eps=0.5)
    p_fg, p_bg = (fg + 0.5) / (4 + 4 * 0.5), (bg + 0.5) / (6 + 4 * 0.5)
    assert s.tolist() == (-2.0 * np.log(p_bg)).tolist() and k.tolist() == (-2.0 * np.log(p_fg)).tolist()   # source: -lam ln Pr(. | bkg)
    assert s.dtype == k.dtype == np.float64 and s.flags.c_contiguous and k.flags.c_contiguous
    assert s[1] > s[0] and k[0] > k[1]   # what the background never showed is tied to the source, and the other way round
    # empty histograms: finite, >= 0 (and uniform), for any eps > 0 -- also at one bin and at 65536
    for nbins in (1, 2, 256, 65536):
        for eps in (1e-9, 0.5, 3.0):
            s, k = h.histogram_tables(np.zeros(nbins, np.int64), np.zeros(nbins, np.int64), 1.0, eps)
            assert np.isfinite(s).all() and np.isfinite(k).all() and (s >= 0).all() and (k >= 0).all() and not np.signbit(s).any()
            assert np.ptp(s) == 0 and np.ptp(k) == 0
    s, k = h.histogram_tables(fg, bg, lam=0.0)
    assert not s.any() and not k.any() and not np.signbit(s).any() and not np.signbit(k).any()
    s, k = h.histogram_tables(fg, np.zeros(4), lam=1.0, eps=1e-12)   # a tiny eps: large, finite
    assert np.isfinite(k).all() and k[0] > 20


# ---- the rule of mgc_binned.h as a stand-alone program --------------------------------------------------------------------------------
def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where this machine's g++ has the runtimes, else nothing"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0 else []


@pytest.fixture(scope="module")
def binned_programs(tmp_path_factory):
    """binned_main.cpp compiled plainly and once more under the sanitizers: both run every case"""
    tmp = tmp_path_factory.mktemp("binned")
    src = os.path.join(HERE, "hostsim", "binned_main.cpp")
    exes = [str(tmp / "binned_plain")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exes[0], src])
    flags = _sanitizer_flags(tmp)
    print("sanitizers:", " ".join(flags) or "none (no runtimes on this machine)")
    if flags:
        exes.append(str(tmp / "binned_san"))
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + flags + ["-o", exes[1], src])
    return tmp, exes


def _program_bins(binned_programs, name, values, nbins, lo, width):
    tmp, exes = binned_programs
    values = np.ascontiguousarray(values, dtype=DTYPES[name])
    values.tofile(str(tmp / "values.bin"))
    outs = []
    for exe in exes:
        out = subprocess.run([exe, "bins", name, str(nbins), float(lo).hex(), float(width).hex(), str(tmp / "values.bin"), str(tmp / "bins.bin")],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        outs.append(np.fromfile(str(tmp / "bins.bin"), dtype=np.int64))
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0])
    return outs[0]


def _border_values(dtype, nbins, lo, width, rng):
    """values next to the borders lo + k * width, one step of the dtype either side, and values far outside"""
    k = np.unique(np.concatenate([np.arange(0, min(nbins, 40)), rng.integers(0, nbins + 1, 200), [nbins - 1, nbins]]))
    with np.errstate(over="ignore"):   # (what overflows the dtype is dropped by the caller)
        b = (lo + k * width).astype(dtype)
        far = np.array([-3.0e38, -1e30, 1e30, 3.0e38, lo - 1e6 * width, lo + (nbins + 1e6) * width]).astype(dtype)
    return np.concatenate([b, np.nextafter(b, dtype.type(-np.inf)), np.nextafter(b, dtype.type(np.inf)), far, -far])


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_program_bins_equal_numpy_next_to_borders(binned_programs, name):
    h = _hist()
    dtype = np.dtype(DTYPES[name])
    rng = np.random.default_rng(17)
    for nbins, lo, width in ((7, -1.0, 0.1), (16, 0.3, 1.0 / 3.0), (256, -1000.0, 7.8125), (4095, 0.0, 1e-3), (65536, -3.0, 3.0e-5),
                             (10, 0.0, 1e300), (10, 0.0, 1e-300), (1000, 1e-310, 5e-324), (3, -1e308, 1e308), (1, 5.0, 2.0)):   # huge and tiny widths
        v = _border_values(dtype, nbins, lo, width, rng)
        v = v[np.isfinite(v)]
        got = _program_bins(binned_programs, name, v, nbins, lo, width)
        want = h.histogram_bins(v, nbins, lo, width)
        np.testing.assert_array_equal(got, want, err_msg="%s nbins %d lo %r width %r" % (name, nbins, lo, width))
        assert got.min() >= 0 and got.max() <= nbins - 1


@pytest.mark.parametrize("name", ["i64", "u64", "i32", "u8", "i8", "u16", "i16", "u32"])
def test_program_bins_equal_numpy_on_integers(binned_programs, name):
    h = _hist()
    dtype = np.dtype(DTYPES[name])
    info = np.iinfo(dtype)
    rng = np.random.default_rng(19)
    edge = np.array([info.min, info.min + 1, info.max - 1, info.max, 0, 1], dtype=dtype)
    vals = [edge, rng.integers(info.min, info.max, 500, dtype=dtype, endpoint=True)]
    if dtype.itemsize == 8:   # beyond 2^53: neighbours that round to the same or to different doubles
        around = np.array([2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, 2 ** 60 + 127, 2 ** 60 + 128, 2 ** 60 + 129, 2 ** 62 + 511, 2 ** 62 + 513], dtype=np.uint64)
        vals.append(around.astype(dtype))
        if dtype.kind == "i":
            vals.append((-around.astype(np.int64)).astype(dtype))
        else:
            vals.append(np.array([2 ** 64 - 1, 2 ** 64 - 1025, 2 ** 63, 2 ** 63 + 1025], dtype=np.uint64))
    v = np.concatenate(vals)
    for nbins, lo, width in ((256, float(info.min), 1.0), (65536, float(info.min), (float(info.max) - float(info.min)) / 65536), (7, 2.0 ** 53, 1.0),
                             (1000, 2.0 ** 60, 128.0), (16, -5.5, 0.75), (3, 0.0, 1e300), (5, 0.0, 1e-300)):
        got = _program_bins(binned_programs, name, v, nbins, lo, width)
        np.testing.assert_array_equal(got, h.histogram_bins(v, nbins, lo, width), err_msg="%s nbins %d lo %r width %r" % (name, nbins, lo, width))


def test_program_argument_and_table_check(binned_programs):
    tmp, exes = binned_programs
    good = np.linspace(-2.0, 5.0, 8)   # negative entries are allowed

    def check(nbins, lo, width, source, sink):
        paths = []
        for k, t in enumerate((source, sink)):
            if t is None:
                paths.append("-")
            else:
                paths.append(str(tmp / ("table%d.bin" % k)))
                np.asarray(t, np.float64).tofile(paths[-1])
        outs = [subprocess.run([exe, "check", str(nbins), repr(float(lo)), repr(float(width))] + paths, capture_output=True, text=True) for exe in exes]
        for o in outs:
            assert o.returncode == 0, o.stdout + o.stderr
            assert o.stdout == outs[0].stdout
        return outs[0].stdout.strip()
    assert check(8, 0.0, 1.0, good, good[::-1].copy()) == "OK"
    for nbins, lo, width, names in ((0, 0.0, 1.0, "nbins"), (65537, 0.0, 1.0, "nbins"), (-3, 0.0, 1.0, "nbins"), (8, np.nan, 1.0, "lo"), (8, np.inf, 1.0, "lo"),
                                    (8, 0.0, 0.0, "width"), (8, 0.0, -1.0, "width"), (8, 0.0, np.inf, "width"), (8, 0.0, np.nan, "width")):
        out = check(nbins, lo, width, np.ones(max(nbins, 1)), np.ones(max(nbins, 1)))
        assert out.startswith("INVALID 0 -1 ") and names in out, out
    assert check(8, 0.0, 1.0, None, good).startswith("INVALID 0 -1 source_table NULL")
    assert check(8, 0.0, 1.0, good, None).startswith("INVALID 1 -1 sink_table NULL")
    for which, idx, value in ((0, 7, np.nan), (1, 0, np.inf), (0, 3, -np.inf), (1, 7, np.nan)):
        s, k = good.copy(), good.copy()
        (s if which == 0 else k)[idx] = value
        if idx < 7:
            (k if which == 0 else s)[7] = np.nan   # a later offender in the other table: not the one named
        out = check(8, 0.0, 1.0, s, k)
        assert out.startswith("INVALID %d %d %s[%d]" % (which, idx, ("source_table", "sink_table")[which], idx)), out
    s, k = good.copy(), good.copy()
    s[2] = k[2] = np.nan   # both tables bad at one index: the source entry is the first
    assert check(8, 0.0, 1.0, s, k).startswith("INVALID 0 2 source_table[2]")
    assert check(65536, -1.0, 1e-3, np.zeros(65536), np.zeros(65536)) == "OK"


# ---- the plug-in on a facade that merges on the host ----------------------------------------------------------------------------------
def _case(shape, dtype, seed=5):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 60, shape).astype(dtype) if np.dtype(dtype).kind != "f" else rng.normal(0.0, 1.0, shape).astype(dtype)
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    fg[tuple(slice(n // 3, n // 3 + 2) for n in shape[:-1]) + (slice(1, 3),)] = True
    bg[..., -1] = True
    bg[tuple(n // 3 for n in shape[:-1]) + (1,)] = True   # one voxel under both kinds of marker
    return img, fg, bg


def _expanded(img, fg, bg, bins, lam, eps):
    h = _hist()
    nbins, lo, width = h.histogram_binning(img, bins)
    b = h.histogram_bins(img, nbins, lo, width).ravel()
    fg_hist = np.bincount(b[fg.ravel()], minlength=nbins)
    bg_hist = np.bincount(b[bg.ravel()], minlength=nbins)
    s, k = h.histogram_tables(fg_hist, bg_hist, lam, eps)
    return s[b], k[b]


@pytest.mark.parametrize("dtype,bins", [(np.uint8, None), (np.int16, 7), (np.float32, 16)], ids=["u8", "i16_7", "f32_16"])
def test_plugin_on_the_host_merge_route_equals_the_hand_expanded_merge(dtype, bins):
    """a set_tweight before the term sends the graph to the host merge: the merged t-links and the flow constant are those of
    merge_tweights_into of the hand-expanded arrays, bit for bit, in call order (set_tweight, histogram, dense)"""
    from medpy_amd.graphcut import GCGraph, energy_voxel
    from medpy_amd.graphcut.graph import merge_tweights_into
    shape = (5, 4, 6)
    n = int(np.prod(shape))
    img, fg, bg = _case(shape, dtype)
    rng = np.random.default_rng(8)
    ds, dk = rng.uniform(0, 5, shape), rng.uniform(0, 5, shape)
    g = GCGraph(n, 0, shape=shape)
    g.set_tweight(7, 1.5, 0.25)
    energy_voxel.regional_histogram(g, (img, bins, 2.0, 0.5))
    g.set_tweights_dense(ds, dk)
    assert len(g._GCGraph__tdense) == 2   # the term waits for the markers, and the dense call behind it waits with it
    g.record_markers(fg, bg)
    g._GCGraph__merge_dense_tweights()
    tr, fc = np.zeros(n), 0.0
    fc = merge_tweights_into(tr, fc, np.array([7]), np.array([1.5]), np.array([0.25]))
    s, k = _expanded(img, fg, bg, bins, 2.0, 0.5)
    fc = merge_tweights_into(tr, fc, np.arange(n), s, k)
    fc = merge_tweights_into(tr, fc, np.arange(n), ds.ravel(), dk.ravel())
    assert g._GCGraph__tr.view(np.int64).tolist() == tr.view(np.int64).tolist() and g._GCGraph__flow_const == fc
    assert g._GCGraph__tdense == []


def test_plugin_records_and_refuses():
    from medpy_amd import graphcut
    from medpy_amd.graphcut import GCGraph, energy_voxel
    assert "regional_histogram" in energy_voxel.__all__ and graphcut.regional_histogram is energy_voxel.regional_histogram
    for name in ("histogram_binning", "histogram_bins", "histogram_tables", "regional_histogram"):
        assert name in graphcut.__all__
    shape = (4, 6)
    img = np.arange(24, dtype=np.uint8).reshape(shape)
    g = GCGraph(24, 0, shape=shape)
    energy_voxel.regional_histogram(g, (img, None, 1.0, 0.5))
    (term, none), = g._GCGraph__tdense
    assert none is None and (term.nbins, term.lo, term.width, term.lam, term.eps) == (24, 0.0, 1.0, 1.0, 0.5) and term.image.shape == shape
    assert g._GCGraph__tr is None   # nothing is merged on the host while the graph can still take the device path
    for bad in ((img.ravel()[:23], None, 1.0, 0.5), (img, 0, 1.0, 0.5), (img, None, -1.0, 0.5), (img, None, 1.0, 0.0),
                (img.astype(np.float32), None, 1.0, 0.5), (np.full(shape, np.nan), 4, 1.0, 0.5)):
        with pytest.raises(ValueError):
            energy_voxel.regional_histogram(g, bad)
    assert len(g._GCGraph__tdense) == 1
    with pytest.raises(TypeError):
        energy_voxel.regional_histogram(object(), (img, None, 1.0, 0.5))
    # a per-node t-weight behind the term before any marker is known: the term cannot be fitted yet
    with pytest.raises(NotImplementedError):
        g.set_tweight(0, 1.0, 0.0)
    assert len(g._GCGraph__tdense) == 1 and g._GCGraph__tr is None


def test_voxel_graph_methods_check_before_the_library():
    from medpy_amd.graphcut import graph
    g = object.__new__(graph.VoxelGraph)
    g._h = None
    g._shape = (2, 2)
    with pytest.raises(ValueError):   # no binning to fall back on
        g.update_tweights_binned(np.ones(4), np.ones(4))
    with pytest.raises(ValueError):
        g.update_tweights_binned(np.ones(4), np.ones(4), nbins=4)   # nbins, lo and width come together
    with pytest.raises(ValueError):
        g.update_tweights_binned(np.ones(3), np.ones(4), 4, 0.0, 1.0)   # a table of another length
    with pytest.raises(ValueError):
        g._add_tweights_binned(np.ones(4), np.ones((2, 2)), 4, 0.0, 1.0)
    with pytest.raises(ValueError):
        g.marker_histograms(0, 0.0, 1.0)
    with pytest.raises(ValueError):
        g.refit_regional_histogram()
    g._tweights_merged = True
    for call in (lambda: g.update_tweights_binned(np.ones(4), np.ones(4), 4, 0.0, 1.0), g.refit_regional_histogram):
        with pytest.raises(NotImplementedError):
            call()
    for cls in (graph.SparseGraph, graph.RegionGraph, graph.EmbeddedLatticeGraph):   # the other graph classes get no new methods
        for name in ("update_tweights_binned", "refit_regional_histogram", "marker_histograms"):
            assert not hasattr(cls, name)


def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    tables = r"int64_t nbins, double lo, double width, const double\* source_table, const double\* sink_table\);"
    want = {"mgc_set_feature_image": r"int mgc_set_feature_image\(mgc_handle h, const void\* image, int dtype\);",
            "mgc_marker_histograms": r"int mgc_marker_histograms\(mgc_handle h, int64_t nbins, double lo, double width, int64_t\* fg_hist, int64_t\* bg_hist, int64_t\* out4\);",
            "mgc_add_tweights_binned": r"int mgc_add_tweights_binned\(mgc_handle h, " + tables,
            "mgc_update_tweights_binned": r"int mgc_update_tweights_binned\(mgc_handle h, " + tables}
    for name, decl in want.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    for d in ("mgc_binned.h", "mgc_binned_ops.inl", "mgc_binned_driver.inl"):
        assert d in build.DEPS and os.path.exists(os.path.join(build.CSRC, d)), d
    text = open(os.path.join(build.CSRC, "mgc_binned.h")).read()
    # the rule and the checks stay plain C++: a stand-alone program includes them
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text
    limits = dict(re.findall(r"#define (MGC_BINNED_\w+) (\d+)", text))
    assert int(limits["MGC_BINNED_LDS_MAX"]) == _lib.BINNED_LDS_MAX and int(limits["MGC_BINNED_MAX_BINS"]) == _lib.BINNED_MAX_BINS
    # behind every kernel that was there before it: at the end of mgc_kernels.hip behind mgc_reach_driver.inl, and nothing in front
    # includes it
    import driver_chain
    driver_chain.assert_behind_everything_before_it("mgc_binned_driver.inl", "mgc_binned")

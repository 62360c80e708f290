"""-m gpu: the histograms over every voxel split by a label, and the histogram term refitted from the cut until nothing moves
 -- mgc_label_histograms against numpy.bincount, its states and its lack of side effects, and
iterate_regional_histogram in lock-step with the same loop on the host: bincount over the reference labels, histogram_tables, BK.

The inputs are the family of tests/test_gpu_histogram_term.py (its helpers are imported, not copied): n-links uniform(0.05, 1)
through _add_nweights, its three image kinds, its markers.  For the loop cases every round's BK cut is unique (the ambiguity set
of oracle/cutcheck.py is empty at tol 0 and at 64 ulp), so labels are compared voxel for voxel, without the tie relaxation, and
the reference reaches the fixed point within 4 refits, well inside the cap of 8.  Every reference loop is computed once per case and
module and shared."""
import numpy as np
import pytest

import test_gpu_histogram_term as fam

pytestmark = pytest.mark.gpu

ALL_DTYPES = fam.ALL_DTYPES
HIST_SHAPES = [(17, 16, 31), (9, 8, 7), (3, 1, 5), (1, 1, 17), (9, 10)]   # several workgroups; groups plus a tail; below one group; 1-D; 2-D
PATTERNS = ["bernoulli", "zeros", "ones", "checkerboard", "block", "bytes"]
EPS = 0.5
# (shape, neighbourhood, image kind): the reference loop takes 4, 3, 2, 3, 4, 2 and 1 refits to the fixed point
LOOP_CASES = [((17, 9, 10), None, "f32"), ((17, 16, 31), None, "f32"), ((17, 16, 31), None, "i16"), ((9, 10), 4, "i16"), ((9, 10, 11), 26, "f32"),
              ((9, 10, 11), 26, "u8"), ((9, 8, 7), None, "u8")]
LOOP_IDS = ["x".join(map(str, s)) + "_n%d_%s" % (c or 2 * len(s), k) for s, c, k in LOOP_CASES]
_LOOPS = {}


# ---- 1. histograms equal numpy.bincount, explicit labels ------------------------------------------------------------------------
def _labels(shape, pattern, seed=13):
    rng = np.random.default_rng(seed)
    if pattern == "bernoulli":
        return rng.random(shape) < 0.5
    if pattern == "zeros":
        return np.zeros(shape, bool)
    if pattern == "ones":
        return np.ones(shape, np.uint8)
    if pattern == "checkerboard":
        return (np.indices(shape).sum(axis=0) % 2).astype(bool)
    if pattern == "block":
        lab = np.zeros(shape, np.uint8)
        lab[tuple(slice(n // 4, n // 4 + max(1, n // 2)) for n in shape)] = 1
        return lab
    lab = rng.integers(0, 256, shape).astype(np.uint8)   # any byte but 0 is foreground
    lab[rng.random(shape) < 0.4] = 0
    return lab


def _expected(img, labels, nbins, lo, width):
    x = np.floor((img.astype(np.float64) - lo) / width)
    b = np.clip(x, 0, nbins - 1).astype(np.int64)
    m = np.asarray(labels) != 0
    out4 = [int(m.sum()), int((~m).sum()), int((x < 0).sum()), int((x > nbins - 1).sum())]
    return np.bincount(b[m], minlength=nbins), np.bincount(b[~m], minlength=nbins), out4


def _check(g, img, labels, nbins, lo, width, given=True):
    fg_hist, bg_hist = g.label_histograms(labels if given else None, nbins, lo, width)
    want_fg, want_bg, out4 = _expected(img, labels, nbins, lo, width)
    assert fg_hist.dtype == bg_hist.dtype == np.int64 and fg_hist.size == bg_hist.size == nbins
    np.testing.assert_array_equal(fg_hist, want_fg)
    np.testing.assert_array_equal(bg_hist, want_bg)
    assert int(fg_hist.sum()) + int(bg_hist.sum()) == img.size
    info = g.label_histogram_info()
    assert [info[k] for k in ("fg_voxels", "bg_voxels", "below", "above")] == out4, (info, out4)
    return out4


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=[np.dtype(d).name for d in ALL_DTYPES])
def test_histograms_equal_bincount(dtype):
    """all ten dtypes; every shape, label pattern and bin count around the LDS threshold; a range that leaves values outside on
    both sides (clamped, and counted).  Before mgc_build: the call with a label plane needs no built graph."""
    from medpy_amd.graphcut import VoxelGraph
    for shape in HIST_SHAPES:
        img = fam._hist_image(shape, dtype, 7)
        g = VoxelGraph(shape)
        g._set_feature_image(img)
        mn, mx = float(img.min()), float(img.max())
        span = (mx - mn) or 1.0
        for pattern in PATTERNS:
            labels = _labels(shape, pattern)
            for nbins in fam._bin_counts():
                out4 = _check(g, img, labels, nbins, mn + 0.3 * span, 0.4 * span / nbins)   # the outer three tenths lie outside
                if img.size > 1000:
                    assert out4[2] > 0 and out4[3] > 0
            _check(g, img, labels, 256, mn, span / 256)
        g.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64], ids=["uint8", "int16", "float32", "float64"])
def test_constant_image_one_bin_for_every_voxel(dtype):
    """maximal contention: every count of the volume lands on one bin of one or two counters, and every run is as long as its group"""
    from medpy_amd import _lib
    from medpy_amd.graphcut import VoxelGraph
    shape = (17, 16, 31)
    img = np.full(shape, 5, dtype)
    g = VoxelGraph(shape)
    g._set_feature_image(img)
    for pattern in ("ones", "zeros", "bernoulli", "block"):
        for nbins, lo, width in ((1, 5.0, 1.0), (7, 2.0, 1.0), (7, 9.0, 1.0), (7, -9.0, 1.0), (_lib.BINNED_LDS_MAX + 1, 2.0, 1.0)):
            _check(g, img, _labels(shape, pattern), nbins, lo, width)
    g.close()


def test_grid_stride_loop_takes_a_second_trip():
    """9.1 M voxels: more groups of 16 than one trip of the grid (2048 workgroups of 256 threads) takes, and an odd tail"""
    from medpy_amd import _lib
    from medpy_amd.graphcut import VoxelGraph
    shape = (211, 207, 209)
    assert int(np.prod(shape)) > 2048 * 256 * 16 and int(np.prod(shape)) % 16
    rng = np.random.default_rng(17)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    img[:100] //= 8   # long runs of few values in one half, noise in the other
    labels = rng.random(shape) < 0.5
    labels[50:150] = True
    g = VoxelGraph(shape)
    g._set_feature_image(img)
    for nbins, lo, width in ((256, 0.0, 1.0), (_lib.BINNED_LDS_MAX + 1, 10.0, 0.05)):
        _check(g, img, labels, nbins, lo, width)
    g.close()


# ---- 2. histograms of the current cut -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", fam.FORMS)
@pytest.mark.parametrize("shape,conn,kind", [((17, 9, 10), None, "f32"), ((9, 10, 11), 26, "u8"), ((9, 10), 4, "i16")], ids=["17x9x10_n6", "9x10x11_n26", "9x10_n4"])
def test_histograms_of_the_current_cut_cold_and_warm(shape, conn, kind, forms):
    nw = fam._nweights(shape, conn)
    fg, bg = fam._markers(shape)
    img = fam._image(shape, kind)
    t = fam._term(img, fg, bg, fam.BINS[kind], lam=fam._lam(conn))
    g = fam._handle(shape, conn, nw, fg, bg, feature=img)
    g._add_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"])
    fam._built(g, forms)
    g.maxflow()
    cold = g.labels().copy()
    assert fg.sum() < cold.sum() < cold.size
    _check(g, img, cold, *t["binning"], given=False)
    _check(g, img, cold, 5, float(img.min()) + 1.0, 0.25, given=False)   # another binning than the term's
    g.edit_markers(fg=fam._stroke(shape, cold, fg, bg))
    g.maxflow()
    warm = g.labels().copy()
    assert (warm != cold).any()
    _check(g, img, warm, *t["binning"], given=False)
    _check(g, img, cold, *t["binning"])   # a plane of the caller's on the solved handle: the plane counts, not the cut
    g.close()


# ---- 3. states and side effects -------------------------------------------------------------------------------------------------
def _raises(code, call, *names):
    from medpy_amd import _lib
    with pytest.raises(_lib.MedpyHipError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    assert "mgc_label_histograms" in str(ei.value) and all(n in str(ei.value) for n in names), str(ei.value)


def test_states_refusals_and_no_side_effects():
    from medpy_amd import _lib
    shape, kind = (9, 8, 7), "f32"
    n = int(np.prod(shape))
    nw = fam._nweights(shape, None)
    fg, bg = fam._markers(shape)
    img = fam._image(shape, kind)
    t = fam._term(img, fg, bg, fam.BINS[kind])
    binning = t["binning"]
    plane = _labels(shape, "bernoulli")
    # no image at all
    g = fam._handle(shape, None, nw, fg, bg)
    _raises(_lib.ERR_STATE, lambda: g.label_histograms(plane, *binning), "no feature image")
    g._set_feature_image(img)
    # labels=None needs a cut: not before build, not before the solve
    _raises(_lib.ERR_STATE, lambda: g.label_histograms(None, *binning), "before mgc_build")
    _check(g, img, plane, *binning)
    g._add_tweights_binned(t["tables"][0], t["tables"][1], *binning)
    fam._built(g, "as_shipped")
    _raises(_lib.ERR_STATE, lambda: g.label_histograms(None, *binning), "before mgc_maxflow")
    _check(g, img, plane, *binning)
    flow0 = g.maxflow()
    labels0 = g.labels().copy()
    bytes0, counts0 = g.stats()["device_bytes"], g.launch_counts()
    _check(g, img, labels0, *binning, given=False)
    _check(g, img, plane, *binning)
    # refusals: the binning, NULL outputs
    lib = _lib.load()
    fgh, bgh = np.zeros(binning[0], np.int64), np.zeros(binning[0], np.int64)
    for nb, lo, w, what in ((0, 0.0, 1.0, "nbins"), (65537, 0.0, 1.0, "nbins"), (4, np.nan, 1.0, "lo"), (4, 0.0, 0.0, "width"), (4, 0.0, np.inf, "width")):
        for lab in (None, _lib.ptr(plane.view(np.uint8))):
            assert lib.mgc_label_histograms(g._h, lab, nb, lo, w, _lib.ptr(fgh), _lib.ptr(bgh), None) == _lib.ERR_INVALID
            msg = lib.mgc_last_error(g._h).decode()
            assert "mgc_label_histograms" in msg and what in msg, msg
    for a, b in ((None, _lib.ptr(bgh)), (_lib.ptr(fgh), None)):
        assert lib.mgc_label_histograms(g._h, None, binning[0], binning[1], binning[2], a, b, None) == _lib.ERR_INVALID
        assert "NULL" in lib.mgc_last_error(g._h).decode()
    assert lib.mgc_label_histograms(g._h, None, binning[0], binning[1], binning[2], _lib.ptr(fgh), _lib.ptr(bgh), None) == _lib.OK   # out4 is optional
    assert fgh.tolist() == _expected(img, labels0, *binning)[0].tolist()
    # a value that is not finite anywhere in the volume, under either label: the lowest flat index and the value are named
    under1, under0 = int(np.flatnonzero(labels0.ravel())[3]), int(np.flatnonzero(~labels0.ravel())[3])
    for idx, value, text in ((under1, np.nan, "nan"), (under0, np.inf, "inf"), (n - 1, -np.inf, "-inf")):
        bad = img.copy()
        bad.ravel()[idx] = value
        if idx != n - 1:
            bad.ravel()[n - 1] = np.nan   # a later offender: not the one named
        g._set_feature_image(bad)
        _raises(_lib.ERR_INVALID, lambda: g.label_histograms(None, *binning), "image[%d] = %s" % (idx, text))
        _raises(_lib.ERR_INVALID, lambda: g.label_histograms(labels0, *binning), "image[%d] = %s" % (idx, text))
        _raises(_lib.ERR_INVALID, lambda: g.label_histograms(~labels0, *binning), "image[%d] = %s" % (idx, text))
    g._set_feature_image(img)
    # nothing on the handle has changed: bytes, launch counts, labels, flow
    assert g.stats()["device_bytes"] == bytes0 and g.launch_counts() == counts0
    assert np.array_equal(g.labels(), labels0) and g.maxflow() == flow0
    # an edit or an update waits for the next maxflow(): no current cut in between; a caller's plane is counted all the same
    stroke = fam._stroke(shape, labels0, fg, bg)
    previous = labels0.copy()
    g.edit_markers(fg=stroke)
    _raises(_lib.ERR_STATE, lambda: g.label_histograms(None, *binning), "before mgc_maxflow")
    _check(g, img, plane, *binning)
    flow1 = g.maxflow()
    labels1 = g.labels().copy()
    counts1, bytes1 = g.launch_counts(), g.stats()["device_bytes"]   # (the label snapshot of the edit is one more plane)
    assert (labels1 != labels0).any()
    _check(g, img, labels1, *binning, given=False)
    _check(g, img, plane, *binning)
    # ... and the label snapshot of the stroke edit is still there: the delta and labels(out=previous) work after both kinds of call
    changed = g.changed_labels()
    assert np.array_equal(np.sort(changed), np.flatnonzero((labels1 != labels0).ravel()))
    assert np.array_equal(g.labels(out=previous), labels1)
    assert g.launch_counts() == counts1 and g.stats()["device_bytes"] == bytes1 and g.maxflow() == flow1
    g.update_tweights_binned(t["tables"][0] * 0.5, t["tables"][1] * 0.5, *binning)
    _raises(_lib.ERR_STATE, lambda: g.label_histograms(None, *binning), "before mgc_maxflow")
    _check(g, img, plane, *binning)
    g.maxflow()
    _check(g, img, g.labels(), *binning, given=False)
    # a VoxelGraph built by hand has no binning to fall back on
    with pytest.raises(ValueError):
        g.label_histograms()
    with pytest.raises(ValueError):
        g.iterate_regional_histogram()
    g.close()


def test_the_boundary_image_is_read_where_no_feature_image_is_set():
    shape = (9, 8, 7)
    img = fam._image(shape, "i16")
    other = fam._image(shape, "u8", seed=77)
    plane = _labels(shape, "block")
    g = fam._handle(shape, None, None, boundary=img)
    _check(g, img, plane, 7, -100.0, 50.0)
    g._set_feature_image(other)
    _check(g, other, plane, 7, 10.0, 9.0)
    g._set_feature_image(None)
    _check(g, img, plane, 7, -100.0, 50.0)
    g.close()


def test_slab_handles_are_refused():
    from medpy_amd import _lib, synthetic
    from medpy_amd.slab import HipSlab, LoopbackExchange, sync_boundary_table
    sph = synthetic.sphere((32, 24, 24))
    slabs = [HipSlab(sph["image"].shape, r, 2) for r in range(2)]
    for sl in slabs:
        planes = slice(sl.plane0, sl.plane1)
        sl.set_boundary(sph["term"], sph["image"][planes], sph["sigma"], False)
        sl.set_markers(sph["fg"][planes], sph["bg"][planes])
    sync_boundary_table(slabs, LoopbackExchange(slabs))
    lib = _lib.load()
    fgh, bgh = np.zeros(8, np.int64), np.zeros(8, np.int64)
    for sl in slabs:
        for build in (False, True):
            if build:
                sl.build()
            plane = np.ascontiguousarray(sph["fg"][sl.plane0:sl.plane1]).view(np.uint8)
            for lab in (None, _lib.ptr(plane)):
                assert lib.mgc_label_histograms(sl._h, lab, 8, 0.0, 0.125, _lib.ptr(fgh), _lib.ptr(bgh), None) == _lib.ERR_UNSUPPORTED
                assert b"slab" in lib.mgc_last_error(sl._h)


# ---- 4. the loop against the oracle ---------------------------------------------------------------------------------------------
def _boundary_by_offset(graph, args):
    """the family's n-links as a boundary plug-in: one dense array pair per offset of the neighbourhood"""
    (nw,) = args
    for o, (there, back) in nw.items():
        graph.set_nweights_dense(o, there, back)


def _inputs(shape, conn, kind):
    return fam._nweights(shape, conn), fam._markers(shape), fam._image(shape, kind)


def _host_loop(shape, conn, kind, max_refits=8):
    """the loop on the host, once per case: the stroke-fitted cut, then bincount over the previous reference labels,
    histogram_tables, BK fed the expanded tables with the markers last.  dict: flow0 / labels0 of the stroke-fitted cut; per refit
    fg_voxels, moved, flow, labels; converged."""
    key = (shape, conn, kind)
    if key in _LOOPS:
        return _LOOPS[key]
    from medpy_amd.graphcut import histogram_tables
    nw, (fg, bg), img = _inputs(shape, conn, kind)
    lam = fam._lam(conn)
    t0 = fam._term(img, fg, bg, fam.BINS[kind], lam, EPS)
    nbins = t0["binning"][0]
    bins = t0["bins"]
    flow, labels = fam._bk(("iterate", key, 0), shape, nw, [(t0["S"], t0["K"])], fg, bg)
    out = {"flow0": flow, "labels0": labels, "rounds": [], "converged": False, "binning": t0["binning"]}
    prev = None
    for r in range(max_refits + 1):
        fg_hist = np.bincount(bins[labels], minlength=nbins)
        bg_hist = np.bincount(bins[~labels], minlength=nbins)
        moved = None if prev is None else int(np.abs(fg_hist - prev).sum())
        if moved is not None and moved <= 0:
            out["converged"] = True
            break
        if r == max_refits:
            break
        s, k = histogram_tables(fg_hist, bg_hist, lam, EPS)
        before = labels
        flow, labels = fam._bk(("iterate", key, r + 1), shape, nw, [(s[bins], k[bins])], fg, bg)
        out["rounds"].append({"fg_voxels": int(fg_hist.sum()), "bg_voxels": int(bg_hist.sum()), "moved": moved, "flow": flow, "labels": labels,
                              "tables": (s, k), "flipped": int((labels != before).sum())})
        prev = fg_hist
    out["fg_hist"], out["bg_hist"] = fg_hist, bg_hist
    _LOOPS[key] = out
    return out


def _public_graph(shape, conn, kind, forms, monkeypatch):
    from conftest import LARGE_VOLUME_FORMS
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel
    if forms == "large_volume_forms":
        monkeypatch.setenv("MEDPY_HIP_PARAMS", LARGE_VOLUME_FORMS)
    nw, (fg, bg), img = _inputs(shape, conn, kind)
    g = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_histogram, regional_term_args=(img, fam.BINS[kind], fam._lam(conn), EPS),
                                   boundary_term=_boundary_by_offset, boundary_term_args=(nw,), connectivity=conn)
    info = g.tweight_edit_info()
    assert info["store_held"] == 1 and info["dense_calls"] == 1   # the tile solver, the term expanded on the device
    return g


def _record_labels(g):
    """the labels behind every solve of the loop, taken as the loop runs (labels() reads; it changes nothing on the graph)"""
    seen, solve = [], g.maxflow

    def maxflow():
        flow = solve()
        seen.append(g.labels().copy())
        return flow
    g.maxflow = maxflow
    return seen


@pytest.mark.parametrize("forms", fam.FORMS)
@pytest.mark.parametrize("shape,conn,kind", LOOP_CASES, ids=LOOP_IDS)
def test_loop_in_lock_step_with_the_host_loop(shape, conn, kind, forms, monkeypatch):
    from medpy_amd import _lib
    from medpy_amd.graphcut import histogram_bins, histogram_tables
    ref = _host_loop(shape, conn, kind)
    print("reference: %d refits, voxels changing side per refit %r, moved %r, converged %r" % (
        len(ref["rounds"]), [r["flipped"] for r in ref["rounds"]], [r["moved"] for r in ref["rounds"]], ref["converged"]))
    assert ref["converged"] and 1 <= len(ref["rounds"]) <= 4 and ref["rounds"][-1]["flipped"] == 0   # the fixed point, well inside the cap
    g = _public_graph(shape, conn, kind, forms, monkeypatch)
    assert g._binning == ref["binning"]
    flow0 = fam._assert_cut(g, ref["flow0"], ref["labels0"])
    seen = _record_labels(g)
    res = g.iterate_regional_histogram(max_refits=8)
    del g.maxflow
    assert res["converged"] is True and len(res["rounds"]) == len(ref["rounds"]) == len(seen)
    for got, want, labels in zip(res["rounds"], ref["rounds"], seen):
        np.testing.assert_array_equal(labels, want["labels"])   # after every refit, voxel for voxel
        assert got["flow"] == pytest.approx(want["flow"], rel=1e-9, abs=1e-300)
        assert (got["moved"], got["fg_voxels"], got["bg_voxels"]) == (want["moved"], want["fg_voxels"], want["bg_voxels"])
    assert res["fg_hist"].tolist() == ref["fg_hist"].tolist() and res["bg_hist"].tolist() == ref["bg_hist"].tolist()
    v = g.validate()
    assert not any(v[k] for k in _lib.VIOLATION_KEYS), v
    assert v["max_pair_error"] <= 1e-9 and v["max_node_error"] <= 1e-9, v
    assert g._hist_params == (fam._lam(conn), EPS)
    # a second handle driven by hand through the calls that existed before: bit-identical flows -- the loop is those calls
    _, _, img = _inputs(shape, conn, kind)
    nbins, lo, width = ref["binning"]
    bins = histogram_bins(img, nbins, lo, width)
    h = _public_graph(shape, conn, kind, forms, monkeypatch)
    assert h.maxflow() == flow0
    for got in res["rounds"]:
        lab = h.labels()
        s, k = histogram_tables(np.bincount(bins[lab], minlength=nbins), np.bincount(bins[~lab], minlength=nbins), fam._lam(conn), EPS)
        h.update_tweights_binned(s, k)
        assert h.maxflow() == got["flow"]
    np.testing.assert_array_equal(h.labels(), g.labels())
    assert fam._bits(h.tweights()) == fam._bits(g.tweights())
    h.close()
    g.close()


def test_loop_cap_and_stop_below(monkeypatch):
    shape, conn, kind = LOOP_CASES[0]
    ref = _host_loop(shape, conn, kind)
    moved = [r["moved"] for r in ref["rounds"]][1:]   # of the looks behind refit 1, 2, ... (the look that found 0 made no round)
    assert len(ref["rounds"]) >= 3 and moved[0] > moved[1] > 0
    # one refit allowed: one refit, and the look behind it still sees the histograms move
    g = _public_graph(shape, conn, kind, "as_shipped", monkeypatch)
    g.maxflow()
    res = g.iterate_regional_histogram(max_refits=1)
    assert res["converged"] is False and len(res["rounds"]) == 1 and res["rounds"][0]["moved"] is None
    assert res["rounds"][0]["flow"] == pytest.approx(ref["rounds"][0]["flow"], rel=1e-9)
    np.testing.assert_array_equal(g.labels(), ref["rounds"][0]["labels"])
    assert int(np.abs(res["fg_hist"] - ref["fg_hist"]).sum()) > 0
    # ... and the loop goes on from there to the same fixed point
    res = g.iterate_regional_histogram()
    assert res["converged"] is True and len(res["rounds"]) == len(ref["rounds"]) - 1
    np.testing.assert_array_equal(g.labels(), ref["rounds"][-1]["labels"])
    g.close()
    # stop_below at the host loop's second moved: the look behind the second refit ends the loop, before the fixed point
    g = _public_graph(shape, conn, kind, "as_shipped", monkeypatch)
    g.maxflow()
    res = g.iterate_regional_histogram(stop_below=moved[1])
    assert res["converged"] is True and len(res["rounds"]) == 2 < len(ref["rounds"])
    assert [r["moved"] for r in res["rounds"]] == [None, moved[0]]
    np.testing.assert_array_equal(g.labels(), ref["rounds"][1]["labels"])
    # a loop without a current cut is refused by the first look
    from medpy_amd import _lib
    g.edit_markers(fg=fam._stroke(shape, g.labels(), *fam._markers(shape)))
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.iterate_regional_histogram()
    assert ei.value.code == _lib.ERR_STATE
    g.close()

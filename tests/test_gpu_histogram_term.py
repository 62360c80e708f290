"""-m gpu: the histogram regional term fitted on the device -- mgc_marker_histograms against numpy.bincount,
mgc_add_tweights_binned / mgc_update_tweights_binned against the dense calls of the expanded arrays, and the cuts against the BK
oracle.

n-link weights are drawn from uniform(0.05, 1) and go in through _add_nweights; images are uint8 and int16 noise with a brighter
block (bins: one per value / 7) and float32 noise (16 bins); markers are a small fg box and the far bg face.  For this family BK's
cut is unique (the ambiguity set of oracle/cutcheck.py is empty at tol 0 and at 64 ulp, and the foreground is larger than the
marker box), so labels are compared voxel for voxel, without the tie relaxation.  The oracle is fed the arrays expanded on the
host (medpy_amd/graphcut/histogram.py, the definition of the term) in the library's merge order: explicit t-links first, the
markers last.  Every reference cut is computed once per input and module and shared."""
import itertools

import numpy as np
import pytest

from oracle import bk

pytestmark = pytest.mark.gpu

MAX = 65535.0  # GCGraph.MAX
CASES = [((9, 8, 7), None), ((1, 1, 17), None), ((3, 1, 5), None), ((17, 9, 10), None), ((17, 16, 31), None), ((9, 10), 4), ((9, 10), 8),
         ((9, 10, 11), 26)]
CASE_IDS = ["x".join(map(str, s)) + "_n%d" % (c or 2 * len(s)) for s, c in CASES]
FORMS = ["as_shipped", "large_volume_forms"]
KINDS = ["u8", "i16", "f32"]
BINS = {"u8": None, "i16": 7, "f32": 16}
ALL_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64, np.float32, np.float64]
_REF = {}


def _lam(conn):
    """the weight of the term: the 26 n-links of the full neighbourhood outweigh the term at 1, and the cut would hug the marker box"""
    return 4.0 if conn == 26 else 1.0


def _kind_of(shape, conn):
    """the image kind a case gets where a test does not run all three"""
    return KINDS[[c for c in CASES].index((shape, conn)) % 3]


def _offsets(ndim, conn):
    if conn in (None, 2 * ndim):
        return [tuple(1 if k == a else 0 for k in range(ndim)) for a in range(ndim)]
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if o > (0,) * ndim]


def _arcs(shape, off):
    ids = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, shape))
    dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, shape))
    mask = np.zeros(shape, bool)
    mask[src] = True
    return mask, ids[src].ravel(), ids[dst].ravel()


def _nweights(shape, conn, seed=23):
    rng = np.random.default_rng(seed)
    return {o: (rng.uniform(0.05, 1.0, shape), rng.uniform(0.05, 1.0, shape)) for o in _offsets(len(shape), conn)}


def _image(shape, kind, seed=11):
    """uint8 / int16 noise with a brighter block around the fg box, or float32 noise"""
    rng = np.random.default_rng(seed)
    block = tuple(slice(0, max(1, (n + 1) // 2)) for n in shape[:-1]) + (slice(0, max(1, shape[-1] // 2)),)
    if kind == "u8":
        img = rng.integers(0, 40, shape).astype(np.uint8)
        img[block] += 60
    elif kind == "i16":
        img = rng.integers(-200, 200, shape).astype(np.int16)
        img[block] += 300
    else:
        img = rng.normal(0.0, 1.0, shape).astype(np.float32)
    return img


def _markers(shape):
    """a small box of fg near the low corner, the far face along the last axis as bg"""
    fg = np.zeros(shape, bool)
    bg = np.zeros(shape, bool)
    fg[tuple(slice(n // 3, n // 3 + 2) for n in shape[:-1]) + (slice(1, 3),)] = True
    bg[..., -1] = True
    return fg, bg


def _term(img, fg, bg, bins, lam=1.0, eps=0.5):
    """the term on the host, by its definition: dict of the binning, the per-voxel bins, the histograms, the tables and the
    expanded arrays S = source_table[bins], K = sink_table[bins]"""
    from medpy_amd.graphcut import histogram as h
    nbins, lo, width = h.histogram_binning(img, bins)
    b = h.histogram_bins(img, nbins, lo, width)
    fg_hist = np.bincount(b[fg], minlength=nbins) if fg is not None else np.zeros(nbins, np.int64)
    bg_hist = np.bincount(b[bg], minlength=nbins) if bg is not None else np.zeros(nbins, np.int64)
    s, k = h.histogram_tables(fg_hist, bg_hist, lam, eps)
    return {"binning": (nbins, lo, width), "bins": b, "fg_hist": fg_hist, "bg_hist": bg_hist, "tables": (s, k), "S": s[b], "K": k[b]}


def _bk(key, shape, nw, calls=(), fg=None, bg=None, graph=None):
    """(flow, labels) of BK: explicit t-links call by call, the markers last (on ``graph``, an oracle graph that holds a boundary
    term already, or on a fresh one with the n-links nw)"""
    if key in _REF:
        return _REF[key]
    n = int(np.prod(shape))
    g = graph if graph is not None else bk.BKGraph(n, n * 13 + 16)
    for s, k in calls:
        g.add_tweights(None, np.asarray(s, np.float64).ravel(), np.asarray(k, np.float64).ravel())
    for o, (there, back) in (nw or {}).items():
        mask, i, j = _arcs(shape, o)
        g.sum_edges(i, j, there[mask], back[mask])
    for m, (s, t) in ((fg, (MAX, 0.0)), (bg, (0.0, MAX))):
        idx = np.flatnonzero(m.ravel()) if m is not None else np.empty(0, np.int64)
        if idx.size:
            g.add_tweights(idx, np.full(idx.size, s), np.full(idx.size, t))
    flow = g.maxflow()
    _REF[key] = (flow, g.labels().astype(bool).reshape(shape))
    return _REF[key]


def _set_forms(g, forms):
    if forms == "large_volume_forms":
        from conftest import LARGE_VOLUME_FORMS
        for kv in LARGE_VOLUME_FORMS.split(","):
            name, v = kv.split("=")
            g.set_param(name, int(v))


def _handle(shape, conn, nw, fg=None, bg=None, feature=None, boundary=None):
    """an unbuilt handle: markers, n-links, the feature image and / or a built-in boundary term on an image of its own"""
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph(shape, connectivity=conn)
    if boundary is not None:
        g._set_boundary("difference_linear", boundary, None, False)
    if feature is not None:
        g._set_feature_image(feature)
    if fg is not None or bg is not None:
        g._set_markers(fg, bg)
    for o, (there, back) in (nw or {}).items():
        g._add_nweights(o, there, back)
    return g


def _built(g, forms):
    g._build()
    _set_forms(g, forms)
    return g


def _assert_cut(g, flow_ref, labels_ref):
    from medpy_amd import _lib
    flow = g.maxflow()
    v = g.validate()
    print("flow %r (BK %r), %d voxels differ, %d in the foreground, pair error %g, node error %g" % (
        flow, flow_ref, int((g.labels() != labels_ref).sum()), int(labels_ref.sum()), v["max_pair_error"], v["max_node_error"]))
    np.testing.assert_array_equal(g.labels(), labels_ref)
    assert flow == pytest.approx(flow_ref, rel=1e-9, abs=1e-300)
    assert not any(v[k] for k in _lib.VIOLATION_KEYS), v
    assert v["max_pair_error"] <= 1e-9 and v["max_node_error"] <= 1e-9, v
    return flow


def _merged(shape, calls):
    from medpy_amd.graphcut.graph import merge_tweights_into
    n = int(np.prod(shape))
    tr, fc = np.zeros(n), 0.0
    for s, k in calls:
        fc = merge_tweights_into(tr, fc, np.arange(n), np.asarray(s, np.float64).ravel(), np.asarray(k, np.float64).ravel())
    return tr, fc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.int64).tolist()


# ---- 1. histograms equal numpy.bincount exactly ----------------------------------------------------------------------------------
def _hist_image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return rng.normal(10.0, 4.0, shape).astype(dtype)
    if dtype.itemsize == 8:   # values beyond 2^53, where neighbouring integers share a double
        base = 2 ** 60 if dtype.kind == "u" else -2 ** 60
        return (base + rng.integers(0, 2 ** 20, shape) * 1024).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(max(info.min, -3000), min(info.max, 3000), shape, endpoint=True).astype(dtype)


def _expected(img, fg, bg, nbins, lo, width):
    x = np.floor((img.astype(np.float64) - lo) / width)
    b = np.clip(x, 0, nbins - 1).astype(np.int64)
    hists, out4 = [], [0, 0, 0, 0]
    for k, m in enumerate((fg, bg)):
        if m is None:
            hists.append(np.zeros(nbins, np.int64))
            continue
        m = np.asarray(m, bool)
        hists.append(np.bincount(b[m], minlength=nbins).astype(np.int64))
        out4[k] = int(m.sum())
        out4[2] += int((x[m] < 0).sum())
        out4[3] += int((x[m] > nbins - 1).sum())
    return hists[0], hists[1], out4


def _check_hist(g, img, fg, bg, nbins, lo, width):
    fg_hist, bg_hist = g.marker_histograms(nbins, lo, width)
    want_fg, want_bg, out4 = _expected(img, fg, bg, nbins, lo, width)
    assert fg_hist.dtype == bg_hist.dtype == np.int64 and fg_hist.size == bg_hist.size == nbins
    np.testing.assert_array_equal(fg_hist, want_fg)
    np.testing.assert_array_equal(bg_hist, want_bg)
    info = g.marker_histogram_info()
    assert [info[k] for k in ("fg_voxels", "bg_voxels", "below", "above")] == out4, (info, out4)
    return out4


def _bin_counts():
    from medpy_amd import _lib
    t = _lib.BINNED_LDS_MAX
    return [1, 7, 256, t - 1, t, t + 1, 65536]


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=[np.dtype(d).name for d in ALL_DTYPES])
def test_histograms_equal_bincount(dtype, forms):
    """all ten dtypes; 10 % random markers with voxels under both; every bin count around the LDS threshold; a range that leaves
    values outside on both sides (clamped, and counted); volumes that are no multiple of 16 voxels, and one below 16.  Before
    mgc_build: the call needs no built graph."""
    from medpy_amd.graphcut import VoxelGraph
    for shape in ((17, 16, 31), (9, 8, 7), (3, 1, 5)):
        rng = np.random.default_rng(41)
        img = _hist_image(shape, dtype, 7)
        fg, bg = rng.random(shape) < 0.1, rng.random(shape) < 0.1
        fg.ravel()[[0, -1]] = True   # the first voxel and the last one (the tail behind the last wide load)
        bg.ravel()[np.flatnonzero(fg.ravel())[:3]] = True   # voxels under both
        g = VoxelGraph(shape)
        _set_forms(g, forms)
        g._set_feature_image(img)
        g._set_markers(fg, bg)
        mn, mx = float(img.min()), float(img.max())
        span = (mx - mn) or 1.0
        for nbins in _bin_counts():
            out4 = _check_hist(g, img, fg, bg, nbins, mn + 0.3 * span, 0.4 * span / nbins)   # the outer three tenths lie outside
            if img.size > 1000:
                assert out4[2] > 0 and out4[3] > 0
            _check_hist(g, img, fg, bg, nbins, mn, span / nbins)
        g.close()


@pytest.mark.parametrize("forms", FORMS)
def test_histograms_under_contention_without_a_plane_and_after_edits(forms):
    from medpy_amd.graphcut import VoxelGraph
    from medpy_amd import _lib
    shape = (17, 16, 31)
    n = int(np.prod(shape))
    img = np.random.default_rng(3).integers(0, 5, shape).astype(np.uint8)   # five values: every count lands on a few bins
    every = np.ones(shape, bool)
    g = VoxelGraph(shape)
    g._set_feature_image(img)
    g._set_markers(every, every)   # markers on every voxel
    for nbins in (7, _lib.BINNED_LDS_MAX + 1):
        out4 = _check_hist(g, img, every, every, nbins, 0.0, 1.0)
        assert out4[:2] == [n, n]
    g._set_markers(None, every)   # no fg plane at all
    for nbins in (7, _lib.BINNED_LDS_MAX + 1):
        assert _check_hist(g, img, None, every, nbins, 0.0, 1.0)[:2] == [0, n]
    g._set_markers(None, None)    # no plane of either kind
    assert _check_hist(g, img, None, None, 7, 0.0, 1.0) == [0, 0, 0, 0]
    g.close()
    # a built and solved graph: the same counts on a second call, and the edited masks after edit_markers
    img = _image(shape, "i16")
    fg, bg = _markers(shape)
    g = _built(_handle(shape, None, _nweights(shape, None), fg, bg, feature=img), forms)
    binning = (64, -250.0, 12.5)
    first = g.marker_histograms(*binning)
    g.maxflow()
    labels0, bytes0 = g.labels().copy(), g.stats()["device_bytes"]
    again = g.marker_histograms(*binning)
    assert first[0].tolist() == again[0].tolist() and first[1].tolist() == again[1].tolist()
    _check_hist(g, img, fg, bg, *binning)
    assert np.array_equal(g.labels(), labels0) and g.stats()["device_bytes"] == bytes0   # the call changed nothing on the handle
    add = np.array([5, 400, n - 2], np.int64)
    erase = np.flatnonzero(fg.ravel())[:2]
    g.edit_markers(fg=add, erase=erase)
    fg1 = fg.copy()
    fg1.ravel()[erase] = False
    fg1.ravel()[add] = True
    bg1 = bg.copy()
    bg1.ravel()[erase] = False
    got_fg, got_bg = g.markers()
    assert np.array_equal(got_fg, fg1) and np.array_equal(got_bg, bg1)
    _check_hist(g, img, fg1, bg1, *binning)
    g.close()


# ---- 2. binned equals expanded ---------------------------------------------------------------------------------------------------
def _assert_same_graph(a, b):
    """two built handles hold the same t-links bit for bit, and solve to the same flow (bit for bit) and labels"""
    from medpy_amd import _lib
    assert _bits(a.tweights()) == _bits(b.tweights())
    fa, fb = a.maxflow(), b.maxflow()
    assert fa == fb, (fa, fb)
    np.testing.assert_array_equal(a.labels(), b.labels())
    for g in (a, b):
        v = g.validate()
        assert not any(v[k] for k in _lib.VIOLATION_KEYS), v
    assert a.tweight_edit_info() == b.tweight_edit_info()


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_binned_equals_expanded(shape, conn, forms):
    nw = _nweights(shape, conn)
    fg, bg = _markers(shape)
    rng = np.random.default_rng(29)
    dense1 = (rng.uniform(0.0, 2.0, shape), rng.uniform(0.0, 2.0, shape).astype(np.float32).astype(np.float64))
    dense2 = (rng.uniform(0.0, 2.0, shape), rng.uniform(0.0, 2.0, shape))
    for kind in KINDS:
        img = _image(shape, kind)
        t = _term(img, fg, bg, BINS[kind], lam=1.5)
        neg = (t["tables"][0] - 1.0, t["tables"][1] - 2.5)   # negative table entries
        for name, tables, before, after in (("plain", t["tables"], (), ()), ("call order", t["tables"], (dense1,), (dense2,)), ("negative", neg, (), ())):
            a = _handle(shape, conn, nw, fg, bg, feature=img)
            b = _handle(shape, conn, nw, fg, bg)
            for g in (a, b):
                for s, k in before:
                    g._add_tweights(s, k)
            a._add_tweights_binned(tables[0], tables[1], *t["binning"])
            b._add_tweights(tables[0][t["bins"]], tables[1][t["bins"]])
            for g in (a, b):
                for s, k in after:
                    g._add_tweights(s, k)
            assert a.tweight_edit_info()["dense_calls"] == 1 + len(before) + len(after)
            print(kind, name)
            _assert_same_graph(_built(a, forms), _built(b, forms))
            # ... and, where no marker lies on top, bit for bit the host merge of the expanded arrays
            tr, _ = _merged(shape, list(before) + [(tables[0][t["bins"]], tables[1][t["bins"]])] + list(after))
            free = ~(fg | bg).ravel()
            np.testing.assert_array_equal(np.asarray(_bits(a.tweights()))[free], tr.view(np.int64)[free])
            a.close()
            b.close()
    # the boundary term's own image where no feature image is set -- and a feature image that differs from the boundary image
    other = _image(shape, "i16", seed=77)
    img = _image(shape, "u8")
    for feature, read in ((None, other), (img, img)):
        t = _term(read, fg, bg, 16, lam=2.0)
        a = _handle(shape, conn, nw, fg, bg, feature=feature, boundary=other)
        b = _handle(shape, conn, nw, fg, bg, boundary=other)
        a._add_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"])
        b._add_tweights(t["S"], t["K"])
        _assert_same_graph(_built(a, forms), _built(b, forms))
        a.close()
        b.close()


# ---- 3. against BK ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_device_fitted_term_against_bk(shape, conn, kind, forms):
    """histograms counted on the device, tables by histogram_tables, expanded on the device: BK's cut of the arrays expanded on
    the host"""
    from medpy_amd.graphcut import histogram_tables
    nw = _nweights(shape, conn)
    fg, bg = _markers(shape)
    img = _image(shape, kind)
    t = _term(img, fg, bg, BINS[kind], lam=_lam(conn))
    g = _handle(shape, conn, nw, fg, bg, feature=img)
    fg_hist, bg_hist = g.marker_histograms(*t["binning"])
    assert fg_hist.tolist() == t["fg_hist"].tolist() and bg_hist.tolist() == t["bg_hist"].tolist()
    s, k = histogram_tables(fg_hist, bg_hist, lam=_lam(conn))
    g._add_tweights_binned(s, k, *t["binning"])
    _built(g, forms)
    flow_ref, labels_ref = _bk(("cold", shape, conn, kind), shape, nw, [(t["S"], t["K"])], fg, bg)
    assert labels_ref.sum() > fg.sum()   # the foreground is larger than the marker box
    _assert_cut(g, flow_ref, labels_ref)
    g.close()


# ---- 4. warm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("shape,conn", CASES, ids=CASE_IDS)
def test_warm_update_equals_cold_and_bk(shape, conn, forms):
    kind = _kind_of(shape, conn)
    nw = _nweights(shape, conn)
    fg, bg = _markers(shape)
    img = _image(shape, kind)
    t0 = _term(img, fg, bg, BINS[kind], lam=_lam(conn))
    t1 = _term(img, fg, bg, BINS[kind], lam=2.5 * _lam(conn), eps=0.1)
    binning = t0["binning"]
    g = _handle(shape, conn, nw, fg, bg, feature=img)
    g._add_tweights_binned(t0["tables"][0], t0["tables"][1], *binning)
    _built(g, forms)
    _assert_cut(g, *_bk(("cold", shape, conn, kind), shape, nw, [(t0["S"], t0["K"])], fg, bg))
    build_ms = g.stats()["build_ms"]
    g.update_tweights_binned(t1["tables"][0], t1["tables"][1], *binning)
    info = g.tweight_edit_info()
    tr0, _ = _merged(shape, [(t0["S"], t0["K"])])
    tr1, _ = _merged(shape, [(t1["S"], t1["K"])])
    assert info["store_held"] == 1 and info["dense_calls"] == 1
    assert info["voxels_changed"] == int((tr0.view(np.int64) != tr1.view(np.int64)).sum()) > 0
    ref = _bk(("warm", shape, conn, kind), shape, nw, [(t1["S"], t1["K"])], fg, bg)
    flow = _assert_cut(g, *ref)
    stats = g.stats()
    assert stats["build_ms"] == build_ms and stats["update_ms"] > 0.0   # folded into the residual graph: mgc_build did not run again
    cold = _handle(shape, conn, nw, fg, bg, feature=img)
    cold._add_tweights_binned(t1["tables"][0], t1["tables"][1], *binning)
    _built(cold, forms)
    assert cold.maxflow() == pytest.approx(flow, rel=1e-9) and np.array_equal(cold.labels(), g.labels())
    assert _bits(g.tweights()) == _bits(cold.tweights())
    cold.close()
    # exactly what update_tweights_dense of the expanded arrays leaves
    dense = _handle(shape, conn, nw, fg, bg)
    dense._add_tweights(t0["S"], t0["K"])
    _built(dense, forms)
    dense.maxflow()
    dense.update_tweights_dense(t1["S"], t1["K"])
    assert dense.tweight_edit_info() == info and _bits(dense.tweights()) == _bits(g.tweights())
    assert dense.maxflow() == pytest.approx(flow, rel=1e-9) and np.array_equal(dense.labels(), g.labels())
    dense.close()
    # the same tables again: nothing changes bitwise; and back to the first tables: the first cut
    g.update_tweights_binned(t1["tables"][0], t1["tables"][1], *binning)
    assert g.tweight_edit_info()["voxels_changed"] == 0
    _assert_cut(g, *ref)
    g.update_tweights_binned(t0["tables"][0], t0["tables"][1], *binning)
    _assert_cut(g, *_bk(("cold", shape, conn, kind), shape, nw, [(t0["S"], t0["K"])], fg, bg))
    g.close()


def test_warm_update_gives_a_handle_its_first_store():
    shape, kind = (17, 9, 10), "u8"
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    img = _image(shape, kind)
    t = _term(img, fg, bg, BINS[kind])
    g = _built(_handle(shape, None, nw, fg, bg, feature=img), "as_shipped")
    _assert_cut(g, *_bk(("first_store", shape), shape, nw, (), fg, bg))
    assert g.tweight_edit_info()["store_held"] == 0
    g.update_tweights_binned(t["tables"][0], t["tables"][1], *t["binning"])
    assert g.tweight_edit_info()["store_held"] == 1
    _assert_cut(g, *_bk(("cold", shape, None, kind), shape, nw, [(t["S"], t["K"])], fg, bg))
    g.close()


# ---- 5. the public round ---------------------------------------------------------------------------------------------------------
def _stroke(shape, labels, fg, bg):
    """three voxels of the background side that hold no marker: the stroke that claims them for the foreground"""
    free = np.flatnonzero(~labels.ravel() & ~bg.ravel() & ~fg.ravel())
    return np.unique(free[[0, free.size // 2, free.size - 1]])


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("shape,kind", [((9, 8, 7), "u8"), ((17, 9, 10), "i16"), ((1, 1, 17), "f32"), ((17, 16, 31), "f32")],
                         ids=["9x8x7_u8", "17x9x10_i16", "1x1x17_f32", "17x16x31_f32"])
def test_public_round(shape, kind, forms, monkeypatch):
    from conftest import LARGE_VOLUME_FORMS
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel
    if forms == "large_volume_forms":
        monkeypatch.setenv("MEDPY_HIP_PARAMS", LARGE_VOLUME_FORMS)
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    img = _image(shape, kind)
    lam, eps = 1.5, 0.5
    weights = [nw[o] for o in _offsets(len(shape), None)]
    g = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_histogram, regional_term_args=(img, BINS[kind], lam, eps),
                                   boundary_term=energy_voxel.boundary_precomputed, boundary_term_args=(weights,))
    info = g.tweight_edit_info()
    assert info["store_held"] == 1 and info["dense_calls"] == 1   # the store, filled on the device: not the host merge
    t0 = _term(img, fg, bg, BINS[kind], lam, eps)
    flow0, labels0 = _bk(("public", shape, kind, 0), shape, nw, [(t0["S"], t0["K"])], fg, bg)
    _assert_cut(g, flow0, labels0)
    previous = g.labels().copy()
    stroke = _stroke(shape, labels0, fg, bg)
    g.edit_markers(fg=stroke)
    fg_hist, bg_hist = g.refit_regional_histogram()
    fg1 = fg.copy()
    fg1.ravel()[stroke] = True
    t1 = _term(img, fg1, bg, BINS[kind], lam, eps)
    assert fg_hist.tolist() == t1["fg_hist"].tolist() and bg_hist.tolist() == t1["bg_hist"].tolist()
    flow1, labels1 = _bk(("public", shape, kind, 1), shape, nw, [(t1["S"], t1["K"])], fg1, bg)
    _assert_cut(g, flow1, labels1)
    assert labels1.ravel()[stroke].all() and (labels1 != labels0).any()
    out = g.labels(out=previous)
    assert out is previous and np.array_equal(previous, labels1)
    g.close()


@pytest.mark.parametrize("forms", FORMS)
def test_public_round_on_a_built_in_boundary_term(forms, monkeypatch):
    """boundary_difference_exponential on a float image, the oracle's n-links through oracle.pipeline: the term reads the boundary
    term's own resident image (no second upload)"""
    from conftest import LARGE_VOLUME_FORMS
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel
    from oracle import pipeline
    if forms == "large_volume_forms":
        monkeypatch.setenv("MEDPY_HIP_PARAMS", LARGE_VOLUME_FORMS)
    shape, sigma, lam, eps, bins = (17, 9, 10), 1.5, 0.5, 0.5, 16
    n = int(np.prod(shape))
    fg, bg = _markers(shape)
    img = _image(shape, "f32")
    img[:9, :5, :5] += 2.0   # a brighter block around the fg box
    none = np.zeros(shape, bool)

    def oracle(key, fg_mask, t):
        graph = pipeline.build_graph(none, none, term="difference_exponential", image=img, sigma=sigma)   # the n-links, no markers yet
        return _bk(key, shape, None, [(t["S"], t["K"])], fg_mask, bg, graph=graph)
    g = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_histogram, regional_term_args=(img, bins, lam, eps),
                                   boundary_term=energy_voxel.boundary_difference_exponential, boundary_term_args=(img, sigma, False))
    bytes_own = g.stats()["device_bytes"]
    t0 = _term(img, fg, bg, bins, lam, eps)
    flow0, labels0 = oracle(("builtin", 0), fg, t0)
    assert labels0.sum() > fg.sum()
    _assert_cut(g, flow0, labels0)
    previous = g.labels().copy()
    stroke = _stroke(shape, labels0, fg, bg)
    g.edit_markers(fg=stroke)
    g.refit_regional_histogram()
    fg1 = fg.copy()
    fg1.ravel()[stroke] = True
    flow1, labels1 = oracle(("builtin", 1), fg1, _term(img, fg1, bg, bins, lam, eps))
    _assert_cut(g, flow1, labels1)
    assert np.array_equal(g.labels(out=previous), labels1)
    g.close()
    # the same call with a copy of the image as the term's: a feature image goes up (4 bytes per voxel more), the same cut
    g = graphcut.graph_from_voxels(fg, bg, regional_term=energy_voxel.regional_histogram, regional_term_args=(img.copy(), bins, lam, eps),
                                   boundary_term=energy_voxel.boundary_difference_exponential, boundary_term_args=(img, sigma, False))
    assert g.stats()["device_bytes"] == bytes_own + 4 * n
    _assert_cut(g, flow0, labels0)
    g.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_offender_and_change_nothing():
    from medpy_amd import _lib
    lib = _lib.load()
    shape, kind = (9, 8, 7), "f32"
    n = int(np.prod(shape))
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    img = _image(shape, kind)
    t = _term(img, fg, bg, BINS[kind])
    nbins, lo, width = t["binning"]
    s, k = t["tables"]
    g = _handle(shape, None, nw, fg, bg, feature=img)
    g._add_tweights_binned(s, k, nbins, lo, width)
    _built(g, "as_shipped")
    ref = _bk(("cold", shape, None, kind), shape, nw, [(t["S"], t["K"])], fg, bg)
    flow0 = _assert_cut(g, *ref)
    state0 = (_bits(g.tweights()), g.tweight_edit_info(), g.stats()["device_bytes"])
    fgh, bgh, out4 = np.zeros(nbins, np.int64), np.zeros(nbins, np.int64), np.zeros(4, np.int64)

    def calls(nb, lo_, w_, st, kt):
        p = [None if a is None else _lib.ptr(a) for a in (st, kt)]
        return (("mgc_add_tweights_binned", lambda: lib.mgc_add_tweights_binned(g._h, nb, lo_, w_, p[0], p[1])),
                ("mgc_update_tweights_binned", lambda: lib.mgc_update_tweights_binned(g._h, nb, lo_, w_, p[0], p[1])))

    def unchanged():
        assert (_bits(g.tweights()), g.tweight_edit_info(), g.stats()["device_bytes"]) == state0
        assert g.maxflow() == flow0 and np.array_equal(g.labels(), ref[1])   # still built, the finished solve still there

    def refused(name, call, code, *names):
        rc = call()
        msg = lib.mgc_last_error(g._h).decode()
        assert rc == code, (name, rc, msg)
        assert name in msg and all(x in msg for x in names), msg
        unchanged()
    # the binning out of range: all three calls
    big = np.zeros(65537)
    for nb, lo_, w_, what in ((0, lo, width, "nbins"), (65537, lo, width, "nbins"), (-1, lo, width, "nbins"), (nbins, np.nan, width, "lo"),
                              (nbins, np.inf, width, "lo"), (nbins, lo, 0.0, "width"), (nbins, lo, -1.0, "width"), (nbins, lo, np.inf, "width"),
                              (nbins, lo, np.nan, "width")):
        for name, call in calls(nb, lo_, w_, big, big):
            refused(name, call, _lib.ERR_INVALID, what)
        refused("mgc_marker_histograms", lambda: lib.mgc_marker_histograms(g._h, nb, lo_, w_, _lib.ptr(fgh), _lib.ptr(bgh), _lib.ptr(out4)), _lib.ERR_INVALID, what)
    # a NULL table, a table entry that is not finite (the first offender is named; negative entries are fine)
    for name, call in calls(nbins, lo, width, None, k):
        refused(name, call, _lib.ERR_INVALID, "source_table NULL")
    for name, call in calls(nbins, lo, width, s, None):
        refused(name, call, _lib.ERR_INVALID, "sink_table NULL")
    for which, idx, value in (("source_table", nbins - 1, np.nan), ("sink_table", 0, np.inf), ("source_table", 3, -np.inf), ("sink_table", 5, np.nan)):
        s1, k1 = s.copy(), k.copy()
        (s1 if which == "source_table" else k1)[idx] = value
        if idx < nbins - 1:
            (k1 if which == "source_table" else s1)[nbins - 1] = np.nan   # a later offender in the other table: not the one named
        for name, call in calls(nbins, lo, width, s1, k1):
            refused(name, call, _lib.ERR_INVALID, "%s[%d]" % (which, idx))
    refused("mgc_marker_histograms", lambda: lib.mgc_marker_histograms(g._h, nbins, lo, width, None, _lib.ptr(bgh), None), _lib.ERR_INVALID, "NULL")
    # a value of a float feature image that is not finite: flat index and value are named
    last = n - 1   # (odd n: the entry behind the last whole vector)
    under_fg = int(np.flatnonzero(fg.ravel())[0])
    for idx, value, text in ((last, np.nan, "nan"), (under_fg, np.inf, "inf"), (3, -np.inf, "-inf")):
        bad = img.copy()
        bad.ravel()[idx] = value
        if idx != last:
            bad.ravel()[last] = np.nan   # a later offender: not the one named
        g._set_feature_image(bad)
        for name, call in calls(nbins, lo, width, s, k):
            refused(name, call, _lib.ERR_INVALID, "image[%d] = %s" % (idx, text))
        hist = lambda: lib.mgc_marker_histograms(g._h, nbins, lo, width, _lib.ptr(fgh), _lib.ptr(bgh), _lib.ptr(out4))   # noqa: E731
        if fg.ravel()[idx] or bg.ravel()[idx] or bg.ravel()[last]:   # the histograms look only under the markers
            first = idx if (fg.ravel()[idx] or bg.ravel()[idx]) else last
            refused("mgc_marker_histograms", hist, _lib.ERR_INVALID, "image[%d]" % first)
        else:
            assert hist() == _lib.OK
    g._set_feature_image(img)
    unchanged()
    # the same checks on a float64 image held as the boundary term's (no feature image)
    h2 = _handle(shape, None, nw, fg, bg, boundary=img.astype(np.float64))
    bad = img.astype(np.float64)
    bad.ravel()[4] = np.nan
    h3 = _handle(shape, None, nw, fg, bg, boundary=bad)
    assert lib.mgc_add_tweights_binned(h2._h, nbins, lo, width, _lib.ptr(s), _lib.ptr(k)) == _lib.OK
    assert lib.mgc_add_tweights_binned(h3._h, nbins, lo, width, _lib.ptr(s), _lib.ptr(k)) == _lib.ERR_INVALID
    assert "image[4] = nan" in lib.mgc_last_error(h3._h).decode() and h3.tweight_edit_info()["store_held"] == 0
    h2.close()
    h3.close()
    g.close()


def test_states_and_feature_image_bytes():
    from medpy_amd import _lib
    from medpy_amd.graphcut import VoxelGraph
    lib = _lib.load()
    shape = (9, 8, 7)
    n = int(np.prod(shape))
    nw = _nweights(shape, None)
    fg, bg = _markers(shape)
    img = _image(shape, "i16")
    t = _term(img, fg, bg, 7)
    nbins, lo, width = t["binning"]
    s, k = t["tables"]
    fgh, bgh = np.zeros(nbins, np.int64), np.zeros(nbins, np.int64)

    def add(g):
        return lib.mgc_add_tweights_binned(g._h, nbins, lo, width, _lib.ptr(s), _lib.ptr(k))

    def update(g):
        return lib.mgc_update_tweights_binned(g._h, nbins, lo, width, _lib.ptr(s), _lib.ptr(k))

    def hist(g):
        return lib.mgc_marker_histograms(g._h, nbins, lo, width, _lib.ptr(fgh), _lib.ptr(bgh), None)
    # no feature image and no boundary image
    g = _handle(shape, None, nw, fg, bg)
    bytes0 = g.stats()["device_bytes"]
    for call in (add, hist):
        assert call(g) == _lib.ERR_STATE and b"no feature image" in lib.mgc_last_error(g._h)
    assert g.tweight_edit_info()["store_held"] == 0 and g.stats()["device_bytes"] == bytes0
    # the feature image is counted in device_bytes, NULL gives the bytes back; a wider dtype takes more
    g._set_feature_image(img)
    assert g.stats()["device_bytes"] == bytes0 + 2 * n
    g._set_feature_image(img.astype(np.float64))
    assert g.stats()["device_bytes"] == bytes0 + 8 * n
    g._set_feature_image(None)
    assert g.stats()["device_bytes"] == bytes0 and hist(g) == _lib.ERR_STATE
    g._set_feature_image(None)   # twice is fine
    g._set_feature_image(img)
    assert lib.mgc_set_feature_image(g._h, _lib.ptr(img), 99) == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        g._set_feature_image(img[:-1])
    # before mgc_build: the histograms and the add are valid, the update is not
    assert hist(g) == _lib.OK and fgh.tolist() == t["fg_hist"].tolist() and bgh.tolist() == t["bg_hist"].tolist()
    assert update(g) == _lib.ERR_STATE and b"before mgc_build" in lib.mgc_last_error(g._h)
    assert g.tweight_edit_info()["store_held"] == 0
    # the store and mgc_set_tweights_merged are exclusive, both ways
    assert add(g) == _lib.OK and b"expand_ms" in lib.mgc_last_error(g._h)
    tr = np.ascontiguousarray((t["S"] - t["K"]).ravel())
    assert lib.mgc_set_tweights_merged(g._h, _lib.ptr(tr), 0.0) == _lib.ERR_STATE
    g._clear_tweights()
    g._set_tweights_merged(tr, 1.5)
    assert add(g) == _lib.ERR_STATE and b"mgc_set_tweights_merged" in lib.mgc_last_error(g._h)
    g._build()
    assert update(g) == _lib.ERR_STATE and b"mgc_set_tweights_merged" in lib.mgc_last_error(g._h)
    assert g.tweight_edit_info()["store_held"] == 0
    with pytest.raises(NotImplementedError):   # ... and the Python layer refuses before the library is asked
        g.update_tweights_binned(s, k, nbins, lo, width)
    g._clear_tweights()
    assert add(g) == _lib.OK
    g._build()
    assert update(g) == _lib.OK and b"fold_ms" in lib.mgc_last_error(g._h)
    # a built handle stays built when the feature image is replaced
    g.maxflow()
    g._set_feature_image(img)
    g.maxflow()
    g.close()
    # a VoxelGraph that was built without the term has no binning to fall back on
    g = VoxelGraph(shape)
    with pytest.raises(ValueError):
        g.refit_regional_histogram()
    g.close()


def test_no_update_after_a_solve_that_did_not_converge():
    from medpy_amd import _lib, graphcut, synthetic
    sph = synthetic.sphere((96, 96, 96))   # (the volume test_gpu_warm_resolve.py stops after one outer round)
    g = graphcut.graph_from_voxels(sph["fg"], sph["bg"], boundary_term=getattr(graphcut.energy_voxel, "boundary_" + sph["term"]),
                                   boundary_term_args=(sph["image"], sph["sigma"], False))
    g.set_param("max_outer", 1)
    with pytest.raises(_lib.MedpyHipError):
        g.maxflow()
    bytes0 = g.stats()["device_bytes"]
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.update_tweights_binned(np.zeros(8), np.ones(8), 8, 0.0, 0.125)
    assert ei.value.code == _lib.ERR_STATE and g.tweight_edit_info()["store_held"] == 0 and g.stats()["device_bytes"] == bytes0
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
    s, k = np.zeros(8), np.ones(8)
    fgh, bgh = np.zeros(8, np.int64), np.zeros(8, np.int64)
    for sl in slabs:
        for build in (False, True):
            if build:
                sl.build()
            image = np.ascontiguousarray(sph["image"][sl.plane0:sl.plane1])
            for rc in (lib.mgc_add_tweights_binned(sl._h, 8, 0.0, 0.125, _lib.ptr(s), _lib.ptr(k)),
                       lib.mgc_update_tweights_binned(sl._h, 8, 0.0, 0.125, _lib.ptr(s), _lib.ptr(k)),
                       lib.mgc_marker_histograms(sl._h, 8, 0.0, 0.125, _lib.ptr(fgh), _lib.ptr(bgh), None),
                       lib.mgc_set_feature_image(sl._h, _lib.ptr(image), _lib.DTYPE_IDS[image.dtype])):
                assert rc == _lib.ERR_UNSUPPORTED and b"slab" in lib.mgc_last_error(sl._h)

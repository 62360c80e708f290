"""-m gpu: the Z-slab path (mgc_create_slab, ghost tile layers, halo messages, mgc_solve_slabs, mgc_finish) at its edges, on ONE MI355X.

(a) the split: HipSlab's planes are slab_cases.slab_spec's on every geometry; more slabs than tile layers and 2-D volumes are refused.
(b) what each slab STORES: mgc_get_nweights_offset, mgc_get_tweights and mgc_get_edge of a slab handle, built as graphcut_voxel_slabs builds
it, against a single handle over the whole volume (slab_cases.check_slab_build): every geometry x the eight terms x float32 / int16 x with
and without spacing x both neighbourhoods; with a regional term (the pre-push instances); with one workgroup building every tile.
(c) what the group CUTS: labels, flow and invariants against the single handle and BK, one term of each kind, again with one record slot
per border message and again with the one-wave-per-tile kernels forced (volumes this small run the workgroup forms otherwise).
(d) an exact family (dyadic capacities): flow == BK's, conservation errors 0.0, and the residuals of every neighbour pair of the volume,
assembled from the slabs that own their tails, add up to the pair's capacities.
tests/test_slab_cases_host.py shows on the CPU that the comparison of (b) rejects the builds it is there to catch, and establishes
which cases of (c) have a unique minimum cut."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import full_nb_cases as fc
import slab_cases as sc
from oracle import energy_numpy, pipeline

pytestmark = pytest.mark.gpu

SHAPES = sorted({g[0] for g in sc.GEOMETRIES})
SLAB_COUNTS = {shape: [n for s, n in sc.GEOMETRIES if s == shape] for shape in SHAPES}


# ---- handles ---------------------------------------------------------------------------------------------------------------------------

def _slabs(shape, nslabs, conn, term, image, spacing, regional=None, params=(), fg=None, bg=None):
    """the slabs of one volume, built as medpy_amd.slab.graphcut_voxel_slabs builds them"""
    from medpy_amd.slab import HipSlab, LoopbackExchange, sync_boundary_table, sync_image_range
    x = sc.inputs(shape)
    fg, bg = (x["fg"] if fg is None else fg), (x["bg"] if bg is None else bg)
    slabs = [HipSlab(shape, r, nslabs, connectivity=conn) for r in range(nslabs)]
    for s in slabs:
        for k, v in params:
            s.set_param(k, v)
        z = slice(s.plane0, s.plane1)
        s.set_boundary(term, image[z], fc.sigma_of(term), spacing)
        if regional is not None:
            s.set_regional(np.asarray(regional[0])[z], regional[1])
        s.set_markers(fg[z], bg[z])
    ex = LoopbackExchange(slabs)
    if term.endswith("linear"):
        sync_image_range(slabs, ex)
    sync_boundary_table(slabs, ex)
    for s in slabs:
        s.build()
    return slabs, ex


def _single(shape, conn, term, image, spacing, regional=None, params=(), fg=None, bg=None):
    from medpy_amd.graphcut.graph import VoxelGraph
    x = sc.inputs(shape)
    g = VoxelGraph(shape, connectivity=conn)
    g._set_boundary(term, image, fc.sigma_of(term), spacing)
    if regional is not None:
        g._set_regional(regional[0], regional[1])
    g._set_markers(x["fg"] if fg is None else fg, x["bg"] if bg is None else bg)
    for k, v in params:
        g.set_param(k, v)
    g._build()
    return g


def _nweights_offset(s):
    from medpy_amd import _lib

    def read(o):
        out = np.empty(s.local_shape, dtype=np.float64)
        s._call("mgc_get_nweights_offset", (C.c_int * 3)(*[int(v) for v in o]), _lib.ptr(out))
        return out
    return read


def _tweights(s):
    from medpy_amd import _lib

    def read():
        out = np.empty(s.local_shape, dtype=np.float64)
        s._call("mgc_get_tweights", _lib.ptr(out))
        return out
    return read


def _get_edge(s):
    def read(i, j):
        out = C.c_double(0.0)
        s._call("mgc_get_edge", int(i), int(j), C.byref(out))
        return out.value
    return read


def _compare(shape, conn, term, image, spacing, regional=None, params=(), what="", seed=0):
    """(b) for every slab count of ``shape``: returns (arcs compared, arcs of owned voxels whose stored value is not the weight)"""
    t0 = time.perf_counter()
    arcs = sc.arcs_to_read(shape, conn, seed)
    g = _single(shape, conn, term, image, spacing, regional, params)
    single = sc.read_handle(shape, conn, g.nweights_offset, g.tweights, g.get_edge, arcs)
    g.close()
    compared = moved = calls = 0
    for nslabs in SLAB_COUNTS[shape]:
        slabs, _ = _slabs(shape, nslabs, conn, term, image, spacing, regional, params)
        for r, s in enumerate(slabs):
            spec = sc.slab_spec(shape[0], r, nslabs)
            assert sc.spec_of(s) == spec
            reads = sc.read_handle(s.local_shape, conn, _nweights_offset(s), _tweights(s), _get_edge(s), sc.local_arcs(arcs, spec))
            compared += sc.check_slab_build(reads, single, spec, conn, prepush=regional is not None)
            calls += reads["calls"]
            own = slice(spec["own0"] - spec["plane0"], spec["own1"] - spec["plane0"])
            for o, m in reads["arcs"].items():
                moved += int((sc.bits(reads["fwd"][o][own][m[own]]) != sc.bits(reads["nw"][o][own][m[own]])).sum())
            s.close()
    print("%s: %d stored arcs compared with the single handle's, %d get_edge calls on slabs + %d on the single handle, %.2f s" % (
        what, compared, calls, single["calls"], time.perf_counter() - t0))
    assert compared > 0
    return compared, moved


# ---- (a) the split ---------------------------------------------------------------------------------------------------------------------

def test_slab_geometry_is_the_restatement():
    from medpy_amd import _lib
    from medpy_amd.slab import HipSlab
    for shape, nslabs in sc.GEOMETRIES:
        for conn in sc.CONNS:
            for r in range(nslabs):
                s = HipSlab(shape, r, nslabs, connectivity=conn)
                assert sc.spec_of(s) == sc.slab_spec(shape[0], r, nslabs), (shape, r, nslabs, conn)
                assert s.local_shape == (s.plane1 - s.plane0,) + tuple(shape[1:])
                s.close()
    for shape, nslabs in (((9, 9, 17), 3), ((17, 13, 9), 4), ((24, 8, 8), 4), ((8, 16, 16), 2)):
        with pytest.raises(ValueError):
            sc.slab_spec(shape[0], 0, nslabs)
        for r in range(nslabs):
            with pytest.raises(_lib.MedpyHipError):
                HipSlab(shape, r, nslabs)
    lib = _lib.load()
    for conn in (4, 8):   # a 2-D volume
        h = C.c_void_p()
        rc = lib.mgc_create_slab(2, (C.c_int64 * 3)(16, 16, 0), conn, 0, 0, 2, C.byref(h))
        assert rc != _lib.OK and not h.value


# ---- (b) what each slab stores -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spacing_on", (False, True), ids=("plain", "spacing"))
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("term", sc.TERMS)
@pytest.mark.parametrize("conn", sc.CONNS)
@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_what_each_slab_stores(shape, conn, term, dtype, spacing_on):
    """every slab of every split of ``shape`` against ONE single handle: the weights, the t-links and the stored arcs of owned voxels are
    the single handle's bit for bit (arcs into the ghost planes and the outside markers at the volume's faces included), the ghost planes
    hold what DESIGN 6 says the build leaves there.  float32: exp / pow on the device; int16: the table of the WHOLE volume"""
    image = sc.inputs(shape)[dtype]
    what = "%s %d %s %s %s" % (fc.shape_id(shape), conn, term, dtype, "spacing" if spacing_on else "plain")
    _, moved = _compare(shape, conn, term, image, fc.spacing_of(shape, spacing_on), what=what, seed=conn + spacing_on)
    assert moved == 0


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("term", sc.CUT_TERMS)
@pytest.mark.parametrize("conn", sc.CONNS)
@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_what_each_slab_stores_with_a_regional_term(shape, conn, term, dtype):
    """set_regional: the pre-push instances of the build (k_build<false, .., PRE6> and the 26-neighbourhood's own).  t-links of owned
    planes are the single handle's bit for bit, and so are the STORED ARCS: the pre-push of either neighbourhood moves flow between the
    voxels of one tile and reads nothing outside the tile (mgc_kernels.hip: k_build_tiles, "voxels that hold excess push ... to their
    neighbours inside the tile"), slabs are cut at tile layers, so a slab's tiles -- ghost layers included at the 6-neighbourhood --
    hold the single handle's inputs and get the single handle's pushes.  fn.check_prepush's looser rules are not needed."""
    image = sc.inputs(shape)[dtype]
    what = "%s %d %s %s regional" % (fc.shape_id(shape), conn, term, dtype)
    _, moved = _compare(shape, conn, term, image, False, regional=sc.regional(shape, term), what=what, seed=3)
    assert moved > 0, "%s: no stored arc of an owned voxel differs from its weight: nothing was pre-pushed" % what


@pytest.mark.parametrize("term,dtype", [("difference_division", "float32"), ("maximum_power", "int16")])
@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_what_each_slab_stores_with_probabilities_of_quarters(shape, term, dtype):
    """the 6-neighbourhood pre-push on a map of quarters with alpha 2 (exact t-links; many voxels at 1/2 hold no t-link at all)"""
    what = "%s 6 %s %s quarters" % (fc.shape_id(shape), term, dtype)
    _, moved = _compare(shape, 6, term, sc.inputs(shape)[dtype], False, regional=(sc.quarters(shape), 2.0), what=what, seed=4)
    assert moved > 0, what


@pytest.mark.parametrize("conn", sc.CONNS)
@pytest.mark.parametrize("shape", [(17, 13, 9), (16, 17, 7)], ids=fc.shape_id)
def test_one_workgroup_builds_every_tile_of_a_slab(shape, conn):
    """grid_cap 1 (a build grid of at most 4 workgroups: tile after tile through the same LDS arrays, ghost layers among them): a float32
    and a table instance with spacing, and the pre-push"""
    params = (("grid_cap", 1),)
    for term, dtype in (("difference_exponential", "float32"), ("maximum_power", "int16")):
        what = "%s %d %s %s spacing grid_cap 1" % (fc.shape_id(shape), conn, term, dtype)
        _compare(shape, conn, term, sc.inputs(shape)[dtype], fc.SPACING, params=params, what=what, seed=5)
    what = "%s %d difference_linear float32 regional grid_cap 1" % (fc.shape_id(shape), conn)
    _, moved = _compare(shape, conn, "difference_linear", sc.inputs(shape)["float32"], False, regional=sc.regional(shape, "difference_linear"),
                        params=params, what=what, seed=6)
    assert moved > 0


# ---- (c) what the group cuts -------------------------------------------------------------------------------------------------------------

_SINGLE_CUTS = {}


def _single_cut(shape, conn, term, dtype):
    key = (shape, conn, term, dtype)
    if key not in _SINGLE_CUTS:
        g = _single(shape, conn, term, sc.inputs(shape)[dtype], False)
        flow = g.maxflow()
        _SINGLE_CUTS[key] = (g.labels(), flow)
        g.close()
    return _SINGLE_CUTS[key]


VARIANTS = {"default": "", "one-record-messages": "halo_max_records=1", "wave-kernels": "wave_min_tiles=0"}


@pytest.mark.parametrize("term", sc.CUT_TERMS)
@pytest.mark.parametrize("conn", sc.CONNS)
@pytest.mark.parametrize("geometry", sc.GEOMETRIES, ids=sc.geometry_id)
def test_what_the_group_cuts(geometry, conn, term, monkeypatch):
    """graphcut_voxel_slabs' calls (all slabs in one process: the borders move between the slabs' buffers in HBM, the only loopback the
    library has) on every geometry: labels the single handle's and BK's -- voxel for voxel where test_slab_cases_host.py finds the
    minimum cut unique, inside BK's ambiguity set at equal exact capacity elsewhere --, flow to 1e-9, the invariants of all slabs
    clean with no border flow left in an outbox.  Again with one record slot per border message (MEDPY_HIP_PARAMS, as the mock-RCCL test
    sets it), and with the one-wave-per-tile kernels on every list (by default lists this short go to the workgroup forms).

    20 x 11 x 10 / 2, 24 x 8 x 8 / 3 and 17 x 13 x 9 / 3 under difference_linear at the 6-neighbourhood are where border flow was lost
    (test_slab_cases_host.py): before the fix of the outbox stores these cases ended "converged" with less flow into the sink than the
    cut holds (71.11 against 79.40 on 17 x 13 x 9)."""
    from medpy_amd import _lib
    from medpy_amd.slab import solve_slabs, validate_slabs
    shape, nslabs = geometry
    base = os.environ.get("MEDPY_HIP_PARAMS", "")   # (what the suite as a whole may be run under stays in front)
    for dtype in sc.DTYPES:
        case, ref, unique = sc.reference_cut(shape, conn, term, dtype)
        monkeypatch.setenv("MEDPY_HIP_PARAMS", base)
        single, sflow = _single_cut(shape, conn, term, dtype)
        what = "%s %d %s %s" % (sc.geometry_id(geometry), conn, term, dtype)
        assert sflow == pytest.approx(ref.flow, rel=1e-9), what
        sc.assert_same_cut(single, case, ref, unique, what + ", single handle")
        for name, spec in VARIANTS.items():
            t0 = time.perf_counter()
            monkeypatch.setenv("MEDPY_HIP_PARAMS", ",".join(filter(None, [base, spec])))
            slabs, ex = _slabs(shape, nslabs, conn, term, case["image"], False)
            st = solve_slabs(slabs, ex)
            assert st["converged"] == 1, (what, name, st)
            parts = [s.finish() for s in slabs]
            v = validate_slabs(slabs, ex)
            for s in slabs:
                s.close()
            labels, flow = np.concatenate([p[0] for p in parts], axis=0), float(sum(p[1] for p in parts))
            print("%s, %s: flow %.12g, source side %.3f, unique cut %s, %d exchanges, %d deferred drains, %.2f s" % (
                what, name, flow, labels.mean(), unique, st.get("exchanges", -1), st.get("deferred_drains", -1), time.perf_counter() - t0))
            assert flow == pytest.approx(ref.flow, rel=1e-9), (what, name)
            assert flow == pytest.approx(sflow, rel=1e-9), (what, name)
            assert v["voxels"] == int(np.prod(shape)) and v["pending_outbox"] == 0, (what, name, v)
            _lib.assert_valid(v)
            if unique:
                np.testing.assert_array_equal(labels, single, err_msg="%s, %s: the single handle's labels" % (what, name))
            sc.assert_same_cut(labels, case, ref, unique, "%s, %s" % (what, name))


# ---- (d) an exact family -----------------------------------------------------------------------------------------------------------------

def _family_b(shape, seed=0):
    """session_model.family_b's arithmetic: difference_division, sigma 1, on an image of 0s and 3s (n-links 1 and 1/4), a float32 map of
    quarters with alpha 2, markers of weight 65535 on the end faces of the last axis"""
    import session_model as sm
    rng = np.random.default_rng(2000 + seed)
    last = shape[-1]
    img = np.zeros(shape, np.float32)
    img[..., last // 3:2 * last // 3] = 3.0
    img[rng.random(shape) < 0.1] = 3.0
    prob = (rng.integers(0, 5, shape) / 4.0).astype(np.float32)
    fg, bg = sm._end_faces(shape)
    return img, prob, fg, bg


@pytest.mark.parametrize("conn", sc.CONNS)
@pytest.mark.parametrize("geometry", [((17, 13, 9), 3), ((9, 9, 17), 2)], ids=sc.geometry_id)
def test_exact_family_across_slabs(geometry, conn):
    """every capacity a multiple of 1/4 far below 2^53 quarters: all arithmetic of the solve is exact.  The summed flow IS BK's, both
    conservation errors are 0.0, and the residual graph the slabs leave is a residual graph of the volume: for every neighbour pair
    r(i -> j) + r(j -> i) == c(i -> j) + c(j -> i) exactly, each residual read from the slab that OWNS its tail (pairs across a slab
    border: one end from either slab -- what crossed in a border message was absorbed on the other side before the solve ended),
    and no residual arc leads from the source side of the cut to the sink side."""
    from medpy_amd import _lib
    from medpy_amd.slab import solve_slabs, validate_slabs
    import face_nb_cases as fn
    shape, nslabs = geometry
    img, prob, fg, bg = _family_b(shape)
    ref = pipeline.graphcut_voxel(fg, bg, term="difference_division", image=img, sigma=1.0, connectivity=conn, prob=prob, alpha=2.0)
    term_sigma = fc.SIGMA["division"]
    fc.SIGMA["division"] = 1.0   # (fc.sigma_of is what _slabs asks; family B's sigma)
    try:
        slabs, ex = _slabs(shape, nslabs, conn, "difference_division", img, False, regional=(prob, 2.0), fg=fg, bg=bg)
    finally:
        fc.SIGMA["division"] = term_sigma
    st = solve_slabs(slabs, ex)
    assert st["converged"] == 1
    parts = [s.finish() for s in slabs]
    labels, flow = np.concatenate([p[0] for p in parts], axis=0), float(sum(p[1] for p in parts))
    v = validate_slabs(slabs, ex)
    assert flow == ref.flow
    assert v["max_pair_error"] == 0.0 and v["max_node_error"] == 0.0 and v["pending_outbox"] == 0 and v["voxels"] == int(np.prod(shape)), v
    _lib.assert_valid(v)
    # the residuals, each from the slab that owns its tail
    cap = energy_numpy.boundary_weights_offsets("difference_division", img, sc.offsets(conn), 1.0)
    res_fwd = {o: np.full(shape, np.nan) for o in cap}
    res_back = {o: np.full(shape, np.nan) for o in cap}
    t0, calls = time.perf_counter(), 0
    for s in slabs:
        get_edge, st_local = _get_edge(s), fn.strides(s.local_shape)
        for o, m in sc.every_arc(shape, conn).items():
            step = sum(k * x for k, x in zip(o, st_local))
            for z in range(s.own0, s.own1):   # tails p in plane z: p -> p + o; tails p + o in plane z: (p + o) -> p, p in plane z - o[0]
                for y, x in zip(*np.nonzero(m[z])):
                    i = ((z - s.plane0) * shape[1] + int(y)) * shape[2] + int(x)
                    res_fwd[o][z, y, x] = get_edge(i, i + step)
                    calls += 1
                zp = z - o[0]
                if 0 <= zp < shape[0]:
                    for y, x in zip(*np.nonzero(m[zp])):
                        i = ((zp - s.plane0) * shape[1] + int(y)) * shape[2] + int(x)
                        res_back[o][zp, y, x] = get_edge(i + step, i)
                        calls += 1
        s.close()
    print("%s %d: %d residuals read in %.2f s, flow %r" % (sc.geometry_id(geometry), conn, calls, time.perf_counter() - t0, flow))
    crossing = 0
    for o, c in cap.items():
        src, dst = fc._slices(shape, o)
        m = ~np.isnan(c)
        assert not np.isnan(res_fwd[o][m]).any() and not np.isnan(res_back[o][m]).any(), "offset %s: not every residual was read" % (o,)
        bad = (res_fwd[o][m] + res_back[o][m]) != (c[m] + c[m])
        assert not bad.any(), "offset %s: %d pairs whose residuals do not add up to their capacities, first at %s" % (o, bad.sum(), tuple(int(k[np.flatnonzero(bad)[0]]) for k in np.nonzero(m)))
        assert not (res_fwd[o][m] < 0).any() and not (res_back[o][m] < 0).any()
        tail, head = labels[src], labels[dst]
        f, b = res_fwd[o][src], res_back[o][src]
        assert not (f[tail & ~head] != 0.0).any(), "offset %s: a residual arc leads from the source side to the sink side" % (o,)
        assert not (b[head & ~tail] != 0.0).any(), "offset %s: a residual arc leads from the source side to the sink side" % (o,)
        if o[0]:
            z = np.indices(shape)[0][src]
            crossing += int((((z + 1) % 8 == 0) & (f != c[src])).sum())
    assert crossing > 0, "no flow crossed a tile layer along z: the family does not exercise the borders"
    # the cut itself: BK's value was matched exactly above; the labels are compared where the cut is unique
    from oracle import cutcheck
    if not cutcheck.ambiguity(ref.graph)[2].any():
        np.testing.assert_array_equal(labels, ref.labels)
    else:
        cutcheck.assert_labels_equivalent(labels, ref)

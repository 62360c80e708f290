"""-m gpu: labels and flow of the full neighbourhood on cuts that are NOT the surface of the seed.

The wall inputs of tests/full_nb_cases.py, all eight terms, float32 (no table) and int16 (table for the exp / pow terms), eleven shapes
from one tile to 27, thin volumes with a diagonal offset, singleton axes and 2-D, spacing on for half of them.  Each solved graph is
compared with the oracle twice -- NumPy weights + BK, and BK fed the device's own weights -- flow to 1e-9, mgc_validate sound, labels
identical; on a tie-degenerate case (maximum_* terms, integer image) every differing voxel lies in the reference's ambiguity set and the
two cuts have the same capacity in exact rationals.  tests/test_full_nb_cases_host.py asserts on the CPU that the reference's cut of
every one of these cases holds 10 % to 90 % of the unmarked voxels and that its ambiguity set is at most 5 % of them."""
import numpy as np
import pytest

import full_nb_cases as fc
from oracle import energy_numpy, pipeline

pytestmark = pytest.mark.gpu

W26_FORCED = (("wave_kernels", 41), ("max_cycles", -1))   # k26_discharge_w, forced as tests/test_gpu_schedule_knobs.py forces it


def _graph(case, params=(), image=None, fg=None, bg=None):
    """graph_from_voxels of a case; with ``params`` the same calls on a VoxelGraph, the knobs set before the build (the pre-push acts there)"""
    from medpy_amd import graphcut
    from medpy_amd.graphcut.graph import VoxelGraph
    image = case["image"] if image is None else image
    fg, bg = case["fg"] if fg is None else fg, case["bg"] if bg is None else bg
    if not params:
        kw = dict(boundary_term=getattr(graphcut.energy_voxel, "boundary_" + case["term"]),
                  boundary_term_args=(image, case["spacing"]) if case["sigma"] is None else (image, case["sigma"], case["spacing"]))
        if case["prob"] is not None:
            kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(case["prob"], case["alpha"]))
        return graphcut.graph_from_voxels(fg, bg, connectivity=case["conn"], **kw)
    g = VoxelGraph(case["shape"], connectivity=case["conn"])
    g._set_boundary(case["term"], image, case["sigma"], case["spacing"])
    if case["prob"] is not None:
        g._set_regional(case["prob"], case["alpha"])
    g._set_markers(fg, bg)
    for k, v in params:
        g.set_param(k, v)
    g._build()
    return g


def _solve_and_compare(case, ref, params=(), what="", **inputs):
    """build, read the weights back, solve; against ``ref`` and against BK on the device's weights.  Returns (graph, device weights)"""
    from medpy_amd import _lib
    g = _graph(case, params, **inputs)
    offs = energy_numpy.forward_offsets(len(case["shape"]), case["conn"])
    wdev = {o: g.nweights_offset(o) for o in offs}
    flow = g.maxflow()
    _lib.assert_valid(g.validate())
    labels = g.labels()
    kw = dict(prob=case["prob"], alpha=case["alpha"]) if case["prob"] is not None else {}
    inj = pipeline.graphcut_voxel(case["fg"], case["bg"], weights=wdev, connectivity=case["conn"], **kw)
    wref = fc.expected_weights(case["term"], case["image"], case["spacing"])[1]
    d1 = fc.assert_cut(labels, flow, case, ref, wref, what + " vs oracle")
    d2 = fc.assert_cut(labels, flow, case, inj, wdev, what + " vs BK on the device's weights")
    print("%s: flow %.12g, source side %.3f, %d / %d voxels differ inside the ambiguity set" % (what, flow, labels.mean(), d1, d2))
    return g, wdev


@pytest.mark.parametrize("dtype", fc.DTYPES)
@pytest.mark.parametrize("term", fc.TERMS)
@pytest.mark.parametrize("conn", fc.CONNECTIVITIES, ids="conn{}".format)
def test_wall_cuts(conn, term, dtype):
    for shape, spacing_on in fc.of_connectivity(fc.CUT_SHAPES, conn):
        case, ref = fc.reference(shape, term, dtype, spacing_on)
        what = "conn %d %s %s %s%s" % (case["conn"], term, dtype, fc.shape_id(shape), " spacing" if spacing_on else "")
        g, _ = _solve_and_compare(case, ref, what=what)
        g.close()


@pytest.mark.parametrize("dtype", fc.DTYPES)
@pytest.mark.parametrize("term", fc.TERMS)
def test_wall_cuts_through_the_wave_discharge(term, dtype):
    """k26_discharge_w is what a volume the size of BASELINE config 3 always runs and what 27 tiles never choose: forced, and seen to run"""
    case, ref = fc.reference((17, 17, 17), term, dtype, False)
    g, _ = _solve_and_compare(case, ref, W26_FORCED, "conn 26 %s %s 17x17x17 k26_discharge_w" % (term, dtype))
    launches = g.launch_counts()
    g.close()
    assert launches["k26_discharge_w"] > 0, launches


@pytest.mark.parametrize("term,dtype", [("difference_exponential", "float32"), ("maximum_power", "int16")])
def test_small_and_thin_wall_cuts_through_the_wave_discharge(term, dtype):
    """the same kernel on one tile, on volumes thinner than a tile along one axis, on singleton axes and in 2-D"""
    for shape, spacing_on in fc.CUT_SHAPES:
        if shape == (17, 17, 17):
            continue
        case, ref = fc.reference(shape, term, dtype, spacing_on)
        g, _ = _solve_and_compare(case, ref, W26_FORCED, "conn %d %s %s %s k26_discharge_w" % (case["conn"], term, dtype, fc.shape_id(shape)))
        launches = g.launch_counts()
        g.close()
        assert launches["k26_discharge_w"] > 0, (shape, launches)


@pytest.mark.parametrize("dtype", fc.DTYPES)
@pytest.mark.parametrize("term", fc.TERMS)
@pytest.mark.parametrize("conn", fc.CONNECTIVITIES, ids="conn{}".format)
def test_wall_cuts_with_a_regional_term(conn, term, dtype):
    """the pre-push path of k_build<true> (prepush 1) and the graph as built (0): the oracle's cut both times, t-links exact"""
    for shape in fc.of_connectivity(fc.REGIONAL_SHAPES, conn):
        case, ref = fc.reference(shape, term, dtype, False, with_regional=True)
        src, snk = energy_numpy.regional_probability_tweights(case["prob"], case["alpha"])
        free = ~(case["fg"] | case["bg"]).ravel()
        for pre in (1, 0):
            g, _ = _solve_and_compare(case, ref, (("prepush", pre),), "conn %d %s %s %s regional prepush %d" % (case["conn"], term, dtype, fc.shape_id(shape), pre))
            np.testing.assert_array_equal(g.tweights().ravel()[free], (src - snk)[free])   # float32 products, exact (energy_voxel.py:61-65)
            g.close()


def test_dyadic_ties_bit_exact():
    """weights in {1, .75, .5, .25, DBL_MIN}: all arithmetic is exact, so labels and flow are the reference solver's bit for bit"""
    from medpy_amd import _lib
    case, ref = fc.dyadic_ties()
    g = _graph(case)
    flow = g.maxflow()
    _lib.assert_valid(g.validate())
    np.testing.assert_array_equal(g.labels(), ref.labels)
    assert flow == ref.flow
    g.close()


def test_layouts_and_dtypes():
    """F-ordered image and markers as medpy.io.load returns them, and an unsigned integer image, at connectivity 26"""
    case, ref = fc.reference((16, 17, 9), "difference_exponential", "float32", False)
    g, _ = _solve_and_compare(case, ref, what="F-ordered", image=np.asfortranarray(case["image"]), fg=np.asfortranarray(case["fg"]),
                              bg=np.asfortranarray(case["bg"]))
    g.close()
    case, ref = fc.reference((16, 17, 9), "difference_exponential", "int16", False)
    img16 = case["image"].astype(np.uint16)
    assert np.array_equal(img16, case["image"])   # the same whole numbers: the same oracle
    g, wdev = _solve_and_compare(case, ref, what="uint16", image=img16)
    g.close()
    fc.check_weights(wdev, fc.expected_weights(case["term"], img16, False)[1], exact=True)

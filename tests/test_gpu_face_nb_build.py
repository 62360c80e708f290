"""-m gpu: what every k_build<false, ...> instance (the 6-neighbourhood; 4 in 2-D, 2 in 1-D) STORES, read arc by arc through get_edge.

The weight read-backs (nweights, nweights_offset) re-evaluate g(.) from the resident image; only get_edge reads the residual planes
the build kernel filled.  k_build<false> evaluates a pair once, in its lower voxel, and hands the weight to the upper voxel through
LDS; the pair that enters a tile through a lower face is evaluated by extra lanes from the halo.  mgc_launch_build<false> has 26
instances: MGC_TERM_NONE, the four linear / division terms, the four exponential / power terms with the host's table (integer-valued
images) and without it (13), each as built and with the pre-push (a regional term: PRE6).

(a) the 13 plain instances, with and without spacing, on 27 tiles (the last one on every axis one voxel thick, two tiles per workgroup
for some), one axis inside a tile, a singleton axis, 2-D and 1-D: the arrays against oracle/energy_numpy.py as in
test_gpu_full_nb_build.py, then get_edge(i, j) and get_edge(j, i) of EVERY arc of 17 x 17 x 17 and 17 x 24 (elsewhere: every arc
through a tile face or at the volume's border, and a sample) bit-identical to nweights_offset, to each other and -- linear, division,
integer image -- to NumPy; 0.0 for pairs that are no neighbours.  Again with one workgroup building seven tiles in a row (grid_cap 1).
(b) the 13 PRE6 instances: what the pre-push may and may not have changed in the stored arcs (face_nb_cases.check_prepush), before any
solve; then labels and flow against BK, with the pre-push and without.
tests/test_face_nb_cases_host.py shows on the CPU that each of these comparisons rejects the build it is there to catch."""
import time

import numpy as np
import pytest

import face_nb_cases as fn
import full_nb_cases as fc
from oracle import energy_numpy

pytestmark = pytest.mark.gpu

_RUNS = {}


def _graph(shape, term, image, spacing, prob=None, alpha=None, params=()):
    """graph_from_voxels of a wall case; with ``params`` the same calls on a VoxelGraph, the knobs set before the build (the pre-push
    and the build grid act there)"""
    from medpy_amd import graphcut
    from medpy_amd.graphcut.graph import VoxelGraph
    w = fc.wall(shape)
    if not params:
        kw = {}
        if term is not None:
            sigma = fc.sigma_of(term)
            kw.update(boundary_term=getattr(graphcut.energy_voxel, "boundary_" + term),
                      boundary_term_args=(image, spacing) if sigma is None else (image, sigma, spacing))
        if prob is not None:
            kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(prob, alpha))
        return graphcut.graph_from_voxels(w["fg"], w["bg"], **kw)
    g = VoxelGraph(shape)
    if term is not None:
        g._set_boundary(term, image, fc.sigma_of(term), spacing)
    if prob is not None:
        g._set_regional(prob, alpha)
    g._set_markers(w["fg"], w["bg"])
    for k, v in params:
        g.set_param(k, v)
    g._build()
    return g


def _check_build(g, term, image, spacing, what, seed=0):
    t0 = time.perf_counter()
    wdev, per, calls = fn.check_build(term, image, spacing, g.nweights_offset, g.get_edge, g.nweights, seed)
    dt = time.perf_counter() - t0
    ulps = "" if not per else ", ulp from the restatement by offset " + " ".join("%s %.2f" % ("".join(map(str, o)), u) for o, u in sorted(per.items()))
    print("%s: %d get_edge calls, %.2f s for all read-backs%s" % (what, calls, dt, ulps))
    return wdev, per


@pytest.mark.parametrize("spacing_on", (False, True), ids=("plain", "spacing"))
@pytest.mark.parametrize("dtype", fn.DTYPES)
@pytest.mark.parametrize("term", fn.TERMS)
def test_every_stored_arc_of_the_build(term, dtype, spacing_on):
    """the eight terms' plain instances (float32: exp / pow without the table; int16: with it), as graph_from_voxels builds them"""
    worst = {}
    for shape in fn.SHAPES:
        image = fc.wall(shape)[dtype]
        spacing = fc.spacing_of(shape, spacing_on)
        g = _graph(shape, term, image, spacing)
        _, per = _check_build(g, term, image, spacing, "%s %s %s %s" % (term, dtype, fc.shape_id(shape), "spacing" if spacing_on else "plain"), seed=len(shape) + spacing_on)
        g.close()
        if len(shape) == 3:
            for o, u in per.items():
                worst[o] = max(worst.get(o, 0.0), u)
    if worst:
        print("%s %s %s: max ulp by axis offset %s (bound %d)" % (term, dtype, "spacing" if spacing_on else "plain", sorted(worst.items()), fc.ULP_BOUND[term]))


@pytest.mark.parametrize("term", ["difference_linear", "maximum_exponential", "difference_power"])
@pytest.mark.parametrize("regional", (False, True), ids=("plain", "prepush"))
def test_one_workgroup_builds_seven_tiles_in_a_row(term, regional):
    """grid_cap 1: a build grid of 4 on 27 tiles.  The float32 image is fetched one tile ahead; the LDS hand-over array, and the
    pre-push's planes, are rewritten tile after tile.  A linear, an exponential and a power term (float32: no table), as built and with
    the pre-push -- whose stored arcs do not depend on which workgroup built the tile"""
    shape = (17, 17, 17)
    if regional:
        a, b = _prepush_run(term, "float32", shape), _prepush_run(term, "float32", shape, grid_cap=1)
        for o in a["w"]:
            assert a["w"][o].tobytes() == b["w"][o].tobytes()
            assert a["fwd"][o].tobytes() == b["fwd"][o].tobytes() and a["back"][o].tobytes() == b["back"][o].tobytes(), "offset %s: the pre-pushed arcs depend on the build grid" % (o,)
        assert a["tr"].tobytes() == b["tr"].tobytes()
        return
    image = fc.wall(shape)["float32"]
    g = _graph(shape, term, image, fc.SPACING, params=(("grid_cap", 1),))
    _check_build(g, term, image, fc.SPACING, "%s float32 17x17x17 spacing, grid_cap 1" % term, seed=5)
    g.close()
    image16 = fc.wall(shape)["int16"]   # ... and a table instance, without the look-ahead
    if not fc.bit_exact(term, image):
        g = _graph(shape, term, image16, fc.SPACING, params=(("grid_cap", 1),))
        _check_build(g, term, image16, fc.SPACING, "%s int16 17x17x17 spacing, grid_cap 1" % term, seed=6)
        g.close()


@pytest.mark.parametrize("prepush", (0, 1), ids=("plain", "prepush"))
def test_no_boundary_term(prepush):
    """MGC_TERM_NONE, as built (prepush 0) and its PRE6 instance (1): a regional map and markers only.  Every arc 0.0, the t-links the
    reference's products, the oracle's cut"""
    from medpy_amd import _lib
    for shape in fn.PREPUSH_SHAPES:
        case, ref = fn.reference_regional_only(shape)
        g = _graph(shape, None, None, False, case["prob"], case["alpha"], params=(("prepush", prepush),))
        arcs = fn.every_arc(shape)
        for o, m in arcs.items():
            for off in (o, fc.negated(o)):
                a = g.nweights_offset(off)
                inside = np.zeros(shape, bool)
                inside[fc._slices(shape, off)[0]] = True
                assert np.array_equal(np.isnan(a), ~inside)
                assert not a[inside].any()
        fwd, back, _ = fn.read_edges(g.get_edge, shape, arcs)
        for o, m in arcs.items():
            assert not fwd[o][m].any() and not back[o][m].any(), "offset %s: an arc of a graph without a boundary term is not 0.0" % (o,)
        fn.check_non_neighbours(g.get_edge, shape)
        src, snk = energy_numpy.regional_probability_tweights(case["prob"], case["alpha"])
        free = ~(case["fg"] | case["bg"]).ravel()
        np.testing.assert_array_equal(g.tweights().ravel()[free], (src - snk)[free])
        flow = g.maxflow()
        _lib.assert_valid(g.validate())
        np.testing.assert_array_equal(g.labels(), ref.labels)
        assert flow == pytest.approx(ref.flow, rel=1e-9)
        g.close()


# ---- (b) the instances with the pre-push -----------------------------------------------------------------------------------------------

def _solve(g, case, ref, what):
    from medpy_amd import _lib
    flow = g.maxflow()
    _lib.assert_valid(g.validate())
    labels = g.labels()
    differing = fc.assert_cut(labels, flow, case, ref, fn.expected_weights(case["term"], case["image"], case["spacing"])[1], what)
    print("%s: flow %.12g, source side %.3f, %d voxels differ inside the ambiguity set" % (what, flow, labels.mean(), differing))
    return labels, flow


def _plain_run(term, dtype, shape):
    """the regional case with prepush 0 -- the plain instance: the assertions of (a), then the solve.  Once per process"""
    key = ("plain", term, dtype, shape)
    if key not in _RUNS:
        case, ref = fn.reference(shape, term, dtype, False, with_regional=True)
        what = "%s %s %s regional prepush 0" % (term, dtype, fc.shape_id(shape))
        g = _graph(shape, term, case["image"], False, case["prob"], case["alpha"], params=(("prepush", 0),))
        wdev, _ = _check_build(g, term, case["image"], False, what, seed=11)
        tr = g.tweights()
        labels, flow = _solve(g, case, ref, what)
        g.close()
        _RUNS[key] = {"w": wdev, "tr": tr, "labels": labels, "flow": flow}
    return _RUNS[key]


def _prepush_run(term, dtype, shape, grid_cap=None):
    """the regional case with prepush 1 -- the PRE6 instance: the weights as built, the stored arcs and the t-links BEFORE any solve,
    fn.check_prepush on them, then the solve.  Once per process"""
    key = ("pre", term, dtype, shape, grid_cap)
    if key not in _RUNS:
        case, ref = fn.reference(shape, term, dtype, False, with_regional=True)
        what = "%s %s %s regional prepush 1%s" % (term, dtype, fc.shape_id(shape), "" if grid_cap is None else " grid_cap %d" % grid_cap)
        g = _graph(shape, term, case["image"], False, case["prob"], case["alpha"],
                   params=(("prepush", 1),) + ((("grid_cap", grid_cap),) if grid_cap else ()))
        t0 = time.perf_counter()
        wdev, wrev, _, _ = fn.check_read_backs(term, case["image"], False, g.nweights_offset, g.nweights)   # still the weights as built
        fwd, back, calls = fn.read_edges(g.get_edge, shape, fn.every_arc(shape))
        tr = g.tweights()
        fn.check_non_neighbours(g.get_edge, shape)
        pushed = fn.check_prepush(shape, wdev, fwd, back, tr)
        cand, pairs = fn.push_candidates(shape, wdev, tr)
        print("%s: %d arcs hold less than their weight (%d in-tile pairs could carry a push, of %d); %d get_edge calls, %.2f s for all read-backs"
              % (what, pushed, cand, pairs, calls, time.perf_counter() - t0))
        labels, flow = _solve(g, case, ref, what)
        g.close()
        _RUNS[key] = {"w": wdev, "fwd": fwd, "back": back, "tr": tr, "labels": labels, "flow": flow, "pushed": pushed}
    return _RUNS[key]


@pytest.mark.parametrize("shape", fn.PREPUSH_SHAPES, ids=fc.shape_id)
@pytest.mark.parametrize("prepush", (0, 1), ids=("plain", "prepush"))
@pytest.mark.parametrize("dtype", fn.DTYPES)
@pytest.mark.parametrize("term", fn.TERMS)
def test_what_the_build_with_a_regional_term_stores(term, dtype, prepush, shape):
    """prepush 0: the plain instance, every assertion of (a).  prepush 1: the PRE6 instance -- the read-backs of the weights unchanged,
    the stored arcs changed only as one push per in-tile pair from a source link to a sink link can change them, and some were; labels
    and flow the oracle's either way, the labels the same where the input has no exact ties"""
    plain = _plain_run(term, dtype, shape)
    if not prepush:
        return
    pre = _prepush_run(term, dtype, shape)
    for o in plain["w"]:
        assert pre["w"][o].tobytes() == plain["w"][o].tobytes(), "offset %s: nweights_offset differs with the pre-push" % (o,)
    assert pre["tr"].tobytes() == plain["tr"].tobytes()
    assert pre["pushed"] > 0
    case, ref = fn.reference(shape, term, dtype, False, with_regional=True)
    src, snk = energy_numpy.regional_probability_tweights(case["prob"], case["alpha"])
    free = ~(case["fg"] | case["bg"]).ravel()
    np.testing.assert_array_equal(pre["tr"].ravel()[free], (src - snk)[free])
    assert pre["flow"] == pytest.approx(plain["flow"], rel=1e-9)
    if not fc.tie_degenerate(term, case["image"]):
        np.testing.assert_array_equal(pre["labels"], plain["labels"])

"""What tests/test_full_nb_cases_host.py (CPU tier) and the -m gpu files of the full neighbourhood (test_gpu_full_nb_build.py,
test_gpu_full_nb_cuts.py, test_gpu_full_neighbourhood.py) share: the wall inputs, the BK oracle on them, and the comparisons of a
device read-back with oracle/energy_numpy.py:boundary_weights_offsets.  Not a test module.

The wall: foreground on the first plane of the longest axis, background on its last, and between them a two-voxel-thick bright
surface (+100 on uniform(0, 5) noise) whose position waves with the other two indices.  The shipped generators cut at the seed under
half of the terms, where labels come out right if no flow moves at all; the minimum cut of a wall lies at the surface, half a volume
away from either marker, under all eight terms (conditions (a), (b) of test_full_nb_cases_host.py).

The comparisons take arrays and callables, never a graph handle: the CPU tier feeds them doctored "device" arrays made from the
oracle's own weights and requires every one to be rejected, which is how the GPU tests are shown to be sensitive without a GPU."""
import math

import numpy as np

from oracle import cutcheck, energy_numpy, pipeline

TERMS = energy_numpy.TERMS
SIGMA = {"linear": None, "exponential": 40.0, "division": 3.0, "power": 1.7}
SPACING = (1.0, 0.7, 2.5)
DTYPES = ("float32", "int16")
MAX = 65535.0

# every arc of every k_build<true, ...> instance (test_gpu_full_nb_build.py) -- 27 tiles (one with all 26 tile neighbours), one axis
# inside a tile and two across, 2-D (connectivity 8, dz = 1)
BUILD_SHAPES = [(17, 17, 17), (7, 9, 17), (17, 24)]
# labels and flow (test_gpu_full_nb_cuts.py): (shape, spacing on) -- spacing on for half of them
CUT_SHAPES = [((8, 8, 8), False), ((9, 9, 9), True), ((17, 17, 17), False), ((7, 9, 17), True), ((16, 17, 9), False), ((24, 9, 10), True),
              ((1, 9, 17), False), ((9, 1, 17), True), ((17, 9, 1), False), ((9, 17), True), ((17, 24), False)]
REGIONAL_SHAPES = [(17, 17, 17), (17, 24)]
# the absolute bound the suite had before the ulp bound, kept beside it: it guards the large weights
ENERGY_TOL = 1e-6
# exp / pow evaluated on the device against NumPy's, in ulp of the expected weight, over the 13 forward offsets with and without
# spacing.  Measured on MI355X on BUILD_SHAPES: 1 ulp without spacing, 2 ulp with it (the division by the Euclidean
# length rounds once more), for each of the four terms; the bound is twice the maximum
ULP_BOUND = {"difference_exponential": 4, "maximum_exponential": 4, "difference_power": 4, "maximum_power": 4}

_CACHE = {}


def shape_id(shape):
    return "x".join(map(str, shape))


def full_connectivity(ndim):
    return 3 ** ndim - 1


CONNECTIVITIES = (26, 8)


def of_connectivity(shapes, conn):
    """the entries of a shape list (shapes, or (shape, ...) tuples) whose full neighbourhood is ``conn``"""
    return [e for e in shapes if full_connectivity(len(e[0] if isinstance(e[0], tuple) else e)) == conn]


def sigma_of(term):
    return SIGMA[term.split("_")[1]]


def spacing_of(shape, on):
    return SPACING[:len(shape)] if on else False


def tie_degenerate(term, image):
    """the project's rule (tests/test_gpu_parity.py:_tie_degenerate): exact ties between minimum cuts are expected"""
    return term.startswith("maximum") or np.issubdtype(np.asarray(image).dtype, np.integer)


def bit_exact(term, image):
    """are the device's weights the restatement's bit for bit?  The linear and division terms are IEEE basic operations; on an
    integer-valued image the exponential and power terms go by the table the host fills with the reference's own NumPy operations"""
    return term.split("_")[1] in ("linear", "division") or np.issubdtype(np.asarray(image).dtype, np.integer)


def wall(shape):
    """{"float32": image, "int16": the same rounded, "fg", "bg"} of one shape, generated once"""
    shape = tuple(int(s) for s in shape)
    key = ("wall", shape)
    if key not in _CACHE:
        ax = int(np.argmax(shape))
        n = shape[ax]
        idx = np.indices(shape)
        others = sum(idx[k] for k in range(len(shape)) if k != ax)
        pos = n // 2 + np.rint(1.5 * np.sin(0.9 * others)).astype(np.int64)
        on_surface = (idx[ax] == pos) | (idx[ax] == pos + 1)   # two voxels thick: no diagonal step crosses it
        rng = np.random.default_rng(1000 + sum((k + 1) * s for k, s in enumerate(shape)))
        img = rng.uniform(0.0, 5.0, shape) + 100.0 * on_surface
        fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
        sl = [slice(None)] * len(shape)
        sl[ax] = 0
        fg[tuple(sl)] = True
        sl[ax] = n - 1
        bg[tuple(sl)] = True
        _CACHE[key] = {"float32": img.astype(np.float32), "int16": np.rint(img).astype(np.int16), "fg": fg, "bg": bg}
    return _CACHE[key]


def _smooth(field, passes):
    """a box blur of width 3 along every axis, ``passes`` times, edges repeated"""
    for _ in range(passes):
        for a in range(field.ndim):
            if field.shape[a] > 1:
                p = np.concatenate([np.take(field, [0], a), field, np.take(field, [-1], a)], axis=a)
                n = field.shape[a]
                field = (np.take(p, range(0, n), a) + np.take(p, range(1, n + 1), a) + np.take(p, range(2, n + 2), a)) / 3.0
    return field


# the regional term of the cases that have one: alpha per kind of boundary term, in proportion to the weights the kind gives a pair
# of noise voxels (linear ~ 0.97, exponential ~ 0.99, division ~ 0.6, power ~ 0.25), so that the map moves the cut -- condition (c)
# of test_full_nb_cases_host.py -- without carrying it to a marker -- condition (a)
ALPHA = {"linear": 3.6, "exponential": 3.6, "division": 1.8, "power": 0.75}


def regional(shape, term):
    """(float32 probability map, alpha): 0.5 + a smooth random field of zero mean, so that neither terminal is favoured overall"""
    shape = tuple(int(s) for s in shape)
    key = ("prob", shape)
    if key not in _CACHE:
        rng = np.random.default_rng(77 + sum(shape))
        f = _smooth(rng.normal(0.0, 1.0, shape), 3)
        f = (f - f.mean()) / np.abs(f - f.mean()).max()
        _CACHE[key] = np.clip(0.5 + 0.45 * f, 0.0, 1.0).astype(np.float32)
    return _CACHE[key], ALPHA[term.split("_")[1]]


def merged_tlinks(fg, bg, prob=None, alpha=None):
    """source weight - sink weight per voxel, as the reference merges them (graph.h:416-425): regional term, then the markers"""
    tr = np.zeros(fg.size)
    if prob is not None:
        src, snk = energy_numpy.regional_probability_tweights(prob, alpha)
        tr = src - snk
    return tr + np.where(fg.ravel(), MAX, 0.0) - np.where(bg.ravel(), MAX, 0.0)


def expected_weights(term, image, spacing, connectivity=None):
    """(forward offsets, {offset: array}) of the restatement at connectivity 3^n - 1 (``connectivity``: at that one)"""
    image = np.asarray(image)
    offs = energy_numpy.forward_offsets(image.ndim, connectivity or full_connectivity(image.ndim))
    return offs, energy_numpy.boundary_weights_offsets(term, image, offs, sigma_of(term), spacing)


def reference(shape, term, dtype, spacing_on, with_regional=False, connectivity=None):
    """the oracle's cut of a wall case, solved once per process: (case dict, pipeline.Cut).  At connectivity 3^n - 1, or at
    ``connectivity``"""
    conn = connectivity or full_connectivity(len(shape))
    key = ("ref", tuple(shape), term, dtype, bool(spacing_on), bool(with_regional)) + ((conn,) if connectivity else ())
    if key not in _CACHE:
        w = wall(shape)
        case = {"shape": tuple(shape), "term": term, "image": w[dtype], "fg": w["fg"], "bg": w["bg"], "sigma": sigma_of(term),
                "spacing": spacing_of(shape, spacing_on), "conn": conn, "prob": None, "alpha": None}
        if with_regional:
            case["prob"], case["alpha"] = regional(shape, term)
        kw = dict(prob=case["prob"], alpha=case["alpha"]) if with_regional else {}
        ref = pipeline.graphcut_voxel(case["fg"], case["bg"], term=term, image=case["image"], sigma=case["sigma"], spacing=case["spacing"],
                                      connectivity=case["conn"], **kw)
        _CACHE[key] = (case, ref)
    return _CACHE[key]


def reference_regional_only(shape, connectivity=None):
    """MGC_TERM_NONE at the full neighbourhood (or at ``connectivity``): a regional map and the markers of the wall, no boundary term
    (no n-link at all)"""
    conn = connectivity or full_connectivity(len(shape))
    key = ("ref_none", tuple(shape)) + ((conn,) if connectivity else ())
    if key not in _CACHE:
        w = wall(shape)
        prob, alpha = regional(shape, "difference_linear")
        case = {"shape": tuple(shape), "term": None, "image": None, "fg": w["fg"], "bg": w["bg"], "sigma": None, "spacing": False,
                "conn": conn, "prob": prob, "alpha": alpha}
        if conn == 2 * len(shape):   # the reference's own neighbourhood: no term, no n-link
            _CACHE[key] = (case, pipeline.graphcut_voxel(w["fg"], w["bg"], prob=prob, alpha=alpha))
            return _CACHE[key]
        none = {o: np.full(shape, np.nan) for o in energy_numpy.forward_offsets(len(shape), case["conn"])}
        _CACHE[key] = (case, pipeline.graphcut_voxel(w["fg"], w["bg"], weights=none, connectivity=case["conn"], prob=prob, alpha=alpha))
    return _CACHE[key]


def dyadic_ties():
    """synthetic.ties((24, 24, 24)) with the range pinned to 4 under difference_linear: every weight is one of 1, .75, .5, .25,
    DBL_MIN and all arithmetic is exact, at connectivity 26 as at 6 (tests/test_gpu_parity.py:test_ties_dyadic_bit_exact)"""
    key = "dyadic"
    if key not in _CACHE:
        from medpy_amd import synthetic
        s = synthetic.ties((24, 24, 24))
        img = s["image"].copy()
        img.flat[0], img.flat[1] = 0.0, 4.0
        case = {"shape": img.shape, "term": "difference_linear", "image": img, "fg": s["fg"], "bg": s["bg"], "sigma": None, "spacing": False,
                "conn": 26, "prob": None, "alpha": None}
        _CACHE[key] = (case, pipeline.graphcut_voxel(s["fg"], s["bg"], term="difference_linear", image=img, connectivity=26))
    return _CACHE[key]


def cut_facts(case, ref):
    """(unmarked voxels, source share of them, ambiguity share of them) of a solved reference cut"""
    free = ~(case["fg"] | case["bg"])
    n = int(free.sum())
    amb = cutcheck.ambiguity(ref.graph)[2].reshape(free.shape)
    return n, float(ref.labels[free].mean()) if n else 0.0, float(amb[free].mean()) if n else 0.0


# ---- the comparisons ---------------------------------------------------------------------------------------------------------------

def _slices(shape, o):
    """(src, dst): the voxels p with p + o inside the volume, and those p + o"""
    src = tuple(slice(max(0, -k), shape[i] - max(0, k)) for i, k in enumerate(o))
    dst = tuple(slice(max(0, k), shape[i] - max(0, -k)) for i, k in enumerate(o))
    return src, dst


def ulp_distance(got, want):
    """|got - want| in units of the spacing of the doubles at ``want``, NaN where either is"""
    with np.errstate(invalid="ignore"):
        return np.abs(got - want) / np.spacing(np.abs(want))


def check_weights(wdev, wref, exact, ulp_bound=None):
    """every offset of ``wref`` in ``wdev``: the NaN pattern identical; the values bit for bit (``exact``) or within ``ulp_bound`` ulp
    of the expected weight AND within 1e-6 of it.  Returns the largest ulp distance seen."""
    worst = 0.0
    for o, want in wref.items():
        got = wdev[o]
        assert got.shape == want.shape and got.dtype == np.float64, (o, got.shape, got.dtype)
        assert np.array_equal(np.isnan(got), np.isnan(want)), "offset %s: the arcs that leave the volume differ" % (o,)
        if exact:
            assert got.tobytes() == np.ascontiguousarray(want, dtype=np.float64).tobytes(), "offset %s: weights are not bit-identical" % (o,)
            continue
        ok = ~np.isnan(want)
        if not ok.any():
            continue
        ulp = float(ulp_distance(got[ok], want[ok]).max())
        worst = max(worst, ulp)
        assert ulp_bound is None or ulp <= ulp_bound, "offset %s: %.1f ulp from the expected weight (bound %d)" % (o, ulp, ulp_bound)
        assert float(np.abs(got[ok] - want[ok]).max()) <= ENERGY_TOL, "offset %s: more than %g from the expected weight" % (o, ENERGY_TOL)
    return worst


def check_reverse(wdev, wrev):
    """``wrev[o]`` is the read-back at -o: at p + o it carries the capacity of the arc (p, p + o), bit for bit, and it is NaN exactly
    where stepping by -o leaves the volume"""
    for o, fwd in wdev.items():
        rev = wrev[o]
        src, dst = _slices(fwd.shape, o)
        want = np.full(fwd.shape, np.nan)
        want[dst] = fwd[src]
        assert np.array_equal(np.isnan(rev), np.isnan(want)), "offset %s: the reverse read-back leaves the volume elsewhere" % (o,)
        assert rev.tobytes() == want.tobytes(), "offset %s: the reverse arcs do not carry the forward capacities" % (o,)


def check_axes(axis_arrays, wdev):
    """the per-axis read-back (shape[a] - 1 along a) against the read-back by offset of the axis offsets"""
    nd = len(axis_arrays)
    for a, got in enumerate(axis_arrays):
        o = tuple(1 if k == a else 0 for k in range(nd))
        src, _ = _slices(wdev[o].shape, o)
        assert got.tobytes() == np.ascontiguousarray(wdev[o][src]).tobytes(), "axis %d: nweights() and nweights_offset() disagree" % a


def _crossing(p, o, tile=8):
    """how many tile borders the arc (p, p + o) crosses: 0 inside a tile, 1 a face, 2 an edge, 3 a corner"""
    return sum(1 for c, k in zip(p, o) if k and (c + k) // tile != c // tile)


def sample_pairs(shape, offsets, seed, count=50):
    """about ``count`` arcs (p, o), p + o inside the volume: every offset at least once, and -- where the shape has them -- six arcs
    each that cross a tile face, a tile edge and a tile corner, besides arcs that stay inside a tile.  Returns (pairs, {borders
    crossed: does the volume have such arcs})"""
    rng = np.random.default_rng(seed)
    pairs, by_cross = [], {0: [], 1: [], 2: [], 3: []}
    for o in offsets:
        src, _ = _slices(shape, o)
        grids = np.meshgrid(*[np.arange(s.start, s.stop) for s in src], indexing="ij")
        ps = np.stack([g.ravel() for g in grids], axis=1)
        if not len(ps):
            continue
        pairs.append((tuple(int(c) for c in ps[rng.integers(len(ps))]), o))
        crossed = sum(((ps[:, a] + k) // 8 != ps[:, a] // 8).astype(int) for a, k in enumerate(o) if k)
        for k in by_cross:
            sel = ps[crossed == k]
            for n in rng.permutation(len(sel))[:6]:
                by_cross[k].append((tuple(int(c) for c in sel[int(n)]), o))
    for k in (3, 2, 1, 0):
        have = by_cross[k]
        want = max(count - len(pairs), 0) if k == 0 else 6
        for n in rng.permutation(len(have))[:want]:
            pairs.append(have[int(n)])
    return pairs, {k: bool(v) for k, v in by_cross.items()}


def check_get_edge(get_edge, shape, wdev, wrev, pairs):
    """``get_edge(i, j)`` of a graph as built against the arrays, for every sampled arc in both orders"""
    strides = [int(np.prod(shape[k + 1:])) for k in range(len(shape))]
    for p, o in pairs:
        i = sum(c * s for c, s in zip(p, strides))
        q = tuple(c + k for c, k in zip(p, o))
        j = sum(c * s for c, s in zip(q, strides))
        there, back = get_edge(i, j), get_edge(j, i)
        assert there == wdev[o][p], "get_edge(%d, %d) = %r, nweights_offset%s there = %r (crosses %d tile borders)" % (i, j, there, o, wdev[o][p], _crossing(p, o))
        assert back == wrev[o][q], "get_edge(%d, %d) = %r, nweights_offset(-%s) there = %r (crosses %d tile borders)" % (j, i, back, o, wrev[o][q], _crossing(p, o))


def negated(o):
    return tuple(-k for k in o)


def check_read_backs(term, image, spacing, read_offset, get_edge, read_axis, seed=0):
    """Every public read-back of the n-links of a graph AS BUILT against the restatement: ``read_offset(o)`` (nweights_offset) for
    the forward offsets and their mirrors, ``read_axis(a)`` (nweights), ``get_edge(i, j)`` on sampled arcs.  Returns
    ({offset: device array}, the largest ulp distance).  The GPU tests pass a graph's methods, the CPU tier doctored stand-ins."""
    image = np.asarray(image)
    offs, wref = expected_weights(term, image, spacing)
    wdev = {o: read_offset(o) for o in offs}
    wrev = {o: read_offset(negated(o)) for o in offs}
    exact = bit_exact(term, image)
    worst = check_weights(wdev, wref, exact, None if exact else ULP_BOUND[term])
    check_reverse(wdev, wrev)
    check_axes([read_axis(a) for a in range(image.ndim)], wdev)
    pairs, crossings = sample_pairs(image.shape, offs, seed)
    for k in range(1, sum(1 for s in image.shape if s > 8) + 1):   # k axes longer than a tile: arcs that cross k tile borders exist
        assert crossings[k], "no sampled arc crosses %d tile borders" % k
    check_get_edge(get_edge, image.shape, wdev, wrev, pairs)
    return wdev, worst


def exact_edges(shape, weights, fg, bg, prob=None, alpha=None):
    """what cutcheck.assert_labels_equivalent(exact=...) takes, from a {offset: array} dict"""
    i, j, w = cutcheck.offset_edges(shape, weights)
    return i, j, w, w, merged_tlinks(fg, bg, prob, alpha)


def assert_cut(labels, flow, case, ref, weights, what):
    """labels and flow of a solved case against an oracle cut ``ref`` whose boundary weights were ``weights``: flow to 1e-9, labels
    identical -- or, on a tie-degenerate case, every differing voxel in the reference's ambiguity set at equal capacity in exact
    rationals"""
    assert math.isclose(flow, ref.flow, rel_tol=1e-9, abs_tol=0.0), "%s: flow %r, oracle %r" % (what, flow, ref.flow)
    differing = int((np.asarray(labels, bool) != ref.labels).sum())
    if differing:
        assert tie_degenerate(case["term"], case["image"]), "%s: %d labels differ on an input without exact ties" % (what, differing)
        cutcheck.assert_labels_equivalent(labels, ref, exact=exact_edges(case["shape"], weights, case["fg"], case["bg"], case["prob"], case["alpha"]))
    return differing

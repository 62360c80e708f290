"""What tests/test_face_nb_cases_host.py (CPU tier) and tests/test_gpu_face_nb_build.py (-m gpu) share: the cases of the face
neighbourhood (6 in 3-D, 4 in 2-D, 2 in 1-D) and the comparisons of what k_build<false, ...> STORED -- read arc by arc through get_edge,
the only read-back of the stored n-links -- with the weights as built (nweights_offset re-evaluates them from the image) and with
oracle/energy_numpy.py.  Not a test module.  Inputs, oracle and the array comparisons are those of tests/full_nb_cases.py (fc), at
connectivity 2 * ndim.

As there, the comparisons take arrays and callables, never a graph handle: the CPU tier feeds them a stand-in made from the oracle's own
weights, doctored in the ways this kernel could be wrong, and requires each to be rejected by the assertion named for it (the constants
below are those names)."""
import numpy as np

import full_nb_cases as fc
from oracle import energy_numpy

TERMS = fc.TERMS
DTYPES = fc.DTYPES
TILE = 8
# 27 tiles: the middle one has all six face neighbours, the last one on every axis is one voxel thick (every bounds predicate of the
# lanes that evaluate the pair entering through a lower face), and the build grid is 24, so some workgroups build two tiles; one axis
# inside a tile; a singleton axis; 2-D; 1-D
SHAPES = [(17, 17, 17), (7, 9, 17), (1, 9, 17), (17, 24), (17,)]
SWEEP_SHAPES = [(17, 17, 17), (17, 24)]   # get_edge of EVERY arc in both orders; elsewhere border_arcs()
PREPUSH_SHAPES = fc.REGIONAL_SHAPES       # (17, 17, 17) and (17, 24)

# the assertions, by name
STORED_FORWARD = "forward arc as stored"
STORED_REVERSE = "reverse arc as stored"
NOT_SYMMETRIC = "forward and reverse arc of a pair differ"
NOT_RESTATEMENT = "stored arc is not the restatement's"
NO_NEIGHBOUR = "is no lattice neighbour"
PUSH_ACROSS_TILES = "arc between two tiles is not as built"
PUSH_IN_QUIET_TILE = "arc of a tile without both signs of t-link is not as built"
NEGATIVE_RESIDUAL = "negative residual"
BOTH_LOWERED = "both directions of a pair are below the weight"
NOT_FROM_SOURCE = "push out of a voxel whose t-link is no source link"
NOT_TO_SINK = "push into a voxel whose t-link is no sink link"
SUM_CHANGED = "the two residuals of a pair do not add up to the two weights"
SOURCE_OVERDRAWN = "more flow out of a voxel than its source link holds"
SINK_OVERDRAWN = "more flow into a voxel than its sink link takes"
NOTHING_PUSHED = "no arc was pre-pushed"


def connectivity(ndim):
    return 2 * ndim


def offsets(ndim):
    return energy_numpy.forward_offsets(ndim, 2 * ndim)


def axis_of(o):
    return [k for k, s in enumerate(o) if s][0]


def strides(shape):
    return [int(np.prod(shape[k + 1:])) for k in range(len(shape))]


def expected_weights(term, image, spacing):
    return fc.expected_weights(term, image, spacing, connectivity(np.asarray(image).ndim))


def reference(shape, term, dtype, spacing_on, with_regional=False):
    """fc.reference at connectivity 2 * ndim: pipeline.graphcut_voxel on the reference's own neighbourhood"""
    return fc.reference(shape, term, dtype, spacing_on, with_regional, connectivity=connectivity(len(shape)))


def reference_regional_only(shape):
    return fc.reference_regional_only(shape, connectivity=connectivity(len(shape)))


def check_read_backs(term, image, spacing, read_offset, read_axis):
    """the array comparisons of fc.check_read_backs at the face offsets: NaN pattern, values (bit for bit, or within fc.ULP_BOUND
    and 1e-6), mirrors, the per-axis read-back.  Returns ({offset: array}, {offset: array at the mirrored offset}, largest ulp,
    {offset: largest ulp})"""
    image = np.asarray(image)
    offs, wref = expected_weights(term, image, spacing)
    wdev = {o: read_offset(o) for o in offs}
    wrev = {o: read_offset(fc.negated(o)) for o in offs}
    exact = fc.bit_exact(term, image)
    worst = fc.check_weights(wdev, wref, exact, None if exact else fc.ULP_BOUND[term])
    fc.check_reverse(wdev, wrev)
    fc.check_axes([read_axis(a) for a in range(image.ndim)], wdev)
    per = {}
    if not exact:
        for o in offs:
            ok = ~np.isnan(wref[o])
            per[o] = float(fc.ulp_distance(wdev[o][ok], wref[o][ok]).max()) if ok.any() else 0.0
    return wdev, wrev, worst, per


def check_sample(get_edge, shape, wdev, wrev, seed=0):
    """fc.check_read_backs' get_edge comparison on fc.sample_pairs' sample (an arc of this neighbourhood crosses one tile border at
    most)"""
    pairs, crossings = fc.sample_pairs(shape, offsets(len(shape)), seed)
    assert crossings[1] == any(s > TILE for s in shape), "no sampled arc crosses a tile face"
    fc.check_get_edge(get_edge, shape, wdev, wrev, pairs)


# ---- which arcs ----------------------------------------------------------------------------------------------------------------------

def every_arc(shape):
    """{offset: bool array, True at p where (p, p + offset) is an arc of the volume}"""
    out = {}
    for o in offsets(len(shape)):
        m = np.zeros(shape, bool)
        m[fc._slices(shape, o)[0]] = True
        out[o] = m
    return out


def border_arcs(shape, seed=0):
    """every arc that crosses a tile face or has an end on the volume's border, and fc.sample_pairs' sample of the others"""
    idx = np.indices(shape)
    rim = np.zeros(shape, bool)
    for a, n in enumerate(shape):
        rim |= (idx[a] == 0) | (idx[a] == n - 1)
    out = {}
    for o, m in every_arc(shape).items():
        a = axis_of(o)
        src, dst = fc._slices(shape, o)
        sel = np.zeros(shape, bool)
        sel[src] = rim[src] | rim[dst] | ((idx[a][src] + 1) % TILE == 0)
        out[o] = sel & m
    for p, o in fc.sample_pairs(shape, offsets(len(shape)), seed)[0]:
        out[o][p] = True
    return out


def arcs_of(shape, seed=0):
    return every_arc(shape) if tuple(shape) in SWEEP_SHAPES else border_arcs(shape, seed)


def non_neighbours(shape, seed=0):
    """[(i, j, what)]: pairs of voxels that are no lattice neighbours at connectivity 2 * ndim -- the last voxel of EVERY row and the
    first of the next (consecutive ids), and a sample of diagonal steps and of steps of two along every axis"""
    nd, st = len(shape), strides(shape)
    rng = np.random.default_rng(seed)
    out = []
    if nd >= 2 and shape[-1] > 1:
        n = int(np.prod(shape))
        for i in range(shape[-1] - 1, n - 1, shape[-1]):
            out.append((i, i + 1, "the end of a row and the start of the next"))
    for a in range(nd):
        for b in range(a + 1, nd):
            if shape[a] > 1 and shape[b] > 1:
                for sign in (1, -1):
                    for _ in range(4):
                        p = [int(rng.integers(0, s)) for s in shape]
                        p[a] = int(rng.integers(0, shape[a] - 1))
                        p[b] = int(rng.integers(0, shape[b] - 1)) + (1 if sign < 0 else 0)
                        i = sum(c * s for c, s in zip(p, st))
                        out.append((i, i + st[a] + sign * st[b], "a diagonal step along axes %d and %d" % (a, b)))
        if shape[a] > 2:
            for c in sorted({0, TILE - 2, TILE - 1, shape[a] - 3} & set(range(shape[a] - 2))):
                p = [int(rng.integers(0, s)) for s in shape]
                p[a] = c
                i = sum(x * s for x, s in zip(p, st))
                out.append((i, i + 2 * st[a], "a step of two along axis %d" % a))
    return out


def check_non_neighbours(get_edge, shape, seed=0):
    pairs = non_neighbours(shape, seed)
    for i, j, what in pairs:
        for x, y in ((i, j), (j, i)):
            got = get_edge(x, y)
            assert got == 0.0 and not np.signbit(got), "get_edge(%d, %d) = %r: %s %s" % (x, y, got, what, NO_NEIGHBOUR)
    return len(pairs)


# ---- what k_build stored -------------------------------------------------------------------------------------------------------------

def read_edges(get_edge, shape, arcs):
    """get_edge(i, j) and get_edge(j, i) of every arc of ``arcs``: ({offset: array}, {offset: array}, calls), both arrays indexed by the
    LOWER voxel of the pair and NaN where no arc was read"""
    st = strides(shape)
    fwd, back, calls = {}, {}, 0
    for o, m in arcs.items():
        step = sum(k * s for k, s in zip(o, st))
        f, b = np.full(int(np.prod(shape)), np.nan), np.full(int(np.prod(shape)), np.nan)
        for i in np.flatnonzero(m.ravel()).tolist():
            f[i] = get_edge(i, i + step)
            b[i] = get_edge(i + step, i)
        calls += 2 * int(m.sum())
        fwd[o], back[o] = f.reshape(shape), b.reshape(shape)
    return fwd, back, calls


def _where(shape, o, mask, bad):
    """the first arc of ``mask`` (lower voxels) at which ``bad`` (one entry per True of mask) holds, in words"""
    p = tuple(int(c[np.flatnonzero(bad)[0]]) for c in np.nonzero(mask))
    tile = tuple(c // TILE for c in p)
    return "arc %s + %s (tile %s, %s)" % (p, o, tile, "crosses a tile face" if (p[axis_of(o)] + 1) % TILE == 0 else "inside the tile")


def _same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)


def check_stored(shape, arcs, fwd, back, wdev, wrev, wref=None):
    """What get_edge read from the graph AS BUILT, arc by arc: both directions bit-identical to nweights_offset at the voxel the arc
    leaves (``wdev`` at p, ``wrev`` -- the read-back at the mirrored offset -- at p + o), to each other (the weights are symmetric),
    and, where ``wref`` is given (the bit-exact cases), to the NumPy restatement"""
    for o, m in arcs.items():
        if not m.any():
            continue
        _, dst = fc._slices(shape, o)
        at_q = np.full(shape, np.nan)
        at_q[fc._slices(shape, o)[0]] = wrev[o][dst]   # nweights_offset(-o) at p + o, moved to p
        f, b = fwd[o][m], back[o][m]
        bad = ~_same_bits(f, wdev[o][m])
        assert not bad.any(), "%s: get_edge(p, p + o) is not nweights_offset(o) at p: %s, %d arcs of %d" % (STORED_FORWARD, _where(shape, o, m, bad), bad.sum(), m.sum())
        bad = ~_same_bits(b, at_q[m])
        assert not bad.any(), "%s: get_edge(p + o, p) is not nweights_offset(-o) at p + o: %s, %d arcs of %d" % (STORED_REVERSE, _where(shape, o, m, bad), bad.sum(), m.sum())
        bad = ~_same_bits(f, b)
        assert not bad.any(), "%s: %s, %d arcs of %d" % (NOT_SYMMETRIC, _where(shape, o, m, bad), bad.sum(), m.sum())
        if wref is not None:
            bad = ~_same_bits(f, wref[o][m])
            assert not bad.any(), "%s: %s, %d arcs of %d" % (NOT_RESTATEMENT, _where(shape, o, m, bad), bad.sum(), m.sum())


def check_build(term, image, spacing, read_offset, get_edge, read_axis, seed=0):
    """everything test_gpu_face_nb_build.py asserts of a graph as built without a pre-push: the arrays, then get_edge of every arc
    (SWEEP_SHAPES) or of the border arcs and a sample, of fc.sample_pairs' sample, and of pairs that are no neighbours.  Returns
    (weights as built, {offset: largest ulp distance}, get_edge calls of the sweep)"""
    image = np.asarray(image)
    shape = image.shape
    wdev, wrev, _, per = check_read_backs(term, image, spacing, read_offset, read_axis)
    arcs = arcs_of(shape, seed)
    fwd, back, calls = read_edges(get_edge, shape, arcs)
    check_stored(shape, arcs, fwd, back, wdev, wrev, expected_weights(term, image, spacing)[1] if fc.bit_exact(term, image) else None)
    check_sample(get_edge, shape, wdev, wrev, seed)
    check_non_neighbours(get_edge, shape, seed)
    return wdev, per, calls


# ---- what the pre-push may leave -----------------------------------------------------------------------------------------------------

def tiles_of(shape):
    """(tile number per voxel, number of tiles)"""
    idx = np.indices(shape)
    tid, n = np.zeros(shape, np.int64), 1
    for a, s in enumerate(shape):
        per = (s + TILE - 1) // TILE
        tid = tid * per + idx[a] // TILE
        n *= per
    return tid, n


def both_signs(shape, tr):
    """per voxel: does its tile hold a voxel with tr > 0 AND one with tr < 0 (the only tiles a pre-push may touch)"""
    tid, n = tiles_of(shape)
    tr = np.asarray(tr).reshape(shape)
    pos = np.bincount(tid.ravel(), (tr > 0).ravel(), n) > 0
    neg = np.bincount(tid.ravel(), (tr < 0).ravel(), n) > 0
    return (pos & neg)[tid]


def push_candidates(shape, weights, tr):
    """(in-tile pairs that could carry a pre-push -- tr > 0 at one end, tr < 0 at the other, weight > 0 --, in-tile pairs)"""
    tid, _ = tiles_of(shape)
    tr = np.asarray(tr).reshape(shape)
    cand = pairs = 0
    for o in offsets(len(shape)):
        src, dst = fc._slices(shape, o)
        inside = tid[src] == tid[dst]
        w = weights[o][src]
        cand += int((inside & (w > 0) & (((tr[src] > 0) & (tr[dst] < 0)) | ((tr[src] < 0) & (tr[dst] > 0)))).sum())
        pairs += int(inside.sum())
    return cand, pairs


def check_prepush(shape, wdev, fwd, back, tr):
    """What a build with the pre-push may have stored.  ``wdev[o]``: the weights as built (w); ``fwd[o]`` / ``back[o]``: get_edge of
    every arc (p, p + o) and of its reverse, at p (r); ``tr``: tweights().  The pre-push moves p = min(excess, weight, what the
    receiver's sink link still takes) from a voxel with a source link to a neighbour IN ITS TILE with a sink link, once per pair:
    r_ij = fl(w - p), r_ji = fl(w + p), and nothing else changes.  Returns the number of arcs with r < w.

    The margins.  r_ij + r_ji against w + w: fl(w - p) is off by at most half an ulp of w, fl(w + p) (< 2 w) by at most half an ulp
    of 2 w, the test's own sum by half an ulp of it: below 2 ulp of 2 w.  Flow out of a voxel against its source link tr: a voxel
    makes at most six pushes (one per neighbour); the kernel's running excess rounds by at most half an ulp of tr per push, and what
    this test sees of a push, w - r, differs from p by the rounding of the stored residual and of the subtraction, at most an ulp of
    2 w each (w the largest weight at the voxel): 6 * (ulp(tr) + 2 ulp(2 w)).  The same for the flow into a voxel against its sink
    link."""
    nd = len(shape)
    tr = np.asarray(tr, dtype=np.float64).reshape(shape)
    tid, _ = tiles_of(shape)
    live = both_signs(shape, tr)
    out, inn, wmax = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    pushed = 0
    for o in offsets(nd):
        src, dst = fc._slices(shape, o)
        m = np.zeros(shape, bool)
        m[src] = True
        w, a, b = wdev[o][src], fwd[o][src], back[o][src]
        assert not (np.isnan(a) | np.isnan(b)).any(), "offset %s: not every arc was read" % (o,)
        ti, tj = tr[src], tr[dst]
        same = tid[src] == tid[dst]
        changed = ~_same_bits(a, w) | ~_same_bits(b, w)

        def say(bad):
            return "%s, %d pairs (w %r, r there %r, back %r, tr %r -> %r)" % (_where(shape, o, m, bad.ravel()), bad.sum(), w[bad][0], a[bad][0], b[bad][0], ti[bad][0], tj[bad][0])
        bad = changed & ~same
        assert not bad.any(), "%s: %s" % (PUSH_ACROSS_TILES, say(bad))
        bad = changed & ~live[src]
        assert not bad.any(), "%s: %s" % (PUSH_IN_QUIET_TILE, say(bad))
        bad = ~(a >= 0) | ~(b >= 0)
        assert not bad.any(), "%s: %s" % (NEGATIVE_RESIDUAL, say(bad))
        bad = (a < w) & (b < w)
        assert not bad.any(), "%s: %s" % (BOTH_LOWERED, say(bad))
        bad = ((a < w) & ~(ti > 0)) | ((b < w) & ~(tj > 0))
        assert not bad.any(), "%s: %s" % (NOT_FROM_SOURCE, say(bad))
        bad = ((a < w) & ~(tj < 0)) | ((b < w) & ~(ti < 0))
        assert not bad.any(), "%s: %s" % (NOT_TO_SINK, say(bad))
        bad = ~(np.abs((a + b) - (w + w)) <= 2 * np.spacing(w + w))
        assert not bad.any(), "%s within 2 ulp: %s" % (SUM_CHANGED, say(bad))
        there, here = np.where(a < w, w - a, 0.0), np.where(b < w, w - b, 0.0)   # pushed p -> p + o, and p + o -> p
        out[src] += there
        inn[dst] += there
        out[dst] += here
        inn[src] += here
        wmax[src] = np.maximum(wmax[src], w)
        wmax[dst] = np.maximum(wmax[dst], w)
        pushed += int((a < w).sum() + (b < w).sum())
    margin = 6 * (np.spacing(np.abs(tr)) + 2 * np.spacing(2 * wmax))
    bad = ~(out <= np.maximum(tr, 0.0) + margin)
    assert not bad.any(), "%s: voxel %s, out %r, tr %r (%d voxels)" % (SOURCE_OVERDRAWN, tuple(int(c[0]) for c in np.nonzero(bad)), out[bad][0], tr[bad][0], bad.sum())
    bad = ~(inn <= np.maximum(-tr, 0.0) + margin)
    assert not bad.any(), "%s: voxel %s, in %r, tr %r (%d voxels)" % (SINK_OVERDRAWN, tuple(int(c[0]) for c in np.nonzero(bad)), inn[bad][0], tr[bad][0], bad.sum())
    assert pushed > 0, "%s: the assertions above saw nothing but the graph as built" % NOTHING_PUSHED
    return pushed


def model_prepush(shape, weights, tr):
    """A host model of a pre-push, for the CPU tier's stand-in: per tile that holds both signs of t-link and per axis (last axis
    first), every voxel with excess pushes min(excess, weight, what the neighbour's sink link still takes) to its lower neighbour in
    the tile, then to its upper one.  Returns (residual of (p, p + o) at p, residual of (p + o, p) at p), NaN where there is no arc"""
    nd = len(shape)
    tr = np.asarray(tr, dtype=np.float64).reshape(shape)
    live = both_signs(shape, tr)
    e, d = np.where(live, np.maximum(tr, 0.0), 0.0), np.where(live, np.maximum(-tr, 0.0), 0.0)
    idx = np.indices(shape)
    fwd, back = {}, {}
    for o in reversed(offsets(nd)):
        a = axis_of(o)
        src, dst = fc._slices(shape, o)
        w = weights[o][src]
        inside = (idx[a][src] + 1) % TILE != 0
        f, b = np.full(shape, np.nan), np.full(shape, np.nan)
        p_down = np.where(inside & (e[dst] > 0) & (w > 0), np.minimum(e[dst], np.minimum(w, d[src])), 0.0)   # upper voxel -> lower
        d[src] -= p_down
        e[dst] -= p_down
        p_up = np.where(inside & (e[src] > 0) & (w > 0), np.minimum(e[src], np.minimum(w, d[dst])), 0.0)     # lower voxel -> upper
        d[dst] -= p_up
        e[src] -= p_up
        f[src] = (w - p_up) + p_down
        b[src] = (w - p_down) + p_up
        fwd[o], back[o] = f, b
    return fwd, back

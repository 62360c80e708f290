"""What tests/test_slab_cases_host.py (CPU tier) and tests/test_gpu_slab_build.py (-m gpu) share: the geometries at which each mechanism
of the Z-slab path (medpy_amd/slab.py) can go wrong, the inputs on them, a plain restatement of the split, and the comparison
of what ONE slab handle stored with what the single handle over the same volume stored.  Not a test module.

Inputs are those of tests/full_nb_cases.py (fc): the wall of every shape with its float32 and int16 image, fc.sigma_of, fc.spacing_of,
the terms and dtypes of tests/face_nb_cases.py.  One change: the lowest value of the volume is planted in its first plane and the
highest in its last, so a range (the *_linear terms) or a table (integer images) taken from one slab's planes is not the volume's.

As in fc / fn the comparison takes arrays, never a handle: the CPU tier feeds it read-backs restated in NumPy and doctored in the ways a
slab build could be wrong, and requires each to be rejected by the assertion named for it (the constants below)."""
import numpy as np

import face_nb_cases as fn
import full_nb_cases as fc
from oracle import cutcheck, energy_numpy, pipeline
from session_model import bits

TERMS = fn.TERMS
DTYPES = fn.DTYPES
TILE = 8
CONNS = (6, 26)
# (shape, slabs).  9 x 9 x 17 / 2: rank 1 owns ONE plane, rank 0's upper ghost layer is that plane, y and x end in partial tiles.
# 17 x 13 x 9 / 2 and / 3: at 3 the middle slab has a ghost layer on both sides and the last owns one plane.  24 x 8 x 8 / 3: one whole
# tile layer each.  20 x 11 x 10 / 2: uneven split (8 + 12 planes), partial last layer.  16 x 17 x 7 / 2: x inside one tile.
# 16 x 16 x 16 / 2: the full-tile control
GEOMETRIES = [((9, 9, 17), 2), ((17, 13, 9), 2), ((17, 13, 9), 3), ((24, 8, 8), 3), ((20, 11, 10), 2), ((16, 17, 7), 2), ((16, 16, 16), 2)]
SWEEP_SHAPES = [(9, 9, 17), (24, 8, 8)]   # the two smallest: get_edge of EVERY arc in both orders; elsewhere arcs_to_read()
# one term of each kind for the cuts (test_slab_cases_host.py asserts that every geometry keeps a unique minimum cut under one of them)
CUT_TERMS = ("difference_linear", "maximum_division", "difference_exponential", "maximum_power")
LOW, HIGH = -40, 230   # planted below and above everything a wall holds (0 .. 105)

# the assertions, by name
NW_NOT_SINGLE = "weight at an owned voxel is not the single handle's"
TW_NOT_SINGLE = "t-link of an owned voxel is not the single handle's"
EDGE_NOT_SINGLE = "stored arc out of an owned voxel is not the single handle's"
EDGE_NOT_WEIGHT = "stored arc out of an owned voxel is not the weight as built"
GHOST_NW = "weight at a ghost voxel is neither the single handle's nor outside"
GHOST_TW = "t-link of a ghost voxel is not the single handle's"
GHOST_EDGE = "stored arc out of a ghost voxel is not what the build leaves there"
NOT_READ = "an arc the comparison needs was not read"

_CACHE = {}


def geometry_id(g):
    return "%s-%dslabs" % (fc.shape_id(g[0]), g[1])


def offsets(conn):
    return energy_numpy.forward_offsets(3, conn)


# ---- the split -------------------------------------------------------------------------------------------------------------------------

def slab_spec(d0, rank, nranks):
    """The Z-slab split in plain words (mgc_common.h:mgc_slab_spec): the ceil(d0 / 8) tile layers are dealt to the ranks in order, rank r
    owning layers [r * n // nranks, (r + 1) * n // nranks); a slab holds its own layers and ONE more on every side that has a neighbour,
    all clipped to the volume.  More slabs than layers (some rank would own nothing) is refused: ValueError"""
    layers = -(-int(d0) // TILE)
    if nranks < 1 or not 0 <= rank < nranks or nranks > layers:
        raise ValueError("cannot cut %d planes (%d tile layers) into %d slabs" % (d0, layers, nranks))
    first, last = rank * layers // nranks, (rank + 1) * layers // nranks
    has_lo, has_hi = rank > 0, rank < nranks - 1
    return {"own0": TILE * first, "own1": min(TILE * last, d0), "plane0": TILE * (first - has_lo), "plane1": min(TILE * (last + has_hi), d0),
            "has_lo": has_lo, "has_hi": has_hi}


def spec_of(slab):
    """the same dict from a slab handle (HipSlab, SimSlab, SimSlab26)"""
    return {k: getattr(slab, k) for k in ("own0", "own1", "plane0", "plane1", "has_lo", "has_hi")}


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------

def inputs(shape):
    """fc.wall(shape) with LOW planted in the first plane and HIGH in the last (no marker voxel of a wall along x or y; a marker voxel of
    a wall along z, whose n-links count all the same): {"float32", "int16", "fg", "bg"}"""
    shape = tuple(shape)
    if ("in", shape) not in _CACHE:
        w = fc.wall(shape)
        out = {"fg": w["fg"], "bg": w["bg"]}
        for dt in DTYPES:
            img = w[dt].copy()
            img[0, 1, 1], img[-1, -2, -2] = LOW, HIGH
            out[dt] = img
        _CACHE[("in", shape)] = out
    return _CACHE[("in", shape)]


def regional(shape, term):
    """fc.regional: (float32 probability map, alpha of the term's kind)"""
    return fc.regional(tuple(shape), term)


def quarters(shape):
    """a probability map of quarters (synthetic.regional's kind, session_model.family_b's values): fc.regional's map rounded to 0, 1/4,
    .., 1 -- every product with a power of two is exact"""
    return (np.rint(fc.regional(tuple(shape), "difference_linear")[0] * 4.0) / 4.0).astype(np.float32)


def reference_cut(shape, conn, term, dtype):
    """BK on one case of the cuts, once per process: (case, pipeline.Cut, the minimum cut is unique).  Unique: the ambiguity set of the
    reference's residual graph (cutcheck.ambiguity) holds no voxel"""
    key = ("cut", tuple(shape), conn, term, dtype)
    if key not in _CACHE:
        x = inputs(shape)
        case = {"shape": tuple(shape), "term": term, "image": x[dtype], "fg": x["fg"], "bg": x["bg"], "sigma": fc.sigma_of(term), "spacing": False,
                "conn": conn, "prob": None, "alpha": None}
        ref = pipeline.graphcut_voxel(case["fg"], case["bg"], term=term, image=case["image"], sigma=case["sigma"], connectivity=conn)
        _CACHE[key] = (case, ref, not cutcheck.ambiguity(ref.graph)[2].any())
    return _CACHE[key]


def cut_weights(case):
    """{forward offset: array} of the restatement for a case of the cuts"""
    return energy_numpy.boundary_weights_offsets(case["term"], case["image"], offsets(case["conn"]), case["sigma"], case["spacing"])


def assert_same_cut(labels, case, ref, unique, what):
    """labels against BK's: voxel for voxel where the minimum cut is unique, else every differing voxel inside the reference's ambiguity
    set at equal capacity in exact rationals (cutcheck.assert_labels_equivalent)"""
    labels = np.asarray(labels, bool)
    if unique:
        differing = int((labels != ref.labels).sum())
        assert not differing, "%s: %d labels differ from BK's on a case whose minimum cut is unique" % (what, differing)
        return 0
    return cutcheck.assert_labels_equivalent(labels, ref, exact=fc.exact_edges(case["shape"], cut_weights(case), case["fg"], case["bg"]))


# ---- which arcs ------------------------------------------------------------------------------------------------------------------------

def every_arc(shape, conn):
    """{forward offset: bool array, True at p where (p, p + offset) is an arc of the volume}"""
    out = {}
    for o in offsets(conn):
        m = np.zeros(shape, bool)
        m[fc._slices(shape, o)[0]] = True
        out[o] = m
    return out


def arcs_to_read(shape, conn, seed=0):
    """The arcs get_edge is asked for, as {forward offset: mask of p}.  SWEEP_SHAPES: every arc.  Elsewhere: every arc that crosses a
    tile face along any axis (a slab border is a tile face along z), every arc with an end in the first or the last plane of the volume
    (where a slab's plane offset shows), and fc.sample_pairs' sample of the others.  (get_edge cannot name an arc that leaves the volume:
    the outside markers at the volume's faces are all read, as arrays, through nweights_offset.)"""
    shape = tuple(shape)
    every = every_arc(shape, conn)
    if shape in SWEEP_SHAPES:
        return every
    idx = np.indices(shape)
    out = {}
    for o, m in every.items():
        sel = np.zeros(shape, bool)
        for a, k in enumerate(o):
            if k:
                sel |= (idx[a] + k) // TILE != idx[a] // TILE
        sel |= (idx[0] == 0) | (idx[0] + o[0] == 0) | (idx[0] == shape[0] - 1) | (idx[0] + o[0] == shape[0] - 1)
        out[o] = sel & m
    for p, o in fc.sample_pairs(shape, offsets(conn), seed)[0]:
        out[o][p] = True
    return out


def local_arcs(arcs, spec):
    """the arcs of ``arcs`` (global masks) that lie inside the planes a slab holds, as masks over those planes"""
    p0, p1 = spec["plane0"], spec["plane1"]
    out = {}
    for o, m in arcs.items():
        loc = m[p0:p1].copy()
        if o[0] > 0:   # (forward offsets: o[0] is 0 or 1) the head lies one plane up
            loc[-1] = False
        out[o] = loc
    return out


# ---- the read-backs --------------------------------------------------------------------------------------------------------------------

def read_handle(shape, conn, nweights_offset, tweights, get_edge, arcs):
    """Everything the comparison takes from one handle over a volume of ``shape`` (a slab: the planes it holds; node ids are local):
    {"shape", "nw": {offset, both directions: nweights_offset}, "tw": tweights, "arcs": the masks read, "fwd" / "back": {forward offset:
    get_edge(p, p + o) / get_edge(p + o, p) at p, NaN where not read}, "calls"}"""
    shape = tuple(shape)
    nw = {}
    for o in offsets(conn):
        nw[o], nw[fc.negated(o)] = np.asarray(nweights_offset(o)), np.asarray(nweights_offset(fc.negated(o)))
    st = fn.strides(shape)
    fwd, back, calls = {}, {}, 0
    for o, m in arcs.items():
        step = sum(k * s for k, s in zip(o, st))
        f, b = np.full(int(np.prod(shape)), np.nan), np.full(int(np.prod(shape)), np.nan)
        for i in np.flatnonzero(m.ravel()).tolist():
            f[i] = get_edge(i, i + step)
            b[i] = get_edge(i + step, i)
        calls += 2 * int(m.sum())
        fwd[o], back[o] = f.reshape(shape), b.reshape(shape)
    return {"shape": shape, "nw": nw, "tw": np.asarray(tweights(), dtype=np.float64).reshape(shape), "arcs": arcs, "fwd": fwd, "back": back, "calls": calls}


def _first(mask, bad):
    """the first voxel of ``mask`` at which ``bad`` (one entry per True of mask) holds"""
    k = np.flatnonzero(bad)[0]
    return tuple(int(c[k]) for c in np.nonzero(mask))


def _differs(a, b):
    return bits(a) != bits(b)


def check_slab_build(slab_reads, single_reads, spec, conn, prepush=False):
    """What one slab's build stored against the single handle's over the same volume (both: read_handle), bit for bit.

    For every arc whose TAIL is a voxel the slab owns -- arcs into a ghost plane and the outside markers (NaN) at the true faces of the
    volume included -- nweights_offset (every offset, both directions), tweights and get_edge are the single handle's at the global
    voxel; without a pre-push get_edge is also nweights_offset at the voxel the arc leaves (fn.check_stored's rule).  With one
    (``prepush``) the stored arcs still have to be the single handle's: the pre-push of either neighbourhood moves flow between voxels
    of ONE tile and reads nothing outside it, and a slab's tiles are the volume's tiles (slabs are cut at tile layers).

    For the voxels of ghost planes, what the build does ("What a slab's build stores"): the ghost layers are built from the
    slab's own copy of their planes like any other layer, so nweights_offset and tweights are the single handle's -- except that an arc
    whose head lies outside the planes the slab holds is "outside" (NaN) although the volume goes on there.  At the 6-neighbourhood the
    stored arcs of a ghost voxel are the single handle's too (an arc out of the held planes cannot be named).  At the 26-neighbourhood
    mgc_build clears the residuals of the ghost layers after the build -- they only collect what is pushed over the border -- so every
    stored arc out of a ghost voxel is +0.0.

    Returns the number of stored arcs compared with the single handle's."""
    p0, p1, o0, o1 = spec["plane0"], spec["plane1"], spec["own0"], spec["own1"]
    shape, gshape = slab_reads["shape"], single_reads["shape"]
    assert shape == (p1 - p0,) + gshape[1:], "the slab holds %s, its split says planes %d .. %d of %s" % (shape, p0, p1, gshape)
    owned = np.zeros(shape, bool)
    owned[o0 - p0:o1 - p0] = True
    plane = np.indices(shape)[0]
    compared = 0
    for o, a in slab_reads["nw"].items():
        want = single_reads["nw"][o][p0:p1]
        bad = _differs(a[owned], want[owned])
        assert not bad.any(), "%s: offset %s, local voxel %s (global plane + %d): %r, single %r; %d voxels" % (
            NW_NOT_SINGLE, o, _first(owned, bad), p0, a[owned][bad][0], want[owned][bad][0], bad.sum())
        inside = (plane + o[0] >= 0) & (plane + o[0] < shape[0])
        m = ~owned & inside
        bad = _differs(a[m], want[m])
        assert not bad.any(), "%s: offset %s, local voxel %s, the head lies in the held planes: %r, single %r; %d voxels" % (
            GHOST_NW, o, _first(m, bad), a[m][bad][0], want[m][bad][0], bad.sum())
        m = ~owned & ~inside
        bad = ~np.isnan(a[m])
        assert not bad.any(), "%s: offset %s, local voxel %s, the head lies outside the held planes: %r; %d voxels" % (
            GHOST_NW, o, _first(m, bad), a[m][bad][0], bad.sum())
    a, want = slab_reads["tw"], single_reads["tw"][p0:p1]
    bad = _differs(a[owned], want[owned])
    assert not bad.any(), "%s: local voxel %s: %r, single %r; %d voxels" % (TW_NOT_SINGLE, _first(owned, bad), a[owned][bad][0], want[owned][bad][0], bad.sum())
    bad = _differs(a[~owned], want[~owned])
    assert not bad.any(), "%s: local voxel %s: %r, single %r; %d voxels" % (GHOST_TW, _first(~owned, bad), a[~owned][bad][0], want[~owned][bad][0], bad.sum())
    for o, m in slab_reads["arcs"].items():
        src, dst = fc._slices(shape, o)
        head_owned = np.zeros(shape, bool)
        head_owned[src] = owned[dst]
        # the arc p -> p + o leaves p, its reverse leaves p + o: (which read-back, tail owned?, nweights_offset at the tail, moved to p)
        at_head = np.full(shape, np.nan)
        at_head[src] = slab_reads["nw"][fc.negated(o)][dst]
        for name, tail_owned, weight in (("fwd", owned, slab_reads["nw"][o]), ("back", head_owned, at_head)):
            got, ref, was_read = slab_reads[name][o], single_reads[name][o][p0:p1], single_reads["arcs"][o][p0:p1]
            mine = m & tail_owned
            assert was_read[mine].all(), "%s: offset %s (%s), of the single handle" % (NOT_READ, o, name)
            assert not np.isnan(got[m]).any(), "%s: offset %s (%s), of the slab" % (NOT_READ, o, name)
            bad = _differs(got[mine], ref[mine])
            assert not bad.any(), "%s: %s arc at local voxel %s + %s: %r, single %r; %d arcs of %d" % (
                EDGE_NOT_SINGLE, name, _first(mine, bad), o, got[mine][bad][0], ref[mine][bad][0], bad.sum(), mine.sum())
            if not prepush:
                bad = _differs(got[mine], weight[mine])
                assert not bad.any(), "%s: %s arc at local voxel %s + %s: %r, weight %r; %d arcs of %d" % (
                    EDGE_NOT_WEIGHT, name, _first(mine, bad), o, got[mine][bad][0], weight[mine][bad][0], bad.sum(), mine.sum())
            compared += int(mine.sum())
            ghost = m & ~tail_owned
            if not ghost.any():
                continue
            if conn == 26:
                bad = _differs(got[ghost], np.zeros(int(ghost.sum())))
                assert not bad.any(), "%s: %s arc at local voxel %s + %s is %r, not +0.0; %d arcs of %d" % (
                    GHOST_EDGE, name, _first(ghost, bad), o, got[ghost][bad][0], bad.sum(), ghost.sum())
            else:
                known = ghost & was_read
                bad = _differs(got[known], ref[known])
                assert not bad.any(), "%s: %s arc at local voxel %s + %s: %r, single %r; %d arcs of %d" % (
                    GHOST_EDGE, name, _first(known, bad), o, got[known][bad][0], ref[known][bad][0], bad.sum(), known.sum())
    return compared


# ---- the read-backs restated in NumPy (the CPU tier's stand-in for a handle) -------------------------------------------------------------

class HostHandle(object):
    """nweights_offset / tweights / get_edge of a handle over ``image`` (a volume, or the planes a slab holds), served from arrays made
    with oracle/energy_numpy.py -- to be doctored.  ``w``: what the library re-evaluates, ``rcap``: what the build stored."""

    def __init__(self, term, image, spacing, conn, tr, weights=None):
        self.shape, self.conn = image.shape, conn
        fwd = weights if weights is not None else energy_numpy.boundary_weights_offsets(term, image, offsets(conn), fc.sigma_of(term), spacing)
        self.w = {}
        for o in offsets(conn):
            src, dst = fc._slices(self.shape, o)
            rev = np.full(self.shape, np.nan)
            rev[dst] = fwd[o][src]
            self.w[o], self.w[fc.negated(o)] = np.array(fwd[o], dtype=np.float64), rev
        self.rcap = {o: a.copy() for o, a in self.w.items()}
        self.tr = np.asarray(tr, dtype=np.float64).reshape(self.shape).copy()

    def prepush(self):
        """store what fn.model_prepush leaves (6-neighbourhood): the residuals of a pair differ from its weight and from each other"""
        assert self.conn == 6
        fwd, back = fn.model_prepush(self.shape, {o: self.w[o] for o in offsets(6)}, self.tr)
        for o in offsets(6):
            src, dst = fc._slices(self.shape, o)
            self.rcap[o] = fwd[o]
            self.rcap[fc.negated(o)] = np.full(self.shape, np.nan)
            self.rcap[fc.negated(o)][dst] = back[o][src]
        return self

    def slab(self, spec):
        """the handle of one slab cut from this (whole-volume) handle as the library cuts it: the held planes, arcs out of them outside,
        the stored arcs of the ghost layers cleared at the 26-neighbourhood"""
        p0, p1 = spec["plane0"], spec["plane1"]
        out = object.__new__(HostHandle)
        out.shape, out.conn = (p1 - p0,) + self.shape[1:], self.conn
        out.w = {o: a[p0:p1].copy() for o, a in self.w.items()}
        out.rcap = {o: a[p0:p1].copy() for o, a in self.rcap.items()}
        out.tr = self.tr[p0:p1].copy()
        for o in out.w:
            for arrays in (out.w, out.rcap):
                if o[0] > 0:
                    arrays[o][-1] = np.nan
                elif o[0] < 0:
                    arrays[o][0] = np.nan
            if self.conn == 26:
                out.rcap[o][:spec["own0"] - p0] = 0.0
                out.rcap[o][spec["own1"] - p0:] = 0.0
        return out

    def nweights_offset(self, o):
        return self.w[tuple(o)]

    def tweights(self):
        return self.tr

    def get_edge(self, i, j):
        p, q = np.unravel_index(i, self.shape), np.unravel_index(j, self.shape)
        o = tuple(int(b) - int(a) for a, b in zip(p, q))
        v = float(self.rcap[o][p]) if o in self.rcap else 0.0
        return 0.0 if np.isnan(v) else v   # (an arc out of the held planes: nothing stored)

    def reads(self, arcs):
        return read_handle(self.shape, self.conn, self.nweights_offset, self.tweights, self.get_edge, arcs)

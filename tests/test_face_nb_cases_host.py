"""CPU tier: what tests/test_gpu_face_nb_build.py (-m gpu, the build of the 6-neighbourhood arc by arc) stands on, checked with the
oracle alone.

(1) The inputs (tests/face_nb_cases.py).  On the REFERENCE's cut at connectivity 2 * ndim: (a) the source side holds 10 % to 90 % of
the unmarked voxels wherever there are at least 100 of them, (b) the reference's ambiguity set is at most 5 % of them, (c) a case with
the regional map differs from the same case without it in at least 1 % of them, (d) at least 5 % of the pairs that lie inside one
8 x 8 x 8 tile could carry a pre-push: a source link at one end, a sink link at the other, a weight above zero.  Conditions, not
measurements: an input that breaks one is changed, never the bound.

(2) The comparisons.  A stand-in for the device made on the host from the oracle's own weights passes them as it is; doctored in each of
the ways k_build<false, ...> could be subtly wrong -- what it stores differs from what the library re-evaluates -- it is rejected by
the functions the GPU tests call, each time by the assertion named for the fault."""
import re

import numpy as np
import pytest

import face_nb_cases as fn
import full_nb_cases as fc
from oracle import energy_numpy

MIN_VOXELS = 100


def _assert_conditions(case, ref, what):
    n, share, amb = fc.cut_facts(case, ref)
    if n >= MIN_VOXELS:
        assert 0.10 <= share <= 0.90, "%s: source share %.3f of %d unmarked voxels" % (what, share, n)
        assert amb <= 0.05, "%s: ambiguity share %.4f of %d unmarked voxels" % (what, amb, n)
    return n, share, amb


@pytest.mark.parametrize("dtype", fn.DTYPES)
@pytest.mark.parametrize("term", fn.TERMS)
def test_wall_cases_cut_away_from_the_seed(term, dtype):
    for shape in fn.SHAPES:
        for spacing_on in (False, True):
            case, ref = fn.reference(shape, term, dtype, spacing_on)
            assert case["conn"] == 2 * len(shape)
            _assert_conditions(case, ref, "%s %s %s spacing %d" % (fc.shape_id(shape), term, dtype, spacing_on))


@pytest.mark.parametrize("dtype", fn.DTYPES)
@pytest.mark.parametrize("term", fn.TERMS)
def test_regional_cases_move_the_cut_and_leave_pairs_to_pre_push(term, dtype):
    for shape in fn.PREPUSH_SHAPES:
        case, ref = fn.reference(shape, term, dtype, False, with_regional=True)
        _, plain = fn.reference(shape, term, dtype, False)
        what = "%s %s %s + regional" % (fc.shape_id(shape), term, dtype)
        _assert_conditions(case, ref, what)
        free = ~(case["fg"] | case["bg"])
        moved = float((ref.labels != plain.labels)[free].mean())
        assert moved >= 0.01, "%s: the map moves %.4f of the unmarked voxels" % (what, moved)
        tr = fc.merged_tlinks(case["fg"], case["bg"], case["prob"], case["alpha"])
        cand, pairs = fn.push_candidates(shape, fn.expected_weights(term, case["image"], False)[1], tr)
        print("%s: %d of %d in-tile pairs could carry a pre-push" % (what, cand, pairs))
        assert cand >= 0.05 * pairs, "%s: %d of %d in-tile pairs could carry a pre-push" % (what, cand, pairs)


def test_regional_only_cases():
    for shape in fn.PREPUSH_SHAPES:
        case, ref = fn.reference_regional_only(shape)
        _assert_conditions(case, ref, "%s regional only" % fc.shape_id(shape))
        tr = fc.merged_tlinks(case["fg"], case["bg"], case["prob"], case["alpha"]).reshape(shape)
        assert np.array_equal(ref.labels, tr >= 0) or np.array_equal(ref.labels, tr > 0)   # no n-link: the sign of the t-link


def test_the_arc_sets():
    for shape in fn.SHAPES:
        every, border = fn.every_arc(shape), fn.border_arcs(shape)
        assert sum(int(m.sum()) for m in every.values()) == sum(int(np.prod(shape)) // s * (s - 1) for s in shape)
        for o, m in border.items():
            assert not (m & ~every[o]).any()
            a = fn.axis_of(o)
            idx = np.indices(shape)
            assert m[every[o] & ((idx[a] + 1) % 8 == 0)].all()           # every arc through a tile face
            for k, n in enumerate(shape):
                assert m[every[o] & ((idx[k] == 0) | (idx[k] == n - 1))].all()   # every arc that leaves a border voxel
        read = fn.arcs_of(shape)   # every arc on the two shapes swept in full
        assert all(np.array_equal(read[o], (every if shape in fn.SWEEP_SHAPES else border)[o]) for o in every)
    assert sum(int(m.sum()) for m in fn.every_arc((17, 17, 17)).values()) == 17 * 17 * 16 * 3
    # the pairs that are no neighbours: every row end, diagonals, steps of two -- none of them one step along one axis
    for shape in fn.SHAPES:
        pairs = fn.non_neighbours(shape)
        kinds = {w.split(" along")[0] for _, _, w in pairs}
        assert "a step of two" in kinds and (len(shape) == 1 or {"a diagonal step", "the end of a row and the start of the next"} <= kinds)
        for i, j, _ in pairs:
            p, q = np.unravel_index(i, shape), np.unravel_index(j, shape)
            assert sum(abs(int(b) - int(a)) for a, b in zip(p, q)) != 1


# ---- (2) the stand-in ------------------------------------------------------------------------------------------------------------------

class HostDevice(object):
    """what the GPU tests read from a VoxelGraph as built -- nweights_offset, nweights (re-evaluated from the image: ``w``), get_edge
    (what k_build stored: ``rcap``) and tweights -- served from host arrays made from the restatement's own weights, to be doctored"""

    def __init__(self, term, image, spacing, weights=None):
        self.shape = image.shape
        offs, fwd = fn.expected_weights(term, image, spacing)
        if weights is not None:
            fwd = weights
        self.w = {}
        for o in offs:
            src, dst = fc._slices(self.shape, o)
            rev = np.full(self.shape, np.nan)
            rev[dst] = fwd[o][src]
            self.w[o], self.w[fc.negated(o)] = fwd[o].copy(), rev
        self.rcap = {o: a.copy() for o, a in self.w.items()}
        self.stray = {}   # get_edge of pairs that are no neighbours

    def nweights_offset(self, o):
        return self.w[tuple(o)]

    def nweights(self, axis):
        o = tuple(1 if k == axis else 0 for k in range(len(self.shape)))
        return np.ascontiguousarray(self.w[o][fc._slices(self.shape, o)[0]])

    def get_edge(self, i, j):
        p, q = np.unravel_index(i, self.shape), np.unravel_index(j, self.shape)
        o = tuple(int(b) - int(a) for a, b in zip(p, q))
        if o not in self.rcap:
            return self.stray.get((i, j), 0.0)
        return float(self.rcap[o][p])

    def check(self, term, image, spacing=False):
        return fn.check_build(term, image, spacing, self.nweights_offset, self.get_edge, self.nweights, seed=3)


BIG, THIN = (17, 17, 17), (7, 9, 17)
EXACT, TOLERANT = "difference_division", "difference_exponential"   # a bit-exact and a tolerance case on the float32 image
X, Y, Z = (0, 0, 1), (0, 1, 0), (1, 0, 0)   # the forward offsets by the kernel's axis names (x: the last axis)
MX, MY = (0, 0, -1), (0, -1, 0)


def _device(term, shape=BIG, spacing=False, dtype="float32"):
    image = fc.wall(shape)[dtype]
    return HostDevice(term, image, spacing), image


def _rejected(d, term, image, name, spacing=False):
    with pytest.raises(AssertionError, match=re.escape(name)):
        d.check(term, image, spacing)


@pytest.mark.parametrize("term", [EXACT, TOLERANT, "maximum_power"])
def test_the_undoctored_stand_in_passes(term):
    for shape in fn.SHAPES:
        for dtype in fn.DTYPES:
            for spacing in (False, fc.SPACING[:len(shape)]):
                d, image = _device(term, shape, spacing, dtype)
                _, _, calls = d.check(term, image, spacing)
                if shape in fn.SWEEP_SHAPES:
                    assert calls == 2 * sum(int(m.sum()) for m in fn.every_arc(shape).values())
    image = fc.wall(BIG)["float32"]
    assert not fc.bit_exact(TOLERANT, image) and fc.bit_exact(EXACT, image) and fc.bit_exact(TOLERANT, fc.wall(BIG)["int16"])


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_1_a_lower_face_pair_taken_from_the_neighbouring_column_is_rejected(term):
    """the index into the hand-over array shifted by one along the face: the upper voxels of the pairs that enter the middle tile
    through its lower x face hold the weight of the pair one row further"""
    d, image = _device(term)
    d.rcap[MX][8:16, 8:16, 8] = d.w[MX][8:16, 9:17, 8]
    _rejected(d, term, image, fn.STORED_REVERSE)
    d, image = _device(term)
    d.rcap[MY][8:16, 8, 8:16] = d.w[MY][8:16, 8, 9:17]   # ... through its lower y face, shifted along x
    _rejected(d, term, image, fn.STORED_REVERSE)
    d, image = _device(term, THIN)   # not swept in full: the arcs through a tile face are all read
    d.rcap[MX][:, :8, 8] = d.w[MX][:, 1:9, 8]
    _rejected(d, term, image, fn.STORED_REVERSE)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_2_the_lower_face_pairs_of_the_last_partial_tile_zeroed_are_rejected(term):
    """a bounds predicate of the lower-face lanes that is wrong on a partial tile: the one voxel of the last tile finds no weight"""
    for o in (MX, MY, (-1, 0, 0)):
        d, image = _device(term)
        d.rcap[o][16, 16, 16] = 0.0
        _rejected(d, term, image, fn.STORED_REVERSE)
    d, image = _device(term, THIN)   # the last tile of the long axis is one voxel thick: its whole lower face
    d.rcap[MX][:, :, 16] = 0.0
    _rejected(d, term, image, fn.STORED_REVERSE)
    d, image = _device(term, (17, 24))
    d.rcap[(-1, 0)][16, 23] = 0.0
    _rejected(d, term, image, fn.STORED_REVERSE)


def test_3_an_arc_out_of_a_row_end_that_wraps_into_the_next_row_is_rejected():
    for shape, row in ((BIG, 100), (BIG, 288), (THIN, 5), ((17, 24), 7), ((1, 9, 17), 2)):
        d, image = _device(EXACT, shape)
        i = row * shape[-1] - 1   # the last voxel of a row
        d.stray[(i, i + 1)] = 0.25
        _rejected(d, EXACT, image, fn.NO_NEIGHBOUR)
        d, image = _device(EXACT, shape)
        d.stray[(i + 1, i)] = 0.25
        _rejected(d, EXACT, image, fn.NO_NEIGHBOUR)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_4_the_upper_voxels_copy_divided_by_another_axis_spacing_is_rejected(term):
    for shape in (BIG, THIN):
        d, image = _device(term, shape, fc.SPACING)
        plain = HostDevice(term, image, False)
        d.rcap[MX] = plain.w[MX] / fc.SPACING[1]   # the x pairs by the y spacing, in the upper voxel's copy only
        _rejected(d, term, image, fn.STORED_REVERSE, fc.SPACING)
        d, image = _device(term, shape, fc.SPACING)
        d.rcap[MY][:, 8, :] = plain.w[MY][:, 8, :] / fc.SPACING[2]   # ... on the pairs that cross a tile face only
        _rejected(d, term, image, fn.STORED_REVERSE, fc.SPACING)


@pytest.mark.parametrize("term", ["difference_exponential", "maximum_power"])
def test_5_the_table_indexed_one_entry_off_is_rejected(term):
    """on the int16 image the exponential and power terms go by table and are bit-exact: g(x + 1) for g(x)"""
    image = fc.wall(BIG)["int16"]
    prepared, nb, g = energy_numpy._prepare(term, image, fc.sigma_of(term))
    off = {}
    for o in fn.offsets(3):
        src, dst = fc._slices(BIG, o)
        off[o] = np.full(BIG, np.nan)
        off[o][src] = g(nb(prepared[src], prepared[dst]) + 1.0)
    d = HostDevice(term, image, False, weights=off)   # stored and re-evaluated alike, as one shared g(.) would give them
    _rejected(d, term, image, "weights are not bit-identical")
    d = HostDevice(term, image, False)                # in what the build stored only
    wrong = HostDevice(term, image, False, weights=off)
    d.rcap = wrong.rcap
    _rejected(d, term, image, fn.STORED_FORWARD)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_6_a_reverse_arc_that_holds_the_weight_of_the_pair_next_to_it_is_rejected(term):
    for o, q, nxt in ((MX, (3, 12, 8), (3, 13, 8)), (MY, (9, 16, 2), (9, 16, 3)), ((-1, 0, 0), (8, 0, 16), (8, 1, 16))):
        d, image = _device(term)
        assert d.w[o][q] != d.w[o][nxt]
        d.rcap[o][q] = d.w[o][nxt]
        _rejected(d, term, image, fn.STORED_REVERSE)
    d, image = _device(term)   # the forward arrays untouched, forward and reverse arc of the pair exchanged with the next pair's
    d.w[MX][3, 12, 8], d.rcap[MX][3, 12, 8] = d.w[MX][3, 13, 8], d.w[MX][3, 13, 8]
    with pytest.raises(AssertionError, match="reverse"):   # (already the array comparison: the reverse read-back is not the forward one)
        d.check(term, image)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_7_a_tile_that_carries_the_weights_of_the_tile_built_before_is_rejected(term):
    """the hand-over array not rewritten between two tiles of one workgroup: tile B stores tile A's arcs"""
    a, b = (slice(0, 8), slice(8, 16), slice(8, 16)), (slice(8, 16), slice(8, 16), slice(8, 16))
    d, image = _device(term)
    for o in d.rcap:
        d.rcap[o][b] = np.nan_to_num(d.rcap[o][a], nan=0.0)
    _rejected(d, term, image, fn.STORED_FORWARD)
    d, image = _device(term)   # ... only the lower-face planes of it (what the 192 extra lanes write)
    for o, first in ((MX, (slice(8, 16), slice(8, 16), 8)), (MY, (slice(8, 16), 8, slice(8, 16)))):
        stale = list(first)
        stale[0] = slice(0, 8)
        d.rcap[o][first] = d.rcap[o][tuple(stale)]
    _rejected(d, term, image, fn.STORED_REVERSE)


def test_a_stored_arc_one_ulp_off_is_rejected_in_a_tolerance_case_too():
    """the ulp bound is for the arrays against NumPy; what is stored against what is re-evaluated is bit for bit in every case"""
    d, image = _device(TOLERANT)
    d.rcap[X][5, 5, 5] = np.nextafter(d.rcap[X][5, 5, 5], 2.0)
    _rejected(d, TOLERANT, image, fn.STORED_FORWARD)
    d, image = _device(TOLERANT)   # both directions alike and one ulp off the arrays
    d.rcap[X][5, 5, 5] = d.rcap[MX][5, 5, 6] = np.nextafter(d.rcap[X][5, 5, 5], 2.0)
    _rejected(d, TOLERANT, image, fn.STORED_FORWARD)
    d, image = _device(EXACT)      # arrays and stored arcs alike, one ulp off the restatement, on an interior arc
    v = np.nextafter(d.w[X][5, 5, 5], 2.0)
    d.w[X][5, 5, 5] = d.w[MX][5, 5, 6] = d.rcap[X][5, 5, 5] = d.rcap[MX][5, 5, 6] = v
    _rejected(d, EXACT, image, "weights are not bit-identical")


# ---- the pre-push ----------------------------------------------------------------------------------------------------------------------

def _prepushed(shape, term="difference_exponential", dtype="float32"):
    """(weights as built, residuals there, residuals back, t-links) of the host model of a pre-push on a regional case"""
    case, _ = fn.reference(shape, term, dtype, False, with_regional=True)
    w = fn.expected_weights(term, case["image"], False)[1]
    tr = fc.merged_tlinks(case["fg"], case["bg"], case["prob"], case["alpha"]).reshape(shape)
    fwd, back = fn.model_prepush(shape, w, tr)
    return w, fwd, back, tr


def _candidate(shape, w, fwd, tr, o, crossing=False, need=None):
    """a pair (p, p + o) with tr > 0 at p and tr < 0 at p + o, inside a tile or across a tile face"""
    src, dst = fc._slices(shape, o)
    idx = np.indices(shape)
    ok = np.zeros(shape, bool)
    ok[src] = (tr[src] > 0) & (tr[dst] < 0) & (w[o][src] > 0) & (((idx[fn.axis_of(o)][src] + 1) % 8 == 0) == crossing)
    if need is not None:
        ok &= need
    assert ok.any()
    return tuple(int(c[0]) for c in np.nonzero(ok))


@pytest.mark.parametrize("term,dtype", [("difference_exponential", "float32"), ("maximum_power", "int16"), ("difference_linear", "float32")])
def test_the_modelled_pre_push_passes(term, dtype):
    for shape in fn.PREPUSH_SHAPES:
        w, fwd, back, tr = _prepushed(shape, term, dtype)
        pushed = fn.check_prepush(shape, w, fwd, back, tr)
        cand, pairs = fn.push_candidates(shape, w, tr)
        print("%s %s %s: %d arcs pushed, %d candidates among %d in-tile pairs" % (fc.shape_id(shape), term, dtype, pushed, cand, pairs))
        assert 0 < pushed <= cand


def test_the_graph_as_built_is_rejected_as_vacuous():
    for shape in fn.PREPUSH_SHAPES:
        w, fwd, back, tr = _prepushed(shape)
        asbuilt = {o: np.where(np.isnan(fwd[o]), np.nan, w[o]) for o in w}
        with pytest.raises(AssertionError, match=re.escape(fn.NOTHING_PUSHED)):
            fn.check_prepush(shape, w, asbuilt, {o: a.copy() for o, a in asbuilt.items()}, tr)


@pytest.mark.parametrize("shape", fn.PREPUSH_SHAPES, ids=fc.shape_id)
def test_a_push_recorded_on_one_side_of_a_pair_only_is_rejected(shape):
    o = fn.offsets(len(shape))[-1]
    w, fwd, back, tr = _prepushed(shape)
    pushed = np.flatnonzero((fwd[o] < w[o]).ravel())
    p = np.unravel_index(int(pushed[0]), shape)
    back[o][p] = w[o][p]   # the sender lowered its arc, the receiver's did not rise
    with pytest.raises(AssertionError, match=re.escape(fn.SUM_CHANGED)):
        fn.check_prepush(shape, w, fwd, back, tr)
    w, fwd, back, tr = _prepushed(shape)
    fwd[o][p] = w[o][p]    # ... the receiver's rose, the sender's is as built
    with pytest.raises(AssertionError, match=re.escape(fn.SUM_CHANGED)):
        fn.check_prepush(shape, w, fwd, back, tr)


@pytest.mark.parametrize("shape", fn.PREPUSH_SHAPES, ids=fc.shape_id)
def test_a_push_across_a_tile_face_is_rejected(shape):
    for o in fn.offsets(len(shape)):
        w, fwd, back, tr = _prepushed(shape)
        p = _candidate(shape, w, fwd, tr, o, crossing=True)
        amount = min(w[o][p], tr[p], -tr[tuple(c + k for c, k in zip(p, o))]) / 2
        fwd[o][p], back[o][p] = w[o][p] - amount, w[o][p] + amount
        with pytest.raises(AssertionError, match=re.escape(fn.PUSH_ACROSS_TILES)):
            fn.check_prepush(shape, w, fwd, back, tr)


def test_a_push_in_a_tile_that_holds_one_sign_of_t_link_only_is_rejected():
    shape = (17, 17, 17)
    w, fwd, back, tr = _prepushed(shape)
    tr = tr.copy()
    tr[:8, :8, :8] = np.abs(tr[:8, :8, :8]) + 0.5   # a tile of source links: nothing to push to
    fwd, back = fn.model_prepush(shape, w, tr)
    fn.check_prepush(shape, w, fwd, back, tr)
    fwd[X][2, 2, 2], back[X][2, 2, 2] = w[X][2, 2, 2] / 2, w[X][2, 2, 2] * 1.5
    with pytest.raises(AssertionError, match=re.escape(fn.PUSH_IN_QUIET_TILE)):
        fn.check_prepush(shape, w, fwd, back, tr)


@pytest.mark.parametrize("shape", fn.PREPUSH_SHAPES, ids=fc.shape_id)
def test_a_push_out_of_a_voxel_without_a_source_link_is_rejected(shape):
    o = fn.offsets(len(shape))[-1]
    src, dst = fc._slices(shape, o)
    for sender_tr in ("negative", "zero"):
        w, fwd, back, tr = _prepushed(shape)
        ok = np.zeros(shape, bool)
        ok[src] = (tr[src] < 0) & (tr[dst] < 0) & (np.indices(shape)[-1][src] % 8 != 7)
        p = tuple(int(c[0]) for c in np.nonzero(ok))
        if sender_tr == "zero":
            tr = tr.copy()
            tr[p] = 0.0
            fwd, back = fn.model_prepush(shape, w, tr)
        assert fwd[o][p] == w[o][p] == back[o][p]
        fwd[o][p], back[o][p] = w[o][p] / 2, w[o][p] * 1.5
        with pytest.raises(AssertionError, match=re.escape(fn.NOT_FROM_SOURCE)):
            fn.check_prepush(shape, w, fwd, back, tr)
    w, fwd, back, tr = _prepushed(shape)   # ... and into a voxel that has no sink link
    ok = np.zeros(shape, bool)
    ok[src] = (tr[src] > 0) & (tr[dst] > 0) & (np.indices(shape)[-1][src] % 8 != 7)
    p = tuple(int(c[0]) for c in np.nonzero(ok))
    fwd[o][p], back[o][p] = w[o][p] / 2, w[o][p] * 1.5
    with pytest.raises(AssertionError, match=re.escape(fn.NOT_TO_SINK)):
        fn.check_prepush(shape, w, fwd, back, tr)


@pytest.mark.parametrize("shape", fn.PREPUSH_SHAPES, ids=fc.shape_id)
def test_a_push_larger_than_the_receivers_sink_link_is_rejected(shape):
    o = fn.offsets(len(shape))[-1]
    src, dst = fc._slices(shape, o)
    w, _, _, tr = _prepushed(shape)
    # one push on the graph as built, where the weight and the sender's excess allow more than the receiver's sink link takes
    room = np.zeros(shape, bool)
    room[src] = (np.minimum(w[o][src], tr[src]) > -1.5 * tr[dst])
    asbuilt = {k: np.where(np.isnan(w[k]), np.nan, w[k]) for k in w}
    fwd, back = {k: a.copy() for k, a in asbuilt.items()}, {k: a.copy() for k, a in asbuilt.items()}
    p = _candidate(shape, w, fwd, tr, o, need=room)
    q = tuple(c + k for c, k in zip(p, o))
    amount = -tr[q]
    fwd[o][p], back[o][p] = w[o][p] - amount, w[o][p] + amount
    assert fn.check_prepush(shape, w, fwd, back, tr) == 1   # all of the sink link: accepted
    amount = -1.25 * tr[q]
    fwd[o][p], back[o][p] = w[o][p] - amount, w[o][p] + amount
    with pytest.raises(AssertionError, match=re.escape(fn.SINK_OVERDRAWN)):
        fn.check_prepush(shape, w, fwd, back, tr)
    # ... and two pushes out of one voxel that together exceed its source link
    w, fwd, back, tr = _prepushed(shape)
    tr = tr.copy()
    p = _candidate(shape, w, fwd, tr, o)
    q = tuple(c + k for c, k in zip(p, o))
    tr[p] = min(w[o][p], -tr[q]) / 2
    fwd, back = {k: a.copy() for k, a in asbuilt.items()}, {k: a.copy() for k, a in asbuilt.items()}
    amount = 1.25 * tr[p]
    fwd[o][p], back[o][p] = w[o][p] - amount, w[o][p] + amount
    with pytest.raises(AssertionError, match=re.escape(fn.SOURCE_OVERDRAWN)):
        fn.check_prepush(shape, w, fwd, back, tr)


def test_a_negative_residual_and_a_pair_lowered_on_both_sides_are_rejected():
    shape = (17, 24)
    o = fn.offsets(2)[-1]
    w, fwd, back, tr = _prepushed(shape)
    p = _candidate(shape, w, fwd, tr, o)
    fwd[o][p], back[o][p] = -w[o][p], 3 * w[o][p]
    with pytest.raises(AssertionError, match=re.escape(fn.NEGATIVE_RESIDUAL)):
        fn.check_prepush(shape, w, fwd, back, tr)
    w, fwd, back, tr = _prepushed(shape)
    fwd[o][p], back[o][p] = w[o][p] / 2, w[o][p] / 2
    with pytest.raises(AssertionError, match=re.escape(fn.BOTH_LOWERED)):
        fn.check_prepush(shape, w, fwd, back, tr)

"""CPU tier: what the -m gpu tests of the full neighbourhood stand on, checked with the oracle alone.

(1) The inputs (tests/full_nb_cases.py).  Label parity says nothing where the minimum cut is the surface of the seed -- labels then come
out right if no flow moves at all -- so for every case the GPU tests use, on the REFERENCE's cut: (a) the source side holds 10 % to 90 %
of the unmarked voxels wherever there are at least 100 of them, (b) the reference's ambiguity set, the only room the tie relaxation
leaves, is at most 5 % of them, (c) a case with a regional term differs from the same case without the map in at least 1 % of them.
Conditions, not measurements: an input that breaks one is changed, never the bound.

(2) The comparisons.  A stand-in for the device made on the host from the oracle's own weights passes them as it is, and every
doctored one -- the ways a 26-neighbourhood build could be subtly wrong -- is rejected by the very functions the GPU tests call."""
import numpy as np
import pytest

import full_nb_cases as fc
from oracle import cutcheck, energy_numpy

MIN_VOXELS = 100


def _assert_conditions(case, ref, what):
    n, share, amb = fc.cut_facts(case, ref)
    if n >= MIN_VOXELS:
        assert 0.10 <= share <= 0.90, "%s: source share %.3f of %d unmarked voxels" % (what, share, n)
        assert amb <= 0.05, "%s: ambiguity share %.4f of %d unmarked voxels" % (what, amb, n)
    return n, share, amb


@pytest.mark.parametrize("dtype", fc.DTYPES)
@pytest.mark.parametrize("term", fc.TERMS)
def test_wall_cases_cut_away_from_the_seed(term, dtype):
    for shape, spacing_on in fc.CUT_SHAPES:
        case, ref = fc.reference(shape, term, dtype, spacing_on)
        n, share, amb = _assert_conditions(case, ref, "%s %s %s" % (fc.shape_id(shape), term, dtype))
        if dtype == "float32" and (term.startswith("difference") or term == "maximum_division") and n >= MIN_VOXELS:
            assert amb == 0.0   # no exact ties: the GPU tests demand identical labels there


@pytest.mark.parametrize("dtype", fc.DTYPES)
@pytest.mark.parametrize("term", fc.TERMS)
def test_regional_cases_move_the_cut_without_carrying_it_to_a_marker(term, dtype):
    for shape in fc.REGIONAL_SHAPES:
        case, ref = fc.reference(shape, term, dtype, False, with_regional=True)
        _, plain = fc.reference(shape, term, dtype, False)
        what = "%s %s %s + regional" % (fc.shape_id(shape), term, dtype)
        _assert_conditions(case, ref, what)
        free = ~(case["fg"] | case["bg"])
        moved = float((ref.labels != plain.labels)[free].mean())
        assert moved >= 0.01, "%s: the map moves %.4f of the unmarked voxels" % (what, moved)
        assert case["prob"].dtype == np.float32 and 0.0 <= case["prob"].min() and case["prob"].max() <= 1.0


def test_regional_only_and_dyadic_cases():
    case, ref = fc.reference_regional_only((9, 9, 9))
    _assert_conditions(case, ref, "9x9x9 regional only")
    case, ref = fc.dyadic_ties()
    assert ref.flow == 2050.25
    assert not cutcheck.ambiguity(ref.graph)[2].any()   # labels must be identical, whatever the order of the additions
    # (not a wall: the cut closes round the background seeds and every unmarked voxel is source side.  What the case is for is its
    # arithmetic -- flow and labels bit for bit -- and its flow only comes out if every one of those seeds is saturated.)
    assert ref.labels[~case["bg"]].all() and not ref.labels[case["bg"]].any()


def test_offset_edges_lists_every_pair_once():
    shape = (3, 4, 5)
    offs = energy_numpy.forward_offsets(3, 26)
    w = energy_numpy.boundary_weights_offsets("difference_division", np.arange(60.0).reshape(shape) ** 2, offs, 3.0)
    i, j, ww = cutcheck.offset_edges(shape, w)
    ci, cj = np.stack(np.unravel_index(i, shape)), np.stack(np.unravel_index(j, shape))
    assert (np.abs(ci - cj).max(axis=0) == 1).all() and (i < j).all()
    assert len(set(zip(i.tolist(), j.tolist()))) == i.size == sum(int((~np.isnan(a)).sum()) for a in w.values())
    k = int(np.flatnonzero((i == 7) & (j == 7 + 20 + 5 + 1))[0])
    assert ww[k] == w[(1, 1, 1)][0, 1, 2]
    # ... and on the axis offsets it is lattice_edges
    ax = energy_numpy.boundary_weights("difference_division", np.arange(60.0).reshape(shape) ** 2, 3.0)
    a = sorted(zip(*[v.tolist() for v in cutcheck.lattice_edges(shape, ax)]))
    b = sorted(zip(*[v.tolist() for v in cutcheck.offset_edges(shape, {o: w[o] for o in offs if sum(map(abs, o)) == 1})]))
    assert a == b


# ---- (2) the comparisons against doctored read-backs -----------------------------------------------------------------------------

class HostDevice(object):
    """what the GPU tests read from a VoxelGraph as built -- nweights_offset, nweights, get_edge -- served from host arrays: the
    restatement's own weights at all 3^n - 1 offsets, to be doctored"""

    def __init__(self, term, image, spacing):
        self.shape = image.shape
        offs, fwd = fc.expected_weights(term, image, spacing)
        self.w = {o: a.copy() for o, a in fwd.items()}
        for o in offs:
            src, dst = fc._slices(self.shape, o)
            rev = np.full(self.shape, np.nan)
            rev[dst] = fwd[o][src]
            self.w[fc.negated(o)] = rev
        self.rcap = None   # what get_edge reads where it differs from the arrays

    def nweights_offset(self, o):
        return self.w[tuple(o)]

    def nweights(self, axis):
        o = tuple(1 if k == axis else 0 for k in range(len(self.shape)))
        return np.ascontiguousarray(self.w[o][fc._slices(self.shape, o)[0]])

    def get_edge(self, i, j):
        p, q = np.unravel_index(i, self.shape), np.unravel_index(j, self.shape)
        o = tuple(int(b - a) for a, b in zip(p, q))
        return float((self.rcap or self.w)[o][p])

    def check(self, term, image, spacing):
        return fc.check_read_backs(term, image, spacing, self.nweights_offset, self.get_edge, self.nweights, seed=3)


SHAPE = (17, 17, 17)
EXACT, TOLERANT = "difference_division", "difference_exponential"   # a bit-exact and a tolerance case on the float32 image


def _device(term, spacing=False):
    image = fc.wall(SHAPE)["float32"]
    return HostDevice(term, image, spacing), image


@pytest.mark.parametrize("term", [EXACT, TOLERANT, "maximum_power"])
@pytest.mark.parametrize("spacing", [False, fc.SPACING])
def test_the_undoctored_stand_in_passes(term, spacing):
    d, image = _device(term, spacing)
    assert not fc.bit_exact(TOLERANT, image) and fc.bit_exact(EXACT, image) and fc.bit_exact(TOLERANT, fc.wall(SHAPE)["int16"])
    d.check(term, image, spacing)
    d2 = HostDevice(term, fc.wall((17, 24))["int16"], spacing[:2] if spacing else False)
    d2.check(term, fc.wall((17, 24))["int16"], spacing[:2] if spacing else False)


def _rejected(d, term, image, spacing=False):
    with pytest.raises(AssertionError):
        d.check(term, image, spacing)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_a_diagonal_offset_exchanged_with_its_mirror_is_rejected(term):
    d, image = _device(term)
    for o in ((1, 1, 0), (1, -1, 1)):
        d, image = _device(term)
        m = fc.negated(o)
        d.w[o], d.w[m] = d.w[m], d.w[o]
        _rejected(d, term, image)
    # ... also where both arrays keep their own NaN pattern and only the values change places
    d, image = _device(term)
    o, m = (0, 1, 1), (0, 1, -1)
    a, b = d.w[o].copy(), d.w[m].copy()
    inner = (slice(None), slice(1, -1), slice(1, -1))
    d.w[o][inner], d.w[m][inner] = b[inner], a[inner]
    _rejected(d, term, image)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_two_offsets_of_equal_length_exchanged_are_rejected(term):
    for spacing in (False, fc.SPACING):
        d, image = _device(term, spacing)
        a, b = (1, 1, 0), (1, 0, 1)
        inner = (slice(0, -1), slice(0, -1), slice(0, -1))   # where both have a neighbour: the NaN patterns stay as they are
        x, y = d.w[a].copy(), d.w[b].copy()
        d.w[a][inner], d.w[b][inner] = y[inner], x[inner]
        for o in (a, b):   # (the reverse read-back follows, so that only the exchange itself is wrong)
            src, dst = fc._slices(SHAPE, o)
            d.w[fc.negated(o)][dst] = d.w[o][src]
        _rejected(d, term, image, spacing)


def test_one_ulp_in_a_bit_exact_case_and_64_ulp_in_a_tolerance_case_are_rejected():
    for term, ulps in ((EXACT, 1), (TOLERANT, 64)):
        for o in ((1, 1, 1), (0, 0, 1)):
            d, image = _device(term)
            a = d.w[o]
            p = np.unravel_index(int(np.nanargmin(a)), SHAPE)   # the smallest weight: 64 ulp of it are far below the absolute 1e-6
            a[p] += ulps * np.spacing(a[p])
            q = tuple(c + k for c, k in zip(p, o))
            d.w[fc.negated(o)][q] = a[p]
            assert ulps * np.spacing(a[p]) < 1e-3 * fc.ENERGY_TOL
            _rejected(d, term, image)
    d, image = _device(TOLERANT)   # within the bound: accepted (the bound is not zero)
    a = d.w[(1, 1, 1)]
    a[2, 3, 4] += np.spacing(a[2, 3, 4])
    d.w[(-1, -1, -1)][3, 4, 5] = a[2, 3, 4]
    d.check(TOLERANT, image, False)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_arcs_that_leave_a_tile_through_an_edge_or_a_corner_zeroed_are_rejected(term):
    """the read-backs by array recompute the weights; what k_build stored is what get_edge reads.  Face arcs and arcs inside a tile kept."""
    for crossings in ((2, 3), (3,), (2,)):
        d, image = _device(term)
        d.rcap = {o: a.copy() for o, a in d.w.items()}
        idx = np.indices(SHAPE)
        for o, a in d.rcap.items():
            crossed = sum(((idx[k] + s) // 8 != idx[k] // 8).astype(int) for k, s in enumerate(o) if s)
            a[np.isin(crossed, crossings) & ~np.isnan(a)] = 0.0
        _rejected(d, term, image)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_a_nan_pattern_shifted_by_one_voxel_on_a_volume_border_is_rejected(term):
    for o, axis in (((1, 1, 0), 1), ((0, 1, -1), 2), ((0, 0, 1), 2)):
        d, image = _device(term)
        d.w[o] = np.roll(d.w[o], 1, axis=axis)
        _rejected(d, term, image)
        d, image = _device(term)   # one border voxel only
        a = d.w[o]
        p = tuple(np.argwhere(np.isnan(a))[0])
        q = list(p)
        q[axis] += -1 if p[axis] else 1
        a[p], a[tuple(q)] = a[tuple(q)], np.nan
        _rejected(d, term, image)


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_spacing_divided_per_axis_instead_of_by_the_euclidean_length_is_rejected(term):
    d, image = _device(term, fc.SPACING)
    plain = HostDevice(term, image, False)
    for o in list(d.w):
        per_axis = 1.0
        for k, s in zip(o, fc.SPACING):
            if k:
                per_axis *= s   # (one division per axis the offset steps along: right on the axes, wrong on every diagonal)
        d.w[o] = plain.w[o] / per_axis
    for a in range(3):   # on the axis offsets nothing has changed ...
        o = tuple(1 if k == a else 0 for k in range(3))
        assert d.w[o].tobytes() == HostDevice(term, image, fc.SPACING).w[o].tobytes()
    _rejected(d, term, image, fc.SPACING)   # ... and still


@pytest.mark.parametrize("term", [EXACT, TOLERANT])
def test_a_wrong_reverse_read_back_is_rejected(term):
    for o in ((-1, -1, -1), (0, -1, 1), (0, 0, -1)):
        d, image = _device(term)
        a = d.w[o]
        p = tuple(np.argwhere(~np.isnan(a))[5])
        a[p] = np.nextafter(a[p], 2.0)
        _rejected(d, term, image)
        d, image = _device(term)   # the reverse arrays of two offsets exchanged
        m = (-1, 0, -1) if o != (-1, 0, -1) else (-1, -1, 0)
        d.w[o], d.w[m] = d.w[m], d.w[o]
        _rejected(d, term, image)


def test_the_per_axis_read_back_is_compared():
    d, image = _device(EXACT)
    good = d.nweights
    d.nweights = lambda axis: good(axis) if axis != 1 else good(axis)[::-1].copy()
    _rejected(d, EXACT, image)

"""-m gpu: what the sparse-graph path BUILDS, arc by arc.  Every comparison reads the whole graph as built through
``SparseGraph.arcs()`` (msg_get_arcs) and holds tail, head and capacity of every arc against a plain statement of the same
operation: ``expected_arcs`` of tests/sparse_cases.py (Graph::sum_edge), oracle/energy_numpy.py (the eight voxel terms on any
number of axes), oracle/energy_label_numpy.py (the three region terms), numpy.bincount (region sums).  A kernel that loses,
duplicates or misplaces an arc fails here with the arc's name even where the cut of an easy graph would still come out right:
k_msg_lattice_edges, k_msg_label_flags / k_msg_label_edges, k_msg_arc_keys / _heads / _sums, k_msg_rows, k_msg_reverse (through the
solves of test_gpu_sparse_solve.py), k_msg_tails, and the loader mgc_load_as_double that the lattice builder k_build shares."""
import ctypes as C

import numpy as np
import pytest

import sparse_cases as sc
from oracle import energy_label_numpy as eln, energy_numpy

pytestmark = pytest.mark.gpu

TERMS = energy_numpy.TERMS
SPACING = (1.3, 0.7, 2.9, 1.1, 0.9, 3.3, 1.7, 0.6)   # none a power of two: the division rounds
REL = 1e-12   # the device's exp / pow against NumPy's: the tolerance of test_gpu_labels.py:test_four_dimensional_voxel_graph (no table on this path)


def _exact(term):
    return term.split("_")[1] in ("linear", "division")


def _edges_added(g):
    from medpy_amd import _lib
    e = C.c_int64(-1)
    assert _lib.load().msg_get_counts(g._h, None, C.byref(e), None) == _lib.OK
    return e.value


def _read(g):
    arcs = g.arcs()
    assert g.get_arc_num() == arcs[0].size
    return arcs


# ---- a. edge lists (msg_add_edges) ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("calls", [1, 3, 40])
@pytest.mark.parametrize("name", sc.BUILD_CASES)
def test_edge_lists_are_summed_like_sum_edge(name, calls):
    """bit-identical to ``expected_arcs``, whether the edges come in 1, 3 or 40 calls (msg_reserve grows past its first 1 024 entries)"""
    from medpy_amd.graphcut import GraphDouble
    n, i, j, cap, rev, once, tr, fc = sc.case(name)
    g = GraphDouble(n, 0)
    for part in np.array_split(np.arange(i.size), calls):
        if part.size:
            g._add_edges(i[part], j[part], cap[part], rev[part])
    assert _edges_added(g) == i.size
    want = sc.arcs_of(name)
    sc.check_arcs(_read(g), want, "%s in %d calls" % (name, calls))
    if calls == 3:
        tail, head, c = want
        rng = np.random.default_rng(17)
        for k in rng.choice(tail.size, 20, replace=False).tolist():
            assert g.get_edge(int(tail[k]), int(head[k])) == c[k], "get_edge(%d, %d)" % (tail[k], head[k])
        have = set(zip(tail.tolist(), head.tolist()))
        absent = [(a, b) for a, b in rng.integers(0, n, (400, 2)).tolist() if a != b and (a, b) not in have][:5]
        assert len(absent) == 5
        for a, b in absent:
            assert g.get_edge(a, b) == 0.0, "get_edge(%d, %d) of an absent pair" % (a, b)
    g.close()


# ---- b. lattice edges (msg_add_lattice_edges) -------------------------------------------------------------------------------------------

def _lattice_expected(term, image, sigma, spacing, nodes=None):
    """oracle/energy_numpy.py:boundary_weights laid out as arcs: p -> p + stride_d and back, both w; axis 0 first, each in C order"""
    image = np.asarray(image)
    with np.errstate(all="ignore"):
        ws = energy_numpy.boundary_weights(term, image, sigma, spacing)
    ids = np.arange(image.size, dtype=np.int64).reshape(image.shape)
    ii, jj, ww = [], [], []
    for d, w in enumerate(ws):
        lo, hi = [slice(None)] * image.ndim, [slice(None)] * image.ndim
        lo[d], hi[d] = slice(None, -1), slice(1, None)
        ii.append(ids[tuple(lo)].ravel()); jj.append(ids[tuple(hi)].ravel()); ww.append(np.asarray(w, np.float64).ravel())
    i, j, w = np.concatenate(ii), np.concatenate(jj), np.concatenate(ww)
    return sc.expected_arcs(nodes or image.size, i, j, w, w), i.size


def _lattice_graph(term, image, sigma, spacing, nodes=None):
    from medpy_amd.graphcut import GraphDouble
    g = GraphDouble(nodes or int(np.prod(np.shape(image))), 0)
    g._add_lattice_edges(term, image, None if term.endswith("linear") else sigma, spacing)
    return g


def _check_lattice(term, image, sigma, spacing, what, nodes=None):
    want, n_edges = _lattice_expected(term, _as_the_library_takes_it(image), sigma, spacing, nodes)
    g = _lattice_graph(term, image, sigma, spacing, nodes)
    assert _edges_added(g) == n_edges, (what, _edges_added(g), n_edges)
    sc.check_arcs(_read(g), want, what, None if _exact(term) else REL)
    return g


def _as_the_library_takes_it(image):
    """the image as the library takes it (SparseGraph._image): bool as uint8, float16 as float32 -- the reference has no answer for a
    bool image (NumPy refuses to subtract booleans), and for float16 the project's definition is the float32 image"""
    image = np.asarray(image)
    if image.dtype == np.bool_:
        return image.astype(np.uint8)
    if image.dtype == np.float16:
        return image.astype(np.float32)
    return image


SHAPES = [(7,), (5, 6), (4, 5, 3), (3, 4, 2, 5), (2, 3, 2, 3, 2), (2,) * 8, (1, 6), (5, 1, 4), (1, 1, 1, 3)]


@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lattice_edges_every_term_and_shape(shape, term):
    """1 to 8 axes, axes of extent 1 (no pair along them), with and without spacing: the linear and division terms bit for bit, the
    exponential and power terms within rel 1e-12"""
    rng = np.random.default_rng(100 + len(shape) + sum(shape))
    image = (40.0 * rng.random(shape) + 25.0 * (rng.random(shape) < 0.2)).astype(np.float32)
    for spacing in (False, SPACING[:len(shape)]):
        g = _check_lattice(term, image, 11.0, spacing, "%s on %s, spacing %s" % (term, shape, bool(spacing)))
        g.close()


def test_lattice_edges_on_one_voxel_and_on_a_graph_with_more_nodes():
    """(1,): no pair, no arc, and maxflow() still answers.  More nodes than voxels: the same arcs, empty rows behind them."""
    g = _lattice_graph("difference_linear", np.array([3.0]), None, False)
    assert _edges_added(g) == 0 and g.get_arc_num() == 0 and g.arcs()[0].size == 0
    assert g.maxflow() == 0.0 and g.labels().tolist() == [True]
    g.close()
    rng = np.random.default_rng(5)
    image = rng.integers(0, 200, (4, 5, 3)).astype(np.uint8)
    g = _check_lattice("difference_division", image, 9.0, SPACING[:3], "60 voxels in a graph of 75 nodes", nodes=75)
    tr = np.zeros(75)
    tr[0], tr[59], tr[60], tr[74] = 5.0, -5.0, 2.0, -3.0
    g._set_tweights_merged(tr, 0.0)
    flow = g.maxflow()
    lab = g.labels()
    assert lab[60] and not lab[74] and lab[61:74].all() and flow > 0.0   # the nodes behind the image: isolated, by the sign of their t-link
    assert g.stats()["nodes"] == 75
    g.close()


def test_lattice_edges_refusals_leave_the_edge_list_alone():
    """9 axes, more voxels than nodes, an unknown term id: MGC_ERR_INVALID each, and msg_get_counts' edges_added as it was"""
    from medpy_amd import _lib
    from medpy_amd.graphcut import GraphDouble
    lib = _lib.load()
    rng = np.random.default_rng(9)
    g = GraphDouble(512, 0)
    g._add_lattice_edges("difference_division", rng.random((4, 5, 3)).astype(np.float32), 2.0, False)
    before = _edges_added(g)
    assert before == 4 * 5 * 2 + 4 * 4 * 3 + 3 * 5 * 3
    want = g.arcs()
    with pytest.raises(_lib.MedpyHipError) as e:
        g._add_lattice_edges("difference_division", rng.random((2,) * 9).astype(np.float32), 2.0, False)
    assert e.value.code == _lib.ERR_INVALID and _edges_added(g) == before
    with pytest.raises(_lib.MedpyHipError) as e:
        g._add_lattice_edges("difference_division", rng.random((9, 8, 8)).astype(np.float32), 2.0, False)   # 576 voxels, 512 nodes
    assert e.value.code == _lib.ERR_INVALID and "voxels" in str(e.value) and _edges_added(g) == before
    image = np.ascontiguousarray(rng.random((4, 5, 3)), np.float32)
    shp = (C.c_int64 * 3)(4, 5, 3)
    for term_id in (0, 9, 99, -1):
        rc = lib.msg_add_lattice_edges(g._h, term_id, 3, shp, _lib.ptr(image), _lib.DTYPE_IDS[image.dtype], 2.0, None)
        assert rc == _lib.ERR_INVALID and b"term" in lib.msg_last_error(g._h) and _edges_added(g) == before
    got = g.arcs()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    g.close()


DTYPES = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64", "float32", "float64", "bool", "float16"]
DSHAPE = (4, 5, 3)


def _full_range(dtype, rng, lowest=True):
    """(4, 5, 3) values over the dtype's whole range, every other one near zero so that neighbouring pairs also meet at small
    differences (where the exponential and power terms are not at their floor), the two ends of the range among them.  64-bit
    integers stay below 2**53 in magnitude: the library carries an image's range in doubles.  ``lowest`` False: without the signed
    minimum (the maximum terms' own case is test_signed_minimum_*)."""
    dt = np.dtype(dtype)
    n = int(np.prod(DSHAPE))
    if dt == np.bool_:
        return rng.random(DSHAPE) < 0.5
    if dt.kind == "f":
        top = {2: 6.0e4, 4: 3.0e38, 8: 1.0e150}[dt.itemsize]
        v = np.where(rng.random(n) < 0.5, rng.uniform(-top, top, n), rng.uniform(-4.0, 4.0, n))
        v[7], v[31] = top, -top
        return v.astype(dt).reshape(DSHAPE)
    info = np.iinfo(dt)
    lo, hi = max(info.min, -(2 ** 53 - 1)), min(info.max, 2 ** 53 - 1)
    if not lowest and dt.kind == "i":
        lo = max(lo, info.min + 1)
    wide = rng.integers(lo, hi, n, dtype=np.int64 if dt.kind == "i" else np.uint64, endpoint=True)
    near = rng.integers(0 if dt.kind == "u" else -4, 5, n).astype(wide.dtype)
    v = np.where(rng.random(n) < 0.5, wide, near)
    v[7], v[31] = hi, lo
    return v.astype(dt).reshape(DSHAPE)


def _sigma_for(image):
    """3, and 30 for the 8-bit types: exp(-(x / sigma)**2) must not land among the subnormal doubles (x / sigma between 26.6 and 27.3),
    where one unit in the last place is no small relative error; differences of 8-bit values reach 80, those of wider types that
    are not near zero lie far beyond"""
    return 30.0 if np.asarray(image).dtype.itemsize == 1 else 3.0


@pytest.mark.parametrize("term", ["difference_linear", "difference_exponential", "difference_division", "difference_power", "maximum_division"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_edges_difference_terms_every_dtype_full_range(dtype, term):
    """All ten of mgc_dtype, bool and float16 (through SparseGraph._image).  The reference converts to float before it subtracts, so
    no difference wraps; only ``image.max() - image.min()`` of difference_linear is taken in the image's dtype, where it wraps for
    the signed integers (mgc_range_in_dtype) -- weights may come out negative there, in the reference as here: arcs only, no solve.
    uint64 / int64 values are limited to |v| < 2**53: the library carries the range of an image in doubles."""
    image = _full_range(dtype, np.random.default_rng(DTYPES.index(dtype)))
    g = _check_lattice(term, image, _sigma_for(image), SPACING[:3], "%s on %s over its range" % (term, dtype))
    g.close()


@pytest.mark.parametrize("term", ["maximum_linear", "maximum_exponential", "maximum_power"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_edges_maximum_terms_every_dtype_full_range(dtype, term):
    """numpy.abs(image) in the image's dtype, then the maximum of the pair: the whole range except the signed minimum"""
    image = _full_range(dtype, np.random.default_rng(50 + DTYPES.index(dtype)), lowest=False)
    g = _check_lattice(term, image, _sigma_for(image), False, "%s on %s over its range" % (term, dtype))
    g.close()


@pytest.mark.parametrize("dtype", ["int8", "int16", "int32"])
def test_lattice_edges_difference_linear_range_wraps_in_the_dtype(dtype):
    """an image that spans more than half its type's range: the reference's ``image.max() - image.min()`` wraps in the image's dtype
    and the divisor with it (mgc_range_in_dtype).  Arcs only."""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(info.bits)
    image = rng.integers(info.min // 2 - 5, info.max // 2 + 9, DSHAPE, endpoint=True).astype(dtype)
    image[0, 0, 0], image[3, 4, 2] = info.min // 2 - 5, info.max // 2 + 9
    with np.errstate(over="ignore"):
        m = float(abs(image.max() - image.min()))
    assert m != float(int(image.max()) - int(image.min()))   # it did wrap
    g = _check_lattice("difference_linear", image, None, False, "difference_linear on %s spanning %d" % (dtype, int(image.max()) - int(image.min())))
    g.close()
    lo = info.min // 2 - 5   # max - min = 2**(bits - 1): wraps onto the minimum, whose abs() is itself
    image = rng.integers(lo, lo + 2 ** (info.bits - 1), DSHAPE, endpoint=True).astype(dtype)
    image[0, 0, 0], image[3, 4, 2] = lo, lo + 2 ** (info.bits - 1)
    with np.errstate(over="ignore"):
        assert float(abs(image.max() - image.min())) == float(info.min)
    _check_lattice("difference_linear", image, None, SPACING[:3], "difference_linear on %s spanning 2**%d" % (dtype, info.bits - 1)).close()


def test_lattice_edges_float32_range_subtracted_in_float32():
    """max - min rounds in float32 (2**24 + 1 is no float32) and not in float64: the divisor is the float32 difference"""
    rng = np.random.default_rng(24)
    image = rng.uniform(0.0, 1000.0, DSHAPE).astype(np.float32)
    image[1, 2, 1], image[2, 0, 0] = np.float32(16777216.0), np.float32(-1.0)
    assert float(abs(image.max() - image.min())) != float(image.max()) - float(image.min())
    _check_lattice("difference_linear", image, None, False, "difference_linear on float32 whose range rounds").close()


SIGNED = ["int8", "int16", "int32", "int64"]


def _signed_minimum_image(dtype, shape=DSHAPE):
    """small values and the type's minimum in three voxels no two of which are neighbours (a pair of two minima has a negative
    maximum, and ``power`` of a negative base is NaN in the reference too)"""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(info.bits + 1)
    image = rng.integers(-7, 8, shape).astype(dtype)
    for p in ((0, 0, 0), (1, 2, 1), (shape[0] - 1, shape[1] - 1, shape[2] - 1)):
        image[p] = info.min
    return image


@pytest.mark.parametrize("term", ["maximum_linear", "maximum_exponential", "maximum_power"])
@pytest.mark.parametrize("dtype", SIGNED)
def test_signed_minimum_stays_negative_under_the_maximum_terms(dtype, term):
    """The reference takes numpy.abs(image) in the image's own dtype (energy_voxel.py:99 and :558), where the minimum wraps onto
    itself: numpy.abs(int16 [-32768, 5, -7]) is [-32768, 5, 7] and its max() is 7.  The weights next to such a voxel are those of its
    neighbour alone, and maximum_linear divides by the largest OTHER magnitude.  (Until the loader negated in the narrow type the
    library widened first: +32768 as the pair's maximum and as the divisor.)"""
    image = _signed_minimum_image(dtype)
    with np.errstate(over="ignore"):
        assert int(np.abs(image).max()) == 7
    for spacing in (False, SPACING[:3]):
        _check_lattice(term, image, 5.0, spacing, "%s on %s holding %d" % (term, dtype, np.iinfo(dtype).min)).close()


@pytest.mark.parametrize("term", ["maximum_linear", "maximum_exponential", "maximum_power"])
def test_signed_minimum_in_the_lattice_builder(term):
    """the same case through graph_from_voxels on a 3-D int16 image: k_build shares the loader and k_minmax.  Compared through
    nweights(); bit for bit, since the exponential and power terms of a whole-number image go by the host's table."""
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel as ev
    shape = (9, 10, 11)   # more than one tile along every axis
    image = _signed_minimum_image("int16", shape)
    image[4, 8, 9] = np.iinfo(np.int16).min   # a second tile
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    fg[0], bg[-1] = True, True
    for spacing in (False, SPACING[:3]):
        args = (image, spacing) if term.endswith("linear") else (image, 5.0, spacing)
        g = graphcut.graph_from_voxels(fg, bg, boundary_term=getattr(ev, "boundary_" + term), boundary_term_args=args)
        with np.errstate(over="ignore"):
            want = energy_numpy.boundary_weights(term, image, 5.0, spacing)
        for axis, w in enumerate(want):
            got = np.asarray(g.nweights(axis))
            assert got.shape == w.shape, (axis, got.shape, w.shape)
            bad = np.argwhere(got.view(np.uint64) != np.ascontiguousarray(w).view(np.uint64))
            assert not len(bad), "%s, axis %d: the weight at %s is %r, expected %r (%d differ)" % (
                term, axis, tuple(bad[0]), got[tuple(bad[0])], w[tuple(bad[0])], len(bad))
        g.close()


# ---- c. label edges (msg_add_label_edges through graph_from_labels) ---------------------------------------------------------------------

def _blocks(cross0, cross1):
    """17 x 23 in blocks, the labels permuted; does the first pair along axis 0 / axis 1 cross a border?"""
    rows = np.searchsorted([1, 5, 9, 13] if cross0 else [4, 8, 12, 16], np.arange(17), side="right")
    cols = np.searchsorted([1, 6, 11, 17] if cross1 else [5, 10, 15, 20], np.arange(23), side="right")
    lab = rows[:, None] * 5 + cols[None, :]
    perm = np.random.default_rng(17 + 2 * cross0 + cross1).permutation(25) + 1
    return perm[lab]


def _nearest_seed():
    """9 x 10 x 11, about 60 regions by nearest seed, a few voxels cut out as regions of their own"""
    rng = np.random.default_rng(91011)
    shape = (9, 10, 11)
    seeds = np.stack([rng.integers(0, s, 57) for s in shape], axis=1)
    idx = np.stack(np.indices(shape), axis=-1).reshape(-1, 3)
    lab = np.argmin(((idx[:, None, :] - seeds[None, :, :]) ** 2).sum(-1), axis=1).reshape(shape)
    for k, p in enumerate([(4, 5, 5), (0, 0, 0), (8, 9, 10), (2, 7, 3)]):
        lab[p] = 1000 + k
    return np.unique(lab, return_inverse=True)[1].reshape(shape) + 1


def _label_images():
    out = {"blocks_%d%d" % (a, b): _blocks(a, b) for a in (0, 1) for b in (0, 1)}
    out["seeds_3d"] = _nearest_seed()
    i4 = np.indices((4, 5, 3, 4))
    out["blocks_4d"] = np.unique((i4[0] // 2) * 1000 + (i4[1] // 2) * 100 + ((i4[2] + i4[0]) // 2) * 10 + i4[3] // 3, return_inverse=True)[1].reshape(4, 5, 3, 4) + 1
    out["stripes_axis0"] = np.repeat(np.arange(1, 13)[:, None], 9, axis=1)   # every pair along axis 0 crosses a border, none along axis 1
    out["stripes_axis1"] = np.ascontiguousarray(out["stripes_axis0"].T)
    out["line_300"] = np.random.default_rng(300).permutation(300) + 1   # one-voxel regions; the scan crosses a 256-thread block
    return out


LABEL_IMAGES = _label_images()
GRADIENT_DTYPES = ["uint8", "uint16", "int16", "int32", "float32", "float64"]


def _gradient(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        g = rng.gamma(1.0, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
        g[rng.random(shape) < 0.3] = 0.0
        return g.astype(dtype)
    hi = {"uint8": 255, "uint16": 2000, "int16": 2000, "int32": 100000}[dtype]
    g = rng.integers(0 if np.dtype(dtype).kind == "u" else -hi, hi, shape, endpoint=True)
    g[rng.random(shape) < 0.3] = 0
    return g.astype(dtype)


def _label_graph(lab, term, args):
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_label as el
    fg, bg = np.zeros(lab.shape, bool), np.zeros(lab.shape, bool)
    fg.flat[0], bg.flat[-1] = True, True
    return graphcut.graph_from_labels(lab, fg, bg, boundary_term=getattr(el, "boundary_" + term), boundary_term_args=args)


def _check_label_arcs(lab, term, args, what, rel=None):
    n = int(lab.max())
    i, j, cap, rev, once = eln.BOUNDARY[term](lab, args)
    g = _label_graph(lab, term, args)
    assert _edges_added(g) == i.size, "%s: %d edges added, the reference makes %d calls" % (what, _edges_added(g), i.size)
    sc.check_arcs(_read(g), sc.expected_arcs(n, i, j, cap, rev, once), what, rel)
    return g


@pytest.mark.parametrize("dtype", GRADIENT_DTYPES)
@pytest.mark.parametrize("image", list(LABEL_IMAGES))
def test_label_edges_stawiaski(image, dtype):
    lab = LABEL_IMAGES[image]
    grad = _gradient(lab.shape, dtype, 7)
    _check_label_arcs(lab, "stawiaski", grad, "stawiaski on %s, %s gradient" % (image, dtype)).close()


@pytest.mark.parametrize("directedness", [-0.5, 0.25, 0.9])
@pytest.mark.parametrize("dtype", GRADIENT_DTYPES)
@pytest.mark.parametrize("image", list(LABEL_IMAGES))
def test_label_edges_stawiaski_directed(image, dtype, directedness):
    """bit for bit, the duplicated first pair of every axis included (blocks_ab: it does / does not cross a border along axis 0 /
    axis 1).  At 0.9 the zero gradients meet the cap of min(1, w + beta)."""
    lab = LABEL_IMAGES[image]
    grad = _gradient(lab.shape, dtype, 8)
    grad.flat[:3] = np.asarray([3, 1, 2], grad.dtype)   # the first pair is not a tie: the extra evaluation has a direction
    _check_label_arcs(lab, "stawiaski_directed", (grad, directedness), "stawiaski_directed(%g) on %s, %s gradient" % (directedness, image, dtype)).close()
    if directedness == 0.9:
        i, j, cap, rev, once = eln.stawiaski_directed_edges(lab, grad, directedness)
        assert (np.maximum(cap, rev) == 1.0).any()   # the cap bit


@pytest.mark.parametrize("dtype", GRADIENT_DTYPES)
@pytest.mark.parametrize("image", list(LABEL_IMAGES))
def test_label_edges_difference_of_means(image, dtype):
    """whole-number images: every region sum is exact in float64 whatever its order, so the means and the weights are the reference's
    bit for bit; float images within rel 1e-9 (tree-ordered sums, the tolerance of test_graph_from_labels_matches_reference)"""
    lab = LABEL_IMAGES[image]
    img = _gradient(lab.shape, dtype, 9)
    _check_label_arcs(lab, "difference_of_means", img, "difference_of_means on %s, %s image" % (image, dtype),
                      rel=1e-9 if np.dtype(dtype).kind == "f" else None).close()


@pytest.mark.parametrize("image", ["blocks_11", "seeds_3d", "line_300"])
def test_label_edges_difference_of_means_on_a_constant_image(image):
    """max_difference is 0: every weight is DBL_MIN"""
    lab = LABEL_IMAGES[image]
    g = _check_label_arcs(lab, "difference_of_means", np.full(lab.shape, 7, np.int16), "difference_of_means on %s, constant image" % image)
    assert (g.arcs()[2] == eln.DBL_MIN).all()
    g.close()


@pytest.mark.parametrize("term", ["stawiaski", "stawiaski_directed", "difference_of_means"])
def test_label_edges_of_a_single_region(term):
    """no border, no arc -- and maxflow() still answers"""
    lab = np.ones((5, 6), np.int64)
    img = np.arange(30, dtype=np.float32).reshape(5, 6)
    g = _check_label_arcs(lab, term, (img, 0.25) if term == "stawiaski_directed" else img, "%s on one region" % term)
    assert g.get_arc_num() == 0
    g.maxflow()
    assert g.labels().shape == (1,)
    g.close()


# ---- d. region_sums (msg_region_sums) -----------------------------------------------------------------------------------------------------

def _sizes_image():
    """regions of 1, 2, 255, 256, 257 and 70 000 voxels, scattered over the image"""
    sizes = [1, 2, 255, 256, 257, 70000]
    lab = np.repeat(np.arange(1, len(sizes) + 1), sizes)
    return np.random.default_rng(70000).permutation(lab), sizes


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_sums_are_exact_on_whole_numbers(dtype):
    """whole numbers small enough that every partial sum is exact (below 2**53; below 2**24 for float32, whose sums take the float32
    accumulator): sums and counts equal numpy.bincount exactly, so an element dropped or counted twice shows"""
    from medpy_amd.graphcut.graph import region_sums
    lab, sizes = _sizes_image()
    rng = np.random.default_rng(DTYPES.index(dtype))
    dt = np.dtype(dtype)
    if dt == np.bool_:
        values = rng.random(lab.size) < 0.5
    elif dt.kind == "f":   # 70 000 * 200 < 2**24
        values = rng.integers(-200, 201, lab.size).astype(dt)
    else:
        hi = min(int(np.iinfo(dt).max), 2 ** 36)   # 70 000 * 2**36 < 2**53
        values = rng.integers(max(int(np.iinfo(dt).min), -hi), hi, lab.size, endpoint=True).astype(dt)
    sums, counts = region_sums(lab, values, len(sizes))
    want = np.bincount(lab, weights=values.astype(np.float64))[1:]
    assert counts.tolist() == sizes
    assert sums.tolist() == want.tolist(), (dtype, sums, want)


@pytest.mark.parametrize("dtype", ["int32", "float32", "float64"])
def test_region_sums_one_region_and_one_region_per_voxel(dtype):
    from medpy_amd.graphcut.graph import region_sums
    rng = np.random.default_rng(3)
    values = rng.integers(-100, 101, 3000).astype(dtype)
    sums, counts = region_sums(np.ones(3000, np.int64), values, 1)
    assert sums.tolist() == [float(values.astype(np.float64).sum())] and counts.tolist() == [3000]
    lab = rng.permutation(3000) + 1
    sums, counts = region_sums(lab.reshape(30, 100), values.reshape(30, 100), 3000)
    assert counts.tolist() == [1] * 3000
    want = np.empty(3000)
    want[lab - 1] = values
    assert sums.tolist() == want.tolist()


def test_region_sums_of_fractions():
    """float64 within rel 1e-9 of the float64 sums, float32 (float32 accumulator, another order than numpy.sum's) within rel 1e-6:
    the two tolerances of test_graph_from_labels_matches_reference for the means and for the atlas sums"""
    from medpy_amd.graphcut.graph import region_sums
    lab, sizes = _sizes_image()
    rng = np.random.default_rng(12)
    values = rng.uniform(0.5, 1.5, lab.size)   # positive: no cancellation, so that a relative tolerance means something
    sums, counts = region_sums(lab, values, len(sizes))
    want = np.bincount(lab, weights=values)[1:]
    assert counts.tolist() == sizes and np.all(np.abs(sums - want) <= 1e-9 * np.abs(want)), (sums, want)
    v32 = values.astype(np.float32)
    sums, counts = region_sums(lab, v32, len(sizes))
    want = np.bincount(lab, weights=v32.astype(np.float64))[1:]
    assert counts.tolist() == sizes and np.all(np.abs(sums - want) <= 1e-6 * np.abs(want)), (sums, want)
    assert np.array_equal(sums, sums.astype(np.float32).astype(np.float64))   # a float32 accumulator leaves float32 values

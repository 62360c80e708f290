"""Graph facade of the voxel graph-cut path.

Mirrors reference medpy/graphcut/graph.py:267-596 (``GCGraph``) and the object it wraps,
``maxflow.GraphDouble`` (lib/maxflow/src/wrapper.cpp:59-89): same method names, argument
meaning and ``ValueError`` contract -- but instead of inserting one edge per Python call into
a CPU adjacency list, the facade records what the energy terms ask for and hands whole
arrays to the HIP library, which builds the residual lattice in HBM and solves it there.
"""
import collections
import ctypes as C
import enum

import numpy

from .. import _lib
from . import histogram as _histogram
from .histogram import histogram_binning, histogram_bins, histogram_tables   # noqa: F401  (the definition of the histogram regional term)


CutSets = collections.namedtuple("CutSets", ("from_source", "to_sink", "ambiguous", "info"))   # what ``cut_sets()`` of every graph kind returns
Components = collections.namedtuple("Components", ("ids", "first", "size", "flags", "info"))   # what ``VoxelGraph.components()`` returns
ULP64 = 64 * 2.0 ** -52   # the rounding granularity of the project's parity statement, for the ``tol`` of VoxelGraph.source_side & co.


class termtype(enum.IntEnum):
    """reference lib/maxflow/src/graph.h:57-61, exposed per class by wrapper.cpp:84-87."""
    SOURCE = 0
    SINK = 1


def _holds_whole_numbers(image, block=1 << 20):
    """every value of a float array is a whole number (NaN / inf: no) -- in blocks, leaving at the first block that holds
    anything else: a 512^3 float32 volume of noise is turned away after 4 MB, and no volume-sized temporary is made"""
    flat = image.reshape(-1) if image.flags.c_contiguous else image.ravel()
    for start in range(0, flat.size, block):
        part = flat[start:start + block]
        if not numpy.array_equal(part, numpy.floor(part)):   # (NaN != NaN, inf == floor(inf): caught by the range check below)
            return False
    return True


def image_table_facts(term, image):
    """what ``boundary_table`` needs to know about an image (or about one slab of it, medpy_amd/slab.py:sync_boundary_table):
    (holds whole numbers only, min, max) -- or None when the term has no table or the image no finite range"""
    import math
    if not (term.endswith("exponential") or term.endswith("power")):
        return None
    image = numpy.asarray(image)
    if image.size == 0 or image.dtype.kind not in "iuf":
        return None
    if image.dtype.kind == "f" and not _holds_whole_numbers(image):
        return False, 0.0, 0.0   # no table whatever the range: not worth two more passes over the volume (20 - 80 ms at 512^3)
    whole = True
    lo, hi = float(image.min()), float(image.max())
    if not (math.isfinite(lo) and math.isfinite(hi)):
        return None
    return whole, lo, hi


def boundary_table_for_range(term, sigma, lo, hi, limit=65536):
    """the table of ``boundary_table`` for an image known to hold whole numbers in [lo, hi]"""
    import math
    import sys
    if not (term.endswith("exponential") or term.endswith("power")) or sigma is None:
        return None
    top = max(abs(lo), abs(hi)) if term.startswith("maximum") else hi - lo
    if top + 1 > limit:
        return None
    x = numpy.arange(int(top) + 1, dtype=float)
    if term.endswith("exponential"):
        x = numpy.power(x, 2)
        x /= math.pow(sigma, 2)
        x *= -1
        x = numpy.exp(x)
    else:
        x = 1.0 / (x + 1)
        x = numpy.power(x, sigma)
    x[x <= 0] = sys.float_info.min
    return numpy.ascontiguousarray(x, dtype=numpy.float64)


def boundary_table(term, image, sigma, limit=65536):
    """The exponential / power boundary function of an INTEGER-VALUED image by table, or None.

    On such images (CT / MR data: uint8, uint16, int16; floats that hold whole numbers) the reference's term functions see
    only whole-number arguments d = |I_p - I_q| (difference terms) or max(|I_p|, |I_q|) (maximum terms), because
    ``__skeleton_base`` casts the image to float64 first (reference energy_voxel.py:633-634).  Evaluating the term ONCE per
    possible d with the very NumPy operations the reference applies to its arrays (energy_voxel.py:226-236 / 290-300:
    power(x, 2), /= pow(sigma, 2), *= -1, exp, floor at float_info.min; 444-452 / 506-513: 1 / (x + 1), power(x, sigma), floor)
    makes the n-link weights bit-identical to the reference's -- the device's own exp / pow (OCML) is up to 2 ulp away, which
    is enough to flip a tie.  The linear and division terms are IEEE-basic arithmetic and need no table."""
    if sigma is None:
        return None
    facts = image_table_facts(term, image)
    if facts is None or not facts[0]:
        return None
    return boundary_table_for_range(term, sigma, facts[1], facts[2], limit)


FACTS_UNKNOWN = "unknown"
"""what a graph remembers of its image where ``image_table_facts`` was never asked (the term it was built with has no table)"""


def _device_image(image):
    """an image as the library takes it: C-contiguous, in one of its dtypes (bool as uint8, float16 as float32, the rest as float64)"""
    image = numpy.ascontiguousarray(image)
    if image.dtype == numpy.bool_:
        image = image.astype(numpy.uint8)
    if image.dtype == numpy.float16:
        image = image.astype(numpy.float32)
    if image.dtype not in _lib.DTYPE_IDS:
        image = image.astype(numpy.float64)
    return image


def _term_has_table(term, sigma):
    return sigma is not None and (term.endswith("exponential") or term.endswith("power"))


def normalise_boundary_update(shape, held_facts, boundary_term, boundary_term_args):
    """What ``VoxelGraph.update_boundary_term`` sends (mgc_update_boundary, include/medpy_hip.h), as a dict: ``term``, ``image``
    (None: the image the graph holds, else the array as the library takes it), ``sigma``, ``spacing``, ``table`` (the term by
    table for whole-number images, or None) and ``facts`` (``image_table_facts`` of the image the graph holds afterwards).

    ``boundary_term`` / ``boundary_term_args`` are what ``graph_from_voxels`` takes; the image in the tuple may be None.
    ``held_facts``: the table facts of the image the graph holds, ``FACTS_UNKNOWN`` where they were never taken.  Pure host code.
    NotImplementedError for ``boundary_precomputed``, for an image of another shape than the graph's, and for an exponential /
    power term on a kept image whose facts are unknown (hand the image over again); ValueError for a callable that records no
    boundary term."""
    shape = tuple(int(s) for s in shape)
    rec = _BoundaryRecorder(shape)
    boundary_term(rec, boundary_term_args)
    if rec.recorded is None:
        raise ValueError("update_boundary_term: %r recorded no built-in boundary term" % (boundary_term,))
    term, image, sigma, spacing = rec.recorded
    facts = held_facts
    if image is not None:
        image = numpy.asarray(image)
        if image.shape != shape:
            raise NotImplementedError("medpy_amd: update_boundary_term with an image of shape %s on a graph of shape %s: build it "
                                      "again with graph_from_voxels" % (image.shape, shape))
        image = _device_image(image)
        facts = image_table_facts(term, image) if _term_has_table(term, sigma) else FACTS_UNKNOWN
    table = None
    if _term_has_table(term, sigma):
        if isinstance(facts, str):
            raise NotImplementedError("medpy_amd: update_boundary_term to an exponential / power term on a graph built with another "
                                      "kind of term: whether its image holds whole numbers was never looked at, pass the image again")
        if facts is not None and facts[0]:
            table = boundary_table_for_range(term, sigma, facts[1], facts[2])
    return {"term": term, "image": image, "sigma": sigma, "spacing": tuple(spacing) if spacing else None, "table": table, "facts": facts}


def _edit_ids(shape, ids, what):
    """one argument of VoxelGraph.edit_markers as a sorted int64 array of distinct flat ids"""
    if ids is None:
        return numpy.empty(0, dtype=numpy.int64)
    nodes = 1
    for s in shape:
        nodes *= int(s)
    if isinstance(ids, tuple):   # per-axis index arrays, as numpy.nonzero returns them
        if len(ids) != len(shape):
            raise ValueError("%s: %d index arrays for a volume of %d axes" % (what, len(ids), len(shape)))
        axes = [numpy.asarray(a) for a in ids]
        if any(a.size and a.dtype.kind not in "iu" for a in axes):
            raise ValueError("%s: index arrays must hold integers" % what)
        if len({a.shape for a in axes}) != 1 or axes[0].ndim != 1:
            raise ValueError("%s: index arrays must be 1-D and of one length" % what)
        if not axes[0].size:
            return numpy.empty(0, dtype=numpy.int64)
        if any(int(a.min()) < 0 or int(a.max()) >= n for a, n in zip(axes, shape)):
            raise ValueError("%s: index outside the volume of shape %s" % (what, tuple(shape)))
        flat = numpy.ravel_multi_index(tuple(a.astype(numpy.int64) for a in axes), tuple(shape))
    else:
        flat = numpy.asarray(ids)
        if flat.ndim != 1:
            raise ValueError("%s: node ids must be a 1-D array (or a tuple of per-axis index arrays)" % what)
        if not flat.size:
            return numpy.empty(0, dtype=numpy.int64)
        if flat.dtype.kind not in "iu":
            raise ValueError("%s: node ids must be integers, not %s" % (what, flat.dtype))
        if int(flat.min()) < 0 or int(flat.max()) >= nodes:
            raise ValueError("%s: node id outside [0, %d)" % (what, nodes))
    return numpy.unique(flat.astype(numpy.int64))


def merge_marker_edits(shape, fg=None, bg=None, erase=None):
    """The list VoxelGraph.edit_markers sends (mgc_edit_markers, include/medpy_hip.h): ``(ids, ops)``, ids ascending and distinct.

    In mask terms the edit is ``fg' = (fg & ~erase) | fg_ids`` and ``bg' = (bg & ~erase) | bg_ids``.  Each argument is None, a
    1-D integer array of flat (C-order) node ids, or a tuple of per-axis index arrays as ``numpy.nonzero`` returns.  An id in
    several lists gets ONE entry: 1 = set fg, 2 = set bg, 4 = clear fg, 8 = clear bg; erase alone = 4|8, erase + fg = 1|8,
    erase + bg = 2|4, fg + bg (with or without erase) = 1|2.  An id repeated inside a list counts once.  ValueError for ids
    outside the volume, non-integer dtypes, and a tuple whose length is not the volume's ndim."""
    shape = tuple(int(s) for s in shape)
    parts = [(_edit_ids(shape, fg, "fg"), 1), (_edit_ids(shape, bg, "bg"), 2), (_edit_ids(shape, erase, "erase"), 12)]
    ids = numpy.unique(numpy.concatenate([p for p, _ in parts]))
    ops = numpy.zeros(ids.size, dtype=numpy.uint8)
    for p, bits in parts:
        ops[numpy.searchsorted(ids, p)] |= bits   # (p is distinct: a plain fancy-indexed |= sees every id once)
    ops[(ops & 1) != 0] &= 0xff ^ 4   # set wins over erase
    ops[(ops & 2) != 0] &= 0xff ^ 8
    return ids, ops


def normalise_nweight_edit(nodes_from, nodes_to, weight_there, weight_back=None):
    """What ``VoxelGraph.edit_nweights`` sends (mgc_edit_nweights, include/medpy_hip.h): ``(i, j, cap, rev)`` -- C-contiguous 1-D
    arrays of one length, ids int64, capacities float64; ``rev`` is None where ``weight_back`` is (both ways ``weight_there``).

    The arguments have the shape of ``GCGraph.set_nweight``: each a scalar or a 1-D array, scalars are broadcast to the length of
    the arrays (all scalars: one arc pair).  Pure host code; the library checks ids, neighbourhood, capacities and repeated pairs.
    ValueError for node ids that are not whole numbers, arrays of more than one axis and arrays of different lengths."""
    given = [nodes_from, nodes_to, weight_there] + ([] if weight_back is None else [weight_back])
    names = ("nodes_from", "nodes_to", "weight_there", "weight_back")
    arrays = [numpy.asarray(a) for a in given]
    for a, name in zip(arrays, names):
        if a.ndim > 1:
            raise ValueError("edit_nweights: %s must be a scalar or a 1-D array, not of shape %s" % (name, a.shape))
    for a, name in zip(arrays[:2], names):
        if a.dtype.kind not in "iu":
            raise ValueError("edit_nweights: %s must hold integers, not %s" % (name, a.dtype))
    for a, name in zip(arrays[2:], names[2:]):
        if a.dtype.kind not in "iufb":
            raise ValueError("edit_nweights: %s of dtype %s" % (name, a.dtype))
    lengths = {a.shape[0] for a in arrays if a.ndim == 1}
    if len(lengths) > 1:
        raise ValueError("edit_nweights: arrays of different lengths %s" % sorted(lengths))
    n = lengths.pop() if lengths else 1
    out = [numpy.ascontiguousarray(numpy.broadcast_to(a, (n,)), dtype=numpy.int64 if k < 2 else numpy.float64) for k, a in enumerate(arrays)]
    return out[0], out[1], out[2], (out[3] if weight_back is not None else None)


def normalise_tweight_edit(shape, nodes, weights_source, weights_sink):
    """What ``VoxelGraph.edit_tweights`` sends (mgc_edit_tweights, include/medpy_hip.h): ``(ids, source, sink)`` -- C-contiguous 1-D
    arrays of one length, ids int64 (flat, C order), weights float64.

    ``nodes``: a flat node id, a 1-D integer array of them, or a tuple of per-axis index arrays as ``numpy.nonzero`` returns
    (one per axis of ``shape``).  ``weights_source`` / ``weights_sink``: scalars or 1-D arrays; scalars are broadcast to the
    length of the arrays (all scalars: one voxel).  Pure host code; the library checks the range of flat ids, the weights and
    repeated ids.  ValueError for ids that are not whole numbers, a tuple of the wrong length or with an index outside the
    volume, arrays of more than one axis and arrays of different lengths."""
    shape = tuple(int(v) for v in shape)
    if isinstance(nodes, tuple):
        if len(nodes) != len(shape):
            raise ValueError("edit_tweights: %d index arrays for a volume of %d axes" % (len(nodes), len(shape)))
        axes = [numpy.atleast_1d(numpy.asarray(a)) for a in nodes]
        if any(a.size and a.dtype.kind not in "iu" for a in axes):
            raise ValueError("edit_tweights: index arrays must hold integers")
        if len({a.shape for a in axes}) != 1 or axes[0].ndim != 1:
            raise ValueError("edit_tweights: index arrays must be 1-D and of one length")
        if axes[0].size and any(int(a.min()) < 0 or int(a.max()) >= n for a, n in zip(axes, shape)):
            raise ValueError("edit_tweights: index outside the volume of shape %s" % (shape,))
        ids = numpy.ravel_multi_index(tuple(a.astype(numpy.int64) for a in axes), shape) if axes[0].size else numpy.empty(0, dtype=numpy.int64)
    else:
        ids = numpy.asarray(nodes)
        if ids.ndim > 1:
            raise ValueError("edit_tweights: nodes must be a scalar, a 1-D array or a tuple of per-axis index arrays, not of shape %s" % (ids.shape,))
        if ids.size and ids.dtype.kind not in "iu":
            raise ValueError("edit_tweights: nodes must hold integers, not %s" % ids.dtype)
    arrays = [ids, numpy.asarray(weights_source), numpy.asarray(weights_sink)]
    for a, name in zip(arrays[1:], ("weights_source", "weights_sink")):
        if a.ndim > 1:
            raise ValueError("edit_tweights: %s must be a scalar or a 1-D array, not of shape %s" % (name, a.shape))
        if a.dtype.kind not in "iufb":
            raise ValueError("edit_tweights: %s of dtype %s" % (name, a.dtype))
    lengths = {a.shape[0] for a in arrays if a.ndim == 1}
    if len(lengths) > 1:
        raise ValueError("edit_tweights: arrays of different lengths %s" % sorted(lengths))
    n = lengths.pop() if lengths else 1
    out = [numpy.ascontiguousarray(numpy.broadcast_to(a, (n,)), dtype=numpy.int64 if k == 0 else numpy.float64) for k, a in enumerate(arrays)]
    return out[0], out[1], out[2]


def _dense_tweight_arrays(shape, weights_source, weights_sink):
    """the two arrays of ``set_tweights_dense`` in the volume's shape and one dtype: float32 / float64 as they are, anything else --
    and two arrays of different dtypes -- as float64; arrays of the volume's shape or flat arrays of one entry per node"""
    shape = tuple(int(v) for v in shape)
    nodes = 1
    for v in shape:
        nodes *= v
    out = []
    for w, what in ((weights_source, "weights_source"), (weights_sink, "weights_sink")):
        w = numpy.asarray(w)
        if w.dtype.kind not in "iufb":
            raise ValueError("%s: weights of dtype %s" % (what, w.dtype))
        if w.shape != shape and w.shape != (nodes,):
            raise ValueError("%s of shape %s on a graph of shape %s (%d nodes)" % (what, w.shape, shape, nodes))
        if w.dtype not in (numpy.float32, numpy.float64):
            w = w.astype(numpy.float64)
        out.append(w.reshape(shape))
    if out[0].dtype != out[1].dtype:
        out = [w.astype(numpy.float64) for w in out]
    return numpy.ascontiguousarray(out[0]), numpy.ascontiguousarray(out[1])


class _HistogramTerm(object):
    """what ``GCGraph.record_regional_histogram`` records: the image (in the volume's shape), its binning and the two parameters"""
    __slots__ = ("image", "nbins", "lo", "width", "lam", "eps")

    def __init__(self, image, nbins, lo, width, lam, eps):
        self.image, self.nbins, self.lo, self.width, self.lam, self.eps = image, nbins, lo, width, lam, eps


def _same_array(a, b):
    """do two arrays view the same memory in the same way (is ``a`` the array ``b`` already went up as)?"""
    a, b = numpy.asarray(a), numpy.asarray(b)
    return a is b or (a.shape == b.shape and a.dtype == b.dtype and a.strides == b.strides
                      and a.__array_interface__["data"][0] == b.__array_interface__["data"][0])


def pad_skeleton_weights(shape, axis, weights):
    """The per-axis weight array of the reference's ``__skeleton_base`` (energy_voxel.py:644-658: extent - 1 along ``axis``, entry p =
    the pair (p, p + e_axis)) as an array of the full ``shape``: the same entries, and one more slice along ``axis`` that holds
    zeros -- the entries whose neighbour lies outside the volume, which the library ignores.  Pure host code; costs one copy of the
    array (8 bytes read and written per voxel: ~0.2 s at 512^3), which arrays of the full shape do not pay."""
    shape = tuple(int(v) for v in shape)
    weights = numpy.asarray(weights)
    want = tuple(n - 1 if k == axis else n for k, n in enumerate(shape))
    if weights.shape != want:
        raise ValueError("weights of shape %s for axis %d of a volume of shape %s (expected %s)" % (weights.shape, axis, shape, want))
    out = numpy.zeros(shape, dtype=weights.dtype)
    out[tuple(slice(0, n) for n in want)] = weights
    return out


def _dense_offset(offset_or_axis, ndim, connectivity):
    """the offset of ``set_nweights_dense`` as a tuple of ndim ints in {-1, 0, 1} that is a neighbour in this connectivity"""
    if isinstance(offset_or_axis, (int, numpy.integer)) and not isinstance(offset_or_axis, bool):
        axis = int(offset_or_axis)
        if axis < 0 or axis >= ndim:
            raise ValueError("axis %d of a %d-D volume" % (axis, ndim))
        return tuple(1 if k == axis else 0 for k in range(ndim))
    try:
        off = tuple(int(v) for v in offset_or_axis)
    except TypeError:
        raise ValueError("offset must be an axis number or a sequence of %d ints" % ndim)
    if len(off) != ndim or any(v != w for v, w in zip(off, offset_or_axis)):
        raise ValueError("offset %r: %d whole-number components expected" % (offset_or_axis, ndim))
    nz = sum(1 for v in off if v != 0)
    full = connectivity not in (None, 2 * ndim)
    if any(v < -1 or v > 1 for v in off) or nz == 0 or (not full and nz != 1):
        raise ValueError("offset %r is not a neighbour of the %s-neighbourhood" % (off, connectivity or 2 * ndim))
    return off


def _dense_array(shape, offset, w, what):
    """one weight array of ``set_nweights_dense`` in the full shape: float32 / float64 as they are, anything else as float64"""
    w = numpy.asarray(w)
    if w.dtype not in (numpy.float32, numpy.float64):
        if w.dtype.kind not in "iufb":
            raise ValueError("%s: weights of dtype %s" % (what, w.dtype))
        w = w.astype(numpy.float64)
    if w.shape != tuple(shape):
        axes = [k for k, v in enumerate(offset) if v != 0]
        if len(axes) == 1 and offset[axes[0]] == 1 and w.shape == tuple(n - 1 if k == axes[0] else n for k, n in enumerate(shape)):
            return pad_skeleton_weights(shape, axes[0], w)
        raise ValueError("%s of shape %s on a graph of shape %s" % (what, w.shape, tuple(shape)))
    return numpy.ascontiguousarray(w)


class _GeodesicTerm(object):
    """what ``GCGraph.record_regional_geodesic`` records: the parameters of the term and the image it reads (None: the boundary term's)"""

    def __init__(self, gamma, lam, step, spacing, connectivity, image):
        self.gamma, self.lam, self.step, self.spacing, self.connectivity, self.image = gamma, lam, step, spacing, connectivity, image


class VoxelGraph(object):
    """What ``graph_from_voxels`` returns: the stand-in for ``maxflow.GraphDouble``.

    Supports what callers of the reference use on the returned object
    (bin/medpy_graphcut_voxel.py:172-181, tests/graphcut_/energy_voxel.py:205-224):
    ``maxflow()``, ``what_segment(i)``, ``termtype``, ``get_edge``, ``get_node_num``,
    ``get_trcap`` -- plus bulk ``labels()`` so that nobody has to loop over voxels in Python.

    Interactive re-segmentation (extension, in the spirit of the reference's ``set_trcap`` + ``maxflow()`` again):
    ``update_markers(fg_markers, bg_markers)`` and ``update_regional_term(probability_map, alpha)`` replace the markers /
    the regional term of the graph in place.  The n-links stay in HBM as they are, the residual graph of the last cut is
    kept, and the next ``maxflow()`` continues from it (warm solve).  ``maxflow()``, ``labels()`` and
    ``what_segment()`` then describe the cut of the new inputs -- the same labels and the same flow, bit for bit, as
    ``graph_from_voxels`` of those inputs.  Explicit edges and t-weights that plug-in terms set stay part of the graph.

    A stroke of a few voxels need not cross the bus as two whole masks, nor its result as a whole label volume:
    ``edit_markers(fg, bg, erase)`` edits the masks resident in HBM by lists of voxel ids, ``changed_labels()`` returns the ids
    of the voxels whose label the next ``maxflow()`` changed, ``labels(out=previous)`` applies them to the caller's copy of the
    previous labels, and ``markers()`` reads the resident masks back.

    Is the cut unique?  After ``maxflow()``, ``source_side()`` is the source side of the SMALLEST minimum cut (``labels()`` is that
    of the largest), ``ambiguous()`` the voxels between the two -- some minimum cut has them on either side -- ``cut_is_unique()``
    whether there are none, ``cut_sets_info()`` the counts; one forward flood of the residual graph on the device.

    The histogram regional term (``energy_voxel.regional_histogram``) moves with every stroke: ``refit_regional_histogram()`` counts
    the intensities under the markers as they stand now on the device, turns the two histograms into two tables on the host and
    expands them into the t-links on the device; ``marker_histograms()`` and ``update_tweights_binned(source_table, sink_table)``
    are its two halves, for terms of the caller's own over the same bins.
    """

    termtype = termtype

    _tweights_merged = False   # the explicit t-links came from set_tweight calls merged on the host (_set_tweights_merged)

    def __init__(self, shape, device=0, connectivity=None):
        lib = _lib.load()
        if _lib.device_count() < 1:
            raise _lib.MedpyHipError(_lib.ERR_NO_DEVICE, "no HIP device visible; medpy_amd has no CPU fallback")
        self._shape = tuple(int(s) for s in shape)
        self._device = int(device)
        nd = len(self._shape)
        if nd < 1 or nd > 3:
            raise NotImplementedError("medpy_amd: %d-D lattices are not implemented (1-D..3-D are)" % nd)
        shp = (C.c_int64 * nd)(*self._shape)
        h = C.c_void_p()
        rc = lib.mgc_create(nd, shp, connectivity or 2 * nd, int(device), C.byref(h))
        self._h = h if h.value else None
        if rc != _lib.OK:
            msg = (lib.mgc_last_error(self._h) or b"").decode()
            self.close()
            raise _lib.MedpyHipError(rc, msg)
        self._nodes = int(numpy.prod(self._shape))
        self._labels = None
        self._table_facts = FACTS_UNKNOWN
        self._full_neighbourhood = bool(connectivity) and connectivity != 2 * nd
        _lib.apply_env_params(self._h)

    # -- life cycle
    def close(self):
        if getattr(self, "_h", None):
            _lib.load().mgc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        _lib.check(self._h, getattr(_lib.load(), name)(self._h, *args))

    # -- inputs (called by GCGraph)
    def _set_boundary(self, term, image, sigma, spacing):
        image = _device_image(image)
        sp = None
        if spacing:
            sp = (C.c_double * len(self._shape))(*[float(s) for s in spacing])
        self._call("mgc_set_boundary", _lib.TERM_IDS[term], _lib.ptr(image), _lib.DTYPE_IDS[image.dtype],
                   float(sigma) if sigma is not None else 0.0, sp)
        # (what update_boundary_term needs to know of an image it is told to keep: taken where the table asks for it anyway)
        self._table_facts = image_table_facts(term, image) if _term_has_table(term, sigma) else FACTS_UNKNOWN
        table = None
        if not isinstance(self._table_facts, str) and self._table_facts is not None and self._table_facts[0]:
            table = boundary_table_for_range(term, sigma, self._table_facts[1], self._table_facts[2])
        if table is not None:
            self._call("mgc_set_boundary_lut", _lib.ptr(table), table.size)

    @staticmethod
    def _prob_array(prob):
        prob = numpy.asarray(prob)
        if prob.dtype not in (numpy.float32, numpy.float64):
            prob = prob.astype(numpy.float64)  # NumPy promotes (non-float array * python float) to float64
        return numpy.ascontiguousarray(prob)

    def _set_regional(self, prob, alpha):
        prob = self._prob_array(prob)
        self._call("mgc_set_regional_probability", _lib.ptr(prob), _lib.DTYPE_IDS[prob.dtype], float(alpha))

    @staticmethod
    def _marker_bytes(m):   # a C-contiguous bool array IS the byte array the library reads: no 1-byte-per-voxel copy (0.1 s at 512^3)
        if m is None:
            return None
        m = numpy.asarray(m)
        if m.dtype in (numpy.bool_, numpy.uint8, numpy.int8) and m.flags.c_contiguous:
            return m.view(numpy.uint8)   # (the library reads "non-zero")
        return numpy.ascontiguousarray(m, dtype=numpy.bool_).view(numpy.uint8)

    def _set_markers(self, fg, bg):
        fg8, bg8 = self._marker_bytes(fg), self._marker_bytes(bg)
        self._call("mgc_set_markers", None if fg8 is None else _lib.ptr(fg8), None if bg8 is None else _lib.ptr(bg8))

    def _check_volume_shape(self, a, what):
        if a is not None and numpy.shape(a) != self._shape:
            raise ValueError("%s of shape %s on a graph of shape %s" % (what, numpy.shape(a), self._shape))

    # -- warm updates
    def update_markers(self, fg_markers, bg_markers):
        """Replace the foreground / background markers (arrays of the volume's shape, non-zero = marked; None = no markers of
        that kind) and keep the residual graph: the next ``maxflow()`` is a warm solve of the graph with the new markers."""
        self._check_volume_shape(fg_markers, "foreground markers")
        self._check_volume_shape(bg_markers, "background markers")
        fg8, bg8 = self._marker_bytes(fg_markers), self._marker_bytes(bg_markers)
        self._labels = None
        self._call("mgc_update_markers", None if fg8 is None else _lib.ptr(fg8), None if bg8 is None else _lib.ptr(bg8))

    def update_regional_term(self, probability_map, alpha):
        """Replace the regional term (foreground probability map of the volume's shape, weight ``alpha``; evaluated in the map's
        dtype as ``regional_probability_map`` does) and keep the residual graph: the next ``maxflow()`` is a warm solve."""
        self._check_volume_shape(probability_map, "probability map")
        prob = self._prob_array(probability_map)
        self._labels = None
        self._call("mgc_update_regional_probability", _lib.ptr(prob), _lib.DTYPE_IDS[prob.dtype], float(alpha))

    def update_boundary_term(self, boundary_term, boundary_term_args):
        """Replace the boundary term: the same ``energy_voxel`` function and argument tuple as ``graph_from_voxels`` takes --
        another sigma, another term, the spacing, another image of the same shape; an image of None in the tuple means the image
        the graph holds (nothing is uploaded).  The residual graph is kept and the change of every n-link folded into it
        ("The boundary term"): the next ``maxflow()`` is a warm solve with the labels and the flow of
        ``graph_from_voxels`` of the new arguments.  If the graph holds a finished cut its labels are kept on the device, so
        ``changed_labels()`` and ``labels(out=previous)`` work afterwards.  NotImplementedError for ``boundary_precomputed`` and
        for an image of another shape; MedpyHipError (ERR_UNSUPPORTED) on graphs with explicit edges or dense weight arrays."""
        u = normalise_boundary_update(self._shape, self._table_facts, boundary_term, boundary_term_args)
        sp = (C.c_double * len(self._shape))(*[float(v) for v in u["spacing"]]) if u["spacing"] else None
        image = u["image"]
        if u["table"] is not None:
            self._call("mgc_update_boundary_lut", _lib.ptr(u["table"]), u["table"].size)
        self._labels = None
        self._call("mgc_update_boundary", _lib.TERM_IDS[u["term"]], None if image is None else _lib.ptr(image),
                   _lib.DTYPE_IDS[image.dtype] if image is not None else 0, float(u["sigma"]) if u["sigma"] is not None else 0.0, sp)
        self._table_facts = u["facts"]

    def boundary_update_info(self):
        """of the last ``update_boundary_term``: arcs whose capacity changed, arcs whose flow no longer fitted, voxels whose excess
        or residual sink link changed, tiles that gained a t-link flag (mgc_get_boundary_update_info)"""
        out = numpy.zeros(4, dtype=numpy.int64)
        self._call("mgc_get_boundary_update_info", _lib.ptr(out))
        return dict(zip(("arcs_changed", "arcs_clamped", "voxels_changed", "tiles_flagged"), out.tolist()))

    # -- edits by list
    def edit_markers(self, fg=None, bg=None, erase=None):
        """Edit the markers by voxel lists instead of whole masks: ``fg' = (fg & ~erase) | fg_ids``, ``bg' = (bg & ~erase) | bg_ids``
        (see ``merge_marker_edits`` for the forms the arguments take).  Otherwise as ``update_markers``: the next ``maxflow()`` is
        a warm solve.  If the graph holds a finished cut, its labels are kept on the device for ``changed_labels()``."""
        ids, ops = merge_marker_edits(self._shape, fg, bg, erase)
        self._call("mgc_edit_markers", ids.size, _lib.ptr(ids), _lib.ptr(ops))
        if ids.size:
            self._labels = None

    def edit_nweights(self, nodes_from, nodes_to, weight_there, weight_back=None):
        """Set the capacities of n-links of the built graph by arc list (REPLACE, not add): afterwards the arc
        ``nodes_from[k] -> nodes_to[k]`` has capacity ``weight_there[k]`` and its reverse ``weight_back[k]`` (None: the same).
        Arguments in the shape of ``GCGraph.set_nweight``, scalars or 1-D arrays (``normalise_nweight_edit``); the nodes must be
        neighbours of the graph's lattice.  0 makes a one-way arc or, both ways, a barrier.  Only the listed arcs are folded into
        the residual graph ("Edits of n-links by list"): the next ``maxflow()`` is a warm solve with the labels and the
        flow of a graph built from the edited weights.  The edits stay with the graph -- a rebuild applies them again -- until
        ``clear_nweight_edits()``.  If the graph holds a finished cut its labels are kept on the device, so ``changed_labels()``
        and ``labels(out=previous)`` work afterwards.  MedpyHipError: ERR_INVALID / ERR_UNSUPPORTED name the first offending
        entry (bad id, capacity, pair twice / not neighbours); the graph is then as it was."""
        i, j, cap, rev = normalise_nweight_edit(nodes_from, nodes_to, weight_there, weight_back)
        self._call("mgc_edit_nweights", i.size, _lib.ptr(i), _lib.ptr(j), _lib.ptr(cap), None if rev is None else _lib.ptr(rev))
        if i.size:
            self._labels = None

    def clear_nweight_edits(self):
        """mgc_clear_nweight_edits: forget the capacities set by ``edit_nweights``; the graph is unbuilt afterwards"""
        self._labels = None
        self._call("mgc_clear_nweight_edits")

    def nweight_edit_info(self):
        """arc pairs the graph keeps from ``edit_nweights`` and, of the last call: pairs whose capacity changed bitwise, arcs whose
        flow no longer fitted, voxels whose excess or residual sink link changed (mgc_get_nweight_edit_info)"""
        out = numpy.zeros(4, dtype=numpy.int64)
        self._call("mgc_get_nweight_edit_info", _lib.ptr(out))
        return dict(zip(("pairs_kept", "pairs_changed", "arcs_clamped", "voxels_changed"), out.tolist()))

    def markers(self):
        """(fg, bg): the markers the graph holds now, bool arrays of the volume's shape"""
        fg = numpy.empty(self._nodes, dtype=numpy.uint8)
        bg = numpy.empty(self._nodes, dtype=numpy.uint8)
        self._call("mgc_get_markers", _lib.ptr(fg), _lib.ptr(bg))
        return fg.view(numpy.bool_).reshape(self._shape), bg.view(numpy.bool_).reshape(self._shape)

    def changed_labels(self):
        """After ``edit_markers`` (one or several) and ``maxflow()``: ascending int64 array of the flat ids of the voxels whose
        label differs from the cut the graph held before the first of those edits.  MedpyHipError (ERR_STATE) when the graph
        holds no such earlier cut (never edited by list since it was built or updated by masks) or is not solved."""
        n = C.c_int64(0)
        ids = numpy.empty(1024, dtype=numpy.int64)   # a stroke flips a few dozen labels: one call; more: the count sizes the buffer
        self._call("mgc_labels_delta", ids.size, _lib.ptr(ids), C.byref(n))
        if n.value > ids.size:
            ids = numpy.empty(n.value, dtype=numpy.int64)
            self._call("mgc_labels_delta", ids.size, _lib.ptr(ids), C.byref(n))
        return ids[:n.value].copy() if ids.size != n.value else ids

    def _add_edges(self, i, j, cap, rev):
        i = numpy.ascontiguousarray(i, dtype=numpy.int64)
        j = numpy.ascontiguousarray(j, dtype=numpy.int64)
        cap = numpy.ascontiguousarray(cap, dtype=numpy.float64)
        rev = numpy.ascontiguousarray(rev, dtype=numpy.float64)
        self._call("mgc_add_edges", i.size, _lib.ptr(i), _lib.ptr(j), _lib.ptr(cap), _lib.ptr(rev))

    def _set_tweights_merged(self, tr, flow_const):
        tr = numpy.ascontiguousarray(tr, dtype=numpy.float64)
        self._call("mgc_set_tweights_merged", _lib.ptr(tr), float(flow_const))
        self._tweights_merged = True

    # -- dense t-link weight arrays
    def _add_tweights(self, weights_source, weights_sink):
        """mgc_add_tweights: one ``add_tweights(source[p], sink[p])`` per voxel on the graph's explicit t-links; arrays of the
        volume's shape (or flat).  float32 / float64 go up as they are, anything else as float64."""
        source, sink = _dense_tweight_arrays(self._shape, weights_source, weights_sink)
        self._labels = None
        self._call("mgc_add_tweights", _lib.ptr(source), _lib.ptr(sink), _lib.DTYPE_IDS[source.dtype])

    def _clear_tweights(self):
        """mgc_clear_tweights: forget the explicit t-links (and free their store); the graph is unbuilt afterwards"""
        self._labels = None
        self._call("mgc_clear_tweights")
        self._tweights_merged = False

    def tweight_edit_info(self):
        """is the store of dense t-link arrays held, dense calls accumulated in it, and of the last ``edit_tweights`` /
        ``update_tweights_dense``: entries of the list, voxels whose explicit t-link changed bitwise (mgc_get_tweight_edit_info)"""
        out = numpy.zeros(4, dtype=numpy.int64)
        self._call("mgc_get_tweight_edit_info", _lib.ptr(out))
        return dict(zip(("store_held", "dense_calls", "list_entries", "voxels_changed"), out.tolist()))

    def _refuse_host_merged(self, what):
        if self._tweights_merged:
            raise NotImplementedError("medpy_amd: %s on a graph whose explicit t-links were merged on the host (set_tweight calls): "
                                      "the per-voxel shares of its flow constant are not known; build it from set_tweights_dense alone" % what)

    def update_tweights_dense(self, weights_source, weights_sink):
        """Replace the explicit t-links by those of ONE ``set_tweights_dense(weights_source, weights_sink)`` -- whatever dense calls
        the graph was built from -- and keep the residual graph: the next ``maxflow()`` is a warm solve with the labels and the flow
        of a graph built from the new arrays (regional probability map and markers on top, as built).  MedpyHipError (ERR_INVALID)
        names the first entry that is not finite; the graph is then as it was."""
        self._refuse_host_merged("update_tweights_dense")
        source, sink = _dense_tweight_arrays(self._shape, weights_source, weights_sink)
        self._labels = None
        self._call("mgc_update_tweights", _lib.ptr(source), _lib.ptr(sink), _lib.DTYPE_IDS[source.dtype])

    def edit_tweights(self, nodes, weights_source, weights_sink):
        """Set the explicit t-links of the built graph by voxel list (REPLACE, not add): afterwards voxel ``nodes[k]`` holds what
        one ``set_tweight(nodes[k], weights_source[k], weights_sink[k])`` leaves on a graph without explicit t-links; the regional
        probability map and the markers stay on top.  ``nodes``: flat ids or a tuple of per-axis index arrays; weights: scalars or
        1-D arrays (``normalise_tweight_edit``).  The next ``maxflow()`` is a warm solve with the labels and the flow of a graph
        built from the edited t-links; the edits stay with the graph, a rebuild sees them.  If the graph holds a finished cut its
        labels are kept on the device, so ``changed_labels()`` and ``labels(out=previous)`` work afterwards.  MedpyHipError
        (ERR_INVALID) names the first offending entry (bad id, weight that is not finite, id twice); the graph is then as it was."""
        self._refuse_host_merged("edit_tweights")
        ids, source, sink = normalise_tweight_edit(self._shape, nodes, weights_source, weights_sink)
        self._call("mgc_edit_tweights", ids.size, _lib.ptr(ids), _lib.ptr(source), _lib.ptr(sink))
        if ids.size:
            self._labels = None

    # -- the binned regional term: histograms of the markers, tables expanded on the device
    _binning = None        # (nbins, lo, width) the graph was built with (GCGraph.record_regional_histogram)
    _hist_params = None    # (lam, eps) of that term
    _hist_counts = None    # out4 of the last marker_histograms

    def _set_feature_image(self, image):
        """mgc_set_feature_image: the scalar image the bins are taken of where it is not the boundary term's own (None forgets it)"""
        if image is None:
            self._call("mgc_set_feature_image", None, 0)
            return
        image = _device_image(image)
        self._check_volume_shape(image, "feature image")
        self._call("mgc_set_feature_image", _lib.ptr(image), _lib.DTYPE_IDS[image.dtype])

    def _binned_args(self, what, nbins, lo, width):
        given = [v is not None for v in (nbins, lo, width)]
        if not any(given):
            if self._binning is None:
                raise ValueError("%s: the graph was built without a histogram term: pass nbins, lo and width" % what)
            return self._binning
        if not all(given):
            raise ValueError("%s: nbins, lo and width come together" % what)
        return _histogram._check_binning(nbins, lo, width)

    @staticmethod
    def _binned_tables(what, nbins, source_table, sink_table):
        tables = [numpy.ascontiguousarray(t, dtype=numpy.float64) for t in (source_table, sink_table)]
        for t in tables:
            if t.ndim != 1 or t.size != nbins:
                raise ValueError("%s: a table of shape %s for %d bins" % (what, t.shape, nbins))
        return tables

    def marker_histograms(self, nbins=None, lo=None, width=None):
        """``(fg_hist, bg_hist)``: per bin the voxels under the foreground and under the background markers the graph holds now
        (after ``edit_markers`` / ``update_markers`` too), int64 arrays of ``nbins`` entries, counted on the device
        (mgc_marker_histograms) -- exactly ``numpy.bincount(histogram_bins(image, nbins, lo, width)[mask], minlength=nbins)``.  The
        image is the feature image of the graph or, where none was set, the boundary term's.  No arguments: the binning the graph
        was built with.  ``marker_histogram_info()`` has the totals of this call."""
        nbins, lo, width = self._binned_args("marker_histograms", nbins, lo, width)
        fg = numpy.zeros(nbins, dtype=numpy.int64)
        bg = numpy.zeros(nbins, dtype=numpy.int64)
        out4 = numpy.zeros(4, dtype=numpy.int64)
        self._call("mgc_marker_histograms", nbins, lo, width, _lib.ptr(fg), _lib.ptr(bg), _lib.ptr(out4))
        self._hist_counts = out4
        return fg, bg

    def marker_histogram_info(self):
        """of the last ``marker_histograms``: counts under the foreground markers, under the background markers, counts whose value
        lay below ``lo`` (clamped into bin 0) and at or above ``lo + nbins * width`` (clamped into the last bin)"""
        out4 = self._hist_counts if self._hist_counts is not None else numpy.zeros(4, dtype=numpy.int64)
        return dict(zip(("fg_voxels", "bg_voxels", "below", "above"), out4.tolist()))

    def _add_tweights_binned(self, source_table, sink_table, nbins, lo, width):
        """mgc_add_tweights_binned: one ``add_tweights(source_table[bin(p)], sink_table[bin(p)])`` per voxel on the graph's explicit
        t-links -- what ``_add_tweights(source_table[bins], sink_table[bins])`` with ``bins = histogram_bins(image, nbins, lo, width)``
        leaves, without the two arrays"""
        nbins, lo, width = _histogram._check_binning(nbins, lo, width)
        source, sink = self._binned_tables("_add_tweights_binned", nbins, source_table, sink_table)
        self._labels = None
        self._call("mgc_add_tweights_binned", nbins, lo, width, _lib.ptr(source), _lib.ptr(sink))

    def update_tweights_binned(self, source_table, sink_table, nbins=None, lo=None, width=None):
        """Replace the explicit t-links by ``source_table[bin(p)]`` / ``sink_table[bin(p)]`` -- what
        ``update_tweights_dense(source_table[bins], sink_table[bins])`` leaves, bit for bit, with the tables expanded on the device
        -- and keep the residual graph: the next ``maxflow()`` is a warm solve.  ``nbins``, ``lo``, ``width`` of None: the binning
        the graph was built with.  The carrier of any regional term that depends on a voxel through its bin: smoothed histograms, a
        mixture model evaluated per bin.  MedpyHipError (ERR_INVALID) names the first table entry that is not finite; the graph is
        then as it was."""
        self._refuse_host_merged("update_tweights_binned")
        nbins, lo, width = self._binned_args("update_tweights_binned", nbins, lo, width)
        source, sink = self._binned_tables("update_tweights_binned", nbins, source_table, sink_table)
        self._labels = None
        self._call("mgc_update_tweights_binned", nbins, lo, width, _lib.ptr(source), _lib.ptr(sink))

    def refit_regional_histogram(self, lam=None, eps=None):
        """Fit the histogram regional term (``energy_voxel.regional_histogram``) to the markers as they stand now: the histograms
        of the intensities under the two kinds of marker are counted on the device, ``histogram_tables`` turns them into the two
        tables on the host, ``update_tweights_binned`` expands those into the graph's t-links.  ``lam`` / ``eps`` of None: those
        the graph was built with.  Returns ``(fg_hist, bg_hist)``.  The next ``maxflow()`` is a warm solve with the labels and the
        flow of a graph built from the markers and the refitted term; ``labels(out=previous)`` brings a copy of the previous labels
        up to date."""
        self._refuse_host_merged("refit_regional_histogram")
        if self._binning is None or self._hist_params is None:
            raise ValueError("refit_regional_histogram: the graph was built without a histogram term (energy_voxel.regional_histogram)")
        lam = self._hist_params[0] if lam is None else lam
        eps = self._hist_params[1] if eps is None else eps
        fg_hist, bg_hist = self.marker_histograms()
        source_table, sink_table = histogram_tables(fg_hist, bg_hist, lam, eps)
        self.update_tweights_binned(source_table, sink_table)
        self._hist_params = (lam, eps)
        return fg_hist, bg_hist

    # -- the term fitted to the cut instead of the strokes
    _label_hist_counts = None    # out4 of the last label_histograms

    def label_histograms(self, labels=None, nbins=None, lo=None, width=None):
        """``(fg_hist, bg_hist)``: per bin the voxels of the foreground and of the background of a segmentation, EVERY voxel in one
        of the two, int64 arrays of ``nbins`` entries, counted on the device (mgc_label_histograms) -- exactly
        ``numpy.bincount(bins[labels], minlength=nbins)`` and ``numpy.bincount(bins[~labels], minlength=nbins)`` with
        ``bins = histogram_bins(image, nbins, lo, width)``.  ``labels`` of None: the labels of the graph's current cut, read where
        they lie on the device (MedpyHipError ERR_STATE unless a converged ``maxflow()`` is current: not before the first solve, not
        between an update or edit and the next ``maxflow()``).  Otherwise a bool or uint8 array of the volume's shape, not zero =
        foreground; it goes up for this call only, and the call then works before the graph is built too.  Image and binning as in
        ``marker_histograms``.  Nothing on the graph changes.  ``label_histogram_info()`` has the totals of this call."""
        nbins, lo, width = self._binned_args("label_histograms", nbins, lo, width)
        plane = None
        if labels is not None:
            if not (isinstance(labels, numpy.ndarray) and labels.dtype in (numpy.bool_, numpy.uint8) and labels.shape == self._shape):
                raise ValueError("label_histograms: labels must be None or a bool / uint8 array of shape %s" % (self._shape,))
            plane = self._marker_bytes(labels)
        fg = numpy.zeros(nbins, dtype=numpy.int64)
        bg = numpy.zeros(nbins, dtype=numpy.int64)
        out4 = numpy.zeros(4, dtype=numpy.int64)
        self._call("mgc_label_histograms", None if plane is None else _lib.ptr(plane), nbins, lo, width, _lib.ptr(fg), _lib.ptr(bg), _lib.ptr(out4))
        self._label_hist_counts = out4
        return fg, bg

    def label_histogram_info(self):
        """of the last ``label_histograms``: voxels of the foreground, of the background, counts whose value lay below ``lo``
        (clamped into bin 0) and at or above ``lo + nbins * width`` (clamped into the last bin)"""
        out4 = self._label_hist_counts if self._label_hist_counts is not None else numpy.zeros(4, dtype=numpy.int64)
        return dict(zip(("fg_voxels", "bg_voxels", "below", "above"), out4.tolist()))

    def iterate_regional_histogram(self, max_refits=8, lam=None, eps=None, stop_below=0):
        """The iterated graph cut of GrabCut on the histogram regional term (``energy_voxel.regional_histogram``): fit the two
        histograms to the CURRENT CUT instead of the strokes (``label_histograms()``), turn them into the two tables
        (``histogram_tables``), expand those into the t-links (``update_tweights_binned``), solve warm -- and again, until the
        histograms stop moving or ``max_refits`` refits are done.  Needs a converged ``maxflow()`` to start from (MedpyHipError
        ERR_STATE otherwise).  The markers stay hard constraints throughout.

        ``moved`` of a round is the sum over the bins of ``|fg_hist - previous fg_hist|``: every voxel that changes side moves one
        count of one bin, so it is a lower bound on the voxels that changed side, and it is 0 exactly when the term is already fitted
        to the histograms of its own cut -- the fixed point (the bg histograms carry the same number: per bin fg + bg is the image's
        histogram).  The loop stops, ``converged`` True, at ``moved <= stop_below``; the first refit is always done.  ``lam`` /
        ``eps`` of None: those the graph was built with; the values used are remembered, as by ``refit_regional_histogram``.

        Returns a dict: ``rounds`` -- one dict per refit with ``fg_voxels``, ``bg_voxels`` (of the cut the refit was fitted to),
        ``moved`` (None in the first) and ``flow`` (of the solve behind it) --, ``converged``, and ``fg_hist`` / ``bg_hist`` of the
        final cut."""
        self._refuse_host_merged("iterate_regional_histogram")
        if self._binning is None or self._hist_params is None:
            raise ValueError("iterate_regional_histogram: the graph was built without a histogram term (energy_voxel.regional_histogram)")
        if isinstance(max_refits, bool) or not isinstance(max_refits, (int, numpy.integer)) or max_refits < 0:
            raise ValueError("iterate_regional_histogram: max_refits = %r: a whole number >= 0" % (max_refits,))
        if isinstance(stop_below, bool) or not isinstance(stop_below, (int, numpy.integer)) or stop_below < 0:
            raise ValueError("iterate_regional_histogram: stop_below = %r: a whole number >= 0" % (stop_below,))
        lam = self._hist_params[0] if lam is None else lam
        eps = self._hist_params[1] if eps is None else eps
        histogram_tables(numpy.zeros(1), numpy.zeros(1), lam, eps)   # (ValueError for lam / eps out of range before anything runs)
        rounds, converged, prev = [], False, None
        for r in range(int(max_refits) + 1):
            fg_hist, bg_hist = self.label_histograms()
            moved = None if prev is None else int(numpy.abs(fg_hist - prev).sum())
            if moved is not None and moved <= stop_below:
                converged = True
                break
            if r == max_refits:
                break
            source_table, sink_table = histogram_tables(fg_hist, bg_hist, lam, eps)
            self.update_tweights_binned(source_table, sink_table)
            self._hist_params = (lam, eps)
            flow = self.maxflow()
            rounds.append({"fg_voxels": int(fg_hist.sum()), "bg_voxels": int(bg_hist.sum()), "moved": moved, "flow": flow})
            prev = fg_hist
        return {"rounds": rounds, "converged": converged, "fg_hist": fg_hist, "bg_hist": bg_hist}

    def _add_nweights(self, offset, there, back=None):
        """mgc_add_nweights: ``there[p]`` is added to the arc p -> p + offset, ``back[p]`` (None: ``there[p]``) to the arc
        p + offset -> p; arrays of the volume's shape.  float32 / float64 go up as they are, anything else as float64."""
        def arr(a):
            a = numpy.asarray(a)
            if a.dtype not in (numpy.float32, numpy.float64):
                a = a.astype(numpy.float64)
            return numpy.ascontiguousarray(a)
        there = arr(there)
        self._check_volume_shape(there, "n-link weights")
        if back is not None:
            back = arr(back)
            self._check_volume_shape(back, "n-link weights (back)")
            if back.dtype != there.dtype:
                there, back = there.astype(numpy.float64), back.astype(numpy.float64)
        if len(tuple(offset)) != len(self._shape):
            raise ValueError("offset %r on a graph of %d axes" % (tuple(offset), len(self._shape)))
        off = (C.c_int * len(self._shape))(*[int(v) for v in offset])
        self._labels = None
        self._call("mgc_add_nweights", off, _lib.ptr(there), None if back is None else _lib.ptr(back), _lib.DTYPE_IDS[there.dtype])

    def _clear_nweights(self):
        """mgc_clear_nweights: forget the dense weight arrays (and free their store)"""
        self._labels = None
        self._call("mgc_clear_nweights")

    def last_note(self):
        """the library's note on the last call that went through (mgc_add_nweights: where its time went)"""
        return (_lib.load().mgc_last_error(self._h) or b"").decode("utf-8", "replace")

    def _build(self):
        self._call("mgc_build")
        self._labels = None

    def set_param(self, name, value):
        self._call("mgc_set_param", name.encode(), int(value))

    def validate(self):
        """invariants of the maximum preflow in HBM (mgc_validate): dict of violation counts (all zero for a correct
        solve), the two conservation errors, the flow into the sink and the capacity of the cut"""
        v = _lib.Validation()
        self._call("mgc_validate", C.byref(v))
        return v.as_dict()

    # -- GraphDouble surface
    def maxflow(self):
        """GraphDouble.maxflow(), reference maxflow.cpp:472-604."""
        flow = C.c_double(0.0)
        self._call("mgc_maxflow", C.byref(flow))
        return flow.value

    def labels(self, out=None):
        """All voxels at once: bool array of the marker shape, False where what_segment == SINK
        (the loop of bin/medpy_graphcut_voxel.py:177-182).

        ``out``: a writeable C-contiguous bool or uint8 array of the volume's shape that holds the labels of the previous cut
        (what ``changed_labels()`` refers to).  Only the ids of the changed voxels are read from the device and ``out`` is
        flipped there and returned; where the graph keeps no previous cut the whole volume is read into ``out``."""
        if out is not None:
            if not (isinstance(out, numpy.ndarray) and out.shape == self._shape and out.dtype in (numpy.bool_, numpy.uint8)
                    and out.flags.c_contiguous and out.flags.writeable):
                raise ValueError("labels(out=...): a writeable C-contiguous bool or uint8 array of shape %s" % (self._shape,))
            flat = out.reshape(-1).view(numpy.uint8)
            try:
                ids = self.changed_labels()
            except _lib.MedpyHipError as e:
                if e.code != _lib.ERR_STATE:
                    raise
                self._call("mgc_labels", _lib.ptr(flat))   # (not solved: ERR_STATE again, from here)
                return out
            flat[ids] ^= 1
            return out
        if self._labels is None:
            out = numpy.empty(self._nodes, dtype=numpy.uint8)
            self._call("mgc_labels", _lib.ptr(out))
            self._labels = out.view(numpy.bool_).reshape(self._shape)   # (the library writes 0 / 1: the bytes ARE the bool array, no second pass over the volume)
        return self._labels

    # -- the other minimum cuts
    CUT_SETS_INFO_KEYS = ("from_source", "to_sink", "ambiguous", "flood_passes", "tile_visits", "tiles_seeded", "tiles_skipped")

    @property
    def _labels(self):
        return self.__dict__.get("_labels_cache")

    @_labels.setter
    def _labels(self, value):
        # every build, update and edit drops the cached labels by assigning None: what mgc_cut_sets computed goes with them
        self.__dict__["_labels_cache"] = value
        if value is None:
            self.__dict__["_cut_sets_cache"] = {}

    def _cut_sets(self, want):
        """one mgc_cut_sets per solve and kind of answer: ``want`` = "source_side", "ambiguous" or "info" (no volume comes down)"""
        cache = self.__dict__.setdefault("_cut_sets_cache", {})
        if want not in cache:
            plane = None if want == "info" else numpy.empty(self._nodes, dtype=numpy.uint8)
            self._call("mgc_cut_sets", _lib.ptr(plane) if want == "source_side" else None, _lib.ptr(plane) if want == "ambiguous" else None)
            out = numpy.zeros(8, dtype=numpy.int64)
            cut = C.c_double(0.0)
            self._call("mgc_get_cut_sets_info", _lib.ptr(out), C.byref(cut))
            cache["info"] = dict(zip(self.CUT_SETS_INFO_KEYS, out.tolist()), source_cut=cut.value)
            if plane is not None:
                cache[want] = plane.view(numpy.bool_).reshape(self._shape)
        return cache[want]

    CUT_SETS_TOL_INFO_KEYS = ("from_source", "to_sink", "ambiguous", "forward_passes", "forward_visits", "forward_seeded", "backward_passes",
                              "backward_visits", "backward_seeded", "arcs_closed", "tlinks_closed", "tiles_skipped")

    def _cut_sets_tol(self, tol, want):
        """one mgc_cut_sets_tol per solve, tolerance and kind of answer: ``want`` = "source_side", "sink_side", "ambiguous" or "info" """
        tol = float(tol)
        cache = self.__dict__.setdefault("_cut_sets_cache", {}).setdefault(("tol", tol), {})
        if want not in cache:
            plane = None if want == "info" else numpy.empty(self._nodes, dtype=numpy.uint8)
            self._call("mgc_cut_sets_tol", tol, *[_lib.ptr(plane) if want == w else None for w in ("source_side", "sink_side", "ambiguous")])
            out, vals = numpy.zeros(16, dtype=numpy.int64), numpy.zeros(4, dtype=numpy.float64)
            self._call("mgc_get_cut_sets_tol_info", _lib.ptr(out), _lib.ptr(vals))
            cache["info"] = dict(zip(self.CUT_SETS_TOL_INFO_KEYS, out.tolist()), tol=float(vals[0]), source_cut=float(vals[1]), sink_cut=float(vals[2]),
                                 scale_max=float(vals[3]))
            if plane is not None:
                cache[want] = plane.view(numpy.bool_).reshape(self._shape)
        return cache[want]

    def source_side(self, tol=None):
        """bool array of the volume's shape, True on the voxels the SOURCE reaches in the residual graph of the maximum flow: the
        source side of the smallest minimum cut (``labels()`` is that of the largest).  After ``maxflow()``; MedpyHipError
        (ERR_STATE) before it and after an update or edit that has not been solved.  Cached until the next update or edit.
        ``tol``: None -- an arc is open iff its residual is > 0 (mgc_cut_sets); a number in [0, 1) -- iff it also exceeds ``tol``
        times the largest arc-pair capacity at either end (mgc_cut_sets_tol, e.g. ``ULP64``): the voxels whose side does not hinge
        on the rounding of the solve."""
        return self._cut_sets("source_side") if tol is None else self._cut_sets_tol(tol, "source_side")

    def sink_side(self, tol=None):
        """bool array, True on the voxels that reach the SINK in the residual graph: ``~labels()`` for ``tol=None`` (no call is made)
        and, by a backward flood of its own, for ``tol=0.0``; a part of it for a larger ``tol``."""
        return ~self.labels() if tol is None else self._cut_sets_tol(tol, "sink_side")

    def ambiguous(self, tol=None):
        """bool array, True on the voxels that are neither reachable from the source nor able to reach the sink: some minimum
        cut has them on the source side, another on the sink side -- where one more stroke would decide something.  With a ``tol``
        also the voxels whose side hinges on a residual below the rounding granularity."""
        return self._cut_sets("ambiguous") if tol is None else self._cut_sets_tol(tol, "ambiguous")

    def cut_sets_info(self, tol=None):
        """dict: voxels ``from_source`` / ``to_sink`` / ``ambiguous``, ``flood_passes``, ``tile_visits``, ``tiles_seeded``,
        ``tiles_skipped`` of the flood, and ``source_cut``, the capacity of the cut around ``source_side()`` (= ``maxflow()``).
        With a ``tol``: the three counts, passes / visits / seeded tiles of the forward and of the backward flood, ``arcs_closed`` and
        ``tlinks_closed`` by the threshold, ``tiles_skipped``, ``tol``, ``source_cut``, ``sink_cut`` (around ``~sink_side(tol)``) and
        ``scale_max``, the largest arc-pair capacity."""
        return dict(self._cut_sets("info") if tol is None else self._cut_sets_tol(tol, "info"))

    def cut_is_unique(self, tol=None):
        """is the minimum cut unique, i.e. the ambiguity set empty?  Counted on the device, no volume is read back."""
        return (self._cut_sets("info") if tol is None else self._cut_sets_tol(tol, "info"))["ambiguous"] == 0

    def cut_sets(self, tol=None):
        """``CutSets(from_source, to_sink, ambiguous, info)``: ``source_side(tol)``, ``sink_side(tol)``, ``ambiguous(tol)`` and
        ``cut_sets_info(tol)`` under the one name every graph kind has (``SparseGraph.cut_sets``); arrays in the volume's shape."""
        return CutSets(self.source_side(tol), self.sink_side(tol), self.ambiguous(tol), self.cut_sets_info(tol))

    def cut_sets_unique(self, tol=None):
        """``cut_is_unique(tol)`` under the name every graph kind has"""
        return self.cut_is_unique(tol)

    # -- connected components of the cut, and the cut cleaned by them
    COMPONENTS_INFO_KEYS = ("components", "voxels", "largest_size", "largest_id", "tiles_skipped", "tiles_processed", "unions", "longest_walk")
    CLEAN_INFO_KEYS = ("fg_components", "survivors", "voxels_removed", "cavities_filled", "voxels_filled", "voxels_changed", "list_written")
    COMPONENTS_TABLE = 65536       # rows the first call of ``components()`` asks for
    CLEAN_LIST = 1 << 20           # ids ``clean_labels(changed_only=True)`` reads back before it falls back to the volume
    _clean_info = None             # out8 of the last clean_labels

    def _cc_plane(self, what, labels):
        if labels is None:
            return None
        if not (isinstance(labels, numpy.ndarray) and labels.dtype in (numpy.bool_, numpy.uint8) and labels.shape == self._shape):
            raise ValueError("%s: labels must be None or a bool / uint8 array of shape %s" % (what, self._shape))
        return self._marker_bytes(labels)

    def _cc_full(self, what, name, connectivity, default):
        if connectivity is None:
            return int(default)
        if isinstance(connectivity, str) and connectivity in ("face", "full"):
            return int(connectivity == "full")
        raise ValueError("%s: %s must be None, \"face\" or \"full\", got %r" % (what, name, connectivity))

    def components(self, labels=None, foreground=True, connectivity=None, ids=True):
        """``Components(ids, first, size, flags, info)``: the connected components of the foreground (``foreground=False``: of the
        background) of a segmentation, labelled on the device (mgc_components).  ``labels`` of None: the graph's current cut, read
        where it lies on the device (MedpyHipError ERR_STATE unless a converged ``maxflow()`` is current); otherwise a bool or uint8
        array of the volume's shape, not zero = foreground, which goes up for this call only -- the call then works before the graph
        is built too.  ``connectivity``: ``"face"`` (2 / 4 / 6 neighbours), ``"full"`` (2 / 8 / 26) or None, the graph's own.

        The components are numbered 1..K in ascending order of their first voxel, the numbering of ``scipy.ndimage.label``.
        ``ids``: int32 array of the volume's shape, 0 on the other side -- or None with ``ids=False``, when no volume comes down.
        ``first`` / ``size`` (int64) and ``flags`` (uint8) have K entries: first voxel id, voxel count, and bits 1 = holds a
        foreground marker of the graph, 2 = holds a background marker, 4 = touches the border of the volume.  ``info``: K, the voxels
        of that side, size and id of the largest component, and counts of the device's work.  Not cached; nothing on the graph changes."""
        plane = self._cc_plane("components", labels)
        full = self._cc_full("components", "connectivity", connectivity, self._full_neighbourhood)
        vol = numpy.empty(self._nodes, dtype=numpy.int32) if ids else None
        cap = self.COMPONENTS_TABLE
        while True:
            first, size = numpy.zeros(cap, dtype=numpy.int64), numpy.zeros(cap, dtype=numpy.int64)
            flags = numpy.zeros(cap, dtype=numpy.uint8)
            out8 = numpy.zeros(8, dtype=numpy.int64)
            self._call("mgc_components", None if plane is None else _lib.ptr(plane), int(bool(foreground)), full, None if vol is None else _lib.ptr(vol), cap,
                       _lib.ptr(first), _lib.ptr(size), _lib.ptr(flags), _lib.ptr(out8))
            k = int(out8[0])
            if k <= cap:
                break
            cap = k   # the table held the first rows only: once more, with room for all
        return Components(None if vol is None else vol.reshape(self._shape), first[:k], size[:k], flags[:k], dict(zip(self.COMPONENTS_INFO_KEYS, out8.tolist())))

    def clean_labels(self, labels=None, min_size=1, largest=None, seeded=False, fill_holes=False, connectivity=None, hole_connectivity=None, out=None,
                     changed_only=False):
        """The segmentation cleaned by components, on the device (mgc_clean_labels), in two steps.  1: of the foreground components
        at ``connectivity`` (None: the graph's own) those pass that hold at least ``min_size`` voxels and, with ``seeded``, a
        foreground marker of the graph; with ``largest=n`` only the n biggest of them survive, ties on size going to the one whose
        first voxel comes first.  2, with ``fill_holes``: the background components of the result at ``hole_connectivity`` (None:
        ``"face"``) that neither touch the border of the volume nor hold a background marker become foreground -- a background
        marker inside a cavity keeps it open.  ``labels`` as in ``components()``.

        Returns the cleaned bool volume (written into ``out``, a writeable C-contiguous bool array of the volume's shape, when
        given).  ``changed_only=True``: the ascending int64 ids of the voxels the rule changed instead, and no volume comes down
        unless there are more than ``CLEAN_LIST`` of them.  ``clean_info()`` has the counts.  Nothing on the graph changes."""
        plane = self._cc_plane("clean_labels", labels)
        default_full = self._full_neighbourhood
        rule = _lib.CleanRule(self._cc_full("clean_labels", "connectivity", connectivity, default_full), int(bool(seeded)), int(bool(fill_holes)),
                              self._cc_full("clean_labels", "hole_connectivity", hole_connectivity, False), 1, 0)
        for name, v, lo in (("min_size", min_size, 1), ("largest", 1 if largest is None else largest, 1)):
            if isinstance(v, (bool, numpy.bool_)) or not isinstance(v, (int, numpy.integer)) or v < lo:
                raise ValueError("clean_labels: %s must be an integer >= %d, got %r" % (name, lo, v))
        rule.min_size, rule.largest = int(min_size), 0 if largest is None else int(largest)
        if out is not None and not (isinstance(out, numpy.ndarray) and out.shape == self._shape and out.dtype == numpy.bool_ and out.flags.c_contiguous
                                    and out.flags.writeable):
            raise ValueError("clean_labels(out=...): a writeable C-contiguous bool array of shape %s" % (self._shape,))
        out8 = numpy.zeros(8, dtype=numpy.int64)
        src = None if plane is None else _lib.ptr(plane)
        if changed_only:
            cap = int(self.CLEAN_LIST)
            ids = numpy.zeros(max(cap, 1), dtype=numpy.int64)
            self._call("mgc_clean_labels", src, C.byref(rule), None, cap, _lib.ptr(ids), _lib.ptr(out8))
            self._clean_info = out8
            if out8[6]:
                return ids[:int(out8[5])].copy()
            # more changes than the list holds (rare: the list takes a million ids): the cleaned volume comes down after all, next to
            # the plane it was cleaned from, and the ids are computed here.  The cut's labels are read into an array of this call:
            # nothing the graph caches is touched.
            vol = numpy.empty(self._nodes, dtype=numpy.uint8)
            self._call("mgc_clean_labels", src, C.byref(rule), _lib.ptr(vol), 0, None, _lib.ptr(out8))
            self._clean_info = out8
            before = plane.reshape(-1) if plane is not None else numpy.empty(self._nodes, dtype=numpy.uint8)
            if plane is None:
                self._call("mgc_labels", _lib.ptr(before))
            return numpy.flatnonzero((vol != 0) != (before != 0)).astype(numpy.int64)
        vol = numpy.empty(self._nodes, dtype=numpy.uint8) if out is None else out.reshape(-1).view(numpy.uint8)
        self._call("mgc_clean_labels", src, C.byref(rule), _lib.ptr(vol), 0, None, _lib.ptr(out8))
        self._clean_info = out8
        return vol.view(numpy.bool_).reshape(self._shape) if out is None else out

    def clean_info(self):
        """of the last ``clean_labels``: ``fg_components``, ``survivors``, ``voxels_removed`` (step 1), ``cavities_filled``,
        ``voxels_filled`` (step 2), ``voxels_changed``, and ``list_written``: 1 when the device wrote the list of changed ids"""
        out8 = self._clean_info if self._clean_info is not None else numpy.zeros(8, dtype=numpy.int64)
        return dict(zip(self.CLEAN_INFO_KEYS, out8.tolist()))

    # -- the Euclidean distance transform of a segmentation and its overlap and surface measures against another
    SURFACE_LIST = 1 << 20         # distances the first call of ``surface_distances()`` asks for
    _edt_info = None               # out4 of the last distance_transform

    def _edt_plane(self, what, name, plane):
        if not (isinstance(plane, numpy.ndarray) and plane.dtype in (numpy.bool_, numpy.uint8) and plane.shape == self._shape):
            raise ValueError("%s: %s must be a bool / uint8 array of shape %s" % (what, name, self._shape))
        return self._marker_bytes(plane)

    def _edt_spacing(self, what, spacing):
        if spacing is None:
            return None
        sp = numpy.asarray(spacing, dtype=numpy.float64)
        if sp.ndim == 0:
            sp = numpy.full(len(self._shape), float(sp))
        if sp.shape != (len(self._shape),):
            raise ValueError("%s: the spacing must be a scalar or %d values, got %r" % (what, len(self._shape), spacing))
        if not (numpy.isfinite(sp).all() and (sp > 0).all()):
            raise ValueError("%s: the spacing must be finite and positive, got %r" % (what, spacing))
        return numpy.ascontiguousarray(sp)

    def distance_transform(self, labels=None, to="foreground", spacing=None, squared=False):
        """float64 array of the volume's shape: the exact Euclidean distance of every voxel to the nearest foreground voxel of a
        segmentation (``to="background"``: to the nearest background voxel -- scipy.ndimage.distance_transform_edt of the
        segmentation), computed on the device (mgc_distance_transform).  ``labels`` as in ``components()``; ``spacing``: None, a
        scalar or one value per axis.  ``squared=True`` returns what the device computes: the minimum over the seeds of
        ``(sx * dx) ** 2 + (sy * dy) ** 2 + (sz * dz) ** 2`` in float64, the last axis first, every operation rounded on its own --
        exact integers at unit spacing; the root is NumPy's.  +inf everywhere when there is no such voxel.  ``edt_info()`` has the
        counts.  Nothing on the graph changes."""
        plane = None if labels is None else self._edt_plane("distance_transform", "labels", labels)
        if to not in ("foreground", "background"):
            raise ValueError("distance_transform: to must be \"foreground\" or \"background\", got %r" % (to,))
        sp = self._edt_spacing("distance_transform", spacing)
        out = numpy.empty(self._nodes, dtype=numpy.float64)
        out4 = numpy.zeros(4, dtype=numpy.int64)
        self._call("mgc_distance_transform", None if plane is None else _lib.ptr(plane), int(to == "foreground"), None if sp is None else _lib.ptr(sp), _lib.ptr(out),
                   _lib.ptr(out4))
        self._edt_info = out4
        out = out.reshape(self._shape)
        return out if squared else numpy.sqrt(out, out=out)

    def edt_info(self):
        """of the last ``distance_transform``: ``seeds``, and ``long_lines``, the lines that were too long for on-chip memory"""
        out4 = self._edt_info if self._edt_info is not None else numpy.zeros(4, dtype=numpy.int64)
        return {"seeds": int(out4[0]), "long_lines": int(out4[1])}

    # -- the geodesic distance transform and the regional term on top of it
    GEODESIC_INFO_KEYS = ("seeds", "rounds", "tile_visits", "sweeps", "capped_visits", "finite")
    _geo_info = None               # out8 of the last geodesic_distance
    _geo_params = None             # (gamma, lam, step, spacing, connectivity) of the geodesic term the graph was built with

    def _geo_full(self, what, connectivity):
        nd = len(self._shape)
        if connectivity is None:
            return int(self._full_neighbourhood)
        if connectivity not in (1, nd):
            raise ValueError("%s: connectivity must be 1 (face neighbours) or %d (the full neighbourhood), got %r" % (what, nd, connectivity))
        return int(connectivity == nd and nd > 1)   # (on one axis the two neighbourhoods are the same)

    @staticmethod
    def _geo_number(what, name, v):
        v = float(v)
        if not (numpy.isfinite(v) and v >= 0):
            raise ValueError("%s: %s must be finite and not negative, got %r" % (what, name, v))
        return v

    def geodesic_distance(self, seeds="fg", gamma=1.0, step=1.0, spacing=None, connectivity=None):
        """float64 array of the volume's shape: the geodesic distance of every voxel to the nearest seed, computed on the device
        (mgc_geodesic_distance).  The length of the arc between neighbours p and q at offset d is
        ``step * sqrt(sum((spacing * d) ** 2)) + gamma * abs(I[p] - I[q])`` in float64, every operation rounded on its own, I the
        feature image of the graph, else its boundary image (``gamma=0``: the chamfer distance, no image needed); the distance is
        the smallest sum over the lattice paths from a seed, added from the seed outwards -- bit for bit what Dijkstra's
        algorithm in float64 gives (tests/geodesic_cases.py states it).  0 on seeds, +inf where no seed connects.  ``seeds``:
        ``"fg"`` / ``"bg"``, the markers of the graph where they lie on the device, or a bool / uint8 array of the volume's shape.
        ``connectivity``: 1 (face neighbours) or the number of axes (the full neighbourhood); None: the graph's own.
        ``spacing``: None, a scalar or one value per axis.  ``geodesic_info()`` has the counts.  Nothing on the graph changes."""
        full = self._geo_full("geodesic_distance", connectivity)
        gamma = self._geo_number("geodesic_distance", "gamma", gamma)
        step = self._geo_number("geodesic_distance", "step", step)
        sp = self._edt_spacing("geodesic_distance", spacing)
        if isinstance(seeds, str):
            if seeds not in ("fg", "bg"):
                raise ValueError("geodesic_distance: seeds must be \"fg\", \"bg\" or an array, got %r" % (seeds,))
            plane, source = None, 1 if seeds == "fg" else 2
        else:
            plane, source = self._edt_plane("geodesic_distance", "seeds", seeds), 0
        out = numpy.empty(self._nodes, dtype=numpy.float64)
        out8 = numpy.zeros(8, dtype=numpy.int64)
        self._call("mgc_geodesic_distance", None if plane is None else _lib.ptr(plane), source, full, gamma, step, None if sp is None else _lib.ptr(sp), _lib.ptr(out),
                   _lib.ptr(out8))
        self._geo_info = out8
        return out.reshape(self._shape)

    def geodesic_info(self):
        """of the last ``geodesic_distance``: ``seeds``, ``rounds`` (launches over the active tiles), ``tile_visits``, ``sweeps``
        (summed over the visits), ``capped_visits`` (visits that ended at the sweep cap and woke their own tile) and ``finite``,
        the voxels a seed reaches"""
        out8 = self._geo_info if self._geo_info is not None else numpy.zeros(8, dtype=numpy.int64)
        return dict(zip(self.GEODESIC_INFO_KEYS, out8.tolist()))

    # -- anisotropic diffusion of the image the graph holds
    _diffusion_info = None         # out4 of the last anisotropic_diffusion

    def anisotropic_diffusion(self, niter, kappa, gamma, voxelspacing=None, option=1, keep=False, download=True):
        """Anisotropic diffusion (``medpy_amd.filter.anisotropic_diffusion`` has the definition) of the image the graph holds -- its
        feature image, else the image of its boundary term -- where it lies on the device (mgc_diffuse).  Returns the float32 array
        of the volume's shape, or None with ``download=False`` (which needs ``keep=True``).  ``keep=True``: the result becomes
        the graph's feature image, as ``set_feature_image`` of it would, without crossing the bus: ``marker_histograms()``,
        ``label_histograms()``, the histogram and the geodesic terms read the smoothed image from then on.  ``keep=False``: nothing
        on the graph changes.  ``diffusion_info()`` has the counts."""
        from ..filter.smoothing import check_arguments
        n, kappa, gamma, sp, option = check_arguments("anisotropic_diffusion", len(self._shape), niter, kappa, gamma, voxelspacing, option)
        if not keep and not download:
            raise ValueError("anisotropic_diffusion: download=False needs keep=True (the result would be lost)")
        out = numpy.empty(self._shape, dtype=numpy.float32) if download else None
        out4 = numpy.zeros(4, dtype=numpy.int64)
        self._call("mgc_diffuse", n, kappa, gamma, None if sp is None else _lib.ptr(sp), option, int(bool(keep)), None if out is None else _lib.ptr(out), _lib.ptr(out4))
        self._diffusion_info = out4
        return out

    def diffusion_info(self):
        """of the last ``anisotropic_diffusion``: ``iterations`` run and ``bricks`` per launch"""
        out4 = self._diffusion_info if self._diffusion_info is not None else numpy.zeros(4, dtype=numpy.int64)
        return {"iterations": int(out4[0]), "bricks": int(out4[1])}

    def _geo_term_args(self, what, gamma, lam, step, spacing, connectivity):
        return (self._geo_number(what, "gamma", gamma), self._geo_number(what, "lam", lam), self._geo_number(what, "step", step),
                self._edt_spacing(what, spacing), self._geo_full(what, connectivity))

    def _add_tweights_geodesic(self, gamma, lam, step=1.0, spacing=None, connectivity=None):
        """mgc_add_tweights_geodesic: one ``add_tweights(S[p], K[p])`` per voxel on the graph's explicit t-links, S and K the
        geodesic term of the markers the graph holds -- what ``_add_tweights(*expected_term(D_F, D_B, lam))`` leaves, without
        the arrays crossing the bus"""
        gamma, lam, step, sp, full = self._geo_term_args("_add_tweights_geodesic", gamma, lam, step, spacing, connectivity)
        self._labels = None
        self._call("mgc_add_tweights_geodesic", full, gamma, step, None if sp is None else _lib.ptr(sp), lam)

    def update_tweights_geodesic(self, gamma, lam, step=1.0, spacing=None, connectivity=None):
        """Replace the explicit t-links by the geodesic term of the markers as they stand now -- what ``update_tweights_dense`` of
        the term's two arrays leaves, bit for bit, with both transforms and the expansion on the device
        (mgc_update_tweights_geodesic) -- and keep the residual graph: the next ``maxflow()`` is a warm solve.  Unlike
        ``update_tweights_dense`` the call keeps the labels of the cut before it (or before the marker edit it follows) on the
        device, so ``changed_labels()`` and ``labels(out=previous)`` work after that solve."""
        self._refuse_host_merged("update_tweights_geodesic")
        gamma, lam, step, sp, full = self._geo_term_args("update_tweights_geodesic", gamma, lam, step, spacing, connectivity)
        self._labels = None
        self._call("mgc_update_tweights_geodesic", full, gamma, step, None if sp is None else _lib.ptr(sp), lam)

    def refit_regional_geodesic(self, gamma=None, lam=None):
        """Fit the geodesic regional term (``energy_voxel.regional_geodesic``) to the markers as they stand now, after
        ``update_markers`` / ``edit_markers``: both transforms run again on the device and the term replaces the explicit t-links.
        ``gamma`` / ``lam`` of None: those the graph was built with; step, spacing and connectivity stay.  The next ``maxflow()``
        is a warm solve with the labels and the flow of a graph built from the markers and the refitted term;
        ``labels(out=previous)`` brings a copy of the previous labels up to date."""
        self._refuse_host_merged("refit_regional_geodesic")
        if self._geo_params is None:
            raise ValueError("refit_regional_geodesic: the graph was built without a geodesic term (energy_voxel.regional_geodesic)")
        g0, l0, step, spacing, connectivity = self._geo_params
        gamma = g0 if gamma is None else gamma
        lam = l0 if lam is None else lam
        self.update_tweights_geodesic(gamma, lam, step, spacing, connectivity)
        self._geo_params = (float(gamma), float(lam), step, spacing, connectivity)

    def surface_distances(self, reference, labels=None, voxelspacing=None, connectivity=1):
        """float64 list: the distance from every border voxel of the segmentation to the nearest border voxel of ``reference``, in
        ascending voxel id -- ``dt[result_border]`` of the reference's surface measures, from which ``hd``, ``asd`` and their kin
        follow (medpy_amd.metric.binary).  Borders, transform and gathering run on the device (mgc_surface_distances); the root is
        NumPy's.  ``connectivity``: 1 .. ndim, as in scipy.ndimage.generate_binary_structure.  RuntimeError when either object is
        empty.  Nothing on the graph changes."""
        ref = self._edt_plane("surface_distances", "reference", reference)
        plane = None if labels is None else self._edt_plane("surface_distances", "labels", labels)
        if isinstance(connectivity, (bool, numpy.bool_)) or not isinstance(connectivity, (int, numpy.integer)) or not 1 <= connectivity <= len(self._shape):
            raise ValueError("surface_distances: connectivity must be an integer 1 .. %d, got %r" % (len(self._shape), connectivity))
        sp = self._edt_spacing("surface_distances", voxelspacing)
        cap = int(self.SURFACE_LIST)
        while True:
            sds = numpy.empty(max(cap, 1), dtype=numpy.float64)
            out8 = numpy.zeros(8, dtype=numpy.int64)
            self._call("mgc_surface_distances", None if plane is None else _lib.ptr(plane), _lib.ptr(ref), int(connectivity), None if sp is None else _lib.ptr(sp), cap,
                       _lib.ptr(sds), _lib.ptr(out8))
            if out8[2] == 0:
                raise RuntimeError("The first supplied array does not contain any binary object.")
            if out8[3] == 0:
                raise RuntimeError("The second supplied array does not contain any binary object.")
            n = int(out8[0])
            if n <= cap:
                break
            cap = n   # the list held the first entries only: once more, with room for all
        sds = sds[:n]
        return numpy.sqrt(sds, out=sds)

    def overlap_counts(self, reference, labels=None):
        """``(tp, fp, fn, tn)``: the voxels of the segmentation and of ``reference``, of the segmentation only, of ``reference``
        only, of neither -- counted on the device (mgc_overlap_counts).  Nothing on the graph changes."""
        ref = self._edt_plane("overlap_counts", "reference", reference)
        plane = None if labels is None else self._edt_plane("overlap_counts", "labels", labels)
        out4 = numpy.zeros(4, dtype=numpy.int64)
        self._call("mgc_overlap_counts", None if plane is None else _lib.ptr(plane), _lib.ptr(ref), _lib.ptr(out4))
        return tuple(int(v) for v in out4)

    def what_segment(self, i):
        """Graph::what_segment, reference graph.h:561-571."""
        seg = C.c_int(0)
        self._call("mgc_what_segment", int(i), C.byref(seg))
        return termtype(seg.value)

    def get_edge(self, i, j):
        out = C.c_double(0.0)
        self._call("mgc_get_edge", int(i), int(j), C.byref(out))
        return out.value

    def get_node_num(self):
        return self._nodes

    def get_trcap(self, i):
        return float(self.tweights().ravel()[int(i)])

    # -- energy read-back (parity tests)
    def nweights_offset(self, offset):
        """weights of the arcs (p, p + offset), NaN where p + offset is outside the volume"""
        off = (C.c_int * len(self._shape))(*[int(v) for v in offset])
        out = numpy.empty(self._shape, dtype=numpy.float64)
        self._call("mgc_get_nweights_offset", off, _lib.ptr(out))
        return out

    def nweights(self, axis):
        shp = list(self._shape)
        shp[axis] -= 1
        out = numpy.empty(shp, dtype=numpy.float64)
        if out.size:
            self._call("mgc_get_nweights", int(axis), _lib.ptr(out))
        return out

    def tweights(self):
        out = numpy.empty(self._shape, dtype=numpy.float64)
        self._call("mgc_get_tweights", _lib.ptr(out))
        return out

    def profile(self):
        out = numpy.zeros(16, dtype=numpy.uint64)
        self._call("mgc_get_profile", _lib.ptr(out))
        names = ("load", "labels", "sweep", "store", "votes", "faceflags", "s6", "s7")
        return {n: {"cycles": int(out[i]), "count": int(out[i + 8])} for i, n in enumerate(names)}

    def stats(self):
        st = _lib.Stats()
        self._call("mgc_get_stats", C.byref(st))
        return st.as_dict()

    def first_relabel(self, radial=False, c_min=8):
        """Run the first global relabel of a solve -- the distance transform towards the sink, with ``radial`` also the radial
        labels of the flood phase (nothing below ``c_min`` hops from source to sink) -- and nothing else (MGC_OP_FIRST_RELABEL).
        On a graph as built; MedpyHipError (ERR_STATE) where the transform does not apply.  ``heights()`` reads the result."""
        self._call("mgc_solver_op", _lib.OP_FIRST_RELABEL, 1 if radial else 0, int(c_min), 0, 0)

    def heights(self, aside=False):
        """the distance labels, int32 array of the volume's shape (_lib.HINF: cannot reach the sink); ``aside``: the array kept
        aside while radial labels are in use, i.e. the exact labels (mgc_get_heights)"""
        out = numpy.empty(self._shape, dtype=numpy.int32)
        self._call("mgc_get_heights", 1 if aside else 0, _lib.ptr(out))
        return out

    def launch_counts(self):
        """{kernel form: launches} of the last solve (mgc_get_launch_counts; names: _lib.LAUNCH_KINDS)"""
        out = numpy.zeros(len(_lib.LAUNCH_KINDS), dtype=numpy.int64)
        self._call("mgc_get_launch_counts", _lib.ptr(out), int(out.size))
        return dict(zip(_lib.LAUNCH_KINDS, out.tolist()))


class SparseGraph(object):
    """``maxflow.GraphDouble`` (reference lib/maxflow/src/wrapper.cpp:59-89) for ARBITRARY graphs, solved in HBM by the
    library's sparse-graph solver (C ABI ``msg_*``).  Returned by ``graph_from_labels``, by ``graph_from_voxels`` for
    images of more than three dimensions and by ``GCGraph.get_graph()`` for graphs that plug-in terms assemble edge by
    edge.  Besides the facade hooks (``_add_*``) it takes the raw GraphDouble calls ``add_node``, ``add_edge``,
    ``sum_edge``, ``add_tweights``, ``get_edge`` and ``reset`` with the reference's semantics (graph.h:428-498,
    graph.cpp:46-60): ``add_edge`` creates a PARALLEL arc pair per call (the flow sees the summed capacity; ``get_edge``
    reports the arc the reference's list walk meets first, i.e. the pair added last), ``sum_edge`` adds to that arc.
    Edges are buffered and uploaded in batches.

    ``_cast`` is the capacity type of the instance (``GraphDouble``: float64; the subclasses ``GraphFloat`` / ``GraphInt``
    quantise every capacity, every running sum and the returned flow to float32 / int, instances.inc:12-15)."""

    termtype = termtype
    _captype = "double"

    @staticmethod
    def _cast(v):
        """a capacity handed in by the caller, in the graph's capacity type"""
        return float(v)

    @classmethod
    def _out(cls, v):
        """a value read back from the device, in the graph's capacity type"""
        return cls._cast(v)

    def __init__(self, nodes, edges=0, device=0):
        lib = _lib.load()
        if _lib.device_count() < 1:
            raise _lib.MedpyHipError(_lib.ERR_NO_DEVICE, "no HIP device visible; medpy_amd has no CPU fallback")
        self._nodes = max(int(nodes), 1)
        self._device = int(device)
        self._h = None
        self._raw = False   # driven through the raw GraphDouble calls (add_node / add_edge / sum_edge / reset) rather than the facade hooks
        self._open()

    def _open(self):
        """a fresh, empty solver graph in HBM (``__init__`` and ``reset``)"""
        lib = _lib.load()
        self.close()
        h = C.c_void_p()
        rc = lib.msg_create(self._nodes, self._device, C.byref(h))
        self._h = h if h.value else None
        if rc != _lib.OK:
            msg = (lib.msg_last_error(self._h) or b"").decode()
            self.close()
            raise _lib.MedpyHipError(rc, msg)
        self._labels = None
        self._pending = ([], [], [], [])
        self._tr = None
        self._flow_const = self._cast(0)
        self._declared = 0
        self._first_arc = {}   # (i, j) -> capacity of the arc get_arc(i, j) meets first (raw add_edge / sum_edge calls only)
        self._raw_pairs = set()
        self._host_arcs = {}   # GraphFloat / GraphInt: (i, j) -> [capacity of the front arc, sum of the parallel arcs behind it]
        self._host_sent = {}   # ... (i, j) with i < j -> (capacity, reverse capacity) the device holds for the pair so far
        self._sent_tr = None   # the merged t-links (and flow constant) the device was last told: maxflow() sends what differs
        self._sent_flow_const = None
        self._dev_solved = False   # the device holds a finished solve of the edges sent so far: the next solve may be warm
        self._dev_updated = False   # ... and was sent t-link updates since

    def update_markers(self, fg_markers, bg_markers):
        """Warm updates exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: update_markers is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: build it again from the new inputs")

    def update_regional_term(self, probability_map, alpha):
        """Warm updates exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: update_regional_term is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: build it again from the new inputs")

    def update_boundary_term(self, boundary_term, boundary_term_args):
        """Warm updates exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: update_boundary_term is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: build it again from the new inputs")

    def edit_markers(self, fg=None, bg=None, erase=None):
        """Edits by list exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: edit_markers is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: build it again from the new inputs")

    def edit_nweights(self, nodes_from, nodes_to, weight_there, weight_back=None):
        """Edits by list exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: edit_nweights is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: build it again from the new inputs")

    def update_tweights_dense(self, weights_source, weights_sink):
        """Whole t-link arrays exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only; here: ``update_tweights``."""
        raise NotImplementedError("medpy_amd: update_tweights_dense is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: update_tweights(nodes, tr)")

    def edit_tweights(self, nodes, weights_source, weights_sink):
        """Edits by list exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only; here: ``update_tweights``."""
        raise NotImplementedError("medpy_amd: edit_tweights is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: update_tweights(nodes, tr)")

    def clear_nweight_edits(self):
        """Edits by list exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: clear_nweight_edits is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: build it again from the new inputs")

    def nweight_edit_info(self):
        """Edits by list exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: nweight_edit_info is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver")

    def _no_cut_sets(self, what):
        raise NotImplementedError("medpy_amd: %s is implemented for the voxel lattice solver (1-D..3-D volumes, VoxelGraph) only; this "
                                  "graph went to the sparse-graph solver, which keeps its residual graph as CSR arcs: the forward "
                                  "flood over tile masks does not apply (labels() is the sink side's complement); use cut_sets() / cut_sets_unique(), "
                                  "which every graph kind has" % what)

    def source_side(self, tol=None):
        """The source side of the smallest minimum cut exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_cut_sets("source_side")

    def sink_side(self, tol=None):
        """The thresholded sink side exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_cut_sets("sink_side")

    def ambiguous(self, tol=None):
        """The ambiguity set exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_cut_sets("ambiguous")

    def cut_is_unique(self, tol=None):
        """The ambiguity set exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_cut_sets("cut_is_unique")

    def cut_sets_info(self, tol=None):
        """The ambiguity set exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_cut_sets("cut_sets_info")

    def _no_components(self, what):
        raise NotImplementedError("medpy_amd: %s is implemented for the voxel lattice solver (1-D..3-D volumes, VoxelGraph) only: the "
                                  "components are those of a label plane on the voxel lattice, and this graph went to the sparse-graph solver" % what)

    def components(self, labels=None, foreground=True, connectivity=None, ids=True):
        """Connected components exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_components("components")

    def clean_labels(self, labels=None, min_size=1, largest=None, seeded=False, fill_holes=False, connectivity=None, hole_connectivity=None, out=None,
                     changed_only=False):
        """Cleaning by components exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_components("clean_labels")

    def clean_info(self):
        """Cleaning by components exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_components("clean_info")

    def _no_metrics(self, what):
        raise NotImplementedError("medpy_amd: %s is implemented for the voxel lattice solver (1-D..3-D volumes, VoxelGraph) only: distances "
                                  "are those between the voxels of a lattice, and this graph went to the sparse-graph solver" % what)

    def distance_transform(self, labels=None, to="foreground", spacing=None, squared=False):
        """The distance transform exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_metrics("distance_transform")

    def surface_distances(self, reference, labels=None, voxelspacing=None, connectivity=1):
        """Surface distances exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_metrics("surface_distances")

    def overlap_counts(self, reference, labels=None):
        """Overlap counts exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_metrics("overlap_counts")

    def geodesic_distance(self, seeds="fg", gamma=1.0, step=1.0, spacing=None, connectivity=None):
        """The geodesic distance transform exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_metrics("geodesic_distance")

    def geodesic_info(self):
        """The geodesic distance transform exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_metrics("geodesic_info")

    def refit_regional_geodesic(self, gamma=None, lam=None):
        """The geodesic regional term exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_metrics("refit_regional_geodesic")

    def anisotropic_diffusion(self, niter=1, kappa=50, gamma=0.1, voxelspacing=None, option=1, keep=False, download=True):
        """The diffusion of the graph's image exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_metrics("anisotropic_diffusion")

    def diffusion_info(self):
        """The diffusion of the graph's image exists for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        self._no_metrics("diffusion_info")

    # -- the other minimum cuts
    CUT_SETS_INFO_KEYS = ("from_source", "to_sink", "ambiguous", "forward_passes", "forward_seeds", "backward_passes", "backward_seeds",
                          "arcs_closed", "tlinks_closed", "tol_path")

    @property
    def _labels(self):
        return self.__dict__.get("_labels_cache")

    @_labels.setter
    def _labels(self, value):
        # every edge, t-link and solve drops the cached labels by assigning None: what cut_sets() computed goes with them
        self.__dict__["_labels_cache"] = value
        if value is None:
            self.__dict__["_cut_sets_cache"] = {}

    def _host_arcs_unsent(self):
        """GraphFloat / GraphInt: does a node pair carry capacities the device has not been told (what ``_send_host_arcs`` would send)"""
        for k, a in self.__dict__.get("_host_arcs", {}).items():
            if k[0] < k[1]:
                b = self._host_arcs[(k[1], k[0])]
                if (float(a[0]) + float(a[1]), float(b[0]) + float(b[1])) != self._host_sent.get(k, (0.0, 0.0)):
                    return True
        return False

    def _refuse_unsolved_edits(self, what):
        """the sets are those of the cut ``maxflow()`` last returned: nothing is flushed from here"""
        d = self.__dict__
        tr, sent = d.get("_tr"), d.get("_sent_tr")
        if d.get("_pending", ([],))[0]:
            held = "edges added since the last maxflow()"
        elif self._host_arcs_unsent():
            held = "arcs added since the last maxflow()"
        elif tr is not None and (sent is None or sent.shape != tr.shape or not numpy.array_equal(sent, tr)):
            held = "t-links changed since the last maxflow()"
        elif d.get("_dev_updated"):
            held = "t-link updates the device has not solved"
        else:
            return
        raise _lib.MedpyHipError(_lib.ERR_STATE, "%s: the graph holds %s; call maxflow() first" % (what, held))

    def _cut_sets_call(self, tol, planes):
        """ONE msg_cut_sets / msg_cut_sets_tol and its info; ``planes``: three uint8 arrays or Nones (from_source, to_sink, ambiguous)"""
        p = [None if a is None else _lib.ptr(a) for a in planes]
        if tol is None:
            self._call("msg_cut_sets", p[0], p[2])
        else:
            self._call("msg_cut_sets_tol", tol, *p)
        out, vals = numpy.zeros(16, dtype=numpy.int64), numpy.zeros(4, dtype=numpy.float64)
        self._call("msg_get_cut_sets_info", _lib.ptr(out), _lib.ptr(vals))
        info = dict(zip(self.CUT_SETS_INFO_KEYS, out.tolist()), tol=None if tol is None else float(vals[0]), source_cut=float(vals[1]),
                    sink_cut=float(vals[2]), scale_max=float(vals[3]))
        info["tol_path"] = bool(info["tol_path"])
        return info

    def cut_sets(self, tol=None):
        """``CutSets(from_source, to_sink, ambiguous, info)`` of the cut ``maxflow()`` last returned: bool arrays of one entry per node
        and a dict.  ``from_source``: the nodes the source reaches in the residual graph of the maximum flow, the source side of the
        SMALLEST minimum cut (``labels()`` is that of the largest); ``to_sink``: the nodes that reach the sink; ``ambiguous``: neither --
        some minimum cut has them on the source side, another on the sink side.  ``tol`` None: an arc is open iff its residual is > 0
        (msg_cut_sets; ``to_sink`` is ``~labels()``); a number in [0, 1), e.g. ``ULP64``: iff it also exceeds ``tol`` times the largest
        capacity of an arc pair at either end (msg_cut_sets_tol): the nodes whose side does not hinge on the rounding of the solve.
        ``info``: the three counts, ``forward_passes`` / ``forward_seeds`` / ``backward_passes`` / ``backward_seeds`` of the floods,
        ``arcs_closed`` and ``tlinks_closed`` by the threshold, ``tol_path``, ``tol``, ``source_cut`` and ``sink_cut`` (the capacities of
        the cuts around ``from_source`` and ``~to_sink``, both equal to the flow up to rounding) and ``scale_max``.
        One library call per solve and ``tol``, cached until the next edge, t-link or solve.  MedpyHipError (ERR_STATE) before
        ``maxflow()`` and while the graph holds edges or t-links that ``maxflow()`` has not seen (nothing is sent from here)."""
        self._refuse_unsolved_edits("cut_sets")
        tol = None if tol is None else float(tol)
        cache = self.__dict__.setdefault("_cut_sets_cache", {})
        if ("sets", tol) not in cache:
            planes = [numpy.empty(self._nodes, dtype=numpy.uint8), None if tol is None else numpy.empty(self._nodes, dtype=numpy.uint8),
                      numpy.empty(self._nodes, dtype=numpy.uint8)]
            info = self._cut_sets_call(tol, planes)
            to_sink = ~self.labels() if tol is None else planes[1].view(numpy.bool_)
            cache[("sets", tol)] = CutSets(planes[0].view(numpy.bool_), to_sink, planes[2].view(numpy.bool_), info)
            cache[("info", tol)] = info
        return cache[("sets", tol)]

    def last_note(self):
        """what the library noted about the last call that went through: after ``cut_sets`` / ``cut_sets_unique`` the device time of
        the call by phase (``device_ms``, ``scale_ms``, ``open_ms``, ``forward_ms``, ``backward_ms``, ``readout_ms``)"""
        return (_lib.load().msg_last_error(self._h) or b"").decode()

    def cut_sets_unique(self, tol=None):
        """is the minimum cut unique, i.e. the ambiguity set empty (at ``tol``)?  Counted on the device: no array comes down."""
        self._refuse_unsolved_edits("cut_sets_unique")
        tol = None if tol is None else float(tol)
        cache = self.__dict__.setdefault("_cut_sets_cache", {})
        if ("info", tol) not in cache:
            cache[("info", tol)] = self._cut_sets_call(tol, [None, None, None])
        return cache[("info", tol)]["ambiguous"] == 0

    def changed_labels(self):
        """Edits by list exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: changed_labels is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver: read labels()")

    def markers(self):
        """Edits by list exist for the voxel lattices of 1-D..3-D volumes (VoxelGraph) only."""
        raise NotImplementedError("medpy_amd: markers is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                  "VoxelGraph) only; this graph went to the sparse-graph solver, which keeps merged t-links, not masks")

    def reset(self):
        """Graph::reset, reference graph.cpp:46-60 (wrapper.cpp:68): back to the state just after construction -- no nodes
        declared, no arcs, no t-links, flow 0."""
        self._raw = True
        self._open()

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().msg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        _lib.check_sparse(self._h, getattr(_lib.load(), name)(self._h, *args))

    @staticmethod
    def _image(image):
        image = numpy.ascontiguousarray(image)
        if image.dtype == numpy.bool_:
            image = image.astype(numpy.uint8)
        if image.dtype == numpy.float16:
            image = image.astype(numpy.float32)
        if image.dtype not in _lib.DTYPE_IDS:
            image = image.astype(numpy.float64)
        return image

    # -- inputs
    def _flush(self):
        i, j, cap, rev = self._pending
        if i:
            self._pending = ([], [], [], [])
            self._add_edges(i, j, cap, rev)

    def _add_edges(self, i, j, cap, rev):
        i = numpy.ascontiguousarray(i, dtype=numpy.int64)
        j = numpy.ascontiguousarray(j, dtype=numpy.int64)
        cap = numpy.ascontiguousarray(cap, dtype=numpy.float64)
        rev = numpy.ascontiguousarray(rev, dtype=numpy.float64)
        self._call("msg_add_edges", i.size, _lib.ptr(i), _lib.ptr(j), _lib.ptr(cap), _lib.ptr(rev))
        self._labels = None
        self._dev_solved = False

    def _add_lattice_edges(self, term, image, sigma, spacing):
        self._flush()
        image = self._image(image)
        shp = (C.c_int64 * image.ndim)(*image.shape)
        sp = (C.c_double * image.ndim)(*[float(v) for v in spacing]) if spacing else None
        self._call("msg_add_lattice_edges", _lib.TERM_IDS[term], image.ndim, shp, _lib.ptr(image), _lib.DTYPE_IDS[image.dtype],
                   float(sigma) if sigma is not None else 0.0, sp)
        self._labels = None
        self._dev_solved = False

    def _add_label_edges(self, term, label_image, image, param=0.0):
        self._flush()
        lab = numpy.ascontiguousarray(label_image, dtype=numpy.int64)
        image = self._image(numpy.asarray(image))
        if image.shape != lab.shape:
            raise ValueError("label image {} and image {} differ in shape".format(lab.shape, image.shape))
        shp = (C.c_int64 * lab.ndim)(*lab.shape)
        self._call("msg_add_label_edges", _lib.LABEL_TERM_IDS[term], lab.ndim, shp, _lib.ptr(lab), _lib.ptr(image),
                   _lib.DTYPE_IDS[image.dtype], float(param))
        self._labels = None
        self._dev_solved = False

    def _set_tweights_merged(self, tr, flow_const):
        self._tr = numpy.array(tr, dtype=numpy.float64)
        self._flow_const = float(flow_const)
        self._labels = None

    def set_param(self, name, value):
        self._call("msg_set_param", name.encode(), int(value))

    # -- raw GraphDouble calls (graph.h:388-480)
    def add_node(self, num=1):
        """Graph::add_node, reference graph.h:388-413: declares ``num`` more nodes, returns the id of the first.  Going beyond
        the constructor's node count grows the graph (the reference reallocates, graph.cpp:62-85): a larger graph is
        created in HBM and what was uploaded so far moves over."""
        first = self._declared
        self._raw = True
        self._declared += int(num)
        if self._declared > self._nodes:
            self._grow(self._declared)
        return first

    def _grow(self, nodes):
        self._flush()
        tail, head, cap = self.arcs()
        lib = _lib.load()
        old = self._h
        h = C.c_void_p()
        rc = lib.msg_create(int(nodes), self._device, C.byref(h))
        if rc != _lib.OK:
            msg = (lib.msg_last_error(h if h.value else None) or b"").decode()
            if h.value:
                lib.msg_destroy(h)
            raise _lib.MedpyHipError(rc, msg)
        self._h, self._nodes = h, int(nodes)
        self._sent_tr, self._sent_flow_const, self._dev_solved = None, None, False   # (a new handle: it was told nothing)
        lib.msg_destroy(old)
        if tail.size:
            self._add_edges(tail, head, cap, numpy.zeros(cap.size))
        if self._tr is not None:
            self._tr = numpy.concatenate([self._tr, numpy.zeros(self._nodes - self._tr.size)])
        self._labels = None

    def _queue(self, i, j, cap, rev_cap):
        p = self._pending
        p[0].append(i); p[1].append(j); p[2].append(float(cap)); p[3].append(float(rev_cap))
        self._labels = None
        if len(p[0]) >= 1 << 20:
            self._flush()

    def _check_ids(self, i, j):
        n = max(self._declared, self._nodes) if self._declared else self._nodes
        if not (0 <= i < n and 0 <= j < n) or i == j:   # the reference asserts (graph.h:430-432); here an exception
            raise ValueError("edge ({}, {}): node ids must differ and lie in [0, {})".format(i, j, n))

    def add_edge(self, i, j, cap, rev_cap):
        """Graph::add_edge, reference graph.h:428-454: a NEW pair of arcs i->j / j->i per call, prepended to both adjacency
        lists.  Parallel arcs carry the flow of one arc with the summed capacity (that is what goes to the device);
        ``get_edge`` afterwards sees the pair added LAST, as the reference's ``get_arc`` walk does (graph.h:500-509)."""
        i, j, cap, rev_cap = int(i), int(j), self._cast(cap), self._cast(rev_cap)
        self._check_ids(i, j)
        self._raw = True
        if self._captype != "double":
            for key, c in (((i, j), cap), ((j, i), rev_cap)):
                front = self._host_arcs.get(key)
                self._host_arcs[key] = [c, 0.0] if front is None else [c, front[1] + front[0]]
            self._labels = None
            return
        if (i, j) in self._raw_pairs or (j, i) in self._raw_pairs:
            self._first_arc[(i, j)], self._first_arc[(j, i)] = cap, rev_cap   # a parallel pair now hides the older ones
        self._raw_pairs.add((i, j))
        self._queue(i, j, cap, rev_cap)

    def sum_edge(self, i, j, cap, rev_cap):
        """Graph::sum_edge, reference graph.h:457-480: adds to the arc ``get_arc(i, j)`` finds (and to its sister), or
        creates the pair."""
        i, j, cap, rev_cap = int(i), int(j), self._cast(cap), self._cast(rev_cap)
        self._check_ids(i, j)
        if self._captype != "double":   # float32 / int arcs: the running sum is rounded per call, in the arc's type (host side)
            if (i, j) not in self._host_arcs:
                return self.add_edge(i, j, cap, rev_cap)
            a, r = self._host_arcs[(i, j)], self._host_arcs[(j, i)]
            a[0], r[0] = self._cast(a[0] + cap), self._cast(r[0] + rev_cap)
            self._labels = None
            return
        if (i, j) in self._first_arc:   # parallel pairs exist: the one in front takes the sum
            self._first_arc[(i, j)] = self._first_arc[(i, j)] + cap
            self._first_arc[(j, i)] = self._first_arc[(j, i)] + rev_cap
        self._raw_pairs.add((i, j))
        self._queue(i, j, cap, rev_cap)

    def add_tweights(self, i, cap_source, cap_sink):
        if self._tr is None:
            self._tr = numpy.zeros(self._nodes, dtype=numpy.float64)
        cs, ck = self._cast(cap_source), self._cast(cap_sink)
        delta = self._cast(self._tr[i])
        if delta > 0:
            cs = self._cast(cs + delta)
        else:
            ck = self._cast(ck - delta)
        self._flow_const = self._cast(self._flow_const + (cs if cs < ck else ck))
        self._tr[i] = self._cast(cs - ck)
        self._labels = None

    # -- GraphDouble surface
    def maxflow(self):
        """GraphDouble.maxflow(), reference maxflow.cpp:472-604.  Called again after ``add_tweights`` / ``update_tweights`` alone
        it goes on from the residual graph of the last solve, as the reference's does (graph.h:129-132, 211-276): only the
        t-links that differ from what the device was last told go down and the solve is warm (``warm_info()``).  Edges added,
        ``reset()`` or a grown graph in between make it a solve from scratch, as does ``set_param("warm", 0)``."""
        self._flush()
        self._send_host_arcs()
        if self._tr is not None:
            tr = numpy.ascontiguousarray(self._tr, dtype=numpy.float64)
            if not self._send_changed_tweights(tr):
                self._call("msg_set_tweights_merged", _lib.ptr(tr), float(self._flow_const))
            self._sent_tr, self._sent_flow_const = tr.copy(), float(self._flow_const)
        flow = C.c_double(0.0)
        self._dev_solved = self._dev_updated = False
        self._call("msg_maxflow", C.byref(flow))
        self._dev_solved = True
        self._labels = None
        return self._out(flow.value)

    def _send_changed_tweights(self, tr):
        """the entries of ``tr`` that differ from what the device holds, through msg_update_tweights; False where the whole
        vector has to go instead (no finished solve of these edges on the device, or values the list call refuses)"""
        if not self._dev_solved or self._sent_tr is None or self._sent_tr.size != tr.size:
            return False
        ids = numpy.flatnonzero(tr != self._sent_tr).astype(numpy.int64)
        if not ids.size and self._dev_updated and self._flow_const == self._sent_flow_const:
            return True   # update_tweights sent it all
        vals = numpy.ascontiguousarray(tr[ids])
        if not (numpy.isfinite(vals).all() and numpy.isfinite(self._flow_const)):
            return False
        self._call("msg_update_tweights", ids.size, _lib.ptr(ids), _lib.ptr(vals), float(self._flow_const))
        self._dev_updated = True
        return True

    # -- warm re-solves ("The sparse-graph solver")
    def update_tweights(self, nodes, tr, flow_const=None):
        """Replace the merged t-links of the DISTINCT node ids ``nodes`` by ``tr`` (positive: capacity from the source, negative:
        to the sink -- ``get_trcap``'s value) and keep the residual graph: on a graph that holds a finished cut the next
        ``maxflow()`` is a warm solve, and that cut's labels are kept on the device for ``changed_nodes()``.  The flow
        ``maxflow()`` reports is ``flow_const`` + the capacity of the minimum cut of the graph with the merged t-links;
        ``flow_const=None`` keeps the constant the graph has (what its ``add_tweights`` calls added up), any other value
        replaces it.  The library checks the list before it writes (MedpyHipError, ERR_INVALID: id out of range or twice,
        value not finite); a refused call changes nothing."""
        ids = numpy.asarray(nodes)
        if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
            raise ValueError("update_tweights: node ids must be a 1-D integer array")
        ids = numpy.ascontiguousarray(ids, dtype=numpy.int64)
        vals = numpy.array([self._cast(v) for v in numpy.asarray(tr).reshape(-1)], dtype=numpy.float64)
        if vals.size != ids.size:
            raise ValueError("update_tweights: %d node ids, %d t-links" % (ids.size, vals.size))
        fc = self._flow_const if flow_const is None else self._cast(flow_const)
        self._flush()
        self._send_host_arcs()
        if self._dev_solved and self._sent_tr is not None:
            self._call("msg_update_tweights", ids.size, _lib.ptr(ids), _lib.ptr(vals), float(fc))
            self._sent_tr[ids] = vals
            self._sent_flow_const = float(fc)
            self._dev_updated = True
        else:   # nothing to keep on the device: checked here the way the library does, sent whole by maxflow()
            if ids.size and (ids.min() < 0 or ids.max() >= self._nodes or numpy.unique(ids).size != ids.size or not numpy.isfinite(vals).all()):
                raise _lib.MedpyHipError(_lib.ERR_INVALID, "update_tweights: node id out of range or twice, or a t-link that is not finite")
        if self._tr is None:
            self._tr = numpy.zeros(self._nodes, dtype=numpy.float64)
        self._tr[ids] = vals
        self._flow_const = fc
        self._labels = None

    def changed_nodes(self):
        """After t-link updates (one or several) on a solved graph and the warm ``maxflow()`` that followed: ascending int64 array
        of the ids of the nodes whose label differs from the cut the graph held before the first of those updates.
        MedpyHipError (ERR_STATE) when the graph holds no such earlier cut (the last solve was cold) or is not solved."""
        n = C.c_int64(0)
        ids = numpy.empty(1024, dtype=numpy.int64)
        self._call("msg_labels_delta", ids.size, _lib.ptr(ids), C.byref(n))
        if n.value > ids.size:
            ids = numpy.empty(n.value, dtype=numpy.int64)
            self._call("msg_labels_delta", ids.size, _lib.ptr(ids), C.byref(n))
        return ids[:n.value].copy() if ids.size != n.value else ids

    def warm_info(self):
        """``skipped_build``: the last ``maxflow()`` went on from the resident residual graph; ``folded``: nodes whose t-link the
        last update changed there; ``snapshot``: labels of an earlier cut are held for ``changed_nodes()``; ``cold_builds``:
        residual graphs built from the edge list on this handle so far"""
        out = numpy.zeros(4, dtype=numpy.int64)
        self._call("msg_get_warm_info", _lib.ptr(out))
        return {"skipped_build": bool(out[0]), "folded": int(out[1]), "snapshot": bool(out[2]), "cold_builds": int(out[3])}

    def _send_host_arcs(self):
        """GraphFloat / GraphInt: the arcs accumulated on the host go to the device, parallel arcs summed (exactly: float32
        values and integers add without rounding in float64).  The reference's Graph<int> / Graph<float> take ``add_edge`` /
        ``sum_edge`` at any time (graph.h:428-480), also between two ``maxflow()`` calls: what goes down here is, per node pair,
        the DIFFERENCE between the pair's capacities now and what the device was last told -- exact in float64 for the same
        reason the sums are -- so edges added after a first solve are part of the next one."""
        if not self._host_arcs:
            return
        ii, jj, cc, rr = [], [], [], []
        for k, a in self._host_arcs.items():
            if k[0] >= k[1]:
                continue
            b = self._host_arcs[(k[1], k[0])]
            now = (float(a[0]) + float(a[1]), float(b[0]) + float(b[1]))
            was = self._host_sent.get(k, (0.0, 0.0))
            if now != was:
                ii.append(k[0]); jj.append(k[1]); cc.append(now[0] - was[0]); rr.append(now[1] - was[1])
                self._host_sent[k] = now
        if ii:
            self._add_edges(numpy.array(ii, dtype=numpy.int64), numpy.array(jj, dtype=numpy.int64),
                            numpy.array(cc, dtype=numpy.float64), numpy.array(rr, dtype=numpy.float64))

    def labels(self, out=None):
        """every node at once: bool array, False where what_segment == SINK.

        ``out``: a writeable C-contiguous bool or uint8 array of one entry per node that holds the labels of the previous cut
        (what ``changed_nodes()`` refers to).  Only the ids of the changed nodes are read from the device and ``out`` is
        flipped there and returned; where the graph keeps no previous cut all labels are read into ``out``.  Same meaning as
        ``VoxelGraph.labels(out=)``."""
        if out is not None:
            if not (isinstance(out, numpy.ndarray) and out.shape == (self._nodes,) and out.dtype in (numpy.bool_, numpy.uint8)
                    and out.flags.c_contiguous and out.flags.writeable):
                raise ValueError("labels(out=...): a writeable C-contiguous bool or uint8 array of shape (%d,)" % self._nodes)
            flat = out.view(numpy.uint8)
            try:
                ids = self.changed_nodes()
            except _lib.MedpyHipError as e:
                if e.code != _lib.ERR_STATE:
                    raise
                self._call("msg_labels", _lib.ptr(flat))   # (not solved: ERR_STATE again, from here)
                return out
            flat[ids] ^= 1
            return out
        if self._labels is None:
            out = numpy.empty(self._nodes, dtype=numpy.uint8)
            self._call("msg_labels", _lib.ptr(out))
            self._labels = out.astype(numpy.bool_)
        return self._labels

    def what_segment(self, i):
        seg = C.c_int(0)
        self._call("msg_what_segment", int(i), C.byref(seg))
        return termtype(seg.value)

    def get_edge(self, i, j):
        """Graph::get_edge, reference graph.h:482-498: the capacity of the first arc i->j of i's adjacency list (the pair
        added last when ``add_edge`` created parallel ones), 0 when there is none"""
        i, j = int(i), int(j)
        if self._captype != "double":
            a = self._host_arcs.get((i, j))
            return self._cast(0) if a is None else a[0]
        if (i, j) in self._first_arc:
            return self._first_arc[(i, j)]
        self._flush()
        out = C.c_double(0.0)
        self._call("msg_get_edge", i, j, C.byref(out))
        return self._out(out.value)

    def get_trcap(self, i):
        return self._cast(0) if self._tr is None else self._cast(self._tr[int(i)])

    def get_node_num(self):
        """nodes declared with ``add_node`` so far (graph.h:413), or the constructor's count when the facade filled the graph"""
        return self._declared if self._raw else self._nodes

    def get_arc_num(self):
        self._flush()
        self._send_host_arcs()
        n = C.c_int64(0)
        self._call("msg_get_counts", None, None, C.byref(n))
        return n.value

    def arcs(self):
        """every distinct arc as built: (tail, head, capacity) arrays sorted by (tail, head)"""
        n = self.get_arc_num()
        tail, head, cap = numpy.zeros(n, numpy.int32), numpy.zeros(n, numpy.int32), numpy.zeros(n, numpy.float64)
        if n:
            self._call("msg_get_arcs", _lib.ptr(tail), _lib.ptr(head), _lib.ptr(cap))
        return tail, head, cap

    def tweights(self):
        return numpy.zeros(self._nodes) if self._tr is None else numpy.array(self._tr)

    def stats(self):
        st = _lib.SparseStats()
        self._call("msg_get_stats", C.byref(st))
        return st.as_dict()


class GraphFloat(SparseGraph):
    """``maxflow.GraphFloat`` = ``Graph<float,float,float>`` (reference instances.inc:14, wrapper.cpp:27-57): capacities,
    t-links, their running sums and the returned flow are float32 values.  The solve itself runs in the library's float64
    arithmetic on those float32-valued capacities (sums of float32 numbers are exact in float64 far beyond any graph's
    size), so the cut is the exact minimum cut of the float32 graph; the reference's float32 augmentations can differ
    from it only where its own rounding decides a tie."""

    _captype = "float"

    @staticmethod
    def _cast(v):
        return float(numpy.float32(v))


class GraphInt(SparseGraph):
    """``maxflow.GraphInt`` = ``Graph<int,int,int>`` (reference instances.inc:12, wrapper.cpp:93-134): integer capacities
    and flow.  Whole numbers below 2**53 are exact in float64, so the device solve is exact integer arithmetic; like the
    Boost.Python binding, a capacity that is not an integer is a ``TypeError`` (there is no implicit float -> int
    conversion at that boundary)."""

    _captype = "int"

    @staticmethod
    def _cast(v):
        if isinstance(v, (bool, numpy.bool_)):
            return int(v)
        if isinstance(v, (int, numpy.integer)):
            return int(v)
        if isinstance(v, numpy.floating) and float(v).is_integer():
            return int(v)   # (the host copy of the t-links is a float64 array that holds whole numbers)
        raise TypeError("GraphInt: capacity %r is not an integer" % (v,))

    @staticmethod
    def _out(v):
        return int(round(v))


def merge_tweights_into(tr, flow_const, nodes, weights_source, weights_sink):
    """``Graph::add_tweights`` (graph.h:416-425), call by call in the order of the DISTINCT ids ``nodes``, on the merged t-links
    ``tr`` (written in place); returns the flow constant after the calls."""
    nodes = numpy.asarray(nodes, dtype=numpy.int64)
    if nodes.size == 0:
        return flow_const
    cs = numpy.array(weights_source, dtype=numpy.float64)
    ck = numpy.array(weights_sink, dtype=numpy.float64)
    delta = tr[nodes]
    cs = cs + numpy.where(delta > 0, delta, 0.0)
    ck = ck - numpy.where(delta > 0, 0.0, delta)
    tr[nodes] = cs - ck
    return float(numpy.cumsum(numpy.concatenate([[flow_const], numpy.minimum(cs, ck)]))[-1])  # in call order


def merge_region_markers(tr, flow_const, fg_nodes, bg_nodes, weight):
    """The hard constraints on top of the t-links the terms left (generate.py:169-172, 322-338; graph.py:334-380): the nodes
    ``fg_nodes`` get (weight, 0), then the nodes ``bg_nodes`` (0, weight), each list ascending and distinct, merged like any other
    t-link (a node in both ends up with weight on both sides).  ``tr`` (None: no t-links so far) is not written; returns
    ``(merged t-links, flow constant)``.  What ``GCGraph`` runs when it hands a graph to the sparse-graph solver, and what
    ``RegionGraph`` runs again on the t-links it kept from before the markers when the markers change."""
    fg_nodes, bg_nodes = numpy.asarray(fg_nodes, dtype=numpy.int64), numpy.asarray(bg_nodes, dtype=numpy.int64)
    out = numpy.array(tr, dtype=numpy.float64)
    flow_const = merge_tweights_into(out, flow_const, fg_nodes, numpy.full(fg_nodes.size, float(weight)), numpy.full(fg_nodes.size, 0.0))
    flow_const = merge_tweights_into(out, flow_const, bg_nodes, numpy.full(bg_nodes.size, 0.0), numpy.full(bg_nodes.size, float(weight)))
    return out, flow_const


class RegionGraph(SparseGraph):
    """What ``graph_from_labels`` returns: a ``SparseGraph`` whose nodes are the regions of a label image (node r - 1 = region r),
    which remembers how its t-links came about -- the merged t-links of the terms from before the markers, and the markers as
    voxel masks of the label image -- so that the markers can be edited and the cut solved again warm:
    ``update_markers`` by masks, ``edit_markers`` by voxel ids, ``markers()``, ``changed_labels()``.  A region is marked while
    at least one marked voxel lies in it."""

    def _set_regions(self, label_image, fg_mask, bg_mask, tr, flow_const):
        self._label_image = label_image   # by reference: never written
        self._lab_flat = numpy.asarray(label_image).reshape(-1)
        self._tr0 = numpy.zeros(self._nodes, dtype=numpy.float64) if tr is None else numpy.array(tr, dtype=numpy.float64)
        self._flow_const0 = float(flow_const)
        self._set_masks(fg_mask, bg_mask)

    def _set_masks(self, fg_mask, bg_mask):
        self._vox, self._cnt = [], []   # [fg, bg]: flat bool mask; marked voxels per region
        for mask in (fg_mask, bg_mask):
            vox = numpy.zeros(self._lab_flat.size, dtype=numpy.bool_) if mask is None else numpy.array(mask, dtype=numpy.bool_).reshape(-1)
            self._vox.append(vox)
            self._cnt.append(numpy.bincount(self._lab_flat[vox].astype(numpy.int64) - 1, minlength=self._nodes))

    def _remerge(self):
        self._tr, self._flow_const = merge_region_markers(self._tr0, self._flow_const0, numpy.flatnonzero(self._cnt[0]),
                                                          numpy.flatnonzero(self._cnt[1]), float(GCGraph.MAX))
        self._labels = None

    def update_markers(self, fg_markers, bg_markers):
        """Replace the markers (arrays of the label image's shape, non-zero = marked; None = no markers of that kind): the regions
        under them are wired to the terminals with ``GCGraph.MAX`` on top of the terms' t-links, foreground first, as
        ``graph_from_labels`` does.  The residual graph is kept; ``maxflow()`` sends the t-links that changed and solves warm."""
        shape = numpy.shape(self._label_image)
        for m, what in ((fg_markers, "foreground markers"), (bg_markers, "background markers")):
            if m is not None and numpy.shape(m) != shape:
                raise ValueError("%s of shape %s on a label image of shape %s" % (what, numpy.shape(m), shape))
        self._set_masks(fg_markers, bg_markers)
        self._remerge()

    def edit_markers(self, fg=None, bg=None, erase=None):
        """Edit the markers by lists of VOXELS of the label image (a stroke is drawn on the image, not on regions):
        ``fg' = (fg & ~erase) | fg_ids``, ``bg' = (bg & ~erase) | bg_ids``; the arguments take the forms ``merge_marker_edits``
        describes.  A region stays marked until its last marked voxel is erased.  Otherwise as ``update_markers``."""
        ids, ops = merge_marker_edits(numpy.shape(self._label_image), fg, bg, erase)
        for vox, cnt, set_bit, clear_bit in ((self._vox[0], self._cnt[0], 1, 4), (self._vox[1], self._cnt[1], 2, 8)):
            for sel, value in (((ops & set_bit) != 0, True), ((ops & clear_bit) != 0, False)):
                v = ids[sel]
                v = v[vox[v] != value]   # (ids are distinct: every voxel that changes counts once)
                vox[v] = value
                numpy.add.at(cnt, self._lab_flat[v].astype(numpy.int64) - 1, 1 if value else -1)
        self._remerge()

    def markers(self):
        """(fg, bg): the markers the graph holds now, bool arrays of the label image's shape"""
        shape = numpy.shape(self._label_image)
        return self._vox[0].reshape(shape).copy(), self._vox[1].reshape(shape).copy()

    def changed_labels(self):
        """``changed_nodes()``: the 0-based ids (node r - 1 = region r) of the regions whose label flipped"""
        return self.changed_nodes()


def region_sums(label_image, values, nregions, device=0):
    """per-region sums of ``values`` for labels 1..nregions, computed in HBM (``msg_region_sums``); float32 maps keep a
    float32 accumulator like numpy.sum does (reference energy_label.py:394-397).  Returns (sums, counts)."""
    lab = numpy.ascontiguousarray(label_image, dtype=numpy.int64)
    values = SparseGraph._image(numpy.asarray(values))
    if values.shape != lab.shape:
        raise ValueError("label image {} and map {} differ in shape".format(lab.shape, values.shape))
    sums = numpy.zeros(int(nregions), dtype=numpy.float64)
    counts = numpy.zeros(int(nregions), dtype=numpy.int64)
    rc = _lib.load().msg_region_sums(int(device), lab.size, _lib.ptr(lab), _lib.ptr(values), _lib.DTYPE_IDS[values.dtype],
                                     int(values.dtype == numpy.float32), int(nregions), _lib.ptr(sums), _lib.ptr(counts))
    _lib.check_sparse(None, rc)
    return sums, counts


class EmbeddedLatticeGraph(object):
    """`nodes` graph nodes of which the first prod(lattice_shape) form a voxel lattice (the boundary image had another
    shape than the markers, see GCGraph.record_boundary); the other nodes carry only their marker t-links.  Same surface
    as VoxelGraph; the lattice part is solved on the GPU, the isolated nodes are read out by the sign of their t-link
    exactly as BK would (tr_cap < 0: sink tree root -> SINK; otherwise SOURCE, graph.h:561-571)."""

    termtype = termtype

    def __init__(self, nodes, lattice_shape, boundary, fg, bg, device=0, connectivity=None):
        self._nodes = int(nodes)
        n = int(numpy.prod(lattice_shape))
        fg = numpy.zeros(self._nodes, numpy.uint8) if fg is None else numpy.asarray(fg, dtype=numpy.uint8).ravel()
        bg = numpy.zeros(self._nodes, numpy.uint8) if bg is None else numpy.asarray(bg, dtype=numpy.uint8).ravel()
        self._inner = VoxelGraph(lattice_shape, device=device, connectivity=connectivity)
        self._inner._set_boundary(*boundary)
        self._inner._set_markers(fg[:n].reshape(lattice_shape), bg[:n].reshape(lattice_shape))
        self._inner._build()
        tr = fg[n:].astype(numpy.float64) * GCGraph.MAX - bg[n:].astype(numpy.float64) * GCGraph.MAX
        self._tail_labels = ~(tr < 0)
        self._tail_tr = tr
        self._tail_flow = float(numpy.sum(numpy.minimum(fg[n:], bg[n:]).astype(numpy.float64)) * GCGraph.MAX)  # graph.h:423
        self._n = n

    def maxflow(self):
        return self._inner.maxflow() + self._tail_flow

    def labels(self):
        return numpy.concatenate([self._inner.labels().ravel(), self._tail_labels])

    def what_segment(self, i):
        i = int(i)
        if i < self._n:
            return self._inner.what_segment(i)
        return termtype.SOURCE if self._tail_labels[i - self._n] else termtype.SINK

    def get_node_num(self):
        return self._nodes

    def get_edge(self, i, j):
        return self._inner.get_edge(i, j) if (i < self._n and j < self._n) else 0.0

    def update_markers(self, fg_markers, bg_markers):
        raise NotImplementedError("medpy_amd: update_markers is not implemented for a graph whose boundary image has another shape "
                                  "than its markers (EmbeddedLatticeGraph): build it again with graph_from_voxels")

    def update_regional_term(self, probability_map, alpha):
        raise NotImplementedError("medpy_amd: update_regional_term is not implemented for a graph whose boundary image has another "
                                  "shape than its markers (EmbeddedLatticeGraph): build it again with graph_from_voxels")

    def update_boundary_term(self, boundary_term, boundary_term_args):
        raise NotImplementedError("medpy_amd: update_boundary_term is not implemented for a graph whose boundary image has another "
                                  "shape than its markers (EmbeddedLatticeGraph): build it again with graph_from_voxels")

    def edit_markers(self, fg=None, bg=None, erase=None):
        raise NotImplementedError("medpy_amd: edit_markers is not implemented for a graph whose boundary image has another shape "
                                  "than its markers (EmbeddedLatticeGraph): build it again with graph_from_voxels")

    def edit_nweights(self, nodes_from, nodes_to, weight_there, weight_back=None):
        raise NotImplementedError("medpy_amd: edit_nweights is not implemented for a graph whose boundary image has another shape "
                                  "than its markers (EmbeddedLatticeGraph): build it again with graph_from_voxels")

    def update_tweights_dense(self, weights_source, weights_sink):
        raise NotImplementedError("medpy_amd: update_tweights_dense is not implemented for a graph whose boundary image has another "
                                  "shape than its markers (EmbeddedLatticeGraph): build it again with graph_from_voxels")

    def edit_tweights(self, nodes, weights_source, weights_sink):
        raise NotImplementedError("medpy_amd: edit_tweights is not implemented for a graph whose boundary image has another shape "
                                  "than its markers (EmbeddedLatticeGraph): build it again with graph_from_voxels")

    def clear_nweight_edits(self):
        raise NotImplementedError("medpy_amd: clear_nweight_edits is not implemented for a graph whose boundary image has another "
                                  "shape than its markers (EmbeddedLatticeGraph): build it again with graph_from_voxels")

    def nweight_edit_info(self):
        raise NotImplementedError("medpy_amd: nweight_edit_info is not implemented for a graph whose boundary image has another "
                                  "shape than its markers (EmbeddedLatticeGraph)")

    def changed_labels(self):
        raise NotImplementedError("medpy_amd: changed_labels is not implemented for a graph whose boundary image has another shape "
                                  "than its markers (EmbeddedLatticeGraph): read labels()")

    def markers(self):
        raise NotImplementedError("medpy_amd: markers is not implemented for a graph whose boundary image has another shape "
                                  "than its markers (EmbeddedLatticeGraph)")

    def source_side(self, tol=None):
        """flat, as ``labels()``: the lattice part from the voxel graph; an isolated node is reached from the source iff its
        t-link points from the source (at every ``tol``: its link is the only number at the node)"""
        return numpy.concatenate([self._inner.source_side(tol).ravel(), self._tail_tr > 0])

    def sink_side(self, tol=None):
        """flat: an isolated node reaches the sink iff its t-link points to the sink"""
        return numpy.concatenate([self._inner.sink_side(tol).ravel(), self._tail_tr < 0])

    def ambiguous(self, tol=None):
        """flat, as ``labels()``: an isolated node is ambiguous iff it holds no t-link at all"""
        return numpy.concatenate([self._inner.ambiguous(tol).ravel(), self._tail_tr == 0])

    def cut_is_unique(self, tol=None):
        return self._inner.cut_is_unique(tol) and not bool(numpy.any(self._tail_tr == 0))

    def cut_sets_info(self, tol=None):
        """of the lattice part (mgc_get_cut_sets_info / mgc_get_cut_sets_tol_info); the cut capacities without the isolated nodes' share
        of the flow"""
        return self._inner.cut_sets_info(tol)

    def cut_sets(self, tol=None):
        """``CutSets(from_source, to_sink, ambiguous, info)`` of the four calls above; arrays flat, as ``labels()``"""
        return CutSets(self.source_side(tol), self.sink_side(tol), self.ambiguous(tol), self.cut_sets_info(tol))

    def cut_sets_unique(self, tol=None):
        return self.cut_is_unique(tol)

    def components(self, labels=None, foreground=True, connectivity=None, ids=True):
        """of the lattice part (``VoxelGraph.components``): arrays in the lattice's shape, ids of lattice voxels; the isolated nodes
        behind the lattice have no neighbours and are left out"""
        return self._inner.components(labels, foreground, connectivity, ids)

    def clean_labels(self, labels=None, min_size=1, largest=None, seeded=False, fill_holes=False, connectivity=None, hole_connectivity=None, out=None,
                     changed_only=False):
        """of the lattice part (``VoxelGraph.clean_labels``), in the lattice's shape"""
        return self._inner.clean_labels(labels, min_size, largest, seeded, fill_holes, connectivity, hole_connectivity, out, changed_only)

    def clean_info(self):
        return self._inner.clean_info()

    def distance_transform(self, labels=None, to="foreground", spacing=None, squared=False):
        """of the lattice part (``VoxelGraph.distance_transform``), in the lattice's shape"""
        return self._inner.distance_transform(labels, to, spacing, squared)

    def surface_distances(self, reference, labels=None, voxelspacing=None, connectivity=1):
        """of the lattice part (``VoxelGraph.surface_distances``)"""
        return self._inner.surface_distances(reference, labels, voxelspacing, connectivity)

    def overlap_counts(self, reference, labels=None):
        """of the lattice part (``VoxelGraph.overlap_counts``)"""
        return self._inner.overlap_counts(reference, labels)

    def geodesic_distance(self, seeds="fg", gamma=1.0, step=1.0, spacing=None, connectivity=None):
        """of the lattice part (``VoxelGraph.geodesic_distance``), in the lattice's shape"""
        return self._inner.geodesic_distance(seeds, gamma, step, spacing, connectivity)

    def geodesic_info(self):
        return self._inner.geodesic_info()

    def refit_regional_geodesic(self, gamma=None, lam=None):
        """of the lattice part (``VoxelGraph.refit_regional_geodesic``: ValueError, such a graph is built without the term)"""
        return self._inner.refit_regional_geodesic(gamma, lam)

    def anisotropic_diffusion(self, niter, kappa, gamma, voxelspacing=None, option=1, keep=False, download=True):
        """of the lattice part (``VoxelGraph.anisotropic_diffusion``), in the lattice's shape"""
        return self._inner.anisotropic_diffusion(niter, kappa, gamma, voxelspacing, option, keep, download)

    def diffusion_info(self):
        return self._inner.diffusion_info()

    def stats(self):
        return self._inner.stats()


class Graph(object):
    """Host-side description of a small graph-cut problem, the input format of ``graph_to_dimacs``.

    Same public surface as the reference's container (medpy/graphcut/graph.py:31-264; what write.py:29-76 reads):
    nodes are numbered 1..n, ``set_nweights`` takes ``{(a, b): (w_ab, w_ba)}``, ``add_tweights`` takes
    ``{node: (w_source, w_sink)}``, marker nodes get a terminal weight of ``MAX``.  Holds no device state."""

    MAX = 65535

    def __init__(self):
        self._count = 0
        self._markers = {"source": [], "sink": []}
        self._edges = {}      # (a, b) -> (w_ab, w_ba), insertion order = output order
        self._terminal = {}   # node -> (w_source, w_sink), insertion order = output order

    # ---- building ----
    def set_nodes(self, nodes):
        self._count = int(nodes)

    def _mark(self, side, nodes):
        self._markers[side] = list(nodes)
        weight = (self.MAX, 0) if side == "source" else (0, self.MAX)
        self._terminal.update(dict.fromkeys(self._markers[side], weight))

    def set_source_nodes(self, source_nodes):
        self._mark("source", source_nodes)

    def set_sink_nodes(self, sink_nodes):
        self._mark("sink", sink_nodes)

    def set_nweights(self, nweights):
        self._edges = nweights

    def add_tweights(self, tweights):
        self._terminal.update(tweights)

    # ---- reading ----
    def get_node_count(self):
        return self._count

    def get_nodes(self):
        return list(range(1, self._count + 1))

    def get_source_nodes(self):
        return self._markers["source"]

    def get_sink_nodes(self):
        return self._markers["sink"]

    def get_edges(self):
        return list(self._edges)

    def get_nweights(self):
        return self._edges

    def get_tweights(self):
        return self._terminal

    def inconsistent(self):
        """``False`` for a well-formed graph, otherwise one message per defect, in the reference's wording and order
        (reference graph.py:227-264): a node id above the node count in the t-weights, the markers or an edge, and every
        edge whose reverse is stored as an edge of its own (the weights of both directions belong into ONE entry)."""
        def unknown(node):
            return not node <= self._count

        messages = ["Node {} in t-weights but not in nodes.".format(n) for n in self._terminal if unknown(n)]
        messages += ["Node {} in s-nodes but not in nodes.".format(n) for n in self._markers["source"] if unknown(n)]
        messages += ["Node {} in t-nodes but not in nodes.".format(n) for n in self._markers["sink"] if unknown(n)]
        for edge in self._edges:
            messages += ["Node {} in edge {} but not in nodes.".format(n, edge) for n in edge if unknown(n)]
            if (edge[1], edge[0]) in self._edges:
                messages.append("The reversed edges of {} is also in the n-weights.".format(edge))
        return messages or False


class GCGraph(object):
    """Validating facade handed to the energy terms; reference graph.py:267-596.

    ``shape`` (not in the reference signature) tells the facade which voxel lattice the node
    ids refer to; ``graph_from_voxels`` supplies it.  Built-in energy terms record themselves
    (``record_boundary`` / ``record_regional``); foreign callables may still drive
    ``set_nweight`` / ``set_tweight*`` -- those calls are validated exactly like the reference
    does, accumulated, and uploaded in one batch.
    """

    __INT_16_BIT = 32767
    __UINT_16_BIT = 65535
    MAX = __UINT_16_BIT
    """The maximum value a terminal weight can take."""

    def __init__(self, nodes, edges, shape=None, device=0, connectivity=None):
        self.__connectivity = connectivity
        self.__nodes = int(nodes)
        self.__edges = int(edges)
        self.__general = shape is None or len(tuple(shape)) > 3  # not a 1-D..3-D voxel lattice: sparse-graph solver
        self.__label_terms = []
        self.__shape = tuple(shape) if shape is not None else (int(nodes),)
        if int(numpy.prod(self.__shape)) != self.__nodes:
            raise ValueError("shape {} does not hold {} nodes".format(self.__shape, nodes))
        self.__device = device
        self.__boundary = None
        self.__regional = None
        self.__fg = None
        self.__bg = None
        self.__edge_i, self.__edge_j, self.__edge_w, self.__edge_r = [], [], [], []
        self.__dense = []  # (offset, there, back or None): whole n-link weight arrays, in call order (set_nweights_dense)
        self.__tr = None  # merged explicit t-links (graph.h:416-425 applied call by call)
        self.__tdense = []  # (source, sink): whole t-link weight arrays, in call order (set_tweights_dense), while no per-node t-weight exists;
        #                     (_HistogramTerm, None): a histogram term (record_regional_histogram), fitted when the markers are known
        #                     (_GeodesicTerm, None): a geodesic term (record_regional_geodesic), fitted when the markers are known
        self.__markers_recorded = False
        self.__flow_const = 0.0
        self.__graph = None
        self.__lattice_shape = None  # set when the boundary image has another shape than the markers
        self.__region_image = None   # (label image, fg mask, bg mask) of graph_from_labels

    # -- fast path hooks used by medpy_amd.graphcut.energy_voxel
    def record_boundary(self, term, image, sigma, spacing):
        image = numpy.asarray(image)
        if image.shape != self.__shape:
            # The reference numbers the n-link endpoints by the IMAGE shape (energy_voxel.py:650-664), whatever the
            # marker shape is (its own tests do that: tests/graphcut_/energy_voxel.py:162-179, 4x4 markers, 3x3 image).
            # The edges then form a lattice of the image shape over node ids 0..image.size-1; the remaining nodes are
            # isolated.  Too many ids -> the same ValueError GCGraph.set_nweight raises (graph.py:418-425).
            if image.size > self.__nodes:
                raise ValueError("Invalid node id (node_to) of {}. Valid values are 0 to {}.".format(image.size - 1, self.__nodes - 1))
            if self.__regional is not None or self.__tr is not None or self.__tdense or self.__edge_i or self.__dense:
                raise NotImplementedError("medpy_amd: a boundary image of another shape cannot be combined with other terms")
            self.__lattice_shape = image.shape
        if self.__boundary is not None:
            raise NotImplementedError("medpy_amd: only one built-in boundary term per graph")
        self.__boundary = (term, image, sigma, spacing)

    def record_label_boundary(self, term, label_image, image, param=0.0):
        """fast path of the region terms (medpy_amd.graphcut.energy_label): the RAG edges are generated in HBM"""
        self.__general = True
        self.__label_terms.append((term, numpy.asarray(label_image), numpy.asarray(image), float(param)))

    def merge_tweights(self, nodes, weights_source, weights_sink):
        """vectorised ``set_tweight`` for DISTINCT node ids, Graph::add_tweights call by call (graph.h:416-425)"""
        nodes = numpy.asarray(nodes, dtype=numpy.int64)
        if nodes.size == 0:
            return
        if nodes.max() >= self.__nodes or nodes.min() < 0:
            raise ValueError("Invalid node id of {} or {}. Valid values are 0 to {}.".format(nodes.max(), nodes.min(), self.__nodes - 1))
        self.__merge_dense_tweights()
        if self.__tr is None:
            self.__tr = numpy.zeros(self.__nodes, dtype=numpy.float64)
        self.__flow_const = merge_tweights_into(self.__tr, self.__flow_const, nodes, weights_source, weights_sink)

    def record_regional(self, probability_map, alpha):
        pm = numpy.asarray(probability_map)
        if pm.size != self.__nodes:
            raise ValueError("probability map holds {} values for {} nodes".format(pm.size, self.__nodes))
        self.__regional = (pm.reshape(self.__shape), alpha)

    def record_regional_histogram(self, image, bins=None, lam=1.0, eps=0.5):
        """The histogram regional term (``energy_voxel.regional_histogram``; medpy_amd/graphcut/histogram.py is its definition):
        the intensities of ``image`` under the foreground and the background markers are counted in the bins of
        ``histogram_binning(image, bins)``, and voxel p gets ``set_tweight(p, source_table[bin(p)], sink_table[bin(p)])`` with the
        tables of ``histogram_tables(fg_hist, bg_hist, lam, eps)``.  The term is FITTED WHEN THE GRAPH IS BUILT, on the markers known
        then, and keeps its place in call order among the dense t-link calls.  On a graph of the tile solver whose explicit
        t-links are nothing but dense calls the histograms are counted and the tables expanded on the device
        (mgc_marker_histograms, mgc_add_tweights_binned), and ``VoxelGraph.refit_regional_histogram`` fits the term again after a
        stroke; every other graph evaluates the same term on the host and merges it like ``set_tweights_dense``.  ValueError for an
        image of another size, a value that is not finite, bad ``bins``, ``lam`` or ``eps``, before anything is recorded."""
        image = numpy.asarray(image)
        if image.size != self.__nodes:
            raise ValueError("histogram image holds {} values for {} nodes".format(image.size, self.__nodes))
        nbins, lo, width = histogram_binning(image, bins)
        histogram_tables(numpy.zeros(1), numpy.zeros(1), lam, eps)   # (lam and eps are checked here, before anything is recorded)
        if self.__graph is not None:
            raise NotImplementedError("medpy_amd: the graph is built already: VoxelGraph.refit_regional_histogram / update_tweights_binned change its t-links")
        self.__tdense.append((_HistogramTerm(image.reshape(self.__shape), nbins, lo, width, float(lam), float(eps)), None))

    def record_regional_geodesic(self, gamma, lam, step=1.0, spacing=None, connectivity=None, image=None):
        """The geodesic regional term (``energy_voxel.regional_geodesic``; medpy_amd/csrc/mgc_geo.h is its definition): with D_F and
        D_B the geodesic distances of a voxel to the foreground and to the background markers (``VoxelGraph.geodesic_distance``
        with ``gamma``, ``step``, ``spacing``, ``connectivity``) voxel p gets ``set_tweight(p, lam * D_B / (D_F + D_B),
        lam * D_F / (D_F + D_B))`` -- all of ``lam`` to the side that alone is reached, half each where both distances are 0,
        nothing where neither side is reached.  The term is FITTED WHEN THE GRAPH IS BUILT, on the markers known then, keeps its
        place in call order among the dense t-link calls, and is computed on the device (mgc_add_tweights_geodesic);
        ``VoxelGraph.refit_regional_geodesic`` fits it again after a stroke.  ``image`` (of the volume's size) becomes the feature
        image of the graph; None: the boundary term's image.  It exists on graphs of the tile solver whose explicit t-links are
        nothing but dense calls: NotImplementedError elsewhere, when the graph is built.  ValueError for a bad parameter or an
        image of another size, before anything is recorded."""
        for name, v in (("gamma", gamma), ("lam", lam), ("step", step)):
            VoxelGraph._geo_number("record_regional_geodesic", name, v)
        nd = len(self.__shape)
        if connectivity is not None and connectivity not in (1, nd):
            raise ValueError("record_regional_geodesic: connectivity must be 1 (face neighbours) or %d (the full neighbourhood), got %r" % (nd, connectivity))
        if spacing is not None:
            sp = numpy.asarray(spacing, dtype=numpy.float64)
            if sp.shape not in ((), (nd,)) or not (numpy.isfinite(sp).all() and (sp > 0).all()):
                raise ValueError("record_regional_geodesic: the spacing must be a finite positive scalar or %d such values, got %r" % (nd, spacing))
        if image is not None:
            image = numpy.asarray(image)
            if image.size != self.__nodes:
                raise ValueError("geodesic image holds {} values for {} nodes".format(image.size, self.__nodes))
            image = image.reshape(self.__shape)
        if self.__graph is not None:
            raise NotImplementedError("medpy_amd: the graph is built already: VoxelGraph.refit_regional_geodesic / update_tweights_geodesic change its t-links")
        self.__tdense.append((_GeodesicTerm(float(gamma), float(lam), float(step), spacing, connectivity, image), None))

    def __histogram_arrays(self, term):
        """the two per-voxel arrays of a histogram term, evaluated on the host on the markers known now"""
        fg_hist, bg_hist, bins = _histogram.marker_histograms(term.image, self.__fg, self.__bg, term.nbins, term.lo, term.width)
        source_table, sink_table = histogram_tables(fg_hist, bg_hist, term.lam, term.eps)
        return source_table[bins], sink_table[bins]

    # -- reference API
    def record_markers(self, fg_mask, bg_mask):
        """fast path of ``graph_from_voxels``: the marker MASKS (bool arrays of the volume's shape) instead of id lists --
        what ``set_source_nodes(flatnonzero(fg))`` / ``set_sink_nodes(flatnonzero(bg))`` would leave, without the lists"""
        self.__markers_recorded = True
        for mask, side in ((fg_mask, "fg"), (bg_mask, "bg")):
            mask = numpy.ascontiguousarray(mask, dtype=numpy.bool_)
            if mask.size != self.__nodes:
                raise ValueError("marker mask of {} voxels on a graph of {} nodes".format(mask.size, self.__nodes))
            if not mask.any():
                continue
            flat = mask.reshape(-1).view(numpy.uint8)
            have = self.__fg if side == "fg" else self.__bg
            if have is not None:   # ids were wired before (a plug-in called set_*_nodes): repeated ids accumulate, the explicit path keeps that
                (self.set_source_nodes if side == "fg" else self.set_sink_nodes)(numpy.flatnonzero(flat))
            elif side == "fg":
                self.__fg = flat
            else:
                self.__bg = flat

    def set_source_nodes(self, source_nodes):
        source_nodes = numpy.asarray(source_nodes)
        if source_nodes.size == 0:
            raise ValueError("max() arg is an empty sequence")  # the reference's max([]) (graph.py:334)
        if source_nodes.max() >= self.__nodes or source_nodes.min() < 0:
            raise ValueError("Invalid node id of {} or {}. Valid values are 0 to {}.".format(
                source_nodes.max(), source_nodes.min(), self.__nodes - 1))
        if self.__fg is None:
            self.__fg = numpy.zeros(self.__nodes, dtype=numpy.uint8)
        elif not self.__fg.flags.owndata:
            self.__fg = self.__fg.copy()   # (a view of the caller's mask, record_markers: never written through)
        if numpy.unique(source_nodes).size != source_nodes.size or self.__fg[source_nodes].any():
            for s in source_nodes:  # repeated ids accumulate in the reference; keep that via the explicit path
                self.set_tweight(int(s), self.MAX, 0)
            return
        self.__fg[source_nodes] = 1

    def set_sink_nodes(self, sink_nodes):
        sink_nodes = numpy.asarray(sink_nodes)
        if sink_nodes.size == 0:
            raise ValueError("max() arg is an empty sequence")
        if sink_nodes.max() >= self.__nodes or sink_nodes.min() < 0:
            raise ValueError("Invalid node id of {} or {}. Valid values are 0 to {}.".format(
                sink_nodes.max(), sink_nodes.min(), self.__nodes - 1))
        if self.__bg is None:
            self.__bg = numpy.zeros(self.__nodes, dtype=numpy.uint8)
        elif not self.__bg.flags.owndata:
            self.__bg = self.__bg.copy()
        if numpy.unique(sink_nodes).size != sink_nodes.size or self.__bg[sink_nodes].any():
            for s in sink_nodes:
                self.set_tweight(int(s), 0, self.MAX)
            return
        self.__bg[sink_nodes] = 1

    def set_nweight(self, node_from, node_to, weight_there, weight_back):
        if node_from >= self.__nodes or node_from < 0:
            raise ValueError("Invalid node id (node_from) of {}. Valid values are 0 to {}.".format(node_from, self.__nodes - 1))
        elif node_to >= self.__nodes or node_to < 0:
            raise ValueError("Invalid node id (node_to) of {}. Valid values are 0 to {}.".format(node_to, self.__nodes - 1))
        elif node_from == node_to:
            raise ValueError("The node_from ({}) can not be equal to the node_to ({}) (self-connections are forbidden in graph cuts).".format(node_from, node_to))
        elif weight_there <= 0 or weight_back <= 0:
            raise ValueError("Negative or zero weights are not allowed.")
        self.__edge_i.append(int(node_from))
        self.__edge_j.append(int(node_to))
        self.__edge_w.append(float(weight_there))
        self.__edge_r.append(float(weight_back))

    def set_nweights_dense(self, offset_or_axis, weight_there, weight_back=None):
        """Whole n-link weight arrays at once: the call a plug-in boundary term makes instead of one ``set_nweight`` per edge
        (extension; the reference has no bulk form).  ``offset_or_axis``: a lattice offset (one component in {-1, 0, 1} per array
        axis, a neighbour in the connectivity of the graph) or an ``int``, the forward unit offset of that axis.
        ``weight_there[p]`` is added to the arc p -> p + offset, ``weight_back[p]`` (None: symmetric) to the arc p + offset -> p,
        with the semantics of ``set_nweight`` / ``sum_edge``: repeated calls accumulate in call order.  Arrays have the shape of
        the volume (entries whose neighbour lies outside are ignored) or, for the forward offset of an axis, the layout of the
        reference's ``__skeleton_base`` (extent - 1 along that axis), which costs a padding copy on the host
        (``pad_skeleton_weights``).  Weights must be finite and >= 0 -- zero is allowed here, for one-way arcs -- which the
        library checks on the device when the graph is built (``MedpyHipError``).  The arrays reach the graph after the built-in
        boundary term and before the edges of ``set_nweight``.  ValueError for a bad offset, shape or dtype, before anything is
        recorded; NotImplementedError on graphs the sparse-graph solver takes (no lattice shape, more than 3 axes, a boundary
        image of another shape, an explicit edge between voxels that are not neighbours)."""
        if self.__general or self.__lattice_shape is not None:
            raise NotImplementedError("medpy_amd: dense n-link weight arrays need a 1-D..3-D voxel lattice on the tile solver")
        off = _dense_offset(offset_or_axis, len(self.__shape), self.__connectivity)
        there = _dense_array(self.__shape, off, weight_there, "weight_there")
        back = None if weight_back is None else _dense_array(self.__shape, off, weight_back, "weight_back")
        if back is not None and numpy.shape(weight_back) != numpy.shape(weight_there):
            raise ValueError("weight_there of shape %s and weight_back of shape %s" % (numpy.shape(weight_there), numpy.shape(weight_back)))
        if self.__graph is not None:
            raise NotImplementedError("medpy_amd: the graph is built already (warm updates of the dense weights are not implemented)")
        self.__dense.append((off, there, back))

    def set_nweights(self, nweights):
        for edge, weight in list(nweights.items()):
            self.set_nweight(edge[0], edge[1], weight[0], weight[1])

    def set_tweight(self, node, weight_source, weight_sink):
        if node >= self.__nodes or node < 0:
            raise ValueError("Invalid node id of {}. Valid values are 0 to {}.".format(node, self.__nodes - 1))
        self.__merge_dense_tweights()
        if self.__tr is None:
            self.__tr = numpy.zeros(self.__nodes, dtype=numpy.float64)
        # Graph::add_tweights, graph.h:416-425, call by call
        cs, ck = float(weight_source), float(weight_sink)
        delta = self.__tr[node]
        if delta > 0:
            cs += delta
        else:
            ck -= delta
        self.__flow_const += cs if cs < ck else ck
        self.__tr[node] = cs - ck

    def set_tweights_dense(self, weights_source, weights_sink):
        """Whole t-link weight arrays at once: the call a plug-in regional term makes instead of one ``set_tweight`` per voxel
        (extension; the reference has no bulk form).  Voxel p gets ``set_tweight(p, weights_source[p], weights_sink[p])``, with
        the semantics of ``Graph::add_tweights``: repeated calls accumulate in call order, negative weights are allowed.  Arrays
        of the volume's shape or flat arrays of one entry per node; float32 / float64 are used as they are (float32 is widened,
        which is exact), anything else -- and two arrays of different dtypes -- as float64.  On a graph of the tile solver whose
        explicit t-links are nothing but such calls the arrays go to the device as they are (mgc_add_tweights) and are checked
        there when the graph is built: every entry must be finite (``MedpyHipError``).  Call order against ``set_tweight`` is
        kept: a call made when per-node t-weights exist is merged into them at once, and the first ``set_tweight`` after such
        calls merges them first -- as are the calls of graphs that go to the sparse-graph solver.  ValueError for a wrong shape
        or dtype, before anything is recorded."""
        source, sink = _dense_tweight_arrays(self.__shape, weights_source, weights_sink)
        if self.__graph is not None:
            raise NotImplementedError("medpy_amd: the graph is built already: VoxelGraph.update_tweights_dense / edit_tweights change its t-links")
        if self.__tr is not None and not self.__tdense:   # per-node t-weights exist: this call comes after them
            self.merge_tweights(numpy.arange(self.__nodes), source.ravel(), sink.ravel())
        else:   # (behind a histogram term that waits for the markers the call waits too: call order)
            self.__tdense.append((source, sink))

    def __merge_dense_tweights(self):
        """the recorded dense calls, merged on the host in call order (a per-node t-weight follows, or the graph goes to a solver
        that takes one merged vector); a histogram term among them is fitted to the markers known now"""
        if any(isinstance(source, _GeodesicTerm) for source, _ in self.__tdense):
            raise NotImplementedError("medpy_amd: the geodesic regional term is implemented for the voxel lattice solver (1-D..3-D volumes, "
                                      "VoxelGraph) on graphs whose explicit t-links are nothing but dense calls: its distances are computed on the device")
        if any(sink is None for _, sink in self.__tdense) and self.__fg is None and self.__bg is None and not self.__markers_recorded:
            raise NotImplementedError("medpy_amd: a per-node t-weight behind a histogram regional term, before the markers are known: "
                                      "the term is fitted to the markers; set the markers first")
        calls, self.__tdense = self.__tdense, []
        for source, sink in calls:
            if sink is None:
                source, sink = self.__histogram_arrays(source)
            self.merge_tweights(numpy.arange(self.__nodes), source.ravel(), sink.ravel())

    def set_tweights(self, tweights):
        for node, weight in list(tweights.items()):
            self.set_tweight(node, weight[0], weight[1])

    def set_tweights_all(self, tweights):
        for node, (twsource, twsink) in enumerate(tweights):
            self.set_tweight(node, twsource, twsink)

    def __edges_join_lattice_neighbours(self):
        """do all explicit edges join neighbours of the voxel lattice (of the neighbourhood in use)?  The tile solver keeps
        exactly those arcs; anything else (the reference accepts arbitrary node pairs, graph.py:382-440) goes to the
        sparse-graph solver."""
        shape = self.__shape if self.__lattice_shape is None else self.__lattice_shape
        if shape is None or not self.__edge_i:
            return True
        i = numpy.asarray(self.__edge_i, dtype=numpy.int64)
        j = numpy.asarray(self.__edge_j, dtype=numpy.int64)
        n = int(numpy.prod(shape))
        if i.max() >= n or j.max() >= n:
            return False
        ci = numpy.stack(numpy.unravel_index(i, shape))
        cj = numpy.stack(numpy.unravel_index(j, shape))
        d = numpy.abs(ci - cj)
        full = self.__connectivity not in (None, 2 * len(shape))
        ok = (d.max(axis=0) == 1) if full else (d.sum(axis=0) == 1)
        return bool(ok.all())

    def get_graph(self):
        """Builds the residual lattice in HBM (once) and returns the solver object."""
        if self.__graph is None and not self.__general and self.__edge_i and len(self.__shape or ()) <= 3 \
                and not self.__edges_join_lattice_neighbours():
            self.__general = True  # a plug-in term added an edge between voxels that are not neighbours
        if self.__graph is None and self.__dense and (self.__general or self.__lattice_shape is not None):
            raise NotImplementedError("medpy_amd: dense n-link weight arrays on a graph that goes to the sparse-graph solver")
        if self.__graph is None and self.__tdense and (self.__general or self.__lattice_shape is not None or self.__tr is not None):
            self.__merge_dense_tweights()   # (these solvers take one merged vector; so does a graph that holds per-node t-weights)
        if self.__graph is None and self.__general:
            self.__graph = self.__sparse_graph()
        if self.__graph is None and self.__lattice_shape is not None:
            self.__graph = EmbeddedLatticeGraph(self.__nodes, self.__lattice_shape, self.__boundary, self.__fg, self.__bg,
                                                device=self.__device, connectivity=self.__connectivity)
        if self.__graph is None:
            g = VoxelGraph(self.__shape, device=self.__device, connectivity=self.__connectivity)
            if self.__boundary is not None:
                g._set_boundary(*self.__boundary)
            if self.__regional is not None:
                g._set_regional(*self.__regional)
            if self.__tr is not None:
                g._set_tweights_merged(self.__tr, self.__flow_const)
            fitted = any(sink is None for _, sink in self.__tdense)   # a histogram term: the markers go up before it is fitted to them
            if fitted and (self.__fg is not None or self.__bg is not None):
                g._set_markers(None if self.__fg is None else self.__fg, None if self.__bg is None else self.__bg)
            feature = None   # the feature image resident on the handle (None: the calls read the boundary term's)
            for source, sink in self.__tdense:   # (nothing but dense calls: __tr is None)
                if sink is not None:
                    g._add_tweights(source, sink)
                    continue
                term = source   # counted and expanded on the device, in its place in call order
                if isinstance(term, _GeodesicTerm):
                    if term.image is not None and not (self.__boundary is not None and _same_array(term.image, self.__boundary[1])):
                        if feature is None or not _same_array(term.image, feature):
                            g._set_feature_image(term.image)
                            feature = term.image
                    elif feature is not None:
                        g._set_feature_image(None)
                        feature = None
                    g._add_tweights_geodesic(term.gamma, term.lam, term.step, term.spacing, term.connectivity)
                    g._geo_params = (term.gamma, term.lam, term.step, term.spacing, term.connectivity)
                    continue
                own = self.__boundary is not None and _same_array(term.image, self.__boundary[1])
                if not own and (feature is None or not _same_array(term.image, feature)):
                    g._set_feature_image(term.image)
                    feature = term.image
                elif own and feature is not None:
                    g._set_feature_image(None)
                    feature = None
                fg_hist, bg_hist = g.marker_histograms(term.nbins, term.lo, term.width)
                source_table, sink_table = histogram_tables(fg_hist, bg_hist, term.lam, term.eps)
                g._add_tweights_binned(source_table, sink_table, term.nbins, term.lo, term.width)
                g._binning, g._hist_params = (term.nbins, term.lo, term.width), (term.lam, term.eps)
            if not fitted and (self.__fg is not None or self.__bg is not None):
                g._set_markers(None if self.__fg is None else self.__fg, None if self.__bg is None else self.__bg)
            for off, there, back in self.__dense:   # (after the boundary term, before the explicit edges: the order mgc_build applies them in)
                g._add_nweights(off, there, back)
            if self.__edge_i:
                g._add_edges(self.__edge_i, self.__edge_j, self.__edge_w, self.__edge_r)
            g._build()
            self.__graph = g
        return self.__graph

    def __sparse_graph(self):
        """the same calls in the same order (regional term, boundary term, explicit edges, markers last:
        generate.py:159-172, 322-338) on the sparse-graph solver"""
        if self.__connectivity not in (None, 2 * len(self.__shape)):
            raise NotImplementedError("medpy_amd: the full neighbourhood exists for 1-D..3-D voxel lattices only")
        g = (SparseGraph if self.__region_image is None else RegionGraph)(self.__nodes, self.__edges, device=self.__device)
        if self.__regional is not None:  # energy_voxel.py:61-65 in the map's dtype, then graph.py:551-552
            pm, alpha = self.__regional
            pm = numpy.asarray(pm)
            if pm.dtype not in (numpy.float32, numpy.float64):
                pm = pm.astype(numpy.float64)
            self.merge_tweights(numpy.arange(self.__nodes), (pm * alpha).ravel().astype(numpy.float64),
                                ((1 - pm) * alpha).ravel().astype(numpy.float64))
            self.__regional = None
        if self.__boundary is not None:
            g._add_lattice_edges(*self.__boundary)
        for term, lab, img, param in self.__label_terms:
            g._add_label_edges(term, lab, img, param)
        if self.__edge_i:
            g._add_edges(self.__edge_i, self.__edge_j, self.__edge_w, self.__edge_r)
        if self.__region_image is not None:   # the t-links as they stand before the markers: what a marker edit merges onto again
            g._set_regions(*self.__region_image, tr=self.__tr, flow_const=self.__flow_const)
        fg_nodes, bg_nodes = (numpy.empty(0, dtype=numpy.int64) if m is None else numpy.flatnonzero(numpy.asarray(m).ravel())
                              for m in (self.__fg, self.__bg))
        if self.__tr is not None or fg_nodes.size or bg_nodes.size:
            self.__tr, self.__flow_const = merge_region_markers(numpy.zeros(self.__nodes) if self.__tr is None else self.__tr,
                                                                self.__flow_const, fg_nodes, bg_nodes, self.MAX)
        self.__fg = self.__bg = None
        if self.__tr is not None:
            g._set_tweights_merged(self.__tr, self.__flow_const)
        return g

    def record_region_markers(self, label_image, fg_mask, bg_mask):
        """``graph_from_labels``: the label image whose regions are the nodes, and the marker masks on it.  The graph built is
        then a ``RegionGraph``, whose markers can be edited (the nodes under the markers still come through
        ``set_source_nodes`` / ``set_sink_nodes``)."""
        self.__region_image = (label_image, fg_mask, bg_mask)

    def get_shape(self):
        """the lattice shape the node ids refer to (``(nodes,)`` for a graph without one)"""
        return self.__shape

    def get_node_count(self):
        return self.__nodes

    def get_nodes(self):
        return list(range(0, self.__nodes))

    def get_edge_count(self):
        return self.__edges


class _BoundaryRecorder(GCGraph):
    """What ``VoxelGraph.update_boundary_term`` hands to an ``energy_voxel`` boundary function in place of the facade: it notes the
    one built-in term the function records (``recorded`` = (term, image, sigma, spacing), the image as given, None allowed) and
    refuses everything else a boundary function could do to a graph."""

    def __init__(self, shape):
        shape = tuple(int(s) for s in shape)
        GCGraph.__init__(self, int(numpy.prod(shape)), 0, shape=shape)
        self.recorded = None

    def record_boundary(self, term, image, sigma, spacing):
        if self.recorded is not None:
            raise NotImplementedError("medpy_amd: only one built-in boundary term per graph")
        self.recorded = (term, image, sigma, spacing)

    def set_nweights_dense(self, offset_or_axis, weight_there, weight_back=None):
        raise NotImplementedError("medpy_amd: update_boundary_term takes the built-in boundary terms; weights the caller evaluated "
                                  "(boundary_precomputed, set_nweights_dense) are part of a cold build: graph_from_voxels")

    def set_nweight(self, node_from, node_to, weight_there, weight_back):
        raise NotImplementedError("medpy_amd: update_boundary_term takes the built-in boundary terms, not edges set one by one")

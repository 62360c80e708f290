"""Overlap and surface measures of two binary objects, with the names, argument order and defaults of ``medpy.metric.binary``,
computed on the device: the four overlap counts by mgc_overlap_counts, the surface distances by mgc_surface_distances
(borders, exact Euclidean distance transform, gathering), the last step -- a ratio, a maximum, a mean, a percentile -- on the host in
NumPy, as the reference takes it.

Every function takes one more keyword, ``graph``: a ``VoxelGraph`` (or ``EmbeddedLatticeGraph``) of the volume's shape whose handle
the call uses -- with ``result=None`` the first object is the graph's current cut, read where it lies on the device, so scoring the
cut just made is ``hd(None, truth, graph=g)``.  Without it a handle of the shape is created for the call and closed again.

Zero is background, everything else object.  1-D to 3-D volumes; more dimensions raise NotImplementedError.
"""
import numpy

__all__ = ["dc", "jc", "precision", "recall", "sensitivity", "specificity", "true_negative_rate", "true_positive_rate", "positive_predictive_value", "ravd", "hd",
           "hd95", "asd", "assd"]

_EMPTY_FIRST = "The first supplied array does not contain any binary object."
_EMPTY_SECOND = "The second supplied array does not contain any binary object."


def _binary(name, a, shape=None):
    a = numpy.atleast_1d(numpy.asarray(a).astype(numpy.bool_))
    if a.ndim > 3:
        raise NotImplementedError("medpy_amd.metric.binary: %d-D volumes are not implemented (1-D..3-D are)" % a.ndim)
    if shape is not None and a.shape != shape:
        raise ValueError("medpy_amd.metric.binary: %s has shape %s, expected %s" % (name, a.shape, shape))
    return numpy.ascontiguousarray(a)


class _Handle(object):
    """the graph of a call: the caller's, or one of the shape that lives as long as the call"""

    def __init__(self, graph, shape):
        self.own = graph is None
        if self.own:
            from ..graphcut.graph import VoxelGraph
            graph = VoxelGraph(shape)
        self.graph = getattr(graph, "_inner", graph)   # (an EmbeddedLatticeGraph scores its lattice part)

    def __enter__(self):
        return self.graph

    def __exit__(self, *exc):
        if self.own:
            self.graph.close()
        return False


def _objects(result, reference, graph):
    """(result plane or None: the graph's cut, reference plane, shape)"""
    if result is None and graph is None:
        raise ValueError("medpy_amd.metric.binary: result=None stands for the current cut of graph=..., and no graph was given")
    shape = tuple(graph._inner._shape if hasattr(graph, "_inner") else graph._shape) if graph is not None else None
    reference = _binary("reference", reference, shape)
    result = None if result is None else _binary("result", result, reference.shape)
    return result, reference, reference.shape


def _spacing(voxelspacing, ndim):
    """the reference's rule: a scalar counts for every axis, a sequence must have one value per axis (RuntimeError otherwise)"""
    if voxelspacing is None:
        return None
    sp = numpy.asarray(voxelspacing, dtype=numpy.float64)
    if sp.ndim == 0:
        sp = numpy.full(ndim, float(sp))
    if sp.shape != (ndim,):
        raise RuntimeError("sequence argument must have length equal to input rank")
    if not (numpy.isfinite(sp).all() and (sp > 0).all()):
        raise ValueError("medpy_amd.metric.binary: the voxel spacing must be finite and positive, got %r" % (voxelspacing,))
    return sp


def _counts(result, reference, graph):
    result, reference, shape = _objects(result, reference, graph)
    with _Handle(graph, shape) as g:
        return g.overlap_counts(reference, result)


def _ratio(num, den, otherwise):
    """num / float(den), and what the reference answers where that divides by zero"""
    try:
        return num / float(den)
    except ZeroDivisionError:
        return otherwise


def _from_counts(name, tp, fp, fn, tn):
    """the count-based measures from (tp, fp, fn, tn), in the reference's own arithmetic"""
    if name == "dc":
        return _ratio(2.0 * tp, (tp + fp) + (tp + fn), 1.0)
    if name == "jc":
        return _ratio(float(tp), tp + fp + fn, 1.0)
    if name in ("precision", "positive_predictive_value"):
        return _ratio(tp, tp + fp, 0.0)
    if name in ("recall", "sensitivity", "true_positive_rate"):
        return _ratio(tp, tp + fn, 0.0)
    if name in ("specificity", "true_negative_rate"):
        return _ratio(tn, tn + fp, 0.0)
    if name == "ravd":
        if tp + fn == 0:
            raise RuntimeError(_EMPTY_SECOND)
        return ((tp + fp) - (tp + fn)) / float(tp + fn)
    raise KeyError(name)


def _count_metric(name, doc):
    def f(result, reference, graph=None):
        return _from_counts(name, *_counts(result, reference, graph))
    f.__name__ = f.__qualname__ = name
    f.__doc__ = doc + "  ``graph``: see the module."
    return f


dc = _count_metric("dc", "Dice coefficient 2 |A & B| / (|A| + |B|); 1.0 when both objects are empty.")
jc = _count_metric("jc", "Jaccard coefficient |A & B| / |A | B|; 1.0 when both objects are empty.")
precision = _count_metric("precision", "tp / (tp + fp); 0.0 when the result is empty.")
recall = _count_metric("recall", "tp / (tp + fn); 0.0 when the reference is empty.")
sensitivity = _count_metric("sensitivity", "``recall``.")
specificity = _count_metric("specificity", "tn / (tn + fp); 0.0 when the reference covers the volume.")
true_negative_rate = _count_metric("true_negative_rate", "``specificity``.")
true_positive_rate = _count_metric("true_positive_rate", "``recall``.")
positive_predictive_value = _count_metric("positive_predictive_value", "``precision``.")
ravd = _count_metric("ravd", "Relative absolute volume difference (|A| - |B|) / |B|, signed as the reference's; RuntimeError when the reference is empty.")


def _surface_lists(result, reference, voxelspacing, connectivity, graph, both):
    """the surface distances result -> reference and, if ``both``, reference -> result"""
    result, reference, shape = _objects(result, reference, graph)
    sp = _spacing(voxelspacing, len(shape))
    with _Handle(graph, shape) as g:
        first = g.surface_distances(reference, result, sp, connectivity)
        if not both:
            return first, None
        if result is None:   # the other way round needs the cut as a plane of the host's: read into an array of this call, nothing the graph caches is touched
            from .. import _lib
            result = numpy.empty(shape, dtype=numpy.uint8)
            g._call("mgc_labels", _lib.ptr(result))
        try:
            second = g.surface_distances(result, reference, sp, connectivity)
        except RuntimeError as e:   # (cannot happen after the first call went through; the messages name the caller's order)
            raise RuntimeError(_EMPTY_SECOND if str(e) == _EMPTY_FIRST else _EMPTY_FIRST)
        return first, second


def hd(result, reference, voxelspacing=None, connectivity=1, graph=None):
    """Hausdorff distance: the largest of the surface distances, both ways round."""
    s1, s2 = _surface_lists(result, reference, voxelspacing, connectivity, graph, True)
    return max(s1.max(), s2.max())


def hd95(result, reference, voxelspacing=None, connectivity=1, graph=None):
    """95th percentile of the surface distances, both ways round."""
    s1, s2 = _surface_lists(result, reference, voxelspacing, connectivity, graph, True)
    return numpy.percentile(numpy.hstack((s1, s2)), 95)


def assd(result, reference, voxelspacing=None, connectivity=1, graph=None):
    """Average symmetric surface distance: the mean of the surface distances, both ways round."""
    s1, s2 = _surface_lists(result, reference, voxelspacing, connectivity, graph, True)
    return numpy.concatenate([s1, s2]).mean()


def asd(result, reference, voxelspacing=None, connectivity=1, graph=None):
    """Average surface distance from the result to the reference (not symmetric)."""
    return _surface_lists(result, reference, voxelspacing, connectivity, graph, False)[0].mean()

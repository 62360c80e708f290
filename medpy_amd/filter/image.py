"""The seeded watershed and the local minima its markers are made from, computed on the device (the definition is
medpy_amd/csrc/mgc_ws.h): what ``medpy_watershed.py`` does between an image and the region image ``graph_from_labels`` takes.

``local_minima`` has the name, the signature and the return pair of ``medpy.filter.image.local_minima``.  ``watershed`` stands
where the reference script calls ``skimage.segmentation.watershed(image, markers, mask=mask)``: face neighbourhood, labels grown
from the markers over the image read as heights.  Where no two values are equal it is Meyer's priority flood; on plateaus the
regions meet where the step counts from the plateau's rim meet, which is a definition of this project's and not skimage's order.
1-D to 3-D images; more dimensions raise NotImplementedError.
"""
import ctypes as C

import numpy

__all__ = ["watershed", "local_minima", "minima_markers", "watershed_info"]

_INFO_KEYS = ("seeds", "rounds", "tile_visits", "sweeps", "capped_visits", "reached", "jump_rounds")
_last_info = dict.fromkeys(_INFO_KEYS, 0)


def orderable(image):
    """The image as the device takes it: C-contiguous, bool as uint8, float16 as float32, and the dtypes of up to 32 bits as they
    are.  64-bit integers and float64 are RANKED (``numpy.unique(..., return_inverse=True)``) and sent as uint32: only the order
    of the values matters, so the result is the same.  ValueError for values that are not finite and beyond 2**32 distinct values."""
    image = numpy.ascontiguousarray(image)
    if image.dtype == numpy.bool_:
        return image.view(numpy.uint8)
    if image.dtype == numpy.float16:
        image = image.astype(numpy.float32)
    if image.dtype.kind not in "uif":
        raise ValueError("medpy_amd.filter: images of dtype %s are not supported" % image.dtype)
    if image.dtype.kind == "f" and not numpy.isfinite(image).all():
        raise ValueError("medpy_amd.filter: the image must be finite")
    if image.dtype.itemsize <= 4:
        return image
    values, inverse = numpy.unique(image, return_inverse=True)   # (-0.0 and 0.0 are equal, and so one rank)
    if values.size > 2 ** 32:
        raise ValueError("medpy_amd.filter: %d distinct values are more than 32-bit ranks hold" % values.size)
    return numpy.ascontiguousarray(inverse.reshape(image.shape), dtype=numpy.uint32)


def _volume(what, image):
    image = numpy.asarray(image)
    if image.ndim < 1 or image.ndim > 3:
        raise NotImplementedError("medpy_amd.filter.%s: %d-D images are not implemented (1-D..3-D are)" % (what, image.ndim))
    if image.size == 0:
        raise ValueError("%s: the image is empty" % what)
    return orderable(image)


def watershed(image, markers, mask=None, device=0):
    """int32 labels of the image's shape: every voxel inside ``mask`` that a marker reaches carries the label of the marker whose
    flood arrives first, 0 elsewhere.  ``markers``: integers, 0 = none, > 0 = a label (up to 2**31 - 1); ``mask``: not zero =
    inside, None = everywhere; a marker outside the mask is no marker.  Face neighbourhood.  ``watershed_info()`` has the counts of
    the device's work."""
    from .. import _lib
    what = "watershed"
    img = _volume(what, image)
    mk = numpy.asarray(markers)
    if mk.shape != img.shape:
        raise ValueError("%s: the markers have shape %s, the image %s" % (what, mk.shape, img.shape))
    if mk.dtype == numpy.bool_:
        mk = mk.astype(numpy.int32)
    if mk.dtype.kind not in "ui":
        raise ValueError("%s: the markers must be of an integer type, got %s" % (what, mk.dtype))
    if mk.size and mk.min() < 0:
        raise ValueError("%s: negative markers" % what)
    if mk.size and mk.max() > 2 ** 31 - 1:
        raise ValueError("%s: markers beyond int32" % what)
    mk = numpy.ascontiguousarray(mk, dtype=numpy.int32)
    m8 = None
    if mask is not None:
        m = numpy.asarray(mask)
        if m.shape != img.shape:
            raise ValueError("%s: the mask has shape %s, the image %s" % (what, m.shape, img.shape))
        m8 = numpy.ascontiguousarray(m != 0).view(numpy.uint8)
    out = numpy.empty(img.shape, dtype=numpy.int32)
    out8 = numpy.zeros(8, dtype=numpy.int64)
    shp = (C.c_int64 * img.ndim)(*img.shape)
    rc = _lib.load().mgc_watershed_image(int(device), img.ndim, shp, _lib.ptr(img), _lib.DTYPE_IDS[img.dtype], _lib.ptr(mk), None if m8 is None else _lib.ptr(m8), _lib.ptr(out),
                                         _lib.ptr(out8))
    _lib.check(None, rc)
    _last_info.update(zip(_INFO_KEYS, out8.tolist()))
    return out


def watershed_info():
    """of the last ``watershed``: seed voxels, rounds, tile visits, sweeps, visits that ended at the sweep cap, reached voxels,
    pointer-jumping rounds"""
    return dict(_last_info)


def _min_distance(what, min_distance):
    try:
        size = int(min_distance)
        ok = size == min_distance and size >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: min_distance must be an integer of at least 1, got %r" % (what, min_distance))
    return size


def minima_mask(img, min_distance=4, device=0):
    """bool array: ``img == scipy.ndimage.minimum_filter(img, size=min_distance)`` (border ``reflect``), on the device"""
    from .. import _lib
    what = "local_minima"
    size = _min_distance(what, min_distance)
    image = _volume(what, img)
    out = numpy.empty(image.shape, dtype=numpy.uint8)
    shp = (C.c_int64 * image.ndim)(*image.shape)
    rc = _lib.load().mgc_local_minima_image(int(device), image.ndim, shp, _lib.ptr(image), _lib.DTYPE_IDS[image.dtype], size, _lib.ptr(out), None)
    _lib.check(None, rc)
    return out.view(numpy.bool_)


def local_minima(img, min_distance=4, device=0):
    """``(indices, values)`` of all local minima of the image, sorted by value: ``medpy.filter.image.local_minima``.  A voxel is a
    minimum where it equals the minimum of the window of ``min_distance`` voxels around it.  The mask is computed on the device;
    ``nonzero``, the values and the sort run on the host.  The sort is STABLE (equal values stay in C order of their indices); the
    reference's ``argsort()`` is not, so against it the values are equal and, per value, the SETS of indices."""
    fits = numpy.asarray(img)
    mask = minima_mask(fits, min_distance, device)
    good_indices = numpy.transpose(mask.nonzero())
    good_fits = fits[mask]
    order = numpy.argsort(good_fits, kind="stable")
    return good_indices[order], good_fits[order]


def minima_markers(img, min_distance=2, mask=None, device=0):
    """int32 markers for ``watershed``, as ``medpy_watershed.py`` makes them: the local minima, those outside ``mask`` dropped,
    touching ones (face neighbourhood) joined and numbered 1..K in the order of ``scipy.ndimage.label``.  The minima and the
    numbering (``VoxelGraph.components``) run on the device."""
    from ..graphcut.graph import VoxelGraph
    plane = minima_mask(img, min_distance, device)
    if mask is not None:
        m = numpy.asarray(mask)
        if m.shape != plane.shape:
            raise ValueError("minima_markers: the mask has shape %s, the image %s" % (m.shape, plane.shape))
        plane = plane & (m != 0)
    g = VoxelGraph(plane.shape, device=device)
    try:
        return g.components(numpy.ascontiguousarray(plane), connectivity="face").ids
    finally:
        g.close()
